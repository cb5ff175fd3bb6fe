"""Geometry buffers of a camera sequence on the GPU (grt_gbuffer_trace_sequence,
grt_gbuffer_shade_sequence; marker `gpu`).

K cameras over one resident scene are traced stacked, as grt_render_sequence traces them, and
every frame is kept as an ordinary g-buffer; K buffers are shaded in one launch.  The
reference of every comparison is the existing per-frame path -- grt_gbuffer_trace on a scene
created with that camera, grt_gbuffer_shade of one buffer, grt_render_pixels -- and every
comparison is exact (bytes of the arrays and of the info, f32 / f64 bits, class, status):
the operations are the same, so no tolerance is involved.

The frames are the sequence tests': 24 cols x 20 rows x 3 cameras, so 8x8 tiles straddle two
frames, and the cameras differ in position and in all three angles.
"""
import ctypes as C
import errno
import math
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import RESOURCES, SCENES
from test_gpu_gbuffer import _grt, assert_same_frame, built_scene, reshade_pair
from test_gpu_sequence import (CAMS_FRONT, CAMS_WINDING, COLS, GRT, K, N, ROWS, Built, _native, _winding,
                               assert_frames_equal, b_checker, make_case, reference)

pytestmark = pytest.mark.gpu

ARRAYS = ("status", "stop", "steps", "sky_u", "sky_v", "sky_redshift", "layer_start", "object", "u", "v", "redshift",
          "radius")


def _rc(exc):
    return int(str(exc.value).split("(")[1].split(")")[0])


def assert_same_buffer(got, want, what=""):
    """Two g-buffers byte for byte: the twelve arrays and the info."""
    a, b = got.arrays(), want.arrays()
    assert set(a) == set(b) == set(ARRAYS)
    for key in ARRAYS:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (what, key)
    assert bytes(got.info) == bytes(want.info), (what, "info")


_SINGLE, _STACKED = {}, {}


def single_buffers(grt, name):
    """The reference: each camera's scene traced alone (grt_gbuffer_trace), once per case."""
    if name not in _SINGLE:
        case = reference(grt, name)[0] if name in _MAKE_CASE else _CASES[name](grt)
        _SINGLE[name] = (case, [case.scene(k).trace_gbuffer() for k in range(K)])
    return _SINGLE[name]


def stacked_buffers(grt, name):
    """(scene with camera 0, cameras, the sequence's buffers), once per case, default group."""
    if name not in _STACKED:
        case = single_buffers(grt, name)[0]
        sc, cams = case.scene(0), case.cameras()
        _STACKED[name] = (sc, cams, sc.trace_gbuffer_sequence(cams))
    return _STACKED[name]


def shade_as_results(shaded, k):
    """Frame k of shade_sequence in the shape assert_same_frame compares."""
    return SimpleNamespace(xyza=shaded["xyza"][k], xyza64=shaded["xyza64"][k], ray_class=shaded["class"][k],
                           status=shaded["status"][k])


# ---- cases beside make_case's -----------------------------------------------------------
_MAKE_CASE = ("schwarzschild", "kerr-bl", "kerr-schild", "euclidean", "winding")

# test_gpu_gbuffer.reshade_pair's frames under three cameras: camera 0 is the pair's own, so
# frame 0 is the frame whose blend that file's tests count
PAIR_CAMS = {
    "schwarzschild": [((-14.0, 0.0, 1.2), 0.0, -3.142, 0.0), ((-13.5, 1.5, 1.6), 0.04, -3.1, 0.03),
                      ((-13.0, -2.0, 0.8), -0.05, -3.2, -0.04)],
    "kerr-bl": [((-10.0, 0.0, -0.5), 0.0, -3.14159, 0.0), ((-9.5, 1.0, -0.8), 0.05, -3.1, 0.02),
                ((-9.0, -1.5, 0.4), -0.06, -3.2, -0.05)],
}


class Pair:
    """reshade_pair(name) under the cameras of PAIR_CAMS: appearance A (alt=False) or B."""

    def __init__(self, grt, name, alt=False):
        self.grt, self.name, self.alt, self.cams = grt, name, alt, PAIR_CAMS[name]

    def desc(self, k):
        grt = self.grt
        d = reshade_pair(grt, self.name)[1 if self.alt else 0]
        cart, phi, theta, psi = self.cams[k]
        pos = _native(grt, d.geometry, d.a, cart)
        d.camera = grt.build_camera(d.geometry, d.radius, d.a, pos, grt.stationary_velocity(d.geometry, d.radius, d.a, pos),
                                    math.pi / 4, ROWS, COLS, phi, theta, psi)
        return d

    def scene(self, k):
        return built_scene(self.grt, self.desc(k))

    def cameras(self):
        return [self.desc(k).camera for k in range(len(self.cams))]


# the winding scene with a Kerr-LUT disc down to r = 0.54 (tests/test_hit_pool.py): the disc
# inside r_isco raises BelowRISCO / NoCircularOrbitPossible in the frames that look at the
# hole (cameras 0 and 2) and in no pixel of camera 1, which looks past it
CAMS_ERRORS = [CAMS_WINDING[0], ((-7.8, -0.8, 0.05), 0.0, -1.5, 0.0), CAMS_WINDING[1]]


def _winding_disc(b):
    _winding(b)
    b.add_disc(0.54, 3.0, b_checker(0.0, 10.0, 10.0, (255, 255, 0), (80, 80, 0)), temperature=4000.0)


def errors_case(grt):
    L = grt._lib
    return Built(grt, L.GEOM_KERR_BL, 1.0, 0.499, 1e-6, (200000, 100.0, 0.01, 1e-7), _winding_disc, CAMS_ERRORS,
                 alpha=0.21)


_CASES = {"errors": errors_case, "pair-schwarzschild": lambda g: Pair(g, "schwarzschild"),
          "pair-kerr-bl": lambda g: Pair(g, "kerr-bl")}


# ------------------------------------------------- 1. the single-frame buffers ------
@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl", "kerr-schild", "euclidean"])
def test_buffers_are_the_single_frame_buffers(grt, gpu, name):
    L = grt._lib
    case, singles = single_buffers(grt, name)
    sc, cams, seq = stacked_buffers(grt, name)
    assert len(seq) == K
    for k in range(K):
        assert_same_buffer(seq[k], singles[k], (name, k))
        info = seq[k].info
        assert (info.row0, info.col0, info.rows, info.cols, info.device) == (0, 0, ROWS, COLS, 0)
        assert bytes(info.camera) == bytes(cams[k]) and int(info.n_pixels) == N
    for key in ("accepted_steps", "attempts", "rays"):
        assert seq.stats[key] == sum(s.stats[key] for s in singles), key
    assert seq.stats["rays"] == K * N and seq.stats["hit_overflows"] == 0
    rep = seq.report
    assert (rep.n_frames, rep.n_launches, rep.frames_per_launch, rep.n_traces) == (K, 1, K, 1)
    assert rep.trace_ms > 0 and rep.fill_ms > 0 and rep.wall_ms >= rep.trace_ms
    assert abs(seq.stats["kernel_ms"] - rep.trace_ms) < 1e-9
    # a buffer reports its launch group's times
    assert all(b.trace_times == seq[0].trace_times for b in seq) and seq[0].trace_times["trace_ms"] > 0
    # three different frames with something in them
    arrays = [b.arrays() for b in seq]
    for i, j in ((0, 1), (1, 2), (0, 2)):
        assert arrays[i]["steps"].tobytes() != arrays[j]["steps"].tobytes()
        assert arrays[i]["sky_u"].tobytes() != arrays[j]["sky_u"].tobytes()
        assert bytes(seq[i].info) != bytes(seq[j].info)
    assert any(int(b.info.n_layers) > 0 for b in seq)
    assert any(np.any((a["stop"] == L.STOP_CELESTIAL) & (a["status"] == 0)) for a in arrays)


# ------------------------------------------------- 2. the stacked shade ------------
@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl", "kerr-schild", "euclidean"])
def test_stacked_shade_equals_the_frames(grt, gpu, name):
    case, refs = reference(grt, name)  # render_pixels of each camera's scene
    sc, cams, seq = stacked_buffers(grt, name)
    shaded = grt.shade_sequence(seq, sc)
    assert shaded["xyza"].shape == (K, N, 4) and shaded["steps"].shape == (K, N)
    assert_frames_equal(shaded, refs, name)  # f32, f64, class, status, and the recorded stop and steps
    for k in range(K):
        assert_same_frame(shade_as_results(shaded, k), seq[k].shade(sc), (name, k))
    assert shaded["stats"]["kernel_ms"] > 0
    # only the fields asked for
    some = grt.shade_sequence(seq, sc, fields=("xyza64", "status"))
    assert set(some) == {"xyza64", "status", "stats"}
    assert np.array_equal(some["xyza64"].view(np.uint64), shaded["xyza64"].view(np.uint64))
    assert np.array_equal(some["status"], shaded["status"])


@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl"])
def test_stacked_shade_under_another_appearance(grt, gpu, name):
    """reshade_pair's B: other textures, alpha, beaming, temperatures and hit threshold."""
    a_case, singles = single_buffers(grt, "pair-" + name)
    sa, cams, seq = stacked_buffers(grt, "pair-" + name)
    b_case = Pair(grt, name, alt=True)
    sb = b_case.scene(0)
    for k in range(K):
        assert_same_buffer(seq[k], singles[k], (name, k))
    layers = np.concatenate([np.diff(b.arrays()["layer_start"].astype(np.int64)) for b in seq])
    assert (layers >= 2).sum() >= 30, (layers >= 2).sum()  # the frames exercise the blend
    shaded = {"A": grt.shade_sequence(seq, sa), "B": grt.shade_sequence(seq, sb)}
    for which, case, app in (("A", a_case, sa), ("B", b_case, sb)):
        for k in range(K):
            want = case.scene(k).render_pixels(0, 0, ROWS, COLS)
            got = shade_as_results(shaded[which], k)
            assert_same_frame(got, want, (name, which, k))
            assert_same_frame(got, seq[k].shade(app), (name, which, k, "single shade"))
            assert np.array_equal(shaded[which]["stop"][k], want.stop_reason)
            assert np.array_equal(shaded[which]["steps"][k], want.steps)
    assert not np.array_equal(shaded["A"]["xyza64"], shaded["B"]["xyza64"])
    assert np.any(shaded["A"]["class"] != shaded["B"]["class"])
    blended = (layers >= 2) & (shaded["B"]["xyza64"].reshape(-1, 4)[:, 3] > 0)
    assert blended.sum() >= 30


# ------------------------------------------------- 3. launch groups ----------------
def test_launch_groups_give_identical_buffers(grt, gpu):
    case, singles = single_buffers(grt, "schwarzschild")
    sc, cams, _ = stacked_buffers(grt, "schwarzschild")
    refs = reference(grt, "schwarzschild")[1]
    try:
        for frames, launches in ((1, 3), (2, 2), (3, 1)):
            grt.set_sequence_group(frames * N)
            seq = sc.trace_gbuffer_sequence(cams)
            rep = seq.report
            assert (rep.n_launches, rep.frames_per_launch, rep.n_traces) == (launches, frames, launches)
            for k in range(K):  # 2 + 1: the last frame's layer_start is rebased in its own group
                assert_same_buffer(seq[k], singles[k], (frames, k))
            for key in ("accepted_steps", "attempts", "rays"):
                assert seq.stats[key] == sum(s.stats[key] for s in singles), (frames, key)
            shaded = grt.shade_sequence(seq, sc)
            assert_frames_equal(shaded, refs, frames)
            # buffers of different groups report their own group's times
            assert (seq[0].trace_times == seq[2].trace_times) == (launches == 1)
        grt.set_sequence_group(1)  # below one frame: a group still holds one
        assert sc.trace_gbuffer_sequence(cams).report.n_launches == 3
    finally:
        grt.set_sequence_group(0)


# ------------------------------------------------- 4. past the slots, the re-trace --
def test_layers_past_the_workspace_slots_and_the_retrace(grt, gpu):
    L = grt._lib
    case, singles = single_buffers(grt, "winding")
    sc, cams, seq = stacked_buffers(grt, "winding")
    layers = np.concatenate([np.diff(b.arrays()["layer_start"].astype(np.int64)) for b in seq])
    assert layers.max() > L.GRT_MAX_HITS and (layers > L.GRT_MAX_HITS).sum() > 30, layers.max()
    for k in range(K):
        assert_same_buffer(seq[k], singles[k], ("winding", k))
    assert seq.report.n_traces == seq.report.n_launches == 1
    refs = reference(grt, "winding")[1]
    assert_frames_equal(grt.shade_sequence(seq, sc), refs, "winding")
    L.check(L.lib().grt_set_hit_pool_min(64))
    try:
        small = case.scene(0)  # a fresh device copy: a 64-record pool
        again = small.trace_gbuffer_sequence(cams)
        assert again.report.n_traces > again.report.n_launches == 1
        assert again.stats["rays"] > K * N and again.stats["rays"] % (K * N) == 0  # whole groups again
        for k in range(K):
            assert_same_buffer(again[k], singles[k], ("winding, small pool", k))
            assert not np.any(again[k].arrays()["status"] & L.FLAG_HIT_OVERFLOW)
        assert_frames_equal(grt.shade_sequence(again, small), refs, "winding, small pool")
    finally:
        L.check(L.lib().grt_set_hit_pool_min(1 << 20))


# ------------------------------------------------- 5. window-error pixels ----------
def test_window_error_pixels(grt, oracle, gpu):
    L = grt._lib
    case, singles = single_buffers(grt, "errors")
    # the inputs, on the CPU: BelowRISCO / NoCircularOrbitPossible in some frames, not in all
    cpu = [oracle.render_pixels(case.desc(k), 0, 0, ROWS, COLS, threads=16)["status"] for k in range(K)]
    with_errors = [bool(np.isin(s, (2, 3)).any()) for s in cpu]
    assert any(with_errors) and not all(with_errors), with_errors
    assert {2, 3} <= set(np.unique(np.concatenate(cpu)))
    sc, cams, seq = stacked_buffers(grt, "errors")
    for k in range(K):
        a, b = seq[k].arrays(), singles[k].arrays()
        assert np.array_equal(a["status"], b["status"]), k
        assert bool(np.isin(a["status"], (2, 3)).any()) == with_errors[k], k
        counts = np.diff(a["layer_start"].astype(np.int64))
        assert np.array_equal(counts, np.diff(b["layer_start"].astype(np.int64))), k
        failed = a["status"] != 0
        assert not np.any(counts[failed])  # an aborted pixel has no layers
        for key in ("sky_u", "sky_v", "sky_redshift"):
            assert a[key].tobytes() == b[key].tobytes(), (k, key)
            assert not np.any(a[key][failed].view(np.uint64)), (k, key)  # +0.0, bit for bit
        assert_same_buffer(seq[k], singles[k], ("errors", k))
    shaded = grt.shade_sequence(seq, sc)
    for k in range(K):
        want = case.scene(k).render_pixels(0, 0, ROWS, COLS)
        assert_same_frame(shade_as_results(shaded, k), want, ("errors", k))
        assert np.array_equal(want.status, seq[k].arrays()["status"])


# ------------------------------------------------- 6. ordinary buffers -------------
def test_the_buffers_are_ordinary(grt, gpu, tmp_path):
    case, refs = reference(grt, "schwarzschild")
    sc, cams, seq = stacked_buffers(grt, "schwarzschild")
    # the file
    seq[1].save(tmp_path / "f1.grtg")
    single_buffers(grt, "schwarzschild")[1][1].save(tmp_path / "s1.grtg")
    assert (tmp_path / "f1.grtg").read_bytes() == (tmp_path / "s1.grtg").read_bytes()
    loaded = grt.GBuffer.load(tmp_path / "f1.grtg", device=0)
    assert_same_frame(loaded.shade(sc), refs[1], "save -> load -> shade")
    assert bytes(loaded.info) == bytes(seq[1].info)
    up = grt.GBuffer.from_arrays(seq[1].info, seq[1].arrays(), device=0)
    assert_frames_equal(grt.shade_sequence([seq[0], up, loaded], sc), [refs[0], refs[1], refs[1]], "uploaded")
    # the adaptive re-shade of one frame, per frame: the buffer's own camera as the tracer
    ad = grt.default_adaptive()
    assert ad.enabled == 1
    want = sc.render_sequence(cams, adaptive=ad, supersample=True)
    mine = sc.trace_gbuffer_sequence(cams)[1]  # a buffer of its own: the call appends a sub-sample set
    got, report = mine.shade_section(sc, adaptive=ad, tracer=case.scene(1))
    assert got.n_supersampled == int(want["n_supersampled"][1]) >= 1
    assert report["n_traced"] == got.n_supersampled
    assert np.array_equal(got.xyza64.view(np.uint64), want["xyza64"][1].view(np.uint64))
    assert np.array_equal(got.ray_class, want["class"][1]) and np.array_equal(got.status, want["status"][1])
    assert not np.array_equal(got.xyza64, refs[1].xyza64)  # the supersampled pixels differ from 1 spp
    # the sub-rays belong to the frame the buffer holds: another frame's camera is refused
    with pytest.raises(grt.GrtError, match="camera") as e:
        seq[1].supersample(case.scene(0), [0, 1, 2], ad.samples_per_axis)
    assert _rc(e) == -errno.EINVAL
    assert seq[1].sub_info.samples_per_axis == 0


# ------------------------------------------------- 7. refusals ---------------------
def test_refusals(grt, gpu):
    L = grt._lib
    lib = L.lib()
    case, refs = reference(grt, "schwarzschild")
    sc, cams, seq = stacked_buffers(grt, "schwarzschild")
    table = (L.CameraDesc * K)(*cams)

    def trace(scene, n, tab):
        out = (C.c_void_p * K)(*([0xdead] * K))
        rc = lib.grt_gbuffer_trace_sequence(scene._s, 0, n, tab, out, None, None)
        return rc, [out[k] for k in range(n)]

    for rows, cols in ((ROWS + 1, COLS), (ROWS, COLS - 8)):
        bad = (L.CameraDesc * K)(*cams)
        bad[1].rows, bad[1].cols = rows, cols
        rc, handles = trace(sc, K, bad)
        assert rc == -errno.EINVAL and "camera 1" in lib.grt_last_error().decode()
        assert handles == [None] * K
    rc, _ = trace(sc, 0, table)
    assert rc == -errno.EINVAL and "at least one camera" in lib.grt_last_error().decode()
    with pytest.raises(grt.GrtError) as e:
        sc.trace_gbuffer_sequence([])
    assert _rc(e) == -errno.EINVAL
    vol = make_case(grt, "volumetric")
    rc, handles = trace(vol.scene(0), K, (L.CameraDesc * K)(*vol.cameras()))
    assert rc == -errno.ENOTSUP and handles == [None] * K
    # the stacked shade
    with pytest.raises(grt.GrtError, match="at least one buffer") as e:
        grt.shade_sequence([], sc)
    assert _rc(e) == -errno.EINVAL
    small = sc.trace_gbuffer(0, 0, ROWS - 4, COLS)  # an ordinary buffer of another rectangle size
    with pytest.raises(grt.GrtError, match="frame 2") as e:
        grt.shade_sequence([seq[0], seq[1], small], sc)
    assert _rc(e) == -errno.EINVAL and "pixels" in str(e.value)
    other = stacked_buffers(grt, "euclidean")[2][0]  # another geometry: the shape key differs
    with pytest.raises(grt.GrtError, match="frame 1") as e:
        grt.shade_sequence([seq[0], other, seq[2]], sc)
    assert _rc(e) == -errno.EINVAL and "geometry" in str(e.value)
    with pytest.raises(grt.GrtError, match="xyza") as e:
        grt.shade_sequence(seq, sc, fields=("status",))  # no colour field
    assert _rc(e) == -errno.EINVAL
    # nothing was left behind: the same calls still give the frames
    assert_frames_equal(grt.shade_sequence(seq, sc), refs, "after the refusals")


# ------------------------------------------------- 8. the fused knob ---------------
def test_sequence_buffers_are_exact_under_the_fused_knob(grt, gpu):
    case, singles = single_buffers(grt, "schwarzschild")
    sc, cams, _ = stacked_buffers(grt, "schwarzschild")
    assert grt.get_arithmetic() == 0
    grt.set_arithmetic("fused")
    try:
        fused = sc.render_pixels(0, 0, ROWS, COLS)
        seq = sc.trace_gbuffer_sequence(cams)
    finally:
        grt.set_arithmetic("exact")
    assert not np.array_equal(fused.xyza64, reference(grt, "schwarzschild")[1][0].xyza64)  # the knob is live
    for k in range(K):
        assert_same_buffer(seq[k], singles[k], ("fused knob", k))


# ------------------------------------------------- 9. CLI --------------------------
def test_cli_gbuffer_sequence_then_reshade_sequence(grt, gpu, tmp_path):
    text = (SCENES / "schwarzschild.toml").read_text() + "\n[adaptive_sampling]\nenabled = false\n"
    a_toml, b_toml = tmp_path / "a.toml", tmp_path / "b.toml"
    a_toml.write_text(text)
    swapped = text.replace("resources/disk.png", "resources/@").replace("resources/sphere.png", "resources/disk.png") \
                  .replace("resources/@", "resources/sphere.png").replace("temperature = 2000.0", "temperature = 3100.0")
    assert swapped != text
    b_toml.write_text(swapped)
    path = tmp_path / "path.txt"
    path.write_text("# x,y,z,phi,theta,psi\n" + "".join(
        f"{c[0]},{c[1]},{c[2]},{phi},{theta},{psi}\n" for c, phi, theta, psi in CAMS_FRONT))
    common = ["--width", 32, "--height", 24, "--max-steps", 20000, "--resource-root", RESOURCES]
    r = _grt(*common, "--config-file", a_toml, "gbuffer-sequence", "--camera-path", path, "--filename-pattern",
             tmp_path / "seq-%03d.grtg", "--first-index", 7)
    assert r.stderr.count("INFO saved g-buffer to") == 3 and "3 frames in 1 stacked launch" in r.stderr
    for k, (c, phi, theta, psi) in enumerate(CAMS_FRONT):
        _grt(*common, "--camera-position", f"{c[0]},{c[1]},{c[2]}", f"--phi={phi}", f"--theta={theta}", f"--psi={psi}",
             "--config-file", a_toml, "gbuffer", "--filename", tmp_path / f"one-{k}.grtg")
        assert (tmp_path / f"seq-{7 + k:03d}.grtg").read_bytes() == (tmp_path / f"one-{k}.grtg").read_bytes(), k
    assert len({(tmp_path / f"seq-{7 + k:03d}.grtg").read_bytes() for k in range(3)}) == 3
    r = _grt(*common, "--raw-out", tmp_path / "raw-%d.bin", "--config-file", b_toml, "reshade-sequence",
             "--gbuffer-pattern", tmp_path / "seq-%03d.grtg", "--frames", 3, "--first-index", 7, "--filename-pattern",
             tmp_path / "out-%03d.png")
    assert r.stderr.count("INFO saved image to") == 3 and "re-shaded 3 frames" in r.stderr
    for k in range(3):
        _grt(*common, "--raw-out", tmp_path / f"one-{k}.bin", "--config-file", b_toml, "reshade", "--gbuffer",
             tmp_path / f"seq-{7 + k:03d}.grtg", "--filename", tmp_path / f"one-{k}.png")
        assert (tmp_path / f"out-{7 + k:03d}.png").read_bytes() == (tmp_path / f"one-{k}.png").read_bytes(), k
        assert (tmp_path / f"raw-{7 + k}.bin").read_bytes() == (tmp_path / f"one-{k}.bin").read_bytes(), k
    assert len({(tmp_path / f"out-{7 + k:03d}.png").read_bytes() for k in range(3)}) == 3
    # a missing frame file is an error, not a shorter sequence
    q = subprocess.run([str(GRT), *map(str, common), "--config-file", str(b_toml), "reshade-sequence", "--gbuffer-pattern",
                        str(tmp_path / "seq-%03d.grtg"), "--frames", "4", "--first-index", "7", "--filename-pattern",
                        str(tmp_path / "miss-%03d.png")], capture_output=True, text=True, timeout=120)
    assert q.returncode == 1 and "seq-010.grtg" in q.stderr and not list(tmp_path.glob("miss-*.png"))
