"""The disc's orbital motion from one geometry buffer on the GPU (grt_gbuffer_shade_times,
grt_gbuffer_shade_section_at; marker `gpu`).

The reference of every frame comparison is the static deferred shade of a buffer whose disc
layers' (u, v) went through the HOST restatement of the rule (grt_gbuffer_orbit_uv), and the
comparisons are exact (assert_same_frame / assert_same_section: the f32 / f64 bits, class,
status): device and host state the rule with the same operations in the same order over the
same glibc-exact pow and sincos, and every |omega t| here is far below 105414350.  The oracle
tie alone has the project's 1e-4.

Frames are the 24 x 20 ones of tests/test_gpu_gbuffer.py, 64 x 48 for the CLI.  Scenes:
KBL / KS  the stock kerr-bl / kerr-schild cases, the appearance with the disc's BlackBody
          texture replaced by a bitmap;
S2        reshade_pair("schwarzschild"): the buffer from A, shaded under A (checker disc) and
          B (sphere + bitmap disc, several layers blend);
S1        a disc-only Schwarzschild scene with a constant-temperature bitmap disc.
"""
import ctypes as C
import errno
import math
import subprocess

import numpy as np
import pytest

from conftest import RESOURCES, SCENES
from test_gpu_gbuffer import (COLS, GRT, ROWS, STOCK, _bitmap, _rc, assert_same_frame, built_scene, reshade_pair, stock,
                              stock_case)
from test_gpu_gbuffer_adaptive import CAP, adaptive, assert_same_section, assert_same_set, reference

pytestmark = pytest.mark.gpu

TIMES = (0.0, 1.0, 37.5, -12.25, 1e4)
T_MOVED = TIMES.index(37.5)


# ------------------------------------------------------------------------ scenes ----
def _bitmap_texture(grt, keep):
    """The grt_texture_desc of `_bitmap(grt, 2, 1.5, alpha_lo=40)` (SceneBuilder's own mapping)."""
    b = grt.SceneBuilder(grt._lib.GEOM_EUCLIDEAN)
    tex = b._texture(_bitmap(grt, 2, 1.5, alpha_lo=40))
    keep.append(b)
    return tex


def _stock_with_bitmap_disc(grt, name):
    """(traced scene, appearance scene): the stock case and its descriptor with the disc's
    BlackBody texture replaced by the bitmap."""
    L = grt._lib
    hs, sc = stock(grt, STOCK[name][0], **STOCK[name][1])
    d = type(hs.desc).from_buffer_copy(hs.desc)
    keep = [hs]
    discs = [k for k in range(d.n_objects) if d.objects[k].kind == L.OBJ_DISC]
    assert len(discs) == 1 and d.objects[discs[0]].texture.kind == L.TEX_BLACKBODY
    d.objects[discs[0]].texture = _bitmap_texture(grt, keep)
    keep.append(d)
    return hs, sc, grt.Scene(C.pointer(d), keepalive=keep, adaptive=hs.adaptive)


def s1_desc(grt):
    L = grt._lib
    b = grt.SceneBuilder(L.GEOM_SCHWARZSCHILD, radius=1.0, a=0.0, horizon_epsilon=1e-4)
    b.integration(20000, 100.0, 0.01, 1e-5)
    pos = grt.cartesian_to_spherical((0.0, -14.0, 0.0, 2.5))
    b.camera(pos, grt.stationary_velocity(L.GEOM_SCHWARZSCHILD, 1.0, 0.0, pos), math.pi / 4, ROWS, COLS, 0.0, -3.142, 0.0)
    b.celestial(grt.Checker(0.0, 16.0, 8.0, (20, 20, 80), (200, 200, 255)))
    # a constant-temperature model: the oracle exposes no temperature lookup for a Kerr-LUT disc
    b.add_disc(3.0, 10.0, _bitmap(grt, 2, 1.5, alpha_lo=40), temperature=2500.0, constant_temperature=True)
    d = b.build()
    d._keep_builder = b
    return d


_CASES = {}


def case(grt, name):
    """name -> dict(tracer, apps: {label: appearance scene}, gb, info, arrays, min_disc), once."""
    if name in _CASES:
        return _CASES[name]
    if name in ("KBL", "KS"):
        hs, sc, app = _stock_with_bitmap_disc(grt, "kerr-bl" if name == "KBL" else "kerr-schild")
        c = dict(tracer=sc, apps={"bitmap": app}, moved="bitmap", min_disc=140, stock_adaptive=hs.adaptive)
    elif name == "S2":
        da, db = reshade_pair(grt, "schwarzschild")
        sa, sb = built_scene(grt, da), built_scene(grt, db)
        c = dict(tracer=sa, apps={"A": sa, "B": sb}, moved="B", min_disc=15)
    else:
        d = s1_desc(grt)
        sc = built_scene(grt, d)
        c = dict(tracer=sc, apps={"bitmap": sc}, moved="bitmap", min_disc=45, desc=d)
    c["gb"] = c["tracer"].trace_gbuffer()
    c["info"], c["arrays"] = c["gb"].info, c["gb"].arrays()
    _CASES[name] = c
    return c


def rotated(grt, info, arrays, t):
    """The arrays with (u, v) through the host rule at time t."""
    out = dict(arrays)
    out["u"], out["v"] = grt.gbuffer_orbit_uv(info.shape, arrays["object"], arrays["u"], arrays["v"], arrays["radius"], t)
    return out


def disc_pixels(grt, info, a):
    """Pixels with at least one disc layer."""
    L = grt._lib
    is_disc = np.array([info.shape.objects[int(o)].kind == L.OBJ_DISC for o in a["object"]], bool)
    per = np.add.reduceat(np.concatenate([is_disc, [False]]).astype(np.int64),
                          np.minimum(a["layer_start"][:-1].astype(np.int64), len(is_disc)))
    return np.where(np.diff(a["layer_start"].astype(np.int64)) > 0, per, 0) > 0


class Frame:
    """Frame k of shade_orbit's dict with RenderResult's field names."""

    def __init__(self, out, k):
        self.xyza, self.xyza64, self.ray_class, self.status = out["xyza"][k], out["xyza64"][k], out["class"][k], out["status"][k]


# ------------------------------------------------------- 1. device against host rule ----
@pytest.mark.parametrize("name", ["KBL", "KS", "S2", "S1"])
def test_device_against_host_rule(grt, gpu, name):
    c = case(grt, name)
    gb, info, a = c["gb"], c["info"], c["arrays"]
    n_disc = int(disc_pixels(grt, info, a).sum())
    layers = np.diff(a["layer_start"].astype(np.int64))
    print(f"{name}: {n_disc} pixels with a disc layer, {(layers >= 2).sum()} with >= 2 layers")
    assert n_disc >= c["min_disc"], n_disc
    for label, app in c["apps"].items():
        out = gb.shade_orbit(app, TIMES)
        assert out["xyza64"].shape == (len(TIMES), ROWS * COLS, 4)
        static = gb.shade(app)
        for k, t in enumerate(TIMES):
            up = grt.GBuffer.from_arrays(info, rotated(grt, info, a, t))
            assert_same_frame(Frame(out, k), up.shade(app), (name, label, t))
            up.close()
            assert np.array_equal(out["stop"][k], a["stop"]) and np.array_equal(out["steps"][k], a["steps"]), (name, t)
        if label == c["moved"]:
            moved = np.any(out["xyza64"][T_MOVED].view(np.uint64) != static.xyza64.view(np.uint64), axis=1)
            print(f"{name} / {label}: {moved.sum()} pixels differ from the static frame at t = 37.5")
            assert moved.sum() * 4 >= c["min_disc"], moved.sum()
            assert not np.any(moved & ~disc_pixels(grt, info, a))  # only pixels with a disc layer move


# ----------------------------------------------------------------- 2. identities ----
@pytest.mark.parametrize("name", ["KBL", "KS", "S2", "S1"])
def test_time_zero_is_the_static_frame(grt, gpu, name):
    c = case(grt, name)
    for label, app in c["apps"].items():
        out = c["gb"].shade_orbit(app, [0.0, -0.0])
        want = c["gb"].shade(app)
        assert_same_frame(Frame(out, 0), want, (name, label))
        assert_same_frame(Frame(out, 1), want, (name, label, "-0.0"))


@pytest.mark.parametrize("name", ["kerr-bl", "kerr-schild", "euclidean", "euclidean-spherical"])
def test_static_appearances_and_flat_charts_do_not_move(grt, gpu, name):
    """A BlackBody disc's colour does not depend on (u, v); the flat charts' emitter is at rest."""
    L = grt._lib
    hs, sc, want, gb = stock_case(grt, name)
    d = hs.desc
    discs = [k for k in range(d.n_objects) if d.objects[k].kind == L.OBJ_DISC]
    assert discs
    if name.startswith("kerr"):
        assert all(d.objects[k].texture.kind == L.TEX_BLACKBODY for k in discs)
    else:
        assert grt.orbit_rate(d.geometry, d.radius, d.a, 5.0) == 0.0
    a = gb.arrays()
    if name.startswith("kerr"):
        assert disc_pixels(grt, gb.info, a).sum() >= 140
    else:  # at 24 x 20 the flat frames' layers may all be the sphere's
        assert a["object"].size > 0
    out = gb.shade_orbit(sc, TIMES)
    for k, t in enumerate(TIMES):
        assert_same_frame(Frame(out, k), want, (name, t))


# ------------------------------------------------------------------- 3. stacking ----
@pytest.mark.parametrize("name", ["KBL", "S2"])
def test_stacking(grt, gpu, name):
    c = case(grt, name)
    gb, app = c["gb"], c["apps"][c["moved"]]
    singles = [gb.shade_orbit(app, [t]) for t in TIMES]

    def check(out, what):
        for k in range(len(TIMES)):
            assert_same_frame(Frame(out, k), Frame(singles[k], 0), (name, what, k))
            for f in ("stop", "steps"):
                assert np.array_equal(out[f][k], singles[k][f][0]), (name, what, f, k)

    check(gb.shade_orbit(app, TIMES), "one group")
    try:
        for frames in (1, 2):
            grt.set_sequence_group(frames * ROWS * COLS)
            check(gb.shade_orbit(app, TIMES), f"groups of {frames}")
    finally:
        grt.set_sequence_group(0)
    # a subset of the fields
    part = gb.shade_orbit(app, TIMES, fields=("xyza64",))
    assert set(part) == {"xyza64", "stats"}
    assert np.array_equal(part["xyza64"].view(np.uint64), gb.shade_orbit(app, TIMES)["xyza64"].view(np.uint64))
    assert part["stats"]["kernel_ms"] > 0


# ----------------------------------------------------------------- 4. oracle tie ----
def test_oracle_tie(grt, oracle, gpu):
    """The rotated coordinates mean what the header says: fed to the ORACLE's texture lookup and
    blend, the host-rotated (u', v') give the device's frame at t = 37.5 within the project's
    1e-4 per channel, on the robust single-layer pixels of S1."""
    from test_gpu_parity import check_parity, oracle_pair, within

    L = grt._lib
    c = case(grt, "S1")
    d, a, gb, sc = c["desc"], c["arrays"], c["gb"], c["tracer"]
    t = 37.5
    got = sc.render_pixels(0, 0, ROWS, COLS)
    ref, probes = oracle_pair(oracle, d, 0, 0, ROWS, COLS)
    robust = check_parity(got, ref, probes, max_sensitive=0.05)
    frame = gb.shade_orbit(sc, [t])["xyza64"][0]
    u2, v2 = grt.gbuffer_orbit_uv(c["info"].shape, a["object"], a["u"], a["v"], a["radius"], t)
    layers = np.diff(a["layer_start"].astype(np.int64))
    black = np.array([0.0, 0.0, 0.0, 1.0])

    def terminal(i):
        if a["stop"][i] == L.STOP_CELESTIAL:
            return oracle.blend(black, oracle.texture_color(d, -1, a["sky_u"][i], a["sky_v"][i], a["sky_redshift"][i],
                                                            d.celestial_temperature))
        assert a["stop"][i] in (L.STOP_HORIZON, L.STOP_CLOSED_ORBIT)
        return oracle.blend(black, black)

    n = n_moved = 0
    for i in np.flatnonzero(robust & (a["status"] == 0) & (layers == 1)):
        if a["stop"][i] == L.STOP_NONE or a["stop"][i] == L.STOP_NAN:
            continue
        k = int(a["layer_start"][i])
        obj = int(a["object"][k])
        assert d.objects[obj].kind == L.OBJ_DISC and d.objects[obj].temp_kind == L.TEMP_CONSTANT
        col = oracle.texture_color(d, obj, u2[k], v2[k], a["redshift"][k], d.objects[obj].temp_constant)
        mine = oracle.blend(terminal(i), col)
        assert within(mine[None, :], frame[i][None, :])[0], ("S1", i, mine, frame[i])
        n += 1
        n_moved += not within(frame[i][None, :], ref["xyza"][i][None, :])[0]
    print(f"oracle tie: {n} pixels, {n_moved} of them moved by more than 1e-4 against the static oracle frame")
    assert n >= 20 and n_moved >= 5, (n, n_moved)


# ---------------------------------------------------------- 5. adaptive at a time ----
@pytest.mark.parametrize("name", ["KBL", "S2"])
def test_adaptive_at_a_time(grt, gpu, name):
    c = case(grt, name)
    tracer, app, info = c["tracer"], c["apps"][c["moved"]], c["info"]
    # KBL under its stock [adaptive_sampling], S2 (a built scene: it has none) at 4 x 4 sub-rays
    ad = c["stock_adaptive"] if name == "KBL" else adaptive(grt, 4)
    assert ad.enabled
    spa = int(ad.samples_per_axis)
    t = 37.5
    kw = dict(adaptive=ad, failure_capacity=CAP, log_events=True)
    gb = tracer.trace_gbuffer()
    assert gb.sub_info.n_sub_pixels == 0
    frame, rep = gb.shade_section(app, tracer=tracer, time=t, **kw)
    print(f"{name}: {frame.n_supersampled} supersampled at t = {t}, {rep['n_traced']} traced")
    assert frame.n_supersampled > 21
    assert rep["n_traced"] == rep["n_selected"] == frame.n_supersampled and rep["n_missing"] == 0
    # the same frame from rotated numbers through today's static path
    a, sub, s = gb.arrays(), gb.sub_info, gb.sub_arrays()
    up = grt.GBuffer.from_arrays(info, rotated(grt, info, a, t))
    up.set_sub_arrays(sub, rotated(grt, info, s, t))
    static, rep_s = up.shade_section(app, **kw)
    assert_same_section(static, frame, (name, "rotated arrays, static path"))
    assert rep_s["n_traced"] == 0 and rep_s["n_held"] == frame.n_supersampled
    # and it differs from the static adaptive frame of the unrotated buffer
    plain, _ = gb.shade_section(app, tracer=tracer, **kw)
    assert not np.array_equal(plain.xyza64.view(np.uint64), frame.xyza64.view(np.uint64))
    # a second call at the time traces nothing
    s = gb.sub_arrays()  # the static call may have topped the set up
    again, rep2 = gb.shade_section(app, tracer=tracer, time=t, **kw)
    assert_same_section(again, frame, (name, "repeat"))
    assert rep2["n_traced"] == 0 and rep2["n_missing"] == 0 and rep2["n_held"] == frame.n_supersampled
    assert_same_set(gb.sub_arrays(), s, "a repeat appends nothing")
    # the set holds unrotated numbers: what grt_gbuffer_supersample leaves on a fresh buffer
    timed = tracer.trace_gbuffer()
    timed.shade_section(app, tracer=tracer, time=t, **kw)
    held = timed.sub_arrays()
    fresh = tracer.trace_gbuffer()
    fresh.supersample(tracer, held["sub_pixel"], spa)
    assert np.array_equal(np.sort(held["sub_pixel"]), held["sub_pixel"])  # one top-up: ascending
    assert_same_set(fresh.sub_arrays(), held, (name, "the set is geometry"))
    # time=None is today's call; t = 0 gives its frame
    want = reference(app, ad)
    none, _ = tracer.trace_gbuffer().shade_section(app, tracer=tracer, time=None, **kw)
    assert_same_section(none, want, (name, "time=None"))
    zero, _ = tracer.trace_gbuffer().shade_section(app, tracer=tracer, time=0.0, **kw)
    assert_same_section(zero, want, (name, "time=0"))
    for g in (gb, up, timed, fresh):
        g.close()


# ------------------------------------------------------------------- 6. refusals ----
def test_refusals(grt, gpu):
    c = case(grt, "KBL")
    gb, app, tracer = c["gb"], c["apps"]["bitmap"], c["tracer"]
    want = gb.shade_orbit(app, [37.5])
    with pytest.raises(grt.GrtError, match="at least one time") as e:
        gb.shade_orbit(app, [])
    assert _rc(e) == -errno.EINVAL
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(grt.GrtError, match=r"times\[1\] is not finite") as e:
            gb.shade_orbit(app, [0.0, bad, 1.0])
        assert _rc(e) == -errno.EINVAL
        with pytest.raises(grt.GrtError, match="not finite") as e:
            gb.shade_section(app, adaptive=c["stock_adaptive"], tracer=tracer, time=bad)
        assert _rc(e) == -errno.EINVAL
    _, schw = stock(grt, STOCK["schwarzschild"][0], **STOCK["schwarzschild"][1])
    with pytest.raises(grt.GrtError, match="geometry") as e:
        gb.shade_orbit(schw, [1.0])
    assert _rc(e) == -errno.EINVAL
    with pytest.raises(grt.GrtError, match="geometry") as e:
        gb.shade_section(schw, adaptive=c["stock_adaptive"], time=1.0)
    assert _rc(e) == -errno.EINVAL
    with pytest.raises(grt.GrtError, match="xyza or xyza64") as e:
        gb.shade_orbit(app, [1.0], fields=("class", "status"))
    assert _rc(e) == -errno.EINVAL
    # the adaptive call without a tracer on an empty set
    empty = tracer.trace_gbuffer()
    with pytest.raises(grt.GBufferMissing) as e:
        empty.shade_section(app, adaptive=c["stock_adaptive"], time=37.5)
    assert f"({-errno.ENODATA})" in str(e.value) and e.value.report["n_missing"] > 21
    assert empty.sub_info.n_sub_pixels == 0
    empty.close()
    # a scene's copy on another device: refused as GBuffer.shade refuses it
    with pytest.raises(grt.GrtError) as e:
        gb.shade_orbit(app, [1.0], device=gb.info.device + 1)
    assert _rc(e) == -errno.EINVAL
    again = gb.shade_orbit(app, [37.5])
    assert np.array_equal(again["xyza64"].view(np.uint64), want["xyza64"].view(np.uint64))  # after the refusals


# ------------------------------------------------------------------------ 7. CLI ----
def _grt(*args):
    """One `grt` run: a fresh child process with its own time limit."""
    r = subprocess.run([str(GRT), *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _png(grt, path, xyza64, w, h):
    L = grt._lib
    rgb = np.ascontiguousarray(grt.xyz_to_srgb8(xyza64, 0), np.uint8)
    L.check(L.lib().grt_write_png_rgb(str(path).encode(), L.ptr(rgb, C.c_uint8), w, h), "grt_write_png_rgb")
    return path.read_bytes()


def test_cli_reshade_orbit(grt, gpu, tmp_path):
    w, h = 64, 48
    base = (SCENES / "schwarzschild.toml").read_text()
    off, on = tmp_path / "off.toml", tmp_path / "on.toml"
    off.write_text(base + "\n[adaptive_sampling]\nenabled = false\n")
    on.write_text(base)
    cam = dict(camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=100000)
    common = ["--width", w, "--height", h, "--camera-position", "-16,0,3.5", "--theta", "-3.142", "--max-steps", 100000,
              "--resource-root", RESOURCES]
    size = ["--width", w, "--height", h, "--resource-root", RESOURCES]
    grtg = tmp_path / "a.grtg"
    _grt(*common, "--config-file", off, "gbuffer", "--filename", grtg)
    _grt(*size, "--config-file", off, "reshade", "--gbuffer", grtg, "--filename", tmp_path / "static.png")
    r = _grt(*size, "--config-file", off, "reshade-orbit", "--gbuffer", grtg, "--times", "0,12.5,3", "--filename-pattern",
             tmp_path / "f-%04d.png", "--raw-out-pattern", tmp_path / "f-%04d.raw")
    assert "at 3 times" in r.stderr
    frames = [(tmp_path / f"f-{k:04d}.png").read_bytes() for k in range(3)]
    assert frames[0] == (tmp_path / "static.png").read_bytes()
    assert frames[1] != frames[0] and frames[2] != frames[1]
    hs = grt.HostScene(str(off), grt.GlobalOpts(width=w, height=h, **cam), str(RESOURCES))
    sc = grt.Scene(hs.desc_ptr(), keepalive=hs, adaptive=hs.adaptive)
    gb = grt.GBuffer.load(grtg)
    out = gb.shade_orbit(sc, [0.0, 12.5, 25.0], fields=("xyza64",))["xyza64"]
    for k in (1, 2):
        assert frames[k] == _png(grt, tmp_path / f"want-{k}.png", out[k], w, h), k
        assert (tmp_path / f"f-{k:04d}.raw").read_bytes() == out[k].tobytes(), k
    # --adaptive: frame 0 is `reshade --adaptive`'s, and the sidecar is written once at the end
    _grt(*size, "--config-file", on, "reshade", "--gbuffer", grtg, "--adaptive", "--filename", tmp_path / "ad.png")
    sidecar = tmp_path / "a.grtg.sub"
    assert sidecar.exists()
    sidecar.unlink()
    r = _grt(*size, "--config-file", on, "reshade-orbit", "--gbuffer", grtg, "--adaptive", "--times", "0,12.5,3",
             "--filename-pattern", tmp_path / "g-%04d.png")
    assert (tmp_path / "g-0000.png").read_bytes() == (tmp_path / "ad.png").read_bytes()
    assert (tmp_path / "g-0001.png").read_bytes() != (tmp_path / "g-0000.png").read_bytes()
    assert r.stderr.count("saved sub-sample set") == 1 and sidecar.exists()
    # frame 1 is shade_section at its time
    ad_hs = grt.HostScene(str(on), grt.GlobalOpts(width=w, height=h, **cam), str(RESOURCES))
    ad_sc = grt.Scene(ad_hs.desc_ptr(), keepalive=ad_hs, adaptive=ad_hs.adaptive)
    f1, _ = gb.shade_section(ad_sc, tracer=ad_sc, time=12.5)
    assert (tmp_path / "g-0001.png").read_bytes() == _png(grt, tmp_path / "want-ad.png", f1.xyza64, w, h)
    gb.close()
