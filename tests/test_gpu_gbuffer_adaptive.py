"""The supersampled geometry buffer on the GPU (grt_gbuffer_supersample,
grt_gbuffer_shade_section; marker `gpu`): the adaptive frame re-shaded bit for bit.

Every comparison is exact and against `render_section_ex` of the scene whose appearance is
applied: array_equal on the f64 bits, class, status, n_supersampled, and the failed
sub-sample and event lists.  The adaptive re-shade runs the selection kernels of that path
on the 1-spp re-shade (itself bit-identical) and the shade kernel's operations on the
numbers each sub-ray's trace had in registers, so no tolerance is involved.

Frames: the 48 x 48 BelowRISCO scene of tests/test_gpu_frames.py at 4 x 4 sub-rays, the
24 x 20 frames of tests/test_gpu_gbuffer.py, a 12 x 12 crop of the 96 x 96 winding frame of
tests/test_hit_pool.py, and 64 x 48 for the CLI.
"""
import ctypes as C
import errno
import math

import numpy as np
import pytest

from conftest import RESOURCES, SCENES

pytestmark = pytest.mark.gpu

MARK = np.array([-1.0, -2.0, -3.0, -4.0])
CAP = 1 << 14  # failed sub-sample capacity: above every count these frames produce


# ------------------------------------------------------------------------ scenes ----
def below_risco_scene(grt):
    """tests/test_gpu_frames.py::test_failed_subsamples_are_reported's scene: a disc that
    reaches inside the ISCO, so sub-rays fail with BelowRISCO."""
    b = grt.SceneBuilder(1, radius=2.0, horizon_epsilon=1e-4)
    b.integration(20000, 100.0, 0.01, 1e-7)
    pos = grt.cartesian_to_spherical((0.0, -16.0, 0.0, 3.5))
    vel = grt.stationary_velocity(1, 2.0, 0.0, pos)
    b.camera(pos, vel, math.pi / 4, 48, 48, 0.0, -3.142, 0.0)
    b.celestial(grt.Checker(0.0, 20.0, 20.0, (0, 255, 0), (0, 100, 0)))
    b.add_disc(3.0, 12.0, grt.BlackBody(1.0), temperature=5000.0)
    d = b.build()
    ad = grt.scene.default_adaptive()
    ad.enabled, ad.samples_per_axis = 1, 4
    return grt.Scene(C.pointer(d), keepalive=(d, b)), ad


def adaptive(grt, spa):
    ad = grt.scene.default_adaptive()
    ad.enabled, ad.samples_per_axis = 1, spa
    return ad


def selection(sc, ad):
    """The pixels the reference path supersamples: its sampling mask."""
    painted = sc.render_section_ex(adaptive=ad, sampling_mask_xyza=MARK, failure_capacity=1)
    return np.flatnonzero(np.all(painted.xyza64 == MARK, axis=1))


# --------------------------------------------------------------------- comparisons ----
def assert_same_section(got, want, what=""):
    assert np.array_equal(got.xyza64.view(np.uint64), want.xyza64.view(np.uint64)), (what, "xyza64")
    assert np.array_equal(got.ray_class, want.ray_class), (what, "class")
    assert np.array_equal(got.status, want.status), (what, "status")
    assert got.n_supersampled == want.n_supersampled, (what, got.n_supersampled, want.n_supersampled)
    assert got.n_failed_subsamples == want.n_failed_subsamples, (what, "failed count")
    assert np.array_equal(got.failed_subsamples, want.failed_subsamples), (what, "failed sub-samples")
    if want.subsample_events is not None:
        assert np.array_equal(got.subsample_events, want.subsample_events), (what, "events")
        assert np.array_equal(got.stop, want.stop) and np.array_equal(got.steps, want.steps), (what, "stop / steps")


def reference(sc, ad, **kw):
    return sc.render_section_ex(adaptive=ad, failure_capacity=CAP, log_events=True, **kw)


def reshade(gb, sc, ad, **kw):
    return gb.shade_section(sc, adaptive=ad, failure_capacity=CAP, log_events=True, **kw)


def assert_same_set(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ------------------------------------------------------------------- 1. identity ----
def identity_case(grt, name):
    from test_gpu_gbuffer import STOCK, stock

    if name == "below-risco":
        return below_risco_scene(grt)
    hs, sc = stock(grt, STOCK[name][0], **STOCK[name][1])
    assert hs.adaptive.enabled  # the stock scenes supersample
    return sc, hs.adaptive


@pytest.mark.parametrize("name", ["below-risco", "schwarzschild", "kerr-bl", "kerr-schild"])
def test_identity(grt, gpu, name):
    sc, ad = identity_case(grt, name)
    want = reference(sc, ad)
    assert want.n_supersampled > 21
    if name == "below-risco":
        assert want.n_failed_subsamples > 10
    gb = sc.trace_gbuffer(adaptive=ad)
    sub = gb.sub_info
    per = ad.samples_per_axis ** 2
    assert sub.samples_per_axis == ad.samples_per_axis and sub.n_sub_pixels == want.n_supersampled
    assert sub.n_sub_rays == sub.n_sub_pixels * per
    got, rep = reshade(gb, sc, ad)
    assert_same_section(got, want, name)
    assert rep["n_selected"] == rep["n_held"] == want.n_supersampled
    assert rep["n_traced"] == 0 and rep["n_missing"] == 0 and rep["top_up"]["rays"] == 0 and rep["trace_ms"] == 0.0
    assert rep["shade_ms"] > 0
    # the set: the selection in ascending pixel order, no ray with the overflow flag
    a = gb.sub_arrays()
    assert np.array_equal(a["sub_pixel"], selection(sc, ad))
    assert not np.any(a["status"] & grt._lib.FLAG_HIT_OVERFLOW)
    assert int(a["layer_start"][-1]) == sub.n_sub_layers == a["object"].size
    # the mask variant paints the same pixels
    painted, rep_m = gb.shade_section(sc, adaptive=ad, sampling_mask_xyza=MARK)
    want_m = sc.render_section_ex(adaptive=ad, sampling_mask_xyza=MARK)
    assert_same_section(painted, want_m, name + " mask")
    assert rep_m["n_selected"] == want.n_supersampled and rep_m["n_traced"] == 0
    # adaptive off, no mask: the 1-spp frame in f64
    off = adaptive(grt, ad.samples_per_axis)
    off.enabled = 0
    plain, _ = gb.shade_section(sc, adaptive=off)
    assert np.array_equal(plain.xyza64.view(np.uint64), gb.shade(sc).xyza64.view(np.uint64))
    assert plain.n_supersampled == 0
    gb.close()


# ------------------------------------------------- 2. another appearance, top-up ----
def busy_pair(grt, name):
    """tests/test_gpu_gbuffer.py's reshade_pair: A, and B with everything that is free to
    differ changed, so that the two appearances select different pixels."""
    from test_gpu_gbuffer import built_scene, reshade_pair

    da, db = reshade_pair(grt, name)
    return built_scene(grt, da), built_scene(grt, db)


@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl"])
def test_another_appearance_tops_up(grt, gpu, name):
    sa, sb = busy_pair(grt, name)
    ad = adaptive(grt, 2)
    sel_a, sel_b = selection(sa, ad), selection(sb, ad)
    new = np.setdiff1d(sel_b, sel_a)
    shared = np.intersect1d(sel_a, sel_b)
    print(f"{name}: A selects {sel_a.size}, B {sel_b.size}, new {new.size}, shared {shared.size}")
    assert new.size >= 10 and shared.size >= 10, (new.size, shared.size)
    want_a, want_b = reference(sa, ad), reference(sb, ad)
    gb = sa.trace_gbuffer(adaptive=ad)
    assert gb.sub_info.n_sub_pixels == sel_a.size
    before = gb.sub_arrays()
    with pytest.raises(grt.GBufferMissing) as e:
        reshade(gb, sb, ad)
    assert f"({-errno.ENODATA})" in str(e.value) and str(new.size) in str(e.value)
    assert e.value.report["n_missing"] == new.size and e.value.report["n_held"] == shared.size
    assert_same_set(gb.sub_arrays(), before, "a refused call leaves the set alone")
    got, rep = reshade(gb, sb, ad, tracer=sb)
    assert_same_section(got, want_b, name + " B, top-up")
    assert (rep["n_selected"], rep["n_held"], rep["n_traced"], rep["n_missing"]) == (sel_b.size, shared.size, new.size, 0)
    assert rep["top_up"]["rays"] == new.size * 4 and rep["trace_ms"] > 0
    a = gb.sub_arrays()
    assert np.array_equal(a["sub_pixel"], np.concatenate([sel_a, new]))  # appended, ascending
    again, rep2 = reshade(gb, sb, ad, tracer=sb)
    assert_same_section(again, want_b, name + " B, repeat")
    assert rep2["n_traced"] == 0 and rep2["top_up"]["rays"] == 0 and rep2["n_held"] == sel_b.size
    assert_same_set(gb.sub_arrays(), a, "a repeat appends nothing")
    back, rep3 = reshade(gb, sa, ad)
    assert_same_section(back, want_a, name + " A, after the top-up")
    assert rep3["n_traced"] == 0
    gb.close()


# ------------------------------------------------------------ 3. chunks and pool ----
def test_chunks(grt, gpu):
    L = grt._lib
    sc, ad = below_risco_scene(grt)
    want = reference(sc, ad)
    one = sc.trace_gbuffer(adaptive=ad)
    L.check(L.lib().grt_set_sub_chunk(7 * 16))  # 7 pixels of 16 sub-rays per chunk
    try:
        assert want.n_supersampled % 7 != 0 or want.n_supersampled > 7  # a part-filled or a second chunk
        many = sc.trace_gbuffer(adaptive=ad)
        got, rep = reshade(many, sc, ad)
    finally:
        L.check(L.lib().grt_set_sub_chunk(0))
    assert_same_set(many.sub_arrays(), one.sub_arrays(), "chunks of 7 pixels")
    assert_same_section(got, want, "chunks of 7 pixels")
    assert rep["n_traced"] == 0
    one.close()
    many.close()


def test_small_pool(grt, gpu):
    """Sub-rays with more window hits than the workspace slots, traced by a scene copy whose
    hit pool starts at 64 records: the chunk is traced again with a grown pool and the set
    equals the one a roomy pool gives."""
    from test_gpu_gbuffer import built_scene
    from test_hit_pool import winding_scene

    L = grt._lib
    d = winding_scene(grt)
    rect = (38, 46, 12, 12)  # inside the heavy band of tests/test_hit_pool.py::test_full_pool
    pixels = np.arange(rect[2] * rect[3], dtype=np.uint32)
    roomy = built_scene(grt, d)
    gb1 = roomy.trace_gbuffer(*rect)
    st1 = gb1.supersample(roomy, pixels, 2)
    assert st1["rays"] == pixels.size * 4
    a = gb1.sub_arrays()
    layers = np.diff(a["layer_start"].astype(np.int64))
    print(f"winding crop: {int((layers > L.GRT_MAX_HITS).sum())} of {layers.size} sub-rays past the slots, "
          f"{int(np.maximum(layers - L.GRT_MAX_HITS, 0).sum())} pool records at least")
    assert np.maximum(layers - L.GRT_MAX_HITS, 0).sum() > 64  # more pool records than the small pool has
    L.check(L.lib().grt_set_hit_pool_min(64))
    try:
        small = built_scene(grt, d)  # a fresh device copy: a 64-record pool
        gb2 = roomy.trace_gbuffer(*rect)
        st2 = gb2.supersample(small, pixels, 2)
    finally:
        L.check(L.lib().grt_set_hit_pool_min(1 << 20))
    assert st2["rays"] > pixels.size * 4  # more than one trace
    b = gb2.sub_arrays()
    assert_same_set(a, b, "small pool")
    assert not np.any(b["status"] & L.FLAG_HIT_OVERFLOW)
    gb1.close()
    gb2.close()


# ------------------------------------------------- 4. round trips and refusals ----
def test_round_trips(grt, gpu, tmp_path):
    from test_gpu_gbuffer import STOCK, stock

    sc, ad = identity_case(grt, "schwarzschild")
    want = reference(sc, ad)
    gb = sc.trace_gbuffer(adaptive=ad)
    up = grt.GBuffer.from_arrays(gb.info, gb.arrays(), device=0)
    assert up.sub_info.samples_per_axis == 0
    up.set_sub_arrays(gb.sub_info, gb.sub_arrays())
    got, rep = reshade(up, sc, ad)
    assert_same_section(got, want, "download -> upload")
    assert rep["n_traced"] == 0
    gb.save(tmp_path / "a.grtg")
    gb.save_sub(tmp_path / "a.grtg.sub")
    loaded = grt.GBuffer.load(tmp_path / "a.grtg", device=0)
    loaded.load_sub(tmp_path / "a.grtg.sub")
    got, rep = reshade(loaded, sc, ad)
    assert_same_section(got, want, "save -> load")
    assert rep["n_traced"] == 0 and bytes(loaded.sub_info) == bytes(gb.sub_info)
    # a second run (a fresh device copy) writes the same bytes
    _, sc2 = stock(grt, STOCK["schwarzschild"][0], **STOCK["schwarzschild"][1])
    gb2 = sc2.trace_gbuffer(adaptive=ad)
    gb2.save_sub(tmp_path / "b.grtg.sub")
    assert (tmp_path / "a.grtg.sub").read_bytes() == (tmp_path / "b.grtg.sub").read_bytes()
    for g in (gb, up, loaded, gb2):
        g.close()


def _rc(exc):
    return int(str(exc.value).split("(")[1].split(")")[0])


def test_refusals(grt, gpu, tmp_path):
    from test_gpu_gbuffer import STOCK, stock

    sc, ad = identity_case(grt, "schwarzschild")
    gb = sc.trace_gbuffer(adaptive=ad)
    want = reference(sc, ad)
    gb.save_sub(tmp_path / "a.sub")
    # a sidecar against another buffer's info
    crop = sc.trace_gbuffer(1, 1, 8, 8)
    with pytest.raises(grt.GrtError, match="info") as e:
        crop.load_sub(tmp_path / "a.sub")
    assert _rc(e) == -errno.EINVAL
    # another samples_per_axis than the set's
    other = adaptive(grt, ad.samples_per_axis + 1)
    for call in (lambda: gb.shade_section(sc, adaptive=other), lambda: gb.supersample(sc, [0], ad.samples_per_axis + 1)):
        with pytest.raises(grt.GrtError, match="samples_per_axis") as e:
            call()
        assert _rc(e) == -errno.EINVAL and str(ad.samples_per_axis) in str(e.value)
    # a tracer with another camera, or another step budget
    opts = dict(STOCK["schwarzschild"][1])
    _, moved = stock(grt, STOCK["schwarzschild"][0], **{**opts, "camera_position": (-15.0, 0.0, 3.5)})
    _, fewer = stock(grt, STOCK["schwarzschild"][0], **{**opts, "max_steps": 99999})
    for tracer, field in ((moved, "camera"), (fewer, "max_steps")):
        with pytest.raises(grt.GrtError, match=field) as e:
            gb.supersample(tracer, [0, 1, 2], ad.samples_per_axis)
        assert _rc(e) == -errno.EINVAL
        with pytest.raises(grt.GrtError, match=field) as e:
            gb.shade_section(sc, adaptive=ad, tracer=tracer)
        assert _rc(e) == -errno.EINVAL
    with pytest.raises(grt.GrtError, match="outside") as e:
        gb.supersample(sc, [int(gb.info.n_pixels)], ad.samples_per_axis)
    assert _rc(e) == -errno.EINVAL
    # an upload is held to the file's checks: no kernel sees a pixel or an object out of range
    sub, good = gb.sub_info, gb.sub_arrays()
    for what, change in (("duplicate", lambda a: a["sub_pixel"].__setitem__(1, a["sub_pixel"][0])),
                         ("outside", lambda a: a["sub_pixel"].__setitem__(0, int(gb.info.n_pixels))),
                         ("GRT_FLAG_HIT_OVERFLOW", lambda a: a["status"].__setitem__(3, 0x80)),
                         ("names object", lambda a: a["object"].__setitem__(0, 7))):
        bad = {k: v.copy() for k, v in good.items()}
        change(bad)
        with pytest.raises(grt.GrtError, match=what) as e:
            gb.set_sub_arrays(sub, bad)
        assert _rc(e) == -errno.EINVAL, what
    got, rep = reshade(gb, sc, ad)
    assert_same_section(got, want, "after the refusals")
    assert rep["n_traced"] == 0
    gb.close()
    crop.close()


# ------------------------------------------------------------------------- 5. CLI ----
def test_cli_adaptive_gbuffer_then_reshade(grt, gpu, tmp_path):
    from test_gpu_gbuffer import _grt

    text = (SCENES / "schwarzschild.toml").read_text()  # adaptive sampling left enabled
    a_toml, b_toml = tmp_path / "a.toml", tmp_path / "b.toml"
    a_toml.write_text(text)
    swapped = text.replace("resources/disk.png", "resources/@").replace("resources/sphere.png", "resources/disk.png") \
                  .replace("resources/@", "resources/sphere.png").replace("temperature = 2000.0", "temperature = 3100.0")
    assert swapped != text and swapped.count("disk.png") == 1
    b_toml.write_text(swapped)
    common = ["--width", 64, "--height", 48, "--camera-position", "-16,0,3.5", "--theta", "-3.142", "--max-steps", 100000,
              "--resource-root", RESOURCES]
    gfile = tmp_path / "a.grtg"
    _grt(*common, "--config-file", a_toml, "gbuffer", "--adaptive", "--filename", gfile)
    sidecar = tmp_path / "a.grtg.sub"
    assert sidecar.exists()
    size_a = sidecar.stat().st_size
    r = _grt(*common, "--raw-out", tmp_path / "reshade.raw", "--config-file", b_toml, "reshade", "--adaptive",
             "--gbuffer", gfile, "--filename", tmp_path / "reshade.png")
    assert "selected" in r.stderr + r.stdout and "traced" in r.stderr + r.stdout
    _grt(*common, "--raw-out", tmp_path / "render.raw", "--config-file", b_toml, "render", "--filename",
         tmp_path / "render.png")
    assert (tmp_path / "reshade.png").read_bytes() == (tmp_path / "render.png").read_bytes()
    raw = (tmp_path / "render.raw").read_bytes()
    assert len(raw) == 64 * 48 * 32 and (tmp_path / "reshade.raw").read_bytes() == raw
    assert sidecar.stat().st_size >= size_a
    # the sampling mask, as `render` shows it
    _grt(*common, "--config-file", b_toml, "--show-sampling-mask", "reshade", "--adaptive", "--gbuffer", gfile,
         "--filename", tmp_path / "reshade_mask.png")
    _grt(*common, "--config-file", b_toml, "--show-sampling-mask", "render", "--filename", tmp_path / "render_mask.png")
    assert (tmp_path / "reshade_mask.png").read_bytes() == (tmp_path / "render_mask.png").read_bytes()
    assert (tmp_path / "render_mask.png").read_bytes() != (tmp_path / "render.png").read_bytes()
    # without --adaptive both commands are the 1-spp pair: no sidecar, the 1-spp picture
    plain = tmp_path / "plain.grtg"
    _grt(*common, "--config-file", a_toml, "gbuffer", "--filename", plain)
    assert not (tmp_path / "plain.grtg.sub").exists()
    assert plain.read_bytes() == gfile.read_bytes()  # the .grtg file keeps its bytes
    _grt(*common, "--config-file", b_toml, "reshade", "--gbuffer", plain, "--filename", tmp_path / "plain.png")
    assert (tmp_path / "plain.png").read_bytes() != (tmp_path / "render.png").read_bytes()
