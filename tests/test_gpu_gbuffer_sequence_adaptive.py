"""Adaptive frames for g-buffer sequences on the GPU (grt_gbuffer_supersample_sequence,
grt_gbuffer_shade_section_sequence; marker `gpu`): the sub-sample sets of a stack of buffers
filled by stacked traces, and the adaptive frames of the stack re-shaded in stacked launches.

The reference of every comparison is the per-frame route: `GBuffer.supersample` and
`GBuffer.shade_section` of a buffer traced alone, with a tracer created with that frame's
camera, `render_section_ex` of a scene with that camera, `grt render` / `grt gbuffer --adaptive`
per camera.  Every comparison is on bits (grt_gbuffer_sub_info, sub_pixel, the twelve arrays,
the sidecar files; f64 frames, class, status, n_supersampled, the failure and event lists): the
stacked calls run the same operations on the same operands, so no tolerance is involved.

The frames are the sequence tests' (tests/test_gpu_sequence.py, tests/test_gpu_gbuffer_sequence.py):
24 cols x 20 rows x 3 cameras, so 8x8 tiles straddle frames and the cameras differ in position
and in all three angles.  The stacked calls get the scene with camera 0 as their tracer, so
frames 1 and 2 hold only if each ray takes the camera its buffer recorded.
"""
import ctypes as C
import errno
import math
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import RESOURCES, SCENES
from test_gpu_gbuffer import _grt
from test_gpu_gbuffer_adaptive import (CAP, MARK, adaptive, assert_same_section, assert_same_set, below_risco_scene,
                                       reshade, selection)
from test_gpu_gbuffer_adaptive import reference as section_reference
from test_gpu_gbuffer_sequence import Pair, _rc
from test_gpu_sequence import CAMS_FRONT, COLS, K, N, ROWS, reference

pytestmark = pytest.mark.gpu

_PER_FRAME = {}


def per_frame(grt, name):
    """(case, stock adaptive configuration, per frame: tracer scene, the selection of its
    adaptive frame, a buffer traced alone with the sub-rays of that selection, its set), once
    per scene and never modified."""
    if name not in _PER_FRAME:
        case = reference(grt, name)[0]
        ad = grt.default_adaptive()  # the stock configuration: enabled, 4 x 4 samples
        assert ad.enabled == 1
        frames = []
        for k in range(K):
            sc = case.scene(k)
            sel = selection(sc, ad).astype(np.uint32)
            gb = sc.trace_gbuffer()
            gb.supersample(sc, sel, ad.samples_per_axis)
            frames.append(SimpleNamespace(scene=sc, sel=sel, gb=gb, sub=gb.sub_arrays(), sub_info=bytes(gb.sub_info)))
        # what the existing tests on these frames hold: every frame selects, one fills a second chunk of 7
        assert all(f.sel.size >= 1 for f in frames), [f.sel.size for f in frames]
        if name != "winding":
            assert max(f.sel.size for f in frames) > 7, [f.sel.size for f in frames]
        _PER_FRAME[name] = (case, ad, frames)
    return _PER_FRAME[name]


def assert_same_sets(bufs, frames, what=""):
    for k, (gb, f) in enumerate(zip(bufs, frames)):
        assert bytes(gb.sub_info) == f.sub_info, (what, k, "sub_info")
        assert_same_set(gb.sub_arrays(), f.sub, (what, k))


# ------------------------------------------------------------- 1. the stacked fill ----
@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl", "kerr-schild", "euclidean"])
def test_stacked_fill_equals_the_per_frame_sets(grt, gpu, name, tmp_path):
    case, ad, frames = per_frame(grt, name)
    spa, per = ad.samples_per_axis, ad.samples_per_axis ** 2
    sc, cams = case.scene(0), case.cameras()
    seq = sc.trace_gbuffer_sequence(cams)
    assert all(b.sub_info.samples_per_axis == 0 for b in seq)
    total = sum(f.sel.size for f in frames)
    # any order, duplicates allowed
    st = grt.supersample_sequence(seq, sc, [np.concatenate([f.sel[::-1], f.sel[:2]]) for f in frames], spa)
    rep = st["report"]
    assert (rep.n_frames, rep.n_launches, rep.n_traces) == (K, 1, 1)
    assert st["rays"] == total * per and st["hit_overflows"] == 0
    assert rep.trace_ms > 0 and rep.fill_ms > 0 and rep.wall_ms >= rep.trace_ms
    assert_same_sets(seq, frames, name)
    for k in range(K):
        seq[k].save_sub(tmp_path / f"stacked-{k}.sub")
        frames[k].gb.save_sub(tmp_path / f"single-{k}.sub")
        assert (tmp_path / f"stacked-{k}.sub").read_bytes() == (tmp_path / f"single-{k}.sub").read_bytes(), k
    # three different sets
    assert len({(tmp_path / f"stacked-{k}.sub").read_bytes() for k in range(K)}) == K
    # held pixels are skipped: a second call traces nothing and appends nothing
    st = grt.supersample_sequence(seq, sc, [f.sel for f in frames], spa)
    assert st["rays"] == 0 and st["report"].n_launches == 0
    assert_same_sets(seq, frames, name + ", again")
    # the buffers in another order, and a stack of one
    order = [2, 0, 1]
    seq = sc.trace_gbuffer_sequence(cams)
    grt.supersample_sequence([seq[k] for k in order], sc, [frames[k].sel for k in order], spa)
    assert_same_sets(seq, frames, name + ", order 2 0 1")
    seq = sc.trace_gbuffer_sequence(cams)
    grt.supersample_sequence([seq[1]], sc, [frames[1].sel], spa)
    assert_same_sets([seq[1]], [frames[1]], name + ", K = 1")
    assert seq[0].sub_info.samples_per_axis == 0 and seq[2].sub_info.n_sub_pixels == 0
    # a set grown in two calls, the second list overlapping the first
    seq = sc.trace_gbuffer_sequence(cams)
    grt.supersample_sequence(seq, sc, [f.sel[: f.sel.size // 2] for f in frames], spa)
    grt.supersample_sequence(seq, sc, [f.sel for f in frames], spa)
    for k, f in enumerate(frames):
        two = seq[k].sub_arrays()
        half = f.sel.size // 2
        assert np.array_equal(two["sub_pixel"], np.concatenate([f.sel[:half], f.sel[half:]])), k
        want = frames[k].scene.trace_gbuffer()
        want.supersample(frames[k].scene, f.sel[:half], spa)
        want.supersample(frames[k].scene, f.sel, spa)
        assert_same_set(two, want.sub_arrays(), (name, k, "two calls"))


# ------------------------------------------------------------- 5. chunks ---------------
def test_chunks_span_frames(grt, gpu):
    L = grt._lib
    case, ad, frames = per_frame(grt, "schwarzschild")
    spa = ad.samples_per_axis
    sc, cams = case.scene(0), case.cameras()
    total = sum(f.sel.size for f in frames)
    starts = np.cumsum([0] + [f.sel.size for f in frames])
    # a chunk of 7 pixels holds the end of one frame's list and the start of the next one's
    assert any(s % 7 != 0 for s in starts[1:-1]), starts
    L.check(L.lib().grt_set_sub_chunk(7 * spa * spa), "grt_set_sub_chunk")
    try:
        seq = sc.trace_gbuffer_sequence(cams)
        st = grt.supersample_sequence(seq, sc, [f.sel for f in frames], spa)
    finally:
        L.check(L.lib().grt_set_sub_chunk(0), "grt_set_sub_chunk")
    assert st["report"].n_launches == st["report"].n_traces == -(-total // 7) > 1
    assert st["rays"] == total * spa * spa
    assert_same_sets(seq, frames, "chunks of 7 pixels")


# ------------------------------------------------------------- 6. small pool -----------
def test_small_pool_retraces_the_chunk(grt, gpu):
    L = grt._lib
    case, ad, frames = per_frame(grt, "winding")
    spa = ad.samples_per_axis
    cams = case.cameras()
    layers = np.concatenate([np.diff(f.sub["layer_start"].astype(np.int64)) for f in frames])
    need = int(np.maximum(layers - L.GRT_MAX_HITS, 0).sum())
    print(f"winding: {[f.sel.size for f in frames]} selected pixels, {need} pool records at least")
    assert need > 64  # more pool records than the small pool has
    L.check(L.lib().grt_set_hit_pool_min(64))
    try:
        roomy = case.scene(0)
        seq = roomy.trace_gbuffer_sequence(cams)
        small = case.scene(0)  # a fresh device copy: a 64-record pool
        st = grt.supersample_sequence(seq, small, [f.sel for f in frames], spa)
    finally:
        L.check(L.lib().grt_set_hit_pool_min(1 << 20))
    rep = st["report"]
    assert rep.n_traces > rep.n_launches == 1
    assert st["rays"] > sum(f.sel.size for f in frames) * spa * spa  # the chunk was traced again, whole
    assert_same_sets(seq, frames, "winding, small pool")
    assert not any(np.any(b.sub_arrays()["status"] & L.FLAG_HIT_OVERFLOW) for b in seq)


# ------------------------------------------------------------- 7. refusals -------------
def test_refusals_of_the_stacked_fill(grt, gpu):
    L = grt._lib
    lib = L.lib()
    case, ad, frames = per_frame(grt, "schwarzschild")
    spa = ad.samples_per_axis
    sc, cams = case.scene(0), case.cameras()
    seq = sc.trace_gbuffer_sequence(cams)
    sels = [f.sel for f in frames]

    def refused(match, bufs, tracer=sc, lists=None, samples=spa):
        with pytest.raises(grt.GrtError, match=match) as e:
            grt.supersample_sequence(bufs, tracer, sels[:len(bufs)] if lists is None else lists, samples)
        assert _rc(e) == -errno.EINVAL, str(e.value)
        return str(e.value)

    refused("at least one buffer", [], lists=[])
    assert "frame 2" in refused("frame 0's too", [seq[0], seq[1], seq[0]])
    crop = sc.trace_gbuffer(0, 0, ROWS - 4, COLS)  # of the frame's camera, but not the whole frame
    assert "frame 1" in refused("pixels", [seq[0], crop])
    assert "frame 0" in refused("whole frame", [crop])
    refused("greater than zero", seq, samples=0)
    refused("more than 64", seq, samples=65)
    held = sc.trace_gbuffer_sequence(cams)
    grt.supersample_sequence([held[1]], sc, [sels[1][:3]], 2)
    msg = refused("samples_per_axis", [seq[0], held[1], seq[2]])
    assert "frame 1" in msg and "differs from the sub-sample set's 2" in msg
    msg = refused("outside", seq, lists=[sels[0], sels[1], np.array([3, N], np.uint32)])
    assert "frame 2" in msg and str(N) in msg
    # the tracer: its shape key, integration parameters and frame size, not its camera
    other = reference(grt, "euclidean")[0].scene(0)
    assert "frame 0" in refused("geometry", seq, tracer=other)
    d = case.desc(0)
    d.max_steps += 1
    fewer = grt.Scene(C.pointer(d), keepalive=d)
    assert "frame 0" in refused("max_steps", seq, tracer=fewer)
    d = case.desc(0)
    d.camera.rows += 1
    taller = grt.Scene(C.pointer(d), keepalive=d)
    assert "frame 0" in refused("camera.rows", seq, tracer=taller)
    # more than INT_MAX - 1 stacked sub-rays: an uploaded, empty 1024 x 1024 frame (nothing is
    # traced for it) whose every pixel is listed at 64 x 64 sub-rays, 2^32 of them
    big_info = seq[0].info
    big_info.rows = big_info.cols = big_info.camera.rows = big_info.camera.cols = 1024
    big_info.n_pixels, big_info.n_layers = 1 << 20, 0
    n_big = 1 << 20
    empty = {"status": np.zeros(n_big, np.uint8), "stop": np.zeros(n_big, np.uint8), "steps": np.zeros(n_big, np.uint32),
             "sky_u": np.zeros(n_big), "sky_v": np.zeros(n_big), "sky_redshift": np.zeros(n_big),
             "layer_start": np.zeros(n_big + 1, np.uint64), "object": np.zeros(0, np.uint8), "u": np.zeros(0),
             "v": np.zeros(0), "redshift": np.zeros(0), "radius": np.zeros(0)}
    big = grt.GBuffer.from_arrays(big_info, empty, device=0)
    d = case.desc(0)
    d.camera.rows = d.camera.cols = 1024
    wide = grt.Scene(C.pointer(d), keepalive=d)
    refused("INT_MAX - 1 stacked sub-rays", [big], tracer=wide, lists=[np.arange(n_big, dtype=np.uint32)], samples=64)
    assert big.sub_info.n_sub_pixels == 0
    # null lists and counts through the C ABI
    handles = (C.c_void_p * K)(*[b._h for b in seq])
    assert lib.grt_gbuffer_supersample_sequence(sc._s, K, handles, spa, None, None, None, None) == -errno.EINVAL
    # every refusal came before any trace: no buffer has a set
    assert all(b.sub_info.n_sub_pixels == 0 for b in seq)
    # afterwards the same call still gives the sets
    grt.supersample_sequence(seq, sc, sels, spa)
    assert_same_sets(seq, frames, "after the refusals")


# ------------------------------------------------------------- 2. the adaptive re-shade --
def shade(grt, bufs, scene, ad, **kw):
    return grt.shade_section_sequence(bufs, scene, adaptive=ad, failure_capacity=CAP, log_events=True, **kw)


def frame_of(shaded, k):
    """Frame k of shade_section_sequence in the shape assert_same_section compares."""
    return SimpleNamespace(xyza64=shaded["xyza64"][k], ray_class=shaded["class"][k], status=shaded["status"][k],
                           n_supersampled=int(shaded["n_supersampled"][k]),
                           n_failed_subsamples=shaded["n_failed_subsamples"][k],
                           failed_subsamples=shaded["failed_subsamples"][k],
                           subsample_events=shaded["subsample_events"][k], stop=shaded["stop"][k],
                           steps=shaded["steps"][k])


_WANTED = {}


def wanted(grt, name):
    """Each camera's render_section_ex alone, with the failure and event lists, once per scene."""
    if name not in _WANTED:
        case, ad, frames = per_frame(grt, name)
        _WANTED[name] = [section_reference(f.scene, ad) for f in frames]
    return _WANTED[name]


def assert_frames(got, wants, what, order=None):
    for k, j in enumerate(order if order is not None else range(len(wants))):
        assert_same_section(frame_of(got, k), wants[j], (what, k))


@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl", "kerr-schild", "euclidean"])
def test_adaptive_reshade_equals_the_frames(grt, gpu, name):
    case, ad, frames = per_frame(grt, name)
    wants = wanted(grt, name)
    sizes = np.array([f.sel.size for f in frames])
    assert all(w.n_supersampled == s for w, s in zip(wants, sizes))
    sc, cams = case.scene(0), case.cameras()
    ref = sc.render_sequence(cams, adaptive=ad, supersample=True)
    bufs = sc.trace_gbuffer_sequence(cams)
    got, rep = shade(grt, bufs, sc, ad, tracer=sc)  # cold: every selected pixel is traced, in one top-up
    assert_frames(got, wants, name)
    for k in range(K):
        assert np.array_equal(got["xyza64"][k].view(np.uint64), ref["xyza64"][k].view(np.uint64)), k
        assert np.array_equal(got["class"][k], ref["class"][k]) and np.array_equal(got["status"][k], ref["status"][k])
        assert int(got["n_supersampled"][k]) == int(ref["n_supersampled"][k])
        assert np.array_equal(got["failed_subsamples"][k], ref["failures"][k][ref["failures"][k][:, 2] != 0])
    assert (rep["n_frames"], rep["n_launches"]) == (K, 1)
    assert (rep["n_selected"], rep["n_held"], rep["n_traced"], rep["n_missing"]) == (sizes.sum(), 0, sizes.sum(), 0)
    assert np.array_equal(rep["per_frame"], np.stack([sizes, 0 * sizes, sizes, 0 * sizes], axis=1))
    assert rep["top_up"]["rays"] == sizes.sum() * ad.samples_per_axis ** 2
    assert rep["shade_ms"] > 0 and rep["trace_ms"] > 0 and rep["wall_ms"] > 0
    assert_same_sets(bufs, frames, name + ", the top-up's sets")
    warm, rep = shade(grt, bufs, sc, ad)  # no tracer needed: the sets hold the selection
    assert_frames(warm, wants, name + ", warm")
    assert (rep["n_selected"], rep["n_held"], rep["n_traced"], rep["n_missing"]) == (sizes.sum(), sizes.sum(), 0, 0)
    assert rep["top_up"]["rays"] == 0 and rep["trace_ms"] == 0.0
    assert np.array_equal(rep["per_frame"], np.stack([sizes, sizes, 0 * sizes, 0 * sizes], axis=1))
    assert_same_sets(bufs, frames, name + ", a warm call appends nothing")
    # the buffers in another order, and a stack of one
    order = [2, 0, 1]
    fresh = sc.trace_gbuffer_sequence(cams)
    got, rep = shade(grt, [fresh[k] for k in order], sc, ad, tracer=sc)
    assert_frames(got, wants, name + ", order 2 0 1", order)
    assert np.array_equal(rep["per_frame"][:, 2], sizes[order])
    assert_same_sets(fresh, frames, name + ", order 2 0 1")
    fresh = sc.trace_gbuffer_sequence(cams)
    got, rep = shade(grt, [fresh[1]], sc, ad, tracer=sc)
    assert_frames(got, wants, name + ", K = 1", [1])
    assert rep["n_traced"] == sizes[1] and fresh[0].sub_info.samples_per_axis == 0
    # the mask frame, and the 1-spp frame with the pass disabled
    painted, rep = grt.shade_section_sequence(bufs, sc, adaptive=ad, mask=MARK)
    for k in range(K):
        want = frames[k].scene.render_section_ex(adaptive=ad, sampling_mask_xyza=MARK)
        assert np.array_equal(painted["xyza64"][k].view(np.uint64), want.xyza64.view(np.uint64)), k
        assert np.array_equal(painted["class"][k], want.ray_class) and np.array_equal(painted["status"][k], want.status)
        assert int(painted["n_supersampled"][k]) == want.n_supersampled and painted["n_failed_subsamples"][k] == 0
    assert rep["n_selected"] == sizes.sum() and rep["n_traced"] == 0
    off = grt.default_adaptive()
    off.enabled = 0
    plain, rep = grt.shade_section_sequence(bufs, sc, adaptive=off)
    one_spp = grt.shade_sequence(bufs, sc)
    for key in ("xyza64", "class", "status", "stop", "steps"):
        assert plain[key].tobytes() == one_spp[key].tobytes(), key
    assert not plain["n_supersampled"].any() and rep["n_selected"] == 0
    # Scene.trace_gbuffer_sequence(adaptive=...): the traced scene's own selections
    both = sc.trace_gbuffer_sequence(cams, adaptive=ad)
    assert_same_sets(both, frames, name + ", trace_gbuffer_sequence(adaptive)")
    assert both.adaptive_report["n_traced"] == sizes.sum()


# ------------------------------------------------------------- 3. another appearance ---
@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl"])
def test_another_appearance_tops_up_stacked(grt, gpu, name):
    L = grt._lib
    a_case, b_case = Pair(grt, name), Pair(grt, name, alt=True)
    ad = adaptive(grt, 2)
    sa, sb, cams = a_case.scene(0), b_case.scene(0), a_case.cameras()
    # the per-frame route: A's buffer with A's selection, re-shaded under B
    singles, wants, missing = [], [], []
    for k in range(K):
        gb = a_case.scene(k).trace_gbuffer(adaptive=ad)
        sbk = b_case.scene(k)
        with pytest.raises(grt.GBufferMissing) as e:
            reshade(gb, sbk, ad)
        missing.append(e.value.report["n_missing"])
        wants.append(section_reference(sbk, ad))  # render_section_ex of B with camera k
        _, rep = reshade(gb, sbk, ad, tracer=sbk)
        assert rep["n_traced"] == missing[-1]
        singles.append(SimpleNamespace(sub=gb.sub_arrays(), sub_info=bytes(gb.sub_info)))
    assert all(w.n_supersampled >= 1 for w in wants) and sum(missing) >= 10, missing
    bufs = sa.trace_gbuffer_sequence(cams, adaptive=ad)
    before = [b.sub_arrays() for b in bufs]
    with pytest.raises(grt.GBufferMissing) as e:
        shade(grt, bufs, sb, ad)
    rep = e.value.report
    assert f"({-errno.ENODATA})" in str(e.value) and str(sum(missing)) in str(e.value)
    assert list(rep["per_frame"][:, 3]) == missing and rep["n_missing"] == sum(missing) and rep["n_traced"] == 0
    assert list(rep["per_frame"][:, 0]) == [w.n_supersampled for w in wants]
    for k in range(K):
        assert_same_set(bufs[k].sub_arrays(), before[k], ("a refused call leaves the sets alone", k))
    # the outputs of a refused call are untouched
    n = K * N
    x64, cls = np.full((n, 4), 7.25), np.full(n, 0x5a, np.uint8)
    out = L.FrameOut(None, L.dptr(x64), L.ptr(cls, C.c_uint8), None, None, None)
    handles = (C.c_void_p * K)(*[b._h for b in bufs])
    rc = L.lib().grt_gbuffer_shade_section_sequence(sb._s, K, handles, C.byref(ad), None, None, C.byref(out), None, None,
                                                    None, None)
    assert rc == -errno.ENODATA and np.all(x64 == 7.25) and np.all(cls == 0x5a)
    got, rep = shade(grt, bufs, sb, ad, tracer=sb)
    assert_frames(got, wants, name + " B, top-up")
    pf = rep["per_frame"]
    assert list(pf[:, 2]) == missing and not pf[:, 3].any() and np.array_equal(pf[:, 1] + pf[:, 2], pf[:, 0])
    assert rep["n_traced"] == sum(missing) and rep["top_up"]["rays"] == sum(missing) * 4
    assert_same_sets(bufs, singles, name + " B, the sets after the top-up")
    again, rep = shade(grt, bufs, sb, ad)
    assert_frames(again, wants, name + " B, warm")
    assert rep["n_traced"] == 0 and rep["n_held"] == rep["n_selected"]


# ------------------------------------------------------------- 4. failed sub-samples ---
def below_risco_at(grt, cart):
    """below_risco_scene (tests/test_gpu_gbuffer_adaptive.py) with the camera at `cart`."""
    b = grt.SceneBuilder(1, radius=2.0, horizon_epsilon=1e-4)
    b.integration(20000, 100.0, 0.01, 1e-7)
    pos = grt.cartesian_to_spherical((0.0,) + tuple(cart))
    b.camera(pos, grt.stationary_velocity(1, 2.0, 0.0, pos), math.pi / 4, 48, 48, 0.0, -3.142, 0.0)
    b.celestial(grt.Checker(0.0, 20.0, 20.0, (0, 255, 0), (0, 100, 0)))
    b.add_disc(3.0, 12.0, grt.BlackBody(1.0), temperature=5000.0)
    d = b.build()
    return grt.Scene(C.pointer(d), keepalive=(d, b)), d.camera


def test_failed_subsamples_per_frame(grt, gpu):
    ad = adaptive(grt, 4)
    scenes, cams = zip(*[below_risco_at(grt, c) for c in ((-16.0, 0.0, 3.5), (-15.7, 0.4, 3.3))])
    own, _ = below_risco_scene(grt)
    assert bytes(own.desc.camera) == bytes(cams[0])  # frame 0 is that file's frame
    wants = [section_reference(s, ad) for s in scenes]
    assert all(w.n_failed_subsamples > 0 for w in wants), [w.n_failed_subsamples for w in wants]
    assert not np.array_equal(wants[0].failed_subsamples, wants[1].failed_subsamples)
    bufs = scenes[0].trace_gbuffer_sequence(cams)
    got, rep = shade(grt, bufs, scenes[0], ad, tracer=scenes[0])
    assert_frames(got, wants, "below r_isco")  # the failure and event lists, stop and steps included
    warm, rep = shade(grt, bufs, scenes[0], ad)
    assert_frames(warm, wants, "below r_isco, warm")
    # a list too small for its frame: the count stays exact
    small, _ = grt.shade_section_sequence(bufs, scenes[0], adaptive=ad, failure_capacity=3)
    assert small["n_failed_subsamples"] == [w.n_failed_subsamples for w in wants]
    assert all(len(rows) == 3 for rows in small["failed_subsamples"])


# ------------------------------------------------------------- 5. chunks and groups ----
def test_chunks_and_groups_give_identical_frames(grt, gpu):
    L = grt._lib
    case, ad, frames = per_frame(grt, "schwarzschild")
    wants = wanted(grt, "schwarzschild")
    sc, cams = case.scene(0), case.cameras()
    try:
        for chunk in (7 * ad.samples_per_axis ** 2, 0):
            L.check(L.lib().grt_set_sub_chunk(chunk), "grt_set_sub_chunk")
            for group, launches in ((1, 3), (2, 2), (3, 1)):
                grt.set_sequence_group(group * N)
                bufs = sc.trace_gbuffer_sequence(cams)
                got, rep = shade(grt, bufs, sc, ad, tracer=sc)
                assert_frames(got, wants, (chunk, group, "cold"))
                assert rep["n_launches"] == launches and rep["n_traced"] == rep["n_selected"]
                assert_same_sets(bufs, frames, (chunk, group))
                warm, rep = shade(grt, bufs, sc, ad)  # groups of one frame, no tracer: counted first
                assert_frames(warm, wants, (chunk, group, "warm"))
                assert rep["n_launches"] == launches and rep["n_traced"] == 0
    finally:
        grt.set_sequence_group(0)
        L.check(L.lib().grt_set_sub_chunk(0), "grt_set_sub_chunk")


# ------------------------------------------------------------- 7. refusals -------------
def test_refusals_of_the_adaptive_reshade(grt, gpu):
    L = grt._lib
    case, ad, frames = per_frame(grt, "schwarzschild")
    wants = wanted(grt, "schwarzschild")
    sc, cams = case.scene(0), case.cameras()
    bufs = sc.trace_gbuffer_sequence(cams, adaptive=ad)

    def refused(match, buffers, **kw):
        with pytest.raises(grt.GrtError, match=match) as e:
            grt.shade_section_sequence(buffers, sc, **{"adaptive": ad, **kw})
        assert _rc(e) == -errno.EINVAL, str(e.value)
        return str(e.value)

    refused("at least one buffer", [])
    assert "frame 1" in refused("frame 0's too", [bufs[0], bufs[0]])
    crop = sc.trace_gbuffer(0, 0, ROWS - 4, COLS)
    assert "frame 2" in refused("pixels", [bufs[0], bufs[1], crop])
    assert "frame 0" in refused("whole frame", [crop])
    other = per_frame(grt, "euclidean")[0].scene(0).trace_gbuffer()  # another geometry: the shape key differs
    assert "frame 1" in refused("geometry", [bufs[0], other, bufs[2]])
    more = adaptive(grt, ad.samples_per_axis + 1)
    msg = refused("samples_per_axis", bufs, adaptive=more)
    assert "frame 0" in msg and str(ad.samples_per_axis) in msg
    zero = adaptive(grt, 0)
    refused("greater than zero", bufs, adaptive=zero)
    d = case.desc(0)
    d.max_steps += 1
    fewer = grt.Scene(C.pointer(d), keepalive=d)
    assert "frame 0" in refused("max_steps", bufs, tracer=fewer)
    # the mask paints: neither the sets' samples_per_axis nor a tracer is held to anything
    painted, _ = grt.shade_section_sequence(bufs, sc, adaptive=more, mask=MARK, tracer=fewer)
    assert int(painted["n_supersampled"].sum()) == sum(f.sel.size for f in frames)
    # xyza64 is required
    handles = (C.c_void_p * K)(*[b._h for b in bufs])
    f32 = np.zeros((K * N, 4), np.float32)
    out = L.FrameOut(L.ptr(f32, C.c_float), None, None, None, None, None)
    rc = L.lib().grt_gbuffer_shade_section_sequence(sc._s, K, handles, C.byref(ad), None, None, C.byref(out), None, None,
                                                    None, None)
    assert rc == -errno.EINVAL and "xyza64" in L.lib().grt_last_error().decode()
    # afterwards the same call still gives the frames, and the sets are the per-frame ones
    got, rep = shade(grt, bufs, sc, ad)
    assert_frames(got, wants, "after the refusals")
    assert rep["n_traced"] == 0
    assert_same_sets(bufs, frames, "after the refusals")


# ------------------------------------------------------------- 8. CLI ------------------
def test_cli_adaptive_stacked(grt, gpu, tmp_path):
    text = (SCENES / "schwarzschild.toml").read_text()  # adaptive sampling left enabled
    a_toml, b_toml = tmp_path / "a.toml", tmp_path / "b.toml"
    a_toml.write_text(text)
    swapped = text.replace("resources/disk.png", "resources/@").replace("resources/sphere.png", "resources/disk.png") \
                  .replace("resources/@", "resources/sphere.png").replace("temperature = 2000.0", "temperature = 3100.0")
    assert swapped != text and swapped.count("disk.png") == 1
    b_toml.write_text(swapped)
    path = tmp_path / "path.txt"
    path.write_text("# x,y,z,phi,theta,psi\n" + "".join(
        f"{c[0]},{c[1]},{c[2]},{phi},{theta},{psi}\n" for c, phi, theta, psi in CAMS_FRONT))
    common = ["--width", 64, "--height", 48, "--max-steps", 20000, "--resource-root", RESOURCES]
    cam_args = [["--camera-position", f"{c[0]},{c[1]},{c[2]}", f"--phi={phi}", f"--theta={theta}", f"--psi={psi}"]
                for c, phi, theta, psi in CAMS_FRONT]
    r = _grt(*common, "--config-file", a_toml, "gbuffer-sequence", "--camera-path", path, "--filename-pattern",
             tmp_path / "seq-%03d.grtg", "--first-index", 7, "--adaptive-stacked")
    assert r.stderr.count("INFO saved g-buffer to") == 3 and "one stacked top-up" in r.stderr
    sizes = []
    for k in range(3):
        _grt(*common, *cam_args[k], "--config-file", a_toml, "gbuffer", "--adaptive", "--filename",
             tmp_path / f"one-{k}.grtg")
        seq = tmp_path / f"seq-{7 + k:03d}.grtg"
        assert seq.read_bytes() == (tmp_path / f"one-{k}.grtg").read_bytes(), k
        sub = tmp_path / f"seq-{7 + k:03d}.grtg.sub"
        assert sub.read_bytes() == (tmp_path / f"one-{k}.grtg.sub").read_bytes(), k
        sizes.append(sub.stat().st_size)
    assert len({(tmp_path / f"seq-{7 + k:03d}.grtg.sub").read_bytes() for k in range(3)}) == 3
    r = _grt(*common, "--raw-out", tmp_path / "raw-%d.bin", "--config-file", b_toml, "reshade-sequence",
             "--gbuffer-pattern", tmp_path / "seq-%03d.grtg", "--frames", 3, "--first-index", 7, "--filename-pattern",
             tmp_path / "out-%03d.png", "--adaptive-stacked")
    assert r.stderr.count("INFO saved image to") == 3
    for k in range(3):
        assert f"frame {k}:" in r.stderr
    assert "selected" in r.stderr and "held" in r.stderr and "traced" in r.stderr
    for k in range(3):
        _grt(*common, *cam_args[k], "--raw-out", tmp_path / f"render-{k}.bin", "--config-file", b_toml, "render",
             "--filename", tmp_path / f"render-{k}.png")
        assert (tmp_path / f"out-{7 + k:03d}.png").read_bytes() == (tmp_path / f"render-{k}.png").read_bytes(), k
        raw = (tmp_path / f"render-{k}.bin").read_bytes()
        assert len(raw) == 64 * 48 * 32 and (tmp_path / f"raw-{7 + k}.bin").read_bytes() == raw, k
        assert (tmp_path / f"seq-{7 + k:03d}.grtg.sub").stat().st_size >= sizes[k]
    assert len({(tmp_path / f"out-{7 + k:03d}.png").read_bytes() for k in range(3)}) == 3
    # the same files without their sidecars: every selected pixel is traced in the stacked top-up,
    # the frames are the same and each set is written
    for k in range(3):
        (tmp_path / f"cold-{k}.grtg").write_bytes((tmp_path / f"seq-{7 + k:03d}.grtg").read_bytes())
    r = _grt(*common, "--config-file", b_toml, "reshade-sequence", "--gbuffer-pattern", tmp_path / "cold-%d.grtg",
             "--frames", 3, "--filename-pattern", tmp_path / "cold-%d.png", "--adaptive-stacked")
    assert r.stderr.count("INFO saved sub-sample set to") == 3 and ", 0 held," in r.stderr
    for k in range(3):
        assert (tmp_path / f"cold-{k}.png").read_bytes() == (tmp_path / f"render-{k}.png").read_bytes(), k
        assert (tmp_path / f"cold-{k}.grtg.sub").stat().st_size > 0
