"""Lapses for the sub-sample set, and the retarded-time adaptive frame (grt_gbuffer_supersample_lapse,
grt_gbuffer_shade_section_at_retarded; marker `gpu`).

Frames are the 24 x 20 ones of tests/test_gpu_gbuffer.py (the winding crop 12 x 12, the CLI's
64 x 48) and the cases those of tests/test_gpu_gbuffer_lapse.py: KBL / KS (the stock kerr-bl /
kerr-schild frames with a bitmap disc), S1 (the disc-only Schwarzschild scene) and the five
stock scenes.  Sets are 4 x 4 unless said otherwise.  Comparisons are on bits unless a bound
is named:

FLAT_BOUND  1e-9 max(1, |lapse|), the bound tests/test_gpu_gbuffer_lapse.py has for the
            Euclidean chart: its ODE is linear, and the window's lerp is exact up to rounding.
WALK_BOUND  relative, 10 x the largest difference measured on the MI355X against the oracle
            walk of the robust sub-rays, never more than 1e-6.  The measured difference is 0 on
            every chart (profiles/gbuffer/sub_lapse_check.json), as it is for the 1-spp rays:
            the device does the oracle's operations on the oracle's states, so the bound is
            bit equality.
"""
import ctypes as C
import errno
import math

import numpy as np
import pytest

from conftest import RESOURCES, SCENES
from test_gpu_gbuffer import COLS, ROWS, built_scene
from test_gpu_gbuffer_adaptive import CAP, MARK, adaptive, assert_same_section, assert_same_set
from test_gpu_gbuffer_lapse import FIVE, MAX_OUT, _bits, _flat_disc_scene, _numpy_cart, case, lapse_case
from test_gpu_gbuffer_orbit import _grt, _png

pytestmark = pytest.mark.gpu

FLAT_BOUND = 1e-9
WALK_BOUND = {"schwarzschild": 0.0, "kerr-schild": 0.0, "kerr-bl": 0.0}
TIMES = (0.0, 37.5, -12.25)
SPA = 4
EVERY_THIRD = np.arange(0, ROWS * COLS, 3, dtype=np.uint32)  # 160 pixels: more than one chunk of 7


def sub_layer_slices(a):
    """Per sub-ray the slice of its layers in the set's layer arrays."""
    ls = a["layer_start"].astype(np.int64)
    return ls[:-1], ls[1:]


def per_pixel(a, lapse, per):
    """{pixel: bytes of its block}: the per-ray arrays of its sub-rays and the layers of each, the
    lapse among them; layer_start enters as the sub-rays' layer counts."""
    lo, hi = sub_layer_slices(a)
    ray_keys = ("status", "stop", "steps", "sky_u", "sky_v", "sky_redshift")
    layer_keys = ("object", "u", "v", "redshift", "radius")
    assert set(ray_keys) | set(layer_keys) | {"layer_start", "sub_pixel"} == set(a)
    out = {}
    for b, p in enumerate(a["sub_pixel"]):
        r0, r1 = b * per, (b + 1) * per
        parts = [a[k][r0:r1].tobytes() for k in ray_keys] + [(hi[r0:r1] - lo[r0:r1]).tobytes()]
        parts += [a[k][lo[r0]:hi[r1 - 1]].tobytes() for k in layer_keys] + [lapse[lo[r0]:hi[r1 - 1]].tobytes()]
        out[int(p)] = b"".join(parts)
    return out


def check_lapse_shape(a, sub, lapse, what):
    """n_sub_layers entries, finite, <= 0, and strictly decreasing along each sub-ray: front to
    back the light left earlier and earlier."""
    assert lapse.shape == (int(sub.n_sub_layers),) == a["object"].shape, what
    assert np.all(np.isfinite(lapse)) and np.all(lapse <= 0.0), what
    lo, hi = sub_layer_slices(a)
    inner = np.ones(lapse.size, bool)
    inner[lo[lo < lapse.size]] = False
    assert np.all(np.diff(lapse)[inner[1:]] < 0.0), what


# ------------------------------------------------------------ 1. the same geometry ----
@pytest.mark.parametrize("name", FIVE)
def test_same_geometry(grt, gpu, name):
    L = grt._lib
    hs, sc, want, gb, gl = lapse_case(grt, name)
    plain, timed = sc.trace_gbuffer(), sc.trace_gbuffer(lapse=True)
    assert not plain.sub_has_lapse and not timed.sub_has_lapse and timed.sub_lapse() is None
    st_p = plain.supersample(sc, EVERY_THIRD, SPA)
    st_t = timed.supersample(sc, EVERY_THIRD, SPA, lapse=True)
    assert timed.sub_has_lapse and not plain.sub_has_lapse and plain.sub_lapse() is None
    assert st_t["rays"] == st_p["rays"] == EVERY_THIRD.size * SPA * SPA
    assert st_t["accepted_steps"] == st_p["accepted_steps"]
    sub, a = timed.sub_info, timed.sub_arrays()
    assert bytes(sub) == bytes(plain.sub_info) and sub._pad == 0, name
    assert_same_set(a, plain.sub_arrays(), name)  # sub_pixel and the twelve arrays
    lapse = timed.sub_lapse()
    assert lapse.size > 0
    check_lapse_shape(a, sub, lapse, name)
    # chunks of 7 pixels: the same set, the same lapses
    L.check(L.lib().grt_set_sub_chunk(7 * SPA * SPA))
    try:
        chunked = sc.trace_gbuffer(lapse=True)
        chunked.supersample(sc, EVERY_THIRD, SPA, lapse=True)
    finally:
        L.check(L.lib().grt_set_sub_chunk(0))
    assert_same_set(chunked.sub_arrays(), a, (name, "chunks of 7 pixels"))
    assert np.array_equal(_bits(chunked.sub_lapse()), _bits(lapse)), name
    # two calls against one: another block order, each pixel's block the same bytes
    twice = sc.trace_gbuffer(lapse=True)
    twice.supersample(sc, EVERY_THIRD[1::2], SPA, lapse=True)
    twice.supersample(sc, EVERY_THIRD, SPA, lapse=True)  # the held ones are skipped
    b = twice.sub_arrays()
    assert not np.array_equal(b["sub_pixel"], a["sub_pixel"]) and bytes(twice.sub_info) == bytes(sub)
    check_lapse_shape(b, twice.sub_info, twice.sub_lapse(), (name, "two calls"))
    assert per_pixel(b, twice.sub_lapse(), SPA * SPA) == per_pixel(a, lapse, SPA * SPA), (name, "two calls")
    for g in (plain, timed, chunked, twice):
        g.close()


def test_sub_rays_past_the_workspace_slots(grt, gpu):
    """Sub-rays with more layers than the 16 workspace slots take the later ones, and their
    times (pool_time), from the hit pool; a 64-record pool is grown and the chunk traced again."""
    from test_hit_pool import winding_scene

    L = grt._lib
    d = winding_scene(grt)
    rect = (38, 46, 12, 12)  # inside the heavy band of tests/test_hit_pool.py::test_full_pool
    pixels = np.arange(rect[2] * rect[3], dtype=np.uint32)
    roomy = built_scene(grt, d)
    plain, gb1 = roomy.trace_gbuffer(*rect), roomy.trace_gbuffer(*rect, lapse=True)
    plain.supersample(roomy, pixels, 2)
    st1 = gb1.supersample(roomy, pixels, 2, lapse=True)
    assert st1["rays"] == pixels.size * 4
    a, lapse = gb1.sub_arrays(), gb1.sub_lapse()
    assert_same_set(a, plain.sub_arrays(), "winding")
    layers = np.diff(a["layer_start"].astype(np.int64))
    assert np.maximum(layers - L.GRT_MAX_HITS, 0).sum() > 64  # more pool records than the small pool has
    check_lapse_shape(a, gb1.sub_info, lapse, "winding")  # pool records included
    L.check(L.lib().grt_set_hit_pool_min(64))
    try:
        small = built_scene(grt, d)  # a fresh device copy: a 64-record pool
        gb2 = roomy.trace_gbuffer(*rect, lapse=True)
        st2 = gb2.supersample(small, pixels, 2, lapse=True)
    finally:
        L.check(L.lib().grt_set_hit_pool_min(1 << 20))
    assert st2["rays"] > pixels.size * 4  # more than one trace
    assert_same_set(gb2.sub_arrays(), a, "small pool")
    assert np.array_equal(_bits(gb2.sub_lapse()), _bits(lapse))
    for g in (plain, gb1, gb2):
        g.close()


# ------------------------------------------------------------ 2. flat space, analytic ----
def test_flat_space_analytic(grt, gpu):
    """Euclidean chart, the oblique disc of tests/test_gpu_gbuffer_lapse.py: each sub-layer's
    lapse is minus the distance from the camera to the point rebuilt from its (u, v)."""
    L = grt._lib
    d = _flat_disc_scene(grt, L.GEOM_EUCLIDEAN)
    sc = built_scene(grt, d)
    gl = sc.trace_gbuffer(lapse=True)
    gl.supersample(sc, np.arange(ROWS * COLS, dtype=np.uint32), SPA, lapse=True)
    a, lapse, info = gl.sub_arrays(), gl.sub_lapse(), gl.info
    cam = np.array(d.camera.position[:])
    worst, n = 0.0, 0
    for k in range(lapse.size):
        o = info.shape.objects[int(a["object"][k])]
        assert o.kind == L.OBJ_DISC
        du, dv = a["u"][k] - 0.5, a["v"][k] - 0.5
        rho, phi = 2.0 * math.hypot(du, dv), math.atan2(dv, du)
        r = o.inner_radius + rho * (o.outer_radius - o.inner_radius)
        assert abs(r - a["radius"][k]) <= 1e-12 * max(1.0, r)  # the in-plane distance in the flat charts
        dist = math.dist(cam[1:], (r * math.cos(phi), r * math.sin(phi), 0.0))
        err = abs(lapse[k] + dist)
        assert err <= FLAT_BOUND * max(1.0, abs(lapse[k])), (k, lapse[k], dist)
        worst, n = max(worst, err), n + 1
    print(f"euclidean / oblique disc: {n} sub-layers, |lapse| up to {np.abs(lapse).max():.6g}, "
          f"max |lapse + distance| {worst:.3e}")
    assert n >= 100 * SPA * SPA // 2, n  # the 1-spp frame has about 150 disc layers
    gl.close()


# ---------------------------------------------------------- 3. oracle walk on sub-rays ----
# Pixels of the 24 x 20 frames, chosen with the oracle alone on the CPU (its 1-spp frame for the
# pixels with a layer, then its sub-rays at spa = 2 under the last-ulp probes of
# tests/test_gpu_parity.py): a spread of pixels whose four sub-rays are all robust and hit
# something, and a few with a sub-ray of two or three layers.  The oracle then counted 96, 100
# and 100 robust sub-rays with a layer (107, 129 and 132 layers).
WALK_SPA = 2
WALK = {
    "schwarzschild": ("S1", [155, 200, 222, 231, 243, 246, 249, 254, 256, 259, 267, 270, 273, 274, 276, 277, 278, 279,
                             282, 285, 294, 297, 300, 303]),
    "kerr-schild": ("kerr-schild", [0, 12, 24, 36, 48, 60, 72, 84, 96, 108, 120, 130, 131, 132, 133, 134, 144, 153, 156,
                                    168, 180, 192, 204, 216, 236]),
    "kerr-bl": ("kerr-bl", [0, 13, 26, 39, 52, 65, 78, 91, 104, 117, 130, 131, 132, 133, 134, 143, 153, 156, 169, 182,
                            195, 208, 221, 235, 258]),
}


def oracle_sub_layers(L, oracle, d, row, col, offset):
    """tests/test_gpu_gbuffer_lapse.py::oracle_layers for a sub-ray: the oracle's camera ray at
    the stratified offset, its trajectory, and per window the nearest of its chord tests."""
    steps, stop, status = oracle.integrate_ray(d, np.array(d.camera.position[:]),
                                               oracle.camera_ray(d, row, col, offset=offset), max_out=MAX_OUT)
    assert len(steps) < MAX_OUT
    if status != 0 or len(steps) < 2:
        return status, []
    x = steps[:, 1:5]
    c = _numpy_cart(L, d, x)
    cand = np.zeros(len(x) - 1, bool)
    for k in range(d.n_objects):
        o = d.objects[k]
        if o.kind == L.OBJ_DISC:
            f = c[:, 2]
            tol = 1e-6 * np.maximum(1.0, np.linalg.norm(c, axis=1))
        else:
            f = np.sum((c - np.array(o.center[:3])) ** 2, axis=1) - o.radius * o.radius
            tol = 1e-6 * max(1.0, o.radius * o.radius) * np.ones(len(c))
        cand |= (f[:-1] * f[1:] <= 0.0) | (np.abs(f[:-1]) <= tol[:-1]) | (np.abs(f[1:]) <= tol[1:])
    out = []
    for i in np.nonzero(cand)[0]:
        ca, cb = oracle.to_cartesian(d, x[i]), oracle.to_cartesian(d, x[i + 1])
        shortest, best = np.inf, None
        for k in range(d.n_objects):
            hit, pt, t = oracle.object_intersects(d, k, ca, cb)
            if not hit:
                continue
            dist = math.sqrt((pt[1] - ca[1]) ** 2 + (pt[2] - ca[2]) ** 2 + (pt[3] - ca[3]) ** 2)
            if dist < shortest:
                shortest, best = dist, (k, t)
        if best is not None:
            k, t = best
            out.append((k, x[i, 0] + t * (x[i + 1, 0] - x[i, 0]) - x[0, 0]))
    return status, out


def walk_scene(grt, frame):
    if frame == "S1":
        c = case(grt, "S1")
        return c["desc"], c["tracer"]
    hs, sc, want, gb, gl = lapse_case(grt, frame)
    return hs.desc, sc


@pytest.mark.parametrize("chart", ["schwarzschild", "kerr-schild", "kerr-bl"])
def test_oracle_walk_on_sub_rays(grt, oracle, gpu, chart):
    """Measured on an MI355X (profiles/gbuffer/sub_lapse_check.json): the
    largest relative difference over the robust sub-rays is 0 on each chart, so the bound (10 x
    the measured value, at most 1e-6) is bit equality."""
    from test_gpu_parity import check_parity, oracle_pair

    L = grt._lib
    frame, pixels = WALK[chart]
    d, sc = walk_scene(grt, frame)
    per = WALK_SPA * WALK_SPA
    pix, dx, dy = [], [], []
    for p in pixels:
        row, col = divmod(p, COLS)
        for s in range(per):
            ox, oy = oracle.stratified_offset(row, col, s // WALK_SPA, s % WALK_SPA, WALK_SPA)
            pix.append(p), dx.append(ox), dy.append(oy)
    offsets = (np.asarray(pix, np.uint32), np.asarray(dx), np.asarray(dy))
    ref, probes = oracle_pair(oracle, d, 0, 0, ROWS, COLS, offsets=offsets)
    robust = check_parity(sc.render_pixels(offsets=offsets), ref, probes, max_sensitive=0.1)
    gl = sc.trace_gbuffer(lapse=True)
    gl.supersample(sc, pixels, WALK_SPA, lapse=True)
    a, lapse = gl.sub_arrays(), gl.sub_lapse()
    assert list(a["sub_pixel"]) == pixels  # ascending: block b is pixels[b], sub-ray b * per + s
    lo, hi = sub_layer_slices(a)
    worst, n_rays, n_layers = 0.0, 0, 0
    for j in np.flatnonzero(robust & (ref["status"] == 0) & (ref["hits"] > 0)):
        row, col = divmod(int(pix[j]), COLS)
        status, layers = oracle_sub_layers(L, oracle, d, row, col, (dx[j], dy[j]))
        assert status == 0 and len(layers) == ref["hits"][j], (chart, j, len(layers), ref["hits"][j])
        assert a["status"][j] == 0
        got_obj, got = a["object"][lo[j]:hi[j]], lapse[lo[j]:hi[j]]
        # a robust sub-ray whose layer count or objects differ from the set's is a failure
        assert list(got_obj) == [k for k, _ in layers], (chart, j, list(got_obj), layers)
        for g, (_, r) in zip(got, layers):
            worst, n_layers = max(worst, abs(g - r) / max(abs(r), 1e-300)), n_layers + 1
        n_rays += 1
    print(f"{chart} / {frame}: {n_rays} robust sub-rays with a layer of {len(pix)}, {n_layers} layers, lapse "
          f"{lapse.min():.4f} .. {lapse.max():.4f}, largest relative difference {worst:.3e}")
    assert n_rays >= 64, n_rays
    assert worst <= min(WALK_BOUND[chart], 1e-6), (chart, worst)
    gl.close()


# ------------------------------------------------------ 4. the retarded adaptive frame ----
def config(grt, c):
    """The stock 4 x 4 [adaptive_sampling] of KBL / KS; S1 (a built scene: it has none) at 4 x 4."""
    ad = getattr(c["app"], "adaptive", None)
    if ad is None or not ad.enabled:
        ad = adaptive(grt, SPA)
    assert ad.enabled and ad.samples_per_axis == SPA
    return ad


def retarded_arrays(grt, info, arrays, lapse, t):
    """The arrays (a buffer's or a set's) with (u, v) through the host's retarded rule at t."""
    out = dict(arrays)
    out["u"], out["v"] = grt.gbuffer_orbit_uv_retarded(info.shape, arrays["object"], arrays["u"], arrays["v"],
                                                       arrays["radius"], lapse, t)
    return out


def host_rule_buffer(grt, c, gb, t):
    """A second buffer whose arrays and set arrays went through gbuffer_orbit_uv_retarded on the
    host, with the buffer's lapse and the set's: today's static shade_section of it is the
    reference of the retarded adaptive frame at t."""
    info = c["info"]
    up = grt.GBuffer.from_arrays(info, retarded_arrays(grt, info, c["arrays"], c["lapse"], t))
    up.set_sub_arrays(gb.sub_info, retarded_arrays(grt, info, gb.sub_arrays(), gb.sub_lapse(), t))
    return up


@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("name", ["KBL", "KS", "S1"])
def test_retarded_adaptive_frame(grt, gpu, name, t):
    c = case(grt, name)
    tracer, app = c["tracer"], c["app"]
    ad = config(grt, c)
    kw = dict(adaptive=ad, failure_capacity=CAP, log_events=True)
    gb = tracer.trace_gbuffer(lapse=True)
    assert gb.sub_info.n_sub_pixels == 0 and not gb.sub_has_lapse
    frame, rep = gb.shade_section(app, tracer=tracer, time=t, retarded=True, **kw)
    assert frame.n_supersampled > 21
    assert rep["n_traced"] == rep["n_selected"] == frame.n_supersampled and rep["n_missing"] == 0
    assert gb.sub_has_lapse and gb.sub_lapse().shape == (int(gb.sub_info.n_sub_layers),)  # the top-up filled it timed
    up = host_rule_buffer(grt, c, gb, t)
    static, rep_s = up.shade_section(app, **kw)
    assert_same_section(frame, static, (name, t, "host rule, static path"))  # frame, class, status, count, failures
    assert rep_s["n_traced"] == 0 and rep_s["n_held"] == frame.n_supersampled
    painted, _ = gb.shade_section(app, sampling_mask_xyza=MARK, time=t, retarded=True, **kw)
    painted_s, _ = up.shade_section(app, sampling_mask_xyza=MARK, **kw)
    assert_same_section(painted, painted_s, (name, t, "mask"))
    assert np.all(painted.xyza64 == MARK, axis=1).sum() == frame.n_supersampled
    # the repeat traces nothing
    held = gb.sub_arrays()
    again, rep2 = gb.shade_section(app, tracer=tracer, time=t, retarded=True, **kw)
    assert_same_section(again, frame, (name, t, "repeat"))
    assert rep2["n_traced"] == 0 and rep2["n_missing"] == 0 and rep2["n_held"] == frame.n_supersampled
    assert_same_set(gb.sub_arrays(), held, "a repeat appends nothing")
    # and it is not the fast-light adaptive frame
    fast, _ = gb.shade_section(app, tracer=tracer, time=t, **kw)
    moved = np.any(fast.xyza64.view(np.uint64) != frame.xyza64.view(np.uint64), axis=1)
    print(f"{name}, t = {t}: {frame.n_supersampled} supersampled, {moved.sum()} pixels differ from the fast-light frame")
    assert moved.sum() >= 1
    gb.close()
    up.close()


# ------------------------------------------------------------ 5. ties to what exists ----
@pytest.mark.parametrize("name", ["KBL", "KS", "S1"])
def test_uploaded_lapses(grt, gpu, name):
    """Zero lapses on the buffer and on the set: the fast-light adaptive frame at t.  A constant
    c on both: the fast-light frame at the double t + c."""
    c = case(grt, name)
    tracer, app = c["tracer"], c["app"]
    ad = config(grt, c)
    kw = dict(adaptive=ad, failure_capacity=CAP, log_events=True)
    shift = -41.625
    for t in TIMES:
        for value, at in ((0.0, t), (shift, t + shift)):
            gb = tracer.trace_gbuffer()
            want, _ = gb.shade_section(app, tracer=tracer, time=at, **kw)
            assert not gb.sub_has_lapse
            gb.set_lapse(np.full(c["lapse"].size, value))
            gb.set_sub_lapse(np.full(int(gb.sub_info.n_sub_layers), value))
            assert gb.sub_has_lapse
            got, rep = gb.shade_section(app, time=t, retarded=True, **kw)  # no tracer: the set holds the selection
            assert_same_section(got, want, (name, t, value))
            assert rep["n_traced"] == 0
            gb.close()


@pytest.mark.parametrize("name", ["kerr-bl", "kerr-schild", "euclidean", "euclidean-spherical"])
def test_static_appearances_and_flat_charts_do_not_move(grt, gpu, name):
    """A BlackBody disc's colour does not depend on (u, v); the flat charts' emitter is at rest."""
    hs, sc, want, gb, gl = lapse_case(grt, name)
    kw = dict(adaptive=hs.adaptive, failure_capacity=CAP, log_events=True)
    assert hs.adaptive.enabled
    ref = sc.trace_gbuffer()
    static, _ = ref.shade_section(sc, tracer=sc, **kw)
    timed = sc.trace_gbuffer(lapse=True)
    for t in TIMES + (1e4,):
        got, _ = timed.shade_section(sc, tracer=sc, time=t, retarded=True, **kw)
        assert_same_section(got, static, (name, t))
    assert timed.sub_has_lapse
    assert_same_set(timed.sub_arrays(), ref.sub_arrays(), name)
    ref.close()
    timed.close()


# ------------------------------------------------------------- 6. a set's kind ----
def _rc(exc):
    return int(str(exc.value).split("(")[1].split(")")[0])


def test_kind_rules(grt, gpu):
    L = grt._lib
    c = case(grt, "KBL")
    tracer, app = c["tracer"], c["app"]
    ad = config(grt, c)
    kw = dict(adaptive=ad, failure_capacity=CAP)
    t = 37.5
    # no buffer lapse: -ENODATA, whatever the set
    plain = tracer.trace_gbuffer()
    with pytest.raises(grt.GrtError, match="holds no lapse") as e:
        plain.shade_section(app, tracer=tracer, time=t, retarded=True, **kw)
    assert _rc(e) == -errno.ENODATA and plain.sub_info.n_sub_pixels == 0
    with pytest.raises(ValueError):
        plain.shade_section(app, tracer=tracer, retarded=True, **kw)
    # a non-empty untimed set: -ENODATA with both counts, and supersample(lapse=True) is -EINVAL
    untimed = tracer.trace_gbuffer(lapse=True)
    untimed.shade_section(app, tracer=tracer, time=t, **kw)
    sub = untimed.sub_info
    assert sub.n_sub_pixels > 21 and not untimed.sub_has_lapse
    with pytest.raises(grt.GrtError, match="untimed") as e:
        untimed.shade_section(app, tracer=tracer, time=t, retarded=True, **kw)
    assert _rc(e) == -errno.ENODATA
    assert f"{sub.n_sub_pixels} pixels" in str(e.value) and f"{sub.n_sub_layers} layers" in str(e.value)
    with pytest.raises(grt.GrtError, match=f"{sub.n_sub_pixels} pixels") as e:
        untimed.supersample(tracer, [0, 1, 2], SPA, lapse=True)
    assert _rc(e) == -errno.EINVAL
    assert bytes(untimed.sub_info) == bytes(sub) and not untimed.sub_has_lapse
    # the mask path and enabled == 0 need the buffer's lapse only
    untimed.shade_section(app, sampling_mask_xyza=MARK, time=t, retarded=True, **kw)
    off = adaptive(grt, SPA)
    off.enabled = 0
    one_spp, _ = untimed.shade_section(app, adaptive=off, time=t, retarded=True)
    want = untimed.shade_orbit(app, [t], retarded=True)["xyza64"][0]
    assert np.array_equal(one_spp.xyza64.view(np.uint64), want.view(np.uint64))
    # clear_sub, then a timed refill
    untimed.clear_sub()
    assert untimed.sub_info.samples_per_axis == 0 and untimed.sub_info.n_sub_pixels == 0 and untimed.sub_lapse() is None
    # without a tracer on the empty set: -ENODATA with n_missing
    with pytest.raises(grt.GBufferMissing) as e:
        untimed.shade_section(app, time=t, retarded=True, **kw)
    assert f"({-errno.ENODATA})" in str(e.value) and e.value.report["n_missing"] > 21
    assert untimed.sub_info.n_sub_pixels == 0
    frame, rep = untimed.shade_section(app, tracer=tracer, time=t, retarded=True, **kw)
    assert untimed.sub_has_lapse and rep["n_traced"] == frame.n_supersampled
    timed = untimed
    # a static top-up on a timed set keeps it timed, its lapse as long as its layers
    n0, lapse0 = int(timed.sub_info.n_sub_pixels), timed.sub_lapse()
    _, rep = timed.shade_section(app, tracer=tracer, **kw)
    assert rep["n_traced"] > 0 and timed.sub_has_lapse
    sub = timed.sub_info
    lapse = timed.sub_lapse()
    assert sub.n_sub_pixels == n0 + rep["n_traced"] and lapse.shape == (int(sub.n_sub_layers),)
    assert np.array_equal(_bits(lapse[:lapse0.size]), _bits(lapse0))
    check_lapse_shape(timed.sub_arrays(), sub, lapse, "static top-up of a timed set")
    # grt_gbuffer_supersample too: the appended block's lapse is the one a timed fill records
    rest = np.setdiff1d(np.arange(ROWS * COLS, dtype=np.uint32), timed.sub_arrays()["sub_pixel"])[:9]
    timed.supersample(tracer, rest, SPA)
    fresh = tracer.trace_gbuffer(lapse=True)
    fresh.supersample(tracer, rest, SPA, lapse=True)
    both = per_pixel(timed.sub_arrays(), timed.sub_lapse(), SPA * SPA)
    assert timed.sub_has_lapse
    for p, block in per_pixel(fresh.sub_arrays(), fresh.sub_lapse(), SPA * SPA).items():
        assert both[p] == block, p
    # the stacked calls refuse a timed buffer and name the frame
    other = tracer.trace_gbuffer()
    px = [np.array([5, 6], np.uint32)] * 2
    with pytest.raises(grt.GrtError, match=r"frame 1: .*timed") as e:
        grt.scene.supersample_sequence([other, timed], tracer, px, SPA)
    assert _rc(e) == -errno.EINVAL
    with pytest.raises(grt.GrtError, match=r"frame 0: .*timed") as e:
        grt.scene.shade_section_sequence([timed, other], app, adaptive=ad, tracer=tracer)
    assert _rc(e) == -errno.EINVAL
    assert other.sub_info.n_sub_pixels == 0
    # uploads: wrong counts and non-finite entries are refused and change nothing
    n = int(timed.sub_info.n_sub_layers)
    held = timed.sub_lapse()
    for bad in (np.zeros(n - 1), np.zeros(n + 1)):
        with pytest.raises(grt.GrtError, match="entries") as e:
            timed.set_sub_lapse(bad)
        assert _rc(e) == -errno.EINVAL
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = held.copy()
        x[n // 2] = bad
        with pytest.raises(grt.GrtError, match="not finite") as e:
            timed.set_sub_lapse(x)
        assert _rc(e) == -errno.EINVAL
    assert np.array_equal(_bits(timed.sub_lapse()), _bits(held))
    with pytest.raises(grt.GrtError, match="holds no set") as e:
        other.set_sub_lapse(np.zeros(0))
    assert _rc(e) == -errno.EINVAL
    assert L.lib().grt_gbuffer_sub_has_lapse(None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_sub_clear(None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_sub_lapse_download(None, None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_sub_lapse_download(other._h, L.dptr(np.zeros(1))) == -errno.ENODATA
    for g in (plain, timed, fresh, other):
        g.close()


# ----------------------------------------------------------------- 7. round trips ----
def test_round_trips(grt, gpu, tmp_path):
    c = case(grt, "KS")
    tracer, app = c["tracer"], c["app"]
    ad = config(grt, c)
    kw = dict(adaptive=ad, failure_capacity=CAP, log_events=True)
    t = -12.25
    gb = tracer.trace_gbuffer(lapse=True)
    want, _ = gb.shade_section(app, tracer=tracer, time=t, retarded=True, **kw)
    sub, arrays, lapse = gb.sub_info, gb.sub_arrays(), gb.sub_lapse()
    # sub_lapse -> set_sub_lapse: an uploaded set is untimed until it is given its lapse
    up = grt.GBuffer.from_arrays(c["info"], c["arrays"])
    up.set_lapse(c["lapse"])
    up.set_sub_arrays(sub, arrays)
    assert not up.sub_has_lapse and up.sub_lapse() is None
    up.set_sub_lapse(lapse)
    assert up.sub_has_lapse and np.array_equal(_bits(up.sub_lapse()), _bits(lapse))
    got, rep = up.shade_section(app, time=t, retarded=True, **kw)
    assert_same_section(got, want, "uploaded")
    assert rep["n_traced"] == 0
    up.set_sub_lapse(lapse - 1.0)  # it replaces a held lapse
    assert np.array_equal(_bits(up.sub_lapse()), _bits(lapse - 1.0))
    up.set_sub_arrays(sub, arrays)  # and a new set is untimed again
    assert not up.sub_has_lapse
    # save_sub -> load_sub, with and without the lapse's sidecar
    path = tmp_path / "a.grtg.sub"
    gb.save_sub(path)
    side = tmp_path / "a.grtg.sub.lapse"
    assert side.exists() and side.read_bytes()[:8] == b"GRTGSLP\0"
    assert side.stat().st_size == 16 + C.sizeof(grt._lib.GBufferInfo) + C.sizeof(grt._lib.GBufferSubInfo) + 8 * lapse.size
    plain = tracer.trace_gbuffer()
    plain.supersample(tracer, arrays["sub_pixel"], SPA)
    plain.save_sub(tmp_path / "plain.sub")
    assert not (tmp_path / "plain.sub.lapse").exists()
    assert (tmp_path / "plain.sub").read_bytes() == path.read_bytes()  # .sub keeps its bytes
    back = grt.GBuffer.from_arrays(c["info"], c["arrays"])
    back.set_lapse(c["lapse"])
    back.load_sub(path)
    assert back.sub_has_lapse and bytes(back.sub_info) == bytes(sub)
    assert_same_set(back.sub_arrays(), arrays, "loaded")
    assert np.array_equal(_bits(back.sub_lapse()), _bits(lapse))
    got, rep = back.shade_section(app, time=t, retarded=True, **kw)
    assert_same_section(got, want, "loaded")
    back.load_sub(tmp_path / "plain.sub")
    assert not back.sub_has_lapse
    # a sidecar left stale by a set that grew is refused, and the buffer keeps its set
    rest = np.setdiff1d(np.arange(ROWS * COLS, dtype=np.uint32), arrays["sub_pixel"])[:5]
    gb.supersample(tracer, rest, SPA)
    old = side.read_bytes()
    gb.save_sub(path)
    assert side.read_bytes() != old
    side.write_bytes(old)
    with pytest.raises(grt.GrtError, match="another sub-sample set"):
        back.load_sub(path)
    assert bytes(back.sub_info) == bytes(sub)
    for g in (gb, up, plain, back):
        g.close()


# ------------------------------------------------------------------------ 8. CLI ----
def test_cli(grt, gpu, tmp_path):
    """`grt gbuffer --adaptive --lapse` writes the bytes each flag writes alone, plus the set's
    lapse; `grt reshade-orbit --adaptive-retarded` writes shade_section(retarded=True)'s frames."""
    w, h = 64, 48
    on = tmp_path / "on.toml"
    on.write_text((SCENES / "schwarzschild.toml").read_text())
    cam = dict(camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=100000)
    common = ["--width", w, "--height", h, "--camera-position", "-16,0,3.5", "--theta", "-3.142", "--max-steps", 100000,
              "--resource-root", RESOURCES, "--config-file", on]
    size = ["--width", w, "--height", h, "--resource-root", RESOURCES, "--config-file", on]
    both, ad_only, lapse_only = tmp_path / "both.grtg", tmp_path / "ad.grtg", tmp_path / "lapse.grtg"
    r = _grt(*common, "gbuffer", "--adaptive", "--lapse", "--filename", both)
    assert "saved sub-sample lapse to" in r.stderr
    _grt(*common, "gbuffer", "--adaptive", "--filename", ad_only)
    _grt(*common, "gbuffer", "--lapse", "--filename", lapse_only)
    assert both.read_bytes() == ad_only.read_bytes() == lapse_only.read_bytes()
    assert (tmp_path / "both.grtg.lapse").read_bytes() == (tmp_path / "lapse.grtg.lapse").read_bytes()
    assert (tmp_path / "both.grtg.sub").read_bytes() == (tmp_path / "ad.grtg.sub").read_bytes()
    assert (tmp_path / "both.grtg.sub.lapse").exists()
    assert not (tmp_path / "ad.grtg.sub.lapse").exists() and not (tmp_path / "lapse.grtg.sub").exists()
    # the same files from Python
    hs = grt.HostScene(str(on), grt.GlobalOpts(width=w, height=h, **cam), str(RESOURCES))
    sc = grt.Scene(hs.desc_ptr(), keepalive=hs, adaptive=hs.adaptive)
    assert hs.adaptive.enabled
    gl = sc.trace_gbuffer(adaptive=hs.adaptive, lapse=True)
    assert gl.sub_has_lapse and gl.sub_info.n_sub_pixels > 21
    gl.save_sub(tmp_path / "py.sub")
    assert (tmp_path / "py.sub").read_bytes() == (tmp_path / "both.grtg.sub").read_bytes()
    assert (tmp_path / "py.sub.lapse").read_bytes() == (tmp_path / "both.grtg.sub.lapse").read_bytes()
    # reshade-orbit --adaptive-retarded against shade_section(retarded=True), frame by frame
    before = (tmp_path / "both.grtg.sub").read_bytes()
    r = _grt(*size, "reshade-orbit", "--gbuffer", both, "--adaptive-retarded", "--times", "1,36.5,2", "--filename-pattern",
             tmp_path / "f-%04d.png", "--raw-out-pattern", tmp_path / "f-%04d.raw")
    grew = r.stderr.count("saved sub-sample set")
    assert grew <= 1
    loaded = grt.GBuffer.load(both)
    loaded.load_sub(tmp_path / "py.sub")
    assert loaded.sub_has_lapse
    for k, t in enumerate((1.0, 37.5)):
        want, _ = loaded.shade_section(sc, tracer=sc, time=t, retarded=True)
        assert (tmp_path / f"f-{k:04d}.raw").read_bytes() == want.xyza64.tobytes(), k
        assert (tmp_path / f"f-{k:04d}.png").read_bytes() == _png(grt, tmp_path / f"want-{k}.png", want.xyza64, w, h), k
    # the set the CLI left is the one these calls left: rewritten once when it grew, still timed
    loaded.save_sub(tmp_path / "after.sub")
    assert (tmp_path / "both.grtg.sub").read_bytes() == (tmp_path / "after.sub").read_bytes()
    assert (tmp_path / "both.grtg.sub.lapse").read_bytes() == (tmp_path / "after.sub.lapse").read_bytes()
    assert grew == (1 if (tmp_path / "after.sub").read_bytes() != before else 0)
    # `reshade --adaptive` on a timed set keeps it timed: both sidecars still fit each other
    _grt(*size, "reshade", "--gbuffer", both, "--adaptive", "--filename", tmp_path / "static.png")
    check = grt.GBuffer.load(both)
    check.load_sub(tmp_path / "both.grtg.sub")
    assert check.sub_has_lapse
    for g in (gl, loaded, check):
        g.close()
