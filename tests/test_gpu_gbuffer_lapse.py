"""Each layer's light-travel time in a geometry buffer, and the retarded-time orbital motion
(grt_gbuffer_trace_lapse, grt_gbuffer_shade_times_retarded; marker `gpu`).

Frames are the 24 x 20 ones of tests/test_gpu_gbuffer.py (the winding frame 96 x 96, the CLI's
64 x 48), the buffers of item 4 those of tests/test_gpu_gbuffer_orbit.py traced again with
their lapse.  Comparisons are on bits unless a bound is named:

FLAT_BOUND       1e-9 max(1, |lapse|): the Euclidean chart's ODE is linear (dt/dlambda = -1,
                 a constant spatial momentum of unit length), and the window's lerp is exact
                 up to rounding over the few dozen steps of a ray.
SPHERICAL_BOUND  10 x the largest difference measured on the euclidean-spherical frames
                 against the same analytic distance (DESIGN section 18 has the figure): there
                 the RKF error of the curvilinear chart enters.
WALK_BOUND       relative, 10 x the largest difference measured on the robust pixels against
                 the oracle walk, never more than 1e-6 (at |lapse| ~ 50 and Omega ~ 0.14 a 1e-6
                 error moves the lookup by under 1e-5 rad, below the project's 1e-4).  The
                 measured difference is 0 on every chart: the device does the oracle's
                 operations on the oracle's states, so the bound is bit equality.
"""
import ctypes as C
import errno
import math
import subprocess

import numpy as np
import pytest

from conftest import RESOURCES, SCENES
from test_gpu_gbuffer import COLS, GRT, ROWS, STOCK, assert_same_frame, built_scene, stock, stock_case
from test_gpu_gbuffer_orbit import TIMES as ORBIT_TIMES
from test_gpu_gbuffer_orbit import Frame, _grt, _png, _stock_with_bitmap_disc, disc_pixels, s1_desc

pytestmark = pytest.mark.gpu

FLAT_BOUND = 1e-9
SPHERICAL_BOUND = 1.4e-5  # absolute: 10 x the measured 1.35e-6 (test_flat_space_analytic)
WALK_BOUND = {"schwarzschild": 0.0, "kerr-schild": 0.0, "kerr-bl": 0.0}
TIMES = (0.0, 1.0, 37.5, -12.25)
T_MOVED = TIMES.index(37.5)
FIVE = ("euclidean", "euclidean-spherical", "schwarzschild", "kerr-schild", "kerr-bl")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def assert_same_buffer(a, b, what=""):
    """info and the twelve arrays, byte for byte."""
    assert bytes(a.info) == bytes(b.info), (what, "info")
    x, y = a.arrays(), b.arrays()
    assert set(x) == set(y) and len(x) == 12, what
    for k in x:
        assert x[k].tobytes() == y[k].tobytes(), (what, k)
    return x


_LAPSE = {}


def lapse_case(grt, name):
    """The stock case of tests/test_gpu_gbuffer.py with its buffer traced again with a lapse."""
    if name not in _LAPSE:
        hs, sc, want, gb = stock_case(grt, name)
        _LAPSE[name] = (hs, sc, want, gb, sc.trace_gbuffer(lapse=True))
    return _LAPSE[name]


# ------------------------------------------------------------ 1. the same geometry ----
@pytest.mark.parametrize("name", FIVE)
def test_same_geometry(grt, gpu, name):
    hs, sc, want, gb, gl = lapse_case(grt, name)
    a = assert_same_buffer(gl, gb, name)
    assert gb.lapse() is None
    lapse = gl.lapse()
    assert lapse.shape == (int(gl.info.n_layers),) and lapse.size > 0
    assert np.all(np.isfinite(lapse)) and np.all(lapse <= 0.0), (name, lapse.max())
    assert gl.stats["rays"] == ROWS * COLS and gl.stats["accepted_steps"] == gb.stats["accepted_steps"]
    assert_same_frame(gl.shade(sc), want, name)
    # front to back along a ray the light left earlier and earlier
    first = a["layer_start"][:-1].astype(np.int64)
    inner = np.ones(lapse.size, bool)
    inner[first[first < lapse.size]] = False
    assert np.all(np.diff(lapse)[inner[1:]] <= 0.0), name
    rect = (3, 5, 9, 11)  # a sub-rectangle off the tile grid
    sub, sub_l = sc.trace_gbuffer(*rect), sc.trace_gbuffer(*rect, lapse=True)
    assert_same_buffer(sub_l, sub, name + " sub-rectangle")
    pick = (np.arange(rect[0], rect[0] + rect[2])[:, None] * COLS + np.arange(rect[1], rect[1] + rect[3])[None, :]).ravel()
    ls = a["layer_start"].astype(np.int64)
    want_lapse = np.concatenate([lapse[ls[p]:ls[p + 1]] for p in pick] + [np.zeros(0)])
    assert np.array_equal(_bits(sub_l.lapse()), _bits(want_lapse)), name
    sub.close()
    sub_l.close()


@pytest.mark.parametrize("disc", [False, True], ids=["spheres", "disc"])
def test_layers_past_the_workspace_slots(grt, gpu, disc):
    """Layers past the 16 workspace slots come from the hit pool, with their times; a 64-record
    pool is grown and the rectangle traced again, as grt_gbuffer_trace does."""
    from test_hit_pool import N, winding_scene

    L = grt._lib
    d = winding_scene(grt, disc=disc)
    sc = built_scene(grt, d)
    gb, gl = sc.trace_gbuffer(), sc.trace_gbuffer(lapse=True)
    a = assert_same_buffer(gl, gb, "winding")
    layers = np.diff(a["layer_start"].astype(np.int64))
    assert (layers > L.GRT_MAX_HITS).sum() >= 300 and layers.max() > 80
    lapse = gl.lapse()
    assert lapse.shape == (int(layers.sum()),) and np.all(np.isfinite(lapse)) and np.all(lapse <= 0.0)
    first = a["layer_start"][:-1].astype(np.int64)
    inner = np.ones(lapse.size, bool)
    inner[first[first < lapse.size]] = False
    assert np.all(np.diff(lapse)[inner[1:]] < 0.0)  # pool records included: later windows, earlier light
    L.check(L.lib().grt_set_hit_pool_min(64))
    try:
        small = built_scene(grt, d)  # a fresh device copy: a 64-record pool
        gl2 = small.trace_gbuffer(lapse=True)
        assert gl2.stats["rays"] > N * N  # more than one trace
        assert_same_buffer(gl2, gb, "winding, small pool")
        assert np.array_equal(_bits(gl2.lapse()), _bits(lapse))
    finally:
        L.check(L.lib().grt_set_hit_pool_min(1 << 20))


# ------------------------------------------------------------ 2. flat space, analytic ----
def _flat_disc_scene(grt, geometry):
    """A disc seen obliquely from off its axis and nothing in front of it (the stock flat frames
    show their disc on no pixel at 24 x 20): about 150 disc layers."""
    L = grt._lib
    b = grt.SceneBuilder(geometry, radius=0.0, a=0.0, horizon_epsilon=0.0)
    b.integration(2000, 60.0, 0.5, 1e-6)
    cart = (0.0, -10.0, 1.0, 7.0)
    pos = cart if geometry == L.GEOM_EUCLIDEAN else grt.cartesian_to_spherical(cart)
    b.camera(pos, grt.stationary_velocity(geometry, 0.0, 0.0, pos), math.pi / 4, ROWS, COLS, 0.0, 0.6, 0.0)
    b.celestial(grt.Checker(0.0, 16.0, 8.0, (20, 20, 80), (200, 200, 255)))
    b.add_disc(2.0, 9.0, grt.Checker(1.0, 12.0, 4.0, (255, 160, 0), (120, 40, 0)), temperature=1.0)
    d = b.build()
    d._keep_builder = b
    return d


def _analytic_difference(grt, d, gl):
    """max |lapse + distance(camera, layer point)| over the disc layers, the largest |lapse|
    among them and their number; the point from the layer's (u, v) by disc.rs' rule."""
    L = grt._lib
    a, lapse, info = gl.arrays(), gl.lapse(), gl.info
    cam = np.array(d.camera.position[:])
    if d.geometry != L.GEOM_EUCLIDEAN:
        r, th, ph = cam[1], cam[2], cam[3]
        cam = np.array([cam[0], r * math.sin(th) * math.cos(ph), r * math.sin(th) * math.sin(ph), r * math.cos(th)])
    worst, n, big = 0.0, 0, 0.0
    for k in range(lapse.size):
        o = info.shape.objects[int(a["object"][k])]
        if o.kind != L.OBJ_DISC:
            continue
        du, dv = a["u"][k] - 0.5, a["v"][k] - 0.5
        rho, phi = 2.0 * math.hypot(du, dv), math.atan2(dv, du)
        r = o.inner_radius + rho * (o.outer_radius - o.inner_radius)
        # the recorded radius is the in-plane distance in the flat charts
        assert abs(r - a["radius"][k]) <= 1e-12 * max(1.0, r)
        dist = math.dist(cam[1:], (r * math.cos(phi), r * math.sin(phi), 0.0))
        worst, big, n = max(worst, abs(lapse[k] + dist)), max(big, abs(lapse[k])), n + 1
    return worst, big, n


@pytest.mark.parametrize("name", ["euclidean", "euclidean-spherical"])
def test_flat_space_analytic(grt, gpu, name):
    """Measured on an MI355X, 151 disc layers with |lapse| up to 18.99:
    euclidean 1.07e-14, euclidean-spherical 1.35e-6 (the RKF error of that chart at the scene's
    epsilon = 1e-6; the CPU oracle's trajectory gives the same figure).  The stock flat frames
    show their disc on no pixel at 24 x 20, so their part of the check is empty."""
    L = grt._lib
    geometry = L.GEOM_EUCLIDEAN if name == "euclidean" else L.GEOM_EUCLIDEAN_SPHERICAL
    hs, sc, want, gb, gl = lapse_case(grt, name)
    d2 = _flat_disc_scene(grt, geometry)
    gl2 = built_scene(grt, d2).trace_gbuffer(lapse=True)
    total = 0
    for what, d, g in (("stock", hs.desc, gl), ("oblique disc", d2, gl2)):
        worst, big, n = _analytic_difference(grt, d, g)
        print(f"{name} / {what}: {n} disc layers, max |lapse| {big:.6g}, max |lapse + distance| {worst:.3e}")
        bound = FLAT_BOUND * max(1.0, big) if name == "euclidean" else SPHERICAL_BOUND
        assert worst <= bound, (name, what, worst, bound)
        total += n
    assert total >= 100, total


# ------------------------------------------------------------------ 3. oracle walk ----
MAX_OUT = 20000


def _numpy_cart(L, d, x):
    """Cartesian positions of native-chart states, for the candidate filter only."""
    if d.geometry in (L.GEOM_EUCLIDEAN, L.GEOM_KERR):
        return x[:, 1:4]
    r, st, ct, sp, cp = x[:, 1], np.sin(x[:, 2]), np.cos(x[:, 2]), np.sin(x[:, 3]), np.cos(x[:, 3])
    a = d.a if d.geometry == L.GEOM_KERR_BL else 0.0
    return np.stack([(r * cp - a * sp) * st, (r * sp + a * cp) * st, r * ct], axis=1)


def oracle_layers(L, oracle, d, row, col):
    """The layers of a pixel rebuilt with the oracle alone: its camera ray, its trajectory, and
    per window the nearest of its chord tests over the objects in config order.  Returns
    (status, [(object, lapse_ref)]) with lapse_ref = x0[i] + t (x0[i+1] - x0[i]) - x0[0].
    Windows that cannot hit are skipped by a filter with wide margins (the disc's plane not
    within 1e-6 of either end and not crossed; a sphere's surface likewise): the chord tests
    themselves, and the Cartesian points they get, are the oracle's."""
    steps, stop, status = oracle.integrate_ray(d, np.array(d.camera.position[:]), oracle.camera_ray(d, row, col),
                                               max_out=MAX_OUT)
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


_WALK = {}
# the frames of a chart: stock cases of tests/test_gpu_gbuffer.py, and for Schwarzschild (whose
# stock frame shows its disc on a dozen pixels) the disc-only scene of tests/test_gpu_gbuffer_orbit.py
WALK_FRAMES = {"schwarzschild": ("schwarzschild", "S1"), "kerr-schild": ("kerr-schild",), "kerr-bl": ("kerr-bl",)}


def walk_frame(grt, frame):
    """(descriptor, scene, render_pixels of the frame, its buffer traced with a lapse)."""
    if frame == "S1":
        c = case(grt, "S1")
        if "want" not in c:
            c["want"] = c["tracer"].render_pixels(0, 0, ROWS, COLS)
        return c["desc"], c["tracer"], c["want"], c["gb"]
    hs, sc, want, gb, gl = lapse_case(grt, frame)
    return hs.desc, sc, want, gl


def walk_reference(grt, oracle, frame):
    """{pixel: [(object, lapse_ref)]} over the robust pixels (check_parity's mask) of a frame
    with status 0 and at least one layer, once."""
    from test_gpu_parity import check_parity, oracle_pair

    if frame not in _WALK:
        d, sc, got, gl = walk_frame(grt, frame)
        ref, probes = oracle_pair(oracle, d, 0, 0, ROWS, COLS)
        robust = check_parity(got, ref, probes, max_sensitive=0.05)
        walked = {}
        for p in np.nonzero(robust & (ref["status"] == 0) & (ref["hits"] > 0))[0]:
            status, layers = oracle_layers(grt._lib, oracle, d, int(p) // COLS, int(p) % COLS)
            # the walk reproduces the oracle's own layer structure
            assert status == 0 and len(layers) == ref["hits"][p], (frame, p, len(layers), ref["hits"][p])
            walked[int(p)] = layers
        _WALK[frame] = walked
    return _WALK[frame]


@pytest.mark.parametrize("chart", ["schwarzschild", "kerr-schild", "kerr-bl"])
def test_oracle_walk(grt, oracle, gpu, chart):
    """Measured on an MI355X over the robust pixels: Schwarzschild 104 pixels
    and 112 layers, Kerr-Schild 272 and 305, KerrBL 283 and 315; largest relative difference 0
    on each chart, so the bound (10 x the measured value, at most 1e-6) is bit equality."""
    worst, n, pixels = 0.0, 0, 0
    for frame in WALK_FRAMES[chart]:
        d, sc, want, gl = walk_frame(grt, frame)
        walked = walk_reference(grt, oracle, frame)
        a, lapse = gl.arrays(), gl.lapse()
        ls = a["layer_start"].astype(np.int64)
        for p, layers in walked.items():
            assert a["status"][p] == 0
            got_obj, got = a["object"][ls[p]:ls[p + 1]], lapse[ls[p]:ls[p + 1]]
            # a robust pixel whose layer count or objects differ from the buffer's is a failure
            assert list(got_obj) == [k for k, _ in layers], (frame, p, list(got_obj), layers)
            for g, (_, r) in zip(got, layers):
                worst, n = max(worst, abs(g - r) / max(abs(r), 1e-300)), n + 1
        pixels += len(walked)
        print(f"{chart} / {frame}: {len(walked)} robust pixels with layers, lapse {lapse.min():.4f} .. {lapse.max():.4f}")
    print(f"{chart}: {pixels} pixels, {n} layers, largest relative difference {worst:.3e}")
    assert pixels >= 50, pixels
    assert worst <= min(WALK_BOUND[chart], 1e-6), (chart, worst)


# ---------------------------------------------- 4. retarded shade against the host rule ----
_CASES = {}


def case(grt, name):
    """The buffers of tests/test_gpu_gbuffer_orbit.py (KBL, KS: the stock frames with a bitmap
    disc; S1: a disc-only Schwarzschild scene), traced with their lapse."""
    if name not in _CASES:
        if name in ("KBL", "KS"):
            hs, sc, app = _stock_with_bitmap_disc(grt, "kerr-bl" if name == "KBL" else "kerr-schild")
            desc = hs.desc
        else:
            desc = s1_desc(grt)
            sc = app = built_scene(grt, desc)
        gl = sc.trace_gbuffer(lapse=True)
        _CASES[name] = dict(tracer=sc, app=app, desc=desc, gb=gl, info=gl.info, arrays=gl.arrays(), lapse=gl.lapse())
    return _CASES[name]


def retarded(grt, c, t, lapse=None):
    out = dict(c["arrays"])
    a = c["arrays"]
    out["u"], out["v"] = grt.gbuffer_orbit_uv_retarded(c["info"].shape, a["object"], a["u"], a["v"], a["radius"],
                                                       c["lapse"] if lapse is None else lapse, t)
    return out


@pytest.mark.parametrize("name", ["KBL", "KS", "S1"])
def test_retarded_shade_against_host_rule(grt, gpu, name):
    c = case(grt, name)
    gb, info, a, app = c["gb"], c["info"], c["arrays"], c["app"]
    assert disc_pixels(grt, info, a).sum() >= 45
    out = gb.shade_orbit(app, TIMES, retarded=True)
    fast = gb.shade_orbit(app, TIMES)
    for k, t in enumerate(TIMES):
        up = grt.GBuffer.from_arrays(info, retarded(grt, c, t))
        assert_same_frame(Frame(out, k), up.shade(app), (name, t))
        up.close()
        assert np.array_equal(out["stop"][k], a["stop"]) and np.array_equal(out["steps"][k], a["steps"]), (name, t)
    moved = np.any(out["xyza64"][T_MOVED].view(np.uint64) != fast["xyza64"][T_MOVED].view(np.uint64), axis=1)
    print(f"{name}: {moved.sum()} pixels differ between the retarded and the fast-light frame at t = 37.5; "
          f"lapse {c['lapse'].min():.3f} .. {c['lapse'].max():.3f}")
    assert moved.sum() >= 30, moved.sum()
    assert not np.any(moved & ~disc_pixels(grt, info, a))
    # K = 5 in one call equals five K = 1 calls, in one launch group and in groups of one and two frames
    times5 = TIMES + (1e4,)
    singles = [gb.shade_orbit(app, [t], retarded=True) for t in times5]

    def check(o, what):
        for k in range(len(times5)):
            assert_same_frame(Frame(o, k), Frame(singles[k], 0), (name, what, k))
            for f in ("stop", "steps"):
                assert np.array_equal(o[f][k], singles[k][f][0]), (name, what, f, k)

    check(gb.shade_orbit(app, times5, retarded=True), "one group")
    try:
        for frames in (1, 2):
            grt.set_sequence_group(frames * ROWS * COLS)
            check(gb.shade_orbit(app, times5, retarded=True), f"groups of {frames}")
    finally:
        grt.set_sequence_group(0)


@pytest.mark.parametrize("name", ["KBL", "KS", "S1"])
def test_uploaded_lapses(grt, gpu, name):
    """All-zero lapse: the fast-light frames.  A constant lapse c: the fast-light frames at t + c."""
    c = case(grt, name)
    gb, app, n = c["gb"], c["app"], c["lapse"].size
    fast = gb.shade_orbit(app, TIMES)
    shift = -41.625
    shifted = gb.shade_orbit(app, [t + shift for t in TIMES])
    try:
        gb.set_lapse(np.zeros(n))
        out = gb.shade_orbit(app, TIMES, retarded=True)
        for k in range(len(TIMES)):
            assert_same_frame(Frame(out, k), Frame(fast, k), (name, "zero", k))
        gb.set_lapse(np.full(n, shift))
        out = gb.shade_orbit(app, TIMES, retarded=True)
        for k in range(len(TIMES)):
            assert_same_frame(Frame(out, k), Frame(shifted, k), (name, "constant", k))
    finally:
        gb.set_lapse(c["lapse"])
    assert np.array_equal(_bits(gb.lapse()), _bits(c["lapse"]))


@pytest.mark.parametrize("name", ["kerr-bl", "kerr-schild", "euclidean", "euclidean-spherical"])
def test_static_appearances_and_flat_charts_do_not_move(grt, gpu, name):
    """A BlackBody disc's colour does not depend on (u, v); the flat charts' emitter is at rest."""
    hs, sc, want, gb, gl = lapse_case(grt, name)
    out = gl.shade_orbit(sc, ORBIT_TIMES, retarded=True)
    for k, t in enumerate(ORBIT_TIMES):
        assert_same_frame(Frame(out, k), want, (name, t))


# ------------------------------------------------------- 5. round trips and refusals ----
def test_round_trips(grt, gpu, tmp_path):
    c = case(grt, "KBL")
    gb, app, lapse = c["gb"], c["app"], c["lapse"]
    want = gb.shade_orbit(app, TIMES, retarded=True)
    up = grt.GBuffer.from_arrays(c["info"], c["arrays"])
    assert up.lapse() is None
    up.set_lapse(lapse)
    assert np.array_equal(_bits(up.lapse()), _bits(lapse))
    other = lapse - 1.0
    up.set_lapse(other)  # it replaces a held lapse
    assert np.array_equal(_bits(up.lapse()), _bits(other))
    up.close()
    path = tmp_path / "a.grtg"
    gb.save(path)
    assert (tmp_path / "a.grtg.lapse").exists()
    plain = tmp_path / "plain.grtg"
    c["tracer"].trace_gbuffer().save(plain)
    assert not (tmp_path / "plain.grtg.lapse").exists() and plain.read_bytes() == path.read_bytes()
    back = grt.GBuffer.load(path)
    assert np.array_equal(_bits(back.lapse()), _bits(lapse))
    out = back.shade_orbit(app, TIMES, retarded=True)
    for k in range(len(TIMES)):
        assert_same_frame(Frame(out, k), Frame(want, k), ("loaded", k))
    assert grt.GBuffer.load(plain).lapse() is None


def test_refusals(grt, gpu):
    L = grt._lib
    c = case(grt, "KBL")
    gb, app, n = c["gb"], c["app"], c["lapse"].size
    plain = c["tracer"].trace_gbuffer()
    out = np.zeros(n)
    assert L.lib().grt_gbuffer_lapse_download(plain._h, L.dptr(out)) == -errno.ENODATA
    with pytest.raises(grt.GrtError, match=r"\(-61\)"):
        plain.shade_orbit(app, TIMES, retarded=True)
    plain.shade_orbit(app, TIMES)  # the fast-light call needs none
    assert L.lib().grt_gbuffer_lapse_upload(plain._h, L.dptr(out), n - 1) == -errno.EINVAL
    assert L.lib().grt_gbuffer_lapse_upload(plain._h, L.dptr(np.zeros(n + 1)), n + 1) == -errno.EINVAL
    for bad in (float("nan"), float("inf")):
        x = c["lapse"].copy()
        x[n // 2] = bad
        with pytest.raises(grt.GrtError, match=r"\(-22\)"):
            plain.set_lapse(x)
    assert plain.lapse() is None  # a refused upload changes nothing
    with pytest.raises(grt.GrtError, match=r"\(-22\)"):
        gb.set_lapse(c["lapse"][:-1])
    assert np.array_equal(_bits(gb.lapse()), _bits(c["lapse"]))
    for bad in ([], [float("nan")]):
        with pytest.raises(grt.GrtError, match=r"\(-22\)"):
            gb.shade_orbit(app, bad, retarded=True)
    assert L.lib().grt_gbuffer_lapse_download(None, L.dptr(out)) == -errno.EINVAL
    h = C.c_void_p()
    assert L.lib().grt_gbuffer_trace_lapse(None, 0, 0, 0, 1, 1, C.byref(h), None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_trace_lapse(c["tracer"]._s, 0, 0, 0, 0, 1, C.byref(h), None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_trace_lapse(c["tracer"]._s, 0, ROWS, 0, 1, 1, C.byref(h), None) == -errno.EINVAL
    # a VolumetricDisc scene has no geometry buffer, with or without a lapse
    _, vol = stock(grt, "schwarzschild-volumetric-stony.toml", **STOCK["schwarzschild"][1])
    with pytest.raises(grt.GrtError, match=r"\(-95\)"):
        vol.trace_gbuffer(lapse=True)
    plain.close()


@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl", "euclidean-spherical"])
def test_fused_knob_does_not_reach_the_lapse_trace(grt, gpu, name):
    hs, sc, want, gb, gl = lapse_case(grt, name)
    L = grt._lib
    assert L.lib().grt_set_arithmetic(1) == 0
    try:
        fused = sc.trace_gbuffer(lapse=True)
    finally:
        assert L.lib().grt_set_arithmetic(0) == 0
    assert_same_buffer(fused, gb, name)
    assert np.array_equal(_bits(fused.lapse()), _bits(gl.lapse()))
    fused.close()


def test_cli(grt, gpu, tmp_path):
    """`grt gbuffer --lapse` then `grt reshade-orbit --retarded`: the files of GBuffer.save and
    the frames of shade_orbit(retarded=True), byte for byte."""
    w, h = 64, 48
    off = tmp_path / "off.toml"
    off.write_text((SCENES / "schwarzschild.toml").read_text() + "\n[adaptive_sampling]\nenabled = false\n")
    cam = dict(camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=100000)
    common = ["--width", w, "--height", h, "--camera-position", "-16,0,3.5", "--theta", "-3.142", "--max-steps", 100000,
              "--resource-root", RESOURCES, "--config-file", off]
    size = ["--width", w, "--height", h, "--resource-root", RESOURCES, "--config-file", off]
    a, b = tmp_path / "a.grtg", tmp_path / "b.grtg"
    r = _grt(*common, "gbuffer", "--lapse", "--filename", a)
    assert "saved lapse to" in r.stderr
    _grt(*common, "gbuffer", "--filename", b)
    assert a.read_bytes() == b.read_bytes() and not (tmp_path / "b.grtg.lapse").exists()
    hs = grt.HostScene(str(off), grt.GlobalOpts(width=w, height=h, **cam), str(RESOURCES))
    sc = grt.Scene(hs.desc_ptr(), keepalive=hs, adaptive=hs.adaptive)
    gl = sc.trace_gbuffer(lapse=True)
    py = tmp_path / "py.grtg"
    gl.save(py)
    assert py.read_bytes() == a.read_bytes()
    assert (tmp_path / "py.grtg.lapse").read_bytes() == (tmp_path / "a.grtg.lapse").read_bytes()
    _grt(*size, "reshade-orbit", "--gbuffer", a, "--retarded", "--times", "1,36.5,2", "--filename-pattern",
         tmp_path / "f-%04d.png", "--raw-out-pattern", tmp_path / "f-%04d.raw")
    _grt(*size, "reshade-orbit", "--gbuffer", a, "--times", "1,36.5,2", "--filename-pattern", tmp_path / "g-%04d.png")
    want = gl.shade_orbit(sc, [1.0, 37.5], fields=("xyza64",), retarded=True)["xyza64"]
    for k in range(2):
        assert (tmp_path / f"f-{k:04d}.raw").read_bytes() == want[k].tobytes(), k
        assert (tmp_path / f"f-{k:04d}.png").read_bytes() == _png(grt, tmp_path / f"want-{k}.png", want[k], w, h), k
        assert (tmp_path / f"f-{k:04d}.png").read_bytes() != (tmp_path / f"g-{k:04d}.png").read_bytes(), k
    # without the sidecar: a usage error, nothing written
    (tmp_path / "b.grtg.lapse").unlink(missing_ok=True)
    r = subprocess.run([str(GRT), *map(str, size), "reshade-orbit", "--gbuffer", str(b), "--retarded", "--times", "1,36.5,2",
                        "--filename-pattern", str(tmp_path / "h-%04d.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "lapse sidecar" in r.stderr and not list(tmp_path.glob("h-*.png"))
