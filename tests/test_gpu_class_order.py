"""The Schwarzschild tile queue grouped by sincos case (grt_set_class_order, schedule.hip
tile_class, geodesic_probe.h class_key_kernel; marker `gpu`).

The order decides which lane traces which pixel and nothing else, so every comparison of
rendered output is exact (array_equal).  Scene: schwarzschild.toml with C2's camera and
max_radius = 1000 (rays of about 1,000 steps).  Each mode renders on a Scene of its own
that has never rendered: the workspace persists between calls, and a pixel the queue
skipped would otherwise inherit the record an earlier render left there.  The forced modes
render before the row-major reference for the same reason.

Mode 2 selected a pixel-level regrouping of the straddling tiles (the seam), which was
measured and deleted: there is no seam_pix to read back, the mode takes
mode 1's path, and it is compared all the same."""
import ctypes as C

import numpy as np
import pytest

from conftest import c2_opts, host_scene

pytestmark = pytest.mark.gpu

MAX_RADIUS = 1000.0
FIELDS = ("xyza64", "xyza", "ray_class", "status", "steps", "stop_reason", "hits")
COUNTERS = ("accepted_steps", "attempts", "rays", "hit_overflows")


def fresh_scene(grt, width, height, **kw):
    hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt, width=width, height=height, max_radius=MAX_RADIUS, **kw))
    return hs, grt.Scene(hs.desc_ptr(), keepalive=hs)


class modes:
    """grt_set_schedule / grt_set_class_order for a block, the defaults restored after it."""

    def __init__(self, grt, schedule, class_order):
        self.L, self.s, self.c = grt._lib, schedule, class_order

    def __enter__(self):
        self.L.check(self.L.lib().grt_set_schedule(self.s))
        self.L.check(self.L.lib().grt_set_class_order(self.c))

    def __exit__(self, *exc):
        self.L.lib().grt_set_schedule(-1)
        self.L.lib().grt_set_class_order(-1)


def assert_same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    for c in COUNTERS:
        assert a.stats[c] == b.stats[c], (what, c)


def render_modes(grt, gpu, width, height, render, order=((0, 1), (0, 2), (0, 0))):
    """{class mode: result}, each on a fresh scene, in the order given (schedule, class mode)."""
    out = {}
    for schedule, mode in order:
        _hs, sc = fresh_scene(grt, width, height)
        with modes(grt, schedule, mode):
            out[mode] = render(sc)
        sc.close()
    return out


# 256x256: automatic mode's smallest frame (1024 tiles); 250x203: the frame edge cuts tiles,
# straddling ones among them; 16x16: four tiles, forced only
@pytest.mark.parametrize("width,height", [(256, 256), (250, 203), (16, 16)])
def test_forced_class_order_is_result_neutral(grt, gpu, width, height):
    out = render_modes(grt, gpu, width, height, lambda sc: sc.render_pixels(device=gpu))
    assert out[0].stats["rays"] == width * height
    assert_same(out[1], out[0], "mode 1")
    assert_same(out[2], out[0], "mode 2")


def test_automatic_mode_is_result_neutral(grt, gpu):
    """Both knobs automatic on 1024 tiles (the impact-parameter order applies, so the class
    order does) against row-major tiles."""
    out = render_modes(grt, gpu, 256, 256, lambda sc: sc.render_pixels(device=gpu), order=((-1, -1), (0, 0)))
    assert_same(out[-1], out[0], "automatic")


def test_row_shard_is_result_neutral(grt, gpu):
    """Shard 1 of 2 with 64-row bands: the two bands 64..127 and 192..255 of the 256^2 frame."""
    out = render_modes(grt, gpu, 256, 256, lambda sc: sc.render_shard(64, 1, 2, device=gpu))
    assert out[0].stats["rays"] == 128 * 256
    assert_same(out[1], out[0], "mode 1")
    assert_same(out[2], out[0], "mode 2")


CAMS = [((-16.0, 0.0, 3.5), 0.0, -3.142, 0.0), ((-15.0, 4.0, 3.0), 0.1, -3.0, 0.05)]


def test_stacked_sequence_equals_the_per_frame_renders(grt, gpu):
    """Two cameras at 128^2 stacked into one queue of 512 tiles (forced), against each
    camera's own row-major render."""
    refs = []
    for pos, phi, theta, psi in CAMS:
        _hs, sc = fresh_scene(grt, 128, 128, camera_position=pos, phi=phi, theta=theta, psi=psi)
        with modes(grt, 0, 0):
            refs.append(sc.render_pixels(device=gpu))
        sc.close()
    for mode in (1, 2):
        hs, sc = fresh_scene(grt, 128, 128)
        cams = [hs.camera(pos, phi, theta, psi) for pos, phi, theta, psi in CAMS]
        with modes(grt, 0, mode):
            seq = sc.render_sequence(cams, device=gpu)
        sc.close()
        for k, ref in enumerate(refs):
            for name, f in (("xyza64", "xyza64"), ("xyza", "xyza"), ("class", "ray_class"), ("status", "status"),
                            ("stop", "stop_reason"), ("steps", "steps")):
                assert np.array_equal(seq[name][k], getattr(ref, f)), (mode, k, name)
        assert seq["stats"]["accepted_steps"] == sum(r.stats["accepted_steps"] for r in refs)
        assert seq["stats"]["rays"] == sum(r.stats["rays"] for r in refs)


# ------------------------------------------------------------------ the order itself ----
def debug_order(grt, sc, gpu, width, height):
    """(order, class, corner pi/2 - theta_f, impact keys) of the whole frame's queue."""
    L = grt._lib
    lib = L.lib()
    tx, ty = (width + 7) // 8, (height + 7) // 8
    n, nc = tx * ty, (tx + 1) * (ty + 1)
    sh = L.RowShard(16, 0, 1)
    fn = lib.grt_debug_class_order
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(L.RowShard), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                   C.c_uint64]
    order, cls, corner = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(nc, np.float32)
    L.check(fn(sc._s, gpu, C.byref(sh), order.ctypes.data, cls.ctypes.data, corner.ctypes.data, n, nc),
            "grt_debug_class_order")
    keys_fn = lib.grt_debug_probe_keys
    keys_fn.restype = C.c_int
    keys_fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(L.RowShard), C.c_int, C.c_void_p, C.c_uint64]
    keys = np.zeros(n, np.uint32)
    L.check(keys_fn(sc._s, gpu, C.byref(sh), 2, keys.ctypes.data, n), "grt_debug_probe_keys")
    return order, cls.reshape(ty, tx), corner.reshape(ty + 1, tx + 1), keys.reshape(ty, tx)


def dilate(keys):
    """schedule.hip dilate_kernel without the edge boost (no impact key counts as capped)."""
    ty, tx = keys.shape
    pad = np.zeros((ty + 2, tx + 2), keys.dtype)
    pad[1:-1, 1:-1] = keys
    return np.max([pad[1 + dr:1 + dr + ty, 1 + dc:1 + dc + tx] for dr in (-1, 0, 1) for dc in (-1, 0, 1)], axis=0)


@pytest.mark.parametrize("width,height", [(256, 256), (250, 203)])
def test_order_is_a_permutation_sorted_by_length_bucket_then_class(grt, gpu, width, height):
    _hs, sc = fresh_scene(grt, width, height)
    order, cls, _corner, keys = debug_order(grt, sc, gpu, width, height)
    sc.close()
    n = cls.size
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))  # every tile exactly once
    assert cls.max() <= 3 and set(np.unique(cls)) == {0, 1, 2, 3}  # C2's view holds every class
    # near-critical tiles (longer predicted rays) still precede the rest: the length in
    # 1024-step buckets never grows along the queue; the class never falls within a bucket;
    # row-major among equals
    bucket = (dilate(keys) >> 10).ravel()[order].astype(np.int64)
    c = cls.ravel()[order].astype(np.int64)
    assert (np.diff(bucket) <= 0).all()
    assert bucket[0] > bucket[-1]
    same_bucket = np.diff(bucket) == 0
    assert (np.diff(c)[same_bucket] >= 0).all()
    same = same_bucket & (np.diff(c) == 0)
    assert (np.diff(order.astype(np.int64))[same] > 0).all()


def test_tile_classes_follow_the_corner_predictions(grt, gpu):
    """A tile is Taylor (0) or table (2) only when its four corners are; the Taylor band is
    the strip round the equator of the sky."""
    taylor_max = float.fromhex("0x1.020c49ba5e354p-3")
    _hs, sc = fresh_scene(grt, 256, 256)
    _order, cls, a, _keys = debug_order(grt, sc, gpu, 256, 256)
    sc.close()
    corners = np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]])
    assert (np.abs(corners[:, cls == 0]) < taylor_max).all()
    tab = corners[:, cls == 2]
    assert (np.abs(tab) > taylor_max).all() and (np.sign(tab) == np.sign(tab[0])).all()
    assert 0.1 < (cls == 0).mean() / ((cls == 0) | (cls == 2)).mean() < 0.3  # the census's Taylor share is 0.178
    # the straddling tiles lie along curves: the two edges of the Taylor band, the two of
    # region B and the shadow's, each crossing at most ~2 x 32 of the 32 x 32 tiles, 1.5
    # tiles wide with the margin: below 5 * 64 * 1.5 / 1024
    assert (cls == 1).mean() < 0.47


def test_predictor_matches_the_rays(grt, gpu):
    """Speed only, never results: the predicted theta_f of 256 escaping rays (a seeded
    sample of the corner pixels (8i, 8j) of the 256^2 frame) against the last theta of
    their trajectories, within 2 b_max / max_radius (theta(r) - theta_f = O(b / r) in the
    far field; b_max the largest impact parameter of the sample, from the initial states);
    captured pixels are predicted captured."""
    L = grt._lib
    _hs, sc = fresh_scene(grt, 256, 256)
    _order, _cls, a, _keys = debug_order(grt, sc, gpu, 256, 256)
    with modes(grt, 0, 0):
        frame = sc.render_pixels(device=gpu)
    stop = frame.stop_reason.reshape(256, 256)[::8, ::8]
    steps = frame.steps.reshape(256, 256)[::8, ::8]
    a = a[:32, :32]  # the corners that are pixels (8i, 8j) themselves, unclamped
    captured = stop == L.STOP_HORIZON
    assert captured.sum() >= 4
    assert (a[captured] > 1e29).all()
    cap = 4096
    ii, jj = np.nonzero((stop == L.STOP_CELESTIAL) & (steps < cap - 1))
    pick = np.random.default_rng(20260).choice(len(ii), 256, replace=False)
    ii, jj = ii[pick], jj[pick]
    tr = sc.trace_pixels(8 * ii, 8 * jj, capacity=cap, device=gpu)
    sc.close()
    assert (tr.stop_reason == L.STOP_CELESTIAL).all() and (tr.n_steps <= cap).all()
    first = tr.steps[:, 0]
    last = tr.steps[np.arange(256), tr.n_steps - 1]
    # record: (l, t, r, theta, phi, dt, dr, dtheta, dphi); b = L / E
    r, th = first[:, 2], first[:, 3]
    rs = float(sc.desc.radius)
    e = np.abs((1.0 - rs / r) * first[:, 5])
    b = r * r * np.sqrt(first[:, 7] ** 2 + np.sin(th) ** 2 * first[:, 8] ** 2) / e
    tol = 2.0 * b.max() / MAX_RADIUS
    predicted = np.pi / 2 - a[ii, jj].astype(np.float64)
    theta_last = np.arccos(np.cos(last[:, 3]))  # the chart's theta folded into [0, pi]
    err = np.abs(predicted - theta_last)
    print(f"predictor: b_max {b.max():.3f}, tolerance {tol:.5f}, largest error {err.max():.5f}")
    assert np.isfinite(predicted).all()
    assert (err <= tol).all(), (err.max(), tol)
