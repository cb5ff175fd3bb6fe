"""The Schwarzschild integrate kernel's two bit-neutral savings, on the GPU (marker `gpu`).

* Short RKF sums (geodesic_rkf.h rkf_attempt_fold, SHORT): the attempt without its zero-weight
  CH2 / CT2 terms, guarded by rkf_short_ok ("every yn finite and not -0, err_sq finite").
  test_short_attempt_equals_full_where_the_guard_admits runs single attempts in both forms
  (grt_debug_rkf_check) on ordinary states and on states planted with signed zeros,
  non-finite velocities and radii at the horizon; the frame tests render with the short sums
  on and off (grt_debug_rkf_short) and want every output array identical.
* Unit-radius quotients (rcp_seed.h unit_radius_quotients): the region-B RHS of a scene with
  radius == 1.0.  Scenes with radius 1.5 and 2.0 keep the general range-free form, which
  still equals the IEEE form (grt_debug_rhs_check, frames with grt_debug_range_free off);
  for radius 1.0 the same frame comparison runs the new block end to end.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest

from conftest import SCENES, RESOURCES, c2_opts, host_scene

pytestmark = pytest.mark.gpu

FRAME_KEYS = ("ray_class", "status", "stop_reason", "steps", "hits")


def _switch(grt, name):
    fn = getattr(grt._lib.lib(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int]
    return fn


def _frame(grt, hs, rect, switch, on):
    fn = _switch(grt, switch)
    assert fn(int(on)) == 0
    try:
        sc = grt.Scene(hs.desc_ptr(), keepalive=hs)
        r = sc.render_pixels(*rect, aux=True)
    finally:
        fn(1)
    return r


def _assert_same_frames(a, b):
    assert np.array_equal(a.xyza64.view(np.uint64), b.xyza64.view(np.uint64))
    for k in FRAME_KEYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


# ---------------------------------------------------------------- (a) single attempts

def _rkf_check(grt, gpu, hs, states, h):
    sc = grt.Scene(hs.desc_ptr(), keepalive=hs)
    n = len(states)
    states = np.ascontiguousarray(states, np.float64)
    h = np.ascontiguousarray(h, np.float64)
    short, full = np.zeros((n, 9), np.float64), np.zeros((n, 9), np.float64)
    guard = np.zeros(n, np.uint8)
    fn = grt._lib.lib().grt_debug_rkf_check
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(sc._s, gpu, n, states.ctypes.data, h.ctypes.data, short.ctypes.data, full.ctypes.data,
              guard.ctypes.data) == 0, grt._lib.lib().grt_last_error()
    return short, full, guard.astype(bool)


def test_short_attempt_equals_full_where_the_guard_admits(grt, gpu):
    """2^18 states, one attempt each in both forms.  70 % ordinary (r in 2 .. 40, theta in
    and outside sincos's region B, velocities within +-3, h in {1, 0.25, 1e-6}); the rest
    planted: -0 / +0 in phi, v_phi, v_theta and t, and v_t = -0 next to the horizon; +-inf or
    NaN in one velocity; r within 2^-30 of the radius (at it, a = 0 and a' / a overflows).
    Wherever the guard admits the short result, yn and err_sq of the two forms are equal bit
    for bit, and every state whose forms differ is refused (measured: 138 of the 2^18 differ,
    all among the v_t = -0 states and all refused)."""
    hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt, width=8, height=8))
    radius = hs.desc.radius
    rng = np.random.default_rng(0x5EED)
    n = 1 << 18
    theta = np.where(rng.random(n) < 0.6, rng.uniform(0.86, 2.42, n), rng.uniform(0.05, 3.09, n))
    st = np.stack([rng.uniform(-10, 10, n), rng.uniform(2.0, 40.0, n), theta, rng.uniform(-3, 3, n)] +
                  [rng.uniform(-3, 3, n) for _ in range(4)], axis=1)
    h = rng.choice((1.0, 0.25, 1e-6), n)
    kind = np.zeros(n, np.int8)  # 0 ordinary, 1 signed zeros, 2 non-finite velocity, 3 r at the horizon
    kind[rng.random(n) >= 0.7] = 1
    planted = np.nonzero(kind)[0]
    kind[planted] = rng.integers(1, 4, planted.size)
    z = np.nonzero(kind == 1)[0]
    for comp in (3, 7, 6, 0):  # phi, v_phi, v_theta, t: each planted in about 70 % of these states
        m = z[rng.random(z.size) < 0.7]
        st[m, comp] = rng.choice((-0.0, 0.0), m.size)
    # half of them with phi and v_phi both -0: phi's short sum is then a sum of -0 terms
    both = z[rng.random(z.size) < 0.5]
    st[both, 3] = -0.0
    st[both, 7] = -0.0
    # a third of them with v_t = -0 and r in 1.02 .. 2 radii, v_r as drawn: next to the horizon
    # v_r changes sign from one stage to the next, and with it the zero k_j[4] = -(a' / a) v_t v_r,
    # which is how a -0 partial sum meets a +0 k2 (measured on the host: about 1.5 % of these)
    near = z[rng.random(z.size) < 0.35]
    st[near, 4] = -0.0
    st[near, 1] = radius * rng.uniform(1.02, 2.0, near.size)
    nf = np.nonzero(kind == 2)[0]
    st[nf, rng.integers(4, 8, nf.size)] = rng.choice((np.inf, -np.inf, np.nan), nf.size)
    hz = np.nonzero(kind == 3)[0]
    st[hz, 1] = radius + rng.integers(-4, 5, hz.size) * 2.0 ** -32 * (rng.random(hz.size) < 0.75)
    assert np.all(np.abs(st[hz, 1] - radius) <= 2.0 ** -30) and np.any(st[hz, 1] == radius)

    short, full, guard = _rkf_check(grt, gpu, hs, st, h)
    su, fu = short.view(np.uint64), full.view(np.uint64)
    same = np.all((su == fu) | (np.isnan(short) & np.isnan(full)), axis=1)
    print("states", n, "admitted", int(guard.sum()), "differ", int((~same).sum()),
          {k: (int((kind == k).sum()), int((guard & (kind == k)).sum())) for k in range(4)})
    bad = np.nonzero(guard & ~np.all(su == fu, axis=1))[0]
    assert bad.size == 0, (bad.size, st[bad[:3]], short[bad[:3]], full[bad[:3]])
    assert not np.any(~same & guard)  # every state whose forms differ is refused
    # conditions that make the check a check
    assert guard[kind == 0].all(), np.nonzero(~guard & (kind == 0))[0][:5]
    for k in (1, 2, 3):
        assert (~guard[kind == k]).any(), k
    assert (~same & ~guard).any()  # some refused state does differ: the guard is needed
    # what differs there is the short form's -0 against +0 (rkf_attempt_fold's lemma)
    d = ~same & (kind == 1) & np.isfinite(short).all(axis=1) & np.isfinite(full).all(axis=1)
    assert d.any()
    yn_diff = (su[:, :8] != fu[:, :8]) & d[:, None]
    assert np.all(su[:, :8][yn_diff] == np.uint64(1 << 63)) and np.all(fu[:, :8][yn_diff] == 0)
    assert np.array_equal(su[d, 8], fu[d, 8])  # err_sq: e enters as e * e


# ---------------------------------------------------------------- (b) frames, short sums on / off

def _meridional_scene(grt):
    # the camera on the x axis' side of the y = 0 plane looking at the hole: the centre column
    # of an odd-width frame lies in that meridional plane, where v_phi starts as a zero
    return host_scene(grt, "schwarzschild.toml",
                      c2_opts(grt, width=65, height=9, camera_position=(16.0, 0.0, 3.5), theta=0.0))


@pytest.mark.parametrize("case", ["shadow_edge", "disc", "meridional", "volumetric"])
def test_frames_with_short_sums_equal_frames_with_full_sums(grt, oracle, gpu, case):
    """grt_debug_rkf_short(1) against (0), where every attempt takes the full form, and
    against (2), where every attempt off the quick step is taken again in the full form: XYZA in
    f64, class, status, stop reason, steps and hits array for array.  C2 crops through the
    shadow edge (retries, the near-field general path) and across the disc; a 65 x 9 frame
    whose centre column lies in the camera's meridional plane (v_phi = +-0 at the start, by
    the host's initial momenta); a crop of the volumetric Schwarzschild scene."""
    if case == "shadow_edge":
        hs, rect = host_scene(grt, "schwarzschild.toml", c2_opts(grt)), (718, 860, 64, 64)
    elif case == "disc":
        hs, rect = host_scene(grt, "schwarzschild.toml", c2_opts(grt)), (718, 980, 64, 64)
    elif case == "meridional":
        hs, rect = _meridional_scene(grt), (0, 0, 9, 65)
        v_phi = np.array([[oracle.camera_ray(hs.desc, r, c)[3] for c in range(65)] for r in range(9)])
        assert (v_phi == 0.0).any(), v_phi[:, 32]
    else:
        hs = host_scene(grt, "schwarzschild-volumetric-stony.toml", c2_opts(grt, width=160, height=160))
        rect = (36, 40, 64, 64)
    a = _frame(grt, hs, rect, "grt_debug_rkf_short", 1)
    b = _frame(grt, hs, rect, "grt_debug_rkf_short", 0)
    _assert_same_frames(a, b)
    # No camera of the host's setup starts a ray with v_phi = -0 (its sums give +0, which
    # meets rkf_short_ok), so the fallback of a missed premise -- the short attempt, then the
    # full one over it -- is forced: mode 2 takes it after every attempt that leaves the quick step.
    c = _frame(grt, hs, rect, "grt_debug_rkf_short", 2)
    _assert_same_frames(a, c)
    assert c.stats["attempts"] == a.stats["attempts"]
    cls = np.bincount(a.ray_class, minlength=3)
    print(case, "classes", cls.tolist(), "steps", a.stats["accepted_steps"], "attempts short / full",
          a.stats.get("attempts"), b.stats.get("attempts"))
    if case == "shadow_edge":
        assert cls[grt._lib.CLASS_CAPTURED] > 0 and cls[grt._lib.CLASS_ESCAPED] > 0
    if case == "disc":
        assert cls[grt._lib.CLASS_HIT] > 0
    if case == "volumetric":
        assert a.stats["march_jobs"] > 0


# ---------------------------------------------------------------- (c) unit radius

def _edge(rng, n, lo, hi, frac_lo=0.15, frac_hi=0.15):
    """|values| log-uniform in [lo, hi), a share of them within a few ulps of either edge."""
    v = np.exp2(rng.uniform(math.log2(lo), math.log2(hi), n))
    k = rng.random(n)
    ulps = rng.integers(0, 4, n).astype(np.float64)
    v = np.where(k < frac_lo, lo * (1.0 + ulps * 2.0 ** -52), v)
    v = np.where(k > 1.0 - frac_hi, np.nextafter(hi, 0.0) * (1.0 - ulps * 2.0 ** -53), v)
    return v * rng.choice((-1.0, 1.0), n)


def _rhs_check(grt, gpu, hs, states):
    sc = grt.Scene(hs.desc_ptr(), keepalive=hs)
    n = len(states)
    states = np.ascontiguousarray(states, np.float64)
    out = np.zeros((n, 16), np.float64)
    pred = np.zeros(n, np.uint8)
    fn = grt._lib.lib().grt_debug_rhs_check
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(sc._s, gpu, n, states.ctypes.data, None, out.ctypes.data, pred.ctypes.data) == 0, \
        grt._lib.lib().grt_last_error()
    fast, ieee = out[:, :8].view(np.uint64), out[:, 8:].view(np.uint64)
    same = np.all((fast == ieee) | (np.isnan(out[:, :8]) & np.isnan(out[:, 8:])), axis=1)
    return pred.astype(bool), same


def _scene_with_radius(grt, tmp_path, radius):
    text = (SCENES / "schwarzschild.toml").read_text()
    # the geometry's radius: the file's first `radius =` line
    new, k = re.subn(r"(?m)^(radius\s*=\s*)1\.0\s*$", lambda m: m.group(1) + repr(radius), text, count=1)
    assert k == 1
    p = tmp_path / f"schwarzschild-r{radius}.toml"
    p.write_text(new)
    hs = grt.HostScene(str(p), c2_opts(grt), str(RESOURCES))
    assert hs.desc.radius == radius
    return hs


@pytest.mark.parametrize("radius", [1.0, 1.5, 2.0])
def test_range_free_rhs_with_and_without_unit_radius(grt, gpu, tmp_path, radius):
    """radius 1.5 and 2.0: the general range-free form still equals the IEEE form on 2^18
    states at the edges of schw_div_ok, and a 64 x 64 crop renders identically with
    grt_debug_range_free on and off.  radius 1.0: the same two checks run the unit-radius
    block (rhs_check_kernel follows DevScene::unit_radius)."""
    hs = _scene_with_radius(grt, tmp_path, radius)
    rng = np.random.default_rng(int(radius * 16))
    n = 1 << 18
    r = _edge(rng, n, 2.0 ** -100, 2.0 ** 100)
    near = rng.random(n) < 0.3  # |r - radius| just above 2^-40 radius, both sides
    off = radius * 2.0 ** -40 * (1.0 + rng.integers(1, 1 << 12, near.sum()) * 2.0 ** -20)
    r[near] = radius + off * rng.choice((-1.0, 1.0), near.sum())
    theta = rng.uniform(0.86, 2.42, n)
    k = rng.random(n)
    theta = np.where(k < 0.1, math.pi / 2 + rng.integers(-8, 9, n) * 2.0 ** -52, theta)
    theta = np.where((k >= 0.1) & (k < 0.15), rng.choice((0.855469, 2.426265), n) + rng.integers(-64, 64, n) * 1e-9,
                     theta)
    st = np.stack([rng.uniform(-1, 1, n), r, theta, rng.uniform(-3, 3, n)] + [rng.uniform(-3, 3, n) for _ in range(4)],
                  axis=1)
    pred, same = _rhs_check(grt, gpu, hs, st)
    assert pred.mean() >= 0.5, pred.mean()
    bad = np.nonzero(pred & ~same)[0]
    assert bad.size == 0, (bad.size, st[bad[:3]])
    rect = (718, 860, 64, 64)  # through the shadow edge of radius 1.0; the disc for the larger holes
    a = _frame(grt, hs, rect, "grt_debug_range_free", True)
    b = _frame(grt, hs, rect, "grt_debug_range_free", False)
    _assert_same_frames(a, b)
    print("radius", radius, "admitted", int(pred.sum()), "classes", np.bincount(a.ray_class, minlength=3).tolist())
