"""The seeded reciprocals of the region-B Schwarzschild RHS on the GPU (marker `gpu`).

rhs<SCHWARZSCHILD>'s range-free form takes 1 / (r r) from its refined 1 / r with one Newton
step (gr_raytracer_amd/csrc/device/rcp_seed.h) instead of a v_rcp_f64 of its own.
grt_debug_rcp_seed runs the RHS's five quotients through those helpers, with the real
v_rcp_f64, against the compiler's division: no tuple may differ in any bit.  The host
restatement with a modelled estimate is tests/test_rcp_seed.py; the whole RHS against its
IEEE form and whole frames are held by tests/test_gpu_arith.py."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _edge(rng, n, lo, hi, frac_lo=0.15, frac_hi=0.15):
    """|values| log-uniform in [lo, hi), a share of them within a few ulps of either edge
    (as tests/test_gpu_arith.py draws them)."""
    v = np.exp2(rng.uniform(math.log2(lo), math.log2(hi), n))
    k = rng.random(n)
    ulps = rng.integers(0, 4, n).astype(np.float64)
    v = np.where(k < frac_lo, lo * (1.0 + ulps * 2.0 ** -52), v)
    v = np.where(k > 1.0 - frac_hi, np.nextafter(hi, 0.0) * (1.0 - ulps * 2.0 ** -53), v)
    return v * rng.choice((-1.0, 1.0), n)


def test_seeded_reciprocals_equal_the_compilers_division(grt, gpu):
    """2^22 tuples (r, radius, a, sin, cos) in the ranges of schw_div_ok and region B:
    |r| in 2^-100 .. 2^100 with 30% within ulps of either end and 30% next to radius;
    radius within 2^+-50; a = 1 - radius / r as the RHS forms it where that exceeds 2^-42,
    and 25% independent of r within ulps of |a| = 2^-42; sin in [0.75, 1] with 15% at 0.75
    and 15% within ulps of 1; |cos| in 2^-55 .. 0.66 with 15% within ulps of 2^-55."""
    rng = np.random.default_rng(20251019)
    n = 1 << 22
    radius = np.abs(_edge(rng, n, 2.0 ** -50, 2.0 ** 50))
    r = _edge(rng, n, np.nextafter(2.0 ** -100, 1.0), 2.0 ** 100)  # schw_div_ok: 2^-100 < |r| < 2^100
    near = rng.random(n) < 0.3  # the far field and the horizon: r a few radii out, or next to radius
    scale = np.where(rng.random(n) < 0.5, 1.0 + np.exp2(rng.uniform(-39.0, 12.0, n)), 1.0 - np.exp2(rng.uniform(-39.0, -1.0, n)))
    r = np.where(near, radius * scale, r)
    a = 1.0 - radius / r
    on_edge = (rng.random(n) < 0.25) | ~(np.abs(a) > 2.0 ** -42)
    a = np.where(on_edge, 2.0 ** -42 * (1.0 + rng.integers(1, 8, n) * 2.0 ** -52) * rng.choice((-1.0, 1.0), n), a)
    k = rng.random(n)
    st = rng.uniform(0.75, 1.0, n)
    st = np.where(k < 0.15, 0.75, st)
    st = np.where(k > 0.85, 1.0 - rng.integers(0, 8, n) * 2.0 ** -53, st)
    ct = _edge(rng, n, np.nextafter(2.0 ** -55, 1.0), 0.66, frac_hi=0.05)
    assert (np.abs(r) > 2.0 ** -100).all() and (np.abs(r) < 2.0 ** 100).all() and (np.abs(a) > 2.0 ** -42).all()
    assert (st >= 0.75).all() and (st <= 1.0).all() and (np.abs(ct) > 2.0 ** -55).all() and (np.abs(ct) < 0.66).all()
    tuples = np.ascontiguousarray(np.stack([r, radius, a, st, ct], axis=1), np.float64)
    flags = np.zeros(n, np.uint8)
    fn = grt._lib.lib().grt_debug_rcp_seed
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
    assert fn(gpu, n, tuples.ctypes.data, flags.ctypes.data) == 0, grt._lib.lib().grt_last_error()
    bad = np.nonzero(flags)[0]
    print("rcp seed: tuples", n, "on the |a| edge", int(on_edge.sum()), "differing", bad.size)
    assert bad.size == 0, (bad.size, flags[bad[:5]], [t.tolist() for t in tuples[bad[:5]]])
