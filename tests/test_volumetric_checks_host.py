"""The VolumetricDisc unit checks, CPU side: the argument tests of the two debug entries
(grt_debug_vdisc_points, grt_debug_vdisc_march; api.hip) that need no device, the oracle's
additions for them, and the precondition of the GPU raymarch test.

tests/test_gpu_volumetric_checks.py holds the device to the oracle at 1e-4 per channel on
every job that the oracle's volumetric atan2 probes (oracle_set_libm_perturbation bits 32 and
64) do not move.  That excuses a job only if few jobs are excused: here, with the oracle
alone, at most 2 % of each job list may move (check_parity's max_sensitive).
"""
import ctypes as C
import math

import numpy as np
import pytest

import volumetric_cases as V
from gr_raytracer_amd import _lib as L

EINVAL = -22


@pytest.fixture(scope="module")
def flat(grt):
    return V.flat_scene(grt)


@pytest.fixture(scope="module")
def two_gas(grt):
    return V.two_gas_scene(grt)


def _scene(grt, hs):
    return grt.Scene(hs.desc_ptr(), keepalive=hs)


# -------------------------------------------------------------- argument validation --
def test_vdisc_points_arguments(grt, flat):
    b = grt.SceneBuilder(L.GEOM_EUCLIDEAN).integration(100, 100.0, 0.01, 1e-5)
    b.camera((0.0, 9.0, 0.0, 0.6), (1.0, 0.0, 0.0, 0.0), 0.7, 8, 8).celestial(grt.Checker(0.0, 4.0, 4.0, (0, 0, 0), (9, 9, 9)))
    b.add_sphere(1.0, (0.0, 0.0, 0.0), grt.Checker(0.0, 4.0, 4.0, (255, 0, 0), (0, 0, 255)))
    plain = b.scene()
    sc = _scene(grt, flat)
    fn = V.points_fn()
    x, out, flag = np.zeros((4, 6)), np.zeros((4, 8)), np.zeros(4, np.uint8)
    args = (x.ctypes.data, out.ctypes.data, flag.ctypes.data)
    assert fn(None, 0, 0, V.FN_PERLIN, 4, *args) == EINVAL
    for bad_fn in (-1, 5):
        assert fn(sc._s, 0, 0, bad_fn, 4, *args) == EINVAL
    for bad_obj in (-1, 1, 8):  # out of range
        assert fn(sc._s, 0, bad_obj, V.FN_DENSITY, 4, *args) == EINVAL
    assert fn(plain._s, 0, 0, V.FN_DENSITY, 4, *args) == EINVAL  # a sphere
    for k in range(3):  # a null buffer
        a = list(args)
        a[k] = None
        assert fn(sc._s, 0, 0, V.FN_CHORD, 4, *a) == EINVAL
    assert b"vdisc points" in L.lib().grt_last_error()
    assert fn(sc._s, 0, 0, V.FN_CHORD, 0, None, None, None) == 0  # n = 0: nothing to do, no device


def test_vdisc_march_arguments(grt, flat):
    sc = _scene(grt, flat)
    kb = grt.SceneBuilder(L.GEOM_KERR, radius=1.0, a=0.5, horizon_epsilon=1e-4).integration(100, 100.0, 0.01, 1e-5)
    kb.celestial(grt.Checker(0.0, 4.0, 4.0, (0, 0, 0), (9, 9, 9)))
    kb.d.camera = flat.desc.camera  # never traced
    kb.add_volumetric_disc(3.0, 6.0, grt.Checker(0.0, 4.0, 4.0, (255, 0, 0), (0, 0, 255)), 1000.0,
                           constant_temperature=True, **V.GAS)
    kerr = kb.scene()
    fn = V.march_fn()
    n = 3
    obj, ro, dr, fq = np.zeros(n, np.uint32), np.ones((n, 3)), np.ones((n, 3)), np.ones((n, 3))
    col, cnt = np.zeros((n, 4)), np.full(4, 7, np.uint64)
    bufs = [obj.ctypes.data, ro.ctypes.data, dr.ctypes.data, fq.ctypes.data]
    outs = [col.ctypes.data, cnt.ctypes.data]

    def call(s=sc._s, n=n, bufs=bufs, blocks=1, arith=0, as_pool=0, outs=outs):
        return fn(s, 0, n, *bufs, blocks, arith, as_pool, *outs)

    assert call(s=None) == EINVAL
    for arith in (-1, 2):
        assert call(arith=arith) == EINVAL
    assert call(s=kerr._s, arith=1) == EINVAL  # Kerr-Schild has no fused kernels
    for blocks in (0, -3, 4097):
        assert call(blocks=blocks) == EINVAL
    for k in range(4):
        b = list(bufs)
        b[k] = None
        assert call(bufs=b) == EINVAL
    for k in range(2):
        o = list(outs)
        o[k] = None
        assert call(outs=o) == EINVAL
    for bad in (1, 8, 0xFFFFFFFF):  # not an object of the scene
        obj[1] = bad
        assert call() == EINVAL
    obj[1] = 0
    assert b"vdisc march" in L.lib().grt_last_error()
    assert call(n=0) == 0 and not cnt.any()  # n = 0: success, counters zeroed, no device


# ------------------------------------------------------------------ oracle additions --
def _local(fr, p, e):
    return p[:, 0] * e[0] + p[:, 1] * e[1] + p[:, 2] * e[2]  # nalgebra dot: a + b + c


@pytest.mark.parametrize("axis", [V.TILT, V.ZAXIS])
def test_density_phi_equals_density_with_glibc_atan2(grt, oracle, axis):
    """compute_density with phi handed in is compute_density when phi is glibc's atan2 of the
    same in-plane coordinates: bit for bit on the whole point set of the GPU density test."""
    hs = V.flat_scene(grt, axis)
    pts = V.density_points(oracle, hs.desc)
    assert 18000 <= len(pts) <= 25000
    fr = V.Frame(hs.desc)
    # libm's atan2, as the oracle calls it (numpy's arctan2 may be a vector routine with other last bits)
    phi = np.array([math.atan2(y, x) for y, x in zip(_local(fr, pts, fr.e2), _local(fr, pts, fr.e1))])
    d = oracle.vdisc_density_n(hs.desc, 0, pts)
    assert np.array_equal(V.bits(oracle.vdisc_density_n(hs.desc, 0, pts, phi)), V.bits(d))
    assert 0.2 < np.mean(d > 0.0) < 0.9
    for i in (0, 17, len(pts) - 1):  # the scalar forms
        assert oracle.vdisc_density(hs.desc, 0, pts[i]) == d[i] == oracle.vdisc_density_phi(hs.desc, 0, pts[i], phi[i])
    # the oracle's export of the same in-plane coordinates and of whether the noise was reached
    x, y, noise = oracle.vdisc_plane_n(hs.desc, 0, pts)
    assert np.array_equal(V.bits(x[noise]), V.bits(_local(fr, pts, fr.e1)[noise]))
    assert np.array_equal(V.bits(y[noise]), V.bits(_local(fr, pts, fr.e2)[noise]))
    assert np.all(d[~noise] == 0.0) and 0.4 < noise.mean() < 0.9 and np.any(d[noise] == 0.0)
    # and another angle gives another density somewhere
    assert np.any(oracle.vdisc_density_n(hs.desc, 0, pts, phi + 0.01) != d)


def test_array_forms_equal_the_scalar_forms(grt, oracle, flat):
    rng = np.random.default_rng(3)
    pts = V.perlin_points()[rng.integers(0, 20000, 40)]
    for seed in V.SEEDS:
        assert np.array_equal(V.bits(oracle.perlin_n(seed, pts)), V.bits([oracle.perlin(seed, *p) for p in pts]))
    seg = V.segments(flat.desc)
    pick = seg[rng.integers(0, len(seg), 60)]
    hit, t, pt = oracle.vdisc_intersects_n(flat.desc, 0, pick[:, :3], pick[:, 3:])
    for i, s in enumerate(pick):
        h1, p1, t1 = oracle.object_intersects(flat.desc, 0, [0.0, *s[:3]], [0.0, *s[3:]])
        assert h1 == hit[i] and (not h1 or (t1 == t[i] and np.array_equal(p1[1:], pt[i])))
    rays = V.exit_rays(flat.desc)[rng.integers(0, 5000, 60)]
    found, dist = oracle.vdisc_exit_distance_n(flat.desc, 0, rays[:, :3], rays[:, 3:])
    for i, r in enumerate(rays):
        assert oracle.vdisc_exit_distance(flat.desc, 0, r[:3], r[3:]) == (found[i], dist[i])
    assert found.any() and not found.all()
    jobs = V.march_jobs(flat.desc, curved=False)
    col, err, ns = V.oracle_march(oracle, flat.desc, jobs)
    rd = V.unit_rows(jobs[2])
    for i in (0, 5, 11, 299):
        e1, c1, n1 = oracle.vdisc_raymarch(flat.desc, 0, jobs[1][i], rd[i], jobs[3][i])
        assert e1 == err[i] and n1 == ns[i] and np.array_equal(c1, col[i])


def test_new_probe_bits_move_a_raymarch_and_nothing_else(grt, oracle, flat):
    jobs = V.march_jobs(flat.desc, curved=False)
    ref = V.oracle_march(oracle, flat.desc, jobs)[0]
    for mode in V.PROBES_VOL:
        moved = np.any(V.bits(V.oracle_march(oracle, flat.desc, jobs, mode)[0]) != V.bits(ref), axis=1)
        assert moved.mean() > 0.3, (mode, moved.mean())  # other last bits wherever the gas emitted
    # a scene without a VolumetricDisc: unchanged under both bits
    b = grt.SceneBuilder(L.GEOM_EUCLIDEAN).integration(2000, 100.0, 0.01, 1e-5)
    b.camera((0.0, 9.0, 0.0, 3.0), (1.0, 0.0, 0.0, 0.0), 0.7, 16, 16).celestial(grt.Checker(0.0, 9.0, 9.0, (0, 255, 0), (0, 90, 0)))
    b.add_disc(1.0, 3.0, grt.Checker(1.0, 5.0, 5.0, (255, 0, 0), (0, 0, 255)), 1000.0)
    d = b.build()
    base = oracle.render_pixels(d, 0, 0, 16, 16, threads=2)["xyza"]
    assert len(np.unique(base, axis=0)) > 2  # sky and both disc colours
    try:
        for mode in V.PROBES_VOL + (96,):
            oracle.lib().oracle_set_libm_perturbation(mode)
            assert np.array_equal(V.bits(oracle.render_pixels(d, 0, 0, 16, 16, threads=2)["xyza"]), V.bits(base))
    finally:
        oracle.lib().oracle_set_libm_perturbation(0)


# ------------------------------------------------- precondition of the GPU raymarch test --
def test_job_lists_are_robust_and_cover_the_cases(grt, oracle):
    for name, hs, jobs in V.march_cases(grt):
        ref, err, ns = V.oracle_march(oracle, hs.desc, jobs)
        robust = V.robust_jobs(oracle, hs.desc, jobs, ref)
        for n in V.JOB_SIZES:
            moved = int((~robust[:n]).sum())
            assert moved <= 0.02 * n, f"{name}: {moved} of the first {n} jobs move under the atan2 probes"
        obj, ro, dr, _ = jobs
        mx = np.array([hs.desc.objects[int(k)].march_max_steps for k in obj])
        assert np.any(ns == mx), f"{name}: no job reaches max_steps"
        rd = V.unit_rows(dr)
        uncached = [not oracle.vdisc_exit_distance(hs.desc, int(obj[i]), ro[i], rd[i])[0] for i in range(len(obj))]
        assert any(uncached), f"{name}: every job has a cached exit"
        lit = np.any(ref[:, :3] > 1e-3, axis=1)
        assert lit.mean() > 0.3, (name, lit.mean())  # colours well above `within`'s 1e-6 floor
        assert np.any(ns == 1) or np.any(~lit)
        if name == "two-gas":
            assert np.any(err != 0) and np.all(obj[err != 0] == 1)  # BelowRISCO inside object 1's rin .. r_isco
            assert set(obj[:64].tolist()) == {0, 1}
