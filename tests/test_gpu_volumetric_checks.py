"""device/volumetric.h beside the oracle, piece by piece (marker `gpu`).

tests/test_gpu_volumetric.py compares rendered pixels, after a curved-space integration, a
window search and a composite.  Here the device functions run alone, through two debug
entries of api.hip: grt_debug_vdisc_points (perlin3, vdisc_density, vdisc_chord,
vdisc_exit_distance, vdisc_no_more_density, one lane per input) and grt_debug_vdisc_march
(the production march_kernel over a job list of the test's making: its size, its block
count, the exact or the fused kernel, slot or pool records).

Bars.  Perlin, density and crossings: the oracle's bits (the density with the device's own
atan2 handed to the oracle, oracle.vdisc_density_n(..., phi): OCML's atan2 is the one
operation there not meant to return glibc's bits).  The early end: wherever the device says
no more density, the oracle's density is 0 on every later sample.  The march: 1e-4 relative
per channel (test_gpu_parity.within) on every job the oracle's atan2 probes do not move --
at most 2 % move, tests/test_volumetric_checks_host.py -- and a job's colour has the same
bits in every list, block count and record form.

Measured on an MI355X (profiles/volumetric/march_check.json): see the record.
"""
import numpy as np
import pytest

import volumetric_cases as V
from gr_raytracer_amd import _lib as L
from test_gpu_parity import gpu_scene
from test_gpu_volumetric import compare

pytestmark = pytest.mark.gpu


def _pair(grt, hs):
    return hs, gpu_scene(grt, hs)


# ------------------------------------------------------------------------ Perlin --
@pytest.mark.parametrize("seed", V.SEEDS)
def test_perlin_equals_the_oracle(grt, oracle, gpu, seed):
    hs, sc = _pair(grt, V.flat_scene(grt, seed=seed))
    pts = V.perlin_points()
    assert 19000 <= len(pts) <= 22000
    out, _ = V.device_points(sc, gpu, 0, V.FN_PERLIN, pts)
    ref = oracle.perlin_n(seed, pts)
    bad = np.nonzero(~V.same_bits(out[:, 0], ref))[0]
    assert bad.size == 0, (bad.size, pts[bad[:4]], out[bad[:4], 0], ref[bad[:4]])
    assert np.mean(ref != 0.0) > 0.8 and np.abs(ref).max() <= 1.0


# ----------------------------------------------------------------------- density --
@pytest.mark.parametrize("axis", [V.TILT, V.ZAXIS], ids=["tilted", "z"])
@pytest.mark.parametrize("scene", ["flat", "schwarzschild"])
def test_density_equals_the_oracle(grt, oracle, gpu, scene, axis):
    hs, sc = _pair(grt, (V.flat_scene if scene == "flat" else V.schw_scene)(grt, axis))
    pts = V.density_points(oracle, hs.desc)
    m = V.density_check(oracle, hs.desc, sc, gpu, pts)
    print(m)
    assert m["n"] >= 18000 and m["positive"] > 0.2 * m["n"] and m["noise_points"] > m["positive"]
    for key in ("density_mismatch", "noise_flag_mismatch", "plane_xy_mismatch", "sincos_mismatch"):
        assert m[key] == 0, m
    # no bound of OCML's f64 atan2 is documented in the ROCm tree: nothing asserted on
    # m["atan2_max_ulp"]; the record holds the measured maximum


# --------------------------------------------------------------------- crossings --
@pytest.mark.parametrize("case", ["flat-tilted", "flat-z", "two-gas-1"])
def test_crossings_equal_the_oracle(grt, oracle, gpu, case):
    hs = V.two_gas_scene(grt) if case == "two-gas-1" else V.flat_scene(grt, V.TILT if case == "flat-tilted" else V.ZAXIS)
    k = 1 if case == "two-gas-1" else 0
    hs, sc = _pair(grt, hs)
    seg = V.segments(hs.desc, k)
    out, hit = V.device_points(sc, gpu, k, V.FN_CHORD, seg)
    want, t, pt = oracle.vdisc_intersects_n(hs.desc, k, seg[:, :3], seg[:, 3:])
    bad = np.nonzero(hit != want)[0]
    assert bad.size == 0, (bad.size, seg[bad[:4]])
    assert 0.2 < want.mean() < 0.9 and len(seg) > 5000
    same = (V.bits(out[want, 0]) == V.bits(t[want])) & np.all(V.bits(out[want, 1:4]) == V.bits(pt[want]), axis=1)
    assert same.all(), (int((~same).sum()), seg[want][~same][:4])
    rays = V.exit_rays(hs.desc, k)
    out, found = V.device_points(sc, gpu, k, V.FN_EXIT, rays)
    want, dist = oracle.vdisc_exit_distance_n(hs.desc, k, rays[:, :3], rays[:, 3:])
    bad = np.nonzero(found != want)[0]
    assert bad.size == 0, (bad.size, rays[bad[:4]])
    assert 0.2 < want.mean() < 0.95
    assert np.array_equal(V.bits(out[want, 0]), V.bits(dist[want]))


# --------------------------------------------------------------------- early end --
@pytest.mark.parametrize("case", ["flat-tilted", "flat-z", "two-gas-1"])
def test_no_more_density_means_no_density(grt, oracle, gpu, case):
    hs = V.two_gas_scene(grt) if case == "two-gas-1" else V.flat_scene(grt, V.TILT if case == "flat-tilted" else V.ZAXIS)
    k = 1 if case == "two-gas-1" else 0
    hs, sc = _pair(grt, hs)
    pairs = V.early_end_pairs(hs.desc, k)
    assert len(pairs) >= 5000
    _, flag = V.device_points(sc, gpu, k, V.FN_NO_MORE, pairs)
    assert 0.1 <= flag.mean() <= 0.9, flag.mean()
    o = hs.desc.objects[k]
    lit = oracle.vdisc_density_along_n(hs.desc, k, pairs[flag, :3], pairs[flag, 3:], o.march_step_size, o.march_max_steps)
    assert not lit.any(), (int(lit.sum()), pairs[flag][lit][:4])
    # the pairs the predicate refuses are not all trivially inside: some of them never meet density either
    dark = ~oracle.vdisc_density_along_n(hs.desc, k, pairs[~flag, :3], pairs[~flag, 3:], o.march_step_size, o.march_max_steps)
    assert dark.any() and not dark.all()


# ------------------------------------------------------------------------- march --
@pytest.fixture(scope="module")
def cases(grt, oracle):
    out = {}
    for name, hs, jobs in V.march_cases(grt):
        ref, err, ns = V.oracle_march(oracle, hs.desc, jobs)
        out[name] = (hs, gpu_scene(grt, hs), jobs, (ref, ns), V.robust_jobs(oracle, hs.desc, jobs, ref))
    return out


def _bar(m, n):
    assert m["max_rel_robust"] <= 1e-4, m["max_rel_robust"]  # test_gpu_parity.within on every robust job
    assert np.isfinite(m["col"]).all()  # every job was coloured
    assert int(m["counters"][0]) == n
    assert 0 < int(m["counters"][1]) <= m["oracle_samples"]  # the early end only removes samples
    assert m["counters"][3] <= m["counters"][2] <= m["counters"][1]


@pytest.mark.parametrize("name", ["flat", "schwarzschild", "two-gas"])
def test_march_equals_the_oracle_in_every_list(grt, oracle, gpu, cases, name):
    hs, sc, jobs, ref, robust = cases[name]
    assert robust.mean() >= 0.98
    full = V.march_check(oracle, hs.desc, sc, gpu, jobs, ref=ref, robust=robust)  # 300 jobs, 8 blocks
    _bar(full, 300)
    print(name, {k: full[k] for k in ("max_rel_robust", "bit_equal_share", "robust_share")})
    for n in V.JOB_SIZES:
        for blocks in (1, 8):
            m = V.march_check(oracle, hs.desc, sc, gpu, jobs, n=n, blocks=blocks, ref=ref, robust=robust)
            _bar(m, n)
            # a job's colour does not depend on the list it is in, nor on the block count
            assert np.array_equal(V.bits(m["col"]), V.bits(full["col"][:n])), (n, blocks)
    for n, blocks in ((300, 8), (65, 1), (1, 8)):  # the same jobs as JOB_POOL records of a HitPool
        m = V.march_check(oracle, hs.desc, sc, gpu, jobs, n=n, blocks=blocks, as_pool=True, ref=ref, robust=robust)
        _bar(m, n)
        assert np.array_equal(V.bits(m["col"]), V.bits(full["col"][:n])), ("pool", n, blocks)
    # more blocks than chunks of 64
    m = V.march_check(oracle, hs.desc, sc, gpu, jobs, n=65, blocks=64, ref=ref, robust=robust)
    assert np.array_equal(V.bits(m["col"]), V.bits(full["col"][:65]))
    # the oracle's (0, 0, 0, 0) arm where the temperature fails
    err = V.oracle_march(oracle, hs.desc, jobs)[1]
    if name == "two-gas":
        assert np.any(err != 0)
    assert not full["col"][err != 0].any()


@pytest.mark.parametrize("name", ["flat", "schwarzschild"])
def test_fused_march_stays_within_the_bar(grt, oracle, gpu, cases, name):
    hs, sc, jobs, ref, robust = cases[name]
    exact = V.march_check(oracle, hs.desc, sc, gpu, jobs, ref=ref, robust=robust)
    for n, blocks in ((300, 8), (65, 1)):
        m = V.march_check(oracle, hs.desc, sc, gpu, jobs, arith=1, n=n, blocks=blocks, ref=ref, robust=robust)
        _bar(m, n)
    print(name, "fused", {k: m[k] for k in ("max_rel_robust", "bit_equal_share")})
    m = V.march_check(oracle, hs.desc, sc, gpu, jobs, arith=1, ref=ref, robust=robust)
    assert not np.array_equal(V.bits(m["col"]), V.bits(exact["col"]))  # the contracted kernel ran


@pytest.mark.parametrize("lut_n", [(1500, 1500), (1500, 1000)], ids=["none-staged", "second-staged"])
def test_march_reads_long_luts_from_global_memory(grt, oracle, gpu, lut_n):
    """Tables longer than 1000 entries are not staged in LDS: with both gases' long, march_kernel reads
    both from global memory; with only object 0's long, it stages object 1's and the first pass reads
    global memory."""
    hs, sc = _pair(grt, V.two_gas_scene(grt, lut_n=lut_n))
    assert (hs.desc.objects[0].lut_n, hs.desc.objects[1].lut_n) == lut_n
    jobs = V.march_jobs(hs.desc, objects=(0, 1), seed=2)
    full = V.march_check(oracle, hs.desc, sc, gpu, jobs)
    assert full["robust_share"] >= 0.98
    _bar(full, 300)
    one = V.march_check(oracle, hs.desc, sc, gpu, jobs, n=129, blocks=1)
    assert np.array_equal(V.bits(one["col"]), V.bits(full["col"][:129]))


def test_two_gases_end_to_end(grt, oracle, gpu):
    """One 48 x 48 Euclidean frame of the two-gas scene: the gather of the jobs of two objects,
    two passes of march_kernel and the composite."""
    hs = V.two_gas_scene(grt, L.GEOM_EUCLIDEAN)
    got, ref = compare(grt, oracle, hs, (0, 0, 48, 48))
    assert got.stats["march_jobs"] > 200 and got.stats["march_emit_samples"] > 0
    assert np.any(got.ray_class == 0) and len(np.unique(got.xyza64, axis=0)) > 100
