"""The device's glibc pow / exp / sin / cos / sincos as the GPU compiles and runs them
(marker `gpu`).

grt_debug_glibc_device runs the wrappers the render calls -- rpow, rsin, rcos, rsincos,
the VolumetricDisc's sincos line, glibc::exp_, the region-B straight-line pair (unit 0:
geodesic.hip, tables staged in LDS) and opow (unit 1: output.hip, tables in constant
memory) -- on tests/glibc_inputs.py's sets.  The expectation is grt_debug_glibc_host, the
same glibc_math.h compiled for the host, which tests/test_glibc_math.py ties to glibc
bit for bit on the same sets; so this test does not depend on the GPU machine's libm.
What only the device build has is under test here: the LDS staging (strided copy, the
flattened table index, the barrier before a partial block's early return), the constant
tables, hipcc honouring -ffp-contract=off for the unit, and waves whose lanes split
between the fast path and the out-of-line OCML fallback."""
import functools

import numpy as np
import pytest

import glibc_inputs as GI

pytestmark = pytest.mark.gpu

CASES = [(fn, 0) for fn in sorted(GI.FN_NAMES)] + [(GI.FN_POW, 1)]
FALLBACK_CASES = [(fn, 0) for fn in GI.HAS_FALLBACK] + [(GI.FN_POW, 1)]
BLOCK_SETS = {"pow": ("render_random", "edge_y_log_x"), "trig": ("render_periods", "edge_thresholds"),
              "exp": ("render_subnormal_and_overflow", "edge_thresholds")}
FAST_POOL = {"pow": "render_controller_wide", "trig": "render_periods"}  # glibc_inputs._mixed's fast side


def _id(case):
    return f"{GI.FN_NAMES[case[0]]}-unit{case[1]}"


@pytest.fixture(scope="module")
def lib(grt):
    return grt._lib.lib()


def _check_against_host(lib, gpu, fn, unit, threads, name, x, y):
    """Device == host hook: the path byte on every lane, (out0, out1) wherever path != 0."""
    dev = GI.run_device(lib, gpu, unit, fn, threads, x, y)
    host = GI.run_host(lib, fn, x, y)
    what = (GI.FN_NAMES[fn], f"unit {unit}", f"{threads} threads", name)
    wrong_path = np.nonzero(dev[2] != host[2])[0]
    assert wrong_path.size == 0, (what, "path differs", wrong_path.size,
                                  [(float(x[i]).hex(), int(dev[2][i]), int(host[2][i])) for i in wrong_path[:5]])
    assert float((dev[2] != 0).mean()) == float((host[2] != 0).mean())
    n_bad, rows = GI.differing(x, y, dev, host, host[2] != 0)
    assert n_bad == 0, (what, n_bad, rows)
    return dev, host


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_device_is_bit_identical_to_the_host_restatement(lib, gpu, case):
    """(a) Every render, edge, off-path and mixed set: the device's path byte equals the
    host's on every lane (so the share of fast lanes is the same and the predicates agree)
    and out0 / out1 equal the host's bit for bit wherever path != 0 (NaN == NaN).  The
    controller pow sets and every trig render set are wholly on the fast path."""
    fn, unit = case
    family = GI.FAMILY[fn]
    for name, x, y in GI.all_sets(family):
        dev, _ = _check_against_host(lib, gpu, fn, unit, 256, name, x, y)
        if fn != GI.FN_SINCOS_B and name in GI.ALL_FAST[family]:
            assert (dev[2] == 1).all(), (GI.FN_NAMES[fn], name)


@pytest.mark.parametrize("fn", sorted(GI.FN_NAMES), ids=lambda f: GI.FN_NAMES[f])
def test_block_sizes_give_the_same_bits(lib, gpu, fn):
    """(b) Unit 0 with 64, 128, 192 and 256 threads per block (what grt_set_launch_config
    admits; tables_to_lds strides by blockDim.x) on one render and one edge set: each equals
    the host, and the four outputs equal each other on every lane, fallback lanes included."""
    family = GI.FAMILY[fn]
    sets = GI.SETS[family]()
    for name in BLOCK_SETS[family]:
        x, y = GI.args_of(family, sets[name])
        outs = [_check_against_host(lib, gpu, fn, 0, t, name, x, y)[0] for t in (64, 128, 192, 256)]
        for t, o in zip((128, 192, 256), outs[1:]):
            n_bad, rows = GI.differing(x, y, o, outs[0], np.ones(x.size, bool))
            assert n_bad == 0 and (o[2] == outs[0][2]).all(), (GI.FN_NAMES[fn], name, t, "vs 64 threads", n_bad, rows)


def _class_mismatch(got, want):
    """Lanes whose class differs: NaN, +-inf, +-0, or the sign of a non-NaN value."""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return (nan_g != nan_w) | (np.isinf(got) != np.isinf(want)) | ((got == 0) != (want == 0)) | \
        (~nan_g & ~nan_w & (np.signbit(got) != np.signbit(want)))


@pytest.mark.parametrize("case", FALLBACK_CASES, ids=_id)
def test_fallback_seam_in_mixed_and_off_path_waves(lib, gpu, case):
    """(c) Waves with lanes on both sides of the fast-path branch (periods 2 and 7), whole
    waves on either side (runs of 64), and the all-off-path sets.  Fast lanes keep the bits
    they have in a launch where every lane is fast (no register lost across the out-of-line
    OCML call, no lane on the wrong side).  Fallback lanes agree with the host libm in
    class (NaN, +-inf, +-0, sign) and in value to the project's bar, 1e-4 relative, plus 4
    subnormal spacings (4 * 2^-1074) for results that are themselves subnormal.  The largest
    ulp distance is printed (DESIGN.md records it); the bar is what is asserted."""
    fn, unit = case
    family = GI.FAMILY[fn]
    fx, fy = GI.args_of(family, GI.SETS[family]()[FAST_POOL[family]])
    all_fast = GI.run_device(lib, gpu, unit, fn, 256, fx, fy)
    assert (all_fast[2] == 1).all()
    sets = [(k, *GI.args_of(family, v if family == "pow" else v[0]), m) for k, (v, m) in GI.MIXED[family]().items()]
    sets += [(k, *GI.args_of(family, v), np.zeros(GI.N, bool)) for k, v in GI.SETS[family]().items()
             if k.startswith("offpath")]
    worst = 0.0
    for name, x, y, is_fast in sets:
        dev = GI.run_device(lib, gpu, unit, fn, 256, x, y)
        host = GI.run_host(lib, fn, x, y)
        what = (GI.FN_NAMES[fn], f"unit {unit}", name)
        assert ((host[2] == 1) == is_fast).all() and (dev[2] == host[2]).all(), what
        n_bad, rows = GI.differing(x, y, dev, all_fast, is_fast)
        assert n_bad == 0, (what, "fast lanes differ from the all-fast launch", n_bad, rows)
        off = ~is_fast
        for k in range(2 if fn in GI.TWO_OUTPUTS else 1):
            got, want = dev[k][off], host[k][off]  # the host's fallback lanes are its libm's values
            bad = np.nonzero(_class_mismatch(got, want))[0]
            assert bad.size == 0, (what, "class", bad.size, [(float(x[off][i]).hex(), None if y is None else float(y[off][i]).hex(),
                                                               float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]])
            fin = np.isfinite(want)
            err = np.abs(got[fin] - want[fin])
            tol = 1e-4 * np.abs(want[fin]) + 4 * 2.0 ** -1074
            far = np.nonzero(~(err <= tol))[0]
            assert far.size == 0, (what, "value", far.size, [(float(got[fin][i]).hex(), float(want[fin][i]).hex()) for i in far[:5]])
            if fin.any():
                worst = max(worst, float(GI.ulp_distance(got[fin], want[fin]).max()))
    print(f"glibc fallback seam: {GI.FN_NAMES[fn]} unit {unit}: largest distance to the host libm {worst:.0f} ulp")


def test_opow_and_rpow_agree_from_both_table_memories(lib, gpu):
    """(d) output.hip's opow (tables in constant memory) and geodesic.hip's rpow (tables in
    LDS) give the same path and, wherever it is the fast path, the same bits on every pow set."""
    for name, x, y in GI.all_sets("pow"):
        lds = GI.run_device(lib, gpu, 0, GI.FN_POW, 256, x, y)
        const = GI.run_device(lib, gpu, 1, GI.FN_POW, 256, x, y)
        assert (lds[2] == const[2]).all(), name
        n_bad, rows = GI.differing(x, y, const, lds, lds[2] != 0)
        assert n_bad == 0, (name, n_bad, rows)


def test_hook_rejects_what_it_cannot_launch(lib, gpu):
    x = np.ones(64)
    f = functools.partial(GI.run_device, lib, gpu)
    for unit, fn, threads in ((0, GI.FN_POW, 96), (0, GI.FN_POW, 512), (1, GI.FN_SIN, 256), (2, GI.FN_POW, 256), (0, 7, 256)):
        with pytest.raises(AssertionError):
            f(unit, fn, threads, x, x)
