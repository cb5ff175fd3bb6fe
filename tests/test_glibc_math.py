"""The device pow (gr_raytracer_amd/csrc/device/glibc_math.h), compiled for the host,
returns glibc's pow bits on its whole fast path (CPU only).

f64::powf in the reference is glibc pow; on x86-64 with FMA glibc 2.35 runs
__pow_fma, whose operation sequence glibc_math.h restates.  The tables come from the
installed libm (tools/gen_glibc_tables.py); this test re-derives them too, so a libm
update that changes them is caught here."""
import subprocess

import pytest

from conftest import ROOT

DEV = ROOT / "gr_raytracer_amd" / "csrc" / "device"
MODES = {0: "controller eps/err over 1e-304..1e304, y = 1/5", 1: "controller range", 2: "beaming exponents",
         3: "x near 1", 4: "random normal x, |y| < 2"}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("glibc") / "check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", str(DEV),
                    str(ROOT / "tests" / "native" / "glibc_pow_check.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("mode", sorted(MODES))
def test_device_pow_is_bit_identical_to_glibc(checker, mode):
    out = subprocess.run([str(checker), str(mode), "400000"], check=True, capture_output=True, text=True).stdout
    n, fast, bad = map(int, out.strip().splitlines()[-1].split())
    assert bad == 0, out
    assert fast >= 0.7 * n, (MODES[mode], fast, n)
    if mode in (0, 1):
        assert fast == n  # the controller's inputs are always on the fast path


def test_tables_match_the_installed_libm():
    gen = subprocess.run(["python3", str(ROOT / "tools" / "gen_glibc_tables.py")], check=True, capture_output=True,
                         text=True).stdout
    assert gen == (DEV / "glibc_tables.h").read_text()


TRIG_MODES = {0: "ray theta", 1: "several periods", 2: "magnitudes 2^-41..2^19", 3: "near pi/2",
              4: "up to the reduction limit", 5: "(-pi, pi): VolumetricDisc phi",
              6: "pi/2 +- 0.15 (region B, Taylor and table)"}


def _build(tmp_path_factory, name, extra=()):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", str(DEV),
                    str(ROOT / "tests" / "native" / f"{name}.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def trig_checkers(tmp_path_factory):
    # -fno-builtin: sin(x) and cos(x) must reach glibc's sin / cos, not a fused sincos
    return (_build(tmp_path_factory, "glibc_trig_check", ("-fno-builtin-sin", "-fno-builtin-cos")),
            _build(tmp_path_factory, "glibc_sincos_check"))


@pytest.mark.parametrize("mode", sorted(TRIG_MODES))
def test_device_sin_cos_sincos_are_bit_identical_to_glibc(trig_checkers, mode):
    """sin_fast / cos_fast == glibc sin / cos (FMA ifunc builds); sincos_fast and its
    branch-free variant sincos_fast_uniform == glibc sincos (baseline build), on
    |x| < 105414350."""
    for exe in trig_checkers:
        out = subprocess.run([str(exe), str(mode), "300000"], check=True, capture_output=True, text=True).stdout
        n, fast, bad = map(int, out.strip().splitlines()[-1].split())
        assert bad == 0, (exe.name, out)
        assert fast == n, (exe.name, TRIG_MODES[mode], fast, n)


EXP_MODES = {0: "vertical falloff -(h/thickness)^2", 1: "boundary falloff -1/max(d^2, 1e-4)",
             2: "attenuation over 60 decades", 3: "subnormal results and the overflow edge", 4: "random bit patterns"}


@pytest.fixture(scope="module")
def exp_checker(tmp_path_factory):
    return _build(tmp_path_factory, "glibc_exp_check", ("-fno-builtin-exp",))


@pytest.mark.parametrize("mode", sorted(EXP_MODES))
def test_device_exp_is_bit_identical_to_glibc(exp_checker, mode):
    """exp_ == glibc exp (__exp_fma) on every input, including the special cases (the
    VolumetricDisc raymarch's falloffs and attenuations, volumetric_disc.rs:97-138, :242-272)."""
    out = subprocess.run([str(exp_checker), str(mode), "400000"], check=True, capture_output=True, text=True).stdout
    n, _, bad = map(int, out.strip().splitlines()[-1].split())
    assert bad == 0, (EXP_MODES[mode], out)


# ------------------------------------------------- the host hook on the shared sets ----
# grt_debug_glibc_host (csrc/host/glibc_check.cpp, in libgrt.so; no GPU) evaluates the same
# glibc_math.h through the render's wrappers on tests/glibc_inputs.py's sets: the random
# modes above restated, every branch threshold +- a few ulps, and what the fast paths
# refuse.  tests/test_gpu_glibc_math.py holds the device to this hook bit for bit; here the
# hook is tied to the installed libm.  Bit identity holds for glibc 2.35 on x86-64 with FMA
# (sin / cos / exp / pow: the FMA ifunc builds; sincos: the baseline build), the libm
# test_tables_match_the_installed_libm insists on.
import glibc_inputs as GI  # noqa: E402


@pytest.mark.parametrize("fn", sorted(GI.FN_NAMES), ids=lambda f: GI.FN_NAMES[f])
def test_host_hook_is_bit_identical_to_libm_on_the_shared_sets(grt, fn):
    """Wherever the hook takes a glibc_math.h path (path != 0) its (out0, out1) are the
    bits of this libm's pow / sin / cos / sincos / exp (sincos for the VolumetricDisc line
    and the region-B pair), on every render, edge, off-path and mixed set; exp_ on every
    lane.  The sets reach both sides of every threshold, and the render sets that must be
    all fast are."""
    import os

    import numpy as np

    lib = grt._lib.lib()
    family = GI.FAMILY[fn]
    libc = os.confstr("CS_GNU_LIBC_VERSION")
    shares = {}
    for name, x, y in GI.all_sets(family):
        assert x.size == GI.N and x.size % 64 != 0
        got = GI.run_host(lib, fn, x, y)
        want = GI.run_host(lib, fn | GI.FN_LIBM, x, y)
        assert (want[2] == 0).all()
        on = got[2] != 0
        n_bad, rows = GI.differing(x, y, got, want, on)
        assert n_bad == 0, (GI.FN_NAMES[fn], name, libc, n_bad, rows)
        shares[name] = float(on.mean())
        if fn == GI.FN_EXP:
            assert on.all()
        elif fn != GI.FN_SINCOS_B and name in GI.ALL_FAST[family]:
            assert on.all(), (GI.FN_NAMES[fn], name, shares[name])
        elif fn != GI.FN_SINCOS_B and name.startswith("offpath"):
            assert not on.any(), (GI.FN_NAMES[fn], name, shares[name])
    print(GI.FN_NAMES[fn], libc, "fast share per set:", shares)
    if fn == GI.FN_POW:  # both sides of |y log x| = 2^-54 / 512 and of the table split
        assert 0.2 < shares["edge_y_log_x"] < 0.8 and 0.3 < shares["edge_x_table"] < 1.0
        assert shares["edge_y_limits"] == 0.0  # |y| at 2^-65 / 2^63: y log x is out of range either way
    elif fn == GI.FN_SINCOS_B:  # both region-B forms on either side of |a| = TAYLOR_MAX
        p = GI.run_host(lib, fn, GI.trig_sets()["edge_region_b_taylor"])[2]
        assert (p[:GI.N // 2] == 1).sum() > 100 and (p[:GI.N // 2] == 2).sum() > 100
        assert set(np.unique(GI.run_host(lib, fn, GI.trig_sets()["render_region_b"])[2])) == {1, 2}
    elif family == "trig":  # the reduction limit's neighbours fall on both sides
        assert 0.5 < shares["edge_thresholds"] < 1.0
