"""Two instruction savings of the Schwarzschild integrate kernel that change no result bit,
restated for the host and checked there (CPU only).

* The RKF45 sums without their zero-weight k2 terms (geodesic_rkf.h rkf_attempt_fold, SHORT;
  weights from gr_raytracer_amd/csrc/device/rkf_weights.h).  CH2 = CT2 = 0.0, so with k2
  finite the full sum differs from the short one only where a -0 partial sum meets the +0
  product, and the difference survives to the result only as short -0 against full +0; the
  error term differs in the sign of a zero at most and enters as its square.  The checker
  (tests/native/rkf_zero_terms_check.cpp) runs all 11^7 combinations of y and a1..a6 from
  {+-0, +-1.5, +-5e-324, +-1e308, +-inf, NaN} and 10^7 random tuples, without contraction,
  with -ffp-contract=fast, and with every product fused explicitly into its add (what the
  fused device build does, whether or not the host compiler contracts).
* The unit-radius quotients of the region-B RHS (rcp_seed.h unit_radius_quotients): 1 / r,
  2 / r, 1 - 1 / r and 1 / (r r) from the refined reciprocals equal `/` bit for bit on 10^7
  operand sets in schw_div_ok's ranges, the edges planted, the reciprocal estimate modelled
  to 2^-20 (tests/native/unit_radius_check.cpp)."""
import subprocess

import pytest

from conftest import ROOT

DEV = ROOT / "gr_raytracer_amd" / "csrc" / "device"
NATIVE = ROOT / "tests" / "native"

BUILDS = {
    "exact": ["-ffp-contract=off"],
    "contract": ["-ffp-contract=fast"],
    "fused": ["-ffp-contract=off", "-DRKF_EXPLICIT_FMA"],
}


@pytest.fixture(scope="module")
def outdir(tmp_path_factory):
    return tmp_path_factory.mktemp("rkf_zero_terms")


@pytest.fixture(scope="module", params=list(BUILDS))
def rkf_checker(request, outdir):
    exe = outdir / f"rkf_zero_terms_check_{request.param}"
    subprocess.run(["g++", "-O2", "-std=c++17", *BUILDS[request.param], "-I", str(DEV),
                    str(NATIVE / "rkf_zero_terms_check.cpp"), "-o", str(exe)], check=True)
    return exe


def _run(exe, *args):
    out = subprocess.run([str(exe), *args], check=True, capture_output=True, text=True)
    return tuple(map(int, out.stdout.strip().splitlines()[-1].split())), out.stderr


def test_short_sums_equal_full_sums_on_the_grid(rkf_checker):
    (n, diff_yn, bad_yn, diff_e2), err = _run(rkf_checker, "grid")
    assert n == 8 * 11 ** 6  # a2 finite: 8 of its 11 values
    assert bad_yn == 0, err  # every differing yn is the short form's -0
    assert diff_e2 == 0, err
    # short -0 against full +0 does occur: the lemma's premise is needed.  (128 tuples without
    # contraction; 12 fused, where 5e-324 times a weight no longer rounds to a zero of its own)
    assert diff_yn > 0
    if "exact" in rkf_checker.name:
        assert diff_yn == 128
    print("grid", n, "tuples,", diff_yn, "differ in yn, all with the short result -0")


def test_short_sums_equal_full_sums_on_random_tuples(rkf_checker):
    (n, diff_yn, bad_yn, diff_e2), err = _run(rkf_checker, "random", "10000000", "0x5EED")
    assert n == 10_000_000
    assert bad_yn == 0, err
    assert diff_e2 == 0, err
    print("random", n, "tuples,", diff_yn, "differ in yn")


def test_unit_radius_quotients_equal_division(outdir):
    exe = outdir / "unit_radius_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", str(DEV),
                    str(NATIVE / "unit_radius_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), "10000000", "0x5EED"], check=True, capture_output=True, text=True)
    n, bad = map(int, out.stdout.strip().splitlines()[-1].split())
    assert n == 10_000_000
    assert bad == 0, out.stderr
