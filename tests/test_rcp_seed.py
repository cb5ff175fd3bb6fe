"""The seeded reciprocals of the region-B Schwarzschild RHS
(gr_raytracer_amd/csrc/device/rcp_seed.h), compiled for the host without contraction: every
quotient equals the compiler's `/` bit for bit (CPU only).

The RHS takes 1 / (r r) from its refined 1 / r with one Newton step instead of a fresh
reciprocal estimate and two.  The checker (tests/native/rcp_seed_check.cpp) models the
hardware's estimate as (1 / y)(1 + e) with |e| up to 2^-20, looser than any plausible
v_rcp_f64, and draws 10^7 operand sets in the ranges of schw_div_ok and region B, a share
of them on the edges: |r| at 2^+-100, r next to radius, |a| at 2^-42, sin at 0.75 and 1,
|cos| down to 2^-55."""
import subprocess

import pytest

from conftest import ROOT

DEV = ROOT / "gr_raytracer_amd" / "csrc" / "device"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rcp_seed") / "rcp_seed_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", str(DEV),
                    str(ROOT / "tests" / "native" / "rcp_seed_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_seeded_reciprocals_give_the_quotients_of_division(checker):
    out = subprocess.run([str(checker), "10000000", "0x5EED"], check=True, capture_output=True, text=True)
    n, bad = map(int, out.stdout.strip().splitlines()[-1].split())
    assert n == 10_000_000
    assert bad == 0, out.stderr
