"""The surface path's pieces beside the oracle, one by one (marker `gpu`).

The parity tests compare rendered pixels at 1e-4 after a curved-space integration.  Here the
device functions run alone through grt_debug_surface_points (api.hip, surface_points_kernel):
disc_chord, sphere_chord and window_far of geodesic.hip, and lut_index, compute_temperature,
sample_blackbody, texture_color and blend of appearance.h, one lane per input row, on the rows
of tests/surface_cases.py (tests/test_surface_checks_host.py holds their input conditions with
the oracle alone).  The kernel is the exact main unit's instantiation of the shared source, for
KerrBL scenes too (not the kerr_bl unit's code objects): every piece here is plain IEEE
arithmetic in an uncontracted build, so its bits do not depend on the unit.

Bars.  Chords: the oracle's hit flag on every row; t and the point on bits on every hit.
Window filter: wherever the device says far, the oracle's chord test of no object of the scene
hits; nothing on how tight it is.  lut_index: numpy's searchsorted.  Temperature: the oracle's
status, and its bits where the status is OK.  Blackbody and the blackbody texture: the oracle's
bits when it is handed the device's own log10(max(T, 10)) -- OCML's log10 is the one operation
there not meant to return glibc's bits, and the ROCm tree documents no bound for it, so its
distance from glibc's is recorded, not asserted.  Bitmap and checker textures: the oracle's
bits (NaN = NaN, +-0 = +-0) wherever the beaming factor is glibc's pow; the OCML pow rows
(redshift 0, negative, NaN, inf) are counted.  One positive finite redshift is outside
glibc::pow_fast, exactly 1.0 (y log x = 0 is glibc's special case for a tiny exponent, which
pow_fast leaves to OCML): pow(1, y) is exactly 1 in C99 and IEEE 754, so those rows are held to
the oracle's bits all the same, and every other positive finite redshift must take pow_fast.
Blend: the oracle's bits.

Measured on an MI355X: profiles/surface/points_check.json (tools/surface_points_record.py).
"""
import pytest

import surface_cases as S
from test_gpu_parity import gpu_scene

pytestmark = pytest.mark.gpu


def _pair(grt, hs):
    return hs, gpu_scene(grt, hs)


# ------------------------------------------------------------------------ chords --
@pytest.mark.parametrize("obj", [0, 1], ids=["disc", "sphere"])
def test_chords_equal_the_oracle(grt, oracle, gpu, obj):
    hs, sc = _pair(grt, S.chord_scene(grt))
    R = S.disc_rows() if obj == 0 else S.sphere_rows()
    m = S.chord_check(oracle, hs.desc, sc, gpu, obj, S.FN_DISC if obj == 0 else S.FN_SPHERE, R)
    print(m)
    assert m["hit_mismatch"] == 0 and m["bits_mismatch"] == 0, m
    assert 0.2 <= m["random_hit_share"] <= 0.9 and m["rows"] > 6000


# ----------------------------------------------------------------- window filter --
@pytest.mark.parametrize("kind", S.FAR_SCENES)
@pytest.mark.parametrize("chart", list(S.FAR_CHARTS))
def test_window_far_never_drops_a_hit(grt, oracle, gpu, chart, kind):
    hs, sc = _pair(grt, S.far_scene(grt, chart, kind))
    R = S.far_rows(chart)
    m, far, hit = S.far_check(oracle, hs.desc, sc, gpu, R)
    print(chart, kind, m)
    assert m["far_but_hit"] == 0, m
    assert 0.1 <= m["random_far_share"] <= 0.9, m
    assert 0 < m["refused_hits"] < m["refused"], m  # among the refused rows some hit and some do not
    if "disc" in kind:
        for k in S.LONG_RATIOS:  # hits of the disc at t = 1.0: refused, each of them
            assert m["long %g" % k]["oracle_hits"] > 0 and m["long %g" % k]["device_far_on_hits"] == 0, m


# ------------------------------------------------------------------------ tables --
@pytest.fixture(scope="module", params=S.LUT_SIZES)
def lut(request, grt):
    return _pair(grt, S.lut_scene(grt, request.param))


def test_lut_index_equals_searchsorted(gpu, lut):
    hs, sc = lut
    m = S.table_check(hs, sc, gpu, 0)
    print(m)
    assert m["mismatch"] == 0 and m["rows"] >= 60, m
    if hs.desc.objects[0].lut_n == S.LUT_SIZES[0]:  # the stock blackbody table, once
        m = S.table_check(hs, sc, gpu, -1)
        print(m)
        assert m["mismatch"] == 0 and m["rows"] > 3900, m


def test_temperature_equals_the_oracle(oracle, gpu, lut):
    hs, sc = lut
    radii = S.temperature_rows(hs)
    m = S.temperature_check(oracle, hs.desc, sc, gpu, 0, radii)
    print(m)
    assert m["status_mismatch"] == 0 and m["value_mismatch"] == 0, m
    assert m["statuses"] == [0, 3, 4] and m["ok_rows"] > 0.9 * m["rows"] - 20
    m = S.temperature_check(oracle, hs.desc, sc, gpu, 1, radii)  # the constant-temperature object
    assert m["status_mismatch"] == 0 and m["value_mismatch"] == 0 and m["statuses"] == [0], m


# --------------------------------------------------------------------- blackbody --
def test_blackbody_equals_the_oracle_given_its_log10(grt, oracle, gpu):
    hs, sc = _pair(grt, S.lut_scene(grt, 3))
    temps = S.blackbody_rows(hs.bb_log_t)
    m = S.blackbody_check(oracle, hs.desc, sc, gpu, temps)
    print(m)
    assert m["mismatch"] == 0 and m["rows"] >= 4000, m
    # nothing asserted on m["log10_rows_differing"] / m["log10_max_ulp"]: no bound of OCML's f64 log10
    # is documented in the ROCm tree; the record holds them


# ----------------------------------------------------------------------- texture --
@pytest.mark.parametrize("beaming", [0.0, 3.0])
@pytest.mark.parametrize("kind", list(S.TEX_OBJECTS))
def test_texture_equals_the_oracle(grt, oracle, gpu, kind, beaming):
    hs, sc = _pair(grt, S.texture_scene(grt, beaming))
    R = S.texture_rows(kind)
    m = S.texture_check(oracle, hs.desc, sc, gpu, kind, R)
    print(kind, beaming, m)
    assert m["mismatch"] == 0, m
    assert m["pow_fallback_on_positive_finite_redshift"] == 0, m  # (redshift == 1.0 apart: the docstring)
    assert m["redshift_one_rows"] >= 8
    assert m["pow_fallback_rows"] < 0.05 * m["rows"], m  # a small minority
    assert (m["pow_fallback_rows"] == 0) == (beaming == 0.0), m
    assert m["distinct_colours"] >= (2 if kind == "checker" else 2000)


# ------------------------------------------------------------------------- blend --
def test_blend_equals_the_oracle(grt, oracle, gpu):
    hs, sc = _pair(grt, S.chord_scene(grt))
    m = S.blend_check(oracle, sc, gpu, S.blend_rows())
    print(m)
    assert m["mismatch"] == 0 and m["rows"] > 4000, m
