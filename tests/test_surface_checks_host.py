"""The surface path's unit checks, CPU side: the argument tests of grt_debug_surface_points
(api.hip) that need no device, the oracle's array forms, and every input condition that
tests/test_gpu_surface_checks.py relies on, checked with the oracle alone -- the hit shares of
the random rows, a hit and a miss inside every edge family where the reference allows either,
the long windows being hits, refused-looking rows that hit and that miss, every table node
present -- so that a row list cannot go vacuous unnoticed.
"""
import numpy as np
import pytest

import surface_cases as S
from gr_raytracer_amd import _lib as L

EINVAL = -22


def _scene(grt, hs):
    return grt.Scene(hs.desc_ptr(), keepalive=hs)


@pytest.fixture(scope="module")
def chords(grt):
    return S.chord_scene(grt)


# -------------------------------------------------------------- argument validation --
def test_surface_points_arguments(grt, chords):
    sc = _scene(grt, chords)                      # object 0 a disc, object 1 a sphere, no blackbody table
    lut = S.lut_scene(grt, 3)
    sl = _scene(grt, lut)                         # object 0 a disc with a table, object 1 one without
    fn = S.points_fn()
    x, out, flag = np.zeros((4, 8)), np.zeros((4, 8)), np.zeros(4, np.uint8)
    args = (x.ctypes.data, out.ctypes.data, flag.ctypes.data)
    assert fn(None, 0, 0, S.FN_DISC, 4, *args) == EINVAL
    for bad_fn in (-1, S.FN_COUNT):
        assert fn(sc._s, 0, 0, bad_fn, 4, *args) == EINVAL
    for bad_obj in (-2, 2, 8):
        for f in range(S.FN_COUNT):
            assert fn(sc._s, 0, bad_obj, f, 4, *args) == EINVAL
    refused = [(sc, S.FN_DISC, 1), (sc, S.FN_DISC, -1), (sc, S.FN_SPHERE, 0), (sc, S.FN_SPHERE, -1),
               (sc, S.FN_FAR, 0), (sc, S.FN_BLEND, 1), (sc, S.FN_BB, -1), (sc, S.FN_BB, 0), (sc, S.FN_LUT, -1),
               (sc, S.FN_LUT, 0), (sc, S.FN_LUT, 1), (sc, S.FN_TEMP, -1), (sc, S.FN_TEMP, 1),
               (sl, S.FN_LUT, 1), (sl, S.FN_BB, 0)]
    for scene, f, obj in refused:
        assert fn(scene._s, 0, obj, f, 4, *args) == EINVAL, (f, obj)
    assert b"surface points" in L.lib().grt_last_error()
    accepted = [(sc, S.FN_DISC, 0), (sc, S.FN_SPHERE, 1), (sc, S.FN_FAR, -1), (sc, S.FN_BLEND, -1), (sc, S.FN_TEMP, 0),
                (sc, S.FN_TEX, -1), (sc, S.FN_TEX, 0), (sc, S.FN_TEX, 1), (sl, S.FN_LUT, 0), (sl, S.FN_LUT, -1),
                (sl, S.FN_TEMP, 0), (sl, S.FN_TEMP, 1), (sl, S.FN_BB, -1)]
    for scene, f, obj in accepted:
        for k in range(3):  # a null buffer is refused ...
            a = list(args)
            a[k] = None
            assert fn(scene._s, 0, obj, f, 4, *a) == EINVAL, (f, obj, k)
        assert fn(scene._s, 0, obj, f, 0, None, None, None) == 0, (f, obj)  # ... n = 0: nothing to do, no device


# ---------------------------------------------------------------- oracle additions --
def test_array_forms_equal_the_scalar_forms(grt, oracle, chords):
    rng = np.random.default_rng(5)
    d = chords.desc
    for obj, R in ((0, S.disc_rows()), (1, S.sphere_rows())):
        x = R.x
        hit, t, pt = oracle.object_intersects_n(d, obj, x[:, :3], x[:, 3:6])
        for i in rng.integers(0, len(x), 150):
            h1, p1, t1 = oracle.object_intersects(d, obj, [0.0, *x[i, :3]], [0.0, *x[i, 3:6]])
            assert h1 == hit[i] and (not h1 or (t1 == t[i] and np.array_equal(p1[1:], pt[i]))), x[i]
    kb = S.far_scene(grt, "kerr_bl", "disc")
    rows = S.far_rows("kerr_bl").x
    c = oracle.to_cartesian_n(kb.desc, rows[:, :3])
    for i in rng.integers(0, len(rows), 100):
        assert np.array_equal(S.bits(oracle.to_cartesian(kb.desc, [0.0, *rows[i, :3]])[1:]), S.bits(c[i]))
    ts = S.texture_scene(grt, 3.0)
    for kind, obj in S.TEX_OBJECTS.items():
        x = S.texture_rows(kind).x[:, :4]
        ref = oracle.texture_color_n(ts.desc, obj, x)
        for i in rng.integers(0, len(x), 100):
            assert np.all(S.same_bits(oracle.texture_color(ts.desc, obj, *x[i]), ref[i])), (kind, x[i])
    b = S.blend_rows().x
    ref = oracle.blend_n(b[:, :4], b[:, 4:])
    for i in rng.integers(0, len(b), 100):
        assert np.all(S.same_bits(oracle.blend(b[i, :4], b[i, 4:]), ref[i]))


def test_given_log_t_stands_in_for_log10(grt, oracle):
    """blackbody_n and texture_color_n with log_t = glibc's log10 are the plain forms, bit for bit;
    another log_t gives another colour."""
    hs = S.lut_scene(grt, 3)
    temps = S.blackbody_rows(hs.bb_log_t)
    assert len(temps) >= 4000
    lt = S.glibc_log10(np.fmax(temps, 10.0))
    plain = oracle.blackbody_n(hs.desc, temps)
    assert np.array_equal(S.bits(oracle.blackbody_n(hs.desc, temps, lt)), S.bits(plain))
    assert np.any(oracle.blackbody_n(hs.desc, temps, lt + 0.01) != plain)
    assert len(np.unique(plain, axis=0)) > 2000 and np.all(plain[:, 3] == 1.0)
    first, last = plain[np.isnan(temps)][0], plain[np.argmax(np.where(np.isfinite(temps), temps, 0.0))]
    for t in (0.0, -5.0, 10.0, np.inf, -np.inf):  # log10(inf) is not finite: the first entry (texture.rs:152)
        assert np.array_equal(plain[temps == t][0], first)
    assert not np.array_equal(first, last)
    assert np.any(np.all(plain == last, axis=1) & np.isfinite(temps))  # the table's upper end is reached
    ts = S.texture_scene(grt, 3.0)
    x = S.texture_rows("blackbody").x[:, :4]
    lt = S.glibc_log10(np.fmax(x[:, 3] * x[:, 2], 10.0))
    assert np.all(S.same_bits(oracle.texture_color_n(ts.desc, 1, x, lt), oracle.texture_color_n(ts.desc, 1, x)))
    # a bitmap and a checker do not read it
    for obj in (-1, 0):
        assert np.all(S.same_bits(oracle.texture_color_n(ts.desc, obj, x, lt + 1.0), oracle.texture_color_n(ts.desc, obj, x)))


# ------------------------------------------------------------------------ chord rows --
@pytest.mark.parametrize("obj", [0, 1], ids=["disc", "sphere"])
def test_chord_rows_cover_their_cases(oracle, chords, obj):
    R = S.disc_rows() if obj == 0 else S.sphere_rows()
    x = R.x
    assert len(x) <= 20000 and len(x[R.family["random"]]) >= 6000
    hit, t, pt = oracle.object_intersects_n(chords.desc, obj, x[:, :3], x[:, 3:6])
    assert 0.2 <= hit[R.family["random"]].mean() <= 0.9
    for name, sl in R.family.items():
        if R.mixed[name]:
            assert hit[sl].any() and not hit[sl].all(), name
    if obj == 0:
        th = t[hit]
        assert np.any(th == 1.0) and np.any(S.bits(th) == S.bits(0.0)) and np.any(S.bits(th) == S.bits(-0.0))
        rr = np.sum(pt[hit] ** 2, axis=1)
        assert np.any(rr == S.RIN ** 2) and np.any(rr == S.ROUT ** 2)  # rr lands on rin2 and rout2
        assert not hit[R.family["p2 = 0"]].any() and not hit[R.family["non-finite"]].any()
        assert not hit[R.family["|p1| = 2 |p2|"]].any()
        # quotients that underflow to -0 (a hit at t = -0): the rows the 1e-200 guard exists for
        assert np.any(S.bits(t[R.family["s.z x dz"]][hit[R.family["s.z x dz"]]]) == S.bits(-0.0))
    else:
        assert hit[R.family["end on the surface"]].mean() > 0.9  # t1 rounds past 1 on a few inside -> surface rows
        two = R.family["two roots"]
        assert hit[two].all() and np.all(t[two] > 0.0)  # the reference prefers t1, the far root
        assert not hit[R.family["zero length"]].any() and not hit[R.family["non-finite"]].any()
        assert np.any(t[R.family["tangent"]][hit[R.family["tangent"]]] == 0.0)


# ----------------------------------------------------------------------- window rows --
@pytest.mark.parametrize("chart", list(S.FAR_CHARTS))
def test_window_rows_cover_their_cases(grt, oracle, chart):
    R = S.far_rows(chart)
    x = R.x
    assert len(x) <= 20000 and len(x[R.family["random"]]) >= 8000
    r = x[R.family["random"]][:, [0, 3]]
    assert r.min() < 2e-3 and r.max() > 5e3
    th = x[R.family["random"]][:, [1, 4]]
    assert th.min() < -3.0 and th.max() > 6.0
    for kind in S.FAR_SCENES:
        hs = S.far_scene(grt, chart, kind)
        hit = S.oracle_window_hits(oracle, hs.desc, x)
        assert 0.01 < hit.mean() < 0.6, (kind, hit.mean())
        if "disc" in kind:
            for k in S.LONG_RATIOS:  # the long windows are hits of the disc
                assert hit[R.family["long %g" % k]].any(), (kind, k)
            m = hit[R.family["theta margins"]]
            assert m.any() and not m.all()
        if "sphere" in kind:
            e = hit[R.family["inner shell edge"]]
            assert e.any(), kind
            if chart == "kerr_bl":  # r < shell_lo <= r + |a| at an end inside the sphere
                lo, _ = S.shell_bounds()
                rows = x[R.family["inner shell edge"]][e]
                assert np.any((np.minimum(rows[:, 0], rows[:, 3]) < lo)), kind
            s = hit[R.family["across the shell"]]
            assert not s.any()  # both ends outside the sphere: the reference's own pre-test refuses them
        if "gas" in kind:
            g = hit[R.family["near the gas"]]
            assert 0.05 < g.mean() < 0.95
            assert hit[R.family["gas bounds"]].any() and not hit[R.family["gas bounds"]].all()


# ------------------------------------------------------------------------ table rows --
@pytest.mark.parametrize("lut_n", S.LUT_SIZES)
def test_table_rows_cover_their_cases(grt, oracle, lut_n):
    hs = S.lut_scene(grt, lut_n)
    o = hs.desc.objects[0]
    assert o.lut_n == lut_n == len(hs.lut_r) and np.all(np.diff(hs.lut_r) > 0) and hs.lut_r[0] == o.r_isco
    for a in (hs.lut_r, hs.bb_log_t):
        x = S.lut_index_rows(a)
        assert np.all((a[0] < x) & (x < a[-1])) and len(x) <= 20000
        assert set(a[1:-1]) <= set(x) and set(np.nextafter(a[1:], -np.inf)) <= set(x) and set(np.nextafter(a[:-1], np.inf)) <= set(x)
        assert set(0.5 * (a[:-1] + a[1:])) <= set(x)
        ref = S.lut_index_reference(a, x)
        assert set(ref) == set(range(len(a) - 1))  # every cell is asked for
    radii = S.temperature_rows(hs)
    status, val = oracle.compute_temperature_n(hs.desc, 0, radii)
    assert set(status.tolist()) == {0, 3, 4}  # GRT_OK, GRT_ERR_BELOW_RISCO, GRT_ERR_NON_FINITE_RADIUS
    assert status[radii == o.r_isco][0] == 0 and status[radii == np.nextafter(o.r_isco, 0.0)][0] == 3
    ok = status == 0
    assert np.all(val[ok] >= 0.0) and val[ok].max() == hs.lut_t.max() and len(np.unique(val[ok])) >= min(lut_n, 100)
    status, val = oracle.compute_temperature_n(hs.desc, 1, radii)  # the constant-temperature object
    assert not status.any() and np.all(val == 1234.5)


# ----------------------------------------------------------- texture and blend rows --
@pytest.mark.parametrize("kind", list(S.TEX_OBJECTS))
def test_texture_rows_cover_their_cases(grt, oracle, kind):
    R = S.texture_rows(kind)
    x = R.x[:, :4]
    assert len(x) <= 20000 and len(x[R.family["random"]]) >= 6000
    u = x[R.family["random"]][:, :2]
    assert u.min() < -0.49 and u.max() > 1.49
    z = x[:, 2]
    bad = ~((z > 0) & np.isfinite(z))
    assert 0 < bad.sum() < 0.05 * len(x)  # the OCML pow rows (exponent 3) are a small minority
    for zb in S.BAD_REDSHIFTS:
        assert np.any(S.same_bits(z, zb))
    ref0 = oracle.texture_color_n(S.texture_scene(grt, 0.0).desc, S.TEX_OBJECTS[kind], x)
    ref3 = oracle.texture_color_n(S.texture_scene(grt, 3.0).desc, S.TEX_OBJECTS[kind], x)
    fin = np.isfinite(ref0).all(1) & np.isfinite(ref3).all(1)
    assert fin.mean() > 0.9
    assert np.any(ref0[fin] != ref3[fin]) and np.array_equal(ref0[fin][:, 3], ref3[fin][:, 3])  # beaming leaves alpha
    assert len(np.unique(ref0[fin], axis=0)) >= (2 if kind == "checker" else 2000)
    if kind == "bitmap":
        w = 2048
        assert np.any(x[:, 0] * w == w) and np.any(x[:, 1] * w == w)  # the clamp at p_x == width
        px = x[:, 0] * w
        assert np.sum(np.floor(px) == np.ceil(px)) > 300  # ceil == floor
        assert np.isnan(ref0).any()
    if kind == "checker":
        sat = R.family["one axis saturates"]
        d0 = S.texture_scene(grt, 0.0).desc
        odd, even = oracle.texture_color_n(d0, 0, [[0.3, 0.05, 1.0, 0.0], [0.05, 0.05, 1.0, 0.0]])
        # the saturated index 2^64 - 1 is odd and the other one 0: always the second colour
        assert np.all(oracle.texture_color_n(d0, 0, x[sat]) == odd) and not np.array_equal(odd, even)
        assert np.all((x[sat][:, 0] * 5.0 >= 2.0 ** 64) ^ (x[sat][:, 1] * 7.0 >= 2.0 ** 64))


def test_blend_rows_cover_their_cases(oracle):
    R = S.blend_rows()
    x = R.x
    assert len(x[R.family["random"]]) == 4000
    a = x[R.family["random"]][:, [3, 7]]
    assert a.min() < -0.45 and a.max() > 1.45
    ref = oracle.blend_n(x[:, :4], x[:, 4:])
    assert not ref[R.family["both transparent"]].any()  # the (0, 0, 0, 0) arm
    assert np.isnan(ref[R.family["alpha"]]).any() and np.isnan(ref[R.family["non-finite colour"]]).any()
    al = x[R.family["alpha"]]
    assert np.any((al[:, 3] == 0.0) & (al[:, 7] == 1.0)) and np.any((al[:, 3] == 1.0) & (al[:, 7] == 0.0))
    assert len(np.unique(ref[R.family["random"]], axis=0)) > 3500  # both alphas <= 0 on 1 row in 16
