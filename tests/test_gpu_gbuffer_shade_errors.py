"""A temperature error raised at re-shade time, in every mode of the deferred shade (marker
`gpu`): the one branch of gbuffer_shade_ray the other g-buffer tests leave out.

The 24 x 20 buffer of the stock Schwarzschild case (tests/test_gpu_gbuffer.py; a Kerr-LUT disc)
is downloaded, and in a copy of `radius` three disc layers are edited: the last layer of a pixel
with two or more layers goes below the disc's r_isco (the frame has no such pixel that ends on
the disc, so one disc pixel is first given a copy of its layer as a second one), the first
layer of a second pixel becomes NaN and that of a third +inf.  The expectation is the rule the kernels document, not a run of
them: an edited pixel is the window error's pixel -- xyza (0, 0, 0, 1), class ESCAPED, status
GRT_ERR_BELOW_RISCO or GRT_ERR_NON_FINITE_RADIUS -- and every other pixel has the bits of the
UNEDITED buffer's static shade (at a time t: of the unedited buffer whose (u, v) went through the
host's restatement of the orbit rule, grt_gbuffer_orbit_uv, as in tests/test_gpu_gbuffer_orbit.py;
at t = 0 that is the unedited buffer itself).  All comparisons are exact.
"""
import numpy as np
import pytest

from test_gpu_gbuffer import COLS, ROWS, stock_case

pytestmark = pytest.mark.gpu

TIMES = (0.0, 37.5)
_CASE = {}


def case(grt):
    """The edited buffers, the edited pixels with their statuses, and the references, once."""
    if _CASE:
        return _CASE
    L = grt._lib
    hs, sc, _want, gb = stock_case(grt, "schwarzschild")
    info, a = gb.info, gb.arrays()
    shape = info.shape
    lut_disc = np.array([shape.objects[int(o)].kind == L.OBJ_DISC and shape.objects[int(o)].temp_kind != L.TEMP_CONSTANT
                         for o in a["object"]], bool)
    start = a["layer_start"].astype(np.int64)
    layers = np.diff(start)
    ok = a["status"] == 0
    multi = [p for p in np.flatnonzero(ok & (layers >= 2)) if lut_disc[start[p + 1] - 1]]
    first = [int(p) for p in np.flatnonzero(ok & (layers >= 1)) if lut_disc[start[p]]]
    print(f"{int(lut_disc.sum())} Kerr-LUT disc layers; {len(multi)} pixels with >= 2 layers ending on one, "
          f"{len(first)} pixels starting on one")
    assert len(first) >= 3
    edited, info_e = {k: v.copy() for k, v in a.items()}, type(info).from_buffer_copy(info)
    if multi:
        p_isco = int(multi[0])
    else:
        # at 24 x 20 no ray of this frame meets the disc after another hit: give one disc pixel a
        # second layer, a copy of its own, behind the first (the buffer is uploaded from arrays anyway)
        p_isco = first[len(first) // 2]
        k = int(start[p_isco + 1] - 1)
        for f in ("object", "u", "v", "redshift", "radius"):
            edited[f] = np.insert(edited[f], k + 1, edited[f][k])
        edited["layer_start"][p_isco + 1:] += 1
        info_e.n_layers += 1
    start_e = edited["layer_start"].astype(np.int64)
    assert start_e[p_isco + 1] - start_e[p_isco] >= 2
    others = [p for p in first if p != p_isco]
    p_nan, p_inf = others[0], others[-1]
    radius = edited["radius"]
    k_isco = int(start_e[p_isco + 1] - 1)
    r_isco = float(shape.objects[int(edited["object"][k_isco])].r_isco)
    assert r_isco > 0.0 and radius[k_isco] >= r_isco and radius[k_isco - 1] >= r_isco
    radius[k_isco] = 0.5 * r_isco
    radius[start_e[p_nan]] = np.nan
    radius[start_e[p_inf]] = np.inf
    want_status = {p_isco: L.ERR_BELOW_RISCO, p_nan: L.ERR_NON_FINITE_RADIUS, p_inf: L.ERR_NON_FINITE_RADIUS}

    def reference(t):  # the unedited buffer at time t, through the host rule and the static shade
        arrays = dict(a)
        arrays["u"], arrays["v"] = grt.gbuffer_orbit_uv(shape, a["object"], a["u"], a["v"], a["radius"], t)
        up = grt.GBuffer.from_arrays(info, arrays)
        out = up.shade(sc)
        up.close()
        return out

    ad = grt.scene.default_adaptive()
    ad.enabled = 0  # grt_gbuffer_shade_section's 1-spp pass alone
    _CASE.update(sc=sc, adaptive=ad, want_status=want_status, static=gb.shade(sc),
                 at={t: reference(t) for t in TIMES},
                 buffers=[grt.GBuffer.from_arrays(info_e, edited) for _ in range(2)])
    assert np.array_equal(_CASE["at"][0.0].xyza64.view(np.uint64), _CASE["static"].xyza64.view(np.uint64))
    # the edit changes something: none of the three pixels was an error pixel before
    assert all(_CASE["static"].status[p] == 0 for p in want_status)
    return _CASE


def check(grt, c, want, xyza64, cls, status, what, xyza=None):
    """The edited pixels are the window error's pixels; every other pixel has `want`'s bits."""
    L = grt._lib
    assert xyza64.shape == (ROWS * COLS, 4), what
    rest = np.ones(ROWS * COLS, bool)
    for p, st in c["want_status"].items():
        rest[p] = False
        assert status[p] == st, (what, p, status[p], st)
        assert cls[p] == L.CLASS_ESCAPED, (what, p, cls[p])
        assert np.array_equal(xyza64[p].view(np.uint64), np.array([0.0, 0.0, 0.0, 1.0]).view(np.uint64)), (what, p, xyza64[p])
        if xyza is not None:
            assert np.array_equal(xyza[p].view(np.uint32), np.array([0, 0, 0, 1], np.float32).view(np.uint32)), (what, p)
    assert np.array_equal(xyza64[rest].view(np.uint64), want.xyza64[rest].view(np.uint64)), (what, "xyza64")
    assert np.array_equal(cls[rest], want.ray_class[rest]), (what, "class")
    assert np.array_equal(status[rest], want.status[rest]), (what, "status")
    if xyza is not None:
        assert np.array_equal(xyza[rest].view(np.uint32), want.xyza[rest].view(np.uint32)), (what, "xyza")


def test_shade(grt, gpu):
    c = case(grt)
    got = c["buffers"][0].shade(c["sc"])
    check(grt, c, c["static"], got.xyza64, got.ray_class, got.status, "shade", got.xyza)


def test_shade_sequence(grt, gpu):
    c = case(grt)
    out = grt.shade_sequence(c["buffers"], c["sc"])
    assert out["xyza64"].shape[0] == 2
    for k in range(2):
        check(grt, c, c["static"], out["xyza64"][k], out["class"][k], out["status"][k], ("shade_sequence", k), out["xyza"][k])


def test_shade_orbit(grt, gpu):
    c = case(grt)
    out = c["buffers"][0].shade_orbit(c["sc"], TIMES)
    for k, t in enumerate(TIMES):
        check(grt, c, c["at"][t], out["xyza64"][k], out["class"][k], out["status"][k], ("shade_orbit", t), out["xyza"][k])


@pytest.mark.parametrize("time", [None, 0.0, 37.5])
def test_shade_section_one_sample_pass(grt, gpu, time):
    c = case(grt)
    frame, rep = c["buffers"][1].shade_section(c["sc"], adaptive=c["adaptive"], time=time)
    assert frame.n_supersampled == 0 and rep["n_selected"] == 0
    want = c["static"] if time is None else c["at"][time]
    check(grt, c, want, frame.xyza64, frame.ray_class, frame.status, ("shade_section", time))
