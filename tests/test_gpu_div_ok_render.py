"""The render's Schwarzschild division predicate (geodesic_rhs.h schw_div_ok_render: r above
the host's edge radius (1 + 2^-40) and below 2^100), on the GPU (marker `gpu`).

It admits a subset of schw_div_ok, whose range-free RHS tests/test_gpu_arith.py holds to
the IEEE form state by state.  Here the frames that the predicate steers are held to the
IEEE frames end to end (grt_debug_range_free off): at the shadow edge, where rays graze
and cross r = radius and the predicate changes within a wave, for the unit radius and for
radii whose product with 1 + 2^-40 rounds (0.7, 1.5, 2/3), so that the host's edge is not
the exact product.
"""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import SCENES, RESOURCES, c2_opts

pytestmark = pytest.mark.gpu

FRAME_KEYS = ("ray_class", "status", "stop_reason", "steps", "hits")


def _scene_with_radius(grt, tmp_path, radius):
    text = (SCENES / "schwarzschild.toml").read_text()
    new, k = re.subn(r"(?m)^(radius\s*=\s*)1\.0\s*$", lambda m: m.group(1) + repr(radius), text, count=1)
    assert k == 1
    p = tmp_path / f"schwarzschild-r{radius}.toml"
    p.write_text(new)
    hs = grt.HostScene(str(p), c2_opts(grt), str(RESOURCES))
    assert hs.desc.radius == radius
    return hs


def _frame(grt, hs, rect, range_free):
    fn = grt._lib.lib().grt_debug_range_free
    fn.restype = C.c_int
    fn.argtypes = [C.c_int]
    assert fn(1 if range_free else 0) == 0
    try:
        sc = grt.Scene(hs.desc_ptr(), keepalive=hs)
        return sc.render_pixels(*rect, aux=True)
    finally:
        fn(1)


@pytest.mark.parametrize("radius", [1.0, 0.7, 1.5, 2.0 / 3.0])
def test_shadow_edge_frames_equal_ieee_frames(grt, gpu, tmp_path, radius):
    hs = _scene_with_radius(grt, tmp_path, radius)
    rect = (750, 750, 4, 256)  # from the middle of the shadow outwards, across its edge for each radius
    a, b = _frame(grt, hs, rect, True), _frame(grt, hs, rect, False)
    assert np.array_equal(a.xyza64.view(np.uint64), b.xyza64.view(np.uint64))
    for k in FRAME_KEYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.stats["accepted_steps"] == b.stats["accepted_steps"] and a.stats["attempts"] == b.stats["attempts"]
    classes = np.bincount(a.ray_class, minlength=3)
    print("radius", radius, "classes", classes.tolist())
    assert (classes > 0).sum() >= 2, classes  # rays that fall in and rays that escape: the edge is in the crop
