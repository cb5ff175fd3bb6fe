"""The Schwarzschild integrate kernel's steady far-field loop, on the GPU (marker `gpu`).

A wave whose quick step leaves every lane at h == 1 stays in a loop of unit attempts and
reduced tests (geodesic.hip steady_step_mask) and leaves it for the general path when a lane
misses the test; the wave votes are compared as lane masks (wave_all, with_sincos<VOTES>).
Neither changes a result, so every array of every frame here is held to the oracle (or to
the same frame rendered another way) bit for bit, every pixel:

* the loop's entry, its exit and the last-step rule i == max_steps - 1 for budgets that put
  the last step on the general path, on the loop's first iteration and on later ones;
* lanes refilled next to lanes inside the loop (a grid smaller than the frame);
* grt_debug_rkf_short 0 / 1 / 2: mode 0 never enters the loop, mode 2 enters it and takes the
  full attempt again on leaving;
* a radius without the unit-radius form and one outside the range-free divisions' range,
  which take the other RHS forms through the same dispatch.
"""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import SCENES, RESOURCES, c2_opts, host_scene

pytestmark = pytest.mark.gpu

ORACLE_THREADS = 16
HIT = 2  # _lib.CLASS_HIT
FRAME_KEYS = ("ray_class", "status", "stop_reason", "steps", "hits")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


HIT_COLOUR_TOL = 1e-10


def _assert_equals_oracle(got, ref, rows=None, hits_exact=True):
    """Class, status, stop reason and per-ray step counts equal, and xyza (f64) bit for bit.
    hits_exact=False: the colour of a ray that hit an object within HIT_COLOUR_TOL instead.
    The trace is the oracle's bit for bit, the surface shade is not: its texture coordinates
    come from the device's atan2 / acos, an ulp or two from glibc's, and an ulp of a coordinate
    is 2^-52 x 2^13 texels = 2e-12 of a texel step, of colours of order 1.  1e-10 leaves room
    for a few such terms; the crop's 74 differing hit pixels of 1,280 were measured at up to
    8.3e-13, and the parent commit's frame has the same bits."""
    sel = slice(None) if rows is None else rows
    for key, mine in (("ray_class", got.ray_class), ("status", got.status), ("stop", got.stop_reason),
                      ("steps", got.steps)):
        assert np.array_equal(mine[sel], ref[key]), key
    mine, want = got.xyza64[sel], ref["xyza"]
    exact = np.ones(len(want), bool) if hits_exact else ref["ray_class"] != HIT
    assert np.array_equal(_bits(mine[exact]), _bits(want[exact]))
    err = np.abs(mine[~exact] - want[~exact])
    print("hit pixels", int((~exact).sum()), "max colour difference", float(err.max()) if err.size else 0.0)
    assert np.all(err <= HIT_COLOUR_TOL * np.maximum(np.abs(want[~exact]), 1.0))


def _assert_same_frames(a, b):
    assert np.array_equal(_bits(a.xyza64), _bits(b.xyza64))
    for k in FRAME_KEYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def _render(grt, hs, rect):
    return grt.Scene(hs.desc_ptr(), keepalive=hs).render_pixels(*rect, aux=True)


@pytest.mark.parametrize("max_steps", [2, 3, 4, 5, 6, 7, 8, 1001, 1002])
def test_entry_exit_and_last_step(grt, oracle, gpu, max_steps):
    """C2, a 13 x 11 rectangle on the shadow edge (partial 8 x 8 tiles: some lanes of each wave
    hold no ray).  A ray starts at h = step_size = 0.01 and h grows fourfold per far-field step
    (0.01, 0.04, 0.16, 0.64, then 1.0), so steps 1 .. 4 are quick steps of the general
    iteration, the fourth one enters the loop, and step 5 is the loop's first iteration.  The
    last step i == max_steps - 1 falls on the general iteration (2 .. 5), on the loop's first
    iteration (6) and on later ones of both parities (7, 8; 1001, 1002, where the captured
    rays have ended long before and left their waves' lanes idle)."""
    hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt, max_steps=max_steps))
    assert hs.desc.step_size == 0.01
    rect = (738, 884, 13, 11)
    got = _render(grt, hs, rect)
    ref = oracle.render_pixels(hs.desc, *rect, threads=ORACLE_THREADS)
    print("max_steps", max_steps, "classes", np.bincount(got.ray_class, minlength=3).tolist(),
          "steps", int(ref["steps"].min()), int(ref["steps"].max()), "attempts", got.stats["attempts"])
    _assert_equals_oracle(got, ref)
    assert got.stats["accepted_steps"] == int(ref["steps"].astype(np.int64).sum())
    assert int(ref["steps"].max()) == max_steps - 1  # some ray runs into the budget
    if max_steps > 1000:
        assert int(ref["steps"].min()) < max_steps - 1  # and some ray ends before it


def test_refill_next_to_rays_in_the_loop(grt, oracle, gpu):
    """A 160 x 128 C2 crop across the shadow edge and the disc's rim, with the default launch
    and with one 64-thread block per CU (16,384 lanes for 20,480 rays: waves refill lanes
    while their neighbours are mid-flight, so the loop is left and entered again).  The two
    frames are equal array for array with equal step totals, and rows 0 mod 16 equal the
    oracle's (_assert_equals_oracle: the trace bit for bit, the disc's colours within
    HIT_COLOUR_TOL)."""
    assert HIT == grt._lib.CLASS_HIT
    hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt))
    rect = (700, 840, 128, 160)
    a = _render(grt, hs, rect)
    lib = grt._lib.lib()
    try:
        grt._lib.check(lib.grt_set_launch_config(1, 64), "grt_set_launch_config")
        b = _render(grt, hs, rect)
    finally:
        lib.grt_set_launch_config(0, 0)
    _assert_same_frames(a, b)
    assert a.stats["accepted_steps"] == b.stats["accepted_steps"] and a.stats["attempts"] == b.stats["attempts"]
    cls = np.bincount(a.ray_class, minlength=3)
    print("classes", cls.tolist(), "steps", a.stats["accepted_steps"], "attempts", a.stats["attempts"])
    assert (cls > 0).all(), cls  # captured, escaped and disc hits: the edge and the rim are in the crop
    rows, cols = rect[2], rect[3]
    for r in range(0, rows, 16):
        ref = oracle.render_pixels(hs.desc, rect[0] + r, rect[1], 1, cols, threads=ORACLE_THREADS)
        _assert_equals_oracle(a, ref, slice(r * cols, (r + 1) * cols), hits_exact=False)


def test_debug_modes(grt, gpu):
    """The 16 x 16 smoke crop with grt_debug_rkf_short 0, 1 and 2: equal frames, and equal
    attempt counts (mode 0 counts its full attempts, once each; mode 2 does not count the
    full attempt it takes over the short one)."""
    hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt))
    fn = grt._lib.lib().grt_debug_rkf_short
    fn.restype = C.c_int
    fn.argtypes = [C.c_int]
    frames = {}
    try:
        for mode in (0, 1, 2):
            assert fn(mode) == 0
            frames[mode] = _render(grt, hs, (740, 740, 16, 16))
    finally:
        fn(1)
    for mode in (0, 2):
        _assert_same_frames(frames[1], frames[mode])
        assert frames[mode].stats["attempts"] == frames[1].stats["attempts"], mode
        assert frames[mode].stats["accepted_steps"] == frames[1].stats["accepted_steps"], mode
    assert frames[1].stats["attempts"] >= frames[1].stats["accepted_steps"] > 0


def _scene_with_radius(grt, tmp_path, toml, radius, objects):
    """The scene `toml` with its geometry's radius replaced and only its objects[objects:] kept."""
    text = (SCENES / toml).read_text()
    new, k = re.subn(r"(?m)^(radius\s*=\s*)[01]\.0\s*$", lambda m: m.group(1) + repr(radius), text, count=1)
    assert k == 1
    blocks = [m.start() for m in re.finditer(r"(?m)^\[\[objects\]\]", new)]
    new = new[:blocks[0]] + new[blocks[objects]:]
    p = tmp_path / f"{toml[:-5]}-r{radius}.toml"
    p.write_text(new)
    hs = grt.HostScene(str(p), c2_opts(grt), str(RESOURCES))
    assert hs.desc.radius == radius
    return hs


@pytest.mark.parametrize("toml,radius,objects,rect", [
    ("schwarzschild.toml", 2.0, 0, (736, 972, 16, 16)),
    ("schwarzschild-sphere.toml", 2.0 ** -60, 1, (740, 622, 16, 16)),
])
def test_other_rhs_forms(grt, oracle, gpu, tmp_path, toml, radius, objects, rect):
    """Radius 2.0 (range-free divisions, no unit-radius form), the C2 scene at its shadow's
    edge; and radius 2^-60, outside the range-free divisions' 2^+-50, so the IEEE divisions in
    every region-B case:
    the sphere scene without its disc (no disc temperature table exists for that radius), a
    crop of rays that graze the sphere within two pixels of its limb (a shell test in the
    loop, which they leave and enter again) and escape.  Neither crop holds a surface hit, so
    every colour is the oracle's bit for bit."""
    hs = _scene_with_radius(grt, tmp_path, toml, radius, objects)
    got = _render(grt, hs, rect)
    ref = oracle.render_pixels(hs.desc, *rect, threads=ORACLE_THREADS)
    cls = np.bincount(got.ray_class, minlength=3)
    print("radius", radius, "classes", cls.tolist(), "steps", got.stats["accepted_steps"])
    _assert_equals_oracle(got, ref)
    assert got.stats["accepted_steps"] == int(ref["steps"].astype(np.int64).sum())
    assert cls[grt._lib.CLASS_HIT] == 0 and (radius != 2.0 or (cls > 0).sum() == 2), cls
