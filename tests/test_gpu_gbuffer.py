"""The geometry buffer on the GPU (grt_gbuffer_*; marker `gpu`): trace a rectangle once,
shade it again under any appearance.

The reference of every comparison but the oracle tie is the existing single-frame path
(`render_pixels` of the scene whose appearance is applied), and the comparisons are exact:
array_equal on the f32 / f64 bits, class and status.  The deferred shade runs the shade
kernel's operations on the numbers that kernel had in registers, so no tolerance is involved.

Frames are 24 cols x 20 rows (rows % 8 != 0, two blocks of the tile grid in each direction),
the winding frames 96 x 96 (tests/test_hit_pool.py).
"""
import ctypes as C
import errno
import math
import subprocess

import numpy as np
import pytest

from conftest import RESOURCES, ROOT, SCENES

pytestmark = pytest.mark.gpu

ROWS, COLS = 20, 24
GRT = ROOT / "gr_raytracer_amd" / "lib" / "grt"


# ------------------------------------------------------------------------ scenes ----
def stock(grt, toml, **opts):
    """A stock TOML scene at 24 x 20: (host scene, device scene)."""
    o = grt.GlobalOpts(width=COLS, height=ROWS, **opts)
    hs = grt.HostScene(str(SCENES / toml), o, str(RESOURCES))
    return hs, grt.Scene(hs.desc_ptr(), keepalive=hs, adaptive=hs.adaptive)


STOCK = {
    "schwarzschild": ("schwarzschild.toml", dict(camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=100000)),
    "kerr-bl": ("kerr-bl.toml", dict(camera_position=(-10.0, 0.0, -0.5), theta=-3.14159, max_steps=1000000)),
    # the step budget and celestial radius of the sequence tests' Kerr-Schild frames
    "kerr-schild": ("kerr.toml", dict(camera_position=(-10.0, 0.0, -0.5), theta=1.52, psi=-1.57, max_steps=10000,
                                      max_radius=100.0)),
    "euclidean": ("euclidean.toml", dict()),
    "euclidean-spherical": ("euclidean-spherical.toml", dict()),
    # the camera inside the sphere (radius 2 at the origin): every ray leaves it once
    "schwarzschild-sphere": ("schwarzschild-sphere.toml", dict(camera_position=(-1.0, 0.0, 0.3), theta=-3.142,
                                                               max_steps=100000)),
}


def _bitmap(grt, seed, beaming, alpha_lo=0):
    rng = np.random.default_rng(seed)
    rgba = rng.integers(0, 256, (9, 13, 4)).astype(np.uint8)
    rgba[..., 3] = rng.integers(alpha_lo, 256, (9, 13))
    return grt.Bitmap(beaming, rgba)


def _set_alpha(tex, a1, a2):
    tex.c1[3], tex.c2[3] = a1, a2


def reshade_pair(grt, name):
    """(descriptor A, descriptor B): B has A's geometry, object shapes, camera and integration
    parameters, and everything that is free to differ changed -- bitmap <-> checker <->
    blackbody textures, a semi-transparent checker (alpha 0.5) so that several layers blend,
    other beaming exponents, disc and sphere temperatures, celestial texture and temperature,
    and hit threshold."""
    L = grt._lib
    out = []
    for alt in (False, True):
        if name == "schwarzschild":  # Kerr-LUT disc (Schwarzschild's temperature model) and a sphere
            b = grt.SceneBuilder(L.GEOM_SCHWARZSCHILD, radius=1.0, a=0.0, horizon_epsilon=1e-4)
            b.integration(20000, 100.0, 0.01, 1e-5)
            pos = grt.cartesian_to_spherical((0.0, -14.0, 0.0, 1.2))
            b.camera(pos, grt.stationary_velocity(L.GEOM_SCHWARZSCHILD, 1.0, 0.0, pos), math.pi / 4, ROWS, COLS, 0.0,
                     -3.142, 0.0)
            # the sphere between the camera and the hole: a ray enters and leaves it (two layers),
            # and many go on through the half-transparent disc
            geometry_objects = (("disc", 3.0, 9.0), ("sphere", 2.5, (-7.0, 2.0, 1.0)))
        else:
            b = grt.SceneBuilder(L.GEOM_KERR_BL, radius=1.0, a=0.499, horizon_epsilon=1e-4)
            b.integration(20000, 100.0, 0.01, 1e-5)
            pos = grt.cartesian_to_boyer_lindquist(0.499, (0.0, -10.0, 0.0, -0.5))
            b.camera(pos, grt.stationary_velocity(L.GEOM_KERR_BL, 1.0, 0.499, pos), math.pi / 4, ROWS, COLS, 0.0,
                     -3.14159, 0.0)
            geometry_objects = (("disc", 2.0, 8.0), ("sphere", 2.0, (-5.0, 1.5, 0.3)))
        if not alt:
            b.celestial(_bitmap(grt, 1, 3.0), temperature=0.0)
            textures = (grt.Checker(3.0, 12.0, 4.0, (255, 160, 0), (120, 40, 0)), grt.BlackBody(0.0))
            temps = (2000.0, 3000.0)
        else:
            b.celestial(grt.BlackBody(1.0), temperature=4500.0)
            textures = (_bitmap(grt, 2, 1.5, alpha_lo=40), grt.Checker(2.0, 5.0, 7.0, (0, 200, 0), (255, 255, 255)))
            temps = (3500.0, 1200.0)
        for (kind, r, x), tex, t in zip(geometry_objects, textures, temps):
            if kind == "disc":
                b.add_disc(r, x, tex, temperature=t)
            else:
                b.add_sphere(r, x, tex, temperature=t)
        d = b.build()
        if not alt:
            _set_alpha(d.objects[0].texture, 0.5, 0.5)  # the disc: half transparent everywhere
            d.object_hit_opacity_threshold = 0.5
        else:
            _set_alpha(d.objects[1].texture, 0.5, 1.0)
            d.object_hit_opacity_threshold = 0.97
        out.append(d)
    return out


def built_scene(grt, d):
    return grt.Scene(C.pointer(d), keepalive=d)


# --------------------------------------------------------------------- comparisons ----
def assert_same_frame(got, want, what=""):
    assert np.array_equal(got.xyza.view(np.uint32), want.xyza.view(np.uint32)), (what, "xyza")
    assert np.array_equal(got.xyza64.view(np.uint64), want.xyza64.view(np.uint64)), (what, "xyza64")
    assert np.array_equal(got.ray_class, want.ray_class), (what, "class")
    assert np.array_equal(got.status, want.status), (what, "status")


def assert_buffer_matches_trace(grt, gb, want, what=""):
    """The buffer's per-pixel arrays against render_pixels' aux outputs."""
    L = grt._lib
    a = gb.arrays()
    info = gb.info
    n = int(info.n_pixels)
    assert n == want.status.size and int(info.n_layers) == a["object"].size == int(a["layer_start"][-1]), what
    assert np.array_equal(a["status"], want.status), (what, "status")
    assert np.array_equal(a["stop"], want.stop_reason), (what, "stop")
    assert np.array_equal(a["steps"], want.steps), (what, "steps")
    assert not np.any(a["status"] & L.FLAG_HIT_OVERFLOW), what
    layers = np.diff(a["layer_start"].astype(np.int64))
    assert a["layer_start"][0] == 0 and np.all(layers >= 0), what
    assert np.array_equal(layers, np.where(want.status == 0, want.hits, 0)), (what, "layer counts")
    no_sky = (a["stop"] != L.STOP_CELESTIAL) | (a["status"] != 0)
    for k in ("sky_u", "sky_v", "sky_redshift"):
        assert not np.any(a[k][no_sky].view(np.uint64)), (what, k)  # +0.0, bit for bit
    assert np.all(a["object"] < info.shape.n_objects), what
    spheres = np.array([info.shape.objects[int(o)].kind == L.OBJ_SPHERE for o in a["object"]], bool)
    assert not np.any(a["radius"][spheres].view(np.uint64)), (what, "sphere radius")
    return a, layers


_CACHE = {}


def stock_case(grt, name):
    """(host scene, scene, render_pixels of the frame, its g-buffer), once per scene."""
    if name not in _CACHE:
        hs, sc = stock(grt, STOCK[name][0], **STOCK[name][1])
        _CACHE[name] = (hs, sc, sc.render_pixels(0, 0, ROWS, COLS), sc.trace_gbuffer())
    return _CACHE[name]


# ------------------------------------------------------------------- 1. identity ----
@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl", "kerr-schild", "euclidean", "euclidean-spherical"])
def test_identity(grt, gpu, name):
    hs, sc, want, gb = stock_case(grt, name)
    assert len(np.unique(want.ray_class)) >= 2, np.unique(want.ray_class)  # a picture with something in it
    assert_same_frame(gb.shade(sc), want, name)
    a, layers = assert_buffer_matches_trace(grt, gb, want, name)
    assert layers.sum() > 0 and np.any(a["stop"] == grt._lib.STOP_CELESTIAL), name
    info = gb.info
    assert (info.row0, info.col0, info.rows, info.cols, info.device) == (0, 0, ROWS, COLS, 0)
    assert bytes(info.camera) == bytes(hs.desc.camera) and info.max_steps == hs.desc.max_steps
    assert gb.stats["rays"] == ROWS * COLS and gb.stats["accepted_steps"] == want.stats["accepted_steps"]
    # a sub-rectangle off the tile grid
    rect = (3, 5, 9, 11)
    sub_want = sc.render_pixels(*rect)
    sub = sc.trace_gbuffer(*rect)
    assert_same_frame(sub.shade(sc), sub_want, name + " sub-rectangle")
    assert_buffer_matches_trace(grt, sub, sub_want, name + " sub-rectangle")
    pick = (np.arange(rect[0], rect[0] + rect[2])[:, None] * COLS + np.arange(rect[1], rect[1] + rect[3])[None, :]).ravel()
    assert np.array_equal(sub_want.xyza64.view(np.uint64), want.xyza64[pick].view(np.uint64))
    sub.close()


# -------------------------------------------------------------------- 2. re-shade ----
@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl"])
def test_reshade_under_another_appearance(grt, gpu, name):
    da, db = reshade_pair(grt, name)
    grt.gbuffer_compatible(da, db)
    sa, sb = built_scene(grt, da), built_scene(grt, db)
    want_a, want_b = sa.render_pixels(0, 0, ROWS, COLS), sb.render_pixels(0, 0, ROWS, COLS)
    gb = sa.trace_gbuffer()
    assert_same_frame(gb.shade(sb), want_b, name + " B")
    assert_same_frame(gb.shade(sa), want_a, name + " A")
    # and the other way round: B's buffer is A's
    gb_b = sb.trace_gbuffer()
    a, b = gb.arrays(), gb_b.arrays()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    # the frames exercise the blend and the threshold
    layers = np.diff(a["layer_start"].astype(np.int64))
    assert (layers >= 2).sum() >= 30, (layers >= 2).sum()
    assert np.any(want_a.ray_class != want_b.ray_class)
    assert not np.array_equal(want_a.xyza, want_b.xyza)
    blended = (layers >= 2) & (want_b.xyza64[:, 3] > 0)
    assert blended.sum() >= 30


# ---------------------------------------------------------------- 3. past the slots ----
@pytest.mark.parametrize("disc", [False, True], ids=["spheres", "disc"])
def test_layers_past_the_workspace_slots(grt, gpu, disc):
    from test_hit_pool import N, winding_scene

    L = grt._lib
    d = winding_scene(grt, disc=disc)
    sc = built_scene(grt, d)
    want = sc.render_pixels(0, 0, N, N)
    gb = sc.trace_gbuffer()
    assert_same_frame(gb.shade(sc), want, "winding")
    a, layers = assert_buffer_matches_trace(grt, gb, want, "winding")
    assert (layers > L.GRT_MAX_HITS).sum() >= 300 and layers.max() > 80, ((layers > L.GRT_MAX_HITS).sum(), layers.max())
    if disc:
        assert {2, 3} <= set(np.unique(a["status"])), np.unique(a["status"])
    # a pool too small for the trace: the rectangle is traced again with a grown pool
    L.check(L.lib().grt_set_hit_pool_min(64))
    try:
        small = built_scene(grt, d)  # a fresh device copy: a 64-record pool
        gb2 = small.trace_gbuffer()
        assert gb2.stats["rays"] > N * N  # more than one trace
        b = gb2.arrays()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert not np.any(b["status"] & L.FLAG_HIT_OVERFLOW)
        assert_same_frame(gb2.shade(small), want, "winding, small pool")
    finally:
        L.check(L.lib().grt_set_hit_pool_min(1 << 20))


# ------------------------------------------------------------------ 4. oracle tie ----
def test_oracle_tie(grt, oracle, gpu):
    """The recorded numbers mean what the header says: fed to the ORACLE's texture lookup and
    blend they give the oracle's pixel, within the project's 1e-4 per channel."""
    from test_gpu_parity import check_parity, oracle_pair, within

    L = grt._lib
    n_sky = n_sphere = 0
    for name in ("schwarzschild", "schwarzschild-sphere"):
        hs, sc, got, gb = stock_case(grt, name)
        d = hs.desc
        ref, probes = oracle_pair(oracle, d, 0, 0, ROWS, COLS)
        robust = check_parity(got, ref, probes, max_sensitive=0.05)
        a = gb.arrays()
        layers = np.diff(a["layer_start"].astype(np.int64))
        black = np.array([0.0, 0.0, 0.0, 1.0])

        def terminal(i):
            if a["stop"][i] == L.STOP_CELESTIAL:
                return oracle.blend(black, oracle.texture_color(d, -1, a["sky_u"][i], a["sky_v"][i], a["sky_redshift"][i],
                                                                d.celestial_temperature))
            assert a["stop"][i] in (L.STOP_HORIZON, L.STOP_CLOSED_ORBIT)
            return oracle.blend(black, black)

        ok = robust & (a["status"] == 0)
        for i in np.flatnonzero(ok & (a["stop"] == L.STOP_CELESTIAL) & (layers == 0)):
            assert within(terminal(i)[None, :], ref["xyza"][i][None, :])[0], (name, "sky", i)
            n_sky += 1
        for i in np.flatnonzero(ok & (layers == 1)):
            k = int(a["layer_start"][i])
            obj = int(a["object"][k])
            if d.objects[obj].kind != L.OBJ_SPHERE or a["stop"][i] == L.STOP_NONE or a["stop"][i] == L.STOP_NAN:
                continue
            col = oracle.texture_color(d, obj, a["u"][k], a["v"][k], a["redshift"][k], d.objects[obj].temperature)
            mine = oracle.blend(terminal(i), col)
            assert within(mine[None, :], ref["xyza"][i][None, :])[0], (name, "sphere", i, mine, ref["xyza"][i])
            n_sphere += 1
    assert n_sky >= 50 and n_sphere >= 20, (n_sky, n_sphere)


# ----------------------------------------------------------------- 5. round trips ----
def test_round_trips(grt, gpu, tmp_path):
    hs, sc, want, gb = stock_case(grt, "schwarzschild")
    up = grt.GBuffer.from_arrays(gb.info, gb.arrays(), device=0)
    assert_same_frame(up.shade(sc), want, "download -> upload")
    gb.save(tmp_path / "a.grtg")
    loaded = grt.GBuffer.load(tmp_path / "a.grtg", device=0)
    assert_same_frame(loaded.shade(sc), want, "save -> load")
    assert bytes(loaded.info) == bytes(gb.info)
    assert loaded.trace_times == {"trace_ms": 0.0, "fill_ms": 0.0} and gb.trace_times["trace_ms"] > 0
    # a second trace of the same scene (a fresh device copy) writes the same bytes
    _, sc2 = stock(grt, STOCK["schwarzschild"][0], **STOCK["schwarzschild"][1])
    sc2.trace_gbuffer().save(tmp_path / "b.grtg")
    assert (tmp_path / "a.grtg").read_bytes() == (tmp_path / "b.grtg").read_bytes()
    # an upload is held to the file's checks: no kernel sees an object index out of range
    bad = gb.arrays()
    bad["object"][0] = 7
    with pytest.raises(grt.GrtError, match="names object"):
        grt.GBuffer.from_arrays(gb.info, bad)
    up.close()
    loaded.close()
    up.close()  # closing twice is harmless


# ---------------------------------------------------------------- 6. independence ----
def test_buffer_outlives_later_traces(grt, gpu):
    hs, sc = stock(grt, STOCK["schwarzschild"][0], **STOCK["schwarzschild"][1])
    want = stock_case(grt, "schwarzschild")[2]
    gb = sc.trace_gbuffer()
    sc.render_pixels(2, 1, 12, 17)  # another rectangle in the same scene's workspace
    _, other = stock(grt, STOCK["kerr-bl"][0], **STOCK["kerr-bl"][1])
    other.render_pixels(0, 0, ROWS, COLS)  # another scene on the device
    other.trace_gbuffer().close()
    assert_same_frame(gb.shade(sc), want, "after other traces")


# ------------------------------------------------------------------ 7. fused knob ----
def test_gbuffer_trace_is_exact_under_the_fused_knob(grt, gpu):
    hs, sc, want, _ = stock_case(grt, "schwarzschild")
    assert grt.get_arithmetic() == 0
    grt.set_arithmetic("fused")
    try:
        fused = sc.render_pixels(0, 0, ROWS, COLS)
        gb = sc.trace_gbuffer()
        shaded = gb.shade(sc)
    finally:
        grt.set_arithmetic("exact")
    assert not np.array_equal(fused.xyza64, want.xyza64)  # the knob does change render_pixels
    assert_same_frame(shaded, want, "fused knob")
    assert np.array_equal(gb.arrays()["steps"], want.steps)


# -------------------------------------------------------------------- 8. refusals ----
def _rc(exc):
    return int(str(exc.value).split("(")[1].split(")")[0])


def test_refusals(grt, gpu):
    L = grt._lib
    _, vol = stock(grt, "schwarzschild-volumetric-stony.toml", **STOCK["schwarzschild"][1])
    with pytest.raises(grt.GrtError) as e:
        vol.trace_gbuffer()
    assert _rc(e) == -errno.ENOTSUP
    hs, sc, want, gb = stock_case(grt, "schwarzschild")
    _, flat = stock(grt, "schwarzschild-sphere.toml", **STOCK["schwarzschild"][1])  # radius 0, the sphere elsewhere
    with pytest.raises(grt.GrtError, match="radius") as e:
        gb.shade(flat)
    assert _rc(e) == -errno.EINVAL
    _, bl = stock(grt, STOCK["kerr-bl"][0], **STOCK["kerr-bl"][1])
    with pytest.raises(grt.GrtError, match="geometry") as e:
        gb.shade(bl)
    assert _rc(e) == -errno.EINVAL
    da, _ = reshade_pair(grt, "schwarzschild")
    moved, _ = reshade_pair(grt, "schwarzschild")
    moved.objects[1].center[2] = 1.5
    gba = built_scene(grt, da).trace_gbuffer()
    with pytest.raises(grt.GrtError, match=r"objects\[1\]\.center") as e:
        gba.shade(built_scene(grt, moved))
    assert _rc(e) == -errno.EINVAL
    for rect in ((0, 0, ROWS + 1, COLS), (3, 5, ROWS - 2, COLS), (0, COLS, 1, 1), (0, 0, 0, 4)):
        with pytest.raises(grt.GrtError) as e:
            sc.trace_gbuffer(*rect)
        assert _rc(e) == -errno.EINVAL, rect
    assert_same_frame(gb.shade(sc), want, "after the refusals")


def test_scene_on_another_device_is_refused(grt, gpu):
    if grt.device_count() < 2:
        pytest.skip("needs two GPUs")
    hs, sc, want, gb = stock_case(grt, "schwarzschild")
    sc.render_pixels(0, 0, ROWS, COLS, device=1)  # the scene has a copy on device 1
    with pytest.raises(grt.GrtError) as e:
        gb.shade(sc, device=1)
    assert _rc(e) == -errno.EINVAL
    on1 = grt.GBuffer.from_arrays(gb.info, gb.arrays(), device=1)
    assert on1.info.device == 1
    assert_same_frame(on1.shade(sc), want, "uploaded to device 1")
    with pytest.raises(grt.GrtError) as e:
        on1.shade(sc, device=0)
    assert _rc(e) == -errno.EINVAL


# ------------------------------------------------------------------------- 9. CLI ----
def _grt(*args):
    """One `grt` run: a fresh child process with its own time limit."""
    r = subprocess.run([str(GRT), *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_cli_gbuffer_then_reshade(grt, gpu, tmp_path):
    text = (SCENES / "schwarzschild.toml").read_text() + "\n[adaptive_sampling]\nenabled = false\n"
    a_toml, b_toml = tmp_path / "a.toml", tmp_path / "b.toml"
    a_toml.write_text(text)
    swapped = text.replace("resources/disk.png", "resources/@").replace("resources/sphere.png", "resources/disk.png") \
                  .replace("resources/@", "resources/sphere.png").replace("temperature = 2000.0", "temperature = 3100.0")
    assert swapped != text and swapped.count("disk.png") == 1
    b_toml.write_text(swapped)
    common = ["--width", 64, "--height", 48, "--camera-position", "-16,0,3.5", "--theta", "-3.142", "--max-steps", 100000,
              "--resource-root", RESOURCES]
    _grt(*common, "--config-file", a_toml, "gbuffer", "--filename", tmp_path / "a.grtg")
    # reshade ignores the camera flags: the frame is the traced one
    _grt("--width", 64, "--height", 48, "--camera-position", "3,3,3", "--resource-root", RESOURCES, "--raw-out",
         tmp_path / "reshade.raw", "--config-file", b_toml, "reshade", "--gbuffer", tmp_path / "a.grtg", "--filename",
         tmp_path / "reshade.png")
    _grt(*common, "--raw-out", tmp_path / "render.raw", "--config-file", b_toml, "render", "--filename",
         tmp_path / "render.png")
    assert (tmp_path / "reshade.png").read_bytes() == (tmp_path / "render.png").read_bytes()
    raw = (tmp_path / "render.raw").read_bytes()
    assert len(raw) == 64 * 48 * 32 and (tmp_path / "reshade.raw").read_bytes() == raw
    # and B's picture is not A's
    _grt(*common, "--config-file", a_toml, "render", "--filename", tmp_path / "render_a.png")
    assert (tmp_path / "render_a.png").read_bytes() != (tmp_path / "render.png").read_bytes()
    info, arrays = grt.GBuffer.read_file(tmp_path / "a.grtg")
    assert (info.rows, info.cols, int(info.n_pixels)) == (48, 64, 48 * 64) and info.n_layers > 0
