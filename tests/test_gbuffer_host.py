"""The host side of the geometry buffer (grt_gbuffer_*; CPU only, no GPU call): the ctypes
mirrors against the header, the shape key's comparison, the file's round trip and its
rejections, and the usage errors of the two CLI subcommands."""
import ctypes as C
import errno
import math
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

GRT = ROOT / "gr_raytracer_amd" / "lib" / "grt"


def test_struct_layout_matches_header(grt, tmp_path):
    L = grt._lib
    structs = {"grt_gbuffer_object_shape": L.GBufferObjectShape, "grt_gbuffer_shape": L.GBufferShape,
               "grt_gbuffer_info": L.GBufferInfo, "grt_gbuffer_arrays": L.GBufferArrays}
    src = tmp_path / "sizes.c"
    body = "".join(f'  printf("{k} %zu\\n", sizeof({k}));\n' for k in structs)
    body += '  printf("version %d\\n", GRT_GBUFFER_FILE_VERSION);\n'
    body += '  printf("shape_offset %zu\\n", offsetof(grt_gbuffer_info, shape));\n'
    body += '  printf("camera_offset %zu\\n", offsetof(grt_gbuffer_info, camera));\n'
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "grt_api.h"\nint main(void) {{\n{body}  return 0;\n}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    sizes = dict(line.split() for line in out if line)
    for k, cls in structs.items():
        assert int(sizes[k]) == C.sizeof(cls), (k, sizes[k], C.sizeof(cls))
    assert int(sizes["version"]) == L.GBUFFER_FILE_VERSION
    assert int(sizes["shape_offset"]) == L.GBufferInfo.shape.offset
    assert int(sizes["camera_offset"]) == L.GBufferInfo.camera.offset


# ------------------------------------------------------------------ the shape key ----
def _scene(grt, alt=False):
    """Schwarzschild with a Kerr-LUT disc and a sphere; alt: the same shapes under another
    appearance, camera and step budget."""
    L = grt._lib
    b = grt.SceneBuilder(L.GEOM_SCHWARZSCHILD, radius=1.0, a=0.0, horizon_epsilon=1e-4)
    b.integration(30000 if alt else 20000, 100.0, 0.01, 1e-5)
    pos = grt.cartesian_to_spherical((0.0, -14.0, 2.0, 3.0) if alt else (0.0, -16.0, 0.0, 3.5))
    b.camera(pos, grt.stationary_velocity(L.GEOM_SCHWARZSCHILD, 1.0, 0.0, pos), math.pi / 4, 20, 24, 0.0, -3.142, 0.0)
    if alt:
        b.celestial(grt.BlackBody(1.0), temperature=5000.0)
        b.add_disc(3.0, 6.0, grt.BlackBody(2.0), temperature=3500.0)
        b.add_sphere(1.5, (0.0, 7.0, 1.0), grt.Checker(1.0, 3.0, 5.0, (255, 0, 0), (0, 0, 255)), temperature=900.0)
    else:
        b.celestial(grt.Checker(0.0, 16.0, 8.0, (20, 20, 80), (200, 200, 255)))
        b.add_disc(3.0, 6.0, grt.Checker(3.0, 12.0, 4.0, (255, 160, 0), (120, 40, 0)), temperature=2000.0)
        b.add_sphere(1.5, (0.0, 7.0, 1.0), grt.Checker(0.0, 6.0, 6.0, (0, 200, 0), (255, 255, 255)), temperature=3000.0)
    d = b.build()
    if alt:
        d.object_hit_opacity_threshold = 0.9
    return d


def _compat(grt, a, b):
    L = grt._lib
    rc = L.lib().grt_gbuffer_compatible(C.byref(a), C.byref(b))
    return rc, L.lib().grt_last_error().decode()


def test_compatible_with_another_appearance(grt):
    a, b = _scene(grt), _scene(grt, alt=True)
    assert bytes(a.camera) != bytes(b.camera) and a.max_steps != b.max_steps
    assert _compat(grt, a, b)[0] == 0
    assert _compat(grt, a, a)[0] == 0
    grt.gbuffer_compatible(a, b)  # the Python wrapper: no exception


def _mutations(L):
    def setter(path, value):
        def f(d):
            obj = d
            *head, last = path
            for p in head:
                obj = obj[p] if isinstance(p, int) else getattr(obj, p)
            if isinstance(last, int):
                obj[last] = value
            else:
                setattr(obj, last, value)
        return f

    return [
        ("geometry", setter(("geometry",), L.GEOM_EUCLIDEAN_SPHERICAL), "geometry"),
        ("a", setter(("a",), 0.25), "a"),
        ("radius", setter(("radius",), 1.5), "radius"),
        ("n_objects", setter(("n_objects",), 1), "n_objects"),
        ("kind", setter(("objects", 1, "kind"), L.OBJ_DISC), "objects[1].kind"),
        ("temp_kind", setter(("objects", 0, "temp_kind"), L.TEMP_CONSTANT), "objects[0].temp_kind"),
        ("inner_radius", setter(("objects", 0, "inner_radius"), 3.5), "objects[0].inner_radius"),
        ("center", setter(("objects", 1, "center", 1), 7.5), "objects[1].center"),
        ("r_isco", setter(("objects", 0, "r_isco"), 3.25), "objects[0].r_isco"),
        ("outer_radius", setter(("objects", 0, "outer_radius"), 6.5), "objects[0].outer_radius"),
        ("sphere radius", setter(("objects", 1, "radius"), 1.25), "objects[1].radius"),
    ]


@pytest.mark.parametrize("index", range(11))
def test_incompatible_names_the_field(grt, index):
    L = grt._lib
    name, mutate, expect = _mutations(L)[index]
    a, b = _scene(grt), _scene(grt, alt=True)
    mutate(b)
    rc, msg = _compat(grt, a, b)
    assert rc == -errno.EINVAL, (name, rc)
    assert msg.endswith(" differs from the traced one in " + expect), (name, msg)
    with pytest.raises(grt.GrtError):
        grt.gbuffer_compatible(a, b)


# ------------------------------------------------------------------------ the file ----
def _synthetic(grt, counts, n_objects=3, seed=5):
    """An info block and arrays for a rows x cols rectangle with the given layer counts."""
    L = grt._lib
    counts = np.asarray(counts, np.uint64)
    rows, cols = 3, len(counts) // 3
    assert rows * cols == len(counts)
    rng = np.random.default_rng(seed)
    info = L.GBufferInfo()
    info.row0, info.col0, info.rows, info.cols = 2, 1, rows, cols
    info.n_pixels, info.n_layers = len(counts), int(counts.sum())
    info.device = 0
    info.shape.geometry, info.shape.n_objects, info.shape.radius, info.shape.a = L.GEOM_KERR_BL, n_objects, 1.0, 0.499
    for k in range(n_objects):
        info.shape.objects[k].kind = k % 2
        info.shape.objects[k].radius = 0.5 + k
    info.camera.rows, info.camera.cols = 40, 50
    info.max_steps, info.max_radius, info.step_size, info.epsilon = 1000, 100.0, 0.01, 1e-5
    n, nl = len(counts), int(counts.sum())
    arrays = {
        "status": rng.integers(0, 4, n).astype(np.uint8), "stop": rng.integers(0, 5, n).astype(np.uint8),
        "steps": rng.integers(0, 1 << 20, n).astype(np.uint32), "sky_u": rng.random(n), "sky_v": rng.random(n),
        "sky_redshift": rng.random(n) + 0.5,
        "layer_start": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64),
        "object": rng.integers(0, max(n_objects, 1), nl).astype(np.uint8), "u": rng.random(nl), "v": rng.random(nl),
        "redshift": rng.random(nl) + 0.5, "radius": rng.random(nl) * 10,
    }
    arrays["sky_u"][0] = -0.0  # bits, not values, survive
    if nl:
        arrays["radius"][0] = np.nan
    return info, arrays


COUNTS_MIXED = [0, 20, 1, 0, 0, 20, 3, 0, 20, 0, 2, 0]


@pytest.mark.parametrize("counts", [COUNTS_MIXED, [0] * 6], ids=["mixed", "no-layers"])
def test_file_round_trip(grt, tmp_path, counts):
    info, arrays = _synthetic(grt, counts)
    path = tmp_path / "a.grtg"
    grt.GBuffer.write_file(path, info, arrays)
    info2, arrays2 = grt.GBuffer.read_file(path)
    assert bytes(info2) == bytes(info)
    assert set(arrays2) == set(arrays)
    for k, v in arrays.items():
        assert arrays2[k].dtype == v.dtype and arrays2[k].tobytes() == v.tobytes(), k
    assert int(info2.n_layers) == sum(counts)
    # writing what was read gives the same bytes
    grt.GBuffer.write_file(tmp_path / "b.grtg", info2, arrays2)
    assert (tmp_path / "b.grtg").read_bytes() == path.read_bytes()


def _read_rc(grt, path):
    """(rc of the size query, rc of the fill or None, message of the failing call)."""
    L = grt._lib
    info = L.GBufferInfo()
    rc = L.lib().grt_gbuffer_read_file(str(path).encode(), C.byref(info), None)
    if rc:
        return rc, None, L.lib().grt_last_error().decode()
    from gr_raytracer_amd.scene import _gbuffer_host_arrays

    held, c = _gbuffer_host_arrays(info)  # `held`: the arrays `c` points into
    rc2 = L.lib().grt_gbuffer_read_file(str(path).encode(), C.byref(info), C.byref(c))
    del held
    return 0, rc2, L.lib().grt_last_error().decode() if rc2 else ""


def _sections(grt, info):
    """Byte offsets of the section boundaries of info's file, in file order."""
    L = grt._lib
    n, nl = int(info.n_pixels), int(info.n_layers)
    sizes = [8, 4, 4, C.sizeof(L.GBufferInfo), 8 * (n + 1), 8 * n, 8 * n, 8 * n, 8 * nl, 8 * nl, 8 * nl, 8 * nl, 4 * n, n,
             n, nl]
    return list(np.cumsum(sizes))


FILE_ORDER = ("layer_start", "sky_u", "sky_v", "sky_redshift", "u", "v", "redshift", "radius", "steps", "status", "stop",
              "object")


def test_file_layout_is_pinned(grt, tmp_path):
    """Every array at its own place of the file: a round trip cannot see two arrays of equal
    size swapped in the writer and the reader alike."""
    info, arrays = _synthetic(grt, COUNTS_MIXED)
    assert (int(info.n_pixels), int(info.n_layers)) == (12, 66)
    path = tmp_path / "a.grtg"
    grt.GBuffer.write_file(path, info, arrays)
    data = path.read_bytes()
    bounds = _sections(grt, info)
    assert bounds[-1] == len(data) and len(bounds) == 4 + len(FILE_ORDER)
    for k, name in enumerate(FILE_ORDER):
        assert data[bounds[3 + k]:bounds[4 + k]] == arrays[name].tobytes(), name


def test_file_rejections(grt, tmp_path):
    L = grt._lib
    info, arrays = _synthetic(grt, COUNTS_MIXED)
    good = tmp_path / "good.grtg"
    grt.GBuffer.write_file(good, info, arrays)
    data = good.read_bytes()
    bounds = _sections(grt, info)
    assert bounds[-1] == len(data)
    assert _read_rc(grt, good)[:2] == (0, 0)
    bad = tmp_path / "bad.grtg"

    def rejected(blob, word):
        bad.write_bytes(blob)
        rc, rc2, msg = _read_rc(grt, bad)
        assert (rc or rc2) == -errno.EINVAL, (word, rc, rc2, msg)
        assert word in msg, (word, msg)

    rejected(b"GRTGBUX\0" + data[8:], "magic")
    rejected(data[:8] + struct.pack("<I", L.GBUFFER_FILE_VERSION + 1) + data[12:], "version")
    rejected(data[:12] + struct.pack("<I", C.sizeof(L.GBufferInfo) + 8) + data[16:], "info block")
    # a truncation at every section boundary (and inside the last section), and a longer file
    for cut in [0] + bounds[:-1] + [len(data) - 1]:
        rejected(data[:cut], "too short" if cut < bounds[3] else "file length")
    rejected(data + b"\0", "file length")
    # sizes that disagree with each other or with the length
    off_info = bounds[2]
    fld = L.GBufferInfo
    def patched(field, fmt, value):
        o = off_info + getattr(fld, field).offset
        return data[:o] + struct.pack(fmt, value) + data[o + struct.calcsize(fmt):]
    rejected(patched("n_pixels", "<Q", int(info.n_pixels) + 1), "n_pixels")
    rejected(patched("n_layers", "<Q", int(info.n_layers) + 1), "file length")
    rejected(patched("n_layers", "<Q", 1 << 62), "layers")
    rejected(patched("rows", "<I", 0), "empty")
    # layer_start: not from 0, decreasing, not ending at n_layers
    ls = bounds[3]
    rejected(data[:ls] + struct.pack("<Q", 1) + data[ls + 8:], "begin at 0")
    rejected(data[:ls + 16] + struct.pack("<Q", 50) + data[ls + 24:], "decreases")
    last = ls + 8 * int(info.n_pixels)
    rejected(data[:last] + struct.pack("<Q", int(info.n_layers) + 4) + data[last + 8:], "end at n_layers")
    # an object index past the shape's objects
    ob = bounds[-2]
    rejected(data[:ob + 7] + bytes([int(info.shape.n_objects)]) + data[ob + 8:], "names object")
    # and a writer refuses the same arrays
    wrong = dict(arrays)
    wrong["object"] = arrays["object"].copy()
    wrong["object"][3] = 200
    with pytest.raises(grt.GrtError, match="names object"):
        grt.GBuffer.write_file(tmp_path / "w.grtg", info, wrong)
    # a missing file is an I/O error, not a crash
    assert _read_rc(grt, tmp_path / "none.grtg")[0] == -errno.EIO


# ------------------------------------------------------------------------- the CLI ----
def _run(*args):
    return subprocess.run([str(GRT), *args], capture_output=True, text=True, timeout=60)


def test_cli_usage_errors(grt, tmp_path):
    scene = str(SCENES / "schwarzschild.toml")
    other = _run("--config-file", scene, "render-ray")  # an existing subcommand's usage error
    assert other.returncode == 2 and other.stderr.startswith("error: ") and "usage: grt" in other.stderr
    r = _run("--config-file", scene, "reshade")
    assert r.returncode == other.returncode and "reshade needs --gbuffer" in r.stderr and "usage: grt" in r.stderr
    r = _run("--config-file", scene, "gbuffer")
    assert r.returncode == other.returncode and "gbuffer needs --filename" in r.stderr and "usage: grt" in r.stderr
    assert "gbuffer --filename" in r.stderr and "reshade --gbuffer" in r.stderr  # the usage text has both
    # reshade: the frame must be the file's (checked before the GPU is touched)
    info, arrays = _synthetic(grt, [0] * 6)
    info.row0 = info.col0 = 0
    info.camera.rows, info.camera.cols = info.rows, info.cols
    path = tmp_path / "frame.grtg"
    grt.GBuffer.write_file(path, info, arrays)
    r = _run("--width", "64", "--height", "48", "--config-file", scene, "reshade", "--gbuffer", str(path))
    assert r.returncode == 2 and "--width / --height must be the g-buffer's frame, 2 x 3" in r.stderr
    # a damaged file is an error message, not a crash
    path.write_bytes(path.read_bytes()[:-3])
    r = _run("--width", "2", "--height", "3", "--config-file", scene, "reshade", "--gbuffer", str(path))
    assert r.returncode == 1 and "file length" in r.stderr
