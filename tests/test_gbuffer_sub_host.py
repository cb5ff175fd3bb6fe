"""The host side of a geometry buffer's sub-sample set (grt_gbuffer_sub_*; CPU only, no GPU
call): the ctypes mirrors against the header, the sidecar's round trip, its binding to a
buffer and its rejections -- and the .grtg file itself, which keeps its bytes and version."""
import ctypes as C
import errno
import hashlib
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES
from test_gbuffer_host import COUNTS_MIXED, FILE_ORDER, _sections, _synthetic

GRT = ROOT / "gr_raytracer_amd" / "lib" / "grt"
SPA = 2


def test_struct_layout_matches_header(grt, tmp_path):
    L = grt._lib
    structs = {"grt_gbuffer_sub_info": L.GBufferSubInfo, "grt_gbuffer_section_report": L.GBufferSectionReport,
               "grt_gbuffer_info": L.GBufferInfo, "grt_gbuffer_arrays": L.GBufferArrays}
    src = tmp_path / "sizes.c"
    body = "".join(f'  printf("{k} %zu\\n", sizeof({k}));\n' for k in structs)
    body += '  printf("version %d\\n", GRT_GBUFFER_FILE_VERSION);\n'
    body += '  printf("sub_version %d\\n", GRT_GBUFFER_SUB_FILE_VERSION);\n'
    body += '  printf("top_up_offset %zu\\n", offsetof(grt_gbuffer_section_report, top_up));\n'
    body += '  printf("n_sub_layers_offset %zu\\n", offsetof(grt_gbuffer_sub_info, n_sub_layers));\n'
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "grt_api.h"\nint main(void) {{\n{body}  return 0;\n}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    sizes = dict(line.split() for line in out if line)
    for k, cls in structs.items():
        assert int(sizes[k]) == C.sizeof(cls), (k, sizes[k], C.sizeof(cls))
    assert int(sizes["version"]) == L.GBUFFER_FILE_VERSION == 1  # the .grtg version stays
    assert int(sizes["sub_version"]) == L.GBUFFER_SUB_FILE_VERSION
    assert int(sizes["top_up_offset"]) == L.GBufferSectionReport.top_up.offset
    assert int(sizes["n_sub_layers_offset"]) == L.GBufferSubInfo.n_sub_layers.offset
    # the pinned sizes of tests/test_gbuffer_host.py's structures, unchanged by the set
    assert C.sizeof(L.GBufferArrays) == 12 * 8


def test_grtg_file_keeps_its_bytes(grt, tmp_path):
    """A synthetic buffer's file, byte for byte what the format of the header says (the
    sub-sample set lives in a sidecar: nothing of it reaches the .grtg file)."""
    L = grt._lib
    info, arrays = _synthetic(grt, COUNTS_MIXED)
    path = tmp_path / "a.grtg"
    grt.GBuffer.write_file(path, info, arrays)
    want = b"GRTGBUF\0" + struct.pack("<II", 1, C.sizeof(L.GBufferInfo)) + bytes(info)
    for k in ("layer_start", "sky_u", "sky_v", "sky_redshift", "u", "v", "redshift", "radius", "steps", "status", "stop",
              "object"):
        want += arrays[k].tobytes()
    assert path.read_bytes() == want
    # and another version is still refused
    data = path.read_bytes()
    path.write_bytes(data[:8] + struct.pack("<I", 2) + data[12:])
    with pytest.raises(grt.GrtError, match="version"):
        grt.GBuffer.read_file(path)


# --------------------------------------------------------------------- the sidecar ----
def _sub(grt, info, pixels, counts, seed=9):
    """A sub-sample set over `pixels` of the buffer `info` with the given sub-ray layer counts."""
    L = grt._lib
    per = SPA * SPA
    counts = np.asarray(counts, np.uint64)
    assert len(counts) == len(pixels) * per
    sub = L.GBufferSubInfo(SPA, 0, len(pixels), len(counts), int(counts.sum()))
    rng = np.random.default_rng(seed)
    n, nl = len(counts), int(counts.sum())
    arrays = {
        "status": rng.integers(0, 4, n).astype(np.uint8), "stop": rng.integers(0, 5, n).astype(np.uint8),
        "steps": rng.integers(0, 1 << 20, n).astype(np.uint32), "sky_u": rng.random(n), "sky_v": rng.random(n),
        "sky_redshift": rng.random(n) + 0.5,
        "layer_start": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64),
        "object": rng.integers(0, int(info.shape.n_objects), nl).astype(np.uint8), "u": rng.random(nl),
        "v": rng.random(nl), "redshift": rng.random(nl) + 0.5, "radius": rng.random(nl) * 10,
        "sub_pixel": np.asarray(pixels, np.uint32),
    }
    if nl:
        arrays["sky_v"][1] = -0.0  # bits, not values, survive
        arrays["u"][0] = np.nan
    return sub, arrays


PIXELS = [7, 2, 11]  # append order, not ascending
COUNTS = [0, 3, 0, 20, 1, 0, 0, 2, 5, 0, 0, 1]


@pytest.mark.parametrize("empty", [False, True], ids=["three-pixels", "no-pixels"])
def test_sidecar_round_trip(grt, tmp_path, empty):
    L = grt._lib
    info, _ = _synthetic(grt, COUNTS_MIXED)
    sub, arrays = _sub(grt, info, [] if empty else PIXELS, [] if empty else COUNTS)
    path = tmp_path / "a.grtg.sub"
    grt.GBuffer.write_sub_file(path, info, sub, arrays)
    sub2, arrays2 = grt.GBuffer.read_sub_file(path, info)
    assert bytes(sub2) == bytes(sub) and set(arrays2) == set(arrays)
    for k, v in arrays.items():
        assert arrays2[k].dtype == v.dtype and arrays2[k].tobytes() == v.tobytes(), k
    grt.GBuffer.write_sub_file(tmp_path / "b.sub", info, sub2, arrays2)
    assert (tmp_path / "b.sub").read_bytes() == path.read_bytes()
    data = path.read_bytes()
    assert data[:8] == b"GRTGSUB\0"
    assert struct.unpack("<II", data[8:16]) == (L.GBUFFER_SUB_FILE_VERSION, C.sizeof(L.GBufferInfo))
    # the buffer's info follows, the device aside: the same sidecar serves a load on any device
    on1 = L.GBufferInfo.from_buffer_copy(bytes(info))
    on1.device = 1
    grt.GBuffer.write_sub_file(tmp_path / "c.sub", on1, sub, arrays)
    assert (tmp_path / "c.sub").read_bytes() == data
    assert bytes(grt.GBuffer.read_sub_file(path, on1)[0]) == bytes(sub)


def test_sidecar_layout_is_pinned(grt, tmp_path):
    """Every array at its own place of the sidecar, sub_pixel before the twelve: a round trip
    cannot see two arrays of equal size swapped in the writer and the reader alike."""
    L = grt._lib
    info, _ = _synthetic(grt, COUNTS_MIXED)
    assert (int(info.n_pixels), int(info.n_layers)) == (12, 66)
    sub, arrays = _sub(grt, info, PIXELS, COUNTS)
    path = tmp_path / "a.grtg.sub"
    grt.GBuffer.write_sub_file(path, info, sub, arrays)
    data = path.read_bytes()
    # the .grtg file's sections for the set's sizes, moved behind the sub info and sub_pixel
    sized = L.GBufferInfo.from_buffer_copy(bytes(info))
    sized.n_pixels, sized.n_layers = len(COUNTS), sum(COUNTS)
    sub_pixel = _sections(grt, sized)[3] + C.sizeof(L.GBufferSubInfo)
    bounds = [b + C.sizeof(L.GBufferSubInfo) + 4 * len(PIXELS) for b in _sections(grt, sized)[3:]]
    assert bounds[-1] == len(data) and len(bounds) == 1 + len(FILE_ORDER)
    assert data[sub_pixel:bounds[0]] == arrays["sub_pixel"].tobytes()
    for k, name in enumerate(FILE_ORDER):
        assert data[bounds[k]:bounds[k + 1]] == arrays[name].tobytes(), name


def _read_rc(grt, path, info):
    """(rc of the size query, rc of the fill or None, message of the failing call)."""
    from gr_raytracer_amd.scene import _gbuffer_sub_host_arrays

    L = grt._lib
    sub = L.GBufferSubInfo()
    rc = L.lib().grt_gbuffer_sub_read_file(str(path).encode(), C.byref(info), C.byref(sub), None, None)
    if rc:
        return rc, None, L.lib().grt_last_error().decode()
    held, c, px = _gbuffer_sub_host_arrays(sub)  # `held`: the arrays `c` points into
    rc2 = L.lib().grt_gbuffer_sub_read_file(str(path).encode(), C.byref(info), C.byref(sub), px, C.byref(c))
    del held
    return 0, rc2, L.lib().grt_last_error().decode() if rc2 else ""


def test_sidecar_rejections(grt, tmp_path):
    L = grt._lib
    info, _ = _synthetic(grt, COUNTS_MIXED)
    sub, arrays = _sub(grt, info, PIXELS, COUNTS)
    good = tmp_path / "good.sub"
    grt.GBuffer.write_sub_file(good, info, sub, arrays)
    data = good.read_bytes()
    m, n, nl = len(PIXELS), len(COUNTS), sum(COUNTS)
    sizes = [8, 4, 4, C.sizeof(L.GBufferInfo), C.sizeof(L.GBufferSubInfo), 4 * m, 8 * (n + 1), 8 * n, 8 * n, 8 * n,
             8 * nl, 8 * nl, 8 * nl, 8 * nl, 4 * n, n, n, nl]
    bounds = list(np.cumsum(sizes))
    assert bounds[-1] == len(data)
    assert _read_rc(grt, good, info)[:2] == (0, 0)
    bad = tmp_path / "bad.sub"

    def rejected(blob, word, against=info):
        bad.write_bytes(blob)
        rc, rc2, msg = _read_rc(grt, bad, against)
        assert (rc or rc2) == -errno.EINVAL, (word, rc, rc2, msg)
        assert word in msg, (word, msg)

    rejected(b"GRTGBUF\0" + data[8:], "magic")  # a .grtg file's magic is not a sidecar's
    rejected(data[:8] + struct.pack("<I", L.GBUFFER_SUB_FILE_VERSION + 1) + data[12:], "version")
    rejected(data[:12] + struct.pack("<I", C.sizeof(L.GBufferInfo) + 8) + data[16:], "info block")
    for cut in [0] + bounds[:-1] + [len(data) - 1]:
        rejected(data[:cut], "too short" if cut < bounds[4] else "file length")
    rejected(data + b"\0", "file length")
    # bound to its buffer: any other info is refused (another layer total, another camera, ...)
    other, _ = _synthetic(grt, COUNTS_MIXED)
    other.n_layers += 1
    rejected(data, "info", against=other)
    other, _ = _synthetic(grt, COUNTS_MIXED)
    other.camera.position[1] = 3.0
    rejected(data, "info", against=other)
    other, _ = _synthetic(grt, COUNTS_MIXED)
    other.max_steps += 1
    rejected(data, "info", against=other)
    # the set's sizes
    off = bounds[3]
    fld = L.GBufferSubInfo

    def patched(field, fmt, value):
        o = off + getattr(fld, field).offset
        return data[:o] + struct.pack(fmt, value) + data[o + struct.calcsize(fmt):]

    rejected(patched("samples_per_axis", "<I", 3), "n_sub_rays")
    rejected(patched("samples_per_axis", "<I", 0), "samples_per_axis is 0")
    rejected(patched("n_sub_pixels", "<Q", int(info.n_pixels) + 1), "n_sub_pixels")
    rejected(patched("n_sub_layers", "<Q", nl + 1), "file length")
    rejected(patched("n_sub_layers", "<Q", 1 << 62), "layers")
    # sub_pixel: outside the buffer, a duplicate
    sp = bounds[4]
    rejected(data[:sp] + struct.pack("<I", int(info.n_pixels)) + data[sp + 4:], "outside")
    rejected(data[:sp + 4] + struct.pack("<I", PIXELS[0]) + data[sp + 8:], "duplicate")
    # layer_start, statuses, objects
    ls = bounds[5]
    rejected(data[:ls] + struct.pack("<Q", 1) + data[ls + 8:], "begin at 0")
    rejected(data[:ls + 16] + struct.pack("<Q", 50) + data[ls + 24:], "decreases")
    last = ls + 8 * n
    rejected(data[:last] + struct.pack("<Q", nl + 4) + data[last + 8:], "end at n_sub_layers")
    st = bounds[14]
    rejected(data[:st + 2] + bytes([0x80 | data[st + 2]]) + data[st + 3:], "GRT_FLAG_HIT_OVERFLOW")
    ob = bounds[-2]
    rejected(data[:ob + 7] + bytes([int(info.shape.n_objects)]) + data[ob + 8:], "names object")
    # a writer refuses the same arrays
    wrong = {k: v.copy() for k, v in arrays.items()}
    wrong["sub_pixel"][2] = wrong["sub_pixel"][0]
    with pytest.raises(grt.GrtError, match="duplicate"):
        grt.GBuffer.write_sub_file(tmp_path / "w.sub", info, sub, wrong)
    # a missing file is an I/O error, not a crash
    assert _read_rc(grt, tmp_path / "none.sub", info)[0] == -errno.EIO
    assert hashlib.sha256(good.read_bytes()).digest() == hashlib.sha256(data).digest()  # the good file was never touched


def test_cli_adaptive_flag_is_a_subcommand_option(grt, tmp_path):
    scene = str(SCENES / "schwarzschild.toml")
    r = subprocess.run([str(GRT), "--config-file", scene, "gbuffer", "--adaptive"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "gbuffer needs --filename" in r.stderr and "--adaptive" in r.stderr
    r = subprocess.run([str(GRT), "--config-file", scene, "reshade", "--adaptive"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "reshade needs --gbuffer" in r.stderr
    r = subprocess.run([str(GRT), "--config-file", scene, "render", "--adaptive"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2  # not an option of `render`
