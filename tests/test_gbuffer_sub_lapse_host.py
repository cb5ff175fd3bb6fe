"""The host side of the timed sub-sample set (CPU only, no GPU call): the ctypes mirrors of the
new entries against the header, the sidecar `<file>.sub.lapse` (round trips and every
rejection, the caller's arrays untouched), the stand-alone sanitizer program of tools/, the
CLI's usage errors, the two new kernels in the library, and the recorded kernel hashes."""
import ctypes as C
import errno
import json
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES
from test_gbuffer_host import COUNTS_MIXED, _synthetic
from test_gbuffer_orbit_host import _CTYPE, _bits, _declaration, _run
from test_gbuffer_sub_host import COUNTS, PIXELS, _sub


# ----------------------------------------------------------------------- mirrors ----
NEW = ("grt_gbuffer_supersample_lapse", "grt_gbuffer_sub_has_lapse", "grt_gbuffer_sub_clear",
       "grt_gbuffer_sub_lapse_download", "grt_gbuffer_sub_lapse_upload", "grt_gbuffer_shade_section_at_retarded",
       "grt_gbuffer_sub_lapse_write_file", "grt_gbuffer_sub_lapse_read_file")


def test_ctypes_mirrors_match_the_header(grt):
    L = grt._lib
    types = dict(_CTYPE)
    types.update({"grt_gbuffer_info*": C.POINTER(L.GBufferInfo), "grt_gbuffer_sub_info*": C.POINTER(L.GBufferSubInfo),
                  "grt_stats*": C.POINTER(L.Stats), "grt_adaptive_config*": C.POINTER(L.AdaptiveConfig),
                  "grt_subsample_failures*": C.POINTER(L.SubsampleFailures),
                  "grt_gbuffer_section_report*": C.POINTER(L.GBufferSectionReport), "uint32_t*": C.POINTER(C.c_uint32),
                  "char*": C.c_char_p})
    for name in NEW:
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)
        fn = getattr(L.lib(), name)
        want = [types[t] for t in _declaration(name)]
        assert fn.restype is C.c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    # the new entries take their siblings' arguments
    assert _declaration("grt_gbuffer_supersample_lapse") == _declaration("grt_gbuffer_supersample")
    assert _declaration("grt_gbuffer_shade_section_at_retarded") == _declaration("grt_gbuffer_shade_section_at")
    assert _declaration("grt_gbuffer_sub_lapse_upload") == _declaration("grt_gbuffer_lapse_upload")
    assert _declaration("grt_gbuffer_sub_lapse_download") == _declaration("grt_gbuffer_lapse_download")
    # no struct changed: the ABI and the three older formats keep their versions
    header = (ROOT / "include" / "grt_api.h").read_text()
    for line in ("#define GRT_ABI_VERSION 3", "#define GRT_GBUFFER_FILE_VERSION 1", "#define GRT_GBUFFER_SUB_FILE_VERSION 1",
                 "#define GRT_GBUFFER_LAPSE_FILE_VERSION 1", "#define GRT_GBUFFER_SUB_LAPSE_FILE_VERSION 1"):
        assert line in header, line
    assert L.GBUFFER_SUB_LAPSE_FILE_VERSION == 1 and C.sizeof(L.GBufferSubInfo) == 32
    # and the feature is no longer listed as missing
    assert "Not covered: lapses for the sub-sample set" not in header and "stays fast-light" not in header
    # the entries that need no device refuse a null buffer
    assert L.lib().grt_gbuffer_sub_has_lapse(None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_sub_clear(None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_sub_lapse_download(None, None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_sub_lapse_upload(None, None, 0) == -errno.EINVAL


def test_python_surface(grt):
    import inspect

    G = grt.GBuffer
    assert inspect.signature(G.supersample).parameters["lapse"].default is False
    assert inspect.signature(G.shade_section).parameters["retarded"].default is False
    assert inspect.signature(grt.Scene.trace_gbuffer).parameters["lapse"].default is False
    assert isinstance(G.sub_has_lapse, property)
    for name in ("sub_lapse", "set_sub_lapse", "clear_sub", "write_sub_lapse_file", "read_sub_lapse_file"):
        assert callable(getattr(G, name)), name
    with pytest.raises(ValueError, match="needs a time"):  # before any library call
        G(None).shade_section(None, retarded=True)


# ------------------------------------------------------------------------ the sidecar ----
HEAD = 16  # magic, version, info-block size: then the info, the sub-info, the doubles


def _case(grt, empty=False):
    info, _ = _synthetic(grt, COUNTS_MIXED)
    sub, arrays = _sub(grt, info, [] if empty else PIXELS, [] if empty else COUNTS)
    lapse = -np.random.default_rng(4).uniform(0.0, 60.0, int(sub.n_sub_layers))
    return info, sub, arrays, lapse


@pytest.mark.parametrize("empty", [False, True], ids=["three-pixels", "no-pixels"])
def test_sidecar_round_trip(grt, tmp_path, empty):
    L = grt._lib
    info, sub, arrays, lapse = _case(grt, empty)
    if lapse.size:
        lapse[0] = -0.0  # bits, not values, survive
    path = tmp_path / "a.grtg.sub.lapse"
    grt.GBuffer.write_sub_lapse_file(path, info, sub, lapse)
    data = path.read_bytes()
    assert len(data) == HEAD + C.sizeof(L.GBufferInfo) + C.sizeof(L.GBufferSubInfo) + 8 * lapse.size
    assert data[:8] == b"GRTGSLP\0"
    assert struct.unpack("<II", data[8:16]) == (L.GBUFFER_SUB_LAPSE_FILE_VERSION, C.sizeof(L.GBufferInfo))
    at_sub = HEAD + C.sizeof(L.GBufferInfo)
    assert data[at_sub:at_sub + C.sizeof(L.GBufferSubInfo)] == bytes(sub)
    assert data[at_sub + C.sizeof(L.GBufferSubInfo):] == lapse.tobytes()
    back = grt.GBuffer.read_sub_lapse_file(path, info, sub)
    assert np.array_equal(_bits(back), _bits(lapse))
    on3 = L.GBufferInfo.from_buffer_copy(bytes(info))
    on3.device = 3  # a load changes the device: not part of what binds the sidecar
    assert np.array_equal(_bits(grt.GBuffer.read_sub_lapse_file(path, on3, sub)), _bits(lapse))
    grt.GBuffer.write_sub_lapse_file(tmp_path / "b.lapse", on3, sub, lapse)
    assert (tmp_path / "b.lapse").read_bytes() == data
    read = L.lib().grt_gbuffer_sub_lapse_read_file
    assert read(str(path).encode(), C.byref(info), C.byref(sub), None) == 0  # the check alone
    # the set's and the buffer's own sidecars keep their bytes beside it
    grt.GBuffer.write_sub_file(tmp_path / "a.grtg.sub", info, sub, arrays)
    assert (tmp_path / "a.grtg.sub").read_bytes()[:8] == b"GRTGSUB\0"


def test_sidecar_rejections(grt, tmp_path):
    L = grt._lib
    info, sub, arrays, lapse = _case(grt)
    n = lapse.size
    path, cut = tmp_path / "a.grtg.sub.lapse", tmp_path / "cut.lapse"
    grt.GBuffer.write_sub_lapse_file(path, info, sub, lapse)
    whole = path.read_bytes()
    at_sub = HEAD + C.sizeof(L.GBufferInfo)
    at_data = at_sub + C.sizeof(L.GBufferSubInfo)
    read = L.lib().grt_gbuffer_sub_lapse_read_file

    def refused(data, bound=info, held=sub, word=None):
        cut.write_bytes(data)
        out = np.full(n, 9.0)
        rc = read(str(cut).encode(), C.byref(bound), C.byref(held), L.dptr(out))
        assert rc == -errno.EINVAL and np.all(out == 9.0), (rc, len(data))
        if word:
            assert word in L.lib().grt_last_error().decode(), L.lib().grt_last_error().decode()
        assert read(str(cut).encode(), C.byref(bound), C.byref(held), None) == -errno.EINVAL

    # a truncation at each section boundary and inside each section, one byte short, one too many
    for length in (0, 7, 8, 12, 16, 17, at_sub - 1, at_sub, at_sub + 7, at_data - 1, at_data, at_data + 8,
                   len(whole) - 8, len(whole) - 1):
        refused(whole[:length])
    refused(whole + b"\0", word="file length")
    refused(b"GRTGLPS\0" + whole[8:], word="magic")  # the buffer's lapse sidecar is another file
    refused(b"GRTGSUB\0" + whole[8:], word="magic")
    refused(whole[:8] + (2).to_bytes(4, "little") + whole[12:], word="version")
    refused(whole[:12] + (8).to_bytes(4, "little") + whole[16:], word="info block")
    # an inconsistent count: the file's n_sub_layers against the set's, with and without the doubles to match
    at_count = at_sub + L.GBufferSubInfo.n_sub_layers.offset
    refused(whole[:at_count] + (n - 1).to_bytes(8, "little") + whole[at_count + 8:], word="another sub-sample set")
    refused(whole[:at_count] + (n - 1).to_bytes(8, "little") + whole[at_count + 8:-8], word="another sub-sample set")
    refused(whole[:at_count] + (1 << 62).to_bytes(8, "little") + whole[at_count + 8:], word="another sub-sample set")
    nan = np.array([np.nan]).tobytes()
    refused(whole[:at_data + 8 * 5] + nan + whole[at_data + 8 * 6:], word="not finite")
    # a sidecar whose info differs from the buffer's
    for field, value in (("rows", 4), ("row0", 0), ("max_steps", 7), ("epsilon", 1e-6), ("n_layers", 5)):
        other, _ = _synthetic(grt, COUNTS_MIXED)
        setattr(other, field, value)
        if field == "rows":
            other.cols, other.n_pixels = 3, 12
        refused(whole, bound=other, word="another g-buffer")
    other, _ = _synthetic(grt, COUNTS_MIXED)
    other.shape.objects[1].radius = 7.0
    refused(whole, bound=other, word="another g-buffer")
    # a sidecar whose sub-info differs from the set's: a .sub that grew since leaves it stale
    grown, _ = _sub(grt, info, PIXELS + [3], COUNTS + [1, 0, 2, 0])
    refused(whole, held=grown, word="another sub-sample set")
    moved = L.GBufferSubInfo.from_buffer_copy(bytes(sub))
    moved.n_sub_layers = n + 1
    refused(whole, held=moved, word="another sub-sample set")
    none = L.GBufferSubInfo()
    refused(whole, held=none, word="another sub-sample set")
    # the writer's refusals, and the files that are not there
    w = L.lib().grt_gbuffer_sub_lapse_write_file
    args = (C.byref(info), C.byref(sub))
    assert w(str(cut).encode(), *args, L.dptr(lapse), n - 1) == -errno.EINVAL
    bad = lapse.copy()
    bad[3] = np.inf
    assert w(str(cut).encode(), *args, L.dptr(bad), n) == -errno.EINVAL
    assert w(str(cut).encode(), *args, None, n) == -errno.EINVAL
    assert w(None, *args, L.dptr(lapse), n) == -errno.EINVAL
    assert w(str(cut).encode(), None, C.byref(sub), L.dptr(lapse), n) == -errno.EINVAL
    assert w(str(cut).encode(), C.byref(info), None, L.dptr(lapse), n) == -errno.EINVAL
    broken = L.GBufferSubInfo.from_buffer_copy(bytes(sub))
    broken.n_sub_rays += 1
    assert w(str(cut).encode(), C.byref(info), C.byref(broken), L.dptr(lapse), n) == -errno.EINVAL
    assert w(str(tmp_path / "no" / "dir.lapse").encode(), *args, L.dptr(lapse), n) == -errno.EIO
    assert read(str(tmp_path / "absent").encode(), *args, None) == -errno.EIO
    assert read(None, *args, None) == -errno.EINVAL
    assert read(str(path).encode(), None, C.byref(sub), None) == -errno.EINVAL
    assert read(str(path).encode(), C.byref(info), None, None) == -errno.EINVAL
    assert read(str(path).encode(), *args, None) == 0  # after the refusals


def test_stand_alone_sanitizer_program(tmp_path):
    """tools/sub_lapse_main.cpp over the two host files alone, built with the address and
    undefined behaviour sanitizers and run on the CPU: the sidecar's round trips with 0 and 5
    sub-layers, and its reader on every truncation of a small file and on every changed field."""
    exe = tmp_path / "sub_lapse_main"
    host = ROOT / "gr_raytracer_amd" / "csrc" / "host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "include"), str(ROOT / "tools" / "sub_lapse_main.cpp"),
                    str(host / "gbuffer.cpp"), str(host / "errors.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    assert not list(tmp_path.glob("*.lapse"))  # it removes its files


# ------------------------------------------------------------------------- the CLI ----
def test_cli_usage_errors(grt, tmp_path):
    L = grt._lib
    scene = str(SCENES / "schwarzschild.toml")
    pat = str(tmp_path / "f-%04d.png")
    info, arrays = _synthetic(grt, [0] * 6)
    info.row0 = info.col0 = 0
    info.camera.rows, info.camera.cols = info.rows, info.cols
    path = tmp_path / "frame.grtg"
    grt.GBuffer.write_file(path, info, arrays)
    orbit = ["--width", "2", "--height", "3", "--config-file", scene, "reshade-orbit", "--gbuffer", str(path), "--times",
             "0,1,3", "--filename-pattern", pat]

    def usage_error(r, *words):
        assert r.returncode == 2 and r.stderr.startswith("error: ") and "usage: grt" in r.stderr, r.stderr
        for word in words:
            assert word in r.stderr, r.stderr
        # the usage text names the flags, the pinned pair as it was
        assert "[--adaptive | --retarded]" in r.stderr and "[--adaptive-retarded]" in r.stderr and "[--lapse]" in r.stderr

    # the pinned one: --retarded shades the 1-spp frames
    usage_error(_run(*orbit, "--retarded", "--adaptive"), "does not combine with --adaptive", "--adaptive-retarded")
    # the new flag stands alone
    usage_error(_run(*orbit, "--adaptive-retarded", "--adaptive"), "--adaptive-retarded does not combine")
    usage_error(_run(*orbit, "--adaptive-retarded", "--retarded"), "--adaptive-retarded does not combine")
    # a missing .lapse is a usage error before the scene is loaded or the GPU touched
    usage_error(_run(*orbit, "--adaptive-retarded"), "needs the lapse sidecar " + str(path) + ".lapse")
    grt.GBuffer.write_lapse_file(str(path) + ".lapse", info, np.zeros(0))
    # a .sub without its .sub.lapse: remove it, or trace it again
    sub = L.GBufferSubInfo()
    empty = {k: v[:0] for k, v in arrays.items()}
    empty["layer_start"] = np.zeros(1, np.uint64)
    empty["sub_pixel"] = np.zeros(0, np.uint32)
    grt.GBuffer.write_sub_file(str(path) + ".sub", info, sub, empty)
    usage_error(_run(*orbit, "--adaptive-retarded"), str(path) + ".sub has no lapse sidecar", "remove it",
                "gbuffer --adaptive --lapse")
    # the flag belongs to reshade-orbit
    assert _run("--config-file", scene, "reshade", "--gbuffer", str(path), "--adaptive-retarded").returncode == 2
    assert _run("--config-file", scene, "gbuffer", "--adaptive-retarded", "--filename", str(path)).returncode == 2
    # damaged or foreign sidecars: an error message, not a crash, no frame
    side = tmp_path / "frame.grtg.sub.lapse"
    other, _ = _synthetic(grt, [0] * 6)
    grt.GBuffer.write_sub_lapse_file(side, other, sub, np.zeros(0))
    r = _run(*orbit, "--adaptive-retarded")
    assert r.returncode == 1 and "another g-buffer" in r.stderr, r.stderr
    grown = L.GBufferSubInfo(2, 0, 1, 4, 0)
    grt.GBuffer.write_sub_lapse_file(side, info, grown, np.zeros(0))
    r = _run(*orbit, "--adaptive-retarded")
    assert r.returncode == 1 and "another sub-sample set" in r.stderr, r.stderr
    grt.GBuffer.write_sub_lapse_file(side, info, sub, np.zeros(0))
    side.write_bytes(side.read_bytes()[:-3])
    r = _run(*orbit, "--adaptive-retarded")
    assert r.returncode == 1 and "too short" in r.stderr, r.stderr
    other_lapse = tmp_path / "frame.grtg.lapse"
    other_lapse.write_bytes(other_lapse.read_bytes()[:-3])
    r = _run(*orbit, "--adaptive-retarded")
    assert r.returncode == 1 and "too short" in r.stderr, r.stderr
    assert not list(tmp_path.glob("f-*.png"))


# --------------------------------------------------------------- kernels and hashes ----
KERNELS = ("gbuffer_shade_at_retarded_kernel", "gbuffer_shade_sub_at_retarded_kernel")


def test_new_kernels_are_in_the_library(grt):
    syms = grt._lib.kernel_symbols()
    for kernel in KERNELS:
        assert sum(s.startswith(f"_ZN3grt{len(kernel)}{kernel}E") for s in syms) == 1, kernel
    # the timed set is filled by the lapse units as they were: no kernel of theirs was added
    assert sum(s.startswith("_ZN3grt5lapse") or s.startswith("_ZN3grt13lapse_kerr_bl") for s in syms) == 16


def test_recorded_kernel_hashes():
    """profiles/gbuffer/sub_lapse_kernel_hashes.json (tools/kernel_hashes.py on a build of the
    parent commit and on a build of this change): every kernel of the parent kept its code in
    all units, the deferred-shade kernels and the lapse units' among them; the two retarded
    single-time shade kernels are new, within their siblings' registers."""
    doc = json.loads((ROOT / "profiles" / "gbuffer" / "sub_lapse_kernel_hashes.json").read_text())
    assert doc["parent"] == doc["this_change"] and len(doc["parent"]) == doc["n_existing"] == 191
    assert doc["existing_kernels_unchanged"] is True
    for kernel in ("gbuffer_shade_kernel", "gbuffer_shade_sub_kernel", "gbuffer_shade_at_kernel", "gbuffer_shade_sub_at_kernel",
                   "gbuffer_shade_times_kernel", "gbuffer_shade_times_retarded_kernel", "gbuffer_shade_stack_kernel",
                   "gbuffer_shade_sub_stack_kernel", "gbuffer_orbit_rate_kernel"):
        hits = [k for k in doc["parent"] if k.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1 and len(doc["parent"][hits[0]]) == 64, kernel
    assert sum(k.startswith("_ZN3grt5lapse") or k.startswith("_ZN3grt13lapse_kerr_bl") for k in doc["parent"]) == 16
    new = doc["new_kernels"]
    assert len(new) == doc["n_new"] == 2 and not set(new) & set(doc["parent"])
    assert all(len(v) == 64 for v in new.values())
    for kernel in KERNELS:
        assert sum(k.startswith(f"_ZN3grt{len(kernel)}{kernel}E") for k in new) == 1, kernel
    # the register lines: no scratch, no VGPR spill, 4 waves per SIMD, the glibc tables' LDS
    assert [row["kernel"] for row in doc["resources"]] == list(KERNELS)
    for row in doc["resources"]:
        for side in ("retarded", "fast_light"):
            r = row[side]
            assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["vgprs"] <= 128, row
            assert r["waves_per_simd"] == 4 and r["lds_bytes"] == 8640, row
        assert row["retarded"]["vgprs"] == row["fast_light"]["vgprs"], row
