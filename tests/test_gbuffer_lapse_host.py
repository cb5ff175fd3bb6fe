"""The host side of the retarded-time animation (grt_gbuffer_orbit_uv_retarded, the lapse's
sidecar; CPU only, no GPU call): the retarded rule against the fast-light one on bits, the
sidecar's round trips and every rejection, the ctypes mirrors against the header, the
stand-alone sanitizer program of tools/, the CLI's usage errors, and the recorded kernel hashes."""
import ctypes as C
import errno
import json
import math
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES
from test_gbuffer_host import COUNTS_MIXED, _synthetic
from test_gbuffer_orbit_host import _CTYPE, _bits, _declaration, _layers, _run, _shape

INFO_BYTES = 16  # magic, version, info-block size: then the info, n_layers, the doubles


# ------------------------------------------------------------------ the retarded rule ----
def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


TIMES = (0.0, 1.0, 37.5, -12.25, 700.0)


@pytest.mark.parametrize("geom,a", [("GEOM_KERR_BL", 0.499), ("GEOM_SCHWARZSCHILD", 0.0), ("GEOM_KERR", -0.3)])
def test_retarded_rule_against_the_fast_light_rule(grt, geom, a):
    L = grt._lib
    geometry = getattr(L, geom)
    obj, u, v, radius = _layers()
    disc = obj == 0
    shape = _shape(grt, geometry, a)
    zero = np.zeros(len(obj))
    for t in TIMES:
        want = grt.gbuffer_orbit_uv(shape, obj, u, v, radius, t)
        # lapse == 0: the fast-light rule at the same time, on bits (-0.0 too: t + -0.0 is t)
        assert _same(grt.gbuffer_orbit_uv_retarded(shape, obj, u, v, radius, zero, t), want), (geom, t)
        assert _same(grt.gbuffer_orbit_uv_retarded(shape, obj, u, v, radius, -zero, t), want), (geom, t)
        # lapse == c: the fast-light rule at the double t + c
        for c in (-41.625, -0.1, -1e-9, 3.0):
            got = grt.gbuffer_orbit_uv_retarded(shape, obj, u, v, radius, np.full(len(obj), c), t)
            assert _same(got, grt.gbuffer_orbit_uv(shape, obj, u, v, radius, t + c)), (geom, t, c)
    # a lapse per layer: sphere layers unchanged, a disc layer's lookup angle decreases by
    # omega (t + lapse) within the 1e-12 of tests/test_gbuffer_orbit_host.py
    rng = np.random.default_rng(3)
    lapse = -rng.uniform(0.5, 60.0, len(obj))
    omega = np.array([grt.orbit_rate(geometry, 1.0, a, float(r)) for r in radius])
    for t in TIMES:
        assert np.abs(omega[disc] * (t + lapse[disc])).max() <= 100.0
        uo, vo = grt.gbuffer_orbit_uv_retarded(shape, obj, u, v, radius, lapse, t)
        assert np.array_equal(_bits(uo[~disc]), _bits(u[~disc])) and np.array_equal(_bits(vo[~disc]), _bits(v[~disc]))
        du, dv, duo, dvo = u[disc] - 0.5, v[disc] - 0.5, uo[disc] - 0.5, vo[disc] - 0.5
        want = np.arctan2(dv, du) - omega[disc] * (t + lapse[disc])
        d = np.mod(np.arctan2(dvo, duo) - want + math.pi, 2.0 * math.pi) - math.pi
        assert np.abs(d).max() <= 1e-12, (geom, t, np.abs(d).max())
        assert np.abs(np.hypot(duo, dvo) - np.hypot(du, dv)).max() <= 1e-15, (geom, t)
        # and it is not the fast-light frame
        fu, fv = grt.gbuffer_orbit_uv(shape, obj, u, v, radius, t)
        assert np.abs(uo[disc] - fu[disc]).max() > 0.01


def test_retarded_rule_flat_charts_and_empty(grt):
    L = grt._lib
    obj, u, v, radius = _layers()
    lapse = -np.linspace(1.0, 50.0, len(obj))
    for g in (L.GEOM_EUCLIDEAN, L.GEOM_EUCLIDEAN_SPHERICAL):  # omega == 0: unchanged at every time
        uo, vo = grt.gbuffer_orbit_uv_retarded(_shape(grt, g), obj, u, v, radius, lapse, 37.5)
        assert np.array_equal(_bits(uo), _bits(u)) and np.array_equal(_bits(vo), _bits(v))
    e = np.zeros(0)
    uo, vo = grt.gbuffer_orbit_uv_retarded(_shape(grt), np.zeros(0, np.uint8), e, e, e, e, 1.0)
    assert uo.shape == vo.shape == (0,)


def _call(grt, shape, obj, u, v, radius, lapse, t, uo, vo, n=None):
    L = grt._lib
    p = lambda x: None if x is None else L.dptr(x)  # noqa: E731
    return L.lib().grt_gbuffer_orbit_uv_retarded(C.byref(shape) if shape is not None else None,
                                                 len(obj) if n is None else n,
                                                 None if obj is None else L.ptr(obj, C.c_uint8), p(u), p(v), p(radius),
                                                 p(lapse), t, p(uo), p(vo))


def test_retarded_rule_aliasing_and_refusals(grt):
    L = grt._lib
    obj, u, v, radius = _layers(64)
    lapse = -np.linspace(1.0, 50.0, 64)
    shape = _shape(grt)
    want = grt.gbuffer_orbit_uv_retarded(shape, obj, u, v, radius, lapse, 37.5)
    ua, va = u.copy(), v.copy()
    assert _call(grt, shape, obj, ua, va, radius, lapse, 37.5, ua, va) == 0
    assert _same((ua, va), want) and not np.array_equal(_bits(ua), _bits(u))
    uo, vo = np.full(64, 9.0), np.full(64, 9.0)
    good = [shape, obj, u, v, radius, lapse, 1.0, uo, vo]
    for k in (0, 2, 3, 4, 5, 7, 8):  # every pointer but `object`, then that one
        args = list(good)
        args[k] = None
        assert _call(grt, *args) == -errno.EINVAL, k
    assert _call(grt, shape, None, u, v, radius, lapse, 1.0, uo, vo, n=64) == -errno.EINVAL
    for t in (float("nan"), float("inf"), float("-inf")):
        assert _call(grt, shape, obj, u, v, radius, lapse, t, uo, vo) == -errno.EINVAL, t
        assert "time" in L.lib().grt_last_error().decode()
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = lapse.copy()
        x[63] = bad
        assert _call(grt, shape, obj, u, v, radius, x, 1.0, uo, vo) == -errno.EINVAL, bad
        assert "lapse" in L.lib().grt_last_error().decode()
    bad = obj.copy()
    bad[63] = 2  # == n_objects
    assert _call(grt, shape, bad, u, v, radius, lapse, 1.0, uo, vo) == -errno.EINVAL
    assert _call(grt, _shape(grt, 99), obj, u, v, radius, lapse, 1.0, uo, vo) == -errno.EINVAL
    assert np.all(uo == 9.0) and np.all(vo == 9.0)  # a refused call writes nothing
    with pytest.raises(grt.GrtError):
        grt.gbuffer_orbit_uv_retarded(shape, obj, u, v, radius, lapse[:10], 1.0)


# ------------------------------------------------------------------------ the sidecar ----
def _lapse_of(info, seed=9):
    return -np.random.default_rng(seed).uniform(0.0, 60.0, int(info.n_layers))


@pytest.mark.parametrize("counts", [COUNTS_MIXED, [0] * 6], ids=["many", "no-layers"])
def test_sidecar_round_trip(grt, tmp_path, counts):
    L = grt._lib
    info, _ = _synthetic(grt, counts)
    lapse = _lapse_of(info)
    if lapse.size:
        lapse[0] = -0.0  # bits, not values, survive
    path = tmp_path / "a.grtg.lapse"
    grt.GBuffer.write_lapse_file(path, info, lapse)
    assert path.stat().st_size == INFO_BYTES + C.sizeof(L.GBufferInfo) + 8 + 8 * lapse.size
    assert path.read_bytes()[:8] == b"GRTGLPS\0"
    back = grt.GBuffer.read_lapse_file(path, info)
    assert np.array_equal(_bits(back), _bits(lapse))
    info.device = 3  # a load changes the device: not part of what binds the sidecar
    assert np.array_equal(_bits(grt.GBuffer.read_lapse_file(path, info)), _bits(lapse))
    assert L.lib().grt_gbuffer_lapse_read_file(str(path).encode(), C.byref(info), None) == 0  # the check alone


def test_sidecar_rejections(grt, tmp_path):
    L = grt._lib
    info, _ = _synthetic(grt, COUNTS_MIXED)
    lapse = _lapse_of(info)
    n = lapse.size
    path, cut = tmp_path / "a.grtg.lapse", tmp_path / "cut.lapse"
    grt.GBuffer.write_lapse_file(path, info, lapse)
    whole = path.read_bytes()
    at_count = INFO_BYTES + C.sizeof(L.GBufferInfo)

    def refused(data, bound=info, word=None):
        cut.write_bytes(data)
        out = np.full(n, 9.0)
        rc = L.lib().grt_gbuffer_lapse_read_file(str(cut).encode(), C.byref(bound), L.dptr(out))
        assert rc == -errno.EINVAL and np.all(out == 9.0), (rc, len(data))
        if word:
            assert word in L.lib().grt_last_error().decode(), L.lib().grt_last_error().decode()
        assert L.lib().grt_gbuffer_lapse_read_file(str(cut).encode(), C.byref(bound), None) == -errno.EINVAL

    # a truncation at each section boundary and inside each section, one byte short, one too many
    for length in (0, 7, 8, 12, 16, 17, at_count - 1, at_count, at_count + 7, at_count + 8, at_count + 8 + 8,
                   len(whole) - 8, len(whole) - 1):
        refused(whole[:length])
    refused(whole + b"\0", word="file length")
    refused(b"GRTGSUB\0" + whole[8:], word="magic")
    refused(whole[:8] + (2).to_bytes(4, "little") + whole[12:], word="version")
    refused(whole[:12] + (8).to_bytes(4, "little") + whole[16:], word="info block")
    # an inconsistent count: the header's against the buffer's, with and without the doubles to match
    refused(whole[:at_count] + (n - 1).to_bytes(8, "little") + whole[at_count + 8:], word="entries")
    refused(whole[:at_count] + (n - 1).to_bytes(8, "little") + whole[at_count + 8:-8], word="entries")
    refused(whole[:at_count] + (1 << 62).to_bytes(8, "little") + whole[at_count + 8:], word="entries")
    nan = np.array([np.nan]).tobytes()
    refused(whole[:at_count + 8 + 8 * 5] + nan + whole[at_count + 8 + 8 * 6:], word="not finite")
    # a sidecar whose info differs from the buffer's
    for field, value in (("rows", 4), ("row0", 0), ("max_steps", 7), ("epsilon", 1e-6)):
        other, _ = _synthetic(grt, COUNTS_MIXED)
        setattr(other, field, value)
        if field == "rows":
            other.cols, other.n_pixels = 3, 12
        refused(whole, bound=other, word="another g-buffer")
    other, _ = _synthetic(grt, COUNTS_MIXED)
    other.camera.position[1] = 2.0
    refused(whole, bound=other, word="another g-buffer")
    other, _ = _synthetic(grt, COUNTS_MIXED)
    other.shape.objects[1].radius = 7.0
    refused(whole, bound=other, word="another g-buffer")
    # the writer's refusals, and the files that are not there
    w = L.lib().grt_gbuffer_lapse_write_file
    assert w(str(cut).encode(), C.byref(info), L.dptr(lapse), n - 1) == -errno.EINVAL
    bad = lapse.copy()
    bad[3] = np.inf
    assert w(str(cut).encode(), C.byref(info), L.dptr(bad), n) == -errno.EINVAL
    assert w(str(cut).encode(), C.byref(info), None, n) == -errno.EINVAL
    assert w(None, C.byref(info), L.dptr(lapse), n) == -errno.EINVAL
    assert w(str(cut).encode(), None, L.dptr(lapse), n) == -errno.EINVAL
    assert w(str(tmp_path / "no" / "dir.lapse").encode(), C.byref(info), L.dptr(lapse), n) == -errno.EIO
    assert L.lib().grt_gbuffer_lapse_read_file(str(tmp_path / "absent").encode(), C.byref(info), None) == -errno.EIO
    assert L.lib().grt_gbuffer_lapse_read_file(None, C.byref(info), None) == -errno.EINVAL
    assert L.lib().grt_gbuffer_lapse_read_file(str(path).encode(), None, None) == -errno.EINVAL


# ----------------------------------------------------------- mirrors and the tools ----
NEW = ("grt_gbuffer_trace_lapse", "grt_gbuffer_lapse_download", "grt_gbuffer_lapse_upload", "grt_gbuffer_lapse_write_file",
       "grt_gbuffer_lapse_read_file", "grt_gbuffer_orbit_uv_retarded", "grt_gbuffer_shade_times_retarded")


def test_ctypes_mirrors_match_the_header(grt):
    L = grt._lib
    types = dict(_CTYPE)
    types.update({"grt_gbuffer_shape*": C.POINTER(L.GBufferShape), "grt_frame_out*": C.POINTER(L.FrameOut),
                  "grt_gbuffer_info*": C.POINTER(L.GBufferInfo), "grt_stats*": C.POINTER(L.Stats),
                  "grt_gbuffer**": C.POINTER(C.c_void_p), "char*": C.c_char_p, "int": C.c_int})
    for name in NEW:
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)
        fn = getattr(L.lib(), name)
        want = [types[t] for t in _declaration(name)]
        assert fn.restype is C.c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    # the lapse entry points take their fast-light siblings' arguments
    assert _declaration("grt_gbuffer_trace_lapse") == _declaration("grt_gbuffer_trace")
    assert _declaration("grt_gbuffer_shade_times_retarded") == _declaration("grt_gbuffer_shade_times")
    uv, ret = _declaration("grt_gbuffer_orbit_uv"), _declaration("grt_gbuffer_orbit_uv_retarded")
    assert ret == uv[:6] + ["double*"] + uv[6:]
    header = (ROOT / "include" / "grt_api.h").read_text()
    assert "#define GRT_ABI_VERSION 3" in header and "#define GRT_GBUFFER_FILE_VERSION 1" in header


def test_stand_alone_sanitizer_program(tmp_path):
    """tools/lapse_main.cpp over the three host files alone, built with the address and undefined
    behaviour sanitizers and run on the CPU: the retarded rule on 0, 1, 7 and 1000 layers,
    aliased and separate, and the sidecar's reader on every truncation of a small file."""
    exe = tmp_path / "lapse_main"
    host = ROOT / "gr_raytracer_amd" / "csrc" / "host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "include"), str(ROOT / "tools" / "lapse_main.cpp"),
                    str(host / "orbit.cpp"), str(host / "gbuffer.cpp"), str(host / "errors.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    assert not list(tmp_path.glob("*.lapse"))  # it removes its files


# ------------------------------------------------------------------------- the CLI ----
def test_cli_usage_errors(grt, tmp_path):
    scene = str(SCENES / "schwarzschild.toml")
    pat = str(tmp_path / "f-%04d.png")
    info, arrays = _synthetic(grt, [0] * 6)
    info.row0 = info.col0 = 0
    info.camera.rows, info.camera.cols = info.rows, info.cols
    path = tmp_path / "frame.grtg"
    grt.GBuffer.write_file(path, info, arrays)
    orbit = ["--width", "2", "--height", "3", "--config-file", scene, "reshade-orbit", "--gbuffer", str(path), "--times",
             "0,1,3", "--filename-pattern", pat]

    def usage_error(r, word):
        assert r.returncode == 2 and r.stderr.startswith("error: ") and "usage: grt" in r.stderr, r.stderr
        assert word in r.stderr, r.stderr
        assert "[--adaptive | --retarded]" in r.stderr and "[--lapse]" in r.stderr  # the usage text names the flags

    # a missing sidecar is a usage error before the GPU is touched
    usage_error(_run(*orbit, "--retarded"), "needs the lapse sidecar " + str(path) + ".lapse")
    usage_error(_run(*orbit, "--retarded", "--adaptive"), "does not combine with --adaptive")
    usage_error(_run("--gpus", "2", "--config-file", scene, "gbuffer", "--lapse", "--filename", str(tmp_path / "a.grtg")),
                "records no lapse")
    # the flags belong to their subcommands
    assert _run("--config-file", scene, "reshade", "--gbuffer", str(path), "--retarded").returncode == 2
    assert _run("--config-file", scene, "reshade-orbit", "--lapse", "--gbuffer", str(path)).returncode == 2
    # a sidecar of another buffer, and a damaged one: an error message, not a crash, no frame
    other, _ = _synthetic(grt, [0] * 6)
    grt.GBuffer.write_lapse_file(str(path) + ".lapse", other, np.zeros(0))
    r = _run(*orbit, "--retarded")
    assert r.returncode == 1 and "another g-buffer" in r.stderr, r.stderr
    grt.GBuffer.write_lapse_file(str(path) + ".lapse", info, np.zeros(0))
    sidecar = tmp_path / "frame.grtg.lapse"
    sidecar.write_bytes(sidecar.read_bytes()[:-3])
    r = _run(*orbit, "--retarded")
    assert r.returncode == 1 and "too short" in r.stderr, r.stderr
    assert not list(tmp_path.glob("f-*.png"))


# --------------------------------------------------------------- recorded hashes ----
KERNELS = {"gbuffer_shade_times_retarded_kernel": 1}
UNITS = {"5lapse": {"integrate_kernel": 4, "tail_kernel": 1, "shade_kernel": 4, "gbuffer_fill_kernel": 4},
         "13lapse_kerr_bl": {"integrate_kernel": 1, "shade_kernel": 1, "gbuffer_fill_kernel": 1}}


def test_new_kernels_are_in_the_library(grt):
    syms = grt._lib.kernel_symbols()
    for kernel in KERNELS:
        assert sum(s.startswith(f"_ZN3grt{len(kernel)}{kernel}E") for s in syms) == 1, kernel
    for unit, kernels in UNITS.items():
        for kernel, count in kernels.items():
            hits = [s for s in syms if s.startswith(f"_ZN3grt{unit}{len(kernel)}{kernel}I")]
            assert len(hits) == len(set(hits)) == count, (unit, kernel, hits)
    assert sum(s.startswith("_ZN3grt5lapse") or s.startswith("_ZN3grt13lapse_kerr_bl") for s in syms) == 16


def test_recorded_kernel_hashes():
    """profiles/gbuffer/lapse_kernel_hashes.json (tools/kernel_hashes.py on a build of the parent
    commit and on a build of this change): every kernel of the parent kept its code in all units,
    the static and fast-light deferred-shade kernels and every integrate kernel among them; the
    kernels of the lapse units and the retarded shade are new."""
    doc = json.loads((ROOT / "profiles" / "gbuffer" / "lapse_kernel_hashes.json").read_text())
    assert doc["parent"] == doc["this_change"] and len(doc["parent"]) == doc["n_existing"] > 160
    assert doc["existing_kernels_unchanged"] is True
    for kernel in ("gbuffer_shade_kernel", "gbuffer_shade_times_kernel", "gbuffer_shade_at_kernel",
                   "gbuffer_shade_sub_at_kernel", "gbuffer_shade_stack_kernel", "gbuffer_orbit_rate_kernel"):
        hits = [k for k in doc["parent"] if k.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1 and len(doc["parent"][hits[0]]) == 64, kernel
    assert sum("integrate_kernelILi" in k for k in doc["parent"]) >= 10  # every chart, every unit
    assert sum("gbuffer_fill_kernelILi" in k for k in doc["parent"]) >= 10
    new = doc["new_kernels"]
    assert len(new) == doc["n_new"] == 17 and not set(new) & set(doc["parent"])
    assert all(len(v) == 64 for v in new.values())
    assert sum(k.startswith("_ZN3grt5lapse") for k in new) == 13 and sum(k.startswith("_ZN3grt13lapse_kerr_bl") for k in new) == 3
    # the register table: each new integrate, tail and fill kernel beside its exact sibling
    for row in doc["resources"]:
        for side in ("lapse", "exact"):
            assert {"vgprs", "sgprs", "scratch_bytes", "waves_per_simd"} <= set(row[side]), row
        # no kernel of the lapse units gained a vector register, scratch or lost occupancy (a fill
        # kernel may hold its extra pointer in scalar registers)
        for key in ("vgprs", "scratch_bytes", "waves_per_simd"):
            assert row["lapse"][key] == row["exact"][key], (row, key)
        assert row["lapse"]["sgprs"] >= row["exact"]["sgprs"], row
    assert len(doc["resources"]) == 5 + 1 + 5
