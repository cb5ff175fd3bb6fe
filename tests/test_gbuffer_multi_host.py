"""Host side of the multi-GPU geometry buffer (grt_gbuffer_trace_multi): the exported entry
point and the report's layout, the two assembly kernels in the library, the assembly's index
arithmetic run on the host (grt_debug_gbuffer_gather_host) against distributed.shard_frame_rows,
the CLI's usage errors and the recorded kernel hashes.  CPU only.
"""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GRT = ROOT / "gr_raytracer_amd" / "lib" / "grt"
KERNELS = ("gbuffer_gather_pixels_kernel", "gbuffer_gather_layers_kernel")
# grt_gbuffer_arrays' members: per pixel, layer_start, per layer
PIXEL = (("status", np.uint8), ("stop", np.uint8), ("steps", np.uint32), ("sky_u", np.float64), ("sky_v", np.float64),
         ("sky_redshift", np.float64))
LAYER = (("object", np.uint8), ("u", np.float64), ("v", np.float64), ("redshift", np.float64), ("radius", np.float64))
GUARD = 64


# ------------------------------------------------------------- symbols and layout ----
def test_entry_point_is_exported(grt):
    from gr_raytracer_amd import _lib as L

    assert "grt_gbuffer_trace_multi" in L.EXPORTED_SYMBOLS and hasattr(L.lib(), "grt_gbuffer_trace_multi")
    assert hasattr(L.lib(), "grt_debug_gbuffer_gather_host")
    assert callable(grt.Scene.trace_gbuffer_multi)


def test_multi_report_layout_matches_header(grt, tmp_path):
    from gr_raytracer_amd import _lib as L

    fields = ("n_devices", "transport", "n_traces", "rows", "layers", "block_bytes", "trace_ms", "fill_ms", "gather_ms",
              "wall_ms")
    src = tmp_path / "size.c"
    offs = "".join(f'  printf("%zu\\n", offsetof(grt_gbuffer_multi_report, {f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grt_api.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(grt_gbuffer_multi_report));\n' + offs + '  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    R = L.GBufferMultiReport
    assert [int(v) for v in out] == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    assert [f for f, _ in R._fields_] == list(fields)
    assert R.n_traces.size == 4 * L.GRT_MULTI_MAX_DEVICES and R.rows.size == 8 * L.GRT_MULTI_MAX_DEVICES


def test_library_carries_the_gather_kernels(grt):
    from gr_raytracer_amd import _lib as L

    syms = L.kernel_symbols()
    for kernel in KERNELS:
        hits = [s for s in syms if s.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1, (kernel, hits)
        assert len(L.kernel_code_sha256(hits[0])) == 64


# --------------------------------------------------------------------- host twin ----
def _encode(index, field, dtype):
    """A value per (index, field) that no other (index, field) of the same width has, up to
    the width: the bit pattern index * 16 + field, truncated."""
    v = index.astype(np.uint64) * 16 + field
    if dtype == np.float64:
        return v.view(np.float64)
    return v.astype(dtype)  # u8 / u32: wraps


def _frame(rng, rows, cols, band, layers=True):
    """A synthetic frame buffer (dict by member): counts from {0..20}, one band without layers."""
    n = rows * cols
    counts = rng.integers(0, 21, n).astype(np.uint64) if layers else np.zeros(n, np.uint64)
    n_bands = -(-rows // band)
    empty_band = None
    if layers and n_bands >= 2:
        empty_band = int(rng.integers(0, n_bands))
        counts[empty_band * band * cols:(empty_band + 1) * band * cols] = 0
    start = np.zeros(n + 1, np.uint64)
    np.cumsum(counts, out=start[1:])
    total = int(start[-1])
    a = {"layer_start": start}
    for f, (k, t) in enumerate(PIXEL):
        a[k] = _encode(np.arange(n), f, t)
    for f, (k, t) in enumerate(LAYER):
        a[k] = _encode(np.arange(total), 8 + f, t)
    return a, counts, empty_band


def _cut(frame, counts, local):
    """The shard buffer of the frame pixels `local` (in local order)."""
    cnt = counts[local]
    start = np.zeros(len(local) + 1, np.uint64)
    np.cumsum(cnt, out=start[1:])
    first = frame["layer_start"][:-1][local]
    # frame layer of each local layer: the pixel's first frame layer plus the place in the pixel
    idx = (np.repeat(first - start[:-1], cnt.astype(np.int64)) + np.arange(int(start[-1]), dtype=np.uint64)).astype(np.int64)
    a = {"layer_start": start}
    for k, _ in PIXEL:
        a[k] = frame[k][local]
    for k, _ in LAYER:
        a[k] = frame[k][idx]
    return a


def _guarded(arr):
    """(buffer, address of the payload): the array's bytes in an allocation of their own,
    sized exactly, between two runs of 0xEE."""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = np.full(raw.size + 2 * GUARD, 0xEE, np.uint8)
    buf[GUARD:GUARD + raw.size] = raw
    assert (buf.ctypes.data + GUARD) % 8 == 0
    return buf, buf.ctypes.data + GUARD


def _guards_intact(buf):
    return bool(np.all(buf[:GUARD] == 0xEE) and np.all(buf[-GUARD:] == 0xEE))


def _arrays_struct(L, addr):
    return L.GBufferArrays(**{k: C.cast(C.c_void_p(addr[k]), t) for k, t in L.GBufferArrays._fields_})


def test_gather_host_matches_shard_frame_rows(grt):
    """The two kernels' index functions, in plain loops over host arrays: frames cut into
    shard buffers by distributed.shard_frame_rows come back byte for byte in all twelve
    arrays, every array an allocation of its own between guard bytes."""
    from gr_raytracer_amd import _lib as L
    from gr_raytracer_amd.distributed import shard_frame_rows

    gather = L.lib().grt_debug_gbuffer_gather_host
    gather.restype = C.c_int
    gather.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(L.GBufferArrays), C.POINTER(C.c_uint64),
                       C.POINTER(L.GBufferArrays)]
    rng = np.random.default_rng(20261020)
    names = [k for k, _ in PIXEL] + ["layer_start"] + [k for k, _ in LAYER]
    empty_ranks = None
    n_empty_bands = n_cases = 0
    for rows, cols in ((1, 5), (7, 3), (40, 36), (20, 9), (257, 9)):
        for n in range(1, 9):
            for band in (1, 8, 16):
                for layers in (True, False):  # and a frame without any layer
                    frame, counts, empty_band = _frame(rng, rows, cols, band, layers)
                    n_empty_bands += empty_band is not None
                    held, shards, n_local = [], (L.GBufferArrays * n)(), (C.c_uint64 * n)()
                    for s in range(n):
                        fr = shard_frame_rows(rows, band, s, n)
                        local = (fr[:, None] * cols + np.arange(cols)[None, :]).reshape(-1).astype(np.int64)
                        n_local[s] = len(local)
                        if len(local) == 0:
                            continue  # a rank without rows: null arrays, never read
                        cut = _cut(frame, counts, local)
                        bufs = {k: _guarded(cut[k]) for k in names}
                        held.append(bufs)
                        shards[s] = _arrays_struct(L, {k: b[1] for k, b in bufs.items()})
                    if (rows, cols, band, n) == (20, 9, 8, 8):
                        empty_ranks = sum(n_local[s] == 0 for s in range(n))
                    out = {k: _guarded(np.zeros_like(frame[k])) for k in names}
                    dst = _arrays_struct(L, {k: b[1] for k, b in out.items()})
                    rc = gather(rows, cols, band, n, shards, n_local, C.byref(dst))
                    assert rc == 0, (rows, cols, n, band, L.lib().grt_last_error())
                    for k in names:
                        buf = out[k][0]
                        want = np.ascontiguousarray(frame[k]).view(np.uint8).reshape(-1)
                        assert np.array_equal(buf[GUARD:buf.size - GUARD], want), (rows, cols, n, band, k)
                        assert _guards_intact(buf), (rows, cols, n, band, k, "frame guard")
                    for bufs in held:
                        assert all(_guards_intact(b[0]) for b in bufs.values()), (rows, cols, n, band, "shard guard")
                    n_cases += 1
    assert empty_ranks == 5  # (20, 9), band 8, n = 8: ranks 3..7 own no row
    assert n_cases == 2 * 5 * 8 * 3 and n_empty_bands >= 80


def test_gather_host_refuses_bad_arguments(grt):
    from gr_raytracer_amd import _lib as L

    gather = L.lib().grt_debug_gbuffer_gather_host
    gather.restype = C.c_int
    gather.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    shards, n_local, frame = (L.GBufferArrays * 1)(), (C.c_uint64 * 1)(4), L.GBufferArrays()
    assert gather(2, 2, 0, 1, shards, n_local, C.byref(frame)) == -22  # band_rows = 0
    assert gather(2, 2, 8, 17, shards, n_local, C.byref(frame)) == -22  # more than 16 shards
    assert gather(2, 2, 8, 1, None, n_local, C.byref(frame)) == -22
    n_local[0] = 3
    assert gather(2, 2, 8, 1, shards, n_local, C.byref(frame)) == -22  # not the shard's pixel count
    n_local[0] = 4
    assert gather(2, 2, 8, 1, shards, n_local, C.byref(frame)) == -22  # null arrays of a shard with rows


# ------------------------------------------------------------------ usage errors ----
@pytest.mark.parametrize("args,needles", [
    (["--gpus", "2", "gbuffer", "--filename", "a.grtg", "--adaptive"], ("gbuffer --adaptive", "--gpus", "reshade --adaptive")),
    (["--gpus", "2", "reshade", "--gbuffer", "a.grtg"], ("reshade", "--gpus", "gbuffer --gpus", "reshade [--adaptive]")),
    (["--devices", "0,x", "gbuffer", "--filename", "a.grtg"], ("--devices", "0,x")),
    (["--transport", "bogus", "--gpus", "1", "gbuffer", "--filename", "a.grtg"], ("--transport", "bogus")),
    (["--devices", "0,0", "gbuffer-sequence", "--camera-path", "PATH", "--filename-pattern", "a-%04d.grtg"],
     ("--devices", "gbuffer --gpus")),
])
def test_usage_errors_come_before_the_scene_and_the_gpu(tmp_path, args, needles):
    """Neither the config file nor the .grtg file exists: the run ends on its arguments, and
    the message names the route (trace with --gpus, then reshade --adaptive tops up)."""
    r = subprocess.run([str(GRT), "--config-file", str(tmp_path / "missing.toml"), *args], capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    first = r.stderr.splitlines()[0]
    assert all(n in first for n in needles) and "usage:" in r.stderr, r.stderr
    assert not list(tmp_path.glob("*.grtg"))


def test_usage_text_names_the_device_list_of_gbuffer(tmp_path):
    r = subprocess.run([str(GRT), "gbuffer"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and "the 1-spp trace over several GPUs" in r.stderr, r.stderr


# --------------------------------------------------------------- recorded hashes ----
def test_recorded_kernel_hashes():
    """profiles/gbuffer/multi_kernel_hashes.json (tools/kernel_hashes.py on a build of the
    parent commit and on a build of this change): every kernel of the parent kept its code in
    all units; the two assembly kernels are new, without scratch or LDS."""
    doc = json.loads((ROOT / "profiles" / "gbuffer" / "multi_kernel_hashes.json").read_text())
    assert doc["parent"] == doc["this_change"] and len(doc["parent"]) == doc["n_existing"] > 150
    assert doc["existing_kernels_unchanged"] is True
    for kernel in ("gbuffer_count_kernel", "gbuffer_rebase_kernel", "gbuffer_shade_kernel", "deinterleave_kernel",
                   "gather_peer_kernel"):
        hits = [k for k in doc["parent"] if k.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1 and len(doc["parent"][hits[0]]) == 64, kernel
    assert sum("gbuffer_fill_kernelILi" in k for k in doc["parent"]) >= 10  # every chart, every unit
    new = doc["new_kernels"]
    assert len(new) == doc["n_new"] == 2 and not set(new) & set(doc["parent"])
    for kernel in KERNELS:
        assert any(k.startswith(f"_ZN3grt{len(kernel)}{kernel}E") for k in new), kernel
        res = doc["new_kernel_resources"][kernel]
        assert 0 < res["vgprs"] <= 64 and res["scratch_bytes"] == 0 and res["lds_bytes"] == 0, res
