"""The peer transports of the multi-GPU frame (grt_set_multi_transport, include/grt_api.h;
csrc/device/multi.hip): the frame's blocks move by direct peer reads ("peer",
gather_peer_kernel) or by peer copies into the reader's staging ("peer-staged"), without
RCCL, and a device list may name one GPU several times (one rank per entry).

CPU: the knob; gather_peer_kernel's per-pixel source function, run on the host through a
test hook with every shard's block an allocation of its own, against
distributed.shard_frame_rows; the CLI's --transport check.

GPU (marker `gpu`): every rank on the one GPU, devices = [gpu] * N.  This runs the whole
N > 1 host path (the receive of shards s >= 1, the de-interleave of real peer blocks, the
supersample pass's neighbourhoods across shards, the failure merge, the barrier with
several threads) and holds every frame to the single-device entry points bit for bit.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import RESOURCES, ROOT, SCENES, c2_opts, c4_opts, host_scene

FIELD_BYTES = [32, 16, 4, 1, 1, 1]  # RF_XYZA64, RF_XYZA32, RF_STEPS, RF_CLASS, RF_STATUS, RF_STOP
ALL_FIELDS = ("xyza", "xyza64", "class", "status", "stop", "steps")
TRANSPORTS = {"rccl": 0, "peer": 1, "peer-staged": 2}
EXE = ROOT / "gr_raytracer_amd" / "lib" / "grt"

both = pytest.mark.parametrize("transport", ["peer", "peer-staged"])


# ------------------------------------------------------------------------------- CPU ---
def test_transport_knob(grt):
    from gr_raytracer_amd import _lib as L

    lib = L.lib()
    assert lib.grt_get_multi_transport() == 0
    assert lib.grt_set_multi_transport(3) == -22 and lib.grt_set_multi_transport(-1) == -22
    assert lib.grt_get_multi_transport() == 0
    try:
        for mode in (1, 2, 0, 2):
            assert lib.grt_set_multi_transport(mode) == 0
            assert lib.grt_get_multi_transport() == mode
    finally:
        assert lib.grt_set_multi_transport(0) == 0
    assert lib.grt_get_multi_transport() == 0
    assert L.MULTI_TRANSPORTS == TRANSPORTS
    # grt_multi_report.transport sits where the padding was
    assert L.MultiReport.transport.offset == 12 and L.MultiReport.wall_ms.offset == 16


def _encode(p, nbytes, f):
    """Distinct bytes per (pixel, field): the pixel index and field number, little endian."""
    v = (p.astype(np.uint64) * 8 + f).view(np.uint8).reshape(-1, 8)
    reps = -(-nbytes // 8)
    return np.tile(v, (1, reps))[:, :nbytes]


@pytest.mark.parametrize("mask", [0b011010, 0b111111, 0b011001])
def test_gather_peer_matches_shard_frame_rows(grt, mask):
    from gr_raytracer_amd import _lib as L
    from gr_raytracer_amd.distributed import shard_frame_rows

    lib = L.lib()
    gather = lib.grt_debug_gather_peer_host
    gather.restype = C.c_int
    gather.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    block_bytes = lib.grt_debug_gather_block_bytes
    block_bytes.restype = C.c_uint64
    block_bytes.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p]
    empty_ranks = None
    for rows, cols in ((1, 5), (7, 3), (40, 36), (20, 9), (257, 9)):
        for n in range(1, 9):
            for band in (1, 8, 16):
                frame = rows * cols
                blocks = []
                for s in range(n):
                    fr = shard_frame_rows(rows, band, s, n)
                    local = (fr[:, None] * cols + np.arange(cols)[None, :]).reshape(-1)  # frame pixel of each local one
                    offs = np.zeros(6, np.uint64)
                    size = block_bytes(mask, len(local), offs.ctypes.data)
                    # a separate allocation per shard, poisoned so that a read outside a field shows
                    blk = np.full(max(int(size), 1), 0xEE, np.uint8)
                    for f in range(6):
                        if mask & (1 << f):
                            o = int(offs[f])
                            assert o % 256 == 0
                            e = FIELD_BYTES[f]
                            blk[o:o + len(local) * e] = _encode(local, e, f).reshape(-1)
                    blocks.append(blk)
                if (rows, cols, band, n) == (20, 9, 8, 8):
                    empty_ranks = sum(len(shard_frame_rows(rows, band, s, n)) == 0 for s in range(n))
                bptr = (C.c_void_p * n)(*[b.ctypes.data for b in blocks])
                dst = [np.zeros(frame * FIELD_BYTES[f], np.uint8) if mask & (1 << f) else None for f in range(6)]
                ptrs = (C.c_void_p * 6)(*[d.ctypes.data if d is not None else None for d in dst])
                assert gather(rows, cols, band, n, mask, bptr, ptrs) == 0
                for f in range(6):
                    if dst[f] is not None:
                        want = _encode(np.arange(frame), FIELD_BYTES[f], f).reshape(-1)
                        assert np.array_equal(dst[f], want), (rows, cols, n, band, f)
    assert empty_ranks == 5  # (20, 9), band 8, n = 8: ranks 3..7 own no row


def test_cli_rejects_an_unknown_transport(grt, tmp_path):
    r = subprocess.run([str(EXE), "--transport", "bogus", "--config-file", str(SCENES / "schwarzschild.toml"),
                        "--resource-root", str(RESOURCES), "render", "--filename", str(tmp_path / "x.png")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr
    assert "--transport" in r.stderr and "bogus" in r.stderr and "usage:" in r.stderr
    assert not (tmp_path / "x.png").exists()


# ------------------------------------------------------------------------------- GPU ---
def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _shard_rows(grt, rows, band, s, n):
    from gr_raytracer_amd import _lib as L

    sh = L.RowShard(band, s, n)
    return L.lib().grt_shard_row_count(rows, C.byref(sh))


def _check_1spp(grt, gpu, transport, height, n):
    hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt, width=64, height=height))
    scene = grt.Scene(hs.desc_ptr(), keepalive=hs)
    ref = scene.render_pixels(device=gpu)
    got = scene.render_frame_multi([gpu] * n, 8, fields=ALL_FIELDS, transport=transport)
    assert _same(got["xyza"], ref.xyza) and _same(got["xyza64"], ref.xyza64)
    assert _same(got["class"], ref.ray_class) and _same(got["status"], ref.status)
    assert _same(got["stop"], ref.stop_reason) and _same(got["steps"], ref.steps)
    rep = got["report"]
    assert rep.n_devices == n and rep.transport == TRANSPORTS[transport]
    assert rep.record_bytes == 32 + 16 + 4 + 3
    rows = [_shard_rows(grt, height, 8, s, n) for s in range(n)]
    assert sum(rows) == height
    assert [rep.rows[s] for s in range(n)] == rows
    assert sum(rep.accepted_steps[s] for s in range(n)) == ref.stats["accepted_steps"]
    assert got["stats"]["accepted_steps"] == ref.stats["accepted_steps"]
    assert got["stats"]["rays"] == 64 * height
    return rows


@pytest.mark.gpu
@both
@pytest.mark.parametrize("n", [2, 3, 8])
def test_peer_1spp_ragged_bands_equal_render_pixels(grt, gpu, transport, n):
    """64 x 76 in bands of 8: ten bands, the last one four rows short; at N = 8 ranks 0
    and 1 own two bands each."""
    rows = _check_1spp(grt, gpu, transport, 76, n)
    if n == 8:
        assert rows == [16, 12, 8, 8, 8, 8, 8, 8]
    from gr_raytracer_amd import _lib as L

    assert L.lib().grt_get_multi_transport() == 0  # the call restored the knob


@pytest.mark.gpu
@both
def test_peer_ranks_without_rows(grt, gpu, transport):
    """64 x 20 in bands of 8 over 8 ranks: ranks 3..7 trace nothing."""
    rows = _check_1spp(grt, gpu, transport, 20, 8)
    assert rows == [8, 8, 4, 0, 0, 0, 0, 0]


@pytest.mark.gpu
@both
def test_peer_kerr_schild_equals_render_pixels(grt, gpu, transport):
    hs = host_scene(grt, "kerr.toml", c4_opts(grt, width=48, height=40, max_steps=100000))
    scene = grt.Scene(hs.desc_ptr(), keepalive=hs)
    ref = scene.render_pixels(device=gpu)
    got = scene.render_frame_multi([gpu] * 3, 16, fields=("xyza", "class", "status", "steps"), transport=transport)
    assert [got["report"].rows[s] for s in range(3)] == [16, 16, 8]
    assert _same(got["xyza"], ref.xyza) and _same(got["class"], ref.ray_class)
    assert _same(got["status"], ref.status) and _same(got["steps"], ref.steps)


def _frame_adaptive(grt, width=72, height=64, spa=4):
    hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt, width=width, height=height))
    ad = hs.adaptive
    ad.enabled = 1
    ad.samples_per_axis = spa
    return hs, ad


_adaptive_ref = {}


def _adaptive_reference(grt, gpu):
    """The 72 x 64 adaptive frame on one device, rendered once for the tests that need it."""
    if "ref" not in _adaptive_ref:
        hs, ad = _frame_adaptive(grt)
        sc = grt.Scene(hs.desc_ptr(), keepalive=hs, adaptive=ad)
        _adaptive_ref["ref"] = sc.render_section_ex(adaptive=ad, device=gpu, log_events=True)
    return _adaptive_ref["ref"]


@pytest.mark.gpu
@both
@pytest.mark.parametrize("n,band", [(2, 8), (3, 16), (8, 8)])
def test_peer_adaptive_equals_render_section(grt, gpu, transport, n, band):
    ref = _adaptive_reference(grt, gpu)
    hs, ad = _frame_adaptive(grt)
    sc = grt.Scene(hs.desc_ptr(), keepalive=hs, adaptive=ad)
    got = sc.render_frame_multi([gpu] * n, band, adaptive=ad, supersample=True,
                                fields=("xyza64", "class", "status", "stop", "steps"), transport=transport)
    assert got["n_supersampled"] == ref.n_supersampled > 0
    assert _same(got["xyza64"], ref.xyza64) and _same(got["class"], ref.ray_class)
    assert _same(got["status"], ref.status) and _same(got["stop"], ref.stop) and _same(got["steps"], ref.steps)
    rep = got["report"]
    assert rep.allgather_ms > 0 and rep.transport == TRANSPORTS[transport] and rep.n_devices == n


@pytest.mark.gpu
@both
def test_peer_sampling_mask_equals_render_section(grt, gpu, transport):
    hs, ad = _frame_adaptive(grt, spa=2)
    sc = grt.Scene(hs.desc_ptr(), keepalive=hs, adaptive=ad)
    mask = grt.srgb_to_xyza(255, 0, 255)
    want, want_cls, want_sel, _ = sc.render_section(adaptive=ad, sampling_mask_xyza=mask, device=gpu)
    got = sc.render_frame_multi([gpu] * 3, 8, adaptive=ad, sampling_mask_xyza=list(mask), fields=("xyza64", "class"),
                                transport=transport)
    assert got["n_supersampled"] == want_sel > 0
    assert _same(got["xyza64"], want) and _same(got["class"], want_cls)


def _failing_scene(grt):
    """The scene of test_supersample_chunks_are_bit_identical (tests/test_gpu_frames.py):
    48 x 48, more than 21 selected pixels and more than 10 failed sub-samples."""
    import math

    b = grt.SceneBuilder(1, radius=2.0, horizon_epsilon=1e-4)
    b.integration(20000, 100.0, 0.01, 1e-7)
    pos = grt.cartesian_to_spherical((0.0, -16.0, 0.0, 3.5))
    vel = grt.stationary_velocity(1, 2.0, 0.0, pos)
    b.camera(pos, vel, math.pi / 4, 48, 48, 0.0, -3.142, 0.0)
    b.celestial(grt.Checker(0.0, 20.0, 20.0, (0, 255, 0), (0, 100, 0)))
    b.add_disc(3.0, 12.0, grt.BlackBody(1.0), temperature=5000.0)  # BelowRISCO sub-rays
    d = b.build()
    sc = grt.Scene(C.pointer(d), keepalive=(d, b))
    ad = grt.scene.default_adaptive()
    ad.enabled, ad.samples_per_axis = 1, 4
    return sc, ad


@pytest.mark.gpu
@both
def test_peer_failure_merge_across_ranks(grt, gpu, transport):
    sc, ad = _failing_scene(grt)
    ref = sc.render_section_ex(adaptive=ad, device=gpu, failure_capacity=1 << 16, log_events=True)
    assert ref.n_supersampled > 21 and len(ref.failed_subsamples) > 10
    fields = ("xyza64", "class", "status", "stop", "steps")
    got = sc.render_frame_multi([gpu] * 3, 8, adaptive=ad, supersample=True, fields=fields, fail_capacity=1 << 16,
                                transport=transport)
    assert got["n_supersampled"] == ref.n_supersampled and _same(got["xyza64"], ref.xyza64)
    f = got["failures"]
    assert f["count"] == ref.n_failed_subsamples + len(ref.subsample_events)
    err = f["status"] != 0
    assert np.array_equal(np.stack([f["pixel"][err], f["sample"][err], f["status"][err].astype(np.uint32)], axis=1),
                          ref.failed_subsamples)
    assert np.array_equal(np.stack([f["pixel"][~err], f["sample"][~err], f["stop"][~err].astype(np.uint32),
                                    f["steps"][~err]], axis=1), ref.subsample_events)
    keys = f["pixel"].astype(np.uint64) * 16 + f["sample"]
    assert np.all(keys[1:] > keys[:-1])  # sorted by (pixel, sample), across the ranks
    # the failures come from more than one rank's bands
    assert len({(int(p) // 48 // 8) % 3 for p in f["pixel"]}) > 1
    # a short list: the count is the frame's, the entries are the first of the sorted list
    few = sc.render_frame_multi([gpu] * 3, 8, adaptive=ad, supersample=True, fields=fields, fail_capacity=5,
                                transport=transport)["failures"]
    assert few["count"] == f["count"] > 5
    for k in ("pixel", "sample", "status", "stop", "steps"):
        assert len(few[k]) == 5 and np.array_equal(few[k], f[k][:5]), k


@pytest.mark.gpu
@both
def test_peer_hit_pool_retry_across_ranks(grt, gpu, transport):
    """A hit pool too small for the ranks' traces (they share the GPU's pool): the frame is
    traced again after the pool grew, and equals the roomy-pool frame."""
    from test_gpu_parity import _desc_ptr
    from test_hit_pool import N, winding_scene

    L = grt._lib
    d = winding_scene(grt)
    roomy = grt.Scene(_desc_ptr(d), keepalive=d).render_pixels(0, 0, N, N, device=gpu)
    L.check(L.lib().grt_set_hit_pool_min(64))
    try:
        sc = grt.Scene(_desc_ptr(d), keepalive=d)  # a fresh device copy: a 64-record pool
        got = sc.render_frame_multi([gpu] * 3, 8, fields=("xyza", "status", "steps"), transport=transport)
    finally:
        L.check(L.lib().grt_set_hit_pool_min(1 << 20))
    print("attempts", got["report"].attempts, "hit_overflows", got["stats"]["hit_overflows"])
    assert got["report"].attempts >= 2 and got["stats"]["hit_overflows"] == 0
    assert _same(got["xyza"], roomy.xyza) and _same(got["status"], roomy.status) and _same(got["steps"], roomy.steps)


def _child(code, *args, timeout=120):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT), str(ROOT / "tests")]))
    r = subprocess.run([sys.executable, "-c", code, *map(str, args)], capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


INJECT_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
import gr_raytracer_amd as grt
from gr_raytracer_amd import _lib as L
from conftest import c2_opts, host_scene

gpu = int(sys.argv[1])
same = lambda a, b: bool(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))
hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt, width=72, height=64))
ad = hs.adaptive
ad.enabled, ad.samples_per_axis = 1, 4
sc = grt.Scene(hs.desc_ptr(), keepalive=hs, adaptive=ad)
ref = sc.render_section_ex(adaptive=ad, device=gpu, log_events=True)
lib = L.lib()
hook = lib.grt_debug_multi_fail
hook.restype, hook.argtypes = C.c_int, [C.c_int, C.c_int]
fields = ("xyza64", "class", "status", "stop", "steps")
frame = lambda: sc.render_frame_multi([gpu] * 3, 8, adaptive=ad, supersample=True, fields=fields, transport="peer")
out = []
for rank, stage in ((1, 1), (2, 2), (0, 3)):
    assert hook(rank, stage) == 0
    rec = {"rank": rank, "stage": stage, "raised": False}
    try:
        frame()
    except L.GrtError as e:
        rec.update(raised=True, text=str(e), last=lib.grt_last_error().decode())
    g = frame()  # the hook fired once; the same device list again
    rec["next_same"] = all([same(g["xyza64"], ref.xyza64), same(g["class"], ref.ray_class),
                            same(g["status"], ref.status), same(g["stop"], ref.stop), same(g["steps"], ref.steps),
                            g["n_supersampled"] == ref.n_supersampled > 0])
    rec["knob"] = lib.grt_get_multi_transport()
    out.append(rec)
assert hook(0, 1) == 0
r = sc.render_frame_multi([gpu], 8, adaptive=ad, supersample=True, fields=fields)  # RCCL: the hook does not fire
out.append({"rccl_same": same(r["xyza64"], ref.xyza64), "disarm": hook(-1, 0), "bad": hook(0, 4)})
print(json.dumps(out))
"""


@pytest.mark.gpu
def test_peer_injected_failure_ends_the_frame_on_every_rank(grt, gpu):
    """A rank that fails (grt_debug_multi_fail) before its trace, after the allgather, or
    after the last barrier: the call returns -EIO naming the rank, every thread has come
    back (the child does not run into its time limit), and the next frame on the same
    device list equals the single-device frame."""
    res = _child(INJECT_CHILD, gpu)
    for rec in res[:3]:
        assert rec["raised"], rec
        assert "(-5)" in rec["text"] and f"rank {rec['rank']} (device {gpu})" in rec["last"], rec
        assert "injected failure" in rec["last"], rec
        assert rec["next_same"] and rec["knob"] == 0, rec
    assert res[3] == {"rccl_same": True, "disarm": 0, "bad": -22}


NO_RCCL_CHILD = r"""
import json, sys
# a host without torch: torch's ROCm build maps a librccl of its own when it is imported
# (gr_raytracer_amd loads it first when it is installed), which says nothing about libgrt.so
sys.modules["torch"] = None
import numpy as np
import gr_raytracer_amd as grt
from conftest import c2_opts, host_scene

gpu = int(sys.argv[1])
hs = host_scene(grt, "schwarzschild.toml", c2_opts(grt, width=64, height=64))
sc = grt.Scene(hs.desc_ptr(), keepalive=hs)
ref = sc.render_pixels(device=gpu)
got = sc.render_frame_multi([gpu], 16, transport="peer")
same = lambda a, b: bool(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))
maps = open("/proc/self/maps").read().splitlines()
assert sys.modules["torch"] is None
print(json.dumps({"same": same(got["xyza"], ref.xyza) and same(got["class"], ref.ray_class)
                          and same(got["status"], ref.status),
                  "transport": got["report"].transport, "n": got["report"].n_devices,
                  "rccl": [ln for ln in maps if "librccl" in ln], "grt": any("libgrt" in ln for ln in maps)}))
"""


@pytest.mark.gpu
def test_peer_one_rank_loads_no_rccl(grt, gpu):
    res = _child(NO_RCCL_CHILD, gpu)
    assert res["same"] and res["transport"] == 1 and res["n"] == 1
    assert res["grt"] and res["rccl"] == []


@pytest.mark.gpu
def test_cli_virtual_ranks_write_the_single_gpu_png(grt, gpu, tmp_path):
    flags = ["--width=80", "--height=72", "--camera-position=-16.0,0.0,3.5", "--theta=-3.142", "--max-steps=100000",
             "--tone-mapping=reinhard", "--config-file", str(SCENES / "schwarzschild.toml"),
             "--resource-root", str(RESOURCES)]
    one, multi = tmp_path / "one.png", tmp_path / "multi.png"
    r1 = subprocess.run([str(EXE), *flags, "render", "--filename", str(one)], capture_output=True, text=True,
                        timeout=120)
    r2 = subprocess.run([str(EXE), "--devices", "0,0,0", "--transport", "peer", "--band-rows", "8", *flags, "render",
                         "--filename", str(multi)], capture_output=True, text=True, timeout=120)
    assert r1.returncode == 0, r1.stderr
    assert r2.returncode == 0, r2.stderr
    assert hashlib.sha256(one.read_bytes()).hexdigest() == hashlib.sha256(multi.read_bytes()).hexdigest()
    assert "Supersampling" in r2.stderr  # the stock TOML supersamples adaptively
    assert "3 GPU(s)" in r2.stderr and "transport peer," in r2.stderr
    phases = [ln for ln in r2.stderr.splitlines() if "phases (ms)" in ln]
    assert len(phases) == 1 and phases[0].endswith("transport peer")
