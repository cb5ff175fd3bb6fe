"""The geometry buffer of the whole frame traced over several ranks (grt_gbuffer_trace_multi;
marker `gpu`).  One GPU is assumed: under the peer transports a device list may name it several
times, one rank per entry, which runs the whole N > 1 host path and the assembly kernels.

Every comparison is on bytes.  "The reference" is `sc.trace_gbuffer()` of the same scene on the
same GPU: the multi-traced buffer has its grt_gbuffer_info and all twelve arrays.  Frames are
24 cols x 20 rows (test_gpu_gbuffer.py) except where noted: in bands of 8 rows that is three
ragged bands 8 / 8 / 4.
"""
import errno
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import RESOURCES, ROOT, SCENES
from test_gpu_gbuffer import COLS, GRT, ROWS, STOCK, assert_same_frame, built_scene, reshade_pair, stock, stock_case

pytestmark = pytest.mark.gpu

TRANSPORTS = {"rccl": 0, "peer": 1, "peer-staged": 2}
both = pytest.mark.parametrize("transport", ["peer", "peer-staged"])


def assert_same_buffer(got, want, what=""):
    assert bytes(got.info) == bytes(want.info), (what, "info")
    a, b = got.arrays(), want.arrays()
    assert a.keys() == b.keys() and len(a) == 12
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def check_report(gb, n, rows, transport, ref, one_trace=True):
    rep = gb.report
    assert rep.n_devices == n and rep.transport == TRANSPORTS[transport]
    assert sum(rep.rows[k] for k in range(n)) == rows
    assert sum(rep.layers[k] for k in range(n)) == int(ref.info.n_layers)
    assert all(rep.block_bytes[k] % 256 == 0 and rep.block_bytes[k] > 0 for k in range(n))
    if one_trace:  # the pools were large enough: the counters are the single trace's
        assert all(rep.n_traces[k] == (1 if rep.rows[k] else 0) for k in range(n)), list(rep.n_traces)[:n]
        assert gb.stats["rays"] == ref.stats["rays"] and gb.stats["accepted_steps"] == ref.stats["accepted_steps"]
    assert gb.stats["hit_overflows"] == 0
    t = gb.trace_times
    assert t["trace_ms"] == max(rep.trace_ms[k] for k in range(n)) > 0
    assert t["fill_ms"] >= rep.gather_ms > 0 and rep.wall_ms > 0


def band_layers(gb, band):
    """Layers of each band of `band` rows of the reference buffer."""
    start = gb.arrays()["layer_start"].astype(np.int64)
    edges = [min(b * band, ROWS) * COLS for b in range(-(-ROWS // band) + 1)]
    return [int(start[edges[b + 1]] - start[edges[b]]) for b in range(len(edges) - 1)]


def telling_band(grt, gb, n=3):
    """The band height, 8 or else 4, at which the reference frame over n ranks has at least two
    ranks that own layers and at least one band without any: decided from the reference alone.
    The euclidean frame's 24 layers lie in rows 8..11, one band at 8 and at 4 alike, so the
    search goes on to the case list's own band of 1 row, where they are four bands of three
    ranks; a scene for which none of the three heights holds fails here."""
    from gr_raytracer_amd.distributed import shard_frame_rows

    seen = {}
    for band in (8, 4, 1):
        per_band = band_layers(gb, band)
        owners = set()
        for s in range(n):
            fr = shard_frame_rows(ROWS, band, s, n)
            if sum(per_band[int(r) // band] for r in fr[::band]) > 0:
                owners.add(s)
        seen[band] = per_band
        if len(owners) >= 2 and 0 in per_band:
            return band
    raise AssertionError(f"no band height with two owners of layers and a band without: {seen}")


# ------------------------------------------------------------------- 1. identity ----
@both
@pytest.mark.parametrize("name", ["schwarzschild", "kerr-bl", "kerr-schild", "euclidean"])
def test_identity(grt, gpu, name, transport):
    hs, sc, want, ref = stock_case(grt, name)
    band = telling_band(grt, ref)
    print(name, "telling band", band, "layers per band", band_layers(ref, band))
    cases = [(1, 8), (2, 8), (3, 8), (5, 8), (3, 1), (3, 7)] + ([(3, band)] if band == 4 else [])
    for n, b in cases:
        gb = sc.trace_gbuffer_multi([gpu] * n, b, transport=transport)
        what = f"{name}, {n} ranks, bands of {b}, {transport}"
        assert_same_buffer(gb, ref, what)
        assert_same_frame(gb.shade(sc), want, what)
        check_report(gb, n, ROWS, transport, ref)
        if (n, b) == (5, 8):
            assert [gb.report.rows[k] for k in range(5)] == [8, 8, 4, 0, 0]
            assert gb.report.layers[3] == gb.report.layers[4] == 0
        if (n, b) == (3, band):
            assert sum(gb.report.layers[k] > 0 for k in range(3)) >= 2
        gb.close()
    assert grt._lib.lib().grt_get_multi_transport() == 0  # every call restored the knob


# ----------------------------------------------------------------------- 2. RCCL ----
def _rc(exc):
    return int(str(exc.value).split("(")[1].split(")")[0])


def test_rccl_one_rank(grt, gpu):
    hs, sc, want, ref = stock_case(grt, "schwarzschild")
    assert grt._lib.lib().grt_get_multi_transport() == 0
    gb = sc.trace_gbuffer_multi([gpu], 8)
    assert_same_buffer(gb, ref, "rccl, one rank")
    check_report(gb, 1, ROWS, "rccl", ref)
    with pytest.raises(grt.GrtError, match="twice") as e:
        sc.trace_gbuffer_multi([gpu, gpu], 8)
    assert _rc(e) == -errno.EINVAL


# --------------------------------------------------------- 3. another appearance ----
def test_reshade_under_another_appearance(grt, gpu):
    da, db = reshade_pair(grt, "schwarzschild")
    sa, sb = built_scene(grt, da), built_scene(grt, db)
    want_b = sb.render_pixels(0, 0, ROWS, COLS)
    gb = sa.trace_gbuffer_multi([gpu] * 3, 8, transport="peer")
    assert_same_frame(gb.shade(sb), want_b, "A's multi trace under B")
    gb_b = sb.trace_gbuffer_multi([gpu] * 3, 8, transport="peer")
    a, b = gb.arrays(), gb_b.arrays()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (np.diff(a["layer_start"].astype(np.int64)) >= 2).sum() >= 30


# ------------------------------------------- 4. past the slots, and the hit pool ----
def test_layers_past_the_workspace_slots_and_a_small_pool(grt, gpu):
    from test_hit_pool import N, winding_scene

    L = grt._lib
    d = winding_scene(grt, disc=True)
    sc = built_scene(grt, d)
    ref = sc.trace_gbuffer()
    layers = np.diff(ref.arrays()["layer_start"].astype(np.int64))
    assert (layers > L.GRT_MAX_HITS).sum() >= 300
    gb = sc.trace_gbuffer_multi([gpu] * 3, 8, transport="peer")
    assert_same_buffer(gb, ref, "winding")
    check_report(gb, 3, N, "peer", ref, one_trace=False)
    L.check(L.lib().grt_set_hit_pool_min(64))
    try:
        small = built_scene(grt, d)  # a fresh device copy: a 64-record pool
        gb2 = small.trace_gbuffer_multi([gpu] * 3, 8, transport="peer")
    finally:
        L.check(L.lib().grt_set_hit_pool_min(1 << 20))
    assert_same_buffer(gb2, ref, "winding, small pool")
    traces = [gb2.report.n_traces[k] for k in range(3)]
    print("traces per rank", traces)
    assert max(traces) > 1 and max(traces) <= 3
    assert not np.any(gb2.arrays()["status"] & L.FLAG_HIT_OVERFLOW)
    assert gb2.stats["hit_overflows"] == 0


# ------------------------------------------------------------- 5. window errors ----
def test_window_errors(grt, gpu):
    from test_gpu_gbuffer_adaptive import below_risco_scene

    sc, _ = below_risco_scene(grt)
    ref = sc.trace_gbuffer()
    status = ref.arrays()["status"]
    assert np.isin(status, (2, 3)).sum() > 0, np.unique(status)
    gb = sc.trace_gbuffer_multi([gpu] * 3, 8, transport="peer-staged")
    assert_same_buffer(gb, ref, "below r_isco")
    assert np.array_equal(gb.arrays()["status"], status)


# ------------------------------------------------------ 6. the buffer is ordinary ----
def test_the_buffer_is_ordinary(grt, gpu, tmp_path):
    from test_gpu_gbuffer_adaptive import assert_same_section, reference, reshade

    hs, sc, want, ref = stock_case(grt, "schwarzschild")
    gb = sc.trace_gbuffer_multi([gpu] * 3, 8, transport="peer")
    gb.save(tmp_path / "multi.grtg")
    ref.save(tmp_path / "one.grtg")
    assert (tmp_path / "multi.grtg").read_bytes() == (tmp_path / "one.grtg").read_bytes()
    loaded = grt.GBuffer.load(tmp_path / "multi.grtg", device=gpu)
    assert_same_buffer(loaded, ref, "save -> load")
    assert_same_frame(loaded.shade(sc), want, "save -> load")
    loaded.close()
    # the adaptive frame: the top-up runs on the buffer's GPU through the existing calls
    ad = hs.adaptive
    assert ad.enabled
    want_s = reference(sc, ad)
    assert want_s.n_supersampled > 21
    got_s, rep = reshade(gb, sc, ad, tracer=sc)
    assert_same_section(got_s, want_s, "adaptive frame of the multi-traced buffer")
    assert rep["n_traced"] == want_s.n_supersampled and rep["n_missing"] == 0
    gb.close()


# ------------------------------------------------------------------ 7. fused knob ----
def test_multi_trace_is_exact_under_the_fused_knob(grt, gpu):
    hs, sc, want, ref = stock_case(grt, "schwarzschild")
    assert grt.get_arithmetic() == 0
    grt.set_arithmetic("fused")
    try:
        gb = sc.trace_gbuffer_multi([gpu] * 3, 8, transport="peer")
    finally:
        grt.set_arithmetic("exact")
    assert_same_buffer(gb, ref, "fused knob")


# -------------------------------------------------------------------- 8. refusals ----
def test_refusals(grt, gpu):
    _, vol = stock(grt, "schwarzschild-volumetric-stony.toml", **STOCK["schwarzschild"][1])
    with pytest.raises(grt.GrtError) as e:
        vol.trace_gbuffer_multi([gpu] * 2, 8, transport="peer")
    assert _rc(e) == -errno.ENOTSUP
    hs, sc, want, ref = stock_case(grt, "schwarzschild")
    for devices, band in (([gpu] * 2, 0), ([], 8), ([gpu] * 17, 8), ([gpu, grt.device_count()], 8)):
        with pytest.raises(grt.GrtError) as e:
            sc.trace_gbuffer_multi(devices, band, transport="peer")
        assert _rc(e) == -errno.EINVAL, (devices, band)
    assert grt._lib.lib().grt_get_multi_transport() == 0
    gb = sc.trace_gbuffer_multi([gpu] * 2, 8, transport="peer")  # the refusals left nothing behind
    assert_same_buffer(gb, ref, "after the refusals")


# ------------------------------------------------------ 9. injected host failure ----
INJECT_CHILD = r"""
import ctypes as C, json, sys
import gr_raytracer_amd as grt
from gr_raytracer_amd import _lib as L
from test_gpu_gbuffer import stock_case

gpu = int(sys.argv[1])
hs, sc, want, ref = stock_case(grt, "schwarzschild")
lib = L.lib()
hook = lib.grt_debug_multi_fail
hook.restype, hook.argtypes = C.c_int, [C.c_int, C.c_int]
trace = lambda: sc.trace_gbuffer_multi([gpu] * 3, 8, transport="peer")
def same(gb):
    a, b = gb.arrays(), ref.arrays()
    return bytes(gb.info) == bytes(ref.info) and all(a[k].tobytes() == b[k].tobytes() for k in b)
out = []
for rank, stage in ((1, 1), (0, 3)):
    assert hook(rank, stage) == 0
    rec = {"rank": rank, "stage": stage, "raised": False}
    try:
        trace()
    except L.GrtError as e:
        rec.update(raised=True, text=str(e), last=lib.grt_last_error().decode())
    rec["next_same"] = same(trace())  # the hook fired once; the same device list again
    rec["knob"] = lib.grt_get_multi_transport()
    out.append(rec)
out.append({"disarm": hook(-1, 0)})
print(json.dumps(out))
"""


def test_injected_failure_ends_the_call_on_every_rank(grt, gpu):
    """A rank that fails in host code (grt_debug_multi_fail) before its trace, or devices[0]
    after the barrier: -EIO naming the rank, every thread has come back (the child returns well
    inside its time limit), and the next call on the same list equals the reference."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT), str(ROOT / "tests")]))
    r = subprocess.run([sys.executable, "-c", INJECT_CHILD, str(gpu)], capture_output=True, text=True, timeout=120,
                       env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for rec in res[:2]:
        assert rec["raised"], rec
        assert "(-5)" in rec["text"] and f"rank {rec['rank']} (device {gpu})" in rec["last"], rec
        assert "injected failure" in rec["last"], rec
        assert rec["next_same"] and rec["knob"] == 0, rec
    assert res[2] == {"disarm": 0}


# ------------------------------------------------------------------------ 10. CLI ----
def _grt(*args):
    r = subprocess.run([str(GRT), *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_cli_gbuffer_over_virtual_ranks(grt, gpu, tmp_path):
    toml = tmp_path / "a.toml"
    toml.write_text((SCENES / "schwarzschild.toml").read_text() + "\n[adaptive_sampling]\nenabled = false\n")
    common = ["--width", 64, "--height", 48, "--camera-position", "-16,0,3.5", "--theta", "-3.142", "--max-steps", 100000,
              "--resource-root", RESOURCES, "--config-file", toml]
    _grt(*common, "gbuffer", "--filename", tmp_path / "one.grtg")
    r = _grt("--devices", "0,0,0", "--transport", "peer", "--band-rows", 8, *common, "gbuffer", "--filename",
             tmp_path / "multi.grtg")
    assert (tmp_path / "multi.grtg").read_bytes() == (tmp_path / "one.grtg").read_bytes()
    ranks = [ln for ln in r.stderr.splitlines() if ln.startswith("[grt] rank ")]
    assert len(ranks) == 3 and all("rows" in ln and "layers" in ln and "trace(s)" in ln and "ms" in ln for ln in ranks)
    assert "3 GPU(s); transport peer," in r.stderr
    _grt("--width", 64, "--height", 48, "--resource-root", RESOURCES, "--config-file", toml, "reshade", "--gbuffer",
         tmp_path / "multi.grtg", "--filename", tmp_path / "reshade.png")
    _grt(*common, "render", "--filename", tmp_path / "render.png")
    assert (tmp_path / "reshade.png").read_bytes() == (tmp_path / "render.png").read_bytes()
