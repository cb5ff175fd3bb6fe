"""bench.py's C2 line on the GPU (marker `gpu`): two frames in flight, each frame's gather
on its slot's stream through an RCCL group of one (--self-gather), every frame traced in
full.  The C2 frame's accepted-step count is fixed by the integration (bit-exact against
the oracle on crops, md5 fc034258a049 since round 3), so the line's per-frame count must be
exactly it: a frame cut short or counted twice by the slot bookkeeping would change it."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

C2_ACCEPTED_PER_FRAME = 33934152115  # profiles/r05i/c2_ab.jsonl (every round-5 C2 frame)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("inflight,extra", [(2, ["--self-gather"]), (1, [])])
def test_bench_c2_line(gpu, inflight, extra, tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    cmd = [sys.executable, str(ROOT / "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
           "--inflight", str(inflight), "--dump-outputs", str(tmp_path)] + extra
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = line["config"]
    assert cfg["frames_in_flight"] == inflight
    assert cfg["accepted_steps_per_frame"] == C2_ACCEPTED_PER_FRAME
    assert line["steps"] == 2 and line["n_gpus"] == 1
    r = line["roofline"]
    assert r["kernel_ms"] > 0 and 0 < r["frac"] < 1
    # the per-frame device time and the wall time per frame describe the same run
    assert abs(r["kernel_ms"] - line["ms_per_step"]) < 0.05 * line["ms_per_step"]
    assert line["value"] == pytest.approx(C2_ACCEPTED_PER_FRAME / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # a plain run (no --full) measures nothing beside its timed steps
    assert "fused" not in line and "render_wall" not in line and line["cpu_baseline"] is None
    assert "single_launch_ms" not in r
    # --dump-outputs: the last timed frame as float32 files, at most 64 MB in all (with the
    # gathered copy the whole is larger, so a fixed sample of the rows is written)
    n = 1500 * 1500
    files = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(files) == {"xyza", "ray_class", "status"} | ({"gathered_xyza_rank0"} if extra else set())
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64e6
    rows = len(files["xyza"])
    assert files["xyza"].shape == (rows, 4) and files["ray_class"].shape == files["status"].shape == (rows,)
    assert rows == n if not extra else n // 2 < rows < n
    assert line["dumped_outputs"]["xyza"] == [rows, n]
    assert np.nanmax(files["xyza"][:, :3]) > 0.0  # a rendered frame, not an untouched buffer
    if extra:  # rank 0's own frame came back through the gather
        assert np.array_equal(files["gathered_xyza_rank0"], files["xyza"])
