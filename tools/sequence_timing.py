"""Time a camera sequence both ways on one MI355X and write profiles/sequence/timing.json.

For C3's scene (kerr-bl.toml) at 256 x 256 and 512 x 512 and C2's scene
(schwarzschild.toml) at 256 x 256, with K = 8 cameras on a circle around the z axis
through the stock camera position (the tetrad turns with the chart, so every camera looks
at the hole as the stock one does), 1 spp:

  (a) frame by frame, as before grt_render_sequence: per camera grt_host_scene_load +
      grt_scene_create + grt_render_pixels -- the wall time of all eight, and the
      kernel-only sum of their stats.kernel_ms (device events);
  (b) one grt_render_sequence over one loaded scene: its wall time (load, create and
      cameras included) and report.trace_ms (device events of the stacked trace).

One untimed pass of each warms the code objects and the allocator up; then (a) and (b)
alternate, three repeats each.  Frames of (b) must equal (a)'s bit for bit.  All raw times
are kept.  The requirement it checks (exit status 1 when missed): (b)'s trace_ms is not
above (a)'s kernel-only sum by more than the run-to-run spread (max - min) of (a) itself.

    python tools/sequence_timing.py [--out profiles/sequence/timing.json] [--repeats 3]
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

K = 8
CONFIGS = [
    # name, TOML, width = height, stock camera (position, phi, theta, psi), max_steps
    ("C3-256", "kerr-bl.toml", 256, ((-10.0, 0.0, -0.5), 0.0, -3.14159, 0.0), 1000000),
    ("C3-512", "kerr-bl.toml", 512, ((-10.0, 0.0, -0.5), 0.0, -3.14159, 0.0), 1000000),
    ("C2-256", "schwarzschild.toml", 256, ((-16.0, 0.0, 3.5), 0.0, -3.142, 0.0), 100000),
]


def circle(stock):
    (x, y, z), phi, theta, psi = stock
    out = []
    for k in range(K):
        a = 2.0 * math.pi * k / K
        out.append(((x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a), z), phi, theta, psi))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sequence" / "timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import gr_raytracer_amd as g

    if g.device_count() < 1:
        raise SystemExit("sequence_timing: no GPU visible (there is no CPU path to time)")
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    results, ok = [], True
    for name, toml, size, stock, max_steps in CONFIGS:
        cams = circle(stock)

        def opts(row):
            return g.GlobalOpts(width=size, height=size, camera_position=row[0], phi=row[1], theta=row[2], psi=row[3],
                                max_steps=max_steps)

        def frame_by_frame():
            t0 = time.perf_counter()
            kernel, frames = 0.0, []
            for row in cams:
                hs = g.HostScene(str(scenes / toml), opts(row), str(res))
                sc = g.Scene(hs.desc_ptr(), keepalive=hs)
                r = sc.render_pixels(0, 0, size, size, aux=False)  # returns after the device has finished
                kernel += r.stats["kernel_ms"]
                frames.append((r.xyza, r.ray_class, r.status))
                sc.close()
                hs.close()
            return {"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": kernel}, frames

        def sequence():
            t0 = time.perf_counter()
            hs = g.HostScene(str(scenes / toml), opts(cams[0]), str(res))
            sc = g.Scene(hs.desc_ptr(), keepalive=hs)
            seq = sc.render_sequence([hs.camera(*row) for row in cams], fields=("xyza", "class", "status"))
            wall = (time.perf_counter() - t0) * 1e3
            rep = seq["report"]
            sc.close()
            hs.close()
            return {"wall_ms": wall, "trace_ms": rep.trace_ms, "call_ms": rep.wall_ms, "n_launches": rep.n_launches,
                    "frames_per_launch": rep.frames_per_launch}, seq

        _, frames = frame_by_frame()  # warm-up of both, and the identity check
        _, seq = sequence()
        same = all(np.array_equal(seq["xyza"][k].view(np.uint32), frames[k][0].view(np.uint32)) and
                   np.array_equal(seq["class"][k], frames[k][1]) and np.array_equal(seq["status"][k], frames[k][2])
                   for k in range(K))
        a_runs, b_runs = [], []
        for _ in range(args.repeats):
            a_runs.append(frame_by_frame()[0])
            b_runs.append(sequence()[0])
        a_k = [r["kernel_ms"] for r in a_runs]
        b_t = [r["trace_ms"] for r in b_runs]
        spread = max(a_k) - min(a_k)
        med = lambda v: float(np.median(v))  # noqa: E731
        entry = {
            "config": name, "scene": toml, "width": size, "height": size, "cameras": K, "max_steps": max_steps,
            "frames_identical": bool(same), "frame_by_frame": a_runs, "sequence": b_runs,
            "kernel_sum_ms_median": med(a_k), "kernel_sum_ms_spread": spread, "trace_ms_median": med(b_t),
            "trace_over_kernel_sum": med(b_t) / med(a_k),
            "wall_over_wall": med([r["wall_ms"] for r in b_runs]) / med([r["wall_ms"] for r in a_runs]),
            # the requirement, on the medians: trace_ms <= kernel sum + (a)'s own spread
            "within_requirement": bool(med(b_t) <= med(a_k) + spread),
        }
        ok = ok and entry["within_requirement"] and same
        results.append(entry)
        print(json.dumps({k: entry[k] for k in ("config", "frames_identical", "kernel_sum_ms_median",
                                                "kernel_sum_ms_spread", "trace_ms_median", "trace_over_kernel_sum",
                                                "wall_over_wall", "within_requirement")}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"tool": "tools/sequence_timing.py", "library_sources": g._lib.source_stamp(),
                               "repeats": args.repeats, "results": results}, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
