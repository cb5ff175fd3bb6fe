"""Time the geometry buffers of a camera sequence both ways on one MI355X and write
profiles/gbuffer/sequence_timing.json.

For C2's scene (schwarzschild.toml) and C3's scene (kerr-bl.toml) at 256 x 256 and
512 x 512, with K = 8 cameras on a circle around the z axis through the stock camera
position (tools/sequence_timing.py's cameras), 1 spp, two comparisons, each against the
existing per-frame path in the same run:

  (a) the trace.  Per frame: per camera grt_host_scene_load + grt_scene_create +
      grt_gbuffer_trace -- the wall time of all eight, scene creation included, and the sum
      of their event times (trace; scan + fill).  Stacked: one load, one scene and one
      grt_gbuffer_trace_sequence -- its wall time, load and create included, and the
      report's trace_ms and fill_ms (fill_ms: scan, fill and the split into frames).
  (b) the shade of those eight buffers under the scene.  Per frame: eight grt_gbuffer_shade
      calls -- the sum of their kernel_ms and the wall time of the eight calls.  Stacked:
      one grt_gbuffer_shade_sequence asking for the same four fields -- its kernel_ms and
      the call's wall time.

One untimed pass of everything warms the code objects and the allocator up; then the two
ways alternate, three repeats each.  The stacked buffers must equal the per-frame ones byte
for byte and the stacked shade the per-frame shades bit for bit (exit status 1 otherwise).
All raw times are kept, with each median's run-to-run spread (max - min) beside it.  No ratio
is required: the file records what came out.

    python tools/gbuffer_sequence_timing.py [--out profiles/gbuffer/sequence_timing.json] [--repeats 3]
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
C2 = ("schwarzschild.toml", ((-16.0, 0.0, 3.5), 0.0, -3.142, 0.0), 100000)
C3 = ("kerr-bl.toml", ((-10.0, 0.0, -0.5), 0.0, -3.14159, 0.0), 1000000)
CONFIGS = [("C2-256", 256) + C2, ("C2-512", 512) + C2, ("C3-256", 256) + C3, ("C3-512", 512) + C3]
FIELDS = ("xyza", "xyza64", "class", "status")  # what grt_gbuffer_shade returns


def circle(stock):
    (x, y, z), phi, theta, psi = stock
    out = []
    for k in range(K):
        a = 2.0 * math.pi * k / K
        out.append(((x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a), z), phi, theta, psi))
    return out


def same_buffers(a, b):
    if bytes(a.info) != bytes(b.info):
        return False
    x, y = a.arrays(), b.arrays()
    return all(x[k].tobytes() == y[k].tobytes() for k in x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "sequence_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import gr_raytracer_amd as g

    if g.device_count() < 1:
        raise SystemExit("gbuffer_sequence_timing: no GPU visible (there is no CPU path to time)")
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    results, ok = [], True
    for name, size, toml, stock, max_steps in CONFIGS:
        cams = circle(stock)

        def opts(row):
            return g.GlobalOpts(width=size, height=size, camera_position=row[0], phi=row[1], theta=row[2], psi=row[3],
                                max_steps=max_steps)

        def per_frame():
            t0 = time.perf_counter()
            trace, fill, bufs = 0.0, 0.0, []
            for row in cams:
                hs = g.HostScene(str(scenes / toml), opts(row), str(res))
                sc = g.Scene(hs.desc_ptr(), keepalive=hs)
                gb = sc.trace_gbuffer()  # returns after the device has finished
                tt = gb.trace_times
                trace += tt["trace_ms"]
                fill += tt["fill_ms"]
                bufs.append(gb)
                sc.close()
                hs.close()
            wall = (time.perf_counter() - t0) * 1e3
            hs = g.HostScene(str(scenes / toml), opts(cams[0]), str(res))  # the appearance, untimed
            sc = g.Scene(hs.desc_ptr(), keepalive=hs)
            bufs[0].shade(sc)  # the scene's device copy, untimed
            t0 = time.perf_counter()
            shades = [gb.shade(sc) for gb in bufs]
            shade_wall = (time.perf_counter() - t0) * 1e3
            times = {"trace_wall_ms": wall, "trace_ms": trace, "fill_ms": fill, "shade_wall_ms": shade_wall,
                     "shade_kernel_ms": sum(s.stats["kernel_ms"] for s in shades)}
            sc.close()
            hs.close()
            return times, bufs, shades

        def stacked():
            t0 = time.perf_counter()
            hs = g.HostScene(str(scenes / toml), opts(cams[0]), str(res))
            sc = g.Scene(hs.desc_ptr(), keepalive=hs)
            seq = sc.trace_gbuffer_sequence([hs.camera(*row) for row in cams])
            wall = (time.perf_counter() - t0) * 1e3
            rep = seq.report
            g.shade_sequence(seq[:1], sc, fields=FIELDS)  # as per_frame: nothing to warm up inside the timed call
            t0 = time.perf_counter()
            shaded = g.shade_sequence(seq, sc, fields=FIELDS)
            shade_wall = (time.perf_counter() - t0) * 1e3
            times = {"trace_wall_ms": wall, "trace_ms": rep.trace_ms, "fill_ms": rep.fill_ms, "call_ms": rep.wall_ms,
                     "n_launches": rep.n_launches, "frames_per_launch": rep.frames_per_launch, "n_traces": rep.n_traces,
                     "shade_wall_ms": shade_wall, "shade_kernel_ms": shaded["stats"]["kernel_ms"]}
            sc.close()
            hs.close()
            return times, seq, shaded

        _, bufs, shades = per_frame()  # warm-up of both, and the identity checks
        _, seq, shaded = stacked()
        same_b = all(same_buffers(seq[k], bufs[k]) for k in range(K))
        same_s = all(np.array_equal(shaded["xyza"][k].view(np.uint32), shades[k].xyza.view(np.uint32)) and
                     np.array_equal(shaded["xyza64"][k].view(np.uint64), shades[k].xyza64.view(np.uint64)) and
                     np.array_equal(shaded["class"][k], shades[k].ray_class) and
                     np.array_equal(shaded["status"][k], shades[k].status) for k in range(K))
        layers = sum(int(b.info.n_layers) for b in seq)
        del bufs, shades, seq, shaded
        a_runs, b_runs = [], []
        for _ in range(args.repeats):
            a_runs.append(per_frame()[0])
            b_runs.append(stacked()[0])

        def stat(runs, key):
            v = [r[key] for r in runs]
            return {"median": float(np.median(v)), "spread": float(max(v) - min(v))}

        entry = {"config": name, "scene": toml, "width": size, "height": size, "cameras": K, "max_steps": max_steps,
                 "n_layers": layers, "buffers_identical": bool(same_b), "shades_identical": bool(same_s),
                 "per_frame": a_runs, "stacked": b_runs}
        for key in ("trace_wall_ms", "trace_ms", "fill_ms", "shade_wall_ms", "shade_kernel_ms"):
            a, b = stat(a_runs, key), stat(b_runs, key)
            entry[key] = {"per_frame": a, "stacked": b, "stacked_over_per_frame": b["median"] / a["median"]}
        entry["stacked_shade_faster"] = {
            "kernel": bool(entry["shade_kernel_ms"]["stacked"]["median"] < entry["shade_kernel_ms"]["per_frame"]["median"]),
            "call": bool(entry["shade_wall_ms"]["stacked"]["median"] < entry["shade_wall_ms"]["per_frame"]["median"])}
        ok = ok and same_b and same_s
        results.append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k not in ("per_frame", "stacked")}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"tool": "tools/gbuffer_sequence_timing.py", "library_sources": g._lib.source_stamp(),
                               "repeats": args.repeats, "results": results}, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
