"""Time the geometry buffer on one MI355X and write profiles/gbuffer/timing.json.

For C2's scene (schwarzschild.toml) and C3's scene (kerr-bl.toml) at 1500 x 1500, 1 spp,
in one process, after one untimed pass of everything (code objects, allocator, the scene's
device copy), three repetitions that alternate between the two scenes; each repetition takes

  * grt_render_pixels: stats.kernel_ms (device events) and the call's wall time;
  * grt_gbuffer_trace: its wall time and its two event times -- the trace, and the layer
    scan plus the fill;
  * grt_gbuffer_shade of that buffer under the traced scene: kernel_ms and wall time;
  * the buffer's size in bytes (its arrays, as the file holds them).

The re-shaded frame must equal render_pixels' bit for bit.  All raw times are kept.
Recorded per scene: the shade's cost relative to a trace, and the scan + fill's cost
against the run-to-run spread (max - min) of render_pixels' own kernel time in this file.
The one requirement (exit status 1 when missed): on C2 the shade's wall time is below
render_pixels' kernel time in every repetition.

    python tools/gbuffer_timing.py [--out profiles/gbuffer/timing.json] [--repeats 3] [--size 1500]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CONFIGS = [
    ("C2", "schwarzschild.toml", dict(camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=100000)),
    ("C3", "kerr-bl.toml", dict(camera_position=(-10.0, 0.0, -0.5), theta=-3.14159, max_steps=1000000)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=1500)
    args = ap.parse_args()
    import gr_raytracer_amd as g

    if g.device_count() < 1:
        raise SystemExit("gbuffer_timing: no GPU visible (there is no CPU path to time)")
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    size = args.size
    loaded = {}
    for name, toml, opts in CONFIGS:
        hs = g.HostScene(str(scenes / toml), g.GlobalOpts(width=size, height=size, **opts), str(res))
        loaded[name] = (hs, g.Scene(hs.desc_ptr(), keepalive=hs))

    def one(name):
        sc = loaded[name][1]
        t0 = time.perf_counter()
        r = sc.render_pixels(0, 0, size, size, aux=False)
        t1 = time.perf_counter()
        gb = sc.trace_gbuffer()
        t2 = time.perf_counter()
        s = gb.shade(sc)
        t3 = time.perf_counter()
        info, tt = gb.info, gb.trace_times
        n, nl = int(info.n_pixels), int(info.n_layers)
        same = (np.array_equal(s.xyza.view(np.uint32), r.xyza.view(np.uint32)) and np.array_equal(s.ray_class, r.ray_class)
                and np.array_equal(s.status, r.status))
        gb.close()
        return {"render_pixels_kernel_ms": r.stats["kernel_ms"], "render_pixels_wall_ms": (t1 - t0) * 1e3,
                "gbuffer_trace_wall_ms": (t2 - t1) * 1e3, "gbuffer_trace_ms": tt["trace_ms"],
                "gbuffer_scan_fill_ms": tt["fill_ms"], "shade_kernel_ms": s.stats["kernel_ms"],
                "shade_wall_ms": (t3 - t2) * 1e3, "n_pixels": n, "n_layers": nl,
                "buffer_bytes": 8 * (n + 1) + 24 * n + 4 * n + 2 * n + 33 * nl, "identical": bool(same)}

    for name, _, _ in CONFIGS:  # warm-up
        one(name)
    runs = {name: [] for name, _, _ in CONFIGS}
    for _ in range(args.repeats):
        for name, _, _ in CONFIGS:
            runs[name].append(one(name))
    med = lambda v: float(np.median(v))  # noqa: E731
    results, ok = [], True
    for name, toml, opts in CONFIGS:
        rr = runs[name]
        rk = [x["render_pixels_kernel_ms"] for x in rr]
        spread = max(rk) - min(rk)
        entry = {
            "config": name, "scene": toml, "width": size, "height": size, "max_steps": opts["max_steps"], "runs": rr,
            "identical": all(x["identical"] for x in rr),
            "render_pixels_kernel_ms_median": med(rk), "render_pixels_kernel_ms_spread": spread,
            "gbuffer_trace_ms_median": med([x["gbuffer_trace_ms"] for x in rr]),
            "gbuffer_scan_fill_ms_median": med([x["gbuffer_scan_fill_ms"] for x in rr]),
            "shade_kernel_ms_median": med([x["shade_kernel_ms"] for x in rr]),
            "shade_wall_ms_median": med([x["shade_wall_ms"] for x in rr]),
            "buffer_bytes": rr[0]["buffer_bytes"], "n_layers": rr[0]["n_layers"],
        }
        entry["shade_kernel_over_render_kernel"] = entry["shade_kernel_ms_median"] / entry["render_pixels_kernel_ms_median"]
        entry["shade_wall_over_render_kernel"] = entry["shade_wall_ms_median"] / entry["render_pixels_kernel_ms_median"]
        entry["scan_fill_over_render_spread"] = (entry["gbuffer_scan_fill_ms_median"] / spread) if spread > 0 else None
        entry["shade_faster_than_render"] = all(x["shade_wall_ms"] < x["render_pixels_kernel_ms"] for x in rr)
        ok = ok and entry["identical"] and (name != "C2" or entry["shade_faster_than_render"])
        results.append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k != "runs"}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"tool": "tools/gbuffer_timing.py", "library_sources": g._lib.source_stamp(),
                               "repeats": args.repeats, "results": results}, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
