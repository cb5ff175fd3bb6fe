"""Time the supersampled geometry buffer on one MI355X and write
profiles/gbuffer/adaptive_timing.json.

For C2's scene (schwarzschild.toml) and C3's scene (kerr-bl.toml) at 1500 x 1500 with their
stock adaptive configuration, in one process, after one untimed pass of everything (code
objects, allocator, the scene's device copy), three repetitions that alternate between the
two scenes; each repetition takes

  * grt_render_section_ex: stats.kernel_ms (device events) and the call's wall time -- the
    adaptive frame as `render` traces it, the yardstick;
  * the cold fill: the wall time of grt_gbuffer_trace followed by the first
    grt_gbuffer_shade_section with the scene as its own tracer (the top-up of the whole
    selection), with the trace's and the top-up's event times;
  * the warm grt_gbuffer_shade_section of that buffer (nothing to trace): shade_ms (device
    events) and the call's wall time;
  * the size of the sub-sample set: pixels, sub-rays, layers and bytes (as its file holds it).

The re-shaded frames must equal render_section_ex's bit for bit.  All raw times are kept.
The one requirement (exit status 1 when missed): the warm shade_section's wall time is
below render_section_ex's kernel time in every repetition.

    python tools/gbuffer_adaptive_timing.py [--out profiles/gbuffer/adaptive_timing.json] [--repeats 3] [--size 1500]
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


def same_section(a, b):
    return bool(np.array_equal(a.xyza64.view(np.uint64), b.xyza64.view(np.uint64))
                and np.array_equal(a.ray_class, b.ray_class) and np.array_equal(a.status, b.status)
                and a.n_supersampled == b.n_supersampled and a.n_failed_subsamples == b.n_failed_subsamples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "adaptive_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=1500)
    args = ap.parse_args()
    import gr_raytracer_amd as g

    if g.device_count() < 1:
        raise SystemExit("gbuffer_adaptive_timing: no GPU visible (there is no CPU path to time)")
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    size = args.size
    loaded = {}
    for name, toml, opts in CONFIGS:
        hs = g.HostScene(str(scenes / toml), g.GlobalOpts(width=size, height=size, **opts), str(res))
        loaded[name] = (hs, g.Scene(hs.desc_ptr(), keepalive=hs, adaptive=hs.adaptive))

    def one(name):
        hs, sc = loaded[name]
        ad = hs.adaptive
        t0 = time.perf_counter()
        r = sc.render_section_ex(adaptive=ad, failure_capacity=1)
        t1 = time.perf_counter()
        gb = sc.trace_gbuffer()
        cold, cold_rep = gb.shade_section(sc, adaptive=ad, tracer=sc)
        t2 = time.perf_counter()
        warm, warm_rep = gb.shade_section(sc, adaptive=ad)
        t3 = time.perf_counter()
        sub, tt = gb.sub_info, gb.trace_times
        m, n, nl = int(sub.n_sub_pixels), int(sub.n_sub_rays), int(sub.n_sub_layers)
        out = {"render_section_kernel_ms": r.stats["kernel_ms"], "render_section_wall_ms": (t1 - t0) * 1e3,
               "cold_fill_wall_ms": (t2 - t1) * 1e3, "gbuffer_trace_ms": tt["trace_ms"],
               "gbuffer_scan_fill_ms": tt["fill_ms"], "top_up_trace_ms": cold_rep["trace_ms"],
               "top_up_rays": cold_rep["top_up"]["rays"], "cold_shade_ms": cold_rep["shade_ms"],
               "warm_shade_ms": warm_rep["shade_ms"], "warm_shade_wall_ms": (t3 - t2) * 1e3,
               "warm_traced": warm_rep["n_traced"], "n_selected": warm_rep["n_selected"],
               "samples_per_axis": int(sub.samples_per_axis), "n_sub_pixels": m, "n_sub_rays": n, "n_sub_layers": nl,
               "sub_set_bytes": 4 * m + 8 * (n + 1) + 24 * n + 4 * n + 2 * n + 33 * nl,
               "identical": same_section(cold, r) and same_section(warm, r)}
        gb.close()
        return out

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
        entry = {
            "config": name, "scene": toml, "width": size, "height": size, "max_steps": opts["max_steps"], "runs": rr,
            "identical": all(x["identical"] for x in rr),
            "render_section_kernel_ms_median": med([x["render_section_kernel_ms"] for x in rr]),
            "cold_fill_wall_ms_median": med([x["cold_fill_wall_ms"] for x in rr]),
            "warm_shade_ms_median": med([x["warm_shade_ms"] for x in rr]),
            "warm_shade_wall_ms_median": med([x["warm_shade_wall_ms"] for x in rr]),
            "n_selected": rr[0]["n_selected"], "n_sub_rays": rr[0]["n_sub_rays"], "sub_set_bytes": rr[0]["sub_set_bytes"],
        }
        entry["warm_wall_over_render_kernel"] = entry["warm_shade_wall_ms_median"] / entry["render_section_kernel_ms_median"]
        entry["cold_fill_over_render_kernel"] = entry["cold_fill_wall_ms_median"] / entry["render_section_kernel_ms_median"]
        entry["warm_faster_than_render"] = all(x["warm_shade_wall_ms"] < x["render_section_kernel_ms"] for x in rr)
        entry["warm_traces_nothing"] = all(x["warm_traced"] == 0 for x in rr)
        ok = ok and entry["identical"] and entry["warm_faster_than_render"] and entry["warm_traces_nothing"]
        results.append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k != "runs"}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"tool": "tools/gbuffer_adaptive_timing.py", "library_sources": g._lib.source_stamp(),
                               "repeats": args.repeats, "results": results}, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
