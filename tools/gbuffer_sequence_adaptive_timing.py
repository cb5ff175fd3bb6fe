"""Time the adaptive frames of a g-buffer sequence both ways on one MI355X and write
profiles/gbuffer/sequence_adaptive_timing.json.

For C2's scene (schwarzschild.toml) and C3's scene (kerr-bl.toml) at 256 x 256 and
512 x 512, with K = 8 cameras on a circle around the z axis through the stock camera
position (tools/sequence_timing.py's cameras) and the scenes' stock adaptive configuration,
two legs in the same process:

  per frame   eight tracer scenes (one per camera), eight grt_gbuffer_trace calls, then
              eight cold grt_gbuffer_shade_section calls (each traces its frame's selection
              as its top-up) and eight warm ones (the sets hold the selections);
  stacked     one scene, grt_gbuffer_trace_sequence, one cold
              grt_gbuffer_shade_section_sequence (one stacked top-up of all the selections)
              and one warm one.

One untimed pass of each leg warms the code objects and the allocator up and gives the
frames that are compared (bit for bit; exit status 1 otherwise); then the legs alternate,
three repeats each.  Event times: the top-up's traces (grt_stats.kernel_ms of the top-up),
the top-up with its scan, fill and cut (trace_ms of the reports) and the shade (shade_ms).
Wall times: a host clock around each synchronising call.  All raw times are kept, with each
median's run-to-run spread (max - min) beside it.  No ratio is fixed in advance; the two
requirements are against the per-frame leg of the same run, with its own spread as margin:

  top_up_trace   stacked top-up trace time <= sum of the eight per-frame ones + that sum's spread
  warm_wall      warm stacked call's wall time <= sum of the eight warm calls' + that sum's spread

    python tools/gbuffer_sequence_adaptive_timing.py [--out FILE] [--repeats 3] [--configs C2-256,...]
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
KEYS = ("trace_wall_ms", "cold_wall_ms", "warm_wall_ms", "top_up_trace_ms", "top_up_ms", "cold_shade_ms",
        "warm_shade_ms")


def circle(stock):
    (x, y, z), phi, theta, psi = stock
    out = []
    for k in range(K):
        a = 2.0 * math.pi * k / K
        out.append(((x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a), z), phi, theta, psi))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "sequence_adaptive_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    args = ap.parse_args()
    import gr_raytracer_amd as g

    if g.device_count() < 1:
        raise SystemExit("gbuffer_sequence_adaptive_timing: no GPU visible (there is no CPU path to time)")
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    wanted = set(args.configs.split(","))
    results, ok = [], True
    for name, size, toml, stock, max_steps in CONFIGS:
        if name not in wanted:
            continue
        cams = circle(stock)

        def opts(row):
            return g.GlobalOpts(width=size, height=size, camera_position=row[0], phi=row[1], theta=row[2], psi=row[3],
                                max_steps=max_steps)

        def per_frame():
            t = dict.fromkeys(KEYS, 0.0)
            pairs, frames, counts = [], [], []
            t0 = time.perf_counter()
            for row in cams:  # eight tracer scenes, eight traces
                hs = g.HostScene(str(scenes / toml), opts(row), str(res))
                sc = g.Scene(hs.desc_ptr(), keepalive=hs, adaptive=hs.adaptive)
                pairs.append((hs, sc, sc.trace_gbuffer()))
            t["trace_wall_ms"] = (time.perf_counter() - t0) * 1e3
            for hs, sc, gb in pairs:  # cold: the frame's selection is its top-up
                t0 = time.perf_counter()
                _, rep = gb.shade_section(sc, adaptive=hs.adaptive, tracer=sc)
                t["cold_wall_ms"] += (time.perf_counter() - t0) * 1e3
                t["top_up_trace_ms"] += rep["top_up"]["kernel_ms"]
                t["top_up_ms"] += rep["trace_ms"]
                t["cold_shade_ms"] += rep["shade_ms"]
                counts.append(rep["n_traced"])
            for hs, sc, gb in pairs:  # warm: the set holds the selection
                t0 = time.perf_counter()
                got, rep = gb.shade_section(sc, adaptive=hs.adaptive)
                t["warm_wall_ms"] += (time.perf_counter() - t0) * 1e3
                t["warm_shade_ms"] += rep["shade_ms"]
                assert rep["n_traced"] == 0
                frames.append(got)
            for hs, sc, gb in pairs:
                gb.close()
                sc.close()
                hs.close()
            return t, frames, counts

        def stacked():
            t = dict.fromkeys(KEYS, 0.0)
            t0 = time.perf_counter()
            hs = g.HostScene(str(scenes / toml), opts(cams[0]), str(res))
            sc = g.Scene(hs.desc_ptr(), keepalive=hs, adaptive=hs.adaptive)
            seq = sc.trace_gbuffer_sequence([hs.camera(*row) for row in cams])
            t["trace_wall_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            _, rep = g.shade_section_sequence(seq, sc, adaptive=hs.adaptive, tracer=sc)
            t["cold_wall_ms"] = (time.perf_counter() - t0) * 1e3
            t["top_up_trace_ms"] = rep["top_up"]["kernel_ms"]
            t["top_up_ms"] = rep["trace_ms"]
            t["cold_shade_ms"] = rep["shade_ms"]
            counts = [int(v) for v in rep["per_frame"][:, 2]]
            t0 = time.perf_counter()
            got, rep = g.shade_section_sequence(seq, sc, adaptive=hs.adaptive)
            t["warm_wall_ms"] = (time.perf_counter() - t0) * 1e3
            t["warm_shade_ms"] = rep["shade_ms"]
            t["n_launches"] = rep["n_launches"]
            assert rep["n_traced"] == 0
            for gb in seq:
                gb.close()
            sc.close()
            hs.close()
            return t, got, counts

        _, frames, counts_a = per_frame()  # warm-up of both legs, and the identity check
        _, got, counts_b = stacked()
        same = counts_a == counts_b and all(
            np.array_equal(got["xyza64"][k].view(np.uint64), frames[k].xyza64.view(np.uint64)) and
            np.array_equal(got["class"][k], frames[k].ray_class) and np.array_equal(got["status"][k], frames[k].status) and
            int(got["n_supersampled"][k]) == frames[k].n_supersampled for k in range(K))
        del frames, got
        a_runs, b_runs = [], []
        for _ in range(args.repeats):
            a_runs.append(per_frame()[0])
            b_runs.append(stacked()[0])

        def stat(runs, key):
            v = [r[key] for r in runs]
            return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "values": v}

        entry = {"config": name, "scene": toml, "width": size, "height": size, "cameras": K, "max_steps": max_steps,
                 "selected_per_frame": counts_b, "frames_identical": bool(same), "per_frame": a_runs, "stacked": b_runs}
        for key in KEYS:
            a, b = stat(a_runs, key), stat(b_runs, key)
            entry[key] = {"per_frame": a, "stacked": b, "stacked_over_per_frame": b["median"] / a["median"]}

        def holds(key):
            a, b = entry[key]["per_frame"], entry[key]["stacked"]
            return bool(b["median"] <= a["median"] + a["spread"])

        entry["requirements"] = {"top_up_trace": holds("top_up_trace_ms"), "warm_wall": holds("warm_wall_ms")}
        ok = ok and same
        results.append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k not in ("per_frame", "stacked")}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"tool": "tools/gbuffer_sequence_adaptive_timing.py",
                               "library_sources": g._lib.source_stamp(), "repeats": args.repeats, "results": results},
                              indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
