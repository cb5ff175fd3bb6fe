"""Time the lapse trace and the retarded-time shade on one MI355X and write
profiles/gbuffer/lapse_timing.json.

For C2's scene (schwarzschild.toml, its stock bitmap disc) and C3's scene (kerr-bl.toml, the
disc's BlackBody texture replaced by a seeded 64 x 64 bitmap) at 1500 x 1500, in one process,
after one untimed pass of everything, medians of three repetitions with all three listed,
measured alternating in the same run:

  (a) grt_gbuffer_trace_lapse against grt_gbuffer_trace: the trace's and the scan + fill's
      event times (grt_gbuffer_trace_times).  No ratio is set in advance: the lapse trace is
      reported relative to the plain trace's median and to the plain trace's own spread
      (max - min over its repetitions) in this run;
  (b) grt_gbuffer_shade_times_retarded with K = 8 times against grt_gbuffer_shade_times on the
      same buffer: kernel_ms (device events) and the call's wall time.

The lapse trace must leave the plain trace's twelve arrays byte for byte, and frame k of the
K = 8 retarded call must equal the K = 1 call at its time (exit status 1 otherwise).  The one
requirement on the times (exit status 1 when missed): the K = 8 retarded call's wall time is
below eight times the plain trace's time in every repetition.

    python tools/gbuffer_lapse_timing.py [--out profiles/gbuffer/lapse_timing.json] [--repeats 3] [--size 1500]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from gbuffer_orbit_timing import CONFIGS, FIELDS, K, TIMES, same, with_bitmap_disc  # noqa: E402


def summary(rows, key):
    v = [r[key] for r in rows]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "lapse_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=1500)
    args = ap.parse_args()
    import gr_raytracer_amd as g

    if g.device_count() < 1:
        raise SystemExit("gbuffer_lapse_timing: no GPU visible (there is no CPU path to time)")
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    results, ok = [], True
    for name, toml, cam in CONFIGS:
        hs = g.HostScene(str(scenes / toml), g.GlobalOpts(width=args.size, height=args.size, **cam), str(res))
        sc, replaced = with_bitmap_disc(g, hs)

        def trace(lapse):
            t0 = time.perf_counter()
            gb = sc.trace_gbuffer(lapse=lapse)
            wall = (time.perf_counter() - t0) * 1e3
            t = gb.trace_times
            return gb, {"trace_ms": t["trace_ms"], "fill_ms": t["fill_ms"], "wall_ms": wall}

        def shade(gb, retarded, times=TIMES):
            t0 = time.perf_counter()
            out = gb.shade_orbit(sc, times, fields=FIELDS, retarded=retarded)
            return out, {"kernel_ms": out["stats"]["kernel_ms"], "wall_ms": (time.perf_counter() - t0) * 1e3}

        # the untimed pass, and the identity checks
        plain, _ = trace(False)
        held, _ = trace(True)
        a, b = plain.arrays(), held.arrays()
        same_arrays = bytes(plain.info) == bytes(held.info) and all(same(a[k], b[k]) for k in a)
        lapse = held.lapse()
        out, _ = shade(held, True)
        shade(held, False)
        stacked = all(same(out[f][k], shade(held, True, [TIMES[k]])[0][f][0]) for k in (0, 3, K - 1) for f in FIELDS)
        ok = ok and same_arrays and stacked
        del a, b, out
        plain.close()

        rows = {"plain": [], "lapse": [], "fast_light": [], "retarded": []}
        for _ in range(args.repeats):  # alternating
            gb, t = trace(False)
            rows["plain"].append(t)
            gb.close()
            gb, t = trace(True)
            rows["lapse"].append(t)
            gb.close()
            rows["fast_light"].append(shade(held, False)[1])
            rows["retarded"].append(shade(held, True)[1])
        tr = {k: {f: summary(rows[k], f) for f in ("trace_ms", "fill_ms", "wall_ms")} for k in ("plain", "lapse")}
        sh = {k: {f: summary(rows[k], f) for f in ("kernel_ms", "wall_ms")} for k in ("fast_light", "retarded")}
        spread = tr["plain"]["trace_ms"]["max"] - tr["plain"]["trace_ms"]["min"]
        diff = tr["lapse"]["trace_ms"]["median"] - tr["plain"]["trace_ms"]["median"]
        faster = all(r["wall_ms"] < K * p["trace_ms"] for r, p in zip(rows["retarded"], rows["plain"]))
        ok = ok and faster
        results.append({
            "config": name, "scene": toml, "size": args.size, "bitmap_discs_substituted": replaced,
            "n_layers": int(held.info.n_layers), "lapse_min": float(lapse.min()), "lapse_max": float(lapse.max()),
            "lapse_trace_leaves_the_plain_arrays": same_arrays, "k8_equals_k1": stacked,
            "trace": tr, "shade_k8": sh,
            "lapse_trace_minus_plain_ms": diff,
            "lapse_trace_over_plain": tr["lapse"]["trace_ms"]["median"] / tr["plain"]["trace_ms"]["median"],
            "plain_trace_spread_ms": spread, "lapse_trace_within_plain_spread": abs(diff) <= spread,
            "lapse_fill_over_plain": tr["lapse"]["fill_ms"]["median"] / tr["plain"]["fill_ms"]["median"],
            "retarded_over_fast_light_kernel": sh["retarded"]["kernel_ms"]["median"] / sh["fast_light"]["kernel_ms"]["median"],
            "k8_retarded_wall_below_eight_traces": faster,
            "eight_traces_ms": K * tr["plain"]["trace_ms"]["median"],
        })
        print(f"{name}: trace plain {tr['plain']['trace_ms']['median']:.2f} ms (spread {spread:.2f}), lapse "
              f"{tr['lapse']['trace_ms']['median']:.2f} ms; scan + fill {tr['plain']['fill_ms']['median']:.3f} / "
              f"{tr['lapse']['fill_ms']['median']:.3f} ms; K = 8 kernel fast-light "
              f"{sh['fast_light']['kernel_ms']['median']:.3f} ms, retarded {sh['retarded']['kernel_ms']['median']:.3f} ms "
              f"(wall {sh['retarded']['wall_ms']['median']:.1f} ms against eight traces "
              f"{K * tr['plain']['trace_ms']['median']:.1f} ms)", flush=True)
        held.close()
    doc = {"what": "tools/gbuffer_lapse_timing.py: one process, one untimed pass, alternating, medians of "
                   f"{args.repeats} with all listed; times in ms", "k": K, "times": TIMES,
           "source_stamp": g._lib.source_stamp(), "ok": ok, "results": results}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
