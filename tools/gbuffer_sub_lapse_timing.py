"""Time the timed sub-sample set and the retarded adaptive re-shade on one MI355X and write
profiles/gbuffer/sub_lapse_timing.json.

For C2's scene (schwarzschild.toml, its stock bitmap disc) and C3's scene (kerr-bl.toml, the
disc's BlackBody texture replaced by a seeded 64 x 64 bitmap) at 1500 x 1500 under the stock
[adaptive_sampling], in one process, after one untimed pass of everything, three repetitions
with all listed, measured alternating in the same run:

  (a) the cold top-up of the stock selection -- the static frame's, so the same pixels either
      way -- through the lapse units (grt_gbuffer_supersample_lapse) against the exact units
      (grt_gbuffer_supersample): the traces' event time (stats.kernel_ms) and the call's wall
      time, each on an empty set.  No ratio is set in advance: the timed fill is reported
      relative to the plain fill's median and to the plain fill's own spread (max - min over
      its repetitions) in this run;
  (b) a warm grt_gbuffer_shade_section_at_retarded (the set holds the selection) against a
      warm grt_gbuffer_shade_section_at on a buffer whose set holds that call's selection:
      shade_ms (device events) and wall time;
  (c) grt_render_section_ex's kernel time (stats.kernel_ms), what a frame costs without the buffer.

The timed fill must leave the plain fill's set byte for byte, and the warm calls must trace
nothing (exit status 1 otherwise).  The one requirement on the times (exit status 1 when
missed): the warm retarded call's wall time is below render_section_ex's kernel time in every
repetition.

    python tools/gbuffer_sub_lapse_timing.py [--out profiles/gbuffer/sub_lapse_timing.json] [--repeats 3] [--size 1500]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from gbuffer_orbit_timing import CONFIGS, same, with_bitmap_disc  # noqa: E402

T = 37.5
MARK = (-1.0, -1.0, -1.0, -1.0)  # the mask pass paints the selection; no shaded pixel has this alpha


def summary(rows, key):
    v = [r[key] for r in rows]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "sub_lapse_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=1500)
    args = ap.parse_args()
    import gr_raytracer_amd as g

    if g.device_count() < 1:
        raise SystemExit("gbuffer_sub_lapse_timing: no GPU visible (there is no CPU path to time)")
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    results, ok = [], True
    for name, toml, cam in CONFIGS:
        hs = g.HostScene(str(scenes / toml), g.GlobalOpts(width=args.size, height=args.size, **cam), str(res))
        sc, replaced = with_bitmap_disc(g, hs)
        ad = hs.adaptive
        spa = int(ad.samples_per_axis)
        gb = sc.trace_gbuffer(lapse=True)  # both kinds of set are filled on this one buffer, in turn
        painted, _ = gb.shade_section(sc, adaptive=ad, sampling_mask_xyza=MARK)
        px = np.flatnonzero(painted.xyza64[:, 3] == -1.0).astype(np.uint32)  # the stock selection

        def fill(lapse):
            gb.clear_sub()
            t0 = time.perf_counter()
            st = gb.supersample(sc, px, spa, lapse=lapse)
            return {"trace_ms": st["kernel_ms"], "wall_ms": (time.perf_counter() - t0) * 1e3, "rays": st["rays"]}

        def section(buf, retarded):
            t0 = time.perf_counter()
            fr, rep = buf.shade_section(sc, adaptive=ad, time=T, retarded=retarded)
            return {"shade_ms": rep["shade_ms"], "wall_ms": (time.perf_counter() - t0) * 1e3, "n_traced": rep["n_traced"],
                    "n_selected": rep["n_selected"]}

        def render():
            t0 = time.perf_counter()
            r = sc.render_section_ex(adaptive=ad, failure_capacity=1)
            return {"kernel_ms": r.stats["kernel_ms"], "wall_ms": (time.perf_counter() - t0) * 1e3}

        # the untimed pass, and the identity checks
        fill(False)
        plain_set, plain_info = gb.sub_arrays(), bytes(gb.sub_info)
        fill(True)
        timed_set = gb.sub_arrays()
        same_set = plain_info == bytes(gb.sub_info) and all(same(plain_set[k], timed_set[k]) for k in plain_set)
        sub_lapse = gb.sub_lapse()
        n_sub_layers = int(gb.sub_info.n_sub_layers)
        del plain_set, timed_set
        render()
        # the two warm buffers: each holds its own call's selection at T after one top-up
        fast, slow = sc.trace_gbuffer(), sc.trace_gbuffer(lapse=True)
        fast.shade_section(sc, adaptive=ad, tracer=sc, time=T)
        slow.shade_section(sc, adaptive=ad, tracer=sc, time=T, retarded=True)
        section(fast, False), section(slow, True)

        rows = {"plain_fill": [], "timed_fill": [], "section_at": [], "section_at_retarded": [], "render_section_ex": []}
        for _ in range(args.repeats):  # alternating
            rows["plain_fill"].append(fill(False))
            rows["timed_fill"].append(fill(True))
            rows["section_at"].append(section(fast, False))
            rows["section_at_retarded"].append(section(slow, True))
            rows["render_section_ex"].append(render())
        warm = all(r["n_traced"] == 0 for k in ("section_at", "section_at_retarded") for r in rows[k])
        fl = {k: {f: summary(rows[k], f) for f in ("trace_ms", "wall_ms")} for k in ("plain_fill", "timed_fill")}
        se = {k: {f: summary(rows[k], f) for f in ("shade_ms", "wall_ms")} for k in ("section_at", "section_at_retarded")}
        rk = summary(rows["render_section_ex"], "kernel_ms")
        spread = fl["plain_fill"]["trace_ms"]["max"] - fl["plain_fill"]["trace_ms"]["min"]
        diff = fl["timed_fill"]["trace_ms"]["median"] - fl["plain_fill"]["trace_ms"]["median"]
        faster = all(s["wall_ms"] < r["kernel_ms"] for s, r in zip(rows["section_at_retarded"], rows["render_section_ex"]))
        ok = ok and same_set and warm and faster
        results.append({
            "config": name, "scene": toml, "size": args.size, "bitmap_discs_substituted": replaced,
            "samples_per_axis": spa, "n_selected_static": int(px.size), "n_sub_layers": n_sub_layers,
            "sub_lapse_min": float(sub_lapse.min()), "sub_lapse_max": float(sub_lapse.max()),
            "n_selected_at_t": {"fast_light": rows["section_at"][0]["n_selected"],
                                "retarded": rows["section_at_retarded"][0]["n_selected"]},
            "timed_fill_leaves_the_plain_set": same_set, "warm_calls_trace_nothing": warm,
            "cold_top_up": fl, "warm_section": se, "render_section_ex_kernel_ms": rk,
            "timed_fill_minus_plain_ms": diff,
            "timed_fill_over_plain": fl["timed_fill"]["trace_ms"]["median"] / fl["plain_fill"]["trace_ms"]["median"],
            "plain_fill_spread_ms": spread, "timed_fill_within_plain_spread": abs(diff) <= spread,
            "retarded_over_fast_light_shade": se["section_at_retarded"]["shade_ms"]["median"] / se["section_at"]["shade_ms"]["median"],
            "warm_retarded_wall_over_render_kernel": se["section_at_retarded"]["wall_ms"]["median"] / rk["median"],
            "warm_retarded_wall_below_render_kernel": faster,
        })
        print(f"{name}: {px.size} selected; cold top-up plain {fl['plain_fill']['trace_ms']['median']:.2f} ms (spread "
              f"{spread:.2f}), timed {fl['timed_fill']['trace_ms']['median']:.2f} ms; warm section at t: fast-light "
              f"{se['section_at']['shade_ms']['median']:.3f} ms, retarded {se['section_at_retarded']['shade_ms']['median']:.3f} ms "
              f"(wall {se['section_at_retarded']['wall_ms']['median']:.1f} ms against render_section_ex's kernel "
              f"{rk['median']:.1f} ms)", flush=True)
        for b in (gb, fast, slow):
            b.close()
    doc = {"what": "tools/gbuffer_sub_lapse_timing.py: one process, one untimed pass, alternating, "
                   f"{args.repeats} repetitions with all listed; times in ms", "time": T,
           "source_stamp": g._lib.source_stamp(), "ok": ok, "results": results}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
