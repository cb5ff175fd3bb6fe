"""Time the disc's orbital motion from one geometry buffer on one MI355X and write
profiles/gbuffer/orbit_timing.json.

For C2's scene (schwarzschild.toml, its stock bitmap disc) and C3's scene (kerr-bl.toml, the
disc's BlackBody texture replaced by a seeded 64 x 64 bitmap) at 1500 x 1500, in one process,
after one untimed pass of everything (code objects, allocator, the scene's device copy),
medians of three repetitions of

  (a) grt_gbuffer_shade_times with K = 8 times (xyza, xyza64, class, status): kernel_ms (device
      events) and the whole call's wall time, against eight grt_gbuffer_shade calls on the same
      buffer -- the static shade is the only yardstick the code before this feature has -- and
      against the trace: render_pixels' kernel_ms of the same scene in the same run;
  (b) where the library still has both variants of the K-times kernel (the debug knob
      grt_debug_orbit_cached; the slower one was deleted after this file was written, see
      DESIGN.md section 15), inline omega against omega cached per layer by a pre-pass,
      alternating, with the default launch groups and with all eight frames in one group;
  (c) a warm grt_gbuffer_shade_section_at (stock adaptive configuration, the set already holds
      the selection) against a warm grt_gbuffer_shade_section: shade_ms and wall time.

Every frame of the K = 8 call must equal the K = 1 call at its time bit for bit, in both
variants, and the frame at t = 0 the static shade (exit status 1 otherwise).  The one
requirement on the times (exit status 1 when missed): the K = 8 call's wall time is below
eight times render_pixels' kernel time in every repetition.  All raw times are kept.

    python tools/gbuffer_orbit_timing.py [--out profiles/gbuffer/orbit_timing.json] [--repeats 3] [--size 1500]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

K = 8
TIMES = [12.5 * k for k in range(K)]
FIELDS = ("xyza", "xyza64", "class", "status")  # what grt_gbuffer_shade returns
CONFIGS = [
    ("C2", "schwarzschild.toml", dict(camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=100000)),
    ("C3", "kerr-bl.toml", dict(camera_position=(-10.0, 0.0, -0.5), theta=-3.14159, max_steps=1000000)),
]


def with_bitmap_disc(g, hs):
    """A scene of hs's descriptor whose discs all have a bitmap texture (BlackBody ones replaced)."""
    L = g._lib
    d = type(hs.desc).from_buffer_copy(hs.desc)
    keep = [hs, d]
    replaced = 0
    for k in range(d.n_objects):
        o = d.objects[k]
        if o.kind == L.OBJ_DISC and o.texture.kind != L.TEX_BITMAP:
            rng = np.random.default_rng(7)
            rgba = rng.integers(0, 256, (64, 64, 4)).astype(np.uint8)
            rgba[..., 3] = 255
            b = g.SceneBuilder(L.GEOM_EUCLIDEAN)
            o.texture = b._texture(g.Bitmap(o.texture.beaming_exponent, rgba))
            keep.append(b)
            replaced += 1
    return g.Scene(C.pointer(d), keepalive=keep, adaptive=hs.adaptive), replaced


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "orbit_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=1500)
    args = ap.parse_args()
    import gr_raytracer_amd as g

    if g.device_count() < 1:
        raise SystemExit("gbuffer_orbit_timing: no GPU visible (there is no CPU path to time)")
    lib = g._lib.lib()
    has_variants = hasattr(lib, "grt_debug_orbit_cached")
    if has_variants:
        lib.grt_debug_orbit_cached.argtypes, lib.grt_debug_orbit_cached.restype = [C.c_int], C.c_int
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    n = args.size * args.size
    results, ok = [], True
    for name, toml, cam in CONFIGS:
        hs = g.HostScene(str(scenes / toml), g.GlobalOpts(width=args.size, height=args.size, **cam), str(res))
        sc, replaced = with_bitmap_disc(g, hs)
        ad = hs.adaptive

        def variant(on):
            if has_variants:
                lib.grt_debug_orbit_cached(1 if on else 0)

        def shade_times(times=TIMES):
            t0 = time.perf_counter()
            out = gb.shade_orbit(sc, times, fields=FIELDS)
            return out, {"kernel_ms": out["stats"]["kernel_ms"], "wall_ms": (time.perf_counter() - t0) * 1e3}

        def eight_shades():
            t0 = time.perf_counter()
            shades = [gb.shade(sc) for _ in range(K)]
            return shades, {"kernel_ms": sum(s.stats["kernel_ms"] for s in shades),
                            "wall_ms": (time.perf_counter() - t0) * 1e3}

        def section(t):
            t0 = time.perf_counter()
            fr, rep = gb.shade_section(sc, adaptive=ad, tracer=sc, time=t)
            return fr, {"shade_ms": rep["shade_ms"], "wall_ms": (time.perf_counter() - t0) * 1e3,
                        "n_traced": rep["n_traced"], "n_selected": rep["n_selected"]}

        # the untimed pass, and the identity checks
        trace = sc.render_pixels(0, 0, args.size, args.size)
        gb = sc.trace_gbuffer()
        static = gb.shade(sc)
        variant(False)
        out, _ = shade_times()
        singles = [shade_times([t])[0] for t in TIMES]
        frames_ok = all(same(out[f][k], singles[k][f][0]) for k in range(K) for f in FIELDS)
        zero_ok = (same(out["xyza"][0], static.xyza) and same(out["xyza64"][0], static.xyza64) and
                   same(out["class"][0], static.ray_class) and same(out["status"][0], static.status))
        moved = int(np.any(out["xyza64"][1].view(np.uint64) != out["xyza64"][0].view(np.uint64), axis=1).sum())
        variants_ok = None
        if has_variants:
            variant(True)
            cached, _ = shade_times()
            variants_ok = all(same(cached[f], out[f]) for f in FIELDS)
            g.set_sequence_group(K * n)
            variants_ok = variants_ok and all(same(shade_times()[0][f], out[f]) for f in FIELDS)
            g.set_sequence_group(0)
            variant(False)
        section(None), section(37.5), section(None)  # fills the set for both selections
        del out, singles
        runs = []
        for _ in range(args.repeats):
            r = {"render_pixels_kernel_ms": sc.render_pixels(0, 0, args.size, args.size).stats["kernel_ms"]}
            r["eight_shades"] = eight_shades()[1]
            r["shade_times"] = shade_times()[1]
            if has_variants:
                for group, label in ((0, "default_groups"), (K * n, "one_group")):
                    g.set_sequence_group(group)
                    for on, key in ((False, "inline"), (True, "cached"), (False, "inline_again"), (True, "cached_again")):
                        variant(on)
                        r[f"{label}_{key}"] = shade_times()[1]
                g.set_sequence_group(0)
                variant(False)
            r["section_static"] = section(None)[1]
            r["section_at"] = section(37.5)[1]
            runs.append(r)

        def med(path):
            v = []
            for r in runs:
                x = r
                for p in path:
                    x = x[p]
                v.append(x)
            return {"median": float(np.median(v)), "spread": float(max(v) - min(v))}

        info = gb.info
        entry = {"config": name, "scene": toml, "width": args.size, "height": args.size, "times": TIMES,
                 "bitmap_discs_replaced": replaced, "n_pixels": int(info.n_pixels), "n_layers": int(info.n_layers),
                 "pixels_moved_between_frames_0_and_1": moved, "frames_equal_k1": bool(frames_ok),
                 "time_zero_equals_static": bool(zero_ok), "variants_identical": variants_ok, "runs": runs,
                 "render_pixels_kernel_ms": med(("render_pixels_kernel_ms",)),
                 "shade_times_kernel_ms": med(("shade_times", "kernel_ms")),
                 "shade_times_wall_ms": med(("shade_times", "wall_ms")),
                 "eight_shades_kernel_ms": med(("eight_shades", "kernel_ms")),
                 "eight_shades_wall_ms": med(("eight_shades", "wall_ms")),
                 "section_static_shade_ms": med(("section_static", "shade_ms")),
                 "section_at_shade_ms": med(("section_at", "shade_ms")),
                 "section_static_wall_ms": med(("section_static", "wall_ms")),
                 "section_at_wall_ms": med(("section_at", "wall_ms"))}
        if has_variants:
            for label in ("default_groups", "one_group"):
                for key in ("inline", "cached"):
                    v = [r[f"{label}_{key}{s}"]["kernel_ms"] for r in runs for s in ("", "_again")]
                    entry[f"{label}_{key}_kernel_ms"] = {"median": float(np.median(v)), "spread": float(max(v) - min(v))}
        tr = entry["render_pixels_kernel_ms"]["median"]
        entry["eight_frames_wall_over_eight_traces"] = entry["shade_times_wall_ms"]["median"] / (K * tr)
        entry["eight_frames_kernel_over_one_trace"] = entry["shade_times_kernel_ms"]["median"] / tr
        entry["beats_eight_traces"] = bool(all(r["shade_times"]["wall_ms"] < K * r["render_pixels_kernel_ms"] for r in runs))
        entry["warm_sections_trace_nothing"] = bool(all(r[k]["n_traced"] == 0 for r in runs
                                                        for k in ("section_static", "section_at")))
        ok = ok and frames_ok and zero_ok and variants_ok is not False and entry["beats_eight_traces"]
        results.append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k != "runs"}), flush=True)
        del trace, static
        gb.close()
        sc.close()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"tool": "tools/gbuffer_orbit_timing.py", "library_sources": g._lib.source_stamp(),
                               "repeats": args.repeats, "both_kernel_variants": has_variants, "results": results},
                              indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
