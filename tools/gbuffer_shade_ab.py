"""A/B timing of the deferred shade on one MI355X: a build of the parent commit against this
checkout's library, and profiles/gbuffer/shade_unit_timing.json.

    python tools/gbuffer_shade_ab.py [--parent variants/parent/libgrt.so] [--rounds 5] [--calls 50] [--out FILE]

The parent's library is an out-of-tree build of the parent commit's csrc (make ALLOW_UNSTAMPED=1
OUT=variants/parent, as tools/build_variant.sh builds a variant).

The tool itself never touches the GPU.  It starts fresh child processes (this file with
--child) alternately with GRT_LIB pointing at each library (GRT_LIB_ALLOW_MISSING=1 for the
unstamped one), `--rounds` of them per library, each under its own `timeout`, and stops at the
first child that fails.

A child loads C2 and C3 as tools/gbuffer_orbit_timing.py sets them up (1500 x 1500, bitmap
disc), traces one buffer per scene, makes one untimed pass of every call -- all output fields;
their SHA-256 is the child's record of what the library computes -- and then takes the median
device time (kernel_ms, or the report's shade_ms) over `--calls` calls of each of
  shade             grt_gbuffer_shade
  shade_sequence    grt_gbuffer_shade_sequence, the buffer K = 8 times
  shade_times       grt_gbuffer_shade_times, K = 8 times
  section           warm grt_gbuffer_shade_section (stock adaptive configuration, the set holds the selection)
  section_at        warm grt_gbuffer_shade_section_at, t = 37.5
  section_sequence  warm grt_gbuffer_shade_section_sequence of the buffer

Acceptance (exit status 1 otherwise): the two libraries' output hashes are equal for every
(scene, call), and for every (scene, call) the change's median over rounds is at most the
parent's median over rounds plus the parent's own range over rounds (max - min of its round
medians): the noise the machine shows on unchanged code in the same session.  All raw values
are kept.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

K = 8
TIMES = [12.5 * k for k in range(K)]
T_AT = 37.5
CALLS = ("shade", "shade_sequence", "shade_times", "section", "section_at", "section_sequence")
LIGHT = ("xyza", "class", "status")  # the timed K = 8 calls: one colour array per frame


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def child(args):
    import numpy as np

    import gr_raytracer_amd as g
    sys.path.insert(0, str(ROOT / "tools"))
    from gbuffer_orbit_timing import CONFIGS, with_bitmap_disc

    if g.device_count() < 1:
        raise SystemExit("gbuffer_shade_ab: no GPU visible (there is no CPU path to time)")
    scenes, res = ROOT / "tests" / "golden" / "scenes", ROOT / "tests" / "golden"
    results = {}
    for name, toml, cam in CONFIGS:
        hs = g.HostScene(str(scenes / toml), g.GlobalOpts(width=args.size, height=args.size, **cam), str(res))
        sc, _ = with_bitmap_disc(g, hs)
        ad = hs.adaptive
        gb = sc.trace_gbuffer()

        def frames(d):
            return [d[f] for f in ("xyza", "xyza64", "class", "status", "stop", "steps")]

        def section(t):
            fr, rep = gb.shade_section(sc, adaptive=ad, tracer=sc, time=t)
            return (fr.xyza64, fr.ray_class, fr.status), rep

        def section_sequence():
            d, rep = g.shade_section_sequence([gb], sc, adaptive=ad, tracer=sc)
            return (d["xyza64"], d["class"], d["status"], d["stop"], d["steps"]), rep

        # the untimed pass of everything; the sections twice, so that the set holds both selections
        section(None), section(T_AT), section_sequence()
        st = gb.shade(sc)
        hashes = {"shade": sha(st.xyza, st.xyza64, st.ray_class, st.status),
                  "shade_sequence": sha(*frames(g.shade_sequence([gb] * K, sc))),
                  "shade_times": sha(*frames(gb.shade_orbit(sc, TIMES))),
                  "section": sha(*section(None)[0]), "section_at": sha(*section(T_AT)[0]),
                  "section_sequence": sha(*section_sequence()[0])}
        del st
        timed = {"shade": lambda: gb.shade(sc).stats["kernel_ms"],
                 "shade_sequence": lambda: g.shade_sequence([gb] * K, sc, fields=LIGHT)["stats"]["kernel_ms"],
                 "shade_times": lambda: gb.shade_orbit(sc, TIMES, fields=LIGHT)["stats"]["kernel_ms"],
                 "section": lambda: section(None)[1], "section_at": lambda: section(T_AT)[1],
                 "section_sequence": lambda: section_sequence()[1]}
        entry = {}
        for call in CALLS:
            ms = []
            for _ in range(args.calls):
                r = timed[call]()
                if isinstance(r, dict):  # a warm section traces nothing
                    assert r["n_traced"] == 0 and r["n_missing"] == 0, (name, call, r)
                    r = r["shade_ms"]
                ms.append(float(r))
            entry[call] = {"sha256": hashes[call], "median_ms": float(np.median(ms)), "ms": ms}
        info = gb.info
        entry["n_pixels"], entry["n_layers"] = int(info.n_pixels), int(info.n_layers)
        entry["n_sub_pixels"] = int(gb.sub_info.n_sub_pixels)
        results[name] = entry
        gb.close()
        sc.close()
    Path(args.out).write_text(json.dumps({"library": str(g._lib.LIB_PATH), "results": results}) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent", default=str(ROOT / "variants" / "parent" / "libgrt.so"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "shade_unit_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--size", type=int, default=1500)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds, per child")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.rounds < 5 or args.calls < 50:
        raise SystemExit("gbuffer_shade_ab: at least 5 rounds of at least 50 calls")
    import numpy as np

    change = ROOT / "gr_raytracer_amd" / "lib" / "libgrt.so"
    libs = {"parent": Path(args.parent).resolve(), "this_change": change}
    for p in libs.values():
        if not p.exists():
            raise SystemExit(f"gbuffer_shade_ab: {p} not found")
    rounds = {"parent": [], "this_change": []}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(args.rounds):
            for label, lib in libs.items():
                out = Path(tmp) / f"{label}_{r}.json"
                env = dict(os.environ, GRT_LIB=str(lib))
                env.pop("GRT_LIB_ALLOW_MISSING", None)
                if label == "parent":
                    env["GRT_LIB_ALLOW_MISSING"] = "1"
                cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, str(Path(__file__).resolve()),
                       "--child", "--out", str(out), "--calls", str(args.calls), "--size", str(args.size)]
                rc = subprocess.run(cmd, env=env, cwd=str(ROOT)).returncode
                if rc != 0:
                    print(f"gbuffer_shade_ab: the {label} child of round {r} ended with status {rc}; stopping", flush=True)
                    return 2
                rounds[label].append(json.loads(out.read_text())["results"])
                print(f"round {r} {label}: " + ", ".join(
                    f"{s}/{c} {rounds[label][-1][s][c]['median_ms']:.3f}" for s in rounds[label][-1] for c in CALLS), flush=True)
    summary, ok = {}, True
    for scene in rounds["parent"][0]:
        for call in CALLS:
            med = {label: [r[scene][call]["median_ms"] for r in rounds[label]] for label in rounds}
            hashes = {r[scene][call]["sha256"] for label in rounds for r in rounds[label]}
            p, c = med["parent"], med["this_change"]
            bar = float(np.median(p)) + (max(p) - min(p))
            e = {"parent_round_medians_ms": p, "this_change_round_medians_ms": c, "parent_median_ms": float(np.median(p)),
                 "parent_range_ms": max(p) - min(p), "this_change_median_ms": float(np.median(c)),
                 "this_change_range_ms": max(c) - min(c), "bar_ms": bar, "outputs_equal": len(hashes) == 1,
                 "within_bar": bool(float(np.median(c)) <= bar)}
            ok = ok and e["outputs_equal"] and e["within_bar"]
            summary[f"{scene}/{call}"] = e
            print(f"{scene}/{call}: parent {e['parent_median_ms']:.3f} ms (range {e['parent_range_ms']:.3f}), this change "
                  f"{e['this_change_median_ms']:.3f} ms, outputs {'equal' if e['outputs_equal'] else 'DIFFER'}, "
                  f"{'within' if e['within_bar'] else 'ABOVE'} the bar", flush=True)
    from gr_raytracer_amd import _lib

    doc = {"tool": "tools/gbuffer_shade_ab.py", "library_sources": _lib.source_stamp(), "size": args.size, "k": K,
           "rounds": args.rounds, "calls_per_round": args.calls, "accepted": bool(ok), "summary": summary, "raw": rounds}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
