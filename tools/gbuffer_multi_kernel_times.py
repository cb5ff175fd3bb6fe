"""Kernel times of the multi-GPU g-buffer's assembly, from a profiler run of its own, written
to profiles/gbuffer/multi_kernel_times.json (DESIGN §14's split of gather_ms).

The trace comes from one repetition of tools/gbuffer_multi_timing.py under the profiler:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o gather -- \
        python tools/gbuffer_multi_timing.py --repeats 1 --out DIR/timing_under_profiler.json
    python tools/gbuffer_multi_kernel_times.py DIR/gather_kernel_trace.csv [--out FILE]

That run makes 16 assemblies in a fixed order: per scene (C2, C3) an untimed and a timed pass,
each over the legs peer-1, staged-1, peer-4, staged-4.  Per assembly this keeps the duration
of gbuffer_gather_pixels_kernel, the summed durations of the scan's kernels that follow it,
and the duration of gbuffer_gather_layers_kernel, in microseconds.  Tracing slows the host, so
only kernel durations are taken from this run; gather_ms is multi_timing.json's.
"""
import argparse
import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LEGS = ("peer-1", "staged-1", "peer-4", "staged-4")
SCENES = ("C2", "C3")


def assemblies(trace_csv):
    out, cur = [], None
    for r in csv.DictReader(open(trace_csv)):
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "gbuffer_gather_pixels_kernel" in name:
            cur = {"pixels_us": us, "scan_us": 0.0, "scan_kernels": 0, "layers_us": None}
            out.append(cur)
        elif "gbuffer_gather_layers_kernel" in name and cur is not None:
            cur["layers_us"] = us
            cur = None
        elif cur is not None and "grt::" in name:
            cur = None  # another kernel of the library: the assembly (one without layers) is over
        elif cur is not None:  # the scan's kernels (rocPRIM), between the two
            cur["scan_us"] += us
            cur["scan_kernels"] += 1
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "multi_kernel_times.json"))
    a = ap.parse_args()
    got = assemblies(a.trace)
    want = len(SCENES) * 2 * len(LEGS)
    if len(got) != want:
        sys.exit(f"{len(got)} assemblies in the trace, expected {want} (one repetition of gbuffer_multi_timing.py)")
    doc = {"what": "kernel durations (us) of each assembly of one repetition of tools/gbuffer_multi_timing.py under "
                   "rocprofv3 --kernel-trace: the pixel kernel, the scan's kernels, the layer kernel",
           "scenes": {}}
    it = iter(got)
    for tag in SCENES:
        doc["scenes"][tag] = {p: {leg: next(it) for leg in LEGS} for p in ("untimed_pass", "timed_pass")}
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print("wrote", a.out)
