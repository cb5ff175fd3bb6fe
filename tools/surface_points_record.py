"""The measured record of the surface path's unit checks (needs an MI355X).

    python tools/surface_points_record.py [--commit SHA] [--out profiles/surface/points_check.json]

Calls the functions tests/test_gpu_surface_checks.py calls (tests/surface_cases.py) on the
same scenes and rows, and writes what they measure: per piece the row counts, the mismatch
counts (all 0 on a correct build) and the hit or far shares; the rows where the device's
log10 (OCML) differs from glibc's and the largest distance in units of the last place; the
rows whose beaming factor came from OCML's pow; and the window filter's refused-but-missing
share, on which no assertion rests.  The record names the sources it came from
(grt_source_hash, and the commit given on the command line) and the device.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))


def main():
    import torch

    import gr_raytracer_amd as grt
    import pyoracle as oracle
    import surface_cases as S
    from test_gpu_parity import gpu_scene

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "surface" / "points_check.json"))
    a = ap.parse_args()
    rec = {"commit": a.commit, "source_hash": grt._lib.source_stamp(), "device": torch.cuda.get_device_name(0),
           "chords": {}, "window_far": {}, "lut_index": {}, "temperature": {}, "texture": {}}

    def drop(m):
        m.pop("first_bad", None)
        return m

    hs = S.chord_scene(grt)
    sc = gpu_scene(grt, hs)
    rec["chords"]["disc"] = drop(S.chord_check(oracle, hs.desc, sc, 0, 0, S.FN_DISC, S.disc_rows()))
    rec["chords"]["sphere"] = drop(S.chord_check(oracle, hs.desc, sc, 0, 1, S.FN_SPHERE, S.sphere_rows()))
    rec["blend"] = drop(S.blend_check(oracle, sc, 0, S.blend_rows()))
    for chart in S.FAR_CHARTS:
        R = S.far_rows(chart)
        for kind in S.FAR_SCENES:
            hs = S.far_scene(grt, chart, kind)
            rec["window_far"][f"{chart}/{kind}"] = drop(S.far_check(oracle, hs.desc, gpu_scene(grt, hs), 0, R)[0])
    for n in S.LUT_SIZES:
        hs = S.lut_scene(grt, n)
        sc = gpu_scene(grt, hs)
        rec["lut_index"][f"lut_r/{n}"] = drop(S.table_check(hs, sc, 0, 0))
        rec["temperature"][f"lut_r/{n}"] = drop(S.temperature_check(oracle, hs.desc, sc, 0, 0, S.temperature_rows(hs)))
    rec["lut_index"]["bb_log_t/1000"] = drop(S.table_check(hs, sc, 0, -1))
    rec["blackbody"] = drop(S.blackbody_check(oracle, hs.desc, sc, 0, S.blackbody_rows(hs.bb_log_t)))
    for beaming in (0.0, 3.0):
        hs = S.texture_scene(grt, beaming)
        sc = gpu_scene(grt, hs)
        for kind in S.TEX_OBJECTS:
            rec["texture"][f"{kind}/beaming {beaming:g}"] = drop(S.texture_check(oracle, hs.desc, sc, 0, kind, S.texture_rows(kind)))
    tex = rec["texture"].values()
    rec["log10_rows_differing"] = rec["blackbody"]["log10_rows_differing"] + sum(m.get("log10_rows_differing", 0) for m in tex)
    rec["log10_max_ulp"] = max([rec["blackbody"]["log10_max_ulp"]] + [m.get("log10_max_ulp", 0) for m in tex])
    rec["pow_fallback_rows"] = sum(m["pow_fallback_rows"] for m in tex)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
