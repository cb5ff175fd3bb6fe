"""The measured record of the VolumetricDisc unit checks (needs an MI355X).

    python tools/volumetric_march_record.py [--commit SHA] [--out profiles/volumetric/march_check.json]

Calls the functions tests/test_gpu_volumetric_checks.py calls (tests/volumetric_cases.py) on
the same scenes and job lists, and writes what they measure -- no assertion rests on these
figures: per raymarch case and arithmetic mode the maximum relative difference to the oracle
over the robust jobs and the share of jobs with the oracle's bits, and the largest distance
of the device's atan2 (OCML) from numpy.arctan2 in units of the last place over the density
test's points.  The record names the sources it came from (grt_source_hash, and the commit
given on the command line) and the device.
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
    import volumetric_cases as V
    from test_gpu_parity import gpu_scene

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "volumetric" / "march_check.json"))
    a = ap.parse_args()
    rec = {"commit": a.commit, "source_hash": grt._lib.source_stamp(), "device": torch.cuda.get_device_name(0),
           "bar": "1e-4 relative per channel on robust jobs (tests/test_gpu_parity.within)", "march": {}, "density": {}}
    for name, hs, jobs in V.march_cases(grt):
        sc = gpu_scene(grt, hs)
        ref_all, _, ns = V.oracle_march(oracle, hs.desc, jobs)
        robust = V.robust_jobs(oracle, hs.desc, jobs, ref_all)
        for arith, mode in ((0, "exact"), (1, "fused")):
            m = V.march_check(oracle, hs.desc, sc, 0, jobs, arith=arith, ref=(ref_all, ns), robust=robust)
            rec["march"][f"{name}/{mode}"] = {
                "jobs": len(jobs[0]), "robust_share": m["robust_share"], "max_rel_robust": m["max_rel_robust"],
                "bit_equal_share": m["bit_equal_share"], "device_samples": int(m["counters"][1]),
                "oracle_samples": m["oracle_samples"]}
    ulp = 0
    for scene, make in (("flat", V.flat_scene), ("schwarzschild", V.schw_scene)):
        for axis_name, axis in (("tilted", V.TILT), ("z", V.ZAXIS)):
            hs = make(grt, axis)
            m = V.density_check(oracle, hs.desc, gpu_scene(grt, hs), 0, V.density_points(oracle, hs.desc))
            rec["density"][f"{scene}/{axis_name}"] = m
            ulp = max(ulp, m["atan2_max_ulp"])
    rec["atan2_max_ulp"] = ulp
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
