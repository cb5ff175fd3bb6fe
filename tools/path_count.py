"""Code-path counts of the integrate kernel on one workload, from a diagnostic build
(-DGRT_PATH_COUNT=1, loaded through GRT_LIB; geodesic_rhs.h path_count): per path, how many
times a wave executed it (counted by its first active lane) and how many lanes did.
Kerr-Schild RHS: 0 range-free, 1 IEEE.  Schwarzschild / KerrBL RHS: 0 region-B table
with range-free divisions, 1 region-B Taylor with them, 2 region B with IEEE divisions,
3 general sincos; what the waves of 3 hold:
8 every lane in glibc's region A on the table path, 9 every lane in region A otherwise,
10 every lane in region C with n = 2, 11 mixed.  All: 4 near-field window pass,
5 accepted step, 6 attempt, 7 Schwarzschild attempt taken again with the full RKF sums
(rkf_short_ok missed).  Also among the waves of 3: 12 every lane in region B (the table and
Taylor cases mixed) with the division predicate, 13 every lane in region B without it.
usage: tools/path_count.py c2|c3|c4 [class-order modes, e.g. 0,1] (c4: row-band shard 2 of 8)
With modes (grt_set_class_order), one line per mode, each on a scene of its own; every
line carries "rhs_wave_share": the wave-level share of all RHS evaluations on paths 0, 1,
12 and 13 and on the general path (3), so a census before and after is one command each."""
import ctypes as C
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import gr_raytracer_amd as g  # noqa: E402
from gr_raytracer_amd import _lib as L  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "c2"
if which == "c4":
    opts = g.GlobalOpts(width=4096, height=4096, camera_position=(-10.0, 0.0, -0.5), theta=1.52, psi=-1.57,
                        max_steps=1000000)
    toml = "kerr.toml"
elif which == "c3":
    opts = g.GlobalOpts(width=1500, height=1500, camera_position=(-10.0, 0.0, -0.5), theta=-3.14159, max_steps=1000000)
    toml = "kerr-bl.toml"
else:
    opts = g.GlobalOpts(width=1500, height=1500, camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=100000)
    toml = "schwarzschild.toml"
modes = [int(m) for m in sys.argv[2].split(",")] if len(sys.argv) > 2 else [None]
fn = L.lib().grt_debug_path_counts
fn.restype = C.c_int
fn.argtypes = [C.POINTER(C.c_uint64), C.c_int]
NPATH = 14
cnt = (C.c_uint64 * (2 * NPATH))()


def census(mode):
    hs = g.HostScene(str(ROOT / "tests/golden/scenes" / toml), opts, str(ROOT / "tests/golden"))
    sc = g.Scene(hs.desc_ptr(), keepalive=hs)
    if mode is not None:
        L.check(L.lib().grt_set_class_order(mode), "grt_set_class_order")
    L.check(fn(cnt, 1), "grt_debug_path_counts")  # reset
    t = time.time()
    r = sc.render_shard(16, 2, 8, aux=False) if which == "c4" else sc.render_pixels(0, 0, 1500, 1500, aux=False)
    L.check(fn(cnt, 1), "grt_debug_path_counts")
    names = (["rhs_range_free", "rhs_ieee"] if which == "c4" else
             ["rhs_b_table_fast", "rhs_b_taylor_fast", "rhs_b_ieee", "rhs_general"]) 
    names += ["near_window", "accepted_general_path", "attempt"]
    keys = [0, 1] if which == "c4" else [0, 1, 2, 3]
    keys += [4, 5, 6]
    if which != "c4":
        names += ["rkf_full_form_recompute", "rhs_general_uniform_a_table", "rhs_general_uniform_a_other",
                  "rhs_general_uniform_c_n2", "rhs_general_mixed", "rhs_general_all_b_div_ok",
                  "rhs_general_all_b_div_missed"]
        keys += [7, 8, 9, 10, 11, 12, 13]
    out = {"workload": which, "kernel_ms": r.stats["kernel_ms"], "wall_s": round(time.time() - t, 3),
           "accepted_steps": r.stats["accepted_steps"], "attempts_total": r.stats["attempts"],
           "md5": hashlib.md5(r.xyza.tobytes() + r.ray_class.tobytes()).hexdigest()[:12]}
    for nm, k in zip(names, keys):
        w, ln = int(cnt[k]), int(cnt[NPATH + k])
        out[nm] = {"waves": w, "lanes": ln, "lanes_per_wave": round(ln / w, 2) if w else 0.0}
    if which != "c4":
        total = sum(int(cnt[k]) for k in (0, 1, 2, 3))
        out["class_order"] = mode
        out["rhs_wave_share"] = {nm: round(int(cnt[k]) / total, 5) for nm, k in
                                 (("path_0_b_table", 0), ("path_1_b_taylor", 1), ("path_2_b_ieee", 2),
                                  ("path_3_general", 3), ("path_12_all_b_mixed", 12), ("path_13_all_b_div_missed", 13))}
    print(json.dumps(out), flush=True)
    sc.close()


for m in modes:
    census(m)
