"""Time the assembly of the multi-GPU geometry buffer on one MI355X and write
profiles/gbuffer/multi_timing.json.

There is no multi-GPU box: nothing here crosses xGMI, and a device list that names GPU 0
four times traces its four shards in turn, so its trace times say nothing about scaling.  What
one GPU can measure is what the assembly itself costs.

For C2's scene (schwarzschild.toml) and C3's scene (kerr-bl.toml) at 1500 x 1500, bands of 16
rows, five legs in one process:

  single          trace_gbuffer (grt_gbuffer_trace)
  peer-1, peer-4  trace_gbuffer_multi over [0] and over [0] * 4 under the peer transport
                  (the assembly kernels read every block where its rank left it)
  staged-1, staged-4
                  the same under peer-staged (one copy per block into devices[0]'s staging first)

One untimed pass of every leg warms the code objects and the allocator up; then the legs
alternate, three repetitions each.  Every buffer of every leg must equal the single-device one
byte for byte (exit status 1 otherwise).  Per leg: the wall time of the call (host clock; the
call ends synchronised), each rank's trace and scan + fill (events), gather_ms (events on
devices[0]: transport + assembly), the bytes the blocks hold.  The yardstick for the gather is a
plain hipMemcpyAsync device-to-device copy of that many bytes, timed with events beside each
repetition: the assembly reads and writes each byte once, so the copy is its floor.  Medians,
all raw values and the ratio gather / copy are kept.  No ratio is required: the file records what
came out.

    python tools/gbuffer_multi_timing.py [--out profiles/gbuffer/multi_timing.json] [--repeats 3] [--size 1500]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BAND = 16
SCENES = [("C2", "schwarzschild.toml", dict(camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=100000)),
          ("C3", "kerr-bl.toml", dict(camera_position=(-10.0, 0.0, -0.5), theta=-3.14159, max_steps=1000000))]
LEGS = [("single", None, 0), ("peer-1", "peer", 1), ("staged-1", "peer-staged", 1), ("peer-4", "peer", 4),
        ("staged-4", "peer-staged", 4)]


class Hip:
    """The four runtime calls of the yardstick copy, from the HIP runtime libgrt.so already loaded."""

    def __init__(self):
        try:
            self.rt = C.CDLL("libamdhip64.so")
        except OSError:
            self.rt = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        for name, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                           ("hipMemcpyAsync", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
                           ("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                           ("hipEventSynchronize", [C.c_void_p]), ("hipEventDestroy", [C.c_void_p]),
                           ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
                           ("hipMemset", [C.c_void_p, C.c_int, C.c_size_t]), ("hipSetDevice", [C.c_int])):
            fn = getattr(self.rt, name)
            fn.restype, fn.argtypes = C.c_int, args

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc})")

    def copy_ms(self, nbytes):
        """Event time of one hipMemcpyAsync device-to-device copy of nbytes on the null stream."""
        self.ok(self.rt.hipSetDevice(0), "hipSetDevice")
        src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ok(self.rt.hipMalloc(C.byref(src), nbytes), "hipMalloc")
        self.ok(self.rt.hipMalloc(C.byref(dst), nbytes), "hipMalloc")
        try:
            self.ok(self.rt.hipMemset(src, 1, nbytes), "hipMemset")
            self.ok(self.rt.hipMemset(dst, 0, nbytes), "hipMemset")
            self.ok(self.rt.hipEventCreate(C.byref(e0)), "hipEventCreate")
            self.ok(self.rt.hipEventCreate(C.byref(e1)), "hipEventCreate")
            self.ok(self.rt.hipEventRecord(e0, None), "hipEventRecord")
            self.ok(self.rt.hipMemcpyAsync(dst, src, nbytes, 3, None), "hipMemcpyAsync")  # hipMemcpyDeviceToDevice
            self.ok(self.rt.hipEventRecord(e1, None), "hipEventRecord")
            self.ok(self.rt.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float()
            self.ok(self.rt.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            self.rt.hipEventDestroy(e0)
            self.rt.hipEventDestroy(e1)
            return float(ms.value)
        finally:
            self.rt.hipFree(src)
            self.rt.hipFree(dst)


def run_leg(sc, transport, n):
    t0 = time.perf_counter()
    gb = sc.trace_gbuffer() if n == 0 else sc.trace_gbuffer_multi([0] * n, BAND, transport=transport)
    wall = (time.perf_counter() - t0) * 1e3
    rec = {"wall_ms": wall, "trace_times": gb.trace_times}
    if n:
        r = gb.report
        rec.update(transport=int(r.transport), rank_trace_ms=[r.trace_ms[k] for k in range(n)],
                   rank_fill_ms=[r.fill_ms[k] for k in range(n)], rank_rows=[int(r.rows[k]) for k in range(n)],
                   rank_layers=[int(r.layers[k]) for k in range(n)], n_traces=[int(r.n_traces[k]) for k in range(n)],
                   block_bytes=sum(int(r.block_bytes[k]) for k in range(n)), gather_ms=float(r.gather_ms),
                   report_wall_ms=float(r.wall_ms))
    return gb, rec


def med(xs):
    return {"median": statistics.median(xs), "spread": max(xs) - min(xs), "values": list(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gbuffer" / "multi_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=1500)
    a = ap.parse_args()
    import gr_raytracer_amd as grt

    if grt.device_count() < 1:
        raise SystemExit("no GPU visible: nothing is measured")
    hip = Hip()
    doc = {"what": __doc__.split("\n\n")[0].replace("\n", " "),
           "note": "No N > 1 frame over distinct GPUs has run on hardware under any transport; the four ranks of "
                   "peer-4 / staged-4 share GPU 0 and trace in turn: their trace times say nothing about scaling",
           "size": a.size, "band_rows": BAND, "repeats": a.repeats, "source": grt._lib.source_stamp(), "scenes": {}}
    equal = True
    for tag, toml, kw in SCENES:
        opts = grt.GlobalOpts(width=a.size, height=a.size, **kw)
        hs = grt.HostScene(str(ROOT / "tests" / "golden" / "scenes" / toml), opts, str(ROOT / "tests" / "golden"))
        sc = grt.Scene(hs.desc_ptr(), keepalive=hs)
        ref = None
        raw = {name: [] for name, _, _ in LEGS}
        copies = {name: [] for name, _, n in LEGS if n}
        for rep in range(a.repeats + 1):  # pass 0 is untimed
            for name, transport, n in LEGS:
                gb, rec = run_leg(sc, transport, n)
                arrays, info = gb.arrays(), bytes(gb.info)
                if ref is None:
                    ref = (info, {k: v.tobytes() for k, v in arrays.items()})
                same = info == ref[0] and all(arrays[k].tobytes() == ref[1][k] for k in ref[1])
                equal &= same
                rec["equal_to_single"] = same
                if n:
                    rec["copy_ms"] = hip.copy_ms(rec["block_bytes"])
                gb.close()
                if rep:
                    raw[name].append(rec)
                    if n:
                        copies[name].append(rec["copy_ms"])
                print(tag, rep, name, json.dumps({k: v for k, v in rec.items() if not k.startswith("rank_")}), flush=True)
        out = {"n_pixels": a.size * a.size, "n_layers": len(ref[1]["object"]), "legs": {}}
        for name, transport, n in LEGS:
            leg = {"wall_ms": med([r["wall_ms"] for r in raw[name]]),
                   "trace_ms": med([r["trace_times"]["trace_ms"] for r in raw[name]]),
                   "fill_ms": med([r["trace_times"]["fill_ms"] for r in raw[name]]),
                   "equal_to_single": all(r["equal_to_single"] for r in raw[name])}
            if n:
                g, c = med([r["gather_ms"] for r in raw[name]]), med(copies[name])
                leg.update(transport=raw[name][0]["transport"], block_bytes=raw[name][0]["block_bytes"],
                           rank_rows=raw[name][0]["rank_rows"], rank_layers=raw[name][0]["rank_layers"],
                           n_traces=[r["n_traces"] for r in raw[name]],
                           rank_trace_ms=[med([r["rank_trace_ms"][k] for r in raw[name]]) for k in range(n)],
                           rank_fill_ms=[med([r["rank_fill_ms"][k] for r in raw[name]]) for k in range(n)],
                           gather_ms=g, copy_ms=c, gather_over_copy=g["median"] / c["median"],
                           copy_gb_per_s=2 * raw[name][0]["block_bytes"] / c["median"] / 1e6,
                           gather_gb_per_s=2 * raw[name][0]["block_bytes"] / g["median"] / 1e6)
            out["legs"][name] = leg
        doc["scenes"][tag] = out
        sc.close()
    doc["all_equal"] = equal
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print("wrote", a.out, "all_equal", equal)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
