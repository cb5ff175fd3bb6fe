"""Input sets for the glibc restatement (gr_raytracer_amd/csrc/device/glibc_math.h), shared
by tests/test_glibc_math.py (host hook against this machine's libm) and
tests/test_gpu_glibc_math.py (device hook against the host hook).

Every set is a deterministic, seeded float64 array (pow: a pair x, y) of N = 2^18 + 37
values: no multiple of any block size, so the last block of a launch is partial.  Names
carry the kind of the set:

  render_*   the arguments a render produces (the modes of tests/native/glibc_*_check.cpp)
  edge_*     every branch threshold of glibc_math.h +- a few ulps, both signs
  offpath_*  what the fast paths refuse (the wrappers fall back to the platform's libm)
  mixed_*    fast-path and off-path values interleaved with period 2, with period 7 and in
             runs of 64: lanes of both kinds in every wave, or whole waves side by side

The arrays are read-only and cached: compute once, share, leave unchanged."""
import functools

import numpy as np

N = (1 << 18) + 37

# function codes of grt_debug_glibc_device / grt_debug_glibc_host (csrc/device/glibc_check.h)
FN_POW, FN_SIN, FN_COS, FN_SINCOS, FN_VDISC_SINCOS, FN_EXP, FN_SINCOS_B = range(7)
FN_LIBM = 16  # host hook: | FN_LIBM = the host libm's own function on every lane
FN_NAMES = {FN_POW: "pow", FN_SIN: "sin", FN_COS: "cos", FN_SINCOS: "sincos", FN_VDISC_SINCOS: "vdisc_sincos",
            FN_EXP: "exp", FN_SINCOS_B: "sincos_b"}
FAMILY = {FN_POW: "pow", FN_SIN: "trig", FN_COS: "trig", FN_SINCOS: "trig", FN_VDISC_SINCOS: "trig", FN_EXP: "exp",
          FN_SINCOS_B: "trig"}
HAS_FALLBACK = (FN_POW, FN_SIN, FN_COS, FN_SINCOS, FN_VDISC_SINCOS)  # wrappers with a libm side
TWO_OUTPUTS = (FN_SINCOS, FN_VDISC_SINCOS, FN_SINCOS_B)

PI = 3.141592653589793
HP0 = float.fromhex("0x1.921fb54442d18p+0")   # glibc_tables.h: pi/2 = HP0 + HP1
HP1 = float.fromhex("0x1.1a62633145c07p-54")
TAYLOR_MAX = float.fromhex("0x1.020c49ba5e354p-3")
# high-word limits of sin_fast / cos_fast / sincos_fast (sin_fast's tiny-x limit is
# 0x3e500000 where the other two use 0x3e400000)
TRIG_HIGH_WORDS = (0x3e400000, 0x3e500000, 0x3feb6000, 0x400368fd, 0x419921fb)
POW_LOG_SPLIT = 0x3fe6955500000000  # pow_fast's log table: the binade is split here


def _from_bits(b):
    return np.asarray(b, np.uint64).view(np.float64)


def _high(word):
    return float(_from_bits([word << 32])[0])


TRIG_LIMIT = _high(0x419921fb)  # the fast paths cover |x| below this (~105414350)


def _rng(tag):
    return np.random.default_rng([20251019] + [ord(c) for c in tag])


def step(v, k):
    """v moved k ulps away from zero (k < 0: towards it); v, k broadcast."""
    v, k = np.broadcast_arrays(np.asarray(v, np.float64), np.asarray(k, np.int64))
    mag = np.abs(v).copy().view(np.int64) + k
    return np.copysign(mag.view(np.float64), v)


def around(points, span):
    """Every point +- 0..span ulps, positive then negative."""
    p = np.abs(np.asarray(points, np.float64))
    v = step(p[:, None], np.arange(-span, span + 1)[None, :]).ravel()
    return np.concatenate([v, -v])


def _edge_set(rng, points, span, spread):
    """around(points, span), filled up to N with points moved by random +-spread ulps."""
    core = around(points, span)[:N]
    m = N - core.size
    fill = step(rng.choice(np.abs(np.asarray(points, np.float64)), m), rng.integers(-spread, spread + 1, m))
    return np.concatenate([core, np.copysign(fill, rng.choice((-1.0, 1.0), m))])


def _mixed(fast, off):
    """fast / off (N each) interleaved three ways: {name: (values, is_fast)}; lane i of a
    mixed set holds fast[i] or off[i], so a fast lane can be compared with lane i of a
    launch over `fast` alone."""
    i = np.arange(N)
    masks = {"mixed_period_2": i % 2 == 0, "mixed_period_7": i % 7 != 3, "mixed_runs_of_64": (i // 64) % 2 == 0}
    return {k: (tuple(np.where(m, f, o) for f, o in zip(fast, off)), m) for k, m in masks.items()}


def _freeze(d):
    for v in d.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return d


# ------------------------------------------------------------------------- trig ----
@functools.lru_cache(maxsize=None)
def trig_sets():
    """{name: x} for sin / cos / sincos / the VolumetricDisc line / the region-B pair."""
    r = _rng("trig")
    u = lambda: r.random(N)
    s = {
        "render_ray_theta": (u() * 1.4 - 0.2) * PI,
        "render_periods": (u() - 0.5) * 40.0,
        "render_magnitudes": np.ldexp(u() - 0.5, r.integers(-40, 20, N)),  # 2^-41 .. 2^19
        "render_near_half_pi": 1.5707963267948966 + (u() - 0.5) * 1e-6,
        "render_reduction_limit": (u() - 0.5) * 2e8,
        "render_disc_phi": (u() * 2.0 - 1.0) * PI,
        "render_region_b": 1.5707963267948966 + (u() - 0.5) * 0.3,  # both sides of TAYLOR_MAX
    }
    s["edge_thresholds"] = _edge_set(r, [_high(w) for w in TRIG_HIGH_WORDS] + [TAYLOR_MAX], 8, 1 << 12)
    # multiples of pi/2 up to the reduction limit: the first 2048, 12000 random ones and the
    # last 64, each +- 4 ulps (n * pi/2 rounded from the 64-bit-mantissa product)
    n_max = int(TRIG_LIMIT / HP0)
    n = np.concatenate([np.arange(1, 2049), r.integers(2049, n_max - 64, 12000), np.arange(n_max - 63, n_max + 1)])
    mult = (n.astype(np.longdouble) * (np.longdouble(HP0) + np.longdouble(HP1))).astype(np.float64)
    s["edge_half_pi_multiples"] = _edge_set(r, mult, 4, 4)
    s["edge_region_b_taylor"] = _edge_set(r, [HP0 - TAYLOR_MAX, HP0 + TAYLOR_MAX], 64, 1 << 10)
    # the upper half of do_sin's Taylor range around every multiple of pi/2 up to +-8, where
    # the polynomial's last bit is most sensitive to how its operations are fused
    s["edge_taylor_top"] = (r.integers(-8, 9, N) * 1.5707963267948966 +
                            r.uniform(0.5, 1.0, N) * TAYLOR_MAX * r.choice((-1.0, 1.0), N))
    # beyond the fast paths: |x| from the limit to 1e300, and inf / nan
    off = np.exp(r.uniform(np.log(TRIG_LIMIT), np.log(1e300), N)) * r.choice((-1.0, 1.0), N)
    off[:9] = step(TRIG_LIMIT, np.arange(9))  # the limit itself and up to 8 ulps beyond
    off[9:18] = -off[:9]
    off[18::997] = np.inf
    off[19::997] = -np.inf
    off[20::997] = np.nan
    s["offpath_large"] = off
    return _freeze(s)


@functools.lru_cache(maxsize=None)
def trig_mixed():
    """{name: ((x,), is_fast)}: render_periods interleaved with offpath_large."""
    t = trig_sets()
    m = _mixed((t["render_periods"],), (t["offpath_large"],))
    for (x,), mask in m.values():
        x.setflags(write=False)
        mask.setflags(write=False)
    return m


# -------------------------------------------------------------------------- pow ----
@functools.lru_cache(maxsize=None)
def pow_sets():
    """{name: (x, y)} for rpow / opow."""
    r = _rng("pow")
    u = lambda: r.random(N)
    normal_bits = lambda: (r.integers(0, 1 << 52, N, dtype=np.uint64) |
                           (r.integers(1, 2047, N, dtype=np.uint64) << np.uint64(52)))
    s = {
        "render_controller_wide": (np.exp(u() * 1400.0 - 700.0), np.full(N, 0.2)),  # eps/err, 1e-304 .. 1e304
        "render_controller": (np.exp(u() * 30.0 - 20.0), np.full(N, 0.2)),
        "render_beaming": (u() * 4.0, np.floor(u() * 8.0) * 0.5),
        "render_near_one": (1.0 + (u() - 0.5) * 1e-6, (u() - 0.5) * 100.0),
        "render_random": (_from_bits(normal_bits()).copy(), (u() - 0.5) * 4.0),
        "render_companding": (np.exp(r.uniform(np.log(0.0031308), np.log(1e6), N)), np.full(N, 1.0 / 2.4)),
    }
    # |y| at pow_fast's limits 2^-65 and 2^63
    xs = np.array([0.5, 1.5, 2.0, 10.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 1e-300, 1e300, 1.0])
    s["edge_y_limits"] = (r.choice(xs, N), _edge_set(r, [2.0 ** -65, 2.0 ** 63], 8, 1 << 12))
    # |y log x| at 2^-54 and at 512: y0 = +-T / log x, then y0 +- 0..8 ulps, so that the
    # product the device forms lands within a couple of ulps of T on either side
    m = N // 17 + 1
    x = np.where(r.random(m) < 0.5, np.exp(r.uniform(-690.0, 690.0, m)), 1.0 + (r.random(m) - 0.5) * 1e-3)
    x = np.where(np.abs(np.log(x)) < 1e-12, 1.5, x)
    t = r.choice((2.0 ** -54, 512.0), m) * r.choice((-1.0, 1.0), m)
    y0 = t / np.log(x)
    s["edge_y_log_x"] = (np.repeat(x, 17)[:N].copy(), step(np.repeat(y0, 17), np.tile(np.arange(-8, 9), m))[:N].copy())
    # x at the log table's split in several binades, at each of the table's 128 interval
    # boundaries, at 1 and at the smallest and largest normal
    split = _from_bits([POW_LOG_SPLIT + (d << 52) for d in (-1000, -512, -100, -3, -2, -1, 0, 1, 2, 3, 100, 512, 1000)])
    bounds = _from_bits([POW_LOG_SPLIT + (j << 45) for j in range(128)])
    pts = np.concatenate([split, bounds, [1.0, 2.0 ** -1022, np.finfo(np.float64).max]])
    xe = _edge_set(r, pts, 8, 1 << 12)
    xe[xe.size // 2::3] = np.abs(xe[xe.size // 2::3])  # keep most of the fill positive (on the fast path)
    s["edge_x_table"] = (xe, r.choice(np.array([0.2, 1.5, 1.0 / 2.4, -3.7, 2.0, 0.5]), N))
    # everything pow_fast refuses, one case per lane in turn
    i = np.arange(N) % 12
    ys = r.choice(np.array([-3.0, -2.5, -1.0, 0.5, 2.0, 3.0]), N)
    pos = np.exp(r.uniform(-600.0, 600.0, N))
    pos = np.where(np.abs(np.log(pos)) < 1e-3, 3.0, pos)
    big = np.ldexp(1.0 + u(), r.integers(63, 1024, N)) * r.choice((-1.0, 1.0), N)
    big[5::24] = np.inf
    big[17::24] = -np.inf
    tiny = np.ldexp(1.0 + u(), r.integers(-1000, -66, N)) * r.choice((-1.0, 1.0), N)
    tiny[7::36] = 0.0
    x = np.select(
        [i == 0, i == 1, i == 2, i == 3, i == 4, i == 5, i == 6, i == 7, i == 8],
        [0.0, -0.0, -pos, -pos, _from_bits(r.integers(1, 1 << 52, N, dtype=np.uint64)),
         np.where(r.random(N) < 0.5, np.inf, -np.inf), np.nan, pos, 0.5 + 1.5 * u()], pos)
    y = np.select(
        [i == 2, i == 3, i == 4, i == 7, i == 8, i == 9, i == 10, i == 11],
        [r.integers(-5, 6, N).astype(np.float64), (u() - 0.5) * 9.0 + 0.01, (u() - 0.5) * 4.0, tiny, big,
         r.uniform(512.0, 800.0, N) / np.log(pos),     # finite up to 709.78, overflow beyond
         r.uniform(-800.0, -512.0, N) / np.log(pos),   # normal, subnormal (-708 .. -745) and zero results
         np.nan], ys)
    s["offpath_all"] = (x, y)
    return _freeze(s)


@functools.lru_cache(maxsize=None)
def pow_mixed():
    """{name: ((x, y), is_fast)}: render_controller_wide interleaved with offpath_all."""
    p = pow_sets()
    m = _mixed(p["render_controller_wide"], p["offpath_all"])
    for (x, y), mask in m.values():
        x.setflags(write=False)
        y.setflags(write=False)
        mask.setflags(write=False)
    return m


# -------------------------------------------------------------------------- exp ----
@functools.lru_cache(maxsize=None)
def exp_sets():
    """{name: x} for glibc::exp_ (defined for every input: no off-path or mixed sets)."""
    r = _rng("exp")
    u = lambda: r.random(N)
    q, d = u() * 4.0, u() * 12.0
    s = {
        "render_vertical_falloff": -(q * q),
        "render_boundary_falloff": -1.0 / np.maximum(d * d, 0.0001),
        "render_attenuation": -np.exp(u() * 60.0 - 50.0),
        "render_subnormal_and_overflow": np.where(np.arange(N) & 1, -745.5 + u() * 45.0, 700.0 + u() * 10.0),
        "render_random_bits": _from_bits(r.integers(0, 1 << 64, N, dtype=np.uint64)).copy(),
    }
    # exp_'s limits 2^-54, 512, 1024; ln of the smallest normal, of the smallest subnormal
    # and of half of it (results round to 0 below), and of the largest double
    pts = [2.0 ** -54, 512.0, 1024.0, 1022.0 * np.log(2.0), 1074.0 * np.log(2.0), 1075.0 * np.log(2.0),
           1024.0 * np.log(2.0)]
    s["edge_thresholds"] = _edge_set(r, pts, 8, 1 << 12)
    return _freeze(s)


SETS = {"pow": pow_sets, "trig": trig_sets, "exp": exp_sets}
MIXED = {"pow": pow_mixed, "trig": trig_mixed}
# render sets on which every lane takes the fast path (tests/test_glibc_math.py's modes)
ALL_FAST = {"pow": ("render_controller_wide", "render_controller"),
            "trig": tuple(k for k in ("render_ray_theta", "render_periods", "render_magnitudes", "render_near_half_pi",
                                      "render_reduction_limit", "render_disc_phi", "render_region_b")),
            "exp": ()}


def args_of(family, value):
    """(x, y or None) of a set's value."""
    return value if family == "pow" else (value, None)


def all_sets(family, mixed=True):
    """[(name, x, y or None)] of a family, the mixed sets included on request."""
    out = [(k, *args_of(family, v)) for k, v in SETS[family]().items()]
    if mixed and family in MIXED:
        out += [(k, *args_of(family, v if family == "pow" else v[0])) for k, (v, _) in MIXED[family]().items()]
    return out


# ------------------------------------------------------------- hooks and checks ----
def _outputs(n):
    return np.empty(n, np.float64), np.empty(n, np.float64), np.empty(n, np.uint8)


def _ptr(a):
    return None if a is None else a.ctypes.data


def run_host(lib, fn, x, y=None):
    """grt_debug_glibc_host: (out0, out1, path)."""
    import ctypes as C

    f = lib.grt_debug_glibc_host
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_uint64] + [C.c_void_p] * 5
    o0, o1, p = _outputs(x.size)
    rc = f(fn, x.size, _ptr(x), _ptr(y), _ptr(o0), _ptr(o1), _ptr(p))
    assert rc == 0, (rc, lib.grt_last_error())
    return o0, o1, p


def run_device(lib, device, unit, fn, threads, x, y=None):
    """grt_debug_glibc_device: (out0, out1, path)."""
    import ctypes as C

    f = lib.grt_debug_glibc_device
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 5
    o0, o1, p = _outputs(x.size)
    rc = f(device, unit, fn, threads, x.size, _ptr(x), _ptr(y), _ptr(o0), _ptr(o1), _ptr(p))
    assert rc == 0, (rc, lib.grt_last_error())
    return o0, o1, p


def same_bits(a, b):
    """Elementwise: the same bits, or both NaN."""
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def differing(x, y, got, want, where, k=5):
    """The first k lanes of `where` whose (out0, out1) differ, as hex-float text:
    (count, ["x=.. y=.. got=(..) want=(..)"])."""
    bad = np.nonzero(where & ~(same_bits(got[0], want[0]) & same_bits(got[1], want[1])))[0]
    rows = []
    for i in bad[:k]:
        yi = "" if y is None else f" y={float(y[i]).hex()}"
        rows.append(f"[{i}] x={float(x[i]).hex()}{yi} got=({float(got[0][i]).hex()}, {float(got[1][i]).hex()}) "
                    f"want=({float(want[0][i]).hex()}, {float(want[1][i]).hex()})")
    return bad.size, rows


def ulp_distance(a, b):
    """Distance in units of the last place between finite doubles of one sign (signed
    zeros coincide), exact in int64."""
    def order(v):
        i = np.ascontiguousarray(v).view(np.int64)
        return np.where(i < 0, -(i & np.int64(0x7fffffffffffffff)), i)
    return np.abs(order(a) - order(b))
