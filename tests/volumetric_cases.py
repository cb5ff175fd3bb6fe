"""Scenes, inputs and device calls of the VolumetricDisc unit checks.

Shared by tests/test_volumetric_checks_host.py (CPU: the oracle alone),
tests/test_gpu_volumetric_checks.py (the device beside the oracle) and
tools/volumetric_march_record.py (the measured record): one definition of every scene,
point set and job list, so the precondition checked on the CPU is the one the GPU test
relies on.  Everything is seeded; nothing here needs a GPU except device_points() and
device_march().
"""
import ctypes as C
import math

import numpy as np

from gr_raytracer_amd import _lib as L

TILT = (0.1, 0.2, 1.0)
ZAXIS = (0.0, 0.0, 1.0)
RS = 0.3  # Schwarzschild radius of the curved scenes: r_isco = 0.9 lies inside the first gas's rin = 1
FN_PERLIN, FN_DENSITY, FN_CHORD, FN_EXIT, FN_NO_MORE = range(5)
SEEDS = (0, 1, 42, 0xFFFFFFFF)
JOB_SIZES = (1, 63, 64, 65, 129, 300)
PROBES_VOL = (32, 64)  # the oracle's volumetric atan2 one ulp up / down


# ------------------------------------------------------------------------ scenes --
class BuiltScene:
    """What tests/test_gpu_parity.gpu_scene and test_gpu_volumetric.compare take."""

    def __init__(self, grt, builder):
        self.builder = builder
        self.desc = builder.build()
        self.adaptive = grt.default_adaptive()
        self.keep = []  # arrays the descriptor points to (attach_lut)

    def desc_ptr(self):
        return C.pointer(self.desc)


def _builder(grt, geometry):
    if geometry == L.GEOM_EUCLIDEAN:
        b = grt.SceneBuilder(L.GEOM_EUCLIDEAN)
        b.integration(2000, 100.0, 0.01, 1e-5)
        b.camera((0.0, 6.5, 0.0, 0.8), (1.0, 0.0, 0.0, 0.0), math.pi / 4, 48, 48)
    else:
        b = grt.SceneBuilder(L.GEOM_SCHWARZSCHILD, radius=RS, a=0.0, horizon_epsilon=1e-4)
        b.integration(20000, 100.0, 0.01, 1e-5)
        pos = grt.cartesian_to_spherical((0.0, -9.0, 0.0, 0.6))
        b.camera(pos, grt.stationary_velocity(L.GEOM_SCHWARZSCHILD, RS, 0.0, pos), math.pi / 4, 48, 48, 0.0, -3.142, 0.0)
    b.celestial(grt.Checker(0.0, 10.0, 10.0, (20, 20, 60), (0, 0, 0)))
    return b


GAS = dict(num_octaves=4, max_steps=500, step_size=0.01, thickness=0.5, density_multiplier=10.0, absorption=0.2,
           scattering=0.2, noise_scale=(1.0, 1.7, 2.3), noise_offset=0.1)


def flat_scene(grt, axis=TILT, seed=42):
    """Euclidean chart, constant temperature, one gas (rin 1, rout 3), checker texture."""
    b = _builder(grt, L.GEOM_EUCLIDEAN)
    b.add_volumetric_disc(1.0, 3.0, grt.Checker(3.0, 5.0, 5.0, (255, 60, 30), (40, 60, 255)), 1000.0,
                          constant_temperature=True, axis=axis, perlin_seed=seed,
                          brightness_reference_temperature=1000.0, **GAS)
    return BuiltScene(grt, b)


def attach_lut(grt, hs, k, temperature, n=1000):
    """Kerr temperature LUT of n entries (spin 0, radius RS) on object k of a built scene."""
    o = hs.desc.objects[k]
    lr, lt, ri = grt.kerr_temperature_lut(temperature, o.outer_radius, 0.0, RS, n)
    hs.keep += [lr, lt]
    o.temp_kind, o.r_isco, o.lut_n = L.TEMP_KERR_LUT, ri, n
    o.lut_r, o.lut_t = L.dptr(lr), L.dptr(lt)


def schw_scene(grt, axis=TILT, seed=42):
    """The same gas in Schwarzschild space with the Kerr temperature LUT and a blackbody texture."""
    b = _builder(grt, L.GEOM_SCHWARZSCHILD)
    b.add_volumetric_disc(1.0, 3.0, grt.BlackBody(1.0), 4000.0, axis=axis, perlin_seed=seed,
                          brightness_reference_temperature=2000.0, **GAS)
    return BuiltScene(grt, b)


def two_gas_scene(grt, geometry=L.GEOM_SCHWARZSCHILD, lut_n=(1000, 1000)):
    """Two gases with different seeds, axes, radii and steps, both with a temperature LUT of lut_n[k]
    entries: march_kernel stages the tables of the first gas with at most 1000 entries in LDS and reads
    the other's from global memory ((1500, 1000): object 1 is staged; (1500, 1500): neither is).  Object 1's rin = 0.8 lies below r_isco = 0.9: samples there fail the temperature."""
    b = _builder(grt, geometry)
    b.add_volumetric_disc(1.0, 3.0, grt.BlackBody(1.0), 4000.0, constant_temperature=True, axis=TILT, perlin_seed=42,
                          brightness_reference_temperature=2000.0, **GAS)
    g2 = dict(GAS, step_size=0.02, max_steps=300, thickness=0.4, noise_scale=(1.3, 0.9, 2.0), num_octaves=3)
    b.add_volumetric_disc(0.8, 2.5, grt.BlackBody(2.0), 5000.0, constant_temperature=True, axis=(0.3, -0.2, 1.0),
                          perlin_seed=7, brightness_reference_temperature=2500.0, **g2)
    hs = BuiltScene(grt, b)
    attach_lut(grt, hs, 0, 4000.0, lut_n[0])
    attach_lut(grt, hs, 1, 5000.0, lut_n[1])
    return hs


# ----------------------------------------------------------------- local frames --
def _unit(v):
    return v / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


class Frame:
    """VolumetricDisc::new's axis / e1 / e2 of object k, to place inputs (device and oracle each
    derive their own from the descriptor)."""

    def __init__(self, desc, k=0):
        o = desc.objects[k]
        ax = np.array(list(o.axis))
        self.ax = np.array([0.0, 0.0, 1.0]) if ax @ ax <= 2.220446049250313e-16 else _unit(ax)
        seed = np.array([0.0, 1.0, 0.0]) if abs(self.ax[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
        self.e1 = _unit(np.cross(seed, self.ax))
        self.e2 = _unit(np.cross(self.ax, self.e1))
        self.rin, self.rout, self.th = o.inner_radius, o.outer_radius, o.thickness
        self.cap = o.thickness * 3.0
        self.step, self.max_steps = o.march_step_size, int(o.march_max_steps)

    def world(self, x, y, h):
        x, y, h = (np.atleast_1d(np.asarray(v, np.float64)) for v in (x, y, h))
        return x[:, None] * self.e1 + y[:, None] * self.e2 + h[:, None] * self.ax

    def polar(self, r, phi, h):
        r, phi = np.atleast_1d(np.asarray(r, np.float64)), np.atleast_1d(np.asarray(phi, np.float64))
        return self.world(r * np.cos(phi), r * np.sin(phi), h)


def ulps(x, ks=(-2, -1, 0, 1, 2)):
    """x moved by k ulps for each k."""
    out = []
    for k in ks:
        v = np.float64(x)
        for _ in range(abs(k)):
            v = np.nextafter(v, np.inf if k > 0 else -np.inf)
        out.append(v)
    return np.array(out)


# ------------------------------------------------------------------------ Perlin --
def perlin_points():
    rng = np.random.default_rng(0x9E71)
    n = 1500
    parts = [rng.uniform(-50, 50, (12000, 3)), rng.integers(-300, 300, (n, 3)).astype(float)]
    near = rng.uniform(-40, 40, (2 * n, 3))  # 1 ulp either side of an integer, in each coordinate
    ints = rng.integers(-300, 300, 2 * n).astype(float)
    near[np.arange(2 * n), np.arange(2 * n) % 3] = np.nextafter(ints, np.where(np.arange(2 * n) % 2, np.inf, -np.inf))
    parts += [near, -rng.uniform(0, 300, (n, 3))]
    m = 256.0 * rng.integers(-4, 5, (n, 3)) + rng.choice((-1.0, -0.5, 0.0, 0.25, 1.0, 255.0, 255.75), (n, 3))
    parts.append(m)
    big = rng.uniform(-5, 5, (n, 3))
    vals = np.array([s * (2.0 ** e) + d for s in (1.0, -1.0) for e, ds in ((31, (0.0, 0.5, -0.5, 1.0, -1.0, 255.5)),
                                                                             (40, (0.5,)), (32, (0.0, -0.5)))
                     for d in ds])
    big[np.arange(n), np.arange(n) % 3] = vals[np.arange(n) % len(vals)]
    big[n // 2:, (np.arange(n - n // 2) + 1) % 3] = vals[(np.arange(n - n // 2) * 7) % len(vals)]
    parts.append(big)
    one = np.nextafter(1.0, 0.0)
    sp = [(-0.0, 0.3, 0.6), (0.3, -0.0, 0.6), (0.3, 0.6, -0.0), (-0.0, -0.0, -0.0), (0.0, 0.0, 0.0), (one, one, one),
          (one, 0.5, 0.5), (0.5, one, -one), (-one, -one, -one), (-0.0, one, 255.0 + one), (2.0 ** 40 + 0.5, -0.0, one)]
    parts.append(np.array(sp))
    return np.ascontiguousarray(np.concatenate(parts))


# ----------------------------------------------------------------------- density --
def _bisect(f, lo, hi):
    """The last double x in [lo, hi] with f(x) == f(lo) (f changes once between them)."""
    flo = f(lo)
    assert f(hi) != flo
    while True:
        mid = lo + (hi - lo) / 2
        if mid <= lo or mid >= hi:
            return lo
        if f(mid) == flo:
            lo = mid
        else:
            hi = mid


def density_points(oracle, desc, k=0):
    fr = Frame(desc, k)
    rng = np.random.default_rng(0xD15C + k)
    n = 16000
    parts = [fr.world(rng.uniform(-1.05, 1.05, n) * fr.rout, rng.uniform(-1.05, 1.05, n) * fr.rout,
                      rng.uniform(-1.1, 1.1, n) * fr.cap)]
    n = 2500  # inside the gas proper, where the noise is evaluated
    parts.append(fr.polar(rng.uniform(fr.rin, fr.rout, n), rng.uniform(-np.pi, np.pi, n), rng.normal(0, 0.5, n) * fr.th))
    # r at rin and rout, 1 ulp either side; d1 / d2 at the 0.0001 clamp (0.01 from an edge)
    edge = np.concatenate([ulps(fr.rin), ulps(fr.rout), ulps(fr.rin + 0.01), ulps(fr.rout - 0.01),
                           fr.rin + np.array([1e-9, 1e-6, 0.0099, 0.0101]), fr.rout - np.array([1e-9, 1e-6, 0.0099, 0.0101])])
    for h in (0.0, 0.3 * fr.th, -fr.th):
        # (r, 0, h), (0, r, h), (-r, 0, h) ... in world coordinates: with the z axis |p x axis| is r exactly
        for v in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            pts = np.zeros((len(edge), 3))
            pts[:, 0], pts[:, 1] = v[0] * edge, v[1] * edge
            parts.append(pts + h * fr.ax)
        parts.append(fr.polar(edge, rng.uniform(-np.pi, np.pi, len(edge)), h))
    # the height where exp(-(h / thickness)^2) crosses 0.001
    r0 = 0.5 * (fr.rin + fr.rout)
    probe = rng.uniform(-np.pi, np.pi, 64)
    cut = []
    for phi in probe:
        c, s = math.cos(phi), math.sin(phi)
        pos = lambda h: fr.world(r0 * c, r0 * s, h)[0]  # noqa: E731
        if oracle.vdisc_density(desc, k, pos(2.0 * fr.th)) > 0.0:
            hc = _bisect(lambda h: oracle.vdisc_density(desc, k, pos(h)) > 0.0, 2.0 * fr.th, 3.0 * fr.th)
            cut.append(np.concatenate([fr.world(r0 * c, r0 * s, sg * ulps(hc, (-3, -1, 0, 1, 2, 5))) for sg in (1, -1)]))
    assert len(cut) >= 8
    parts += cut
    hcut = fr.th * math.sqrt(-math.log(0.001))
    parts.append(fr.polar(rng.uniform(fr.rin, fr.rout, 400), rng.uniform(-np.pi, np.pi, 400),
                          rng.choice((-1, 1), 400) * (hcut + rng.choice((1e-15, 1e-12, 1e-9), 400) * rng.normal(0, 1, 400))))
    # on the axis (r = 0); y_local = +0 or tiny of either sign and x_local < 0 (phi = +-pi).  y_local is a sum
    # of three products, so a -0.0 coordinate gives +0.0: a true -0.0 is out of reach here as in production,
    # and phi = -pi comes from the tiny negative values only
    parts.append(fr.world(0.0, 0.0, np.array([0.0, -0.0, 0.1, -0.7, fr.cap])))
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-17, -1e-17])
    for xr in (-2.0, -1.5, -fr.rout + 0.3):
        parts.append(fr.world(np.full(len(tiny), xr), tiny, np.full(len(tiny), 0.1)))
    zx = np.zeros((len(tiny), 3))  # with the z axis: x_local = -p.y, y_local = p.x
    zx[:, 0], zx[:, 1], zx[:, 2] = tiny, 2.0, 0.1
    parts.append(zx)
    # where n + noise_offset changes sign: scan a mid-plane circle for a density that starts or stops
    phis = np.linspace(-3.0, 3.0, 1201)
    d = oracle.vdisc_density_n(desc, k, fr.polar(np.full(len(phis), r0), phis, 0.0))
    flips = np.nonzero((d[:-1] > 0.0) != (d[1:] > 0.0))[0]
    assert flips.size, "no sign change of n + noise_offset on the scanned circle"
    for i in flips[:6]:
        pc = _bisect(lambda p: oracle.vdisc_density(desc, k, fr.polar(r0, p, 0.0)[0]) > 0.0, phis[i], phis[i + 1])
        parts.append(fr.polar(np.full(7, r0), ulps(pc, (-3, -2, -1, 0, 1, 2, 3)), 0.0))
        parts.append(fr.polar(np.full(4, r0), pc + np.array([-1e-9, 1e-9, -1e-12, 1e-12]), 0.0))
    return np.ascontiguousarray(np.concatenate(parts))


# --------------------------------------------------------------------- crossings --
def segments(desc, k=0):
    """(from, to) pairs, (n, 6)."""
    fr = Frame(desc, k)
    rng = np.random.default_rng(0x5E65 + k)
    seg = []

    def add(a, b):
        a, b = np.atleast_2d(a), np.atleast_2d(b)
        seg.append(np.concatenate([a, np.broadcast_to(b, a.shape)], axis=1))

    def box(n, s=1.35):
        return fr.world(rng.uniform(-s, s, n) * fr.rout, rng.uniform(-s, s, n) * fr.rout, rng.uniform(-1.7, 1.7, n) * fr.cap)

    def interior(n):
        return fr.polar(rng.uniform(fr.rin, fr.rout, n) * 0.98 + 0.01, rng.uniform(-np.pi, np.pi, n),
                        rng.uniform(-0.9, 0.9, n) * fr.cap)

    n = 3000
    add(box(n), box(n))  # through and beside the region
    add(box(600), interior(600))  # one end inside
    a = box(400)  # parallel to the axis (a < 1e-10), and around that threshold
    add(a, a + rng.uniform(-4, 4, 400)[:, None] * fr.ax)
    a = box(300)
    tilt = rng.choice((0.3e-5, 0.9e-5, 1e-5, 1.1e-5, 3e-5), 300)
    add(a, a + 3.0 * fr.ax + (3.0 * tilt)[:, None] * fr.e1)
    a = box(400)  # perpendicular to it: no cap hit
    add(a, a + fr.world(rng.uniform(-5, 5, 400), rng.uniform(-5, 5, 400), 0.0))
    for R in (fr.rout, fr.rin):  # tangent to a cylinder: the discriminant at and around 0
        off = np.concatenate([ulps(R, (-4, -2, -1, 0, 1, 2, 4)), R + np.array([-1e-9, 1e-9, -1e-12, 1e-12, -1e-6, 1e-6])])
        for h in (0.0, 0.4 * fr.cap):
            add(fr.world(off, np.full(len(off), -4.0), h), fr.world(off, np.full(len(off), 4.0), h))
            add(fr.world(np.full(len(off), -3.5), off, h), fr.world(np.full(len(off), 4.5), off, -h))
    # starting exactly on each of the four surfaces, and ending there (the same pairs reversed)
    m = 150
    phi = np.concatenate([[0.0, np.pi / 2, np.pi, -np.pi / 2], rng.uniform(-np.pi, np.pi, m - 4)])
    on = [fr.polar(np.full(m, fr.rout), phi, rng.uniform(-0.9, 0.9, m) * fr.cap),
          fr.polar(np.full(m, fr.rin), phi, rng.uniform(-0.9, 0.9, m) * fr.cap),
          fr.polar(rng.uniform(fr.rin, fr.rout, m), phi, np.full(m, fr.cap)),
          fr.polar(rng.uniform(fr.rin, fr.rout, m), phi, np.full(m, -fr.cap))]
    for s in on:
        for other in (interior(m), box(m)):
            add(s, other)
            add(other, s)
    a = box(300)  # shorter than 1e-12, and around that length
    d = rng.normal(0, 1, (300, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    add(a, a + d * rng.choice((1e-13, 0.9e-12, 1e-12, 1.1e-12, 1e-11), 300)[:, None])
    a = interior(100)
    add(a, a + d[:100] * 1e-13)
    # through the hole: a cap is hit inside rin
    q = 200
    add(fr.polar(rng.uniform(0, fr.rin, q) * 0.95, rng.uniform(-np.pi, np.pi, q), rng.uniform(1.1, 1.6, q) * fr.cap),
        fr.polar(rng.uniform(0, fr.rin, q) * 0.95, rng.uniform(-np.pi, np.pi, q), -rng.uniform(1.1, 1.6, q) * fr.cap))
    # through a cap at exactly rin and rout; two equal crossings where a cap meets a cylinder
    for R in (fr.rin, fr.rout):
        for sg in (1.0, -1.0):
            for ph in (0.0, np.pi / 2, 0.7):
                c, s = math.cos(ph), math.sin(ph)
                for dr in (0.0, 0.5, -0.5, 0.25):
                    add(fr.world((R - dr) * c, (R - dr) * s, sg * (fr.cap + 0.5)), fr.world((R + dr) * c, (R + dr) * s, sg * (fr.cap - 0.5)))
    return np.ascontiguousarray(np.concatenate(seg))


def unit_rows(v):
    """nalgebra's normalize per row: v / sqrt(x x + y y + z z), the device's and the oracle's bits."""
    v = np.ascontiguousarray(v, np.float64)
    nrm = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return v / nrm[:, None]


def exit_rays(desc, k=0):
    """(ro, rd) pairs for the exit distance: the segments' starts and unit directions."""
    s = segments(desc, k)
    d = s[:, 3:] - s[:, :3]
    ok = np.linalg.norm(d, axis=1) > 1e-9
    return np.ascontiguousarray(np.concatenate([s[ok, :3], unit_rows(d[ok])], axis=1))


# --------------------------------------------------------------------- early end --
def early_end_pairs(desc, k=0):
    """(p, rd) pairs, (n, 6), around the vol_h_cut height and around rout."""
    fr = Frame(desc, k)
    rng = np.random.default_rng(0xEA71 + k)
    hcut = 2.62826 * fr.th * (1.0 + 1e-6)
    n = 1700
    small = lambda m: rng.choice((1e-8, 3e-9, 1e-9, 1e-10), m) * rng.uniform(-1, 1, m)  # noqa: E731
    wide = lambda m: rng.uniform(-0.3, 0.3, m)  # noqa: E731
    dh = np.where(rng.random(n) < 0.4, small(n), wide(n))
    p1 = fr.polar(rng.uniform(0, 1.2, n) * fr.rout, rng.uniform(-np.pi, np.pi, n), rng.choice((-1, 1), n) * (hcut + dh))
    dr = np.where(rng.random(n) < 0.4, small(n), wide(n))
    phi2 = rng.uniform(-np.pi, np.pi, n)
    p2 = fr.polar(fr.rout + dr, phi2, rng.uniform(-1.1, 1.1, n) * fr.cap)
    p3 = fr.polar(fr.rout + np.abs(wide(n)), rng.uniform(-np.pi, np.pi, n), rng.choice((-1, 1), n) * (hcut + np.abs(wide(n))))
    p = np.concatenate([p1, p2, p3])
    rd = rng.normal(0, 1, (3 * n, 3))
    # slopes along the axis / along the radius within 1e-14 of zero, on both sides
    tiny = rng.choice((0.0, 1e-16, -1e-16, 0.9e-15, -0.9e-15, 1.1e-15, -1.1e-15, 3e-15, -3e-15, 1e-14, -1e-14), 3 * n)
    flat = rng.random(3 * n) < 0.25
    ang = rng.uniform(-np.pi, np.pi, 3 * n)
    inplane = np.cos(ang)[:, None] * fr.e1 + np.sin(ang)[:, None] * fr.e2
    rd[flat] = inplane[flat] + tiny[flat, None] * fr.ax
    tang = np.zeros(3 * n, bool)
    tang[n:2 * n] = rng.random(n) < 0.25
    radial = np.cos(phi2)[:, None] * fr.e1 + np.sin(phi2)[:, None] * fr.e2
    tangent = -np.sin(phi2)[:, None] * fr.e1 + np.cos(phi2)[:, None] * fr.e2
    t2 = tangent + tiny[n:2 * n, None] * radial + rng.uniform(-0.5, 0.5, n)[:, None] * fr.ax
    rd[tang] = t2[tang[n:2 * n]]
    return np.ascontiguousarray(np.concatenate([p, unit_rows(rd)], axis=1))


# ------------------------------------------------------------------------- march --
def march_jobs(desc, objects=(0,), curved=True, seed=0):
    """300 jobs (object, ro, chord direction, frequency data); the lists of JOB_SIZES are its
    prefixes, so a job keeps its index in every list it is in.  With two objects the first
    130 jobs alternate between them and the rest come in runs of 37."""
    rng = np.random.default_rng(0x70B5 + seed)
    n = JOB_SIZES[-1]
    idx = np.arange(n)
    which = np.where(idx < 130, idx % len(objects), (idx // 37) % len(objects))
    obj = np.array(objects, np.uint32)[which]
    frames = {k: Frame(desc, k) for k in objects}
    ro, dr = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        fr = frames[int(obj[i])]
        phi, h = rng.uniform(-np.pi, np.pi), rng.uniform(-0.8, 0.8) * fr.cap
        rad = math.cos(phi) * fr.e1 + math.sin(phi) * fr.e2
        tan = -math.sin(phi) * fr.e1 + math.cos(phi) * fr.e2
        inner = fr.polar(rng.uniform(fr.rin + 0.1, fr.rout - 0.1), rng.uniform(-np.pi, np.pi), rng.uniform(-0.5, 0.5) * fr.th)[0]
        rmid = rng.uniform(fr.rin + 0.2, fr.rout - 0.2)
        sg = rng.choice((-1.0, 1.0))
        cat = i % 14
        if cat == 0:  # inside the gas (job 0: in every list)
            p, d = inner, rng.normal(0, 1, 3)
        elif cat == 1:  # on the outer cylinder, inward
            p, d = fr.polar(fr.rout, phi, h)[0], None
            d = inner - p
        elif cat == 2:  # on the outer cylinder, outward: the common production case
            p, d = fr.polar(fr.rout, phi, h)[0], rad + 0.5 * rng.normal(0, 1) * tan + 0.3 * rng.normal(0, 1) * fr.ax
        elif cat == 3:  # on a cap, inward
            p = fr.polar(rmid, phi, sg * fr.cap)[0]
            d = inner - p
        elif cat == 4:  # on a cap, outward
            p, d = fr.polar(rmid, phi, sg * fr.cap)[0], sg * fr.ax + 0.4 * rng.normal(0, 1) * rad + 0.4 * rng.normal(0, 1) * tan
        elif cat == 5:  # on the inner cylinder, into the gas
            p, d = fr.polar(fr.rin, phi, 0.3 * h)[0], rad + 0.3 * rng.normal(0, 1) * tan + 0.1 * rng.normal(0, 1) * fr.ax
        elif cat == 6:  # on the inner cylinder, into the hole (and out through the gas beyond it)
            p, d = fr.polar(fr.rin, phi, 0.3 * h)[0], -rad + 0.3 * rng.normal(0, 1) * tan + 0.05 * rng.normal(0, 1) * fr.ax
        elif cat == 7:  # grazing the outer cylinder
            p, d = fr.polar(fr.rout, phi, 0.2 * h)[0], tan - rng.choice((1e-3, 1e-2, 0.05)) * rad
        elif cat == 8:  # through the hole
            p, d = fr.polar(0.6 * fr.rin * rng.random(), phi, sg * fr.cap)[0], -sg * fr.ax + 0.05 * rng.normal(0, 1) * rad
        elif cat == 9:  # along the mid-plane
            p, d = fr.polar(fr.rout, phi, 0.0)[0], -rad + 0.2 * rng.normal(0, 1) * tan
        elif cat == 10:  # nearly parallel to the axis
            p, d = fr.polar(rmid, phi, -sg * fr.cap)[0], sg * fr.ax + 1e-6 * rad
        elif cat == 11:  # a chord longer than max_steps * step_size that stays in the gas: no cached exit, max_steps
            dmin = fr.rin + 0.2
            beta = math.asin(dmin / fr.rout)
            p, d = fr.polar(fr.rout, phi, 0.1 * fr.th)[0], -math.cos(beta) * rad + math.sin(beta) * tan
        elif cat == 12:  # outside, heading away: ends on its first sample
            p, d = fr.polar(fr.rout + 0.3, phi, sg * (fr.cap + 0.2))[0], rad + sg * fr.ax
        else:  # inside the gas near an edge
            p, d = fr.polar(rng.choice((fr.rin + 0.02, fr.rout - 0.02)), phi, 0.2 * h)[0], rng.normal(0, 1, 3)
        ro[i], dr[i] = p, np.asarray(d) * rng.uniform(0.01, 3.0)
    freq = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.8, 1.2, n),
                     rng.uniform(-0.3, 0.3, n) if curved else np.zeros(n)], axis=1)
    return obj, np.ascontiguousarray(ro), np.ascontiguousarray(dr), np.ascontiguousarray(freq)


def march_cases(grt):
    """(name, scene, jobs) of the raymarch checks, CPU precondition and GPU test alike."""
    flat, schw, two = flat_scene(grt), schw_scene(grt), two_gas_scene(grt)
    return [("flat", flat, march_jobs(flat.desc, curved=False)),
            ("schwarzschild", schw, march_jobs(schw.desc, seed=1)),
            ("two-gas", two, march_jobs(two.desc, objects=(0, 1), seed=2))]


def oracle_march(oracle, desc, jobs, probe=0):
    """oracle.vdisc_raymarch(cached=True) per job: colours (n, 4) -- (0, 0, 0, 0) where the
    temperature fails, as color_at_uv substitutes -- errors and sample counts."""
    obj, ro, dr, freq = jobs
    oracle.lib().oracle_set_libm_perturbation(probe)
    try:
        err, col, ns = oracle.vdisc_raymarch_n(desc, obj, ro, unit_rows(dr), freq, cached=True)
    finally:
        oracle.lib().oracle_set_libm_perturbation(0)
    col[err != 0] = 0.0
    return col, err, ns


def robust_jobs(oracle, desc, jobs, ref=None):
    """Jobs no volumetric atan2 probe moves by more than 1e-4 relative in any channel."""
    from test_gpu_parity import within

    ref = oracle_march(oracle, desc, jobs)[0] if ref is None else ref
    robust = np.ones(len(ref), bool)
    for mode in PROBES_VOL:
        robust &= within(oracle_march(oracle, desc, jobs, mode)[0], ref)
    return robust


# ------------------------------------------------------------------ device calls --
def _fn(name, argtypes):
    f = getattr(L.lib(), name)
    f.restype, f.argtypes = C.c_int, argtypes
    return f


def points_fn():
    return _fn("grt_debug_vdisc_points", [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.c_void_p])


def march_fn():
    return _fn("grt_debug_vdisc_march", [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p])


def device_points(sc, gpu, obj, fn, inp):
    """grt_debug_vdisc_points: out (n, 8), flag (n,) bool.  inp: (n, 3) or (n, 6)."""
    inp = np.asarray(inp, np.float64)
    n = len(inp)
    buf = np.zeros((n, 6))
    buf[:, :inp.shape[1]] = inp
    out, flag = np.zeros((n, 8)), np.zeros(n, np.uint8)
    rc = points_fn()(sc._s, gpu, obj, fn, n, buf.ctypes.data, out.ctypes.data, flag.ctypes.data)
    assert rc == 0, L.lib().grt_last_error()
    return out, flag.astype(bool)


def device_march(sc, gpu, jobs, n=None, blocks=8, arith=0, as_pool=False):
    """grt_debug_vdisc_march over the first n jobs: colours (n, 4), counters (jobs, samples, noise, emit)."""
    obj, ro, dr, freq = jobs
    n = len(obj) if n is None else n
    obj, ro, dr, freq = (np.ascontiguousarray(a[:n]) for a in (obj, ro, dr, freq))
    col, cnt = np.zeros((n, 4)), np.zeros(4, np.uint64)
    rc = march_fn()(sc._s, gpu, n, obj.ctypes.data, ro.ctypes.data, dr.ctypes.data, freq.ctypes.data, blocks, arith,
                    int(as_pool), col.ctypes.data, cnt.ctypes.data)
    assert rc == 0, L.lib().grt_last_error()
    return col, cnt


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    """Equal bits, a zero of either sign equal to a zero of either sign."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (bits(a) == bits(b)) | ((a == 0.0) & (b == 0.0))


# ------------------------------------------------------ measurements (test and record) --
FLOOR = 1e-6  # tests/test_gpu_parity.within's absolute floor


def ulp_distance(a, b):
    """Distance in units of the last place between two finite f64 arrays."""
    def key(x):
        u = bits(x).astype(np.int64)
        return np.where(u < 0, np.int64(-2 ** 63) - u, u)
    return np.abs(key(a) - key(b))


_libm = None


def glibc_sincos(phi):
    """glibc's sincos() per element: the entry point the reference's compiled code calls."""
    global _libm
    if _libm is None:
        _libm = C.CDLL("libm.so.6")
        _libm.sincos.restype, _libm.sincos.argtypes = None, [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    s, c = C.c_double(), C.c_double()
    out = np.zeros((len(phi), 2))
    for i, p in enumerate(phi):
        _libm.sincos(float(p), C.byref(s), C.byref(c))
        out[i] = s.value, c.value
    return out[:, 0], out[:, 1]


def density_check(oracle, desc, sc, gpu, pts, k=0):
    """Device density beside the oracle's with the device's phi: a dict of mismatch counts
    (all 0 when the device is right) and the atan2 ulp maximum against numpy.arctan2."""
    out, noise = device_points(sc, gpu, k, FN_DENSITY, pts)
    phi = out[:, 5]
    ref = oracle.vdisc_density_n(desc, k, pts, phi)
    x, y, want_noise = oracle.vdisc_plane_n(desc, k, pts)  # compute_density's own x_local, y_local and early returns
    m = noise & want_noise
    sp, cp = glibc_sincos(phi[m])
    return {"n": len(pts), "noise_points": int(noise.sum()), "positive": int((ref > 0).sum()),
            "density_mismatch": int((bits(out[:, 0]) != bits(ref)).sum()),
            "noise_flag_mismatch": int((noise != want_noise).sum()),
            "plane_xy_mismatch": int(((bits(out[m, 1]) != bits(x[m])) | (bits(out[m, 2]) != bits(y[m]))).sum()),
            "sincos_mismatch": int(((bits(out[m, 3]) != bits(sp)) | (bits(out[m, 4]) != bits(cp))).sum()),
            "atan2_max_ulp": int(ulp_distance(phi[m], np.arctan2(y[m], x[m])).max())}


def march_check(oracle, desc, sc, gpu, jobs, arith=0, n=None, blocks=8, as_pool=False, ref=None, robust=None):
    """The device's march of the first n jobs beside the oracle's: colours, counters, and the
    figures of the record (relative difference as tests/test_gpu_parity.within measures it)."""
    n = len(jobs[0]) if n is None else n
    if ref is None:
        ref_all, _, ns_all = oracle_march(oracle, desc, jobs)
        ref = (ref_all, ns_all)
    robust = robust_jobs(oracle, desc, jobs, ref[0]) if robust is None else robust
    col, cnt = device_march(sc, gpu, jobs, n, blocks, arith, as_pool)
    want, rb = ref[0][:n], robust[:n]
    rel = np.max(np.abs(col - want) / np.maximum(np.abs(want), FLOOR), axis=1)
    return {"col": col, "counters": cnt, "oracle_samples": int(ref[1][:n].sum()), "robust": rb,
            "max_rel_robust": float(np.max(rel[rb], initial=0.0)), "robust_share": float(rb.mean()),
            "bit_equal_share": float(np.all(bits(col) == bits(want), axis=1).mean())}
