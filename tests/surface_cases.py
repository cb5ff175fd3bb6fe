"""Scenes, input rows and device calls of the surface path's unit checks.

Shared by tests/test_surface_checks_host.py (CPU: the oracle alone),
tests/test_gpu_surface_checks.py (the device beside the oracle) and
tools/surface_points_record.py (the measured record): one definition of every scene and row
list, so the input conditions checked on the CPU are the ones the GPU test relies on.
Everything is seeded; nothing here needs a GPU except device_points().

A row list is a `Rows`: the (n, 8) input array and, per named family, the slice of its rows
("random" first), so a test can ask for a share of the random rows or for a hit and a miss
inside one edge family.
"""
import ctypes as C
import math
from pathlib import Path

import numpy as np

import volumetric_cases as V
from gr_raytracer_amd import _lib as L
from volumetric_cases import bits  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parents[1]
FN_DISC, FN_SPHERE, FN_FAR, FN_LUT, FN_TEMP, FN_BB, FN_TEX, FN_BLEND = range(8)
FN_COUNT = 8
NAN, INF = float("nan"), float("inf")

RIN, ROUT = 2.0, 6.0                 # the disc of every scene here
CENTRE, RADIUS = (0.75, -1.25, 2.5), 1.5  # the chord tests' sphere: dyadic, so local + centre - centre is exact
FAR_CENTRE, FAR_RADIUS = (5.0, -11.0, 4.8), 10.0  # the window scenes' sphere: its shell spans r = 3 .. 23
KERR_A = 0.4
FAR_CHARTS = {"schwarzschild": L.GEOM_SCHWARZSCHILD, "kerr_bl": L.GEOM_KERR_BL,
              "euclidean_spherical": L.GEOM_EUCLIDEAN_SPHERICAL}
FAR_SCENES = ("disc", "sphere", "disc+sphere", "disc+gas")
LONG_RATIOS = (1e9, 1e12, 1e16)
LUT_SIZES = (2, 3, 1000)  # 2: the smallest table validate_desc accepts


def near(x, ks=(-1, 0, 1)):
    """x and its neighbours in the last place."""
    return [float(v) for v in V.ulps(x, ks)]


def same_bits(a, b):
    """Equal bits; a NaN equals a NaN and a zero of either sign a zero of either sign."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (bits(a) == bits(b)) | ((a == 0.0) & (b == 0.0)) | (np.isnan(a) & np.isnan(b))


class Rows:
    def __init__(self):
        self._parts, self.family, self.mixed, self._n = [], {}, {}, 0

    def add(self, name, rows, mixed=False):
        """mixed: the reference allows a hit and a miss in this family, and both must occur."""
        rows = np.atleast_2d(np.asarray(rows, np.float64))
        buf = np.zeros((len(rows), 8))
        buf[:, :rows.shape[1]] = rows
        assert name not in self.family and len(rows)
        self.family[name] = slice(self._n, self._n + len(rows))
        self.mixed[name] = mixed
        self._parts.append(buf)
        self._n += len(rows)
        return self

    @property
    def x(self):
        return np.concatenate(self._parts)

    def __len__(self):
        return self._n


# ------------------------------------------------------------------------ scenes --
Built = V.BuiltScene


def _builder(grt, geometry):
    if geometry == L.GEOM_KERR_BL:
        b = grt.SceneBuilder(geometry, radius=1.0, a=KERR_A, horizon_epsilon=1e-4)
    elif geometry == L.GEOM_SCHWARZSCHILD:
        b = grt.SceneBuilder(geometry, radius=1.0, a=0.0, horizon_epsilon=1e-4)
    else:
        b = grt.SceneBuilder(geometry)
    b.integration(1000, 1e5, 0.01, 1e-5)
    # never traced: any valid camera
    b.d.camera = grt.build_camera(L.GEOM_EUCLIDEAN, 0.0, 0.0, (0.0, 9.0, 0.0, 0.6), (1.0, 0.0, 0.0, 0.0), 0.7, 8, 8)
    b.celestial(grt.Checker(0.0, 10.0, 10.0, (20, 20, 60), (0, 0, 0)))
    return b


_CHECK = dict(width=5.0, height=7.0, color1=(255, 60, 30), color2=(40, 60, 255))


def chord_scene(grt):
    """Euclidean: object 0 the disc (rin 2, rout 6), object 1 the sphere (radius 1.5 off the origin)."""
    b = _builder(grt, L.GEOM_EUCLIDEAN)
    b.add_disc(RIN, ROUT, grt.Checker(0.0, **_CHECK), 1000.0)
    b.add_sphere(RADIUS, CENTRE, grt.Checker(0.0, **_CHECK), 1000.0)
    return Built(grt, b)


def far_scene(grt, chart, kind):
    """A window-filter scene: `kind` of FAR_SCENES on chart `chart` of FAR_CHARTS (the gas is
    volumetric_cases' GAS about the z axis, rin 1, rout 3, so vol_far's slab test is live)."""
    b = _builder(grt, FAR_CHARTS[chart])
    tex = grt.Checker(0.0, **_CHECK)
    if "disc" in kind:
        b.add_disc(RIN, ROUT, tex, 1000.0, constant_temperature=True)
    if "sphere" in kind:
        b.add_sphere(FAR_RADIUS, FAR_CENTRE, tex, 1000.0)
    if "gas" in kind:
        b.add_volumetric_disc(1.0, 3.0, tex, 1000.0, constant_temperature=True, axis=V.ZAXIS, perlin_seed=42,
                              brightness_reference_temperature=1000.0, **V.GAS)
    return Built(grt, b)


def lut_scene(grt, lut_n):
    """Schwarzschild: object 0 a disc with a Kerr temperature table of lut_n entries, object 1 a
    disc of constant temperature; a blackbody texture, so the scene holds the stock (log10 T, XYZ)
    table of 1000 entries."""
    b = _builder(grt, L.GEOM_SCHWARZSCHILD)
    b.add_disc(3.0, 9.0, grt.BlackBody(0.0), 4000.0, constant_temperature=True)
    b.add_disc(3.0, 9.0, grt.Checker(0.0, **_CHECK), 1234.5, constant_temperature=True)
    hs = Built(grt, b)
    o = hs.desc.objects[0]
    lr, lt, ri = grt.kerr_temperature_lut(4000.0, o.outer_radius, 0.0, 1.0, lut_n)
    hs.keep += [lr, lt]
    o.temp_kind, o.r_isco, o.lut_n = L.TEMP_KERR_LUT, ri, lut_n
    o.lut_r, o.lut_t = L.dptr(lr), L.dptr(lt)
    hs.lut_r, hs.lut_t = lr, lt
    hs.bb_log_t = np.ctypeslib.as_array(hs.desc.bb_log_t, shape=(hs.desc.bb_n,)).copy()
    return hs


_celestial = None


def celestial_map(grt):
    """The stock celestial bitmap (tests/golden/resources/celestial.png) as an (H, W, 4) array."""
    global _celestial
    if _celestial is None:
        opts = grt.GlobalOpts(width=8, height=8, camera_position=(-16.0, 0.0, 3.5), theta=-3.142, max_steps=10)
        hs = grt.HostScene(str(ROOT / "tests/golden/scenes/schwarzschild.toml"), opts, str(ROOT / "tests/golden"))
        t = hs.desc.celestial
        assert t.kind == L.TEX_BITMAP
        _celestial = np.ctypeslib.as_array(t.rgba, shape=(t.height, t.width, 4)).copy()
        hs.close()
    return _celestial


TEX_OBJECTS = {"bitmap": -1, "checker": 0, "blackbody": 1}


def texture_scene(grt, beaming):
    """The celestial texture is the stock bitmap, object 0 carries a 5 x 7 checker and object 1 a
    blackbody texture, each with the beaming exponent `beaming` (TEX_OBJECTS)."""
    b = _builder(grt, L.GEOM_EUCLIDEAN)
    b.celestial(grt.Bitmap(beaming, celestial_map(grt)))
    b.add_sphere(1.0, (0.0, 0.0, 0.0), grt.Checker(beaming, **_CHECK), 1000.0)
    b.add_sphere(1.0, (0.0, 0.0, 3.0), grt.BlackBody(beaming), 1000.0)
    return Built(grt, b)


# -------------------------------------------------------------------- disc rows --
_IN = (3.0, 0.5, 3.5, 1.0)    # (sx, sy, ex, ey) of a segment over the annulus
_OUT = (7.0, 7.0, 7.5, 7.25)  # and of one beside it


def _seg(xy, sz, ez):
    return [xy[0], xy[1], sz, xy[2], xy[3], ez]


def disc_rows():
    rng = np.random.default_rng(11)
    R = Rows()
    n = 6000
    rho, ang = 8.0 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * math.pi, n)
    p = np.stack([rho * np.cos(ang), rho * np.sin(ang), np.zeros(n)], 1)
    d = rng.normal(size=(n, 3)) * rng.uniform(0.05, 3.0, (n, 1))
    t0 = rng.uniform(-0.3, 1.3, (n, 1))
    s = p - t0 * d
    R.add("random", np.hstack([s, s + d]))
    mags = [0.0, 5e-324, 1e-250] + near(1e-200) + [1.0]
    sz = [v for m in mags for v in (m, -m)]
    dz = [v for m in [1e-300] + near(1e100) + [1e300, 1.0, 4.0, 1e99] for v in (m, -m)]
    R.add("s.z x dz", [_seg(xy, a, a + b) for xy in (_IN, _OUT) for a in sz for b in dz], mixed=True)
    R.add("t = 0", [_seg(xy, a, b) for xy in (_IN, _OUT) for a in (0.0, -0.0) for b in (1.0, -1.0, 5e-324, -1e300)], mixed=True)
    R.add("t = 1", [_seg(xy, a, b) for xy in (_IN, _OUT) for b in (0.0, -0.0) for a in (1.0, -1.0, 5e-324, -1e300)], mixed=True)
    R.add("p2 = 0", [_seg(xy, a, a) for xy in (_IN, _OUT) for a in (0.0, -0.0, 1.0, -1e-250, 1e300)])
    # |p1| = 2 |p2| and its neighbours: t = +-2 (a miss), and |p1| = |p2| / 2 beside them (t = 1/2)
    R.add("|p1| = 2 |p2|", [_seg(_IN, a, a - sg * b) for a in near(2.0) + near(-2.0) for b in near(1.0) for sg in (1.0, -1.0)])
    R.add("|p1| = |p2| / 2", [_seg(_IN, a, a - sg * 2.0 * abs(a)) for a in near(0.5) + near(-0.5) for sg in (1.0, -1.0)], mixed=True)
    R.add("rim", [[r, 0.0, 1.0, r, 0.0, -1.0] for c in (RIN, ROUT) for r in near(c, (-2, -1, 0, 1, 2))], mixed=True)
    base = np.array(_seg(_IN, 1.0, -1.0))
    bad = []
    for k in range(6):
        for v in (NAN, INF, -INF):
            row = base.copy()
            row[k] = v
            bad.append(row)
    R.add("non-finite", bad)
    return R


# ------------------------------------------------------------------ sphere rows --
def _surface_points():
    pts = []
    for perm in ((0.5, 1.0, 1.0), (1.0, 0.5, 1.0), (1.0, 1.0, 0.5)):  # 1/4 + 1 + 1 = 9/4 exactly
        for sx in (1, -1):
            for sy in (1, -1):
                for sz in (1, -1):
                    pts.append((sx * perm[0], sy * perm[1], sz * perm[2]))
    for k in range(3):
        for sg in (1.5, -1.5):
            p = [0.0, 0.0, 0.0]
            p[k] = sg
            pts.append(tuple(p))
    return np.array(pts)


def sphere_rows():
    rng = np.random.default_rng(12)
    R = Rows()
    c = np.array(CENTRE)
    n = 6000

    def ball(k, rmax):
        v = rng.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.0, rmax, (k, 1))

    R.add("random", np.hstack([ball(n, 3.0) + c, ball(n, 3.0) + c]))
    sp = _surface_points()  # local points with |p|^2 == R^2 exactly
    assert np.all(np.sum(sp * sp, 1) == RADIUS * RADIUS) and np.all((sp + c) - c == sp)
    k = len(sp)
    inside, outside = ball(k, 1.0), sp * 1.75
    on = [np.hstack([sp + c, inside + c]), np.hstack([inside + c, sp + c]), np.hstack([sp + c, outside + c]),
          np.hstack([outside + c, sp + c])]
    R.add("end on the surface", np.vstack(on), mixed=False)
    # both roots in [0, 1]: a chord between two surface points, and one from a surface point through
    # the ball to a point outside
    j = rng.permutation(k)
    keep = np.any(sp != sp[j], axis=1)
    through = -1.5 * sp  # beyond the antipode
    R.add("two roots", np.vstack([np.hstack([sp[keep] + c, sp[j][keep] + c]), np.hstack([sp + c, through + c])]))
    # tangents at the axis points p: d orthogonal to p, so b = 0 exactly
    tan = []
    for p in sp[-6:]:
        axis = int(np.argmax(np.abs(p)))
        for q in range(3):
            if q == axis:
                continue
            for scale in (1.0, 1e-8, 1e8, -0.25):
                d = np.zeros(3)
                d[q] = scale
                tan.append(np.hstack([p + c, p + d + c]))           # from the tangent point outwards: t = 0
                tan.append(np.hstack([p - d + c, p + d + c]))       # symmetric about it: both ends outside
                tan.append(np.hstack([p + c, p * (1 - 2.0 ** -40) + d + c]))  # just inside the tangent
                tan.append(np.hstack([p + c, p * (1 + 2.0 ** -40) + d + c]))  # just outside it
    R.add("tangent", tan, mixed=True)
    zero = [np.hstack([q + c, q + c]) for q in (sp[0], sp[-1], np.zeros(3), np.array([0.1, 0.2, 0.3]), np.array([3.0, 0.0, 0.0]))]
    R.add("zero length", zero)
    far = sp[:8] * 2.0
    R.add("centre", np.vstack([np.hstack([np.tile(c, (8, 1)), far + c]), np.hstack([far + c, np.tile(c, (8, 1))]),
                               np.hstack([np.tile(c, (4, 1)), sp[:4] * 0.5 + c])]), mixed=True)
    base = np.hstack([np.array([0.1, 0.2, 0.3]) + c, np.array([2.0, 1.0, 0.5]) + c])
    bad = []
    for q in range(6):
        for v in (NAN, INF, -INF):
            row = base.copy()
            row[q] = v
            bad.append(row)
    R.add("non-finite", bad)
    return R


def world_point(local, centre=CENTRE):
    """window_pass's wx = pt[0] + o.cx, ..."""
    return np.stack([local[:, 0] + centre[0], local[:, 1] + centre[1], local[:, 2] + centre[2]], 1)


# ----------------------------------------------------------------- window rows --
def to_chart(geometry, a, xyz):
    """Native-chart (r, theta, phi) of Cartesian points: to place rows only (no bit of a check rests on it)."""
    x, y, z = (np.asarray(xyz, np.float64)[:, k] for k in range(3))
    rho2 = x * x + y * y + z * z
    if geometry == L.GEOM_KERR_BL:
        d = rho2 - a * a
        r = np.sqrt(0.5 * (d + np.sqrt(d * d + 4.0 * a * a * z * z)))
        return np.stack([r, np.arccos(np.clip(z / r, -1.0, 1.0)), np.arctan2(r * y - a * x, r * x + a * y)], 1)
    r = np.sqrt(rho2)
    return np.stack([r, np.arccos(z / r), np.arctan2(y, x)], 1)


def shell_bounds(centre=FAR_CENTRE, radius=FAR_RADIUS):
    """shell_lo, shell_hi as api.hip derives them."""
    cn = math.sqrt(centre[0] * centre[0] + centre[1] * centre[1] + centre[2] * centre[2])
    return (cn - radius) * (1.0 - 1e-9) - 1e-9, (cn + radius) * (1.0 + 1e-9) + 1e-9


def gas_bounds():
    """vol_far_r, vol_slab_h of far_scene's gas as api.hip derives them."""
    cap = V.GAS["thickness"] * 3.0
    return 2.0 * math.sqrt(3.0 * 3.0 + cap * cap) * (1.0 + 1e-6), cap * (1.0 + 1e-6) + 1e-12


HALF_PI = math.pi / 2


def far_rows(chart):
    """State pairs (ra, ta, pa, rb, tb, pb) for every scene of FAR_SCENES on `chart`."""
    g = FAR_CHARTS[chart]
    a = KERR_A if g == L.GEOM_KERR_BL else 0.0
    rng = np.random.default_rng(13 + g)
    R = Rows()
    n = 8000

    def states(k):
        return np.stack([10.0 ** rng.uniform(-3, 4, k), rng.uniform(-math.pi, 2 * math.pi, k), rng.uniform(-7.0, 7.0, k)], 1)

    ya = states(n)
    yb = states(n)
    half = n // 2  # the second half: short windows, as an accepted step makes them
    yb[half:, 0] = ya[half:, 0] * np.exp(rng.normal(0.0, 0.15, n - half))
    yb[half:, 1] = ya[half:, 1] + rng.normal(0.0, 0.08, n - half)
    yb[half:, 2] = ya[half:, 2] + rng.normal(0.0, 0.08, n - half)
    R.add("random", np.hstack([ya, yb]))
    # windows near the objects (Cartesian ends within a few units of them), where the refused rows hit
    k = 3000
    p = np.stack([rng.uniform(-8, 8, k), rng.uniform(-14, 8, k), rng.uniform(-3, 8, k)], 1)
    q = p + rng.normal(0.0, 1.5, (k, 3))
    R.add("near the objects", np.hstack([to_chart(g, a, p), to_chart(g, a, q)]))
    p = np.stack([rng.uniform(-4, 4, k), rng.uniform(-4, 4, k), rng.uniform(-2.5, 2.5, k)], 1)
    q = p + rng.normal(0.0, 0.6, (k, 3))
    R.add("near the gas", np.hstack([to_chart(g, a, p), to_chart(g, a, q)]))
    # theta at the zeros of cos +- the margin
    th = [c + s * dlt for c in (HALF_PI, -HALF_PI, 3 * HALF_PI) for dlt in (0.5e-9, 1e-9, 2e-9) for s in (1.0, -1.0)]
    th += [HALF_PI, -HALF_PI, 3 * HALF_PI]
    edge = []
    for t in th:
        for other in (t, 0.3, 2.5, HALF_PI - 0.5e-9, HALF_PI + 0.5e-9):
            for rb in (4.0, 4.5):
                edge.append([4.0, t, 0.2, rb, other, 0.25])
                edge.append([4.0, other, 0.2, rb, t, 0.25])
    R.add("theta margins", edge)
    ratio = []
    for f in (0.9e-3, 1e-3, 1.1e-3):
        for r in (4.0, 4000.0, 1.0):
            for t in (0.3, 2.5):
                ratio.append([r * f, t, 0.2, r, t, 0.2])
                ratio.append([r, t, 0.2, r * f, t, 0.2])
    for r in (0.0, -0.0, -1.0, -4.0):
        ratio += [[r, 0.3, 0.2, 4.0, 0.3, 0.2], [4.0, 0.3, 0.2, r, 0.3, 0.2], [r, 0.3, 0.2, r, 0.3, 0.2]]
    R.add("radius ratio", ratio)
    # the long windows the ratio test exists for: z_b - z_a rounds to -z_a, the reference's t is exactly 1
    for ratio_k in LONG_RATIOS:
        R.add("long %g" % ratio_k, [[ratio_k * ROUT, 0.1, ph, rb, HALF_PI - 2e-9, ph] for rb in (2.5, 3.0, 4.0, 5.0)
                                    for ph in (0.0, 1.0)])
    lo, hi = shell_bounds()
    rs = near(lo) + near(hi) + near(lo - a) + [lo - 2 * a, 0.5 * lo, 2.0 * hi]
    cth, cph = to_chart(g, a, [FAR_CENTRE])[0, 1:]
    R.add("shell", [[ra, cth, cph, rb, cth + dt, cph] for ra in rs for rb in rs for dt in (0.0, 0.01)])
    # one end beyond shell_hi, the other below shell_lo, along the centre's direction and beside it
    R.add("across the shell", [[f * hi, cth + dt, cph, g2 * (lo - a), cth, cph + dp] for f in (1.001, 2.0, 50.0)
                               for g2 in (0.999, 0.5, 0.01) for dt in (0.0, 0.3) for dp in (0.0, 3.0)])
    # just inside the sphere along the centre's direction (KerrBL: r < shell_lo <= r + |a| there) to far outside
    c_hat = np.array(FAR_CENTRE) / np.linalg.norm(FAR_CENTRE)
    inner = to_chart(g, a, [c_hat * (lo + e) for e in (0.002, 0.005, 0.01, 0.02)])
    R.add("inner shell edge", [[*y, 30.0, t2, cph] for y in inner for t2 in (cth, 0.3)]
          + [[30.0, t2, cph, *y] for y in inner for t2 in (cth, 0.3)])
    vfr, slab = gas_bounds()
    gas = []
    for r in near(vfr) + [vfr * (1 + 1e-9), vfr * (1 - 1e-9)]:
        gas += [[r, 0.4, 0.2, r, 0.4, 0.2], [r, 2.0, 0.2, r, 2.0, 0.2], [r, HALF_PI, 0.2, r, HALF_PI, 0.2]]
    for r in near(vfr + 1.0 * (1.0 + 1e-9)) + [vfr + 1.0 + 1e-6, vfr + 1.0 - 1e-6]:  # L = |rb - ra| = 1
        gas += [[r, 0.4, 0.2, r + 1.0, 0.4, 0.2], [r + 1.0, 2.0, 0.2, r, 2.0, 0.2]]
    for t in (0.5, 1.2, math.pi - 0.5, 4.0):  # the slab height on either hemisphere
        x = HALF_PI - abs(t if t < HALF_PI else t - math.pi)
        r0 = slab / (0.63661977236758134 * x)
        for f in (1.0 - 1e-8, 1.0, 1.0 + 1e-9, 1.0 + 2e-9, 1.0 + 1e-8, 1.05, 0.95):
            gas += [[r0 * f, t, 0.2, r0 * f, t, 0.7], [r0 * f, t, 0.2, r0 * 0.9, t, 0.2], [r0 * 1.1, t, 0.2, r0 * f, t, 0.2],
                    [r0 * f, t, 0.2, r0 * 0.5, t, 0.2]]  # the last one enters the capture region
    R.add("gas bounds", gas)
    assert len(R) <= 20000
    return R


def far_objects(desc):
    return [(k, desc.objects[k].kind) for k in range(desc.n_objects)]


def oracle_window_hits(oracle, desc, rows):
    """Per row: whether the reference's chord test of any object of the scene hits the window."""
    ca, cb = oracle.to_cartesian_n(desc, rows[:, 0:3]), oracle.to_cartesian_n(desc, rows[:, 3:6])
    hit = np.zeros(len(rows), bool)
    for k, kind in far_objects(desc):
        if kind == L.OBJ_VOLUMETRIC_DISC:
            hit |= oracle.vdisc_intersects_n(desc, k, ca, cb)[0]
        else:
            hit |= oracle.object_intersects_n(desc, k, ca, cb)[0]
    return hit


# ------------------------------------------------------------------- table rows --
def table_rows(a):
    """x over a sorted table: every node with its neighbours in the last place, every midpoint,
    and the interiors of the first and the last cell."""
    a = np.asarray(a, np.float64)
    rng = np.random.default_rng(14)
    x = [np.nextafter(a, -np.inf), a, np.nextafter(a, np.inf), 0.5 * (a[:-1] + a[1:]),
         rng.uniform(a[0], a[1], 60), rng.uniform(a[-2], a[-1], 60)]
    return np.concatenate(x)


def lut_index_rows(a):
    x = table_rows(a)
    return x[(a[0] < x) & (x < a[-1])]  # lut_index's contract


def lut_index_reference(a, x):
    return np.clip(np.searchsorted(a, x, "right") - 1, 0, len(a) - 2)


def temperature_rows(hs):
    lr, ri = hs.lut_r, hs.desc.objects[0].r_isco
    extra = near(ri, (-2, -1, 0, 1, 2)) + near(lr[0]) + near(lr[-1]) + [NAN, INF, -INF, 0.0, -0.0, -3.0, 1e300, 0.5 * ri]
    return np.concatenate([table_rows(lr), extra])


def blackbody_rows(bb_log_t=None):
    rng = np.random.default_rng(15)
    x = [10.0 ** rng.uniform(0, 9, 4000), [NAN, INF, -INF, 0.0, -5.0] + near(10.0)]
    if bb_log_t is not None:  # the ends of the table
        x.append([v for e in (bb_log_t[0], bb_log_t[-1]) for v in near(10.0 ** e, (-2, -1, 0, 1, 2))])
    return np.concatenate(x)


# ----------------------------------------------------------------- texture rows --
BAD_REDSHIFTS = (0.0, -1.0, NAN, INF)


def texture_rows(kind, width=2048, height=2048):
    """(u, v, redshift, temperature) for a texture of TEX_OBJECTS."""
    rng = np.random.default_rng(16)
    R = Rows()
    n = 6000

    def zt(k):
        return np.stack([10.0 ** rng.uniform(-3, 3, k), 10.0 ** rng.uniform(2.5, 4.5, k)], 1)

    R.add("random", np.hstack([rng.uniform(-0.5, 1.5, (n, 2)), zt(n)]))
    if kind == "bitmap":
        ks = np.unique(np.concatenate([[0, 1, 2, width // 2, width - 2, width - 1, width], rng.integers(0, width + 1, 300)]))
        us = np.concatenate([np.nextafter(ks / width, -np.inf), ks / width, np.nextafter(ks / width, np.inf)])
        ks = np.unique(np.concatenate([[0, 1, 2, height // 2, height - 2, height - 1, height], rng.integers(0, height + 1, 300)]))
        vs = np.concatenate([np.nextafter(ks / height, -np.inf), ks / height, np.nextafter(ks / height, np.inf)])
    else:
        cells = np.arange(0, 8)
        us = np.concatenate([np.nextafter(cells / 5.0, -np.inf), cells / 5.0, np.nextafter(cells / 5.0, np.inf)])
        vs = np.concatenate([np.nextafter(cells / 7.0, -np.inf), cells / 7.0, np.nextafter(cells / 7.0, np.inf)])
    m = max(len(us), len(vs))
    R.add("texel edges u", np.hstack([us[:, None], rng.uniform(0, 1, (len(us), 1)), zt(len(us))]))
    R.add("texel edges v", np.hstack([rng.uniform(0, 1, (len(vs), 1)), vs[:, None], zt(len(vs))]))
    R.add("texel edges u, v", np.hstack([np.resize(us, m)[:, None], np.resize(rng.permutation(vs), m)[:, None], zt(m)]))
    special = [0.0, -0.0, 1.0, NAN, INF, -INF, 1e30, -1e30, 5e-324, -1e-300, 0.999999, 4294967296.0]
    R.add("special u, v", [[u, v, 0.8, 3000.0] for u in special for v in special + [0.37] if not (u > 1e18 and v > 1e18)] +
          [[0.37, v, 1.3, 5000.0] for v in special])
    # beyond 2^64 cells on one axis only: the checker's sum does not wrap
    R.add("one axis saturates", [[u, v, 0.8, 3000.0] for u in (1e30, INF, 4e18, 1.9e19 / 5.0) for v in (0.0, 0.05, 0.1)] +
          [[u, v, 0.8, 3000.0] for v in (1e30, INF, 3e18) for u in (0.0, 0.05, 0.15)])
    R.add("bad redshift", [[u, v, z, t] for z in BAD_REDSHIFTS for u, v in ((0.3, 0.6), (0.61, 0.2)) for t in (3000.0, 20000.0)])
    # (a subnormal redshift, or one whose power over- or underflows, is outside glibc::pow_fast by design:
    # rpow's OCML arm, like the bad redshifts above; a render's redshift is nowhere near)
    R.add("redshift range", [[0.3, 0.6, z, 3000.0] for z in near(1e-3) + near(1e3) + near(1.0, (-1, 1))])
    R.add("redshift 1", [[u, v, 1.0, t] for u, v in ((0.3, 0.6), (0.61, 0.2), (0.999, 0.001), (1.2, -0.3)) for t in (3000.0, 20000.0)])
    assert len(R) <= 20000
    return R


# -------------------------------------------------------------------- blend rows --
def blend_rows():
    rng = np.random.default_rng(17)
    R = Rows()
    n = 4000
    col = rng.uniform(0.0, 2.0, (n, 8))
    col[:, 3], col[:, 7] = rng.uniform(-0.5, 1.5, n), rng.uniform(-0.5, 1.5, n)
    R.add("random", col)
    alphas = [0.0, -0.0, 1.0, -0.25, 1.5, NAN, INF, -INF, 5e-324, 0.5] + near(1.0, (-1, 1))
    R.add("alpha", [[0.3, 0.9, 0.2, a, 1.1, 0.4, 0.7, b] for a in alphas for b in alphas])
    R.add("both transparent", [[0.3, 0.9, 0.2, a, 1.1, 0.4, 0.7, b] for a in (0.0, -0.0, -1.0, -INF) for b in (0.0, -0.0, -0.5)])
    bad = []
    for k in (0, 1, 2, 4, 5, 6):
        for v in (NAN, INF):
            for a, b in ((0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)):
                row = [0.3, 0.9, 0.2, a, 1.1, 0.4, 0.7, b]
                row[k] = v
                bad.append(row)
    R.add("non-finite colour", bad)
    return R


# ------------------------------------------------------------------ device calls --
def points_fn():
    return V._fn("grt_debug_surface_points", [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                                              C.c_void_p])


def device_points(sc, gpu, obj, fn, inp):
    """grt_debug_surface_points: out (n, 8), flag (n,) bool.  inp: (n,) or (n, k), k <= 8."""
    inp = np.asarray(inp, np.float64)
    inp = inp[:, None] if inp.ndim == 1 else inp
    n = len(inp)
    buf = np.zeros((n, 8))
    buf[:, :inp.shape[1]] = inp
    out, flag = np.full((n, 8), np.nan), np.full(n, 7, np.uint8)
    rc = points_fn()(sc._s, gpu, obj, fn, n, buf.ctypes.data, out.ctypes.data, flag.ctypes.data)
    assert rc == 0, L.lib().grt_last_error()
    assert np.all(flag <= 1)
    return out, flag.astype(bool)


# ------------------------------------------------------ measurements (test and record) --
def chord_check(oracle, desc, sc, gpu, obj, fn, R):
    """A chord test beside the oracle: mismatch counts (0 when the device is right) and the hit share."""
    x = R.x
    out, hit = device_points(sc, gpu, obj, fn, x[:, :6])
    want, t, pt = oracle.object_intersects_n(desc, obj, x[:, 0:3], x[:, 3:6])
    got_pt = world_point(out[:, 1:4]) if fn == FN_SPHERE else out[:, 1:4]
    both = hit & want
    bad_bits = (bits(out[both, 0]) != bits(t[both])) | np.any(bits(got_pt[both]) != bits(pt[both]), axis=1)
    return {"rows": len(x), "hit_mismatch": int((hit != want).sum()), "bits_mismatch": int(bad_bits.sum()),
            "first_bad": x[np.nonzero(hit != want)[0][:3]].tolist() + x[both][bad_bits][:3].tolist(),
            "random_hit_share": float(want[R.family["random"]].mean()), "hits": int(want.sum())}


def far_check(oracle, desc, sc, gpu, R):
    x = R.x
    _, far = device_points(sc, gpu, -1, FN_FAR, x[:, :6])
    hit = oracle_window_hits(oracle, desc, x)
    rnd = R.family["random"]
    m = {"rows": len(x), "far_but_hit": int((far & hit).sum()), "first_bad": x[far & hit][:3].tolist(),
         "random_far_share": float(far[rnd].mean()), "far_share": float(far.mean()),
         "refused": int((~far).sum()), "refused_hits": int((~far & hit).sum()),
         "refused_but_missing_share": float((~far & ~hit).sum() / max(1, (~far).sum()))}
    for k in LONG_RATIOS:
        s = R.family["long %g" % k]
        m["long %g" % k] = {"oracle_hits": int(hit[s].sum()), "device_far_on_hits": int((far[s] & hit[s]).sum())}
    return m, far, hit


def table_check(hs, sc, gpu, obj):
    a = hs.bb_log_t if obj < 0 else hs.lut_r
    x = lut_index_rows(a)
    out, _ = device_points(sc, gpu, obj, FN_LUT, x)
    bad = out[:, 0] != lut_index_reference(a, x)
    return {"rows": len(x), "mismatch": int(bad.sum()), "first_bad": x[bad][:3].tolist()}


def temperature_check(oracle, desc, sc, gpu, obj, radii):
    out, _ = device_points(sc, gpu, obj, FN_TEMP, radii)
    status, val = oracle.compute_temperature_n(desc, obj, radii)
    ok = status == 0
    bad_s = out[:, 0] != status
    bad_v = ok & ~bad_s & (bits(out[:, 1]) != bits(val))
    return {"rows": len(radii), "ok_rows": int(ok.sum()), "status_mismatch": int(bad_s.sum()),
            "value_mismatch": int(bad_v.sum()), "first_bad": radii[bad_s | bad_v][:3].tolist(),
            "statuses": sorted(set(status.tolist()))}


_libm = None


def glibc_log10(x):
    global _libm
    if _libm is None:
        _libm = C.CDLL("libm.so.6")
        _libm.log10.restype, _libm.log10.argtypes = C.c_double, [C.c_double]
    return np.array([_libm.log10(float(v)) for v in x])


def log10_stats(temperature, dev_log_t):
    """The device's log10(fmax(T, 10)) beside glibc's: rows that differ, the largest distance in ulp."""
    want = glibc_log10(np.fmax(temperature, 10.0))
    fin = np.isfinite(want) & np.isfinite(dev_log_t)
    d = V.ulp_distance(dev_log_t[fin], want[fin])
    return {"log10_rows_differing": int((d != 0).sum()) + int((~same_bits(dev_log_t[~fin], want[~fin])).sum()),
            "log10_max_ulp": int(d.max(initial=0))}


def blackbody_check(oracle, desc, sc, gpu, temps):
    out, _ = device_points(sc, gpu, -1, FN_BB, temps)
    ref = oracle.blackbody_n(desc, temps, out[:, 4])
    bad = np.any(bits(out[:, :4]) != bits(ref), axis=1)
    m = {"rows": len(temps), "mismatch": int(bad.sum()), "first_bad": temps[bad][:3].tolist(),
         "bits_equal_with_glibc_log10": int(np.all(bits(out[:, :4]) == bits(oracle.blackbody_n(desc, temps)), axis=1).sum())}
    m.update(log10_stats(temps, out[:, 4]))
    return m


def texture_check(oracle, desc, sc, gpu, kind, R):
    x = R.x[:, :4]
    obj = TEX_OBJECTS[kind]
    out, _ = device_points(sc, gpu, obj, FN_TEX, x)
    log_t = None
    m = {}
    if kind == "blackbody":  # the device's own log10 of temperature * redshift (the same IEEE product)
        tz = x[:, 3] * x[:, 2]
        log_t = device_points(sc, gpu, -1, FN_BB, tz)[0][:, 4]
        m.update(log10_stats(tz, log_t))
    ref = oracle.texture_color_n(desc, obj, x, log_t)
    glibc_pow = out[:, 4] == 1.0
    z = x[:, 2]
    # redshift == 1.0 exactly is the one positive finite redshift outside glibc::pow_fast: y log(x) = 0 is
    # glibc's "tiny" special case, so rpow asks OCML.  pow(1, y) is exactly 1 for every y (C99 F.9.4.4,
    # IEEE 754-2008 9.2.1), for OCML as for glibc, so those rows are held to the oracle's bits all the same.
    one = z == 1.0
    bad = (glibc_pow | one) & ~np.all(same_bits(out[:, :4], ref), axis=1)
    m.update({"rows": len(x), "mismatch": int(bad.sum()), "first_bad": x[bad][:3].tolist(),
              "pow_fallback_rows": int((~glibc_pow).sum()),
              "pow_fallback_at_redshift_one": int((~glibc_pow & one).sum()), "redshift_one_rows": int(one.sum()),
              "pow_fallback_on_positive_finite_redshift": int((~glibc_pow & (z > 0) & np.isfinite(z) & ~one).sum()),
              "fallback_rows_equal_anyway": int(np.all(same_bits(out[~glibc_pow, :4], ref[~glibc_pow]), axis=1).sum()),
              "distinct_colours": int(len(np.unique(ref[np.isfinite(ref).all(1)], axis=0)))})
    return m


def blend_check(oracle, sc, gpu, R):
    x = R.x
    out, _ = device_points(sc, gpu, -1, FN_BLEND, x)
    ref = oracle.blend_n(x[:, :4], x[:, 4:])
    bad = ~np.all((bits(out[:, :4]) == bits(ref)) | (np.isnan(out[:, :4]) & np.isnan(ref)), axis=1)
    return {"rows": len(x), "mismatch": int(bad.sum()), "first_bad": x[bad][:3].tolist()}
