"""CPU model of the Schwarzschild tile queue ordered by sincos case (schedule.hip, numpy only).

    python tools/class_order_model.py [--pos X Y Z] [--alpha A] [--size N] [--radius R_S]

A pinhole camera at `pos` looking at the hole (the C2 camera: theta = -pi turns the
tetrad's outward axis inward) sends one ray per pixel.  Each ray moves in the plane of the
camera's position and its own direction; u = 1 / r obeys u'' = -u + 1.5 r_s u^2 in the
angle psi swept in that plane, integrated with fixed-step RK4 to u = 0 (escape) or
u = 1 / r_s (capture).  Rotating the camera's position direction by the swept angle gives
the asymptotic direction and its polar angle theta_f.  In the far field a ray keeps
theta_f to O(b / r), so theta_f decides which case the right-hand side's sincos takes for
nearly all of the ray's steps: Taylor when |pi/2 - theta_f| < TAYLOR_MAX, table elsewhere
in region B.  A wave of the integrate kernel holds rays of W consecutive queue tiles and
leaves the straight-line forms when its lanes disagree.

Prints one JSON object: the Taylor share of the escaping rays (of those in region B), the number of 8x8 tiles
that hold both cases (the straddling tiles), and the share of mixed groups of W
consecutive tiles for the row-major order and for the tiles partitioned by class (stable).
The observer is taken as static: the aberration of the scene's actual observer moves the
border by a few pixels and the shares by less than a percent."""
import argparse
import json
import math

import numpy as np

TAYLOR_MAX = float.fromhex("0x1.020c49ba5e354p-3")
B_LO, B_HI = 0.85546875, 2.4262638092041016  # region B: high word of |theta| in [0x3feb6000, 0x400368fd)
TAYLOR, STRADDLE, TABLE, OTHER = 0, 1, 2, 3


def asymptotic_theta(pos, alpha, size, r_s=1.0, dpsi=1.0 / 32, steps=400):
    """theta_f per pixel (size x size); NaN for captured or undecided rays."""
    pos = np.asarray(pos, float)
    r0 = float(np.linalg.norm(pos))
    th0, ph0 = math.acos(pos[2] / r0), math.atan2(pos[1], pos[0])
    e_r = np.array([math.sin(th0) * math.cos(ph0), math.sin(th0) * math.sin(ph0), math.cos(th0)])
    e_th = np.array([math.cos(th0) * math.cos(ph0), math.cos(th0) * math.sin(ph0), -math.sin(th0)])
    e_ph = np.array([-math.sin(ph0), math.cos(ph0), 0.0])
    z, x, y = -e_r, -e_ph, e_th
    k = 2.0 * math.tan(alpha / 2.0) / size
    c = (np.arange(size) + 1.0 - (size + 1.0) / 2.0) * k
    jj, ii = np.meshgrid(c, c, indexing="ij")  # rows: j', columns: i'
    w = z[None, None, :] + ii[..., None] * x + jj[..., None] * y
    d = -z + 2.0 * w / np.sum(w * w, axis=-1, keepdims=True)  # unit vectors (stereographic camera)
    d_r = d @ e_r
    tang = d - d_r[..., None] * e_r
    s = np.linalg.norm(tang, axis=-1)
    s = np.maximum(s, 1e-300)
    t_hat = tang / s[..., None]
    lapse = math.sqrt(1.0 - r_s / r0)
    u = np.full(d_r.shape, 1.0 / r0)
    v = -lapse * d_r / (r0 * s)
    psi = np.zeros_like(u)
    psi_f = np.full_like(u, np.nan)
    live = np.ones(u.shape, bool)

    def acc(q):
        return -q + 1.5 * r_s * q * q

    for _ in range(steps):
        k1u, k1v = v, acc(u)
        k2u, k2v = v + 0.5 * dpsi * k1v, acc(u + 0.5 * dpsi * k1u)
        k3u, k3v = v + 0.5 * dpsi * k2v, acc(u + 0.5 * dpsi * k2u)
        k4u, k4v = v + dpsi * k3v, acc(u + dpsi * k3u)
        un = u + dpsi / 6.0 * (k1u + 2 * k2u + 2 * k3u + k4u)
        vn = v + dpsi / 6.0 * (k1v + 2 * k2v + 2 * k3v + k4v)
        esc = live & ~(un > 0.0)
        psi_f[esc] = psi[esc] + dpsi * u[esc] / (u[esc] - un[esc])
        live &= ~esc & ~(un >= 1.0 / r_s)
        u = np.where(live, un, u)
        v = np.where(live, vn, v)
        psi = psi + dpsi
        if not live.any():
            break
    nz = np.cos(psi_f) * e_r[2] + np.sin(psi_f) * t_hat[..., 2]
    return np.arccos(np.clip(nz, -1.0, 1.0))


def pixel_class(theta_f):
    a = math.pi / 2 - theta_f
    cls = np.full(theta_f.shape, OTHER, np.int8)
    in_b = (theta_f >= B_LO) & (theta_f < B_HI)
    cls[in_b & (np.abs(a) < TAYLOR_MAX)] = TAYLOR
    cls[in_b & ~(np.abs(a) < TAYLOR_MAX)] = TABLE
    return cls


def tile_sets(cls):
    """Per 8x8 tile: (holds a Taylor ray, holds a table ray), row-major tiles."""
    n = cls.shape[0]
    t = (n + 7) // 8
    pad = np.full((t * 8, t * 8), OTHER, np.int8)
    pad[:n, :n] = cls
    blocks = pad.reshape(t, 8, t, 8).transpose(0, 2, 1, 3).reshape(t * t, 64)
    return (blocks == TAYLOR).any(axis=1), (blocks == TABLE).any(axis=1)


def mixed_fraction(has_tay, has_tab, order, w):
    ht, hb = has_tay[order], has_tab[order]
    m = len(order) // w * w
    gt = ht[:m].reshape(-1, w).any(axis=1)
    gb = hb[:m].reshape(-1, w).any(axis=1)
    return float((gt & gb).mean())


def model(pos, alpha, size, r_s=1.0, widths=(1, 4, 10)):
    theta_f = asymptotic_theta(pos, alpha, size, r_s)
    cls = pixel_class(theta_f)
    escaping = np.isfinite(theta_f)
    has_tay, has_tab = tile_sets(cls)
    tile_cls = np.where(has_tay & has_tab, STRADDLE, np.where(has_tay, TAYLOR, np.where(has_tab, TABLE, OTHER)))
    row_major = np.arange(len(tile_cls))
    by_class = np.argsort(tile_cls, kind="stable")
    return {
        "camera": list(map(float, pos)), "alpha": alpha, "size": size, "radius": r_s,
        "escaping_share": float(escaping.mean()),
        "taylor_share_of_escaping": float((cls == TAYLOR).sum() / max(1, ((cls == TAYLOR) | (cls == TABLE)).sum())),
        "tiles": int(len(tile_cls)),
        "straddling_tiles": int((tile_cls == STRADDLE).sum()),
        "tile_rows_with_a_straddling_tile": int((tile_cls.reshape(-1, (size + 7) // 8) == STRADDLE).any(axis=1).sum()),
        "mixed_fraction": {
            "row_major": {str(w): mixed_fraction(has_tay, has_tab, row_major, w) for w in widths},
            "by_class": {str(w): mixed_fraction(has_tay, has_tab, by_class, w) for w in widths},
        },
    }


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pos", type=float, nargs=3, default=(-16.0, 0.0, 3.5))
    ap.add_argument("--alpha", type=float, default=math.pi / 4)
    ap.add_argument("--size", type=int, default=1500)
    ap.add_argument("--radius", type=float, default=1.0)
    a = ap.parse_args()
    print(json.dumps(model(a.pos, a.alpha, a.size, a.radius), indent=1))
