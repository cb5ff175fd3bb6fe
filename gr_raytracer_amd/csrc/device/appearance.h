// appearance.h — from the numbers of a hit to a pixel: what the trace (geodesic.hip) and the
// deferred shade of a geometry buffer (gbuffer_shade.hip) both need and neither may restate,
// because the deferred shade's pixels have shade_kernel's bits.
//   the reference's pow / sin / cos (glibc's fast paths, OCML outside them), f64::clamp and
//   the saturating casts; XYZA and its blend; texture, blackbody and temperature lookups;
//   write_out, the one place a pixel's outputs are stored.
// Included once per unit, inside its namespaces (namespace grt or grt::<unit>), after
// dev_scene.h, glibc_math.h and kernels.h and after GDEV is defined.
#pragma once

// The OCML fallbacks below run outside glibc's fast paths only (never for the angles and
// controller ratios of a render): out of line, so their code stays out of the hot loops.
#ifndef GRT_SLOW_NOINLINE
#define GRT_SLOW_NOINLINE 1
#endif
#if GRT_SLOW_NOINLINE
#define GRT_SLOW __device__ __attribute__((noinline, cold))
#else
#define GRT_SLOW GDEV
#endif
GRT_SLOW double ocml_pow(double x, double y) { return pow(x, y); }
// returned by value: a pointer into the caller's frame passed to an out-of-line call would
// keep the caller's (sin, cos) in scratch memory at every rsincos site, fast path included
struct SinCos {
  double s, c;
};
GRT_SLOW SinCos ocml_sincos(double x) {
  SinCos r;
  sincos(x, &r.s, &r.c);
  return r;
}
GRT_SLOW double ocml_sin(double x) { return sin(x); }
GRT_SLOW double ocml_cos(double x) { return cos(x); }

// f64::powf == glibc pow: bit-exact on glibc's fast path, OCML outside it.
GDEV double rpow(double x, double y) {
  double r;
  if (glibc::pow_fast(x, y, &r)) return r;
  return ocml_pow(x, y);
}
// f64::sin / f64::cos of one operand in one reference function: the compiler fuses
// them into glibc's sincos (glibc_math.h); a lone sin() stays glibc's sin.  Both are
// bit-exact for |x| < 105414350; OCML beyond (never reached by angles here).
GDEV void rsincos(double x, double* s, double* c) {
  double ss, cc;
  if (!glibc::sincos_fast(x, &ss, &cc)) {
    const SinCos r = ocml_sincos(x);
    ss = r.s;
    cc = r.c;
  }
  *s = ss;
  *c = cc;
}
GDEV double rsin(double x) {
  double r;
  if (glibc::sin_fast(x, &r)) return r;
  return ocml_sin(x);
}
GDEV double rcos(double x) {
  double r;
  if (glibc::cos_fast(x, &r)) return r;
  return ocml_cos(x);
}

GDEV double rclamp(double v, double lo, double hi) {  // f64::clamp
  if (v < lo) v = lo;
  if (v > hi) v = hi;
  return v;
}
GDEV uint32_t sat_u32(double v) {
  if (!(v > 0.0)) return 0u;
  if (v >= 4294967296.0) return 0xffffffffu;
  return (uint32_t)v;
}
GDEV uint64_t sat_u64(double v) {
  if (!(v > 0.0)) return 0ull;
  if (v >= 18446744073709551616.0) return ~0ull;
  return (uint64_t)v;
}

struct XYZA {
  double x, y, z, a;
};

// color.rs:49-69  ("other over self")
GDEV XYZA blend(const XYZA& self, const XYZA& other) {
  double ab = rclamp(self.a, 0.0, 1.0);
  double af = rclamp(other.a, 0.0, 1.0);
  double ao = af + ab * (1.0 - af);
  if (ao <= 0.0) return XYZA{0.0, 0.0, 0.0, 0.0};
  XYZA r;
  r.x = (other.x * af + self.x * ab * (1.0 - af)) / ao;
  r.y = (other.y * af + self.y * ab * (1.0 - af)) / ao;
  r.z = (other.z * af + self.z * ab * (1.0 - af)) / ao;
  r.a = ao;
  return r;
}

// ============================================================== shading =========
GDEV XYZA texel(const DevScene& S, const DevTexture& t, uint32_t x, uint32_t y) {
  uint32_t px = t.rgba[(uint64_t)y * t.width + x];
  double r = S.srgb_lin[px & 0xffu];
  double g = S.srgb_lin[(px >> 8) & 0xffu];
  double b = S.srgb_lin[(px >> 16) & 0xffu];
  XYZA c;  // srgb_to_xyz (color.rs:310-332), nalgebra gemv order
  c.x = 0.4124564 * r;
  c.x = 0.3575761 * g + c.x;
  c.x = 0.1804375 * b + c.x;
  c.y = 0.2126729 * r;
  c.y = 0.7151522 * g + c.y;
  c.y = 0.0721750 * b + c.y;
  c.z = 0.0193339 * r;
  c.z = 0.1191920 * g + c.z;
  c.z = 0.9503041 * b + c.z;
  c.a = (double)(px >> 24) / 255.0;
  return c;
}

// The reference's table searches (binary search, then idx = partition point - 1) over a
// sorted table a[0..n) with a[0] < x < a[n - 1]: the last idx with a[idx] <= x.  Both
// tables are evenly spaced grids (host/setup.cpp: x0 + i * step), so the index is guessed
// from the spacing and corrected by comparisons against the table itself: the same idx
// for any sorted table (a poor guess only costs more steps), with two dependent loads
// instead of the ~10 of the bisection.
GDEV uint32_t lut_index(const double* a, uint32_t n, double a0, double a_last, double x) {
  const double g = (x - a0) * ((double)(n - 1) / (a_last - a0));
  uint32_t idx = g >= (double)(n - 2) ? n - 2 : (g > 0.0 ? (uint32_t)g : 0u);
  while (idx < n - 2 && a[idx + 1] <= x) ++idx;
  while (idx > 0 && a[idx] > x) --idx;
  return idx;
}

// texture.rs:149-195 over a (log10 T, XYZ) table in global memory or LDS
GDEV XYZA sample_blackbody_lut(const double* lt, const double* c, uint32_t n, double temperature) {
  double log_t = log10(fmax(temperature, 10.0));
  const double lt_first = lt[0], lt_last = lt[n - 1];
  if (!isfinite(log_t) || log_t <= lt_first) return XYZA{c[0], c[1], c[2], 1.0};
  if (log_t >= lt_last) return XYZA{c[3 * (n - 1)], c[3 * (n - 1) + 1], c[3 * (n - 1) + 2], 1.0};
  const uint32_t idx = lut_index(lt, n, lt_first, lt_last, log_t);
  double lt0 = lt[idx], lt1 = lt[idx + 1];
  const double* c0 = c + 3 * idx;
  const double* c1 = c + 3 * (idx + 1);
  double t = (log_t - lt0) / (lt1 - lt0);
  return XYZA{c0[0] + t * (c1[0] - c0[0]), c0[1] + t * (c1[1] - c0[1]), c0[2] + t * (c1[2] - c0[2]), 1.0};
}
GDEV XYZA sample_blackbody(const DevScene& S, double temperature) {
  return sample_blackbody_lut(S.bb_log_t, S.bb_xyz, S.bb_n, temperature);
}

// TextureMap::color_at_uv (texture.rs:93-257); bb_lt / bb_xyz: the blackbody table
// (S.bb_log_t / S.bb_xyz, or an LDS copy of it)
GDEV XYZA texture_color_lut(const DevScene& S, const DevTexture& t, double u, double v, double redshift,
                            double temperature, const double* bb_lt, const double* bb_xyz) {
  XYZA c;
  if (t.kind == GRT_TEX_BITMAP) {
    uint32_t width = t.width, height = t.height;
    double p_x = (double)width * u;
    double p_y = (double)height * v;
    uint32_t xf = min(sat_u32(floor(p_x)), width - 1);
    uint32_t yf = min(sat_u32(floor(p_y)), height - 1);
    uint32_t xc = min(sat_u32(ceil(p_x)), width - 1);
    uint32_t yc = min(sat_u32(ceil(p_y)), height - 1);
    XYZA c00 = texel(S, t, xf, yf), c01 = texel(S, t, xf, yc);
    XYZA c11 = texel(S, t, xc, yc), c10 = texel(S, t, xc, yf);
    double dx = p_x - (double)xf;
    double dy = p_y - (double)yf;
    double w00 = (1.0 - dx) * (1.0 - dy);
    double w01 = (1.0 - dx) * dy;
    double w10 = dx * (1.0 - dy);
    double w11 = dx * dy;
    c.x = w00 * c00.x + w10 * c10.x + w01 * c01.x + w11 * c11.x;
    c.y = w00 * c00.y + w10 * c10.y + w01 * c01.y + w11 * c11.y;
    c.z = w00 * c00.z + w10 * c10.z + w01 * c01.z + w11 * c11.z;
    c.a = w00 * c00.a + w10 * c10.a + w01 * c01.a + w11 * c11.a;
  } else if (t.kind == GRT_TEX_CHECKER) {
    uint64_t ut = sat_u64(floor(u * t.cw));
    uint64_t vt = sat_u64(floor(v * t.ch));
    const double* cc = ((ut + vt) % 2 == 0) ? t.c1 : t.c2;
    c = XYZA{cc[0], cc[1], cc[2], cc[3]};
  } else {
    c = sample_blackbody_lut(bb_lt, bb_xyz, S.bb_n, temperature * redshift);
  }
  // apply_beaming (color.rs:72-80): powf(redshift, e); pow(x, +-0) is 1 for every x (C99
  // F.9.4.4, glibc), so the stock scenes' exponent 0 skips the call
  double f = t.beaming == 0.0 ? 1.0 : rpow(redshift, t.beaming);
  return XYZA{c.x * f, c.y * f, c.z * f, c.a};
}
GDEV XYZA texture_color(const DevScene& S, const DevTexture& t, double u, double v, double redshift,
                        double temperature) {
  return texture_color_lut(S, t, u, v, redshift, temperature, S.bb_log_t, S.bb_xyz);
}

// KerrTemperatureComputer::compute_temperature (temperature.rs:198-253); lut_r / lut_t:
// the object's (r, T) table in global memory or an LDS copy
GDEV int compute_temperature_lut(const DevObject& o, const double* lut_r, const double* lut_t, double radius,
                                 double* out) {
  if (o.temp_kind == GRT_TEMP_CONSTANT) {
    *out = o.temp_constant;
    return GRT_OK;
  }
  if (!isfinite(radius)) return GRT_ERR_NON_FINITE_RADIUS;
  if (radius < o.r_isco) return GRT_ERR_BELOW_RISCO;
  uint32_t n = o.lut_n;
  const double r_first = lut_r[0], r_last = lut_r[n - 1];
  if (radius <= r_first) { *out = lut_t[0]; return GRT_OK; }
  if (radius >= r_last) { *out = lut_t[n - 1]; return GRT_OK; }
  const uint32_t idx = lut_index(lut_r, n, r_first, r_last, radius);
  double r0 = lut_r[idx], t0 = lut_t[idx], r1 = lut_r[idx + 1], t1 = lut_t[idx + 1];
  double t = (radius - r0) / (r1 - r0);
  *out = t0 + t * (t1 - t0);
  return GRT_OK;
}
GDEV int compute_temperature(const DevObject& o, double radius, double* out) {
  return compute_temperature_lut(o, o.lut_r, o.lut_t, radius, out);
}

// (the step count goes to out.steps from store_ray, KerrBL's from shade_kernel)
GDEV void write_out(const Outputs& out, uint64_t idx, const XYZA& c, int cls, int status, int stop, uint32_t hits) {
  if (out.hits) out.hits[idx] = hits;
  reinterpret_cast<float4*>(out.xyza)[idx] = make_float4((float)c.x, (float)c.y, (float)c.z, (float)c.a);
  out.cls[idx] = (uint8_t)cls;
  out.status[idx] = (uint8_t)status;
  if (out.xyza64) {
    double* d = out.xyza64 + 4 * idx;
    d[0] = c.x;
    d[1] = c.y;
    d[2] = c.z;
    d[3] = c.a;
  }
  if (out.stop) out.stop[idx] = (uint8_t)stop;
}
