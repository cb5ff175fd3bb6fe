// geodesic_rhs.h — the first layer of geodesic.hip: the range-free division and square root, the
// charts' metrics, the sincos dispatch (with_sincos) and the ODE right-hand sides (rhs<G>,
// the quad-split Kerr-Schild form).  Included by every unit; needs only the GRT_* knobs.

// x1 / y and x2 / y with one reciprocal refinement.  This is the compiler's own IEEE f64
// division expansion (div_scale, rcp, 2 Newton steps, div_fmas, div_fixup -- identical
// instructions), with the y-only part shared.  The shared part is v_div_scale(y, y, x),
// whose result depends on x only when |x| is extreme (exponent gap >= 768, x/y
// denormal, or exp(x) <= 53); the host enables this (DevScene::div_share) only when
// both numerators are normal with |exponent| < 500, where it cannot.  Every quotient
// is therefore bit-identical to x / y.
GDEV void div2_same_den(double x1, double x2, double y, double* q1, double* q2) {
  bool f0, f1, f2;
  const double ds0 = __builtin_amdgcn_div_scale(x1, y, false, &f0);
  const double rcp = __builtin_amdgcn_rcp(ds0);
  const double fma0 = __builtin_fma(-ds0, rcp, 1.0);
  const double fma1 = __builtin_fma(rcp, fma0, rcp);
  const double fma2 = __builtin_fma(-ds0, fma1, 1.0);
  const double fma3 = __builtin_fma(fma1, fma2, fma1);
  const double n1 = __builtin_amdgcn_div_scale(x1, y, true, &f1);
  const double m1 = n1 * fma3;
  *q1 = __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(__builtin_fma(-ds0, m1, n1), fma3, m1, f1), y, x1);
  const double n2 = __builtin_amdgcn_div_scale(x2, y, true, &f2);
  const double m2 = n2 * fma3;
  *q2 = __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(__builtin_fma(-ds0, m2, n2), fma3, m2, f2), y, x2);
}

// x / y as that same expansion without its range steps, for operands the caller has
// shown to be normals with |x|, |y|, |x / y| all within 2^-600 .. 2^600: there
// v_div_scale returns its operand unchanged and raises no flag (the exponent gap is
// < 768, neither 1 / y nor x / y is denormal, exp(x) > 53), so v_div_fmas is a plain
// fma, and v_div_fixup, which only rewrites NaN / infinity / zero / overflow / underflow
// cases, passes the quotient through.
// The same instructions on the same values, hence x / y's bits.  Measured over the whole
// exponent plane, the exact region is larger (E: |y| normal below 2^1022, x of exponent
// >= -969, gap -1021 .. 1022; the gap >= 768 scaling is an identity there too), and the
// first failures are one exponent outside it (tests/test_gpu_arith.py
// ::test_range_free_arithmetic_map, profiles/r05a/arith_map.json).
// 8 VALU instead of 11; div2_inrange shares 1 / y: 11 instead of 16.
GDEV double div_inrange(double x, double y) {
  const double rcp = __builtin_amdgcn_rcp(y);
  const double fma0 = __builtin_fma(-y, rcp, 1.0);
  const double fma1 = __builtin_fma(rcp, fma0, rcp);
  const double fma2 = __builtin_fma(-y, fma1, 1.0);
  const double fma3 = __builtin_fma(fma1, fma2, fma1);
  const double m = x * fma3;
  return __builtin_fma(__builtin_fma(-y, m, x), fma3, m);
}
GDEV void div2_inrange(double x1, double x2, double y, double* q1, double* q2) {
  const double rcp = __builtin_amdgcn_rcp(y);
  const double fma0 = __builtin_fma(-y, rcp, 1.0);
  const double fma1 = __builtin_fma(rcp, fma0, rcp);
  const double fma2 = __builtin_fma(-y, fma1, 1.0);
  const double fma3 = __builtin_fma(fma1, fma2, fma1);
  const double m1 = x1 * fma3;
  *q1 = __builtin_fma(__builtin_fma(-y, m1, x1), fma3, m1);
  const double m2 = x2 * fma3;
  *q2 = __builtin_fma(__builtin_fma(-y, m2, x2), fma3, m2);
}
// |x| in (2^-300, 2^300), NaN excluded: two compares with the abs modifier
GDEV bool in_div_range(double x) { return fabs(x) > 0x1p-300 && fabs(x) < 0x1p300; }

// x / y as the compiler's expansion without its two v_div_scale steps but with
// v_div_fixup: exact (the same instructions on the same values) when y is a normal within
// 2^+-600 and x is 0 or a normal with |x|, |x / y| within 2^+-600 -- v_div_scale would
// return its operand unchanged with no flag (so v_div_fmas is a plain fma), and
// v_div_fixup rewrites the zero-numerator case from the operands alone (a -0 / y chain
// gives +0; the fixup returns the signed zero).  9 VALU instead of 11.
GDEV double div_fx(double x, double y) {
  const double rcp = __builtin_amdgcn_rcp(y);
  const double fma0 = __builtin_fma(-y, rcp, 1.0);
  const double fma1 = __builtin_fma(rcp, fma0, rcp);
  const double fma2 = __builtin_fma(-y, fma1, 1.0);
  const double fma3 = __builtin_fma(fma1, fma2, fma1);
  const double m = x * fma3;
  return __builtin_amdgcn_div_fixup(__builtin_fma(__builtin_fma(-y, m, x), fma3, m), y, x);
}

// Kerr-Schild metric quotients: the compiler's division, or div_fx (FD) where the caller
// has established ks_fd_ok for the state
template <bool FD>
GDEV double kdiv(double x, double y) {
  if constexpr (FD) return div_fx(x, y);
  else return x / y;
}
// sqrt(x) as the compiler's f64 expansion for gfx950 without its range steps: for a
// normal x >= 2^-767 the input scaling (ldexp by 0), the output rescaling and the
// zero / infinity select are identities, leaving v_rsq_f64 and the Newton steps on the
// same values, hence sqrt's bits (device check: tests/test_gpu_arith.py: exact for every
// x >= 2^-969, the first failure at 2^-971).  10 VALU instead of 17.
GDEV double sqrt_fx(double x) {
  const double r = __builtin_amdgcn_rsq(x);
  double g = x * r, h = r * 0.5;
  const double e = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, e, g);
  h = __builtin_fma(h, e, h);
  double d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  d = __builtin_fma(-g, g, x);
  return __builtin_fma(d, h, g);
}
template <bool FD>
GDEV double ksqrt(double x) {
  if constexpr (FD && GRT_FAST_SQRT_KS) return sqrt_fx(x);
  else return sqrt(x);
}

constexpr double PI = 3.14159265358979323846;
constexpr double TWO_PI = 2.0 * 3.14159265358979323846;

GDEV double rem_euclid(double x, double m) {
  double r = fmod(x, m);
  return r < 0.0 ? r + fabs(m) : r;
}

// Per-ray constants: observer energy (redshift.rs:40-60) and, for KerrBL, the
// conserved E, L_z, Carter Q (kerr_bl.rs:505-577).
struct RayConst {
  double obs;
  double e, lz, q;
  double pt, pphi;  // RayFrequencyData p_t, p_phi (redshift.rs:45-60), volumetric scenes only
};

// =========================================================== geometry kernels ======
// ---- Kerr-Schild helpers (kerr.rs:31-110) ----
template <bool FD = false>
GDEV double ks_r_sqr(double a, double x, double y, double z) {
  double rho_sqr = x * x + y * y + z * z;
  return 0.5 * (rho_sqr - a * a + ksqrt<FD>((rho_sqr - a * a) * (rho_sqr - a * a) + 4.0 * a * a * z * z));
}
// metric(): symmetric by construction; returns the 10 distinct entries in g.
template <bool FD = false>
GDEV void ks_metric(double radius, double a, double x, double y, double z, double g[4][4]) {
  double r_sqr = ks_r_sqr<FD>(a, x, y, z);
  double r = ksqrt<FD>(r_sqr);
  double f = kdiv<FD>(r * r * r * radius, r * r * r * r + a * a * z * z);
  double k_0 = 1.0;
  double k_x = kdiv<FD>(r * x + a * y, r_sqr + a * a);
  double k_y = kdiv<FD>(r * y - a * x, r_sqr + a * a);
  double k_z = kdiv<FD>(z, r);
  g[0][0] = k_0 * k_0 * f - 1.0;
  g[0][1] = k_0 * k_x * f;
  g[0][2] = k_0 * k_y * f;
  g[0][3] = k_0 * k_z * f;
  g[1][1] = k_x * k_x * f + 1.0;
  g[1][2] = k_x * k_y * f;
  g[1][3] = k_x * k_z * f;
  g[2][2] = k_y * k_y * f + 1.0;
  g[2][3] = k_y * k_z * f;
  g[3][3] = k_z * k_z * f + 1.0;
  g[1][0] = g[0][1];
  g[2][0] = g[0][2];
  g[2][1] = g[1][2];
  g[3][0] = g[0][3];
  g[3][1] = g[1][3];
  g[3][2] = g[2][3];
}
template <bool FD = false>
GDEV void ks_metric_contra(double radius, double a, double x, double y, double z, double g[4][4]) {
  double r_sqr = ks_r_sqr<FD>(a, x, y, z);
  double r = ksqrt<FD>(r_sqr);
  double f = kdiv<FD>(r * r * r * radius, r * r * r * r + a * a * z * z);
  double kc[4];
  kc[0] = -1.0;
  kc[1] = kdiv<FD>(r * x + a * y, r_sqr + a * a);
  kc[2] = kdiv<FD>(r * y - a * x, r_sqr + a * a);
  kc[3] = kdiv<FD>(z, r);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double eta = (i == j) ? (i == 0 ? -1.0 : 1.0) : 0.0;
      g[i][j] = eta - f * kc[i] * kc[j];
    }
}
// nalgebra gemv order: y_i = A_i0 x_0; y_i = A_ik x_k + y_i
GDEV void mat_vec(const double A[4][4], const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double s = A[i][0] * x[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) s = A[i][k] * x[k] + s;
    y[i] = s;
  }
}
GDEV double quad_form(const double* v, const double M[4][4], const double* w) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double r = v[0] * M[0][j];
#pragma unroll
    for (int k = 1; k < 4; ++k) r = v[k] * M[k][j] + r;
    s = (j == 0) ? r * w[0] : r * w[j] + s;
  }
  return s;
}

// kerr.rs:149-186 + :228-235: returns 0.5 * p^T (G dG_i G) p, which equals
// -0.5 * p^T d_matrix_contravariant(i) p exactly (negation commutes with rounding).
template <bool FD = false>
GDEV double ks_accel(double radius, double a, int index, double x, double y, double z,
                     const double G[4][4], const double* p) {
  double c = index == 1 ? x : (index == 2 ? y : z);
  double h = 1e-10 * fmax(fabs(c), 1.0);
  double dx = index == 1 ? h : 0.0, dy = index == 2 ? h : 0.0, dz = index == 3 ? h : 0.0;
  double mp[4][4], mm[4][4];
  ks_metric<FD>(radius, a, x + dx, y + dy, z + dz, mp);
  ks_metric<FD>(radius, a, x - dx, y - dy, z - dz, mm);
  double two_h = 2.0 * h;
  double D[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) D[i][j] = kdiv<FD>(mp[i][j] - mm[i][j], two_h);
  double GD[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double s = G[i][0] * D[0][j];
#pragma unroll
      for (int k = 1; k < 4; ++k) s = G[i][k] * D[k][j] + s;
      GD[i][j] = s;
    }
  // stream the columns of (GD)G straight into the quadratic form
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double col[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double s = GD[i][0] * G[0][j];
#pragma unroll
      for (int k = 1; k < 4; ++k) s = GD[i][k] * G[k][j] + s;
      col[i] = s;
    }
    double r = p[0] * col[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) r = p[k] * col[k] + r;
    q = (j == 0) ? r * p[0] : r * p[j] + q;
  }
  return 0.5 * q;
}

// ---- KerrBL helpers (kerr_bl.rs:62-118, :253-272) ----
GDEV double bl_delta(double r, double r_s, double a) { return r * r - r_s * r + a * a; }
GDEV void metric_bl(double r_s, double a, double r, double sin_t, double cos_t, double g[4][4]) {
  double sig = r * r + a * a * (cos_t * cos_t);
  double sin2 = sin_t * sin_t;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) g[i][j] = 0.0;
  g[0][0] = -(1.0 - r_s * r / sig);
  g[1][1] = sig / bl_delta(r, r_s, a);
  g[2][2] = sig;
  g[3][3] = (r * r + a * a + a * a * r_s * r * sin2 / sig) * sin2;
  double g_tph = -a * r_s * r * sin2 / sig;
  g[0][3] = g_tph;
  g[3][0] = g_tph;
}

#if GRT_PATH_COUNT
// Diagnostic counters of integrate_kernel, [k] wave-level executions (one lane counts each),
// [8 + k] the same in lanes.  Kerr-Schild RHS: 0 range-free form, 1 IEEE form.  Light
// charts' RHS: 0 region-B table with range-free divisions, 1 region-B Taylor with them,
// 2 region-B with the IEEE divisions, 3 general (branchy) sincos.  All: 4 near-field window
// pass, 5 accepted step, 6 attempt, 7 attempt taken again in the full form (rkf_short_ok
// missed).  What the waves of path 3 hold: 8 every lane in glibc's region A
// (2^-27 <= |x| < 0.855469) on do_sin's table path, 9 every lane in region A otherwise,
// 10 every lane in region C (|x| >= 2.426265) with quadrant n = 2, 11 mixed.  Counted besides
// those four: 12 every lane in region B (its table and Taylor cases mixed) with div_ok, 13 every
// lane in region B with div_ok missed on some lane.
constexpr int NPATH = 14;
__shared__ unsigned long long path_lds[2 * NPATH];
__device__ unsigned long long g_path[2 * NPATH];
GDEV void path_count(int k) {
  const uint64_t m = __ballot(1);  // the lanes executing this path together
  if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) {
    atomicAdd(&path_lds[k], 1ull);
    atomicAdd(&path_lds[NPATH + k], (unsigned long long)__popcll(m));
  }
}
#define PATH_COUNT(k) path_count(k)
#else
#define PATH_COUNT(k) ((void)0)
#endif

// Whether every lane executing this holds p: the votes of p and of the executing lanes are
// taken as 64-bit masks and compared on the scalar side (`__ballot(!p) == 0` is lowered
// through a 0/1 vector register and a compare of it: 2 VALU per vote).
GDEV bool wave_all(bool p) { return __ballot(p) == __ballot(true); }

// sincos(theta), then body(sin, cos, fast).  When every lane of the wave is in one of
// sincos's region-B cases (x near pi/2; glibc_math.h sincos_b_*), the sincos is the
// straight-line form of that case and body runs in the same basic block, so its own
// dependency chains (the divisions) interleave with the sincos polynomial; fast = true
// there (the caller passes fast_ok = whether body may then take its fast form).  The same
// bits as rsincos in every case (tests/test_glibc_math.py).
// div_ok (per lane): the body's divisions may drop their range steps (div_inrange) in the
// region-B cases; body's fourth argument says so at compile time (std::true_type), so
// each form is one basic block from the sincos through the body.
// UNIT (Schwarzschild only): with `unit` set (DevScene::unit_radius, a scene constant in a
// scalar register) the range-free cases hand body its unit-radius form, div_form<2>.  The
// scalar branch is taken before the sincos, so that form too is one basic block from the
// sincos through the body (a ballot between the two cost 1 %: DESIGN.md 3).
template <int K>
using div_form = std::integral_constant<int, K>;  // 0 IEEE, 1 range-free, 2 range-free with radius == 1.0
// VOTES (Schwarzschild, GRT_SCALAR_VOTES): div_ok is the wave's vote on it, a 64-bit lane mask
// (schw_div_ok_render_mask), and the region-B case predicates are voted on compare by compare
// (a vote on one compare is that compare's own lane mask; a vote on a product of compares
// goes through a 0/1 vector register); the four cases are then decided by mask arithmetic
// against the executing lanes.  The same decisions.
template <bool FDIV = false, bool UNIT = false, bool VOTES = false, class F, class D = bool>
GDEV void with_sincos(double theta, bool fast_ok, F&& body, D div_ok = false, bool unit = false) {
#if GRT_SINCOS_B
  if (fast_ok) {
    double st, ct;
    [[maybe_unused]] bool tab = false, tay = false;
    [[maybe_unused]] uint64_t ex = 0, mt = 0, my = 0, md = 0;
    if constexpr (VOTES) {
      static_assert(std::is_same<D, uint64_t>::value, "with_sincos<VOTES>: div_ok as a lane mask");
      const uint64_t mb = __ballot(glibc::sincos_b_region(theta)), ms = __ballot(glibc::sincos_b_small(theta));
      ex = __ballot(true);
      mt = mb & ~ms;
      my = mb & ms;
      md = div_ok;
    } else {
      tab = glibc::sincos_b_table_ok(theta);
      tay = glibc::sincos_b_taylor_ok(theta);
    }
    if constexpr (FDIV) {
      if (VOTES ? (mt & md) == ex : __ballot(!(tab & div_ok)) == 0) {
        PATH_COUNT(0);
        if constexpr (UNIT) {
          if (unit) {
            glibc::sincos_b_table(theta, &st, &ct);
            body(st, ct, true, div_form<2>{});
            return;
          }
        }
        glibc::sincos_b_table(theta, &st, &ct);
        body(st, ct, true, std::true_type{});
        return;
      }
      if (VOTES ? (my & md) == ex : __ballot(!(tay & div_ok)) == 0) {
        PATH_COUNT(1);
        if constexpr (UNIT) {
          if (unit) {
            glibc::sincos_b_taylor(theta, &st, &ct);
            body(st, ct, true, div_form<2>{});
            return;
          }
        }
        glibc::sincos_b_taylor(theta, &st, &ct);
        body(st, ct, true, std::true_type{});
        return;
      }
    }
    if (VOTES ? mt == ex : __ballot(!tab) == 0) {
      PATH_COUNT(2);
      glibc::sincos_b_table(theta, &st, &ct);
      body(st, ct, true, std::false_type{});
      return;
    }
    if (VOTES ? my == ex : __ballot(!tay) == 0) {
      PATH_COUNT(2);
      glibc::sincos_b_taylor(theta, &st, &ct);
      body(st, ct, true, std::false_type{});
      return;
    }
  }
#endif
  PATH_COUNT(3);
#if GRT_PATH_COUNT
  {
    const uint32_t k = (uint32_t)(glibc::as_u64(theta) >> 32) & 0x7fffffffu;
    const bool ra = k >= 0x3e400000u && k < 0x3feb6000u, ra_tab = ra && !(fabs(theta) < glibc::TAYLOR_MAX);
    double ca, cda;
    const bool rc2 = k >= 0x400368fdu && k < 0x419921fbu && glibc::reduce_sincos_nf(theta, &ca, &cda) == 2;
    const bool rb = k >= 0x3feb6000u && k < 0x400368fdu;
    bool dk;
    if constexpr (VOTES) dk = ((div_ok >> (threadIdx.x & 63)) & 1) != 0;
    else dk = div_ok;
    if (fast_ok && __ballot(!(rb & dk)) == 0) PATH_COUNT(12);
    else if (fast_ok && __ballot(!rb) == 0) PATH_COUNT(13);
    if (__ballot(!ra_tab) == 0) PATH_COUNT(8);
    else if (__ballot(!ra) == 0) PATH_COUNT(9);
    else if (__ballot(!rc2) == 0) PATH_COUNT(10);
    else PATH_COUNT(11);
  }
#endif
  double st, ct;
  rsincos(theta, &st, &ct);
  body(st, ct, false, std::false_type{});
}

// Whether every quotient and square root of rhs<KERR> at state (x, y, z) is in the exact
// region of div_fx / sqrt_fx.  That region (measured over the whole exponent plane,
// tests/test_gpu_arith.py::test_range_free_arithmetic_map) is E: y normal with
// |y| < 2^1022, x = 0 or of exponent >= -969, exponent gap within -1021 .. 1022; sqrt_fx:
// x >= 2^-969.  Bound chain, with cap = S.ks_cap <= 2^32 (host: 2^ceil(log2(2 max_radius)),
// within 2^10 .. 2^32) and S.div_fast (radius within 2^+-20, a = 0 or within 2^+-20):
//  * the state: each coordinate 0 or 2^-100 <= |c| < cap; D = rho^2 - a^2 >= 2^-10 + 2^-31 rho^2.
//  * the finite-difference points of ks_accel move one coordinate by h = 1e-10 max(|c|, 1):
//    it stays 0 / >= 2^-86 / +-1e-10 and <= 2^32, and rho^2 moves by < 2^-32 (rho^2 + 1), so
//    D >= 2^-11 and rho^2 < 2^66 at every point the metric is evaluated.
//  * sqrt_fx arguments: D^2 + 4 a^2 z^2 in 2^-22 .. 2^133; r^2 = (D + sqrt(..)) / 2 in
//    2^-11 .. 2^66 (r^2 <= rho^2), so r in 2^-5.5 .. 2^33.
//  * f = r^3 radius / (r^4 + a^2 z^2): numerator 2^-36.5 .. 2^119, denominator 2^-22 .. 2^133.
//  * k_x, k_y: numerator r x + a y is 0, or a nonzero sum of terms >= 2^-120 (>= 2^-172, a
//    multiple of the smaller term's ulp), <= 2^66; denominator r^2 + a^2 in 2^-11 .. 2^67.
//    k_z = z / r: numerator 0 or >= 2^-100, denominator 2^-5.5 .. 2^33.  So every k is 0 or
//    within 2^-239 .. 2^76, f within 2^-170 .. 2^15, metric entries 0 or within 2^-648 .. 2^168.
//  * D_ij = (mp - mm) / 2h: numerator 0 or >= an ulp of the smaller entry (>= 2^-700), <= 2^169;
//    2h = 2e-10 max(|c|, 1) within 2^-33 .. 2^0.
// Every numerator is 0 or of exponent -700 .. 169, every denominator of exponent -33 .. 133:
// inside E, with the box |x|, |y|, |x / y| <= 2^+-600 of the earlier argument to spare.  The
// device check of the whole RHS against its IEEE form on states at these edges, cap 2^15 and
// 2^32: tests/test_gpu_arith.py::test_rhs_kerr_schild_fast_form_matches_ieee.
GDEV bool ks_fd_ok(double a, double x, double y, double z, double cap) {
  auto c_ok = [cap](double c) { return (c == 0.0) | ((fabs(c) >= 0x1p-100) & (fabs(c) < cap)); };
  const double rho2 = x * x + y * y + z * z;
  return c_ok(x) & c_ok(y) & c_ok(z) & (rho2 - a * a >= 0x1p-10 + 0x1p-31 * rho2);
}
// Region-B division predicates of the Schwarzschild and KerrBL RHS (see there)
GDEV bool schw_div_ok(const DevScene& S, double r) {
  return S.div_fast && (fabs(r) > 0x1p-100) & (fabs(r) < 0x1p100) & (fabs(r - S.radius) > S.radius * 0x1p-40);
}
// What the render asks at each RHS: r > S.div_r_lo and r < 2^100, where the host (api.hip)
// sets div_r_lo to radius (1 + 2^-40), moved up until schw_div_ok's third test holds at
// div_r_lo itself.  With S.div_fast (0 < radius within 2^+-50) this implies schw_div_ok:
// r > div_r_lo > radius > 2^-50 gives |r| > 2^-100, and the rounded r - radius is monotone
// in r, so it is >= div_r_lo - radius > 2^-40 radius.  So the proofs at rhs<SCHWARZSCHILD>
// hold unchanged on this subset, in two compares instead of a subtraction and three.  A ray
// inside the horizon or at a negative r takes the IEEE divisions, as every r may.
GDEV bool schw_div_ok_render(const DevScene& S, double r) {
#if GRT_DIV_OK_CHEAP
  return S.div_fast && (r > S.div_r_lo) & (r < 0x1p100);
#else
  return schw_div_ok(S, r);
#endif
}
#if GRT_SCALAR_VOTES
// schw_div_ok_render as the vote of the executing lanes, one vote per compare (with_sincos<VOTES>)
GDEV uint64_t schw_div_ok_render_mask(const DevScene& S, double r) {
  static_assert(GRT_DIV_OK_CHEAP, "schw_div_ok_render_mask: the two-compare predicate");
  const uint64_t lo = __ballot(r > S.div_r_lo), hi = __ballot(r < 0x1p100);
  return S.div_fast ? lo & hi : 0ull;
}
#endif
GDEV bool bl_div_ok(const DevScene& S, double r, double del, double l_z) {
  return S.div_fast && (fabs(r) < 0x1p100) & in_div_range(del) & (fabs(l_z) > 0x1p-200) & (fabs(l_z) < 0x1p100);
}

// ---- the ODE right-hand sides ----
// MODE 0: the render's RHS.  MODE 1 / 2 (rhs_check_kernel only): region-B sincos (or no
// sincos: Kerr-Schild), then the range-free (1) or the IEEE (2) form of the body, whatever
// the predicates say -- the check compares the two where the predicate holds.
template <int G, int MODE = 0>
GDEV void rhs(const DevScene& S, const RayConst& rc, const double* y, double* o) {
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD) {  // schwarzschild.rs:54-80
    double radius = S.radius;
    double r = y[1], theta = y[2];
    double v_t = y[4], v_r = y[5], v_theta = y[6], v_phi = y[7];
    auto body = [&](double st, double ct, bool fast, auto fdiv) {
      if constexpr (decltype(fdiv)::value != 0) {
        // rcp_seed.h: 1 / (r r) seeded from the refined 1 / r
        auto hw_rcp = [](double v) { return __builtin_amdgcn_rcp(v); };
        const double rr = r * r;
        double Yr, Yrr, Ya, Yst;
        rcpseed::rcp_r_rr(r, rr, hw_rcp, &Yr, &Yrr);
        double radius_over_r, two_over_r, a, a_prime;
        if constexpr (decltype(fdiv)::value == 2) {
          // radius == 1.0 (S.unit_radius): the same bits from 6 fewer instructions (rcp_seed.h)
          rcpseed::unit_radius_quotients(r, rr, Yr, Yrr, &radius_over_r, &two_over_r, &a, &a_prime);
          rcpseed::rcp_pair(a, st, hw_rcp, &Ya, &Yst);
        } else {
          radius_over_r = rcpseed::div_by_rcp(radius, r, Yr);
          two_over_r = rcpseed::div_by_rcp(2.0, r, Yr);
          a = 1.0 - radius_over_r;
          rcpseed::rcp_pair(a, st, hw_rcp, &Ya, &Yst);
          a_prime = rcpseed::div_by_rcp(radius, rr, Yrr);
        }
        double aprime_over_a = rcpseed::div_by_rcp(a_prime, a, Ya);
        o[0] = v_t;
        o[1] = v_r;
        o[2] = v_theta;
        o[3] = v_phi;
        o[4] = -(aprime_over_a)*v_t * v_r;
        o[5] = -0.5 * a * a_prime * v_t * v_t + 0.5 * (aprime_over_a)*v_r * v_r +
               a * r * (v_theta * v_theta + v_phi * v_phi * st * st);
        o[6] = -(two_over_r)*v_r * v_theta + st * ct * v_phi * v_phi;
        o[7] = -(two_over_r)*v_phi * v_r - rcpseed::div_by_rcp(2.0 * ct, st, Yst) * v_theta * v_phi;
        return;
      }
      double radius_over_r, two_over_r;
#if GRT_SHARED_DIV
      if (fast || S.div_share) {
        div2_same_den(radius, 2.0, r, &radius_over_r, &two_over_r);
      } else
#endif
      {
        radius_over_r = radius / r;
        two_over_r = 2.0 / r;
      }
      double a = 1.0 - radius_over_r;
      double a_prime = radius / (r * r);
      double aprime_over_a = a_prime / a;
      o[0] = v_t;
      o[1] = v_r;
      o[2] = v_theta;
      o[3] = v_phi;
      o[4] = -(aprime_over_a)*v_t * v_r;
      o[5] = -0.5 * a * a_prime * v_t * v_t + 0.5 * (aprime_over_a)*v_r * v_r +
             a * r * (v_theta * v_theta + v_phi * v_phi * st * st);
      o[6] = -(two_over_r)*v_r * v_theta + st * ct * v_phi * v_phi;
      o[7] = -(two_over_r)*v_phi * v_r - 2.0 * ct / st * v_theta * v_phi;
    };
    // fast form: the shared reciprocal, decided with the wave-uniform case (S.div_share).
    // Divisions without range steps (div_inrange) in region B: there sin theta >= 0.75 and
    // 2^-55 < |cos theta| < 0.66, and with S.div_fast (0 < radius within 2^+-50),
    // 2^-100 < |r| < 2^100 and |r - radius| > 2^-40 radius (so |a| > 2^-42), every operand
    // and quotient of the five divisions is within 2^+-600 (schw_div_ok; device check of the
    // two forms at the predicate's edges: tests/test_gpu_arith.py
    // ::test_rhs_schwarzschild_fast_form_matches_ieee).  1 / (r r) takes its seed from the
    // refined 1 / r instead of a v_rcp_f64 of its own (rcp_seed.h: 16 cycles of the SIMD
    // against a multiply's 4, tools/valu_issue_cost.hip); the new intermediates are the seed
    // Y_r Y_r within 2^+-200 and its Newton residual 1 - (r r) Y_r Y_r within 2^-50 of 0,
    // both inside E with the box to spare (tests/test_gpu_rcp_seed.py).  S.unit_radius
    // (radius == 1.0 and S.div_fast, every black-hole scene of the reference): the third
    // form, value-identical there, so it needs no predicate of its own.
    if constexpr (MODE != 0) {
      double st, ct;
      if (glibc::sincos_b_table_ok(theta)) glibc::sincos_b_table(theta, &st, &ct);
      else glibc::sincos_b_taylor(theta, &st, &ct);
      if constexpr (MODE == 1) {  // the form the render takes for this scene
        if (S.unit_radius) body(st, ct, true, div_form<2>{});
        else body(st, ct, true, std::true_type{});
      } else body(st, ct, true, std::false_type{});
      return;
    }
#if GRT_SCALAR_VOTES
    with_sincos<GRT_FAST_DIV, GRT_UNIT_RADIUS, true>(theta, S.div_share, body, schw_div_ok_render_mask(S, r),
                                                     S.unit_radius != 0);
#else
    with_sincos<GRT_FAST_DIV, GRT_UNIT_RADIUS>(theta, S.div_share, body, schw_div_ok_render(S, r),
                                               S.unit_radius != 0);
#endif
  } else if constexpr (G == GRT_GEOM_EUCLIDEAN_SPHERICAL) {  // euclidean_spherical.rs:48-70
    double r = y[1], theta = y[2];
    double v_t = y[4], v_r = y[5], v_theta = y[6], v_phi = y[7];
    double st, ct;
    rsincos(theta, &st, &ct);
    o[0] = v_t;
    o[1] = v_r;
    o[2] = v_theta;
    o[3] = v_phi;
    o[4] = 0.0;
    o[5] = r * (v_theta * v_theta + v_phi * v_phi * st * st);
    o[6] = -(2.0 / r) * v_r * v_theta + st * ct * v_phi * v_phi;
    o[7] = -(2.0 / r) * v_phi * v_r - 2.0 * ct / st * v_theta * v_phi;
  } else if constexpr (G == GRT_GEOM_KERR_BL) {  // kerr_bl.rs:141-174
    double radius = S.radius, a = S.a, e = rc.e, l_z = rc.lz, q = rc.q;
    double r = y[1], theta = y[2];
    const double del = bl_delta(r, radius, a);
    auto body = [&](double st, double ct, bool, auto fdiv) {
      double r2a2 = r * r + a * a;
      double p_r = r2a2 * e - a * l_z;
      double sin2 = st * st;
      if constexpr (decltype(fdiv)::value) {
        double r2a2_del, a_del;
        div2_inrange(r2a2, a, del, &r2a2_del, &a_del);
        o[0] = r2a2_del * p_r + a * (l_z - a * e * sin2);
        o[1] = y[4];
        o[2] = y[5];
        o[3] = a_del * p_r + div_inrange(l_z, sin2) - a * e;
        double le = l_z - a * e;
        double carter = le * le + q;
        o[4] = (4.0 * r * e * p_r - (2.0 * r - radius) * carter) / 2.0;
        o[5] = (-2.0 * a * a * e * e * ct * st + div_inrange(2.0 * l_z * l_z * ct, st * (st * st))) / 2.0;
        o[6] = 0.0;
        o[7] = 0.0;
        return;
      }
      o[0] = r2a2 / del * p_r + a * (l_z - a * e * sin2);
      o[1] = y[4];
      o[2] = y[5];
      o[3] = a / del * p_r + l_z / sin2 - a * e;
      double le = l_z - a * e;
      double carter = le * le + q;
      o[4] = (4.0 * r * e * p_r - (2.0 * r - radius) * carter) / 2.0;
      o[5] = (-2.0 * a * a * e * e * ct * st + 2.0 * l_z * l_z * ct / (st * (st * st))) / 2.0;
      o[6] = 0.0;
      o[7] = 0.0;
    };
    // Divisions without range steps (div_inrange) in region B: there sin theta >= 0.75 and
    // 2^-55 < |cos theta| < 0.66, and with S.div_fast (radius, |a| within 2^+-50),
    // 2^-200 < |l_z| < 2^100, |r| < 2^100 and del within 2^+-300, every operand and
    // quotient of the four divisions is within 2^+-600 (bl_div_ok; device check:
    // tests/test_gpu_arith.py::test_rhs_kerr_bl_fast_form_matches_ieee).
    if constexpr (MODE != 0) {
      double st, ct;
      if (glibc::sincos_b_table_ok(theta)) glibc::sincos_b_table(theta, &st, &ct);
      else glibc::sincos_b_taylor(theta, &st, &ct);
      if constexpr (MODE == 1) body(st, ct, true, std::true_type{});
      else body(st, ct, true, std::false_type{});
      return;
    }
    with_sincos<GRT_FAST_DIV_BL>(theta, true, body, bl_div_ok(S, r, del, l_z));
  } else if constexpr (G == GRT_GEOM_KERR) {  // kerr.rs:200-241
    double radius = S.radius, a = S.a;
    double x = y[1], yy = y[2], z = y[3];
    double p[4] = {y[4], y[5], y[6], y[7]};
    auto body = [&](auto fd) {
      constexpr bool FD = decltype(fd)::value;
      double Gc[4][4];
      ks_metric_contra<FD>(radius, a, x, yy, z, Gc);
      double xdot[4];
      mat_vec(Gc, p, xdot);
      o[0] = xdot[0];
      o[1] = xdot[1];
      o[2] = xdot[2];
      o[3] = xdot[3];
      o[4] = 0.0;
      o[5] = ks_accel<FD>(radius, a, 1, x, yy, z, Gc, p);
      o[6] = ks_accel<FD>(radius, a, 2, x, yy, z, Gc, p);
      o[7] = ks_accel<FD>(radius, a, 3, x, yy, z, Gc, p);
    };
    if constexpr (MODE != 0) {
      if constexpr (MODE == 1) body(std::true_type{});
      else body(std::false_type{});
      return;
    }
#if GRT_FAST_DIV_KS
    // The metric quotients without v_div_scale (div_fx) when every lane's state passes
    // ks_fd_ok (wave-uniform, like the region-B forms above)
    if (S.div_fast && __ballot(!ks_fd_ok(a, x, yy, z, S.ks_cap)) == 0) {
      PATH_COUNT(0);
      body(std::true_type{});
      return;
    }
#endif
    PATH_COUNT(1);
    body(std::false_type{});
  } else {  // Euclidean, euclidean.rs:47-53
    o[0] = y[4];
    o[1] = y[5];
    o[2] = y[6];
    o[3] = y[7];
    o[4] = 0.0;
    o[5] = 0.0;
    o[6] = 0.0;
    o[7] = 0.0;
  }
}

// Lane K's value of v in every lane of its quad (DPP quad_perm [K,K,K,K], no LDS).
template <int K>
GDEV double quad_bcast(double v) {
  constexpr int ctrl = K | (K << 2) | (K << 4) | (K << 6);
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), ctrl, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), ctrl, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// rhs<KERR> on the 4 lanes of a quad (tail_kernel): every lane forms the contravariant
// metric and xdot as rhs<KERR> does; lane `sub` < 3 evaluates acceleration component
// sub + 1 (lane 3 repeats component 3), and the three components are broadcast across
// the quad.  Every value comes out of the same operations as in rhs<KERR>, so o is
// bit-identical in all four lanes; the quad's lanes must be active together.
template <bool FD>
GDEV void rhs_ks_quad_form(const DevScene& S, const double* y, double* o, int sub) {
  const double radius = S.radius, a = S.a;
  const double x = y[1], yy = y[2], z = y[3];
  const double p[4] = {y[4], y[5], y[6], y[7]};
  double Gc[4][4];
  ks_metric_contra<FD>(radius, a, x, yy, z, Gc);
  double xdot[4];
  mat_vec(Gc, p, xdot);
  const double acc = ks_accel<FD>(radius, a, sub < 3 ? sub + 1 : 3, x, yy, z, Gc, p);
  o[0] = xdot[0];
  o[1] = xdot[1];
  o[2] = xdot[2];
  o[3] = xdot[3];
  o[4] = 0.0;
  o[5] = quad_bcast<0>(acc);
  o[6] = quad_bcast<1>(acc);
  o[7] = quad_bcast<2>(acc);
}
// with rhs<KERR>'s range-free metric quotients and square roots when every lane's state
// passes ks_fd_ok (the quad's four lanes hold the same state)
GDEV void rhs_ks_quad(const DevScene& S, const double* y, double* o, int sub) {
#if GRT_FAST_DIV_KS
  if (S.div_fast && __ballot(!ks_fd_ok(S.a, y[1], y[2], y[3], S.ks_cap)) == 0) {
    rhs_ks_quad_form<true>(S, y, o, sub);
    return;
  }
#endif
  rhs_ks_quad_form<false>(S, y, o, sub);
}

template <int G, bool QUAD>
GDEV void rhs_sel(const DevScene& S, const RayConst& rc, const double* y, double* o, int sub) {
  if constexpr (QUAD) {
    static_assert(G == GRT_GEOM_KERR, "the quad-split RHS is the Kerr-Schild one");
    rhs_ks_quad(S, y, o, sub);
  } else {
    rhs<G>(S, rc, y, o);
  }
}
