// geodesic_rkf.h — the second layer of geodesic.hip: one RKF45 attempt (rkf_attempt: the plain form
// and the running sums of rkf_attempt_fold) with its constants, and the LDS parking of the
// leading stages (kl_buf).  Included by every unit, after geodesic_rhs.h.

// runge_kutta.rs:16-84
constexpr double B21 = 2.0 / 9.0;
constexpr double B31 = 1.0 / 12.0, B32 = 1.0 / 4.0;
constexpr double B41 = 69.0 / 128.0, B42 = -243.0 / 128.0, B43 = 135.0 / 64.0;
constexpr double B51 = -17.0 / 12.0, B52 = 27.0 / 4.0, B53 = -27.0 / 5.0, B54 = 16.0 / 15.0;
constexpr double B61 = 65.0 / 432.0, B62 = -5.0 / 16.0, B63 = 13.0 / 16.0, B64 = 4.0 / 27.0,
                 B65 = 5.0 / 144.0;
// CH1..CH6, CT1..CT6 (CH2 = CT2 = 0.0): rkf_weights.h, shared with the host check
constexpr double BETA = 0.9;
constexpr double INV_ORDER = 1.0 / 5.0;
constexpr double SMALL_ERR = 1e-5;
constexpr int MAX_RETRY = 100;
constexpr double H_MAX = 1.0, H_MIN = 1e-12, H_GROWTH = 4.0;
constexpr double POW_SATURATED = 1800.0;  // (H_GROWTH / BETA)^5 = 1734.1, plus margin

// Number of state components that can be non-zero: KerrBL's y[6], y[7] are
// identically 0 (its RHS returns literal zeros), so every RKF term on them is an
// exact +-0 and the norm term a2 + a6 == a2; skipping them is bit-exact.
template <int G>
struct Dim {
  static constexpr int D = (G == GRT_GEOM_KERR_BL) ? 6 : 8;
};

// One rkf45_step (runge_kutta.rs:86-125).  Returns the SQUARED truncation error norm:
// the controller takes the (correctly rounded) sqrt only when the decision needs it.
// UNIT_H: every lane of the wave has h == 1.0 (H_MAX, the far field), where h * o is o
// itself (x * 1.0 == x for every finite and infinite x and keeps the sign of zero; a NaN
// stays a NaN, which stops the ray either way), so the eight products per stage go.
// Stage values k1..k4 parked in LDS (KLDS): slot j of component i of thread t at
// kl_buf[(j * 8 + i) * KL_STRIDE + t].  The Kerr-Schild attempt keeps 6 x 8 stage doubles
// live across RHS evaluations that need ~100 registers of their own; at 2 waves per SIMD
// (256 registers) the compiler spilled ~90 registers to scratch.  The reads take their
// offset through an empty asm that depends on the stage just computed, so the compiler
// neither forwards the stored registers (keeping them live) nor hoists the reads above
// that RHS evaluation.  Values are stored and re-read unchanged: the arithmetic is the same.
constexpr int KL_STRIDE = 256;
__shared__ double kl_buf[GRT_KL_STAGES * 8 * KL_STRIDE];  // 16 KB per stage, only in kernels that use it
GDEV void kl_put(int j, const double* k, int D, int skip = -1) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (i < D && i != skip) kl_buf[(j * 8 + i) * KL_STRIDE + (int)threadIdx.x] = k[i];
}
// threadIdx.x, opaque to the compiler and ordered after `dep`
GDEV int kl_slot_after(double dep) {
  int t = (int)threadIdx.x;
  __asm__ volatile("" : "+v"(t) : "v"(dep));
  return t;
}
GDEV double kl_get(int t, int j, int i) { return kl_buf[(j * 8 + i) * KL_STRIDE + t]; }

// State components the RHS reads (the others -- t, and phi where the metric does not
// depend on it -- only receive stage values, so their stage inputs are never formed).
template <int G>
GDEV constexpr bool rhs_reads(int i) {
  if (G == GRT_GEOM_EUCLIDEAN) return i >= 4;
  if (G == GRT_GEOM_KERR) return i >= 1;
  return i == 1 || i == 2 || i >= 4;  // Schwarzschild, EuclideanSpherical, KerrBL: r, theta, velocities
}

// The state component whose derivative the RHS sets to the constant 0.0, or -1: p_t in
// Kerr-Schild (kerr.rs:233-241, the metric does not depend on t).  Its stage values are
// k_j = h * 0.0 = kz for every stage j of an attempt (kz = +0 for h > 0), so each of
// rkf45_step's left-to-right sums for it, y + c_1 kz + ... + c_m kz, is a sum of signed
// zeros (or NaNs) onto y, and IEEE addition gives it in one step: y + kz when every
// coefficient is >= 0 (each term carries kz's sign), y + kz * kz when the signs are mixed
// (some term is +0, which makes any later zero sum +0; kz * kz is +0, or NaN for a NaN
// kz).  Its error term (a mixed sum, no y) squares to +0: kz * kz as well.  Same bits as
// the full sums for every y, signed zeros and NaN included.
template <int G>
GDEV constexpr int zero_k() {
  return G == GRT_GEOM_KERR ? 4 : -1;
}

// nalgebra norm(): 8-accumulator unrolled dot, ((a0+a4) + (a1+a5)) + (a2+a6) + (a3+a7)
// z >= 0: e[z] * e[z] is given as zz (zero_k)
template <int D>
GDEV double err_norm_sq(const double* e, int z = -1, double zz = 0.0) {
  double res;
  if constexpr (D == 8) {
    double sq[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sq[i] = (i == z) ? zz : e[i] * e[i];
    res = sq[0] + sq[4];
    res += sq[1] + sq[5];
    res += sq[2] + sq[6];
    res += sq[3] + sq[7];
  } else {
    res = e[0] * e[0] + e[4] * e[4];
    res += e[1] * e[1] + e[5] * e[5];
    res += e[2] * e[2];
    res += e[3] * e[3];
  }
  return res;
}

// rkf45_step with every left-to-right sum of runge_kutta.rs:94-124 evaluated as a running
// sum as soon as its terms exist.  The sums are the reference's, term by term in the same
// order ((y + B61*k1) + B62*k2) + ..., so every value is bit-identical to rkf_attempt_full;
// what changes is how many stage values are live across an RHS evaluation:
//   - a component the RHS does not read (rhs_reads) folds k_j into y_new and the error
//     right away: 2 live values instead of up to 6;
//   - the others keep k1..k3 until k4 exists, then fold k1..k4 into the stage-5 input, the
//     stage-6 partial, y_new and the error: 3 live values across RHS 5 and 2 across RHS 6,
//     instead of 4 and 5.
//
// SHORT: the sums without their k2 terms.  The Fehlberg weights CH2 and CT2 are 0.0, but
// without fast-math `X + 0.0 * k2` stays a multiply and an add (0 * k2 is -0, or NaN for a
// non-finite k2, and X + (+-0) can turn a -0 into +0): 24 instructions per attempt that
// change a result bit only in the cases of this lemma.
//   Lemma (Schwarzschild chart; 0 < h <= 1, which rclamp to [H_MIN, H_MAX] gives).
//   If every yn'[i] of the short attempt is finite and not -0 and its err_sq' is finite,
//   then yn and err_sq of the full attempt have the same bits.  (rkf_short_ok)
// Proof.  Both forms compute the same k1..k6 (the stage inputs never hold a CH / CT term).
//  * Zeros, a2 = k2[i] finite: t = 0.0 * a2 is +-0, and X + t differs from X only for
//    X = -0 with t = +0 (a2 sign-positive), giving +0.  The running sums then add the same
//    later terms to -0 (short) and +0 (full): the first non-zero term makes them equal for
//    good, and while every later term is a zero the short sum is -0 (all of them -0) or
//    both are +0.  So a difference that survives to yn shows as yn'[i] = -0 against
//    yn[i] = +0, which the premise excludes.  The same holds for e[i], where it is a
//    difference in the sign of a zero only, and e[i] enters err_sq as e[i] * e[i] alone:
//    err_sq needs no premise beyond the one on a2.
//  * a2 not finite: then 0.0 * a2 is NaN and yn[i], e[i] of the full form are NaN.  In this
//    chart o[0..3] are the stage input's velocities (rhs: o[i] = y[4 + i]), so the short
//    outputs are non-finite as well, against the premise:
//      i >= 4: tmp3[i] = y[i] + B31 k1[i] + B32 k2[i] is non-finite (B32 != 0, and no sum
//        of non-finite terms is finite), hence k3[i - 4] = h tmp3[i], hence yn'[i - 4]
//        through CH3 k3[i - 4] (CH3 != 0).
//      i < 4: k2[i] = h v with v = y[4 + i] + B21 k1[4 + i], stage 2's input velocity, and
//        h <= 1, so v is non-finite.  Either y[4 + i] or k1[4 + i] is non-finite, hence
//        yn'[4 + i] = y[4 + i] + CH1 k1[4 + i] + ... (CH1 != 0); or both are finite and the
//        sum overflowed (two values near 1e308), which can leave yn'[4 + i] finite: but then
//        stage 2's o[5] holds a term (coefficient) v v, non-finite whatever the coefficient
//        (inf times 0 is NaN), so k2[5] is non-finite and the case i >= 4 gives yn'[1].
// The identities hold under FMA contraction too: fma(0.0, a2, X) follows the same zero and
// NaN rules (geodesic_fused.hip).  Host check over every combination of the special values:
// tests/test_rkf_zero_terms.py; device check of both forms: tests/test_gpu_rkf_short.py.
// KerrBL is out of scope: its k2[0] and k2[3] come from formulas (l_z / sin^2 ...) and reach
// nothing but the dropped terms (o[6] = o[7] = 0 and the RHS reads neither t nor phi), so a
// non-finite k2[0] or k2[3] can leave the short outputs finite where the full sum is NaN.
template <int G, bool UNIT_H, bool QUAD, int NKL, bool SHORT = false>
GDEV double rkf_attempt_fold(const DevScene& S, const RayConst& rc, const double* y, double h, double* yn,
                             int sub) {
  static_assert(!SHORT || G == GRT_GEOM_SCHWARZSCHILD, "short RKF sums: the lemma is the Schwarzschild chart's");
  constexpr int D = Dim<G>::D;
  double k1[8], k2[8], k3[8], k4[8], k5[8], k6[8], tmp[8], o[8], p6[8], e[8];
  int t = 0;  // LDS slot, re-derived after each stage (kl_slot_after)
#define KV(j, i) (((j) <= NKL) ? kl_get(t, (j) - 1, (i)) : k##j[i])
#define STAGE(kj)                                                   \
  _Pragma("unroll") for (int i = 0; i < D; ++i) kj[i] = UNIT_H ? o[i] : h * o[i];
  rhs_sel<G, QUAD>(S, rc, y, o, sub);
  STAGE(k1)
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (!rhs_reads<G>(i)) {
      yn[i] = y[i] + CH1 * k1[i];
      e[i] = CT1 * k1[i];
    }
  if (NKL >= 1) kl_put(0, k1, D);
#pragma unroll
  for (int i = 0; i < D; ++i) tmp[i] = y[i] + B21 * k1[i];
  if (D < 8) { tmp[6] = 0.0; tmp[7] = 0.0; }
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
  STAGE(k2)
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (!rhs_reads<G>(i) && !SHORT) {
      yn[i] = yn[i] + CH2 * k2[i];
      e[i] = e[i] + CT2 * k2[i];
    }
  if (NKL >= 2) kl_put(1, k2, D);
  if (NKL >= 1) t = kl_slot_after(k2[D - 1]);
#pragma unroll
  for (int i = 0; i < D; ++i) tmp[i] = y[i] + B31 * KV(1, i) + B32 * k2[i];
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
  STAGE(k3)
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (!rhs_reads<G>(i)) {
      yn[i] = yn[i] + CH3 * k3[i];
      e[i] = e[i] + CT3 * k3[i];
    }
  if (NKL >= 3) kl_put(2, k3, D);
  if (NKL >= 1) t = kl_slot_after(k3[D - 1]);
#pragma unroll
  for (int i = 0; i < D; ++i) tmp[i] = y[i] + B41 * KV(1, i) + B42 * KV(2, i) + B43 * k3[i];
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
  STAGE(k4)
  if (NKL >= 1) t = kl_slot_after(k4[D - 1]);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    if (!rhs_reads<G>(i)) {
      yn[i] = yn[i] + CH4 * k4[i];
      e[i] = e[i] + CT4 * k4[i];
    } else {
      const double a1 = KV(1, i), a2 = KV(2, i), a3 = KV(3, i), a4 = k4[i];
      tmp[i] = y[i] + B51 * a1 + B52 * a2 + B53 * a3 + B54 * a4;
      p6[i] = y[i] + B61 * a1 + B62 * a2 + B63 * a3 + B64 * a4;
      if constexpr (SHORT) {
        yn[i] = y[i] + CH1 * a1 + CH3 * a3 + CH4 * a4;
        e[i] = CT1 * a1 + CT3 * a3 + CT4 * a4;
      } else {
        yn[i] = y[i] + CH1 * a1 + CH2 * a2 + CH3 * a3 + CH4 * a4;
        e[i] = CT1 * a1 + CT2 * a2 + CT3 * a3 + CT4 * a4;
      }
    }
  }
  if (D < 8) { tmp[6] = 0.0; tmp[7] = 0.0; }
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
  STAGE(k5)
#pragma unroll
  for (int i = 0; i < D; ++i) {
    if (rhs_reads<G>(i)) tmp[i] = p6[i] + B65 * k5[i];
    yn[i] = yn[i] + CH5 * k5[i];
    e[i] = e[i] + CT5 * k5[i];
  }
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
  STAGE(k6)
#pragma unroll
  for (int i = 0; i < D; ++i) {
    yn[i] = yn[i] + CH6 * k6[i];
    e[i] = e[i] + CT6 * k6[i];
  }
#undef STAGE
#undef KV
  if (D < 8) {
    yn[6] = 0.0;
    yn[7] = 0.0;
  }
  return err_norm_sq<D>(e);
}

// QUAD: the Kerr-Schild RHS split over a quad (rhs_ks_quad), `sub` = lane & 3.
// NKL: stages k1..k_NKL kept in LDS (see kl_put), 0 = none.
// SHORT: without the zero-weight k2 terms (rkf_attempt_fold's lemma; the caller checks
// rkf_short_ok and takes the attempt again in the full form where it fails).
template <int G, bool UNIT_H = false, bool QUAD = false, int NKL = 0, bool SHORT = false>
GDEV double rkf_attempt(const DevScene& S, const RayConst& rc, const double* y, double h,
                        double* yn, int sub = 0) {
  static_assert(!SHORT || (GRT_RK_FOLD && G == GRT_GEOM_SCHWARZSCHILD), "short RKF sums: rkf_attempt_fold only");
  // Kerr-Schild keeps the plain form: its stages k1..k4 sit in LDS (NKL), which frees
  // more registers than the running sums (measured: 17 -> 122 spilled VGPRs with them)
  if constexpr (GRT_RK_FOLD && G != GRT_GEOM_KERR) {
    return rkf_attempt_fold<G, UNIT_H, QUAD, NKL, SHORT>(S, rc, y, h, yn, sub);
  }
  constexpr int D = Dim<G>::D;
  constexpr int Z = zero_k<G>();  // component with k_j = kz in every stage (zero_k)
  double k1[8], k2[8], k3[8], k4[8], k5[8], k6[8], tmp[8], o[8];
  int t = 0;  // LDS slot, re-derived after each stage (kl_slot_after)
  // stage j's value k_j[i] (from LDS when parked there)
#define KV(j, i) (((j) <= NKL) ? kl_get(t, (j) - 1, (i)) : k##j[i])
  rhs_sel<G, QUAD>(S, rc, y, o, sub);
  // signs: B21 > 0; B31, B32 > 0; B4x, B5x, B6x mixed; CH1..CH6 >= 0; CT mixed
  const double kz = Z < 0 ? 0.0 : (UNIT_H ? o[Z < 0 ? 0 : Z] : h * o[Z < 0 ? 0 : Z]);
  const double kzz = kz * kz;
#pragma unroll
  for (int i = 0; i < D; ++i) k1[i] = UNIT_H ? o[i] : h * o[i];
  if (NKL >= 1) kl_put(0, k1, D, Z);
#pragma unroll
  for (int i = 0; i < D; ++i) tmp[i] = (i == Z) ? y[i] + kz : y[i] + B21 * k1[i];
  if (D < 8) { tmp[6] = 0.0; tmp[7] = 0.0; }
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
#pragma unroll
  for (int i = 0; i < D; ++i) k2[i] = UNIT_H ? o[i] : h * o[i];
  if (NKL >= 2) kl_put(1, k2, D, Z);
  if (NKL >= 1) t = kl_slot_after(k2[D - 1]);
#pragma unroll
  for (int i = 0; i < D; ++i) tmp[i] = (i == Z) ? y[i] + kz : y[i] + B31 * KV(1, i) + B32 * k2[i];
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
#pragma unroll
  for (int i = 0; i < D; ++i) k3[i] = UNIT_H ? o[i] : h * o[i];
  if (NKL >= 3) kl_put(2, k3, D, Z);
  if (NKL >= 1) t = kl_slot_after(k3[D - 1]);
#pragma unroll
  for (int i = 0; i < D; ++i)
    tmp[i] = (i == Z) ? y[i] + kzz : y[i] + B41 * KV(1, i) + B42 * KV(2, i) + B43 * k3[i];
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
#pragma unroll
  for (int i = 0; i < D; ++i) k4[i] = UNIT_H ? o[i] : h * o[i];
  if (NKL >= 4) kl_put(3, k4, D, Z);
  if (NKL >= 1) t = kl_slot_after(k4[D - 1]);
#pragma unroll
  for (int i = 0; i < D; ++i)
    tmp[i] = (i == Z) ? y[i] + kzz : y[i] + B51 * KV(1, i) + B52 * KV(2, i) + B53 * KV(3, i) + B54 * k4[i];
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
#pragma unroll
  for (int i = 0; i < D; ++i) k5[i] = UNIT_H ? o[i] : h * o[i];
  if (NKL >= 1) t = kl_slot_after(k5[D - 1]);
#pragma unroll
  for (int i = 0; i < D; ++i)
    tmp[i] = (i == Z) ? y[i] + kzz
                      : y[i] + B61 * KV(1, i) + B62 * KV(2, i) + B63 * KV(3, i) + B64 * KV(4, i) + B65 * k5[i];
  rhs_sel<G, QUAD>(S, rc, tmp, o, sub);
#pragma unroll
  for (int i = 0; i < D; ++i) k6[i] = UNIT_H ? o[i] : h * o[i];
  if (NKL >= 1) t = kl_slot_after(k6[D - 1]);
  double e[8];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    if (i == Z) {  // e[Z] only enters the norm as e[Z]^2 = kz * kz
      yn[i] = y[i] + kz;
      e[i] = 0.0;
      continue;
    }
    const double a1 = KV(1, i), a2 = KV(2, i), a3 = KV(3, i), a4 = KV(4, i);
    yn[i] = y[i] + CH1 * a1 + CH2 * a2 + CH3 * a3 + CH4 * a4 + CH5 * k5[i] + CH6 * k6[i];
    e[i] = CT1 * a1 + CT2 * a2 + CT3 * a3 + CT4 * a4 + CT5 * k5[i] + CT6 * k6[i];
  }
#undef KV
  if (D < 8) {
    yn[6] = 0.0;
    yn[7] = 0.0;
  }
  return err_norm_sq<D>(e, Z, kzz);
}
