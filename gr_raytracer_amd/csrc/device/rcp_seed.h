// rcp_seed.h — the range-free f64 division (geodesic_rhs.h div_inrange) taken apart, so that
// a reciprocal seed already in registers can stand in for v_rcp_f64.
//
// div_inrange(x, y) is  Y = refine2(y, rcp(y));  m = x Y;  q = fma(fma(-y, m, x), Y, m):
// two Newton steps on the hardware's reciprocal estimate (relative error eps0 <= 2^-20,
// far looser than the hardware's), then the quotient with one correction.  Each Newton step
// from a seed s = (1 - d) / y gives, before its one rounding, exactly (1 - d^2) / y, so
//   Y = RN((1 - e) / y),  0 <= e <= (eps0^2 + 2^-52)^2 ~ 2^-80,
// and the compiler's division is correct for every Y of that kind (its own Y is one).  A
// seed from another source is as good when its last Newton step starts within 2^-40 of
// 1 / y.  1 / (r r) from the refined Y_r ~ 1 / r:  Y_r Y_r is within 2^-50 of 1 / RN(r r)
// (Y_r within 2^-52 of 1 / r, the product and RN(r r) rounded once each), so ONE Newton
// step gives RN((1 - e) / y) with e <= 2^-100  (rcp_refine1).
// (1 / a and 1 / sin from one estimate of a sin, seeds R sin and R a, is exact as well but
// trades a 16-cycle v_rcp_f64 for three multiplies and measured no faster: DESIGN.md 3.)
// The one divisor for which Y matters to the last bit is a mantissa of all ones (1 / y lies
// 2^-106 above a rounding midpoint): there e >= 2^-105 keeps every such Y on the same side,
// the compiler's and these alike; RN(r r) has that mantissa for about one r in 2^52.
// Host restatement against `/` with a modelled estimate of relative error up to 2^-20:
// tests/test_rcp_seed.py; on the device against the compiler's division:
// tests/test_gpu_rcp_seed.py.
#pragma once

#if defined(__HIPCC__)
#define GRT_RCP_FN __device__ static inline __attribute__((always_inline))
#else
#include <cmath>
#define GRT_RCP_FN static inline
#endif

namespace grt {
namespace rcpseed {

// the four Newton FMAs of the compiler's f64 division, from seed s ~ 1 / y
GRT_RCP_FN double rcp_refine2(double y, double s) {
  const double fma0 = __builtin_fma(-y, s, 1.0);
  const double fma1 = __builtin_fma(s, fma0, s);
  const double fma2 = __builtin_fma(-y, fma1, 1.0);
  return __builtin_fma(fma1, fma2, fma1);
}
// its last two alone, for a seed already within 2^-40 of 1 / y
GRT_RCP_FN double rcp_refine1(double y, double s) {
  const double e = __builtin_fma(-y, s, 1.0);
  return __builtin_fma(s, e, s);
}
// x / y from the refined reciprocal Y: the division's last three instructions
GRT_RCP_FN double div_by_rcp(double x, double y, double Y) {
  const double m = x * Y;
  return __builtin_fma(__builtin_fma(-y, m, x), Y, m);
}

// The reciprocals of the region-B Schwarzschild RHS (schwarzschild.rs:54-80), whose five
// quotients are radius / r, 2 / r, a' = radius / (r r), a' / a with a = 1 - radius / r, and
// (2 cos) / sin.  RCP: the reciprocal estimate (v_rcp_f64 on the device).  Operand ranges:
// schw_div_ok and region B (geodesic_rhs.h).
// 1 / r and 1 / RN(r r) from one estimate
template <class RCP>
GRT_RCP_FN void rcp_r_rr(double r, double rr, RCP&& rcp, double* Yr, double* Yrr) {
  *Yr = rcp_refine2(r, rcp(r));
  *Yrr = rcp_refine1(rr, *Yr * *Yr);
}
// 1 / a and 1 / s, each from its own estimate
template <class RCP>
GRT_RCP_FN void rcp_pair(double a, double s, RCP&& rcp, double* Ya, double* Ys) {
  *Ya = rcp_refine2(a, rcp(a));
  *Ys = rcp_refine2(s, rcp(s));
}

// The first three quotients for radius == 1.0 (the unit of every black-hole scene of the
// reference; DevScene::unit_radius), from the same Y_r and Y_rr, each with the general
// form's bits:
//  * q = radius / r:  div_by_rcp(1.0, r, Y_r), whose m = 1.0 Y_r is Y_r itself (x 1.0 == x
//    for every x), so the multiply folds away and the two FMAs are the general form's.
//  * 2 / r = 2 q:  the general form is m2 = 2 Y_r, fma(fma(-r, m2, 2), Y_r, m2).  With
//    2^-100 < |r| < 2^100 every value of q's chain (Y_r, the residual fma(-r, Y_r, 1) within
//    2^-52 of 0 or exactly 0, the correction, q) is normal or zero and far from overflow, so
//    doubling each is exact and commutes with every rounding: m2 = 2 m, the residual
//    fma(-r, 2 m, 2) = 2 fma(-r, m, 1), and the result 2 q.  One exact multiply stands for a
//    multiply and two FMAs.
//  * a' = radius / (r r):  div_by_rcp(1.0, rr, Y_rr), the multiply folded as for q.
// a = 1 - q is the general form's own subtraction.  Host check against `/` with the modelled
// estimate: tests/test_rkf_zero_terms.py (tests/native/unit_radius_check.cpp); on the device
// the whole block against the IEEE form: rhs_check_kernel.
GRT_RCP_FN void unit_radius_quotients(double r, double rr, double Yr, double Yrr, double* q, double* two_over_r,
                                      double* a, double* a_prime) {
  *q = div_by_rcp(1.0, r, Yr);
  *two_over_r = 2.0 * *q;
  *a = 1.0 - *q;
  *a_prime = div_by_rcp(1.0, rr, Yrr);
}

}  // namespace rcpseed
}  // namespace grt
