// Host check of the RKF45 sums without their zero-weight k2 terms (geodesic_rkf.h
// rkf_attempt_fold, SHORT) against the full sums, in the reference's left-to-right order
// (runge_kutta.rs:94-124) with the device's weights (rkf_weights.h):
//   yn = y + CH1 a1 + CH2 a2 + CH3 a3 + CH4 a4 + CH5 a5 + CH6 a6,   CH2 = 0.0
//   e  =     CT1 a1 + CT2 a2 + CT3 a3 + CT4 a4 + CT5 a5 + CT6 a6,   CT2 = 0.0, used as e e.
// usage: rkf_zero_terms_check grid | rkf_zero_terms_check random N [SEED]
//   grid: all 11^7 combinations of y, a1..a6 from {+-0, +-1.5, +-5e-324, +-1e308, +-inf, NaN}
//   random: N tuples of special values and random doubles of every exponent
// prints "TUPLES DIFF_YN BAD_YN DIFF_E2" over the tuples with a2 finite: DIFF_YN those whose
// short and full yn differ in bits (two NaNs count as equal), BAD_YN those of them whose
// short yn is not -0, DIFF_E2 those whose e e differ.
// -DRKF_EXPLICIT_FMA: the sums as the compiler contracts them under -ffp-contract=fast
// (geodesic_fused.hip), each product fused into the add that takes it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rkf_weights.h"

using namespace grt;

static uint64_t bits(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  return u;
}
static bool same(double a, double b) { return bits(a) == bits(b) || (a != a && b != b); }

// volatile weights: the compiler must not fold 0.0 * a2 on the host either
static volatile double vCH2 = CH2, vCT2 = CT2;

#ifdef RKF_EXPLICIT_FMA
#define MADD(c, a, x) __builtin_fma((c), (a), (x))
#else
#define MADD(c, a, x) ((x) + (c) * (a))
#endif

template <bool SHORT>
static double sum_yn(double y, const double* a) {
  double s = MADD(CH1, a[0], y);
  if (!SHORT) s = MADD(vCH2, a[1], s);
  s = MADD(CH3, a[2], s);
  s = MADD(CH4, a[3], s);
  s = MADD(CH5, a[4], s);
  return MADD(CH6, a[5], s);
}
template <bool SHORT>
static double sum_e(const double* a) {
  double s = CT1 * a[0];
  if (!SHORT) s = MADD(vCT2, a[1], s);
  s = MADD(CT3, a[2], s);
  s = MADD(CT4, a[3], s);
  s = MADD(CT5, a[4], s);
  return MADD(CT6, a[5], s);
}

static long n_tuples, diff_yn, bad_yn, diff_e2;
static void check(double y, const double* a) {
  if (!std::isfinite(a[1])) return;  // the lemma's other part: a non-finite k2 reaches the outputs
  n_tuples++;
  const double ys = sum_yn<true>(y, a), yf = sum_yn<false>(y, a);
  if (!same(ys, yf)) {
    diff_yn++;
    if (bits(ys) != bits(-0.0)) {
      if (bad_yn < 5) fprintf(stderr, "yn differs, short %a full %a: y %a a %a %a %a %a %a %a\n", ys, yf, y, a[0], a[1], a[2], a[3], a[4], a[5]);
      bad_yn++;
    }
  }
  const double es = sum_e<true>(a), ef = sum_e<false>(a);
  if (!same(es * es, ef * ef)) {
    if (diff_e2 < 5) fprintf(stderr, "e e differs, short %a full %a: a %a %a %a %a %a %a\n", es, ef, a[0], a[1], a[2], a[3], a[4], a[5]);
    diff_e2++;
  }
}

static uint64_t g_s;
static uint64_t next() {  // splitmix64
  uint64_t z = (g_s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

int main(int argc, char** argv) {
  const double inf = INFINITY;
  const double V[11] = {0.0, -0.0, 1.5, -1.5, 5e-324, -5e-324, 1e308, -1e308, inf, -inf, NAN};
  if (argc > 1 && !strcmp(argv[1], "grid")) {
    int idx[7] = {0, 0, 0, 0, 0, 0, 0};
    while (true) {
      double a[6];
      for (int k = 0; k < 6; ++k) a[k] = V[idx[k + 1]];
      check(V[idx[0]], a);
      int k = 0;
      while (k < 7 && ++idx[k] == 11) idx[k++] = 0;
      if (k == 7) break;
    }
  } else if (argc > 2 && !strcmp(argv[1], "random")) {
    const long n = atol(argv[2]);
    g_s = argc > 3 ? strtoull(argv[3], nullptr, 0) : 0x5EEDull;
    for (long i = 0; i < n; ++i) {
      double v[7];
      for (int k = 0; k < 7; ++k) {
        double x;
        do {
          const uint64_t r = next();
          if ((r & 3) == 0) x = V[(r >> 2) % 11];  // a quarter special values
          else {
            const uint64_t u = next();  // any bit pattern: every exponent, subnormals, NaNs, both signs
            memcpy(&x, &u, 8);
          }
        } while (k == 2 && !std::isfinite(x));  // a2 finite, so that all N tuples count
        v[k] = x;
      }
      check(v[0], v + 1);
    }
  } else {
    fprintf(stderr, "usage: %s grid | random N [SEED]\n", argv[0]);
    return 2;
  }
  printf("%ld %ld %ld %ld\n", n_tuples, diff_yn, bad_yn, diff_e2);
  return 0;
}
