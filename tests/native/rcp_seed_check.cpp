// Host check of the seeded reciprocals of the region-B Schwarzschild RHS
// (gr_raytracer_amd/csrc/device/rcp_seed.h) against the compiler's `/` (IEEE on the host).
// The hardware's reciprocal estimate is modelled as (1 / y)(1 + e), e uniform within
// +-2^-20: looser than any plausible v_rcp_f64.  usage: rcp_seed_check N [SEED]
// prints "N BAD", BAD the operand sets with any quotient differing from `/`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rcp_seed.h"

static uint64_t g_s;
static uint64_t next() {  // splitmix64
  uint64_t z = (g_s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static double uni() { return (double)(next() >> 11) * 0x1p-53; }  // [0, 1)
static double sign() { return (next() & 1) ? -1.0 : 1.0; }
static uint64_t bits(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  return u;
}
// |v| log-uniform in [2^lo, 2^hi) with a random mantissa; 15% of the draws within a few
// ulps of either edge.  The upper edge stops two ulps short: for a divisor whose mantissa is
// all ones (the one exception of Markstein's theorem on the final correction step), whether
// the sequence -- the unchanged one for x / r as well -- returns the quotient depends on
// which estimate the reciprocal instruction returns there, and the random model here does
// not know; that divisor is checked with the instruction itself (tests/test_gpu_rcp_seed.py,
// and every exponent in tests/test_gpu_arith.py's map).
static double edge(int lo, int hi) {
  const double k = uni();
  if (k < 0.15) return ldexp(1.0 + (double)(next() & 3) * 0x1p-52, lo);
  if (k > 0.85) return ldexp(2.0 - (double)(2 + (next() & 3)) * 0x1p-52, hi - 1);
  return ldexp(1.0 + uni(), lo + (int)(next() % (uint64_t)(hi - lo)));
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 1000000;
  g_s = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x5EEDull;
  auto rcp = [](double y) { return (1.0 / y) * (1.0 + (uni() - 0.5) * 0x1p-19); };
  long bad = 0;
  for (long i = 0; i < n; ++i) {
    // the ranges of schw_div_ok and region B: 2^-100 < |r| < 2^100, radius within 2^+-50,
    // |a| > 2^-42, sin in [0.75, 1], 2^-55 < |cos| < 0.66
    const double radius = edge(-50, 50);
    const double r = (i & 3) ? radius * (1.0 + ldexp(1.0 + uni(), -(int)(next() % 40)) * sign()) * ((i & 4) ? 1.0 : edge(0, 20))
                             : edge(-100, 100) * sign();
    const double st = (i & 8) ? 0.75 + 0.25 * uni() : ((i & 16) ? 0.75 : 1.0 - (double)(next() & 7) * 0x1p-53);
    const double ct = ((i & 32) ? ldexp(1.0 + uni(), -55 + (int)(next() % 54)) : 0.66 * uni() + 0x1p-54) * sign();
    using namespace grt::rcpseed;
    const double rr = r * r, two_ct = 2.0 * ct;
    double Yr, Yrr, Ya, Yst;
    rcp_r_rr(r, rr, rcp, &Yr, &Yrr);
    const double radius_over_r = div_by_rcp(radius, r, Yr);
    // a as the RHS forms it, or independent of r on the predicate's edge |a| = 2^-42
    double a = 1.0 - radius_over_r;
    if ((i & 192) == 192 || !(a > 0x1p-42 || a < -0x1p-42)) a = ldexp(1.0 + (double)(next() & 7) * 0x1p-52, -42) * sign();
    rcp_pair(a, st, rcp, &Ya, &Yst);
    const double a_prime = div_by_rcp(radius, rr, Yrr);
    int f = 0;
    f |= bits(radius_over_r) != bits(radius / r);
    f |= bits(div_by_rcp(2.0, r, Yr)) != bits(2.0 / r);
    f |= bits(a_prime) != bits(radius / rr);
    f |= bits(div_by_rcp(a_prime, a, Ya)) != bits(a_prime / a);
    f |= bits(div_by_rcp(two_ct, st, Yst)) != bits(two_ct / st);
    if (f && bad < 5)
      fprintf(stderr, "differs: r %a radius %a a %a st %a ct %a\n", r, radius, a, st, ct);
    bad += f;
  }
  printf("%ld %ld\n", n, bad);
  return 0;
}
