// orbit_uv_main.cpp — a stand-alone caller of grt_orbit_rate / grt_gbuffer_orbit_uv for CPU
// sanitizer builds: no GPU, no Python, no libgrt.so.  Build it with the two host files it
// needs and run it:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/orbit_uv_main.cpp gr_raytracer_amd/csrc/host/orbit.cpp \
//       gr_raytracer_amd/csrc/host/errors.cpp -o orbit_uv_main && ./orbit_uv_main
//
// It calls the rule on synthetic layer arrays (a disc and a sphere, seeded) whose sizes
// include 0 and 1, with separate and with aliased outputs, on exactly sized heap arrays (so
// an access past an end is the sanitizer's to report), checks the properties that need no
// reference (sphere layers and t = 0 unchanged, aliased == separate, the rotation keeps the
// distance from (0.5, 0.5)), and runs every -EINVAL.  Exit status 0 and "ok" on success.
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "grt_api.h"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond);  \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // xorshift64*, [0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0);
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), 8 * a.size()) == 0);
}

int main() {
  grt_gbuffer_shape shape;
  std::memset(&shape, 0, sizeof(shape));
  shape.geometry = GRT_GEOM_KERR_BL;
  shape.n_objects = 2;
  shape.radius = 1.0;
  shape.a = 0.499;
  shape.objects[0].kind = GRT_OBJ_DISC;
  shape.objects[1].kind = GRT_OBJ_SPHERE;
  const double times[] = {0.0, 1.0, 37.5, -12.25, 1e4};
  double one = 1.0;  // a valid address for the empty arrays' pointers
  for (uint64_t n : {0ull, 1ull, 7ull, 1000ull}) {
    std::vector<uint8_t> object(n);
    std::vector<double> u(n), v(n), radius(n);
    for (uint64_t k = 0; k < n; ++k) {
      object[k] = uniform() < 0.7 ? 0 : 1;
      const double rho = 0.5 * uniform(), phi = 6.283185307179586 * uniform();
      u[k] = 0.5 + rho * std::cos(phi);
      v[k] = 0.5 + rho * std::sin(phi);
      radius[k] = object[k] == 0 ? 2.0 + 8.0 * uniform() : 0.0;
    }
    const uint8_t* po = n ? object.data() : (const uint8_t*)&one;
    const double *pu = n ? u.data() : &one, *pv = n ? v.data() : &one, *pr = n ? radius.data() : &one;
    for (double t : times) {
      std::vector<double> uo(n), vo(n);
      CHECK(grt_gbuffer_orbit_uv(&shape, n, po, pu, pv, pr, t, n ? uo.data() : &one, n ? vo.data() : &one) == 0);
      std::vector<double> ua = u, va = v;  // aliased: the outputs are the inputs
      CHECK(grt_gbuffer_orbit_uv(&shape, n, po, n ? ua.data() : &one, n ? va.data() : &one, pr, t,
                                 n ? ua.data() : &one, n ? va.data() : &one) == 0);
      CHECK(same_bits(ua, uo) && same_bits(va, vo));
      if (t == 0.0) CHECK(same_bits(uo, u) && same_bits(vo, v));
      for (uint64_t k = 0; k < n; ++k) {
        if (object[k] == 1) {
          CHECK(std::memcmp(&uo[k], &u[k], 8) == 0 && std::memcmp(&vo[k], &v[k], 8) == 0);
          continue;
        }
        const double before = std::hypot(u[k] - 0.5, v[k] - 0.5), after = std::hypot(uo[k] - 0.5, vo[k] - 0.5);
        CHECK(std::fabs(after - before) <= 1e-15);
      }
    }
  }
  double omega = -1.0;
  CHECK(grt_orbit_rate(GRT_GEOM_SCHWARZSCHILD, 1.0, 0.0, 6.0, &omega) == 0 && omega > 0.0);
  CHECK(grt_orbit_rate(GRT_GEOM_EUCLIDEAN, 1.0, 0.0, 6.0, &omega) == 0 && omega == 0.0 && !std::signbit(omega));
  CHECK(grt_orbit_rate(99, 1.0, 0.0, 6.0, &omega) == -EINVAL);
  CHECK(grt_orbit_rate(GRT_GEOM_KERR, 1.0, 0.0, 6.0, nullptr) == -EINVAL);
  // every -EINVAL of grt_gbuffer_orbit_uv; the outputs stay as they were
  {
    uint8_t obj[2] = {0, 1};
    double a[2] = {0.6, 0.7}, b[2] = {0.4, 0.3}, r[2] = {5.0, 0.0}, o1[2] = {9.0, 9.0}, o2[2] = {9.0, 9.0};
    CHECK(grt_gbuffer_orbit_uv(nullptr, 2, obj, a, b, r, 1.0, o1, o2) == -EINVAL);
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, nullptr, a, b, r, 1.0, o1, o2) == -EINVAL);
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, obj, nullptr, b, r, 1.0, o1, o2) == -EINVAL);
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, obj, a, nullptr, r, 1.0, o1, o2) == -EINVAL);
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, obj, a, b, nullptr, 1.0, o1, o2) == -EINVAL);
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, obj, a, b, r, 1.0, nullptr, o2) == -EINVAL);
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, obj, a, b, r, 1.0, o1, nullptr) == -EINVAL);
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, obj, a, b, r, NAN, o1, o2) == -EINVAL);
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, obj, a, b, r, INFINITY, o1, o2) == -EINVAL);
    obj[1] = 2;  // past shape.n_objects
    CHECK(grt_gbuffer_orbit_uv(&shape, 2, obj, a, b, r, 1.0, o1, o2) == -EINVAL);
    CHECK(o1[0] == 9.0 && o1[1] == 9.0 && o2[0] == 9.0 && o2[1] == 9.0);
    CHECK(std::strlen(grt_last_error()) > 0);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
