// lapse_main.cpp — a stand-alone caller of grt_gbuffer_orbit_uv_retarded and of the lapse
// sidecar's writer and reader for CPU sanitizer builds: no GPU, no Python, no libgrt.so.
// Build it with the three host files it needs and run it:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/lapse_main.cpp gr_raytracer_amd/csrc/host/orbit.cpp \
//       gr_raytracer_amd/csrc/host/gbuffer.cpp gr_raytracer_amd/csrc/host/errors.cpp -o lapse_main \
//     && ./lapse_main SCRATCH_DIR
//
// The retarded rule on synthetic layer arrays (a disc and a sphere, seeded) of 0, 1, 7 and 1000
// layers, with separate and with aliased outputs, on exactly sized heap arrays (so an access
// past an end is the sanitizer's to report): lapse == 0 is grt_gbuffer_orbit_uv at the same
// time, lapse == c is grt_gbuffer_orbit_uv at the double time + c, sphere layers stay, and
// every -EINVAL leaves the outputs alone.  The sidecar: a round trip with 0 and with 5 layers,
// then every truncation of the small file, a byte too many, a sidecar of another buffer, a
// wrong count and a non-finite entry, each -EINVAL with the caller's array untouched.
// Files go to SCRATCH_DIR (default "."), and are removed.  Exit status 0 and "ok" on success.
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
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

static std::vector<char> slurp(const std::string& path) {
  std::vector<char> out;
  if (FILE* f = std::fopen(path.c_str(), "rb")) {
    char buf[4096];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + k);
    std::fclose(f);
  }
  return out;
}
static bool spit(const std::string& path, const char* p, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = n == 0 || std::fwrite(p, 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}

static void retarded_rule() {
  grt_gbuffer_shape shape;
  std::memset(&shape, 0, sizeof(shape));
  shape.geometry = GRT_GEOM_KERR_BL;
  shape.n_objects = 2;
  shape.radius = 1.0;
  shape.a = 0.499;
  shape.objects[0].kind = GRT_OBJ_DISC;
  shape.objects[1].kind = GRT_OBJ_SPHERE;
  const double times[] = {0.0, 1.0, 37.5, -12.25};
  double one = 1.0;  // a valid address for the empty arrays' pointers
  for (uint64_t n : {0ull, 1ull, 7ull, 1000ull}) {
    std::vector<uint8_t> object(n);
    std::vector<double> u(n), v(n), radius(n), lapse(n), zero(n, 0.0), same(n, -41.625);
    for (uint64_t k = 0; k < n; ++k) {
      object[k] = uniform() < 0.7 ? 0 : 1;
      const double rho = 0.5 * uniform(), phi = 6.283185307179586 * uniform();
      u[k] = 0.5 + rho * std::cos(phi);
      v[k] = 0.5 + rho * std::sin(phi);
      radius[k] = object[k] == 0 ? 2.0 + 8.0 * uniform() : 0.0;
      lapse[k] = -60.0 * uniform();
    }
    const uint8_t* po = n ? object.data() : (const uint8_t*)&one;
    const double *pu = n ? u.data() : &one, *pv = n ? v.data() : &one, *pr = n ? radius.data() : &one;
    auto at = [&](std::vector<double>& x) { return n ? x.data() : &one; };
    for (double t : times) {
      std::vector<double> uo(n), vo(n), uf(n), vf(n);
      // lapse == 0: the fast-light rule at t
      CHECK(grt_gbuffer_orbit_uv_retarded(&shape, n, po, pu, pv, pr, at(zero), t, at(uo), at(vo)) == 0);
      CHECK(grt_gbuffer_orbit_uv(&shape, n, po, pu, pv, pr, t, at(uf), at(vf)) == 0);
      CHECK(same_bits(uo, uf) && same_bits(vo, vf));
      // lapse == c: the fast-light rule at the double t + c
      CHECK(grt_gbuffer_orbit_uv_retarded(&shape, n, po, pu, pv, pr, at(same), t, at(uo), at(vo)) == 0);
      CHECK(grt_gbuffer_orbit_uv(&shape, n, po, pu, pv, pr, t + -41.625, at(uf), at(vf)) == 0);
      CHECK(same_bits(uo, uf) && same_bits(vo, vf));
      // a lapse per layer: separate and aliased outputs agree, sphere layers stay
      CHECK(grt_gbuffer_orbit_uv_retarded(&shape, n, po, pu, pv, pr, at(lapse), t, at(uo), at(vo)) == 0);
      std::vector<double> ua = u, va = v;
      CHECK(grt_gbuffer_orbit_uv_retarded(&shape, n, po, at(ua), at(va), pr, at(lapse), t, at(ua), at(va)) == 0);
      CHECK(same_bits(ua, uo) && same_bits(va, vo));
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
  // every -EINVAL; the outputs stay as they were
  uint8_t obj[2] = {0, 1};
  double a[2] = {0.6, 0.7}, b[2] = {0.4, 0.3}, r[2] = {5.0, 0.0}, l[2] = {-3.0, -4.0}, o1[2] = {9.0, 9.0},
         o2[2] = {9.0, 9.0};
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, l, 1.0, o1, o2) == 0);
  o1[0] = o1[1] = o2[0] = o2[1] = 9.0;
  CHECK(grt_gbuffer_orbit_uv_retarded(nullptr, 2, obj, a, b, r, l, 1.0, o1, o2) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, nullptr, a, b, r, l, 1.0, o1, o2) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, nullptr, b, r, l, 1.0, o1, o2) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, nullptr, r, l, 1.0, o1, o2) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, nullptr, l, 1.0, o1, o2) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, nullptr, 1.0, o1, o2) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, l, 1.0, nullptr, o2) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, l, 1.0, o1, nullptr) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, l, NAN, o1, o2) == -EINVAL);
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, l, -INFINITY, o1, o2) == -EINVAL);
  l[1] = NAN;
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, l, 1.0, o1, o2) == -EINVAL);
  l[1] = INFINITY;
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, l, 1.0, o1, o2) == -EINVAL);
  l[1] = -4.0;
  obj[1] = 2;  // past shape.n_objects
  CHECK(grt_gbuffer_orbit_uv_retarded(&shape, 2, obj, a, b, r, l, 1.0, o1, o2) == -EINVAL);
  CHECK(o1[0] == 9.0 && o1[1] == 9.0 && o2[0] == 9.0 && o2[1] == 9.0);
  CHECK(std::strlen(grt_last_error()) > 0);
}

static grt_gbuffer_info small_info(uint64_t n_layers) {
  grt_gbuffer_info info;
  std::memset(&info, 0, sizeof(info));
  info.rows = 3;
  info.cols = 2;
  info.n_pixels = 6;
  info.n_layers = n_layers;
  info.device = 5;  // a load changes it: not part of what binds the sidecar
  info.shape.geometry = GRT_GEOM_SCHWARZSCHILD;
  info.shape.n_objects = 1;
  info.shape.radius = 1.0;
  info.camera.rows = 3;
  info.camera.cols = 2;
  return info;
}

static void sidecar(const std::string& dir) {
  const std::string path = dir + "/lapse_main.grtg.lapse", cut = dir + "/lapse_main.cut.lapse";
  {  // no layers
    grt_gbuffer_info info = small_info(0);
    CHECK(grt_gbuffer_lapse_write_file(path.c_str(), &info, nullptr, 0) == 0);
    CHECK(grt_gbuffer_lapse_read_file(path.c_str(), &info, nullptr) == 0);
    double none = 9.0;
    CHECK(grt_gbuffer_lapse_read_file(path.c_str(), &info, &none) == 0 && none == 9.0);
  }
  grt_gbuffer_info info = small_info(5);
  const std::vector<double> lapse = {-1.5, -0.0, -17.25, -1e-300, -52.0};
  CHECK(grt_gbuffer_lapse_write_file(path.c_str(), &info, lapse.data(), 5) == 0);
  {
    std::vector<double> back(5, 9.0);  // exactly sized
    grt_gbuffer_info other_device = info;
    other_device.device = 0;
    CHECK(grt_gbuffer_lapse_read_file(path.c_str(), &other_device, back.data()) == 0 && same_bits(back, lapse));
    CHECK(grt_gbuffer_lapse_read_file(path.c_str(), &info, nullptr) == 0);  // the check alone
  }
  const std::vector<char> whole = slurp(path);
  CHECK(whole.size() == 16 + sizeof(grt_gbuffer_info) + 8 + 5 * 8);
  const std::vector<double> untouched(5, 9.0);
  auto refused = [&](const std::vector<char>& bytes, const grt_gbuffer_info& bound) {
    std::vector<double> back(5, 9.0);
    CHECK(spit(cut, bytes.data(), bytes.size()));
    const int rc = grt_gbuffer_lapse_read_file(cut.c_str(), &bound, back.data());
    CHECK(rc == -EINVAL && same_bits(back, untouched) && std::strlen(grt_last_error()) > 0);
    CHECK(grt_gbuffer_lapse_read_file(cut.c_str(), &bound, nullptr) == -EINVAL);
  };
  for (size_t len = 0; len < whole.size(); ++len)  // every truncation, the section boundaries among them
    refused(std::vector<char>(whole.begin(), whole.begin() + len), info);
  {
    std::vector<char> longer = whole;
    longer.push_back(0);
    refused(longer, info);
    std::vector<char> magic = whole, version = whole, size = whole, count = whole, entry = whole;
    magic[3] ^= 1;
    refused(magic, info);
    version[8] ^= 2;
    refused(version, info);
    size[12] ^= 4;
    refused(size, info);
    const size_t at_count = 16 + sizeof(grt_gbuffer_info);
    count[at_count] = 4;  // a count other than the buffer's (and than the file's length)
    refused(count, info);
    const double nan = NAN;
    std::memcpy(entry.data() + at_count + 8 + 2 * 8, &nan, 8);
    refused(entry, info);
    grt_gbuffer_info other = info;  // a sidecar of another buffer: each bound field in turn
    other.rows = 2;
    other.cols = 3;
    refused(whole, other);
    other = info;
    other.camera.position[0] = 1.0;
    refused(whole, other);
    other = info;
    other.max_steps = 7;
    refused(whole, other);
    other = info;
    other.n_layers = 4;
    refused(whole, other);
  }
  // the writer's refusals
  const double bad[5] = {-1.0, NAN, -1.0, -1.0, -1.0};
  CHECK(grt_gbuffer_lapse_write_file(cut.c_str(), &info, lapse.data(), 4) == -EINVAL);
  CHECK(grt_gbuffer_lapse_write_file(cut.c_str(), &info, bad, 5) == -EINVAL);
  CHECK(grt_gbuffer_lapse_write_file(cut.c_str(), &info, nullptr, 5) == -EINVAL);
  CHECK(grt_gbuffer_lapse_write_file(nullptr, &info, lapse.data(), 5) == -EINVAL);
  CHECK(grt_gbuffer_lapse_write_file(cut.c_str(), nullptr, lapse.data(), 5) == -EINVAL);
  CHECK(grt_gbuffer_lapse_read_file((dir + "/lapse_main.absent").c_str(), &info, nullptr) == -EIO);
  std::remove(path.c_str());
  std::remove(cut.c_str());
}

int main(int argc, char** argv) {
  retarded_rule();
  sidecar(argc > 1 ? argv[1] : ".");
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
