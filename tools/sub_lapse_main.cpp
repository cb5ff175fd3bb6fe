// sub_lapse_main.cpp — a stand-alone caller of the writer and reader of the sub-sample set's
// lapse sidecar (`<file>.sub.lapse`) for CPU sanitizer builds: no GPU, no Python, no libgrt.so.
// Build it with the two host files it needs and run it:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/sub_lapse_main.cpp gr_raytracer_amd/csrc/host/gbuffer.cpp \
//       gr_raytracer_amd/csrc/host/errors.cpp -o sub_lapse_main \
//     && ./sub_lapse_main SCRATCH_DIR
//
// A round trip with 0 and with 5 sub-layers on exactly sized heap arrays (so an access past an
// end is the sanitizer's to report), then every truncation of the small file, a byte too many,
// a changed magic, version, info-block size and count, a NaN entry, and infos and sub-infos
// that differ from the file's (a set that grew since among them): each -EINVAL with the
// caller's array untouched.  Files go to SCRATCH_DIR (default "."), and are removed.
// Exit status 0 and "ok" on success.
#include <cerrno>
#include <cmath>
#include <cstddef>
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

static grt_gbuffer_info small_info() {
  grt_gbuffer_info info;
  std::memset(&info, 0, sizeof(info));
  info.rows = 3;
  info.cols = 2;
  info.n_pixels = 6;
  info.n_layers = 4;
  info.device = 5;  // a load changes it: not part of what binds the sidecar
  info.shape.geometry = GRT_GEOM_SCHWARZSCHILD;
  info.shape.n_objects = 1;
  info.shape.radius = 1.0;
  info.camera.rows = 3;
  info.camera.cols = 2;
  return info;
}

static grt_gbuffer_sub_info small_sub(uint32_t spa, uint64_t pixels, uint64_t layers) {
  grt_gbuffer_sub_info sub;
  std::memset(&sub, 0, sizeof(sub));
  sub.samples_per_axis = spa;
  sub.n_sub_pixels = pixels;
  sub.n_sub_rays = pixels * spa * spa;
  sub.n_sub_layers = layers;
  return sub;
}

static void sidecar(const std::string& dir) {
  const std::string path = dir + "/sub_lapse_main.grtg.sub.lapse", cut = dir + "/sub_lapse_main.cut.sub.lapse";
  const grt_gbuffer_info info = small_info();
  {  // no layers: a set of two pixels whose sub-rays hit nothing, and no set at all
    for (const grt_gbuffer_sub_info& sub : {small_sub(2, 2, 0), small_sub(0, 0, 0)}) {
      CHECK(grt_gbuffer_sub_lapse_write_file(path.c_str(), &info, &sub, nullptr, 0) == 0);
      CHECK(grt_gbuffer_sub_lapse_read_file(path.c_str(), &info, &sub, nullptr) == 0);
      double none = 9.0;
      CHECK(grt_gbuffer_sub_lapse_read_file(path.c_str(), &info, &sub, &none) == 0 && none == 9.0);
      CHECK(slurp(path).size() == 16 + sizeof(grt_gbuffer_info) + sizeof(grt_gbuffer_sub_info));
    }
  }
  const grt_gbuffer_sub_info sub = small_sub(2, 2, 5);
  const std::vector<double> lapse = {-1.5, -0.0, -17.25, -1e-300, -52.0};
  CHECK(grt_gbuffer_sub_lapse_write_file(path.c_str(), &info, &sub, lapse.data(), 5) == 0);
  {
    std::vector<double> back(5, 9.0);  // exactly sized
    grt_gbuffer_info other_device = info;
    other_device.device = 0;
    grt_gbuffer_sub_info padded = sub;
    padded._pad = 77;  // not part of what binds the sidecar
    CHECK(grt_gbuffer_sub_lapse_read_file(path.c_str(), &other_device, &padded, back.data()) == 0 &&
          same_bits(back, lapse));
    CHECK(grt_gbuffer_sub_lapse_read_file(path.c_str(), &info, &sub, nullptr) == 0);  // the check alone
  }
  const std::vector<char> whole = slurp(path);
  const size_t at_sub = 16 + sizeof(grt_gbuffer_info), at_data = at_sub + sizeof(grt_gbuffer_sub_info);
  CHECK(whole.size() == at_data + 5 * 8);
  CHECK(std::memcmp(whole.data(), "GRTGSLP\0", 8) == 0);
  const std::vector<double> untouched(5, 9.0);
  auto refused = [&](const std::vector<char>& bytes, const grt_gbuffer_info& bound, const grt_gbuffer_sub_info& set) {
    std::vector<double> back(5, 9.0);
    CHECK(spit(cut, bytes.data(), bytes.size()));
    const int rc = grt_gbuffer_sub_lapse_read_file(cut.c_str(), &bound, &set, back.data());
    CHECK(rc == -EINVAL && same_bits(back, untouched) && std::strlen(grt_last_error()) > 0);
    CHECK(grt_gbuffer_sub_lapse_read_file(cut.c_str(), &bound, &set, nullptr) == -EINVAL);
  };
  for (size_t len = 0; len < whole.size(); ++len)  // every truncation, the section boundaries among them
    refused(std::vector<char>(whole.begin(), whole.begin() + len), info, sub);
  {
    std::vector<char> longer = whole;
    longer.push_back(0);
    refused(longer, info, sub);
    std::vector<char> magic = whole, version = whole, size = whole, count = whole, entry = whole;
    magic[5] ^= 1;
    refused(magic, info, sub);
    std::memcpy(magic.data(), "GRTGLPS\0", 8);  // the buffer's own lapse sidecar is another file
    refused(magic, info, sub);
    version[8] ^= 2;
    refused(version, info, sub);
    size[12] ^= 4;
    refused(size, info, sub);
    const uint64_t four = 4;  // the file's n_sub_layers: not the set's, and not the file's length
    std::memcpy(count.data() + at_sub + offsetof(grt_gbuffer_sub_info, n_sub_layers), &four, 8);
    refused(count, info, sub);
    count.resize(count.size() - 8);  // nor with the doubles to match
    refused(count, info, sub);
    const double nan = NAN;
    std::memcpy(entry.data() + at_data + 2 * 8, &nan, 8);
    refused(entry, info, sub);
    const double inf = INFINITY;
    std::memcpy(entry.data() + at_data + 2 * 8, &inf, 8);
    refused(entry, info, sub);
    grt_gbuffer_info other = info;  // a sidecar of another buffer: each bound field in turn
    other.rows = 2;
    other.cols = 3;
    refused(whole, other, sub);
    other = info;
    other.camera.position[0] = 1.0;
    refused(whole, other, sub);
    other = info;
    other.max_steps = 7;
    refused(whole, other, sub);
    other = info;
    other.n_layers = 3;
    refused(whole, other, sub);
    // a sidecar of another set: one that grew since (more pixels, more layers), one with
    // as many layers in other pixels, another samples_per_axis
    refused(whole, info, small_sub(2, 3, 8));
    refused(whole, info, small_sub(2, 3, 5));
    refused(whole, info, small_sub(2, 2, 4));
    refused(whole, info, small_sub(1, 2, 5));
    refused(whole, info, small_sub(0, 0, 0));
  }
  // the writer's refusals
  const double bad[5] = {-1.0, NAN, -1.0, -1.0, -1.0};
  grt_gbuffer_sub_info broken = sub;
  broken.n_sub_rays = 7;  // not n_sub_pixels * samples_per_axis^2
  CHECK(grt_gbuffer_sub_lapse_write_file(cut.c_str(), &info, &sub, lapse.data(), 4) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_write_file(cut.c_str(), &info, &sub, bad, 5) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_write_file(cut.c_str(), &info, &sub, nullptr, 5) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_write_file(cut.c_str(), &info, &broken, lapse.data(), 5) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_write_file(nullptr, &info, &sub, lapse.data(), 5) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_write_file(cut.c_str(), nullptr, &sub, lapse.data(), 5) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_write_file(cut.c_str(), &info, nullptr, lapse.data(), 5) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_read_file(nullptr, &info, &sub, nullptr) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_read_file(path.c_str(), nullptr, &sub, nullptr) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_read_file(path.c_str(), &info, nullptr, nullptr) == -EINVAL);
  CHECK(grt_gbuffer_sub_lapse_read_file((dir + "/sub_lapse_main.absent").c_str(), &info, &sub, nullptr) == -EIO);
  std::remove(path.c_str());
  std::remove(cut.c_str());
}

int main(int argc, char** argv) {
  sidecar(argc > 1 ? argv[1] : ".");
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
