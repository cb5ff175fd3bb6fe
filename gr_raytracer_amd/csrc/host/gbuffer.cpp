// gbuffer.cpp — host side of the geometry buffer (grt_api.h, grt_gbuffer_*): the shape key
// of a scene, its comparison, the consistency checks of a buffer's arrays, and the file.
// No device code: api_gbuffer.hip owns the device-resident buffer.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_internal.h"

namespace {

int fail(int code, const std::string& msg) {
  grt_host::set_error(msg);
  return code;
}

const char MAGIC[8] = {'G', 'R', 'T', 'G', 'B', 'U', 'F', '\0'};
constexpr uint64_t HEADER_BYTES = 16 + sizeof(grt_gbuffer_info);
const char SUB_MAGIC[8] = {'G', 'R', 'T', 'G', 'S', 'U', 'B', '\0'};
constexpr uint64_t SUB_HEADER_BYTES = HEADER_BYTES + sizeof(grt_gbuffer_sub_info);
const char LAPSE_MAGIC[8] = {'G', 'R', 'T', 'G', 'L', 'P', 'S', '\0'};
constexpr uint64_t LAPSE_HEADER_BYTES = HEADER_BYTES + 8;
const char SUB_LAPSE_MAGIC[8] = {'G', 'R', 'T', 'G', 'S', 'L', 'P', '\0'};  // its header is SUB_HEADER_BYTES long
// no frame comes near these; they keep the size arithmetic below far from overflow
constexpr uint64_t MAX_PIXELS = (1ull << 31) - 2;
constexpr uint64_t MAX_LAYERS = 1ull << 40;

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// bytes of the arrays after the header
uint64_t payload_bytes(uint64_t n, uint64_t l) {
  uint64_t bytes = 0;
  for (const grt_host::GBufferField& f : grt_host::GBUFFER_FIELDS) bytes += f.bytes(n, l);
  return bytes;
}

struct File {
  FILE* f = nullptr;
  ~File() {
    if (f) std::fclose(f);
  }
};

}  // namespace

namespace grt_host {

int gbuffer_check_info(const grt_gbuffer_info* info) {
  if (!info) return fail(-EINVAL, "g-buffer: null info");
  if (info->rows == 0 || info->cols == 0) return fail(-EINVAL, "g-buffer: empty rectangle");
  if (info->n_pixels != (uint64_t)info->rows * info->cols)
    return fail(-EINVAL, "g-buffer: n_pixels is not rows * cols");
  if (info->n_pixels > MAX_PIXELS) return fail(-EINVAL, "g-buffer: too many pixels");
  if (info->n_layers > MAX_LAYERS) return fail(-EINVAL, "g-buffer: too many layers");
  if (info->shape.n_objects > GRT_MAX_OBJECTS) return fail(-EINVAL, "g-buffer: more than GRT_MAX_OBJECTS objects");
  return 0;
}

int gbuffer_check_arrays(const grt_gbuffer_info* info, const grt_gbuffer_arrays* a) {
  if (int rc = gbuffer_check_info(info)) return rc;
  if (!a || GBufferPtrs(*a).missing(false)) return fail(-EINVAL, "g-buffer: null array");
  if (info->n_layers && GBufferPtrs(*a).missing(true)) return fail(-EINVAL, "g-buffer: null layer array");
  const uint64_t n = info->n_pixels;
  if (a->layer_start[0] != 0) return fail(-EINVAL, "g-buffer: layer_start does not begin at 0");
  for (uint64_t i = 0; i < n; ++i)
    if (a->layer_start[i + 1] < a->layer_start[i])
      return fail(-EINVAL, "g-buffer: layer_start decreases at pixel " + std::to_string(i));
  if (a->layer_start[n] != info->n_layers) return fail(-EINVAL, "g-buffer: layer_start does not end at n_layers");
  for (uint64_t k = 0; k < info->n_layers; ++k)
    if (a->object[k] >= info->shape.n_objects)
      return fail(-EINVAL, "g-buffer: layer " + std::to_string(k) + " names object " + std::to_string(a->object[k]) +
                               " of " + std::to_string(info->shape.n_objects));
  return 0;
}

int gbuffer_sub_check(const grt_gbuffer_info* info, const grt_gbuffer_sub_info* sub, const uint32_t* sub_pixel,
                      const grt_gbuffer_arrays* a) {
  if (int rc = gbuffer_check_info(info)) return rc;
  if (!sub) return fail(-EINVAL, "g-buffer: null sub-sample info");
  const uint64_t spa = sub->samples_per_axis;
  if (spa == 0) {
    if (sub->n_sub_pixels || sub->n_sub_rays || sub->n_sub_layers)
      return fail(-EINVAL, "g-buffer: samples_per_axis is 0 but the sub-sample set is not empty");
    return 0;
  }
  if (spa > 64) return fail(-EINVAL, "g-buffer: samples_per_axis " + std::to_string(spa) + " is more than 64");
  if (sub->n_sub_pixels > info->n_pixels)
    return fail(-EINVAL, "g-buffer: n_sub_pixels " + std::to_string(sub->n_sub_pixels) + " is more than n_pixels");
  if (sub->n_sub_rays != sub->n_sub_pixels * spa * spa)
    return fail(-EINVAL, "g-buffer: n_sub_rays is not n_sub_pixels * samples_per_axis^2");
  if (sub->n_sub_rays > MAX_PIXELS) return fail(-EINVAL, "g-buffer: too many sub-rays");
  if (sub->n_sub_layers > MAX_LAYERS) return fail(-EINVAL, "g-buffer: too many sub-ray layers");
  if (!a) return 0;
  const uint64_t m = sub->n_sub_pixels, n = sub->n_sub_rays, l = sub->n_sub_layers;
  if (m && !sub_pixel) return fail(-EINVAL, "g-buffer: null sub_pixel");
  if (GBufferPtrs(*a).missing(false)) return fail(-EINVAL, "g-buffer: null sub-ray array");
  if (l && GBufferPtrs(*a).missing(true)) return fail(-EINVAL, "g-buffer: null sub-ray layer array");
  {
    std::vector<bool> seen(info->n_pixels, false);
    for (uint64_t j = 0; j < m; ++j) {
      const uint32_t p = sub_pixel[j];
      if (p >= info->n_pixels)
        return fail(-EINVAL, "g-buffer: sub_pixel[" + std::to_string(j) + "] = " + std::to_string(p) +
                                 " is outside the " + std::to_string(info->n_pixels) + " pixels");
      if (seen[p])
        return fail(-EINVAL, "g-buffer: sub_pixel[" + std::to_string(j) + "] = " + std::to_string(p) + " is a duplicate");
      seen[p] = true;
    }
  }
  if (a->layer_start[0] != 0) return fail(-EINVAL, "g-buffer: sub-ray layer_start does not begin at 0");
  for (uint64_t i = 0; i < n; ++i) {
    if (a->layer_start[i + 1] < a->layer_start[i])
      return fail(-EINVAL, "g-buffer: sub-ray layer_start decreases at sub-ray " + std::to_string(i));
    if (a->status[i] & GRT_FLAG_HIT_OVERFLOW)
      return fail(-EINVAL, "g-buffer: sub-ray " + std::to_string(i) + " has the status flag GRT_FLAG_HIT_OVERFLOW");
  }
  if (a->layer_start[n] != l) return fail(-EINVAL, "g-buffer: sub-ray layer_start does not end at n_sub_layers");
  for (uint64_t k = 0; k < l; ++k)
    if (a->object[k] >= info->shape.n_objects)
      return fail(-EINVAL, "g-buffer: sub-ray layer " + std::to_string(k) + " names object " +
                               std::to_string(a->object[k]) + " of " + std::to_string(info->shape.n_objects));
  return 0;
}

}  // namespace grt_host

extern "C" {

void grt_gbuffer_shape_of(const grt_scene_desc* d, grt_gbuffer_shape* out) {
  std::memset(out, 0, sizeof(*out));
  out->geometry = d->geometry;
  out->n_objects = std::min<uint32_t>(d->n_objects, GRT_MAX_OBJECTS);
  out->radius = d->radius;
  out->a = d->a;
  for (uint32_t k = 0; k < out->n_objects; ++k) {
    const grt_object_desc& o = d->objects[k];
    grt_gbuffer_object_shape& s = out->objects[k];
    s.kind = o.kind;
    s.temp_kind = o.temp_kind;
    s.radius = o.radius;
    for (int q = 0; q < 3; ++q) s.center[q] = o.center[q];
    s.inner_radius = o.inner_radius;
    s.outer_radius = o.outer_radius;
    s.r_isco = o.r_isco;
  }
}

int grt_gbuffer_shape_compatible(const grt_gbuffer_shape* t, const grt_scene_desc* appearance) {
  if (!t || !appearance) return fail(-EINVAL, "null argument");
  if (appearance->n_objects > GRT_MAX_OBJECTS) return fail(-EINVAL, "too many objects");
  grt_gbuffer_shape b;
  grt_gbuffer_shape_of(appearance, &b);
  auto differs = [](const std::string& field) {
    return fail(-EINVAL, "g-buffer: the appearance scene differs from the traced one in " + field);
  };
  if (t->geometry != b.geometry) return differs("geometry");
  if (!same(t->radius, b.radius)) return differs("radius");
  if (!same(t->a, b.a)) return differs("a");
  if (t->n_objects != b.n_objects) return differs("n_objects");
  for (uint32_t k = 0; k < b.n_objects; ++k) {
    const grt_gbuffer_object_shape &x = t->objects[k], &y = b.objects[k];
    const std::string o = "objects[" + std::to_string(k) + "].";
    if (x.kind != y.kind) return differs(o + "kind");
    if (x.temp_kind != y.temp_kind) return differs(o + "temp_kind");
    if (!same(x.radius, y.radius)) return differs(o + "radius");
    for (int q = 0; q < 3; ++q)
      if (!same(x.center[q], y.center[q])) return differs(o + "center");
    if (!same(x.inner_radius, y.inner_radius)) return differs(o + "inner_radius");
    if (!same(x.outer_radius, y.outer_radius)) return differs(o + "outer_radius");
    if (!same(x.r_isco, y.r_isco)) return differs(o + "r_isco");
  }
  return 0;
}

int grt_gbuffer_compatible(const grt_scene_desc* traced, const grt_scene_desc* appearance) {
  if (!traced || !appearance) return fail(-EINVAL, "null argument");
  if (traced->n_objects > GRT_MAX_OBJECTS) return fail(-EINVAL, "too many objects");
  grt_gbuffer_shape a;
  grt_gbuffer_shape_of(traced, &a);
  return grt_gbuffer_shape_compatible(&a, appearance);
}

int grt_gbuffer_write_file(const char* path, const grt_gbuffer_info* info, const grt_gbuffer_arrays* a) {
  if (!path) return fail(-EINVAL, "null path");
  if (int rc = grt_host::gbuffer_check_arrays(info, a)) return rc;
  File file;
  file.f = std::fopen(path, "wb");
  if (!file.f) return fail(-EIO, std::string("cannot create ") + path);
  const uint64_t n = info->n_pixels, l = info->n_layers;
  const uint32_t head[2] = {GRT_GBUFFER_FILE_VERSION, (uint32_t)sizeof(grt_gbuffer_info)};
  bool ok = true;
  auto put = [&](const void* p, uint64_t bytes) {
    if (ok && bytes) ok = std::fwrite(p, 1, bytes, file.f) == bytes;
  };
  put(MAGIC, 8);
  put(head, 8);
  put(info, sizeof(*info));
  const grt_host::GBufferPtrs P(*a);
  for (int k = 0; k < grt_host::GB_N_FIELDS; ++k) put(P.p[k], grt_host::GBUFFER_FIELDS[k].bytes(n, l));
  FILE* f = file.f;
  file.f = nullptr;
  if (std::fclose(f) != 0) ok = false;
  if (!ok) return fail(-EIO, std::string("cannot write ") + path);
  return 0;
}

int grt_gbuffer_read_file(const char* path, grt_gbuffer_info* info, const grt_gbuffer_arrays* a) {
  if (!path || !info) return fail(-EINVAL, "null argument");
  File file;
  file.f = std::fopen(path, "rb");
  if (!file.f) return fail(-EIO, std::string("cannot open ") + path);
  const std::string name = std::string(path) + ": ";
  if (std::fseek(file.f, 0, SEEK_END) != 0) return fail(-EIO, name + "cannot seek");
  const long end = std::ftell(file.f);
  if (end < 0 || std::fseek(file.f, 0, SEEK_SET) != 0) return fail(-EIO, name + "cannot seek");
  const uint64_t length = (uint64_t)end;
  if (length < HEADER_BYTES) return fail(-EINVAL, name + "too short for a g-buffer header");
  char magic[8];
  uint32_t head[2];
  grt_gbuffer_info in;
  if (std::fread(magic, 1, 8, file.f) != 8 || std::fread(head, 1, 8, file.f) != 8)
    return fail(-EIO, name + "cannot read the header");
  if (std::memcmp(magic, MAGIC, 8) != 0) return fail(-EINVAL, name + "not a g-buffer file (magic)");
  if (head[0] != GRT_GBUFFER_FILE_VERSION)
    return fail(-EINVAL, name + "g-buffer file version " + std::to_string(head[0]) + ", this library reads " +
                             std::to_string(GRT_GBUFFER_FILE_VERSION));
  if (head[1] != sizeof(grt_gbuffer_info)) return fail(-EINVAL, name + "info block of another size");
  if (std::fread(&in, 1, sizeof(in), file.f) != sizeof(in)) return fail(-EIO, name + "cannot read the info block");
  if (int rc = grt_host::gbuffer_check_info(&in)) return rc;
  const uint64_t n = in.n_pixels, l = in.n_layers;
  if (length != HEADER_BYTES + payload_bytes(n, l))
    return fail(-EINVAL, name + "file length " + std::to_string(length) + " disagrees with its sizes (" +
                             std::to_string(HEADER_BYTES + payload_bytes(n, l)) + " expected)");
  if (!a) {  // size query
    *info = in;
    return 0;
  }
  const grt_host::GBufferPtrs P(*a);
  if (P.missing(false) || (l && P.missing(true))) return fail(-EINVAL, "g-buffer: null array");
  bool ok = true;
  auto get = [&](void* p, uint64_t bytes) {
    if (ok && bytes) ok = std::fread(p, 1, bytes, file.f) == bytes;
  };
  for (int k = 0; k < grt_host::GB_N_FIELDS; ++k) get(P.p[k], grt_host::GBUFFER_FIELDS[k].bytes(n, l));
  if (!ok) return fail(-EIO, name + "cannot read the arrays");
  if (int rc = grt_host::gbuffer_check_arrays(&in, a)) return rc;
  *info = in;
  return 0;
}

// ---- the sub-sample set's sidecar ----
// The buffer's info with the fields a load changes (the device) zeroed: what binds a set to it.
static grt_gbuffer_info bound_info(const grt_gbuffer_info* info) {
  grt_gbuffer_info b = *info;
  b.device = 0;
  b._pad = 0;
  return b;
}

int grt_gbuffer_sub_write_file(const char* path, const grt_gbuffer_info* info, const grt_gbuffer_sub_info* sub,
                               const uint32_t* sub_pixel, const grt_gbuffer_arrays* a) {
  if (!path) return fail(-EINVAL, "null path");
  if (!a) return fail(-EINVAL, "g-buffer: null sub-ray array");
  if (int rc = grt_host::gbuffer_sub_check(info, sub, sub_pixel, a)) return rc;
  File file;
  file.f = std::fopen(path, "wb");
  if (!file.f) return fail(-EIO, std::string("cannot create ") + path);
  const uint64_t m = sub->n_sub_pixels, n = sub->n_sub_rays, l = sub->n_sub_layers;
  const uint32_t head[2] = {GRT_GBUFFER_SUB_FILE_VERSION, (uint32_t)sizeof(grt_gbuffer_info)};
  const grt_gbuffer_info bound = bound_info(info);
  grt_gbuffer_sub_info si = *sub;
  si._pad = 0;
  bool ok = true;
  auto put = [&](const void* p, uint64_t bytes) {
    if (ok && bytes) ok = std::fwrite(p, 1, bytes, file.f) == bytes;
  };
  put(SUB_MAGIC, 8);
  put(head, 8);
  put(&bound, sizeof(bound));
  put(&si, sizeof(si));
  put(sub_pixel, 4 * m);
  if (si.samples_per_axis) {
    const grt_host::GBufferPtrs P(*a);
    for (int k = 0; k < grt_host::GB_N_FIELDS; ++k) put(P.p[k], grt_host::GBUFFER_FIELDS[k].bytes(n, l));
  }
  FILE* f = file.f;
  file.f = nullptr;
  if (std::fclose(f) != 0) ok = false;
  if (!ok) return fail(-EIO, std::string("cannot write ") + path);
  return 0;
}

int grt_gbuffer_sub_read_file(const char* path, const grt_gbuffer_info* info, grt_gbuffer_sub_info* sub,
                              uint32_t* sub_pixel, const grt_gbuffer_arrays* a) {
  if (!path || !info || !sub) return fail(-EINVAL, "null argument");
  File file;
  file.f = std::fopen(path, "rb");
  if (!file.f) return fail(-EIO, std::string("cannot open ") + path);
  const std::string name = std::string(path) + ": ";
  if (std::fseek(file.f, 0, SEEK_END) != 0) return fail(-EIO, name + "cannot seek");
  const long end = std::ftell(file.f);
  if (end < 0 || std::fseek(file.f, 0, SEEK_SET) != 0) return fail(-EIO, name + "cannot seek");
  const uint64_t length = (uint64_t)end;
  if (length < SUB_HEADER_BYTES) return fail(-EINVAL, name + "too short for a sub-sample set header");
  char magic[8];
  uint32_t head[2];
  grt_gbuffer_info in;
  grt_gbuffer_sub_info si;
  if (std::fread(magic, 1, 8, file.f) != 8 || std::fread(head, 1, 8, file.f) != 8)
    return fail(-EIO, name + "cannot read the header");
  if (std::memcmp(magic, SUB_MAGIC, 8) != 0) return fail(-EINVAL, name + "not a g-buffer sub-sample file (magic)");
  if (head[0] != GRT_GBUFFER_SUB_FILE_VERSION)
    return fail(-EINVAL, name + "sub-sample file version " + std::to_string(head[0]) + ", this library reads " +
                             std::to_string(GRT_GBUFFER_SUB_FILE_VERSION));
  if (head[1] != sizeof(grt_gbuffer_info)) return fail(-EINVAL, name + "info block of another size");
  if (std::fread(&in, 1, sizeof(in), file.f) != sizeof(in) || std::fread(&si, 1, sizeof(si), file.f) != sizeof(si))
    return fail(-EIO, name + "cannot read the info blocks");
  const grt_gbuffer_info bound = bound_info(info);
  if (std::memcmp(&in, &bound, sizeof(in)) != 0)
    return fail(-EINVAL, name + "the sub-sample set belongs to another g-buffer (its info block differs)");
  if (int rc = grt_host::gbuffer_sub_check(info, &si, nullptr, nullptr)) return rc;
  const uint64_t m = si.n_sub_pixels, n = si.n_sub_rays, l = si.n_sub_layers;
  const uint64_t expect = SUB_HEADER_BYTES + 4 * m + (si.samples_per_axis ? payload_bytes(n, l) : 0);
  if (length != expect)
    return fail(-EINVAL, name + "file length " + std::to_string(length) + " disagrees with its sizes (" +
                             std::to_string(expect) + " expected)");
  if (!a) {  // size query
    *sub = si;
    return 0;
  }
  if (si.samples_per_axis == 0) {
    *sub = si;
    return 0;
  }
  const grt_host::GBufferPtrs P(*a);
  if ((m && !sub_pixel) || P.missing(false) || (l && P.missing(true)))
    return fail(-EINVAL, "g-buffer: null sub-ray array");
  bool ok = true;
  auto get = [&](void* p, uint64_t bytes) {
    if (ok && bytes) ok = std::fread(p, 1, bytes, file.f) == bytes;
  };
  get(sub_pixel, 4 * m);
  for (int k = 0; k < grt_host::GB_N_FIELDS; ++k) get(P.p[k], grt_host::GBUFFER_FIELDS[k].bytes(n, l));
  if (!ok) return fail(-EIO, name + "cannot read the arrays");
  if (int rc = grt_host::gbuffer_sub_check(info, &si, sub_pixel, a)) return rc;
  *sub = si;
  return 0;
}

// ---- the lapse's sidecar ----
// magic, version and info-block size, the bound info, n_layers, the doubles.
int grt_gbuffer_lapse_write_file(const char* path, const grt_gbuffer_info* info, const double* lapse,
                                 uint64_t n_layers) {
  if (!path) return fail(-EINVAL, "null path");
  if (int rc = grt_host::gbuffer_check_info(info)) return rc;
  if (n_layers != info->n_layers)
    return fail(-EINVAL, "g-buffer: a lapse of " + std::to_string(n_layers) + " entries for " +
                             std::to_string(info->n_layers) + " layers");
  if (n_layers && !lapse) return fail(-EINVAL, "g-buffer: null lapse");
  for (uint64_t k = 0; k < n_layers; ++k)
    if (!std::isfinite(lapse[k])) return fail(-EINVAL, "g-buffer: lapse[" + std::to_string(k) + "] is not finite");
  File file;
  file.f = std::fopen(path, "wb");
  if (!file.f) return fail(-EIO, std::string("cannot create ") + path);
  const uint32_t head[2] = {GRT_GBUFFER_LAPSE_FILE_VERSION, (uint32_t)sizeof(grt_gbuffer_info)};
  const grt_gbuffer_info bound = bound_info(info);
  bool ok = true;
  auto put = [&](const void* p, uint64_t bytes) {
    if (ok && bytes) ok = std::fwrite(p, 1, bytes, file.f) == bytes;
  };
  put(LAPSE_MAGIC, 8);
  put(head, 8);
  put(&bound, sizeof(bound));
  put(&n_layers, 8);
  put(lapse, 8 * n_layers);
  FILE* f = file.f;
  file.f = nullptr;
  if (std::fclose(f) != 0) ok = false;
  if (!ok) return fail(-EIO, std::string("cannot write ") + path);
  return 0;
}

int grt_gbuffer_lapse_read_file(const char* path, const grt_gbuffer_info* info, double* lapse) {
  if (!path || !info) return fail(-EINVAL, "null argument");
  if (int rc = grt_host::gbuffer_check_info(info)) return rc;
  File file;
  file.f = std::fopen(path, "rb");
  if (!file.f) return fail(-EIO, std::string("cannot open ") + path);
  const std::string name = std::string(path) + ": ";
  if (std::fseek(file.f, 0, SEEK_END) != 0) return fail(-EIO, name + "cannot seek");
  const long end = std::ftell(file.f);
  if (end < 0 || std::fseek(file.f, 0, SEEK_SET) != 0) return fail(-EIO, name + "cannot seek");
  const uint64_t length = (uint64_t)end;
  if (length < LAPSE_HEADER_BYTES) return fail(-EINVAL, name + "too short for a lapse header");
  char magic[8];
  uint32_t head[2];
  grt_gbuffer_info in;
  uint64_t l = 0;
  if (std::fread(magic, 1, 8, file.f) != 8 || std::fread(head, 1, 8, file.f) != 8)
    return fail(-EIO, name + "cannot read the header");
  if (std::memcmp(magic, LAPSE_MAGIC, 8) != 0) return fail(-EINVAL, name + "not a g-buffer lapse file (magic)");
  if (head[0] != GRT_GBUFFER_LAPSE_FILE_VERSION)
    return fail(-EINVAL, name + "lapse file version " + std::to_string(head[0]) + ", this library reads " +
                             std::to_string(GRT_GBUFFER_LAPSE_FILE_VERSION));
  if (head[1] != sizeof(grt_gbuffer_info)) return fail(-EINVAL, name + "info block of another size");
  if (std::fread(&in, 1, sizeof(in), file.f) != sizeof(in) || std::fread(&l, 1, 8, file.f) != 8)
    return fail(-EIO, name + "cannot read the info block");
  const grt_gbuffer_info bound = bound_info(info);
  if (std::memcmp(&in, &bound, sizeof(in)) != 0)
    return fail(-EINVAL, name + "the lapse belongs to another g-buffer (its info block differs)");
  if (l != info->n_layers)
    return fail(-EINVAL, name + "a lapse of " + std::to_string(l) + " entries for " + std::to_string(info->n_layers) +
                             " layers");
  if (length != LAPSE_HEADER_BYTES + 8 * l)  // l <= MAX_LAYERS (gbuffer_check_info): no overflow
    return fail(-EINVAL, name + "file length " + std::to_string(length) + " disagrees with its sizes (" +
                             std::to_string(LAPSE_HEADER_BYTES + 8 * l) + " expected)");
  // the entries go through a buffer of the file's: the caller's array is written only once all are finite
  std::vector<double> v(l);
  if (l && std::fread(v.data(), 8, l, file.f) != l) return fail(-EIO, name + "cannot read the lapse");
  for (uint64_t k = 0; k < l; ++k)
    if (!std::isfinite(v[k])) return fail(-EINVAL, name + "lapse[" + std::to_string(k) + "] is not finite");
  if (lapse && l) std::memcpy(lapse, v.data(), 8 * l);
  return 0;
}

// ---- the sub-sample set's lapse sidecar ----
// magic, version and info-block size, the bound info, the set's sub-info, the doubles.  The
// sub-info binds the sidecar to the set it was written for: a `.sub` that grew since has
// other counts, and its stale `.sub.lapse` is refused.
int grt_gbuffer_sub_lapse_write_file(const char* path, const grt_gbuffer_info* info, const grt_gbuffer_sub_info* sub,
                                     const double* lapse, uint64_t n_sub_layers) {
  if (!path) return fail(-EINVAL, "null path");
  if (int rc = grt_host::gbuffer_sub_check(info, sub, nullptr, nullptr)) return rc;
  if (n_sub_layers != sub->n_sub_layers)
    return fail(-EINVAL, "g-buffer: a lapse of " + std::to_string(n_sub_layers) + " entries for " +
                             std::to_string(sub->n_sub_layers) + " sub-ray layers");
  if (n_sub_layers && !lapse) return fail(-EINVAL, "g-buffer: null lapse");
  for (uint64_t k = 0; k < n_sub_layers; ++k)
    if (!std::isfinite(lapse[k])) return fail(-EINVAL, "g-buffer: lapse[" + std::to_string(k) + "] is not finite");
  File file;
  file.f = std::fopen(path, "wb");
  if (!file.f) return fail(-EIO, std::string("cannot create ") + path);
  const uint32_t head[2] = {GRT_GBUFFER_SUB_LAPSE_FILE_VERSION, (uint32_t)sizeof(grt_gbuffer_info)};
  const grt_gbuffer_info bound = bound_info(info);
  grt_gbuffer_sub_info si = *sub;
  si._pad = 0;
  bool ok = true;
  auto put = [&](const void* p, uint64_t bytes) {
    if (ok && bytes) ok = std::fwrite(p, 1, bytes, file.f) == bytes;
  };
  put(SUB_LAPSE_MAGIC, 8);
  put(head, 8);
  put(&bound, sizeof(bound));
  put(&si, sizeof(si));
  put(lapse, 8 * n_sub_layers);
  FILE* f = file.f;
  file.f = nullptr;
  if (std::fclose(f) != 0) ok = false;
  if (!ok) return fail(-EIO, std::string("cannot write ") + path);
  return 0;
}

int grt_gbuffer_sub_lapse_read_file(const char* path, const grt_gbuffer_info* info, const grt_gbuffer_sub_info* sub,
                                    double* lapse) {
  if (!path || !info || !sub) return fail(-EINVAL, "null argument");
  if (int rc = grt_host::gbuffer_sub_check(info, sub, nullptr, nullptr)) return rc;
  File file;
  file.f = std::fopen(path, "rb");
  if (!file.f) return fail(-EIO, std::string("cannot open ") + path);
  const std::string name = std::string(path) + ": ";
  if (std::fseek(file.f, 0, SEEK_END) != 0) return fail(-EIO, name + "cannot seek");
  const long end = std::ftell(file.f);
  if (end < 0 || std::fseek(file.f, 0, SEEK_SET) != 0) return fail(-EIO, name + "cannot seek");
  const uint64_t length = (uint64_t)end;
  if (length < SUB_HEADER_BYTES) return fail(-EINVAL, name + "too short for a sub-sample lapse header");
  char magic[8];
  uint32_t head[2];
  grt_gbuffer_info in;
  grt_gbuffer_sub_info si;
  if (std::fread(magic, 1, 8, file.f) != 8 || std::fread(head, 1, 8, file.f) != 8)
    return fail(-EIO, name + "cannot read the header");
  if (std::memcmp(magic, SUB_LAPSE_MAGIC, 8) != 0)
    return fail(-EINVAL, name + "not a g-buffer sub-sample lapse file (magic)");
  if (head[0] != GRT_GBUFFER_SUB_LAPSE_FILE_VERSION)
    return fail(-EINVAL, name + "sub-sample lapse file version " + std::to_string(head[0]) + ", this library reads " +
                             std::to_string(GRT_GBUFFER_SUB_LAPSE_FILE_VERSION));
  if (head[1] != sizeof(grt_gbuffer_info)) return fail(-EINVAL, name + "info block of another size");
  if (std::fread(&in, 1, sizeof(in), file.f) != sizeof(in) || std::fread(&si, 1, sizeof(si), file.f) != sizeof(si))
    return fail(-EIO, name + "cannot read the info blocks");
  const grt_gbuffer_info bound = bound_info(info);
  if (std::memcmp(&in, &bound, sizeof(in)) != 0)
    return fail(-EINVAL, name + "the lapse belongs to another g-buffer (its info block differs)");
  grt_gbuffer_sub_info want = *sub;
  want._pad = 0;
  if (std::memcmp(&si, &want, sizeof(si)) != 0)
    return fail(-EINVAL, name + "the lapse belongs to another sub-sample set (" + std::to_string(si.n_sub_pixels) +
                             " pixels and " + std::to_string(si.n_sub_layers) + " layers, the set has " +
                             std::to_string(want.n_sub_pixels) + " and " + std::to_string(want.n_sub_layers) + ")");
  const uint64_t l = want.n_sub_layers;  // <= MAX_LAYERS (gbuffer_sub_check): no overflow
  if (length != SUB_HEADER_BYTES + 8 * l)
    return fail(-EINVAL, name + "file length " + std::to_string(length) + " disagrees with its sizes (" +
                             std::to_string(SUB_HEADER_BYTES + 8 * l) + " expected)");
  // the entries go through a buffer of the file's: the caller's array is written only once all are finite
  std::vector<double> v(l);
  if (l && std::fread(v.data(), 8, l, file.f) != l) return fail(-EIO, name + "cannot read the lapse");
  for (uint64_t k = 0; k < l; ++k)
    if (!std::isfinite(v[k])) return fail(-EINVAL, name + "lapse[" + std::to_string(k) + "] is not finite");
  if (lapse && l) std::memcpy(lapse, v.data(), 8 * l);
  return 0;
}

}  // extern "C"
