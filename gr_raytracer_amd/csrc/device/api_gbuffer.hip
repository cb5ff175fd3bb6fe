// api_gbuffer.hip — geometry buffers of the C ABI (include/grt_api.h): the exact trace and
// fill of a frame or of a camera sequence, the sub-sample set (of one buffer, or of a stack
// of buffers filled by stacked traces), and the re-shades, the adaptive ones through the
// pass of api_adaptive.hip (AdaptivePlan, api_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "grt_api.h"
#include "../host/host_internal.h"
#include "dev_scene.h"
#include "kernels.h"
#include "api_internal.h"

using namespace grt_api;

// ---- geometry buffer (grt_api.h): trace once, re-shade many times -------------------------
// The device-resident buffer: its arrays belong to it, not to a scene's scratch, so later
// traces on the device leave it alone.
// Grow a device array to `want` bytes, keeping its first `keep` bytes.
static int grow_buf(DevBuf& b, size_t keep, size_t want) {
  void* p = nullptr;
  if (hipMalloc(&p, want ? want : 16) != hipSuccess) {
    (void)hipGetLastError();
    return fail(-ENOMEM, "cannot grow the g-buffer's sub-sample set");
  }
  if (keep && b.p) {
    hipError_t e = hipMemcpy(p, b.p, keep, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return fail(-EIO, std::string("HIP error: ") + hipGetErrorString(e));
    }
  }
  b.reset();
  b.p = p;
  return 0;
}

using namespace grt_host;  // the field table: GRT_GBUFFER_FIELDS, GBUFFER_FIELDS, GB_*

// The twelve device arrays of a buffer, of a sub-sample set or of a transient stack, by the
// table.  Counts and capacities are the owner's: every size is an argument.
struct GBufferDev {
  DevBuf a[GB_N_FIELDS];
  uint8_t* status() const { return (uint8_t*)a[GB_status].p; }
  uint8_t* stop() const { return (uint8_t*)a[GB_stop].p; }
  uint32_t* steps() const { return (uint32_t*)a[GB_steps].p; }
  uint64_t* layer_start() const { return (uint64_t*)a[GB_layer_start].p; }
  // fresh per-ray (`layer`: per-layer) arrays of `count` elements; what they held is freed
  int alloc(bool layer, uint64_t count) {
    for (int k = 0; k < GB_N_FIELDS; ++k) {
      const GBufferField& f = GBUFFER_FIELDS[k];
      if (f.layer != layer) continue;
      a[k].reset();
      if (int rc = a[k].alloc(f.size * (count + f.extra))) return rc;
    }
    return 0;
  }
  // those arrays grown to `count` elements, the first `keep` kept; a new layer_start begins at 0
  int grow(bool layer, uint64_t keep, uint64_t count) {
    for (int k = 0; k < GB_N_FIELDS; ++k) {
      const GBufferField& f = GBUFFER_FIELDS[k];
      if (f.layer != layer) continue;
      const bool first = a[k].p == nullptr;
      if (int rc = grow_buf(a[k], f.size * (keep + f.extra), f.size * (count + f.extra))) return rc;
      if (first && f.extra) HIP_TRY(hipMemset(a[k].p, 0, f.size * f.extra));
    }
    return 0;
  }
  // the n rays from `first_ray` on, over all the layers (layer offsets stay the owner's)
  grt::GBufferArrays view(uint64_t first_ray, uint64_t n) const {
    auto f64 = [&](int k, uint64_t at) { return (double*)a[k].p + at; };
    const uint64_t r = first_ray;
    return grt::GBufferArrays{n, status() + r, stop() + r, layer_start() + r, f64(GB_sky_u, r), f64(GB_sky_v, r),
                              f64(GB_sky_redshift, r), (uint8_t*)a[GB_object].p, f64(GB_u, 0), f64(GB_v, 0),
                              f64(GB_redshift, 0), f64(GB_radius, 0)};
  }
  // n rays and l layers to the host's arrays (hipMemcpyDeviceToHost) or from them
  int copy(const grt_gbuffer_arrays& h, uint64_t n, uint64_t l, hipMemcpyKind kind) const {
    const GBufferPtrs H(h);
    for (int k = 0; k < GB_N_FIELDS; ++k) {
      const uint64_t bytes = GBUFFER_FIELDS[k].bytes(n, l);
      if (!bytes) continue;
      const bool down = kind == hipMemcpyDeviceToHost;
      HIP_TRY(hipMemcpy(down ? H.p[k] : a[k].p, down ? a[k].p : H.p[k], bytes, kind));
    }
    return 0;
  }
  // n_rays rays and n_layers layers from (src_ray, src_layer) to (dst_ray, dst_layer) of `dst`
  // on `st`, empty copies skipped; not layer_start, which gbuffer_rebase / gbuffer_sub_append
  // write rebased
  int copy_slice(GBufferDev& dst, uint64_t dst_ray, uint64_t dst_layer, uint64_t src_ray, uint64_t src_layer,
                 uint64_t n_rays, uint64_t n_layers, hipStream_t st) const {
    for (int k = 0; k < GB_N_FIELDS; ++k) {
      const GBufferField& f = GBUFFER_FIELDS[k];
      const uint64_t to = f.layer ? dst_layer : dst_ray, from = f.layer ? src_layer : src_ray;
      const uint64_t bytes = f.size * (f.layer ? n_layers : n_rays);
      if (k == GB_layer_start || !bytes) continue;
      HIP_TRY(hipMemcpyAsync((char*)dst.a[k].p + to * f.size, (const char*)a[k].p + from * f.size, bytes,
                             hipMemcpyDeviceToDevice, st));
    }
    return 0;
  }
};

// The sub-sample set of a buffer (grt_api.h): append-only, capacities grow geometrically.
// Block b holds the per sub-rays of pixel sub_pixel[b] at rays [b * per, (b + 1) * per).
struct GBufferSub {
  uint32_t spa = 0;  // 0: no set
  uint64_t n_pix = 0, cap_pix = 0, n_layers = 0, cap_layers = 0;
  DevBuf sub_pixel;  // u32[cap_pix]
  DevBuf sub_block;  // u32[n_pixels], GBUFFER_NIL where a pixel has no block (derived, never stored)
  std::vector<uint32_t> h_block;  // host copy of sub_block
  GBufferDev arr;
  // A set is timed or untimed, decided when its first block is appended (sub_fill) or by
  // grt_gbuffer_sub_lapse_upload.  A timed set holds one lapse per sub-layer beside the twelve
  // arrays: f64[cap_layers], indexed as they are, grown with them.
  bool timed = false;
  DevBuf lapse;
  uint64_t per() const { return (uint64_t)spa * spa; }
  uint64_t n_rays() const { return n_pix * per(); }
  // the pixel -> block map, all NIL, before any block exists
  int ensure_map(uint64_t n_pixels) {
    if (sub_block.p) return 0;
    if (int rc = sub_block.alloc(4 * n_pixels)) return rc;
    HIP_TRY(hipMemset(sub_block.p, 0xff, 4 * n_pixels));
    h_block.assign(n_pixels, grt::GBUFFER_NIL);
    return 0;
  }
  int reserve_pixels(uint64_t want) {
    if (want <= cap_pix) return 0;
    const uint64_t cap = std::max<uint64_t>({want, 2 * cap_pix, 1024});
    int rc;
    if ((rc = grow_buf(sub_pixel, 4 * n_pix, 4 * cap)) || (rc = arr.grow(false, n_rays(), cap * per()))) return rc;
    cap_pix = cap;
    return 0;
  }
  int reserve_layers(uint64_t want) {
    if (want <= cap_layers && arr.a[GB_object].p && (!timed || lapse.p)) return 0;
    const uint64_t cap = std::max<uint64_t>({want, 2 * cap_layers, 4096});
    if (int rc = arr.grow(true, n_layers, cap)) return rc;
    if (timed)
      if (int rc = grow_buf(lapse, 8 * n_layers, 8 * cap)) return rc;
    cap_layers = cap;
    return 0;
  }
  grt::GBufferArrays view() const { return arr.view(0, n_rays()); }
};

struct grt_gbuffer {
  grt_gbuffer_info info;
  double times[2] = {0.0, 0.0};  // trace, scan + fill (ms)
  GBufferDev arr;
  GBufferSub sub;
  // scratch of grt_gbuffer_shade_times: the layers' orbit rates, written once per call;
  // allocated by the first such call and kept (the buffer's layers never change)
  mutable DevBuf omega;
  // optional: each layer's light-travel time, n_layers doubles (grt_gbuffer_trace_lapse,
  // grt_gbuffer_lapse_upload); not one of the twelve arrays
  DevBuf lapse;
  bool has_lapse = false;
  grt_gbuffer() { std::memset(&info, 0, sizeof(info)); }
  grt::GBufferArrays view() const { return arr.view(0, info.n_pixels); }
};

// What a buffer records of the scene it was traced with, beside the camera: written by
// info_from_scene, held to the tracer of the sub-rays by check_tracer, byte for byte.
#define GRT_GBUFFER_RECORDED(X) X(max_steps) X(max_radius) X(step_size) X(epsilon) X(horizon_epsilon)

static void info_from_scene(const grt_scene_desc& d, const grt_camera_desc& camera, grt_gbuffer_info* info) {
  grt_gbuffer_shape_of(&d, &info->shape);
  info->camera = camera;
#define X(field) info->field = d.field;
  GRT_GBUFFER_RECORDED(X)
#undef X
}

// The sub-rays of a buffer belong to the frame it holds: the tracer's geometry (shape key),
// camera and integration parameters must be the recorded ones.  A stacked trace takes each
// frame's camera from the buffer's record (`camera` false): the tracer's own is then held
// to the frame size only.
static int check_tracer(const grt_gbuffer* gb, const grt_scene* t, bool camera = true) {
  if (int rc = grt_gbuffer_shape_compatible(&gb->info.shape, &t->desc)) return rc;
  auto differs = [](const char* field) {
    return fail(-EINVAL, std::string("g-buffer: the tracer differs from the traced scene in ") + field);
  };
  const grt_gbuffer_info& i = gb->info;
  if (camera && std::memcmp(&i.camera, &t->desc.camera, sizeof(i.camera)) != 0) return differs("camera");
  if (!camera && (t->desc.camera.rows != i.camera.rows || t->desc.camera.cols != i.camera.cols))
    return differs("camera.rows x camera.cols");
#define X(field) \
  if (std::memcmp(&i.field, &t->desc.field, sizeof(i.field)) != 0) return differs(#field);
  GRT_GBUFFER_RECORDED(X)
#undef X
  return 0;
}

// Trace `wl` with the exact kernels, waited for (trace_sync), the whole list again with a
// larger pool while a trace loses candidates: the workspace and pool a fill reads must be
// one complete trace's.  acc[3] is 0 on success; *n_traces (nullable) counts the traces.
static int trace_exact(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, const grt::Outputs& o,
                       unsigned long long acc[8], float* ms, const grt::CamTable* ct = nullptr,
                       uint32_t* n_traces = nullptr, bool lapse = false) {
  for (int traces = 1;; ++traces) {
    unsigned long long need = 0;
    acc[3] = 0;
    if (n_traces) ++*n_traces;
    if (int rc = trace_sync(s, dc, wl, o, acc, ms, &need, ct, true, lapse)) return rc;
    if (acc[3] == 0) return 0;
    if (traces == 3 || dc.pool_cap >= POOL_MAX)
      return fail(-ENOMEM, "the hit pool still overflows after " + std::to_string(traces) + " traces");
    if (int rc = ensure_pool(dc, need + need / 4)) return rc;
  }
}

// The layer scan's scratch, sized once per call for scans of at most `cap` rays.
struct LayerScan {
  DevBuf counts, temp;
  size_t temp_bytes = 0;
  int alloc(uint64_t cap) {
    if (int rc = counts.alloc(8 * (cap + 1))) return rc;
    HIP_TRY(grt::gbuffer_layer_scan(nullptr, nullptr, cap, nullptr, nullptr, nullptr, &temp_bytes, nullptr));
    return temp.alloc(temp_bytes);
  }
  // The scan of a trace's n rays on `st` into layer_start (n + 1 entries), then the entries
  // at the ray positions `at`, read back in order: one 8-byte copy each, the first waits.
  int run(const uint8_t* status, const uint32_t* hits, uint64_t n, uint64_t* layer_start, hipStream_t st,
          const std::vector<uint64_t>& at, std::vector<uint64_t>* starts) {
    HIP_TRY(grt::gbuffer_layer_scan(status, hits, n, (uint64_t*)counts.p, layer_start, temp.p, &temp_bytes, st));
    starts->assign(at.size(), 0);
    if (st) HIP_TRY(hipStreamSynchronize(st));  // a stream of its own: the copies below do not wait for it
    for (size_t q = 0; q < at.size(); ++q)
      HIP_TRY(hipMemcpy(&(*starts)[q], layer_start + at[q], 8, hipMemcpyDeviceToHost));
    return 0;
  }
};

// The fill of `gb` on `st` after a complete trace of the n rays of `wl`: the workspace as
// that trace carved it, its hit pool, and the fill kernel of the unit that traced -- the
// sequence unit's with a camera table, the lapse unit's with a lapse array (d_lapse, over the
// buffer's layers), else KerrBL's own or the default.
static int enqueue_fill(const grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, uint64_t n,
                        const grt::GBufferArrays& gb, hipStream_t st, const grt::CamTable* ct = nullptr,
                        double* d_lapse = nullptr) {
  grt::Workspace ws;
  if (int rc = ensure_workspace(dc, n, &ws)) return rc;
  ws.pool = dc.d_pool;
  const int geom = s->desc.geometry;
  if (d_lapse)
    HIP_TRY((geom == GRT_GEOM_KERR_BL ? grt::lapse_kerr_bl::launch_gbuffer_fill : grt::lapse::launch_gbuffer_fill)(
        geom, dc.d_scene, wl, ws, gb, st, d_lapse));
  else if (ct) HIP_TRY(grt::seq::launch_gbuffer_fill(geom, dc.d_scene, wl, ws, gb, st, *ct));
  else if (geom == GRT_GEOM_KERR_BL) HIP_TRY(grt::kerr_bl::launch_gbuffer_fill(geom, dc.d_scene, wl, ws, gb, st));
  else HIP_TRY(grt::launch_gbuffer_fill(geom, dc.d_scene, wl, ws, gb, st));
  return 0;
}

// ---- a row-band shard's buffer as one block, and the frame's buffer it goes into (api_internal.h) ----
static grt::GBufferArrays block_view(const GBufferBlock& B, uint8_t* b) {
  auto f64 = [&](int k) { return (double*)(b + B.off[k]); };
  return grt::GBufferArrays{B.n, b + B.off[GB_status], b + B.off[GB_stop], (const uint64_t*)(b + B.off[GB_layer_start]),
                            f64(GB_sky_u), f64(GB_sky_v), f64(GB_sky_redshift), b + B.off[GB_object], f64(GB_u),
                            f64(GB_v), f64(GB_redshift), f64(GB_radius)};
}

GRT_API_NAMESPACE {

// grt_gbuffer_trace's steps over the shard's work list, into the block instead of a buffer's
// own arrays, the scan and the fill on the caller's stream.
int gbuffer_trace_shard(grt_scene* s, int device, hipStream_t st, const grt_row_shard& sh,
                        const GBufferReserve& reserve, GBufferShard* R) {
  const grt::WorkList wl = shard_worklist(s, &sh);
  const uint64_t n = (uint64_t)wl.rows * wl.cols;
  DeviceCopy* dc;
  int rc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  GBufferBlock B(n, 0);
  uint8_t* base = nullptr;
  if ((rc = reserve(B.bytes, 0, &base))) return rc;
  if (n == 0) {  // layer_start's one entry
    HIP_TRY(hipMemsetAsync(base + B.off[GB_layer_start], 0, 8, st));
    HIP_TRY(hipStreamSynchronize(st));
    R->block = B;
    R->base = base;
    return 0;
  }
  DevBuf xyza, cls, hits;
  LayerScan scan;
  if ((rc = xyza.alloc(16 * n)) || (rc = cls.alloc(n)) || (rc = hits.alloc(4 * n)) || (rc = scan.alloc(n))) return rc;
  uint8_t* status = base + B.off[GB_status];
  uint64_t* layer_start = (uint64_t*)(base + B.off[GB_layer_start]);
  const grt::Outputs o{(float*)xyza.p, (uint8_t*)cls.p, status, nullptr, (uint32_t*)(base + B.off[GB_steps]),
                       base + B.off[GB_stop], (uint32_t*)hits.p};
  if ((rc = trace_exact(s, *dc, wl, o, R->acc, &R->trace_ms, nullptr, &R->n_traces))) return rc;
  if ((rc = stream_order(*dc, st))) return rc;
  HIP_TRY(hipEventRecord(dc->ev0, st));
  std::vector<uint64_t> total;  // the layers of the shard
  if ((rc = scan.run(status, (const uint32_t*)hits.p, n, layer_start, st, {n}, &total))) return rc;
  B = GBufferBlock(n, total[0]);
  if ((rc = reserve(B.bytes, B.ray_bytes, &base)) || (rc = enqueue_fill(s, *dc, wl, n, block_view(B, base), st)))
    return rc;
  HIP_TRY(hipEventRecord(dc->ev1, st));
  HIP_TRY(hipEventSynchronize(dc->ev1));
  HIP_TRY(hipEventElapsedTime(&R->fill_ms, dc->ev0, dc->ev1));
  if ((rc = stream_done(*dc, st))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  R->block = B;
  R->base = base;
  return 0;
}

int gbuffer_frame_alloc(const grt_scene* s, int device, uint64_t n_layers, grt_gbuffer** out, void* p[GB_N_FIELDS]) {
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<grt_gbuffer> gb(new grt_gbuffer());
  grt_gbuffer_info& info = gb->info;
  info.rows = (uint32_t)s->desc.camera.rows;
  info.cols = (uint32_t)s->desc.camera.cols;
  info.n_pixels = (uint64_t)info.rows * info.cols;
  info.n_layers = n_layers;
  info.device = device;
  info_from_scene(s->desc, s->desc.camera, &info);
  int rc;
  if ((rc = gb->arr.alloc(false, info.n_pixels)) || (rc = gb->arr.alloc(true, n_layers))) return rc;
  for (int k = 0; k < GB_N_FIELDS; ++k) p[k] = gb->arr.a[k].p;
  *out = gb.release();
  return 0;
}

void gbuffer_set_times(grt_gbuffer* gb, double trace_ms, double fill_ms) {
  gb->times[0] = trace_ms;
  gb->times[1] = fill_ms;
}

}  // namespace grt_api

// grt_gbuffer_trace, and with `lapse` grt_gbuffer_trace_lapse: the same steps through the
// lapse unit's trace and fill, the buffer's lapse array filled beside the twelve.
static int gbuffer_trace_impl(grt_scene* s, int device, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols,
                              grt_gbuffer** out, grt_stats* stats, bool lapse) {
  if (!s || !out) return fail(-EINVAL, "null argument");
  *out = nullptr;
  if (rows == 0 || cols == 0) return fail(-EINVAL, "empty rectangle");
  int rc = check_rect(s, row0, col0, rows, cols);
  if (rc) return rc;
  for (uint32_t k = 0; k < s->desc.n_objects; ++k)
    if (s->desc.objects[k].kind == GRT_OBJ_VOLUMETRIC_DISC)
      return fail(-ENOTSUP, "a VolumetricDisc's colour is raymarched: the scene has no geometry buffer");
  const uint64_t n = (uint64_t)rows * cols;
  if (n + 1 > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "more than INT_MAX - 1 pixels");
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<grt_gbuffer> gb(new grt_gbuffer());
  grt_gbuffer_info& info = gb->info;
  info.row0 = row0;
  info.col0 = col0;
  info.rows = rows;
  info.cols = cols;
  info.n_pixels = n;
  info.device = device;
  info_from_scene(s->desc, s->desc.camera, &info);
  GBufferDev& A = gb->arr;
  // the trace's other outputs, and the scan's scratch
  DevBuf xyza, cls, hits;
  LayerScan scan;
  if ((rc = A.alloc(false, n)) || (rc = xyza.alloc(16 * n)) || (rc = cls.alloc(n)) || (rc = hits.alloc(4 * n)) ||
      (rc = scan.alloc(n)))
    return rc;
  const grt::WorkList wl = rect_worklist(row0, col0, rows, cols);
  const grt::Outputs o{(float*)xyza.p, (uint8_t*)cls.p, A.status(), nullptr, A.steps(), A.stop(), (uint32_t*)hits.p};
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float ms = 0;
  if ((rc = trace_exact(s, *dc, wl, o, acc, &ms, nullptr, nullptr, lapse))) return rc;
  hipStream_t st = nullptr;
  if ((rc = stream_order(*dc, st))) return rc;
  HIP_TRY(hipEventRecord(dc->ev0, st));
  std::vector<uint64_t> total;  // the layers of the rectangle
  if ((rc = scan.run(A.status(), (const uint32_t*)hits.p, n, A.layer_start(), st, {n}, &total))) return rc;
  info.n_layers = total[0];
  if ((rc = A.alloc(true, info.n_layers))) return rc;
  if (lapse) {
    if ((rc = gb->lapse.alloc(8 * info.n_layers))) return rc;
    gb->has_lapse = true;
  }
  if ((rc = enqueue_fill(s, *dc, wl, n, gb->view(), st, nullptr, (double*)gb->lapse.p))) return rc;
  HIP_TRY(hipEventRecord(dc->ev1, st));
  HIP_TRY(hipEventSynchronize(dc->ev1));
  float fill_ms = 0;
  HIP_TRY(hipEventElapsedTime(&fill_ms, dc->ev0, dc->ev1));
  if ((rc = stream_done(*dc, st))) return rc;
  gb->times[0] = ms;
  gb->times[1] = fill_ms;
  // the overflows are 0 (trace_exact) and so are the march counters: only march_kernel
  // (volumetric.h) adds to them, and scenes with a VolumetricDisc are refused above
  if (stats) stats_from(acc, ms, stats);
  *out = gb.release();
  return 0;
}

extern "C" {

int grt_gbuffer_trace(grt_scene* s, int device, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols,
                      grt_gbuffer** out, grt_stats* stats) {
  return gbuffer_trace_impl(s, device, row0, col0, rows, cols, out, stats, false);
}

int grt_gbuffer_trace_lapse(grt_scene* s, int device, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols,
                            grt_gbuffer** out, grt_stats* stats) {
  return gbuffer_trace_impl(s, device, row0, col0, rows, cols, out, stats, true);
}

int grt_gbuffer_lapse_download(const grt_gbuffer* gb, double* out) {
  if (!gb || !out) return fail(-EINVAL, "null argument");
  if (!gb->has_lapse) return fail(-ENODATA, "the g-buffer holds no lapse (grt_gbuffer_trace_lapse, grt_gbuffer_lapse_upload)");
  HIP_TRY(hipSetDevice(gb->info.device));
  if (gb->info.n_layers) HIP_TRY(hipMemcpy(out, gb->lapse.p, 8 * gb->info.n_layers, hipMemcpyDeviceToHost));
  return 0;
}

int grt_gbuffer_lapse_upload(grt_gbuffer* gb, const double* lapse, uint64_t n_layers) {
  if (!gb || (!lapse && n_layers)) return fail(-EINVAL, "null argument");
  if (n_layers != gb->info.n_layers)
    return fail(-EINVAL, "a lapse of " + std::to_string(n_layers) + " entries for a g-buffer of " +
                             std::to_string(gb->info.n_layers) + " layers");
  for (uint64_t k = 0; k < n_layers; ++k)
    if (!std::isfinite(lapse[k])) return fail(-EINVAL, "lapse[" + std::to_string(k) + "] is not finite");
  HIP_TRY(hipSetDevice(gb->info.device));
  DevBuf fresh;
  if (int rc = fresh.alloc(8 * n_layers)) return rc;
  if (n_layers) HIP_TRY(hipMemcpy(fresh.p, lapse, 8 * n_layers, hipMemcpyHostToDevice));
  gb->lapse = std::move(fresh);  // what the buffer held is freed
  gb->has_lapse = true;
  return 0;
}

int grt_gbuffer_trace_times(const grt_gbuffer* gb, double ms[2]) {
  if (!gb || !ms) return fail(-EINVAL, "null argument");
  ms[0] = gb->times[0];
  ms[1] = gb->times[1];
  return 0;
}

int grt_gbuffer_info_get(const grt_gbuffer* gb, grt_gbuffer_info* out) {
  if (!gb || !out) return fail(-EINVAL, "null argument");
  *out = gb->info;
  return 0;
}

int grt_gbuffer_download(const grt_gbuffer* gb, const grt_gbuffer_arrays* h) {
  if (!gb || !h || GBufferPtrs(*h).missing(false)) return fail(-EINVAL, "null argument");
  const uint64_t n = gb->info.n_pixels, l = gb->info.n_layers;
  if (l && GBufferPtrs(*h).missing(true)) return fail(-EINVAL, "null layer array");
  HIP_TRY(hipSetDevice(gb->info.device));
  return gb->arr.copy(*h, n, l, hipMemcpyDeviceToHost);
}

int grt_gbuffer_upload(const grt_gbuffer_info* info, const grt_gbuffer_arrays* h, int device, grt_gbuffer** out) {
  if (!out) return fail(-EINVAL, "null argument");
  *out = nullptr;
  // the shade kernel indexes by layer_start and object: hold them to their ranges first
  int rc = grt_host::gbuffer_check_arrays(info, h);
  if (rc) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(-ENODEV, "invalid device ordinal");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<grt_gbuffer> gb(new grt_gbuffer());
  gb->info = *info;
  gb->info.device = device;
  gb->info._pad = 0;
  const uint64_t n = info->n_pixels, l = info->n_layers;
  if ((rc = gb->arr.alloc(false, n)) || (rc = gb->arr.alloc(true, l)) ||
      (rc = gb->arr.copy(*h, n, l, hipMemcpyHostToDevice)))
    return rc;
  *out = gb.release();
  return 0;
}

int grt_gbuffer_shade(grt_scene* s, const grt_gbuffer* gb, float* xyza_out, uint8_t* class_out, uint8_t* status_out,
                      double* xyza64_out, float* kernel_ms) {
  if (!s || !gb || !xyza_out || !class_out || !status_out) return fail(-EINVAL, "null argument");
  int rc = grt_gbuffer_shape_compatible(&gb->info.shape, &s->desc);
  if (rc) return rc;
  const int device = gb->info.device;
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  const uint64_t n = gb->info.n_pixels;
  DevBuf xyza, cls, status, x64;
  if ((rc = xyza.alloc(16 * n)) || (rc = cls.alloc(n)) || (rc = status.alloc(n))) return rc;
  if (xyza64_out && (rc = x64.alloc(32 * n))) return rc;
  const grt::Outputs o{(float*)xyza.p, (uint8_t*)cls.p, (uint8_t*)status.p, (double*)x64.p, nullptr, nullptr, nullptr};
  hipStream_t st = nullptr;
  HIP_TRY(hipEventRecord(dc->ev0, st));
  HIP_TRY(grt::launch_gbuffer_shade(dc->d_scene, gb->view(), o, st));
  HIP_TRY(hipEventRecord(dc->ev1, st));
  HIP_TRY(hipEventSynchronize(dc->ev1));
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, dc->ev0, dc->ev1));
  if (kernel_ms) *kernel_ms = t;
  HIP_TRY(hipMemcpy(xyza_out, xyza.p, 16 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(class_out, cls.p, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(status_out, status.p, n, hipMemcpyDeviceToHost));
  if (xyza64_out) HIP_TRY(hipMemcpy(xyza64_out, x64.p, 32 * n, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"

// ---- geometry buffers of a camera sequence (grt_api.h) ----
namespace {
struct GbSeqTimes {
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // as trace_sync's
  double trace_ms = 0.0, fill_ms = 0.0;
  uint32_t traces = 0;
};

// One launch group: the stacked 1-spp trace of the group's frames through the sequence unit,
// the layer scan and the fill over the whole stack in slot order (frame after frame), then
// the cut into one buffer per frame: device-to-device copies of the frame's slice of every
// array, and its layer_start rebased to 0 at its first pixel.  Appends the buffers to `made`.
// Not grt_gbuffer_trace's body: that one fills the buffer in place from a rectangle through
// the default / KerrBL unit; the two share LayerScan and enqueue_fill.
int gbuffer_sequence_group(grt_scene* s, DeviceCopy& dc, int device, const grt::CamTable& ct,
                           const grt_camera_desc* cameras, uint32_t rows, uint32_t cols,
                           std::vector<std::unique_ptr<grt_gbuffer>>& made, GbSeqTimes* T) {
  int rc;
  const uint32_t kg = ct.n_cams;
  const uint64_t per = (uint64_t)rows * cols, n = per * kg;
  GBufferDev stack;
  DevBuf xyza, cls, hits;
  LayerScan scan;
  if ((rc = stack.alloc(false, n)) || (rc = xyza.alloc(16 * n)) || (rc = cls.alloc(n)) || (rc = hits.alloc(4 * n)) ||
      (rc = scan.alloc(n)))
    return rc;
  const grt::WorkList wl = rect_worklist(0, 0, kg * rows, cols);
  const grt::Outputs o{(float*)xyza.p, (uint8_t*)cls.p,   stack.status(), nullptr,
                       stack.steps(),  stack.stop(),      (uint32_t*)hits.p};
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float ms = 0;
  if ((rc = trace_exact(s, dc, wl, o, acc, &ms, &ct, &T->traces))) return rc;
  hipStream_t st = nullptr;
  if ((rc = stream_order(dc, st))) return rc;
  HIP_TRY(hipEventRecord(dc.ev0, st));
  // where each frame's layers begin in the stack's, and the total
  std::vector<uint64_t> at(kg + 1), base;
  for (uint32_t f = 0; f <= kg; ++f) at[f] = per * f;
  if ((rc = scan.run(stack.status(), (const uint32_t*)hits.p, n, stack.layer_start(), st, at, &base))) return rc;
  if ((rc = stack.alloc(true, base[kg])) || (rc = enqueue_fill(s, dc, wl, n, stack.view(0, n), st, &ct))) return rc;
  const size_t first = made.size();
  for (uint32_t f = 0; f < kg; ++f) {
    std::unique_ptr<grt_gbuffer> gb(new grt_gbuffer());
    grt_gbuffer_info& info = gb->info;
    info.row0 = 0;
    info.col0 = 0;
    info.rows = rows;
    info.cols = cols;
    info.n_pixels = per;
    info.n_layers = base[f + 1] - base[f];
    info.device = device;
    info_from_scene(s->desc, cameras[f], &info);
    if ((rc = gb->arr.alloc(false, per)) || (rc = gb->arr.alloc(true, info.n_layers)) ||
        (rc = stack.copy_slice(gb->arr, 0, 0, per * f, base[f], per, info.n_layers, st)))
      return rc;
    HIP_TRY(grt::gbuffer_rebase(stack.layer_start() + per * f, per, gb->arr.layer_start(), st));
    made.push_back(std::move(gb));
  }
  HIP_TRY(hipEventRecord(dc.ev1, st));
  HIP_TRY(hipEventSynchronize(dc.ev1));  // the stacked arrays are freed on return
  float fill_ms = 0;
  HIP_TRY(hipEventElapsedTime(&fill_ms, dc.ev0, dc.ev1));
  if ((rc = stream_done(dc, st))) return rc;
  for (size_t k = first; k < made.size(); ++k) {
    made[k]->times[0] = ms;
    made[k]->times[1] = fill_ms;
  }
  for (int k = 0; k < 8; ++k) T->acc[k] += acc[k];
  T->trace_ms += ms;
  T->fill_ms += fill_ms;
  return 0;
}

// What every stacked call asks of its buffers: none null, and (check_frame) frame f on frame
// 0's device and of its size.  Per frame, because each caller has further checks of a frame
// and a refusal names the first frame with any fault.
int check_no_null_buffer(uint32_t n, grt_gbuffer* const* buffers) {
  for (uint32_t f = 0; f < n; ++f)
    if (!buffers[f]) return fail(-EINVAL, "frame " + std::to_string(f) + ": null buffer");
  return 0;
}
int check_frame(grt_gbuffer* const* buffers, uint32_t f) {
  const std::string frame = "frame " + std::to_string(f) + ": ";
  const grt_gbuffer_info &i = buffers[f]->info, &i0 = buffers[0]->info;
  if (i.device != i0.device)
    return fail(-EINVAL, frame + "the g-buffer is on device " + std::to_string(i.device) + ", frame 0's on device " +
                             std::to_string(i0.device));
  if (i.rows != i0.rows || i.cols != i0.cols)
    return fail(-EINVAL, frame + "the g-buffer has " + std::to_string(i.rows) + " x " + std::to_string(i.cols) +
                             " pixels, frame 0's " + std::to_string(i0.rows) + " x " + std::to_string(i0.cols));
  return 0;
}
}  // namespace

extern "C" {

int grt_gbuffer_trace_sequence(grt_scene* s, int device, uint32_t n_cameras, const grt_camera_desc* cameras,
                               grt_gbuffer** out, grt_stats* stats, grt_gbuffer_sequence_report* report) {
  const auto wall0 = std::chrono::steady_clock::now();
  if (out)
    for (uint32_t f = 0; f < n_cameras; ++f) out[f] = nullptr;
  if (!s || !cameras || !out) return fail(-EINVAL, "null argument");
  if (n_cameras == 0) return fail(-EINVAL, "a sequence needs at least one camera");
  const int64_t rows64 = s->desc.camera.rows, cols64 = s->desc.camera.cols;
  for (uint32_t f = 0; f < n_cameras; ++f)
    if (cameras[f].rows != rows64 || cameras[f].cols != cols64)
      return fail(-EINVAL, "camera " + std::to_string(f) + " of the sequence has " + std::to_string(cameras[f].rows) +
                               " x " + std::to_string(cameras[f].cols) + " pixels, the scene's frame " +
                               std::to_string(rows64) + " x " + std::to_string(cols64));
  for (uint32_t k = 0; k < s->desc.n_objects; ++k)
    if (s->desc.objects[k].kind == GRT_OBJ_VOLUMETRIC_DISC)
      return fail(-ENOTSUP, "a VolumetricDisc's colour is raymarched: the scene has no geometry buffer");
  const uint32_t rows = (uint32_t)rows64, cols = (uint32_t)cols64;
  const uint64_t per = (uint64_t)rows * cols;
  if (per == 0) return fail(-EINVAL, "empty frame");
  if (per + 1 > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "more than INT_MAX - 1 pixels");
  // frames per launch group: grt_render_sequence's arithmetic; the scan runs over n + 1 entries
  const uint64_t g = frames_per_group(per, n_cameras, (uint64_t)INT_MAX - 1, rows);
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  DevBuf b_cams;
  grt::CamTable all;
  if ((rc = upload_cam_table(cameras, n_cameras, rows, b_cams, &all))) return rc;
  // the buffers die with `made` on any failure below
  std::vector<std::unique_ptr<grt_gbuffer>> made;
  made.reserve(n_cameras);
  GbSeqTimes T;
  uint32_t launches = 0;
  for (uint32_t f0 = 0; f0 < n_cameras; f0 += (uint32_t)g, ++launches) {
    const uint32_t kg = (uint32_t)std::min<uint64_t>(g, n_cameras - f0);
    const grt::CamTable ct{all.cams + f0, rows, kg};
    if ((rc = gbuffer_sequence_group(s, *dc, device, ct, cameras + f0, rows, cols, made, &T))) return rc;
  }
  if (stats) stats_from(T.acc, T.trace_ms, stats);  // as grt_gbuffer_trace: no overflows, no raymarch
  if (report) {
    std::memset(report, 0, sizeof(*report));
    report->n_frames = n_cameras;
    report->n_launches = launches;
    report->frames_per_launch = (uint32_t)g;
    report->n_traces = T.traces;
    report->trace_ms = T.trace_ms;
    report->fill_ms = T.fill_ms;
    report->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  }
  for (uint32_t f = 0; f < n_cameras; ++f) out[f] = made[f].release();
  return 0;
}

int grt_gbuffer_shade_sequence(grt_scene* s, uint32_t n_buffers, grt_gbuffer* const* buffers, const grt_frame_out* out,
                               float* kernel_ms) {
  if (!s || !buffers || !out) return fail(-EINVAL, "null argument");
  if (n_buffers == 0) return fail(-EINVAL, "a sequence needs at least one buffer");
  if (!out->xyza && !out->xyza64) return fail(-EINVAL, "grt_frame_out needs xyza or xyza64");
  int rc;
  if ((rc = check_no_null_buffer(n_buffers, buffers))) return rc;
  // no more than that: a re-shade takes rectangles, and the same buffer twice
  for (uint32_t f = 0; f < n_buffers; ++f) {
    if ((rc = check_frame(buffers, f))) return rc;
    if ((rc = grt_gbuffer_shape_compatible(&buffers[f]->info.shape, &s->desc)))
      return fail(rc, "frame " + std::to_string(f) + ": " + grt_last_error());
  }
  const int device = buffers[0]->info.device;
  const uint64_t per = buffers[0]->info.n_pixels;
  if (per == 0 || per > (uint64_t)INT_MAX) return fail(-EINVAL, "frames of 0 or more than INT_MAX pixels");
  const uint64_t g = frames_per_group(per, n_buffers);
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  const uint64_t ng = per * g;  // slots of a full group
  DevBuf xyza, cls, status, x64, stop, steps, table;
  if ((rc = xyza.alloc(16 * ng)) || (rc = cls.alloc(ng)) || (rc = status.alloc(ng))) return rc;
  if (out->xyza64 && (rc = x64.alloc(32 * ng))) return rc;
  if (out->stop && (rc = stop.alloc(ng))) return rc;
  if (out->steps && (rc = steps.alloc(4 * ng))) return rc;
  std::vector<grt::GBufferFrame> frames(n_buffers);
  for (uint32_t f = 0; f < n_buffers; ++f) frames[f] = grt::GBufferFrame{buffers[f]->view(), buffers[f]->arr.steps()};
  if ((rc = table.alloc(n_buffers * sizeof(grt::GBufferFrame)))) return rc;
  HIP_TRY(hipMemcpy(table.p, frames.data(), n_buffers * sizeof(grt::GBufferFrame), hipMemcpyHostToDevice));
  const grt::Outputs o{(float*)xyza.p,     (uint8_t*)cls.p,  (uint8_t*)status.p, (double*)x64.p,
                       (uint32_t*)steps.p, (uint8_t*)stop.p, nullptr};
  hipStream_t st = nullptr;
  float total_ms = 0;
  for (uint32_t f0 = 0; f0 < n_buffers; f0 += (uint32_t)g) {
    const uint32_t kg = (uint32_t)std::min<uint64_t>(g, n_buffers - f0);
    const uint64_t n = per * kg, at = per * f0;
    HIP_TRY(hipEventRecord(dc->ev0, st));
    HIP_TRY(grt::launch_gbuffer_shade_stack(dc->d_scene, (const grt::GBufferFrame*)table.p + f0, kg, per, o, st));
    HIP_TRY(hipEventRecord(dc->ev1, st));
    HIP_TRY(hipEventSynchronize(dc->ev1));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, dc->ev0, dc->ev1));
    total_ms += t;
    if (out->xyza) HIP_TRY(hipMemcpy(out->xyza + 4 * at, xyza.p, 16 * n, hipMemcpyDeviceToHost));
    if (out->xyza64) HIP_TRY(hipMemcpy(out->xyza64 + 4 * at, x64.p, 32 * n, hipMemcpyDeviceToHost));
    if (out->ray_class) HIP_TRY(hipMemcpy(out->ray_class + at, cls.p, n, hipMemcpyDeviceToHost));
    if (out->status) HIP_TRY(hipMemcpy(out->status + at, status.p, n, hipMemcpyDeviceToHost));
    if (out->stop) HIP_TRY(hipMemcpy(out->stop + at, stop.p, n, hipMemcpyDeviceToHost));
    if (out->steps) HIP_TRY(hipMemcpy(out->steps + at, steps.p, 4 * n, hipMemcpyDeviceToHost));
  }
  if (kernel_ms) *kernel_ms = total_ms;
  return 0;
}

}  // extern "C"

// ---- the sub-sample set and the adaptive re-shade (grt_api.h) ----
static int check_spa(const grt_gbuffer* gb, uint32_t spa) {
  if (spa == 0) return fail(-EINVAL, "adaptive_sampling.samples_per_axis must be greater than zero");
  if (spa > 64) return fail(-EINVAL, "samples_per_axis is more than 64");
  if (gb->sub.spa && gb->sub.spa != spa)
    return fail(-EINVAL, "g-buffer: samples_per_axis " + std::to_string(spa) + " differs from the sub-sample set's " +
                             std::to_string(gb->sub.spa));
  return 0;
}

// Trace the sub-rays of `px` (ascending, unique, none held) and append them to the set:
// enqueue_supersample's machinery -- jitter offsets, the offset-list trace, in chunks of
// grt_set_sub_chunk -- with the exact kernels and the `hits` output, then per chunk the
// layer scan (one host sync for the layer total), the growth of the arrays and the fill.
// The fill is gbuffer_fill_kernel over the chunk's own work list, its arrays pointing at
// the chunk's place in the set; a chunk launches exactly its rays, so no live count.
// acc / ms[2]: counters and event times (trace; scan + fill), added to.
// `lapse` decides the kind of an empty set: timed (the lapse units trace and fill, the set's
// lapse array written at the set-wide layer offsets beside the twelve) or untimed (the exact
// units, as ever).  A set that holds blocks keeps its kind, whoever asks.
static int sub_fill(grt_scene* tracer, grt_gbuffer* gb, uint32_t spa, const std::vector<uint32_t>& px,
                    unsigned long long acc[8], double ms[2], bool lapse = false) {
  const uint64_t m = px.size();
  if (m == 0) return 0;
  const grt_gbuffer_info& info = gb->info;
  GBufferSub& S = gb->sub;
  DeviceCopy* dc;
  int rc;
  if ((rc = ensure_device(tracer, info.device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(info.device));
  if ((rc = S.ensure_map(info.n_pixels))) return rc;
  S.spa = spa;
  if (S.n_pix == 0) S.timed = lapse;
  const bool timed = S.timed;
  const uint64_t per = S.per();
  if ((S.n_pix + m) * per + 1 > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "more than INT_MAX - 1 sub-rays");
  SuperBufs C;  // the chunking of enqueue_supersample; the buffers are this call's own
  C.plan(m, spa);
  const uint64_t chunk_pix = C.chunk_pix, cap = C.cap;
  DevBuf d_px, pix, dx, dy, xyza, cls, hits, local;
  LayerScan scan;
  if ((rc = d_px.alloc(4 * m)) || (rc = pix.alloc(4 * cap)) || (rc = dx.alloc(8 * cap)) || (rc = dy.alloc(8 * cap)) ||
      (rc = xyza.alloc(16 * cap)) || (rc = cls.alloc(cap)) || (rc = hits.alloc(4 * cap)) ||
      (rc = local.alloc(8 * (cap + 1))) || (rc = scan.alloc(cap)))
    return rc;
  HIP_TRY(hipMemcpy(d_px.p, px.data(), 4 * m, hipMemcpyHostToDevice));
  hipStream_t st = nullptr;
  std::vector<uint64_t> total;  // the chunk's layers
  for (uint64_t base = 0; base < m; base += chunk_pix) {
    const uint64_t mc = std::min(chunk_pix, m - base), nr = mc * per;
    if ((rc = S.reserve_pixels(S.n_pix + mc))) return rc;
    const uint64_t off = S.n_rays();
    const uint32_t* d_chunk = (const uint32_t*)d_px.p + base;
    HIP_TRY(grt::launch_make_offsets(d_chunk, mc, nullptr, 0, spa, info.row0, info.col0, info.cols, (uint32_t*)pix.p,
                                     (double*)dx.p, (double*)dy.p, st));
    const grt::WorkList wo = offsets_worklist(info.row0, info.col0, info.rows, info.cols, nr, (const uint32_t*)pix.p,
                                              (const double*)dx.p, (const double*)dy.p);
    const grt::Outputs o{(float*)xyza.p,         (uint8_t*)cls.p,       S.arr.status() + off, nullptr,
                         S.arr.steps() + off,    S.arr.stop() + off,    (uint32_t*)hits.p};
    float t_ms = 0;
    if ((rc = trace_exact(tracer, *dc, wo, o, acc, &t_ms, nullptr, nullptr, timed))) return rc;
    ms[0] += t_ms;
    if ((rc = stream_order(*dc, st))) return rc;
    HIP_TRY(hipEventRecord(dc->ev0, st));
    if ((rc = scan.run(S.arr.status() + off, (const uint32_t*)hits.p, nr, (uint64_t*)local.p, st, {nr}, &total)))
      return rc;
    const uint64_t n_new = total[0];
    if ((rc = S.reserve_layers(S.n_layers + n_new))) return rc;
    HIP_TRY(grt::gbuffer_sub_append((const uint64_t*)local.p, nr, S.n_layers, S.arr.layer_start() + off, d_chunk, mc,
                                    (uint32_t)S.n_pix, (uint32_t*)S.sub_block.p, (uint32_t*)S.sub_pixel.p, st));
    if ((rc = enqueue_fill(tracer, *dc, wo, nr, S.arr.view(off, nr), st, nullptr,
                           timed ? (double*)S.lapse.p : nullptr)))
      return rc;
    HIP_TRY(hipEventRecord(dc->ev1, st));
    HIP_TRY(hipEventSynchronize(dc->ev1));
    float f_ms = 0;
    HIP_TRY(hipEventElapsedTime(&f_ms, dc->ev0, dc->ev1));
    ms[1] += f_ms;
    if ((rc = stream_done(*dc, st))) return rc;
    for (uint64_t j = 0; j < mc; ++j) S.h_block[px[base + j]] = (uint32_t)(S.n_pix + j);
    S.n_pix += mc;
    S.n_layers += n_new;
  }
  return 0;
}

// ---- the sub-sample sets of a stack of buffers (grt_gbuffer_supersample_sequence) ----
// What a stacked call asks of its buffers: distinct whole frames of one size on one device,
// and, for the sub-ray pass, a samples_per_axis every existing set agrees with and a tracer
// (nullable) that check_tracer accepts for every frame, the camera aside.  Every refusal
// names the frame.
static int check_sequence_buffers(uint32_t n, grt_gbuffer* const* buffers, bool sub_pass, uint32_t spa,
                                  const grt_scene* tracer) {
  if (!buffers) return fail(-EINVAL, "null argument");
  if (n == 0) return fail(-EINVAL, "a sequence needs at least one buffer");
  if (int rc = check_no_null_buffer(n, buffers)) return rc;
  const grt_gbuffer_info& i0 = buffers[0]->info;
  for (uint32_t f = 0; f < n; ++f) {
    const std::string frame = "frame " + std::to_string(f) + ": ";
    const grt_gbuffer_info& i = buffers[f]->info;
    for (uint32_t g = 0; g < f; ++g)
      if (buffers[g] == buffers[f]) return fail(-EINVAL, frame + "the g-buffer is frame " + std::to_string(g) + "'s too");
    if (int rc = check_frame(buffers, f)) return rc;
    if (i.row0 != 0 || i.col0 != 0 || (int64_t)i.rows != i.camera.rows || (int64_t)i.cols != i.camera.cols)
      return fail(-EINVAL, frame + "the g-buffer holds the rectangle (" + std::to_string(i.row0) + ", " +
                               std::to_string(i.col0) + ", " + std::to_string(i.rows) + ", " + std::to_string(i.cols) +
                               ") of a frame of " + std::to_string(i.camera.rows) + " x " +
                               std::to_string(i.camera.cols) + " pixels, not the whole frame");
    if (sub_pass && check_spa(buffers[f], spa)) return fail(-EINVAL, frame + grt_last_error());
    if (sub_pass && buffers[f]->sub.timed)  // the stacked traces take camera tables, which lapse traces refuse
      return fail(-EINVAL, frame + "the g-buffer's sub-sample set is timed (it holds lapses): the stacked calls "
                               "fill and shade untimed sets only");
    if (tracer)
      if (int rc = check_tracer(buffers[f], tracer, false)) return fail(rc, frame + grt_last_error());
  }
  if (i0.n_pixels == 0 || (uint64_t)n * i0.n_pixels > 0xffffffffull || (uint64_t)n * i0.rows > 0xffffffffull)
    return fail(-EINVAL, "the stack of " + std::to_string(n) + " frames has 0 or more than 2^32 - 1 pixels");
  return 0;
}

// The pixels of `pixels` that buffer f does not hold yet, ascending and unique
// (ascending pixel index: two runs append the same bytes).  prefix: "frame k: " of a stack.
static int missing_of(const std::string& prefix, const grt_gbuffer* gb, uint64_t n, const uint32_t* pixels,
                      std::vector<uint32_t>* px) {
  px->clear();
  px->reserve(n);
  for (uint64_t k = 0; k < n; ++k) {
    if (pixels[k] >= gb->info.n_pixels)
      return fail(-EINVAL, prefix + "g-buffer: pixel " + std::to_string(pixels[k]) + " is outside the " +
                               std::to_string(gb->info.n_pixels) + " pixels of the buffer");
    if (gb->sub.h_block.empty() || gb->sub.h_block[pixels[k]] == grt::GBUFFER_NIL) px->push_back(pixels[k]);
  }
  std::sort(px->begin(), px->end());
  px->erase(std::unique(px->begin(), px->end()), px->end());
  return 0;
}

struct SubSeqTimes {
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // as trace_sync's
  double trace_ms = 0.0, fill_ms = 0.0;
  uint32_t traces = 0, chunks = 0;
};

// sub_fill for K buffers at once (check_sequence_buffers holds): px[k] are buffer k's new
// pixels (ascending, unique, none held).  The lists are concatenated frame-major as stacked
// indices P = k * rows * cols + p and cut into chunks of grt_set_sub_chunk sub-rays, so a
// chunk may span frames.  Per chunk: the stacked jitter offsets, one offset-list trace
// through the sequence unit over the stack of K * rows rows with the buffers' recorded
// cameras as the table (trace_exact: a chunk that loses candidates is traced again), one
// layer scan and one gbuffer_fill_kernel launch of that unit into a transient stacked set,
// then the cut: per frame of the chunk, device-to-device copies of its slice of every array
// to the end of its own set, and gbuffer_sub_append with the layer offsets rebased from the
// chunk's to the set's.  The sets' counts move only after a chunk is complete.
// Not sub_fill's body: that one runs the default / KerrBL unit straight into the set and
// accepts rectangle buffers; this one the sequence unit over whole frames, into a stack.
static int sub_fill_sequence(grt_scene* tracer, uint32_t K, grt_gbuffer* const* buffers, uint32_t spa,
                             const std::vector<std::vector<uint32_t>>& px, SubSeqTimes* T) {
  const grt_gbuffer_info& i0 = buffers[0]->info;
  const uint32_t rows = i0.rows, cols = i0.cols;
  const uint64_t npix = i0.n_pixels, per = (uint64_t)spa * spa;
  std::vector<uint64_t> start(K + 1, 0);
  for (uint32_t k = 0; k < K; ++k) start[k + 1] = start[k] + px[k].size();
  const uint64_t m = start[K];
  if (m == 0) return 0;
  if (m * per + 1 > (uint64_t)INT_MAX)
    return fail(-EINVAL, "g-buffer: more than INT_MAX - 1 stacked sub-rays (" + std::to_string(m) + " pixels x " +
                             std::to_string(per) + ")");
  for (uint32_t k = 0; k < K; ++k)
    if ((buffers[k]->sub.n_pix + px[k].size()) * per + 1 > (uint64_t)INT_MAX)
      return fail(-EOVERFLOW, "frame " + std::to_string(k) + ": more than INT_MAX - 1 sub-rays");
  DeviceCopy* dc;
  int rc;
  if ((rc = ensure_device(tracer, i0.device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(i0.device));
  std::vector<uint32_t> h_local(m), h_stack(m);
  for (uint32_t k = 0; k < K; ++k)
    for (uint64_t j = 0; j < px[k].size(); ++j) {
      h_local[start[k] + j] = px[k][j];
      h_stack[start[k] + j] = (uint32_t)(k * npix + px[k][j]);
    }
  std::vector<grt_camera_desc> cams(K);  // the buffers' recorded cameras
  for (uint32_t k = 0; k < K; ++k) cams[k] = buffers[k]->info.camera;
  DevBuf b_cams;
  grt::CamTable ct;
  if ((rc = upload_cam_table(cams.data(), K, rows, b_cams, &ct))) return rc;
  for (uint32_t k = 0; k < K; ++k) {
    if (px[k].empty()) continue;
    if ((rc = buffers[k]->sub.ensure_map(npix))) return rc;
    buffers[k]->sub.spa = spa;
  }
  SuperBufs C;  // the chunking of enqueue_supersample, over the concatenation
  C.plan(m, spa);
  const uint64_t chunk_pix = C.chunk_pix, cap = C.cap;
  DevBuf d_local, d_stack, pix, dx, dy, xyza, cls, hits;
  GBufferDev stack;  // the transient stacked set of one chunk; its layer_start is the chunk's own scan
  LayerScan scan;
  if ((rc = d_local.alloc(4 * m)) || (rc = d_stack.alloc(4 * m)) || (rc = pix.alloc(4 * cap)) ||
      (rc = dx.alloc(8 * cap)) || (rc = dy.alloc(8 * cap)) || (rc = xyza.alloc(16 * cap)) || (rc = cls.alloc(cap)) ||
      (rc = hits.alloc(4 * cap)) || (rc = stack.alloc(false, cap)) || (rc = scan.alloc(cap)))
    return rc;
  uint64_t cap_layers = 0;
  HIP_TRY(hipMemcpy(d_local.p, h_local.data(), 4 * m, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_stack.p, h_stack.data(), 4 * m, hipMemcpyHostToDevice));
  hipStream_t st = nullptr;
  struct Seg {
    uint32_t frame;
    uint64_t a, b;  // the frame's pixels of the chunk, [a, b) of its mc
  };
  std::vector<Seg> segs;
  std::vector<uint64_t> at;  // each segment's first ray of the chunk, then the chunk's end
  std::vector<uint64_t> lb;  // the chunk's layer offset there: each segment's first, then the total
  uint32_t k0 = 0;           // first frame that may have pixels in the chunk
  for (uint64_t base = 0; base < m; base += chunk_pix) {
    const uint64_t mc = std::min(chunk_pix, m - base), nr = mc * per;
    segs.clear();
    while (start[k0 + 1] <= base) ++k0;
    for (uint32_t k = k0; k < K && start[k] < base + mc; ++k) {
      const uint64_t a = std::max(start[k], base), b = std::min(start[k + 1], base + mc);
      if (a < b) segs.push_back(Seg{k, a - base, b - base});
    }
    HIP_TRY(grt::launch_make_offsets_stack((const uint32_t*)d_stack.p + base, mc, spa, rows, cols, (uint32_t*)pix.p,
                                           (double*)dx.p, (double*)dy.p, st));
    const grt::WorkList wo = offsets_worklist(0, 0, K * rows, cols, nr, (const uint32_t*)pix.p, (const double*)dx.p,
                                              (const double*)dy.p);
    const grt::Outputs o{(float*)xyza.p, (uint8_t*)cls.p, stack.status(), nullptr,
                         stack.steps(),  stack.stop(),    (uint32_t*)hits.p};
    float t_ms = 0;
    ++T->chunks;
    if ((rc = trace_exact(tracer, *dc, wo, o, T->acc, &t_ms, &ct, &T->traces))) return rc;
    T->trace_ms += t_ms;
    if ((rc = stream_order(*dc, st))) return rc;
    HIP_TRY(hipEventRecord(dc->ev0, st));
    at.clear();
    for (const Seg& g : segs) at.push_back(g.a * per);
    at.push_back(nr);
    if ((rc = scan.run(stack.status(), (const uint32_t*)hits.p, nr, stack.layer_start(), st, at, &lb))) return rc;
    const uint64_t total = lb.back();
    if (total > cap_layers || !stack.a[GB_object].p) {  // nothing of the last chunk is kept
      const uint64_t want = std::max<uint64_t>({total, 2 * cap_layers, 4096});
      if ((rc = stack.alloc(true, want))) return rc;
      cap_layers = want;
    }
    if ((rc = enqueue_fill(tracer, *dc, wo, nr, stack.view(0, nr), st, &ct))) return rc;
    for (size_t q = 0; q < segs.size(); ++q) {
      GBufferSub& S = buffers[segs[q].frame]->sub;
      const uint64_t mk = segs[q].b - segs[q].a, nk = mk * per, r0 = segs[q].a * per;
      const uint64_t l0 = lb[q], nl = lb[q + 1] - lb[q];
      if ((rc = S.reserve_pixels(S.n_pix + mk)) || (rc = S.reserve_layers(S.n_layers + nl))) return rc;
      const uint64_t off = S.n_rays(), loff = S.n_layers;
      if ((rc = stack.copy_slice(S.arr, off, loff, r0, l0, nk, nl, st))) return rc;
      // layer_start[off + i] = the chunk's [r0 + i] - l0 + loff: the rebase, in wrapping u64 arithmetic
      HIP_TRY(grt::gbuffer_sub_append(stack.layer_start() + r0, nk, loff - l0, S.arr.layer_start() + off,
                                      (const uint32_t*)d_local.p + base + segs[q].a, mk, (uint32_t)S.n_pix,
                                      (uint32_t*)S.sub_block.p, (uint32_t*)S.sub_pixel.p, st));
    }
    HIP_TRY(hipEventRecord(dc->ev1, st));
    HIP_TRY(hipEventSynchronize(dc->ev1));
    float f_ms = 0;
    HIP_TRY(hipEventElapsedTime(&f_ms, dc->ev0, dc->ev1));
    T->fill_ms += f_ms;
    if ((rc = stream_done(*dc, st))) return rc;
    for (size_t q = 0; q < segs.size(); ++q) {
      GBufferSub& S = buffers[segs[q].frame]->sub;
      const uint64_t mk = segs[q].b - segs[q].a;
      for (uint64_t j = 0; j < mk; ++j) S.h_block[h_local[base + segs[q].a + j]] = (uint32_t)(S.n_pix + j);
      S.n_pix += mk;
      S.n_layers += lb[q + 1] - lb[q];
    }
  }
  return 0;
}

// grt_gbuffer_supersample, and with `lapse` grt_gbuffer_supersample_lapse.
static int supersample_impl(grt_scene* tracer, grt_gbuffer* gb, uint32_t spa, uint64_t n, const uint32_t* pixels,
                            grt_stats* stats, bool lapse) {
  if (!tracer || !gb || (n && !pixels)) return fail(-EINVAL, "null argument");
  int rc;
  if ((rc = check_spa(gb, spa)) || (rc = check_tracer(gb, tracer))) return rc;
  if (lapse && gb->sub.n_pix && !gb->sub.timed)
    return fail(-EINVAL, "g-buffer: the sub-sample set of " + std::to_string(gb->sub.n_pix) +
                             " pixels is untimed (it holds no lapse): grt_gbuffer_sub_clear it, or give it one "
                             "(grt_gbuffer_sub_lapse_upload)");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  std::vector<uint32_t> px;
  if ((rc = missing_of("", gb, n, pixels, &px))) return rc;
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double ms[2] = {0.0, 0.0};
  if ((rc = sub_fill(tracer, gb, spa, px, acc, ms, lapse))) return rc;
  if (stats) stats_from(acc, (float)ms[0], stats);
  return 0;
}

extern "C" {

int grt_gbuffer_supersample(grt_scene* tracer, grt_gbuffer* gb, uint32_t spa, uint64_t n, const uint32_t* pixels,
                            grt_stats* stats) {
  return supersample_impl(tracer, gb, spa, n, pixels, stats, false);
}

int grt_gbuffer_supersample_lapse(grt_scene* tracer, grt_gbuffer* gb, uint32_t spa, uint64_t n, const uint32_t* pixels,
                                  grt_stats* stats) {
  return supersample_impl(tracer, gb, spa, n, pixels, stats, true);
}

}  // extern "C"

// grt_gbuffer_shade_section (SECTION_STATIC: the static kernels, exactly its launches),
// grt_gbuffer_shade_section_at (SECTION_AT: the kernels at `time`) and
// grt_gbuffer_shade_section_at_retarded (SECTION_AT_RETARDED: the kernels at `time` + each
// layer's lapse): one pipeline.  The mode picks the 1-spp launch and the sub-ray launch and
// nothing else.  The set is geometry: a top-up appends what grt_gbuffer_supersample leaves,
// whatever the time; the retarded mode needs a timed set, and fills an empty one timed.
enum SectionMode { SECTION_STATIC, SECTION_AT, SECTION_AT_RETARDED };
static int shade_section_impl(grt_scene* s, grt_gbuffer* gb, const grt_adaptive_config* cfg, const double* mask_xyza,
                              grt_scene* tracer, double* xyza_out, uint8_t* class_out, uint8_t* status_out,
                              uint64_t* n_supersampled, grt_subsample_failures* failures,
                              grt_gbuffer_section_report* report, SectionMode mode, double time) {
  if (!s || !gb || !cfg || !xyza_out) return fail(-EINVAL, "null argument");
  if (mode != SECTION_STATIC && !std::isfinite(time)) return fail(-EINVAL, "g-buffer: the time is not finite");
  const bool retarded = mode == SECTION_AT_RETARDED;
  if (retarded && !gb->has_lapse)
    return fail(-ENODATA, "the g-buffer holds no lapse (grt_gbuffer_trace_lapse, grt_gbuffer_lapse_upload)");
  if (cfg->samples_per_axis == 0) return fail(-EINVAL, "adaptive_sampling.samples_per_axis must be greater than zero");
  int rc = grt_gbuffer_shape_compatible(&gb->info.shape, &s->desc);
  if (rc) return rc;
  const bool supersampled = cfg->enabled || mask_xyza != nullptr;
  const bool sub_pass = supersampled && !mask_xyza;
  const uint32_t spa = cfg->samples_per_axis;
  if (sub_pass && (rc = check_spa(gb, spa))) return rc;
  if (sub_pass && tracer && (rc = check_tracer(gb, tracer))) return rc;
  if (report) std::memset(report, 0, sizeof(*report));
  if (retarded && sub_pass && gb->sub.n_pix && !gb->sub.timed)
    return fail(-ENODATA, "g-buffer: the sub-sample set of " + std::to_string(gb->sub.n_pix) + " pixels and " +
                              std::to_string(gb->sub.n_layers) + " layers is untimed (it holds no lapse): "
                              "grt_gbuffer_sub_clear it, or give it one (grt_gbuffer_sub_lapse_upload)");
  if (n_supersampled) *n_supersampled = 0;
  if (failures) failures->count = 0;
  const int device = gb->info.device;
  const uint32_t w = gb->info.cols, h = gb->info.rows;
  const uint64_t n = gb->info.n_pixels;
  if (n > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "section larger than INT_MAX pixels");
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::unique_lock<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  GBufferSub& S = gb->sub;
  if (sub_pass && (rc = S.ensure_map(n))) return rc;
  // the section's buffers, then the selection's, then one chunk of sub-ray outputs; the
  // counts: [0] selected, [1] failed sub-samples, [2] held, [3] missing
  AdaptivePlan P;
  P.n = n;
  P.w = w;
  P.h = h;
  P.spa = spa;
  P.held = true;
  P.supersampled = supersampled;
  P.device_floor = supersampled && !cfg->has_minimum_luminance;
  P.sub_rays = sub_pass;
  if ((rc = P.plan(*dc, sub_pass ? failures : nullptr))) return rc;  // the mask records no failures
  const SectionBufs& b = P.sec;
  const SuperBufs& B = P.B;
  unsigned long long* const d_cnt = P.d_cnt;
  hipStream_t st = nullptr;
  float shade_ms = 0;
  unsigned long long cnt[4] = {0, 0, 0, 0};
  // split the selection by what the set holds, shade the held sub-rays, average them
  auto enqueue_sub_pass = [&]() -> int {
    HIP_TRY(hipMemsetAsync(d_cnt + 1, 0, 24, st));
    HIP_TRY(grt::gbuffer_split(P.sel, d_cnt, n, (const uint32_t*)S.sub_block.p, P.split, P.held_px, d_cnt + 2,
                               P.missing_px, d_cnt + 3, P.split_tmp, &P.split_bytes, st));
    if (S.n_pix == 0) return 0;  // nothing held: every selected pixel is missing
    grt::SubsampleFailures fails = P.fails[0].f;
    fails.count = d_cnt + 1;
    fails.ray_stop = B.stop;
    fails.ray_steps = B.steps;
    const grt::Outputs so{B.xyza, B.cls, B.status, B.x64, B.steps, B.stop, nullptr};
    const grt::GBufferArrays sv = S.view();
    for (uint32_t c = 0; c < B.n_chunks; ++c) {
      const uint64_t base = (uint64_t)c * B.chunk_pix;
      if (retarded)
        HIP_TRY(grt::launch_gbuffer_shade_sub_at_retarded(dc->d_scene, sv, S.arr.steps(), (const uint32_t*)S.sub_block.p,
                                                          P.held_px + base, B.chunk_pix, d_cnt + 2, base, spa, time,
                                                          (const double*)S.lapse.p, so, st));
      else if (mode == SECTION_AT)
        HIP_TRY(grt::launch_gbuffer_shade_sub_at(dc->d_scene, sv, S.arr.steps(), (const uint32_t*)S.sub_block.p,
                                                 P.held_px + base, B.chunk_pix, d_cnt + 2, base, spa, time, so, st));
      else
        HIP_TRY(grt::launch_gbuffer_shade_sub(dc->d_scene, sv, S.arr.steps(), (const uint32_t*)S.sub_block.p,
                                              P.held_px + base, B.chunk_pix, d_cnt + 2, base, spa, so, st));
      HIP_TRY(grt::launch_average(P.held_px + base, P.held_px + base, B.chunk_pix, d_cnt + 2, base, spa, B.x64, B.status,
                                  b.x64, fails, st));
    }
    return 0;
  };
  auto finish_pass = [&]() -> int {
    HIP_TRY(hipEventRecord(dc->ev1, st));
    HIP_TRY(hipEventSynchronize(dc->ev1));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, dc->ev0, dc->ev1));
    shade_ms += t;
    if (supersampled) HIP_TRY(hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    return stream_done(*dc, st);
  };
  if ((rc = stream_order(*dc, st))) return rc;
  if (supersampled) HIP_TRY(hipMemsetAsync(d_cnt, 0, 32, st));
  HIP_TRY(hipEventRecord(dc->ev0, st));
  if (retarded)
    HIP_TRY(grt::launch_gbuffer_shade_at_retarded(dc->d_scene, gb->view(), time, (const double*)gb->lapse.p,
                                                  b.outputs(), st));
  else if (mode == SECTION_AT) HIP_TRY(grt::launch_gbuffer_shade_at(dc->d_scene, gb->view(), time, b.outputs(), st));
  else HIP_TRY(grt::launch_gbuffer_shade(dc->d_scene, gb->view(), b.outputs(), st));
  if (supersampled) {
    if ((rc = P.enqueue_select(st, b.x64, b.cls, adaptive_params(cfg, w, h, cfg->minimum_luminance), d_cnt))) return rc;
    if (mask_xyza) HIP_TRY(grt::launch_paint(P.sel, n, d_cnt, mask_xyza, b.x64, st));
    else if ((rc = enqueue_sub_pass())) return rc;
  }
  if ((rc = finish_pass())) return rc;
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double trace_ms[2] = {0.0, 0.0};
  const uint64_t n_held = cnt[2], n_missing = sub_pass ? cnt[3] : 0;
  if (report) {
    report->n_selected = cnt[0];
    report->n_held = n_held;
    report->shade_ms = shade_ms;
  }
  if (n_missing) {
    if (!tracer) {
      if (report) report->n_missing = n_missing;
      return fail(-ENODATA, "g-buffer: the sub-sample set misses " + std::to_string(n_missing) + " of the " +
                                std::to_string(cnt[0]) + " selected pixels and the call has no tracer");
    }
    // top-up: trace the missing pixels once, append them, then the sub-ray pass again over
    // the whole selection, which the set now holds
    std::vector<uint32_t> px(n_missing);
    HIP_TRY(hipMemcpy(px.data(), P.missing_px, 4 * n_missing, hipMemcpyDeviceToHost));
    lk.unlock();  // the tracer may be this scene: sub_fill takes its device's lock
    rc = sub_fill(tracer, gb, spa, px, acc, trace_ms, retarded);
    lk.lock();
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    if ((rc = stream_order(*dc, st))) return rc;
    HIP_TRY(hipEventRecord(dc->ev0, st));
    if ((rc = enqueue_sub_pass()) || (rc = finish_pass())) return rc;
    if (cnt[3] != 0) return fail(-EIO, "g-buffer: the top-up left selected pixels without sub-rays");
    if (report) {
      report->n_traced = n_missing;
      report->shade_ms = shade_ms;
      report->trace_ms = trace_ms[0] + trace_ms[1];
      stats_from(acc, (float)trace_ms[0], &report->top_up);
    }
  }
  HIP_TRY(hipMemcpy(xyza_out, b.x64, n * 32, hipMemcpyDeviceToHost));
  if (class_out) HIP_TRY(hipMemcpy(class_out, b.cls, n, hipMemcpyDeviceToHost));
  if (status_out) HIP_TRY(hipMemcpy(status_out, b.status, n, hipMemcpyDeviceToHost));
  if (supersampled) {
    if (n_supersampled) *n_supersampled = cnt[0];
    if ((rc = P.fails[0].read(cnt[1], spa, sub_pass ? failures : nullptr))) return rc;
  }
  return 0;
}

extern "C" {

int grt_gbuffer_shade_section(grt_scene* s, grt_gbuffer* gb, const grt_adaptive_config* cfg, const double* mask_xyza,
                              grt_scene* tracer, double* xyza_out, uint8_t* class_out, uint8_t* status_out,
                              uint64_t* n_supersampled, grt_subsample_failures* failures,
                              grt_gbuffer_section_report* report) {
  return shade_section_impl(s, gb, cfg, mask_xyza, tracer, xyza_out, class_out, status_out, n_supersampled, failures,
                            report, SECTION_STATIC, 0.0);
}

int grt_gbuffer_shade_section_at(grt_scene* s, grt_gbuffer* gb, const grt_adaptive_config* cfg, const double* mask_xyza,
                                 grt_scene* tracer, double* xyza_out, uint8_t* class_out, uint8_t* status_out,
                                 uint64_t* n_supersampled, grt_subsample_failures* failures,
                                 grt_gbuffer_section_report* report, double time) {
  return shade_section_impl(s, gb, cfg, mask_xyza, tracer, xyza_out, class_out, status_out, n_supersampled, failures,
                            report, SECTION_AT, time);
}

int grt_gbuffer_shade_section_at_retarded(grt_scene* s, grt_gbuffer* gb, const grt_adaptive_config* cfg,
                                          const double* mask_xyza, grt_scene* tracer, double* xyza_out,
                                          uint8_t* class_out, uint8_t* status_out, uint64_t* n_supersampled,
                                          grt_subsample_failures* failures, grt_gbuffer_section_report* report,
                                          double time) {
  return shade_section_impl(s, gb, cfg, mask_xyza, tracer, xyza_out, class_out, status_out, n_supersampled, failures,
                            report, SECTION_AT_RETARDED, time);
}

// grt_gbuffer_shade_times, and with `retarded` grt_gbuffer_shade_times_retarded.
static int shade_times_impl(grt_scene* s, const grt_gbuffer* gb, uint32_t n_times, const double* times,
                            const grt_frame_out* out, float* kernel_ms, bool retarded) {
  if (!s || !gb || !times || !out) return fail(-EINVAL, "null argument");
  if (n_times == 0) return fail(-EINVAL, "grt_gbuffer_shade_times needs at least one time");
  for (uint32_t k = 0; k < n_times; ++k)
    if (!std::isfinite(times[k])) return fail(-EINVAL, "times[" + std::to_string(k) + "] is not finite");
  if (!out->xyza && !out->xyza64) return fail(-EINVAL, "grt_frame_out needs xyza or xyza64");
  int rc = grt_gbuffer_shape_compatible(&gb->info.shape, &s->desc);
  if (rc) return rc;
  if (retarded && !gb->has_lapse)
    return fail(-ENODATA, "the g-buffer holds no lapse (grt_gbuffer_trace_lapse, grt_gbuffer_lapse_upload)");
  const int device = gb->info.device;
  const uint64_t per = gb->info.n_pixels;
  if (per == 0 || per > (uint64_t)INT_MAX) return fail(-EINVAL, "frames of 0 or more than INT_MAX pixels");
  const uint64_t g = frames_per_group(per, n_times);  // whole frames, at least one (grt_set_sequence_group)
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  const uint64_t ng = per * g;  // slots of a full group
  DevBuf xyza, cls, status, x64, stop, steps, d_times;
  if ((rc = xyza.alloc(16 * ng)) || (rc = cls.alloc(ng)) || (rc = status.alloc(ng))) return rc;
  if (out->xyza64 && (rc = x64.alloc(32 * ng))) return rc;
  if (out->stop && (rc = stop.alloc(ng))) return rc;
  if (out->steps && (rc = steps.alloc(4 * ng))) return rc;
  if ((rc = d_times.alloc(8 * (uint64_t)n_times))) return rc;
  HIP_TRY(hipMemcpy(d_times.p, times, 8 * (uint64_t)n_times, hipMemcpyHostToDevice));
  if (!gb->omega.p && (rc = gb->omega.alloc(8 * gb->info.n_layers))) return rc;  // a buffer's layers never change
  const grt::Outputs o{(float*)xyza.p,     (uint8_t*)cls.p,  (uint8_t*)status.p, (double*)x64.p,
                       (uint32_t*)steps.p, (uint8_t*)stop.p, nullptr};
  hipStream_t st = nullptr;
  float total_ms = 0;
  for (uint32_t f0 = 0; f0 < n_times; f0 += (uint32_t)g) {
    const uint32_t kg = (uint32_t)std::min<uint64_t>(g, n_times - f0);
    const uint64_t n = per * kg, at = per * f0;
    HIP_TRY(hipEventRecord(dc->ev0, st));
    if (f0 == 0)  // the layers' rates, once per call, in the first group's event time
      HIP_TRY(grt::launch_gbuffer_orbit_rate(dc->d_scene, gb->view(), gb->info.n_layers, (double*)gb->omega.p, st));
    HIP_TRY(grt::launch_gbuffer_shade_times(dc->d_scene, gb->view(), gb->arr.steps(), (const double*)d_times.p + f0, kg,
                                            (const double*)gb->omega.p, retarded ? (const double*)gb->lapse.p : nullptr,
                                            retarded, o, st));
    HIP_TRY(hipEventRecord(dc->ev1, st));
    HIP_TRY(hipEventSynchronize(dc->ev1));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, dc->ev0, dc->ev1));
    total_ms += t;
    if (out->xyza) HIP_TRY(hipMemcpy(out->xyza + 4 * at, xyza.p, 16 * n, hipMemcpyDeviceToHost));
    if (out->xyza64) HIP_TRY(hipMemcpy(out->xyza64 + 4 * at, x64.p, 32 * n, hipMemcpyDeviceToHost));
    if (out->ray_class) HIP_TRY(hipMemcpy(out->ray_class + at, cls.p, n, hipMemcpyDeviceToHost));
    if (out->status) HIP_TRY(hipMemcpy(out->status + at, status.p, n, hipMemcpyDeviceToHost));
    if (out->stop) HIP_TRY(hipMemcpy(out->stop + at, stop.p, n, hipMemcpyDeviceToHost));
    if (out->steps) HIP_TRY(hipMemcpy(out->steps + at, steps.p, 4 * n, hipMemcpyDeviceToHost));
  }
  if (kernel_ms) *kernel_ms = total_ms;
  return 0;
}

int grt_gbuffer_shade_times(grt_scene* s, const grt_gbuffer* gb, uint32_t n_times, const double* times,
                            const grt_frame_out* out, float* kernel_ms) {
  return shade_times_impl(s, gb, n_times, times, out, kernel_ms, false);
}

int grt_gbuffer_shade_times_retarded(grt_scene* s, const grt_gbuffer* gb, uint32_t n_times, const double* times,
                                     const grt_frame_out* out, float* kernel_ms) {
  return shade_times_impl(s, gb, n_times, times, out, kernel_ms, true);
}

int grt_gbuffer_supersample_sequence(grt_scene* tracer, uint32_t n, grt_gbuffer* const* buffers, uint32_t spa,
                                     const uint64_t* n_pixels, const uint32_t* const* pixels, grt_stats* stats,
                                     grt_gbuffer_sequence_report* report) {
  const auto wall0 = std::chrono::steady_clock::now();
  if (!tracer || !buffers || !n_pixels || !pixels) return fail(-EINVAL, "null argument");
  int rc;
  if ((rc = check_sequence_buffers(n, buffers, true, spa, tracer))) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (report) std::memset(report, 0, sizeof(*report));
  std::vector<std::vector<uint32_t>> px(n);
  for (uint32_t f = 0; f < n; ++f) {
    if (n_pixels[f] && !pixels[f]) return fail(-EINVAL, "frame " + std::to_string(f) + ": null pixel list");
    if ((rc = missing_of("frame " + std::to_string(f) + ": ", buffers[f], n_pixels[f], pixels[f], &px[f]))) return rc;
  }
  SubSeqTimes T;
  rc = sub_fill_sequence(tracer, n, buffers, spa, px, &T);
  if (stats) stats_from(T.acc, T.trace_ms, stats);
  if (report) {
    report->n_frames = n;
    report->n_launches = T.chunks;
    report->n_traces = T.traces;
    report->trace_ms = T.trace_ms;
    report->fill_ms = T.fill_ms;
    report->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  }
  return rc;
}

int grt_gbuffer_shade_section_sequence(grt_scene* s, uint32_t n, grt_gbuffer* const* buffers,
                                       const grt_adaptive_config* cfg, const double* mask_xyza, grt_scene* tracer,
                                       const grt_frame_out* out, uint64_t* n_supersampled,
                                       grt_subsample_failures* failures, uint64_t* per_frame,
                                       grt_gbuffer_section_sequence_report* report) {
  const auto wall0 = std::chrono::steady_clock::now();
  if (!s || !buffers || !cfg || !out) return fail(-EINVAL, "null argument");
  if (!out->xyza64) return fail(-EINVAL, "grt_frame_out needs xyza64");
  if (cfg->samples_per_axis == 0) return fail(-EINVAL, "adaptive_sampling.samples_per_axis must be greater than zero");
  const bool supersampled = cfg->enabled || mask_xyza != nullptr;
  const bool sub_pass = supersampled && !mask_xyza;
  const uint32_t spa = cfg->samples_per_axis;
  int rc;
  if ((rc = check_sequence_buffers(n, buffers, sub_pass, spa, sub_pass ? tracer : nullptr))) return rc;
  for (uint32_t f = 0; f < n; ++f)
    if ((rc = grt_gbuffer_shape_compatible(&buffers[f]->info.shape, &s->desc)))
      return fail(rc, "frame " + std::to_string(f) + ": " + grt_last_error());
  if (report) std::memset(report, 0, sizeof(*report));
  for (uint32_t f = 0; f < n; ++f) {
    if (n_supersampled) n_supersampled[f] = 0;
    if (failures) failures[f].count = 0;
  }
  if (per_frame) std::memset(per_frame, 0, 32ull * n);
  const grt_gbuffer_info& i0 = buffers[0]->info;
  const int device = i0.device;
  const uint32_t rows = i0.rows, cols = i0.cols;
  const uint64_t per = i0.n_pixels;
  if (per > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "frame larger than INT_MAX pixels");
  // frames per launch group: whole buffers within the group's rays, at least one; the
  // split compacts the group's slots with 32-bit counts
  const uint64_t g = frames_per_group(per, n, INT_MAX);
  const uint32_t n_groups = (uint32_t)((n + g - 1) / g);
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::unique_lock<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  if (sub_pass)
    for (uint32_t f = 0; f < n; ++f)
      if ((rc = buffers[f]->sub.ensure_map(per))) return rc;
  const grt::AdaptiveParams ap = adaptive_params(cfg, cols, rows, cfg->minimum_luminance);
  hipStream_t st = nullptr;
  double shade_ms = 0.0;
  // One launch group, everything on `st`: the stacked 1-spp shade; per frame the floor, the
  // selection and its compaction on the frame's slice (the mask: the paint); then, over all
  // the group's selections, the split, and with `chunks` the sub-ray shade, the average and
  // the failure records per chunk.  cnt: per frame selected, failed, held, missing; then the
  // totals held, missing.
  auto run_group = [&](AdaptivePlan& P, uint32_t f0, uint32_t kg, bool chunks,
                       std::vector<unsigned long long>& cnt) -> int {
    P.n = per;
    P.w = cols;
    P.h = rows;
    P.frames = kg;
    P.spa = spa;
    P.held = P.stack = true;
    P.supersampled = supersampled;
    P.device_floor = supersampled && !cfg->has_minimum_luminance;
    P.sub_rays = sub_pass;
    P.sec_stop = out->stop != nullptr;
    P.sec_steps = out->steps != nullptr;
    if (int rc = P.plan(*dc, sub_pass && failures ? failures + f0 : nullptr)) return rc;
    const SectionBufs& b = P.sec;
    const SuperBufs& B = P.B;
    std::vector<grt::GBufferFrame> frames(kg);
    std::vector<grt::GBufferSubFrame> subs(kg);
    std::vector<grt::SubsampleFailures> lists(kg);
    for (uint32_t f = 0; f < kg; ++f) {
      const grt_gbuffer* gb = buffers[f0 + f];
      const GBufferSub& S = gb->sub;
      frames[f] = grt::GBufferFrame{gb->view(), gb->arr.steps()};
      subs[f] = grt::GBufferSubFrame{S.view(), S.arr.steps(), (const uint32_t*)S.sub_block.p};
      if (!supersampled) continue;
      lists[f] = P.fails[f].f;
      lists[f].count = P.d_cnt + 4 * f + 1;
      lists[f].ray_stop = B.stop;
      lists[f].ray_steps = B.steps;
    }
    HIP_TRY(hipMemcpy(P.frame_tab, frames.data(), kg * sizeof(frames[0]), hipMemcpyHostToDevice));
    if (sub_pass) {
      HIP_TRY(hipMemcpy(P.sub_tab, subs.data(), kg * sizeof(subs[0]), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(P.fail_tab, lists.data(), kg * sizeof(lists[0]), hipMemcpyHostToDevice));
    }
    if (int rc = stream_order(*dc, st)) return rc;
    if (supersampled) HIP_TRY(hipMemsetAsync(P.d_cnt, 0, P.cnt_bytes(), st));
    HIP_TRY(hipEventRecord(dc->ev0, st));
    HIP_TRY(grt::launch_gbuffer_shade_stack(dc->d_scene, P.frame_tab, kg, per, b.outputs(), st));
    for (uint32_t f = 0; f < kg && supersampled; ++f) {  // the frame's slice, its own counts
      double* x64 = b.x64 + 4 * per * f;
      unsigned long long* c = P.d_cnt + 4 * f;
      uint32_t* sel = sub_pass ? P.sel + per * f : P.sel;
      if (int rc = P.enqueue_select(st, x64, b.cls + per * f, ap, c, nullptr, nullptr, 0, sel)) return rc;
      if (mask_xyza) HIP_TRY(grt::launch_paint(sel, per, c, mask_xyza, x64, st));
    }
    if (sub_pass) {
      unsigned long long* tot = P.d_totals();
      HIP_TRY(grt::gbuffer_split_stack(P.sel, P.d_cnt, kg, per, P.sub_tab, P.split, P.stack_px, P.held_px, tot,
                                       P.missing_px, tot + 1, P.split_tmp, &P.split_bytes, st));
      const grt::Outputs so{B.xyza, B.cls, B.status, B.x64, B.steps, B.stop, nullptr};
      const grt::SubsampleFailures none{};  // the records are failures_stack_kernel's
      for (uint32_t c = 0; c < B.n_chunks && chunks; ++c) {
        const uint64_t base = (uint64_t)c * B.chunk_pix;
        const uint32_t* px = P.held_px + base;
        HIP_TRY(grt::launch_gbuffer_shade_sub_stack(dc->d_scene, P.sub_tab, kg, per, px, B.chunk_pix, tot, base, spa, so,
                                                    st));
        HIP_TRY(grt::launch_average(px, px, B.chunk_pix, tot, base, spa, B.x64, B.status, b.x64, none, st));
        HIP_TRY(grt::launch_failures_stack(px, B.chunk_pix, tot, base, spa, per, kg, B.status, P.fail_tab, st));
      }
    }
    HIP_TRY(hipEventRecord(dc->ev1, st));
    HIP_TRY(hipEventSynchronize(dc->ev1));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, dc->ev0, dc->ev1));
    shade_ms += t;
    cnt.assign(4 * (size_t)kg + 4, 0);
    if (supersampled) HIP_TRY(hipMemcpy(cnt.data(), P.d_cnt, P.cnt_bytes(), hipMemcpyDeviceToHost));
    return stream_done(*dc, st);
  };
  // the group's frames, counts and failure lists to the caller's arrays
  auto finish_group = [&](const AdaptivePlan& P, uint32_t f0, uint32_t kg,
                          const std::vector<unsigned long long>& cnt) -> int {
    const SectionBufs& b = P.sec;
    const uint64_t m = per * kg, at = per * f0;
    HIP_TRY(hipMemcpy(out->xyza64 + 4 * at, b.x64, 32 * m, hipMemcpyDeviceToHost));
    if (out->ray_class) HIP_TRY(hipMemcpy(out->ray_class + at, b.cls, m, hipMemcpyDeviceToHost));
    if (out->status) HIP_TRY(hipMemcpy(out->status + at, b.status, m, hipMemcpyDeviceToHost));
    if (out->stop) HIP_TRY(hipMemcpy(out->stop + at, b.stop, m, hipMemcpyDeviceToHost));
    if (out->steps) HIP_TRY(hipMemcpy(out->steps + at, b.steps, 4 * m, hipMemcpyDeviceToHost));
    for (uint32_t f = 0; f < kg && supersampled; ++f) {
      if (n_supersampled) n_supersampled[f0 + f] = cnt[4 * f];
      if (int rc = P.fails[f].read(cnt[4 * f + 1], spa, sub_pass && failures ? &failures[f0 + f] : nullptr)) return rc;
    }
    return 0;
  };
  // per frame: selected, held when the call began, missing then
  std::vector<uint64_t> first(3ull * n, 0);
  std::vector<std::vector<uint32_t>> missing(n);
  std::vector<uint8_t> dirty(n_groups, 0);
  uint64_t n_missing = 0;
  std::vector<unsigned long long> cnt;
  // without a tracer a later group may still refuse the call: count first, write nothing
  const bool count_first = sub_pass && !tracer && n_groups > 1;
  for (int pass = count_first ? 0 : 1; pass < 2; ++pass) {
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
      const uint32_t f0 = (uint32_t)(gi * g), kg = (uint32_t)std::min<uint64_t>(g, n - f0);
      AdaptivePlan P;
      if ((rc = run_group(P, f0, kg, pass == 1, cnt))) return rc;
      if (pass == 1 && count_first) {  // nothing is missing: the counts stand
        if ((rc = finish_group(P, f0, kg, cnt))) return rc;
        continue;
      }
      for (uint32_t f = 0; f < kg; ++f) {
        first[3 * (f0 + f)] = cnt[4 * f];
        first[3 * (f0 + f) + 1] = cnt[4 * f + 2];
        first[3 * (f0 + f) + 2] = cnt[4 * f + 3];
      }
      const uint64_t gm = sub_pass ? cnt[4 * kg + 1] : 0;
      if (gm) {
        dirty[gi] = 1;
        n_missing += gm;
        std::vector<uint32_t> px(gm);
        HIP_TRY(hipMemcpy(px.data(), P.missing_px, 4 * gm, hipMemcpyDeviceToHost));
        for (uint32_t p : px) missing[f0 + p / per].push_back((uint32_t)(p % per));
      } else if (pass == 1 && (rc = finish_group(P, f0, kg, cnt))) {
        return rc;
      }
    }
    if (pass == 0 && n_missing) break;
  }
  uint64_t n_selected = 0, n_held = 0;
  for (uint32_t f = 0; f < n; ++f) {
    n_selected += first[3 * f];
    n_held += first[3 * f + 1];
    if (per_frame) {
      per_frame[4 * f] = first[3 * f];
      per_frame[4 * f + 1] = first[3 * f + 1];
      per_frame[4 * f + 3] = first[3 * f + 2];
    }
  }
  auto fill_report = [&](uint64_t traced, uint64_t still_missing, const SubSeqTimes* T) {
    if (!report) return;
    report->n_frames = n;
    report->n_launches = n_groups;
    report->n_selected = n_selected;
    report->n_held = n_held;
    report->n_traced = traced;
    report->n_missing = still_missing;
    report->shade_ms = shade_ms;
    if (T) {
      report->trace_ms = T->trace_ms + T->fill_ms;
      stats_from(T->acc, T->trace_ms, &report->top_up);
    }
    report->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  };
  if (n_missing == 0) {
    fill_report(0, 0, nullptr);
    return 0;
  }
  if (!tracer) {
    fill_report(0, n_missing, nullptr);
    return fail(-ENODATA, "g-buffer: the sub-sample sets miss " + std::to_string(n_missing) + " of the " +
                              std::to_string(n_selected) + " selected pixels of the " + std::to_string(n) +
                              " frames and the call has no tracer");
  }
  // one stacked top-up of every frame's missing pixels, then the groups that missed some again
  SubSeqTimes T;
  lk.unlock();  // the tracer may be this scene: sub_fill_sequence takes its device's lock
  rc = sub_fill_sequence(tracer, n, buffers, spa, missing, &T);
  lk.lock();
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  for (uint32_t gi = 0; gi < n_groups; ++gi) {
    if (!dirty[gi]) continue;
    const uint32_t f0 = (uint32_t)(gi * g), kg = (uint32_t)std::min<uint64_t>(g, n - f0);
    AdaptivePlan P;
    if ((rc = run_group(P, f0, kg, true, cnt))) return rc;
    if (cnt[4 * kg + 1] != 0) return fail(-EIO, "g-buffer: the top-up left selected pixels without sub-rays");
    if ((rc = finish_group(P, f0, kg, cnt))) return rc;
  }
  if (per_frame)
    for (uint32_t f = 0; f < n; ++f) {
      per_frame[4 * f + 2] = first[3 * f + 2];
      per_frame[4 * f + 3] = 0;
    }
  fill_report(n_missing, 0, &T);
  return 0;
}

int grt_gbuffer_sub_info_get(const grt_gbuffer* gb, grt_gbuffer_sub_info* out) {
  if (!gb || !out) return fail(-EINVAL, "null argument");
  std::memset(out, 0, sizeof(*out));
  out->samples_per_axis = gb->sub.spa;
  out->n_sub_pixels = gb->sub.n_pix;
  out->n_sub_rays = gb->sub.n_rays();
  out->n_sub_layers = gb->sub.n_layers;
  return 0;
}

int grt_gbuffer_sub_download(const grt_gbuffer* gb, uint32_t* sub_pixel, const grt_gbuffer_arrays* h) {
  if (!gb) return fail(-EINVAL, "null argument");
  const GBufferSub& S = gb->sub;
  const uint64_t m = S.n_pix, n = S.n_rays(), l = S.n_layers;
  if (S.spa == 0 || m == 0) return 0;  // nothing to copy
  if (!sub_pixel || !h || GBufferPtrs(*h).missing(false)) return fail(-EINVAL, "null argument");
  if (l && GBufferPtrs(*h).missing(true)) return fail(-EINVAL, "null layer array");
  HIP_TRY(hipSetDevice(gb->info.device));
  HIP_TRY(hipMemcpy(sub_pixel, S.sub_pixel.p, 4 * m, hipMemcpyDeviceToHost));
  return S.arr.copy(*h, n, l, hipMemcpyDeviceToHost);
}

int grt_gbuffer_sub_upload(grt_gbuffer* gb, const grt_gbuffer_sub_info* sub, const uint32_t* sub_pixel,
                           const grt_gbuffer_arrays* h) {
  if (!gb || !sub) return fail(-EINVAL, "null argument");
  static const grt_gbuffer_arrays none{};
  // the shade kernel indexes by sub_pixel, layer_start and object: hold them to their ranges
  int rc = grt_host::gbuffer_sub_check(&gb->info, sub, sub_pixel, sub->samples_per_axis ? h : &none);
  if (rc) return rc;
  if (sub->samples_per_axis && !h) return fail(-EINVAL, "g-buffer: null sub-ray array");
  HIP_TRY(hipSetDevice(gb->info.device));
  std::unique_ptr<GBufferSub> N(new GBufferSub());
  if ((rc = N->ensure_map(gb->info.n_pixels))) return rc;
  N->spa = sub->samples_per_axis;
  const uint64_t m = sub->n_sub_pixels, n = sub->n_sub_rays, l = sub->n_sub_layers;
  if (N->spa && m) {
    if ((rc = N->reserve_pixels(m)) || (rc = N->reserve_layers(l))) return rc;
    HIP_TRY(hipMemcpy(N->sub_pixel.p, sub_pixel, 4 * m, hipMemcpyHostToDevice));
    if ((rc = N->arr.copy(*h, n, l, hipMemcpyHostToDevice))) return rc;
    N->n_pix = m;
    N->n_layers = l;
    HIP_TRY(grt::gbuffer_sub_index((const uint32_t*)N->sub_pixel.p, m, gb->info.n_pixels, (uint32_t*)N->sub_block.p,
                                   nullptr));
    HIP_TRY(hipDeviceSynchronize());
    for (uint64_t j = 0; j < m; ++j) N->h_block[sub_pixel[j]] = (uint32_t)j;
  }
  std::swap(gb->sub, *N);  // the old set's arrays are freed with N
  return 0;
}

int grt_gbuffer_sub_has_lapse(const grt_gbuffer* gb) {
  if (!gb) return fail(-EINVAL, "null argument");
  return gb->sub.spa && gb->sub.timed ? 1 : 0;
}

int grt_gbuffer_sub_clear(grt_gbuffer* gb) {
  if (!gb) return fail(-EINVAL, "null argument");
  HIP_TRY(hipSetDevice(gb->info.device));
  GBufferSub none;
  std::swap(gb->sub, none);  // the set's arrays, map and lapse are freed with `none`
  return 0;
}

int grt_gbuffer_sub_lapse_download(const grt_gbuffer* gb, double* out) {
  if (!gb) return fail(-EINVAL, "null argument");
  const GBufferSub& S = gb->sub;
  if (S.spa == 0 || !S.timed)
    return fail(-ENODATA, "the g-buffer's sub-sample set holds no lapse (grt_gbuffer_supersample_lapse, "
                          "grt_gbuffer_sub_lapse_upload)");
  if (S.n_layers == 0) return 0;
  if (!out) return fail(-EINVAL, "null argument");
  HIP_TRY(hipSetDevice(gb->info.device));
  HIP_TRY(hipMemcpy(out, S.lapse.p, 8 * S.n_layers, hipMemcpyDeviceToHost));
  return 0;
}

int grt_gbuffer_sub_lapse_upload(grt_gbuffer* gb, const double* lapse, uint64_t n) {
  if (!gb || (!lapse && n)) return fail(-EINVAL, "null argument");
  GBufferSub& S = gb->sub;
  if (S.spa == 0) return fail(-EINVAL, "g-buffer: a lapse for a sub-sample set, but the buffer holds no set");
  if (n != S.n_layers)
    return fail(-EINVAL, "a lapse of " + std::to_string(n) + " entries for a sub-sample set of " +
                             std::to_string(S.n_layers) + " layers");
  for (uint64_t k = 0; k < n; ++k)
    if (!std::isfinite(lapse[k])) return fail(-EINVAL, "lapse[" + std::to_string(k) + "] is not finite");
  HIP_TRY(hipSetDevice(gb->info.device));
  DevBuf fresh;  // as large as the layer arrays: a later fill grows it with them
  if (int rc = fresh.alloc(8 * std::max(S.cap_layers, n))) return rc;
  if (n) HIP_TRY(hipMemcpy(fresh.p, lapse, 8 * n, hipMemcpyHostToDevice));
  S.lapse = std::move(fresh);  // what the set held is freed
  S.timed = true;
  return 0;
}

int grt_gbuffer_destroy(grt_gbuffer* gb) {
  if (!gb) return 0;
  (void)hipSetDevice(gb->info.device);
  delete gb;
  return 0;
}

}  // extern "C"
