// api_adaptive.hip — the adaptive pass of the C ABI (include/grt_api.h): the supersampled
// section, camera sequences, the supersample pass of a row-band shard and the luminance
// floor.  The pass's plan and pipeline (AdaptivePlan) are in api_internal.h, which the
// geometry buffer's re-shade (api_gbuffer.hip) runs too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cerrno>
#include <climits>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "grt_api.h"
#include "../host/host_internal.h"
#include "dev_scene.h"
#include "kernels.h"
#include "api_internal.h"

using namespace grt_api;

GRT_API_NAMESPACE {

// ------------------------------------------------------------- adaptive pass ----
int ad_reserve(DeviceCopy& dc, uint64_t bytes) {
  if (bytes <= dc.ad_bytes && dc.ad_mem) return 0;
  if (dc.ad_mem) {
    (void)hipDeviceSynchronize();  // earlier async launches may still use the old arena
    (void)hipFree(dc.ad_mem);
    dc.ad_mem = nullptr;
    dc.ad_bytes = 0;
  }
  const uint64_t cap = bytes + (bytes >> 3);
  if (hipMalloc(&dc.ad_mem, cap) != hipSuccess) {
    (void)hipGetLastError();
    dc.ad_mem = nullptr;
    return fail(-ENOMEM, "cannot allocate the adaptive-pass scratch");
  }
  dc.ad_bytes = cap;
  return 0;
}

std::atomic<uint64_t> g_sub_chunk{SUB_CHUNK};  // grt_set_sub_chunk (tests force several chunks)
constexpr uint64_t SEQ_GROUP = 1ull << 22;     // rays per launch group of a camera sequence
std::atomic<uint64_t> g_seq_group{SEQ_GROUP};  // grt_set_sequence_group

uint64_t frames_per_group(uint64_t per, uint64_t n, uint64_t max_slots, uint64_t rows) {
  uint64_t g = std::max<uint64_t>(1, g_seq_group.load(std::memory_order_relaxed) / per);
  g = std::min<uint64_t>(g, n);
  if (max_slots) g = std::min<uint64_t>(g, std::max<uint64_t>(1, max_slots / per));
  if (rows) g = std::min<uint64_t>(g, std::max<uint64_t>(1, 0xffffffffull / rows));
  return g;
}

// supersample (raytracer.rs:320-384) over a selection that lives on the device: entries
// j < *d_count <= n_max of sel_px (pixel index in the rect row0/col0/rows/cols: camera
// ray and jitter hash) and sel_out (index into d_out64).  The sub-rays go through the
// trace in chunks of g_sub_chunk; the integrate / shade kernels read each chunk's live
// count from the device, so nothing waits for the host between the passes.
int enqueue_supersample(grt_scene* s, DeviceCopy& dc, hipStream_t st, const SuperBufs& B, uint32_t row0,
                        uint32_t col0, uint32_t rows, uint32_t cols, const uint32_t* sel_px, const uint32_t* sel_out,
                        const unsigned long long* d_count, uint32_t spa, double* d_out64, unsigned long long* d_stats,
                        const grt::SubsampleFailures& fails_in, const grt::CamTable* ct, uint32_t stack_row0) {
  grt::SubsampleFailures fails = fails_in;
  fails.ray_stop = B.stop;
  fails.ray_steps = B.steps;
  HIP_TRY(grt::launch_chunk_live(d_count, B.n_chunks, B.chunk_pix, B.per, B.live, st));
  for (uint32_t c = 0; c < B.n_chunks; ++c) {
    const uint64_t base = (uint64_t)c * B.chunk_pix;
    HIP_TRY(grt::launch_make_offsets(sel_px + base, B.chunk_pix, d_count, base, spa, row0, col0, cols, B.pix, B.dx,
                                     B.dy, st));
    // a camera sequence: the rect is a frame of the stack, stack_row0 its first stacked row
    // (the jitter above hashes the frame's own pixel coordinates, as a frame alone does)
    grt::WorkList wo = offsets_worklist(row0 + stack_row0, col0, rows, cols, B.cap, B.pix, B.dx, B.dy);
    wo.n_live = B.live + c;
    grt::Outputs so{B.xyza, B.cls, B.status, B.x64, B.steps, B.stop};
    int rc = enqueue_trace(s, dc, wo, so, d_stats, st, ct);
    if (rc) return rc;
    HIP_TRY(grt::launch_average(sel_out + base, sel_px + base, B.chunk_pix, d_count, base, spa, B.x64, B.status,
                                d_out64, fails, st));
  }
  return 0;
}

// resolve_minimum_luminance's relative floor (raytracer.rs:118-129): 1e-3 x the element
// at ((n - 1) * 0.99) as usize in f64::total_cmp order (select_nth_unstable_by selects
// the same element as nth_element under the same total order).  Reorders `lum`.
static double relative_min_luminance(std::vector<double>& lum) {
  if (lum.empty()) return 0.0;
  uint64_t index = (uint64_t)((double)(lum.size() - 1) * 0.99);
  auto key = [](double v) {
    int64_t b;
    std::memcpy(&b, &v, 8);
    return b ^ (int64_t)((uint64_t)(b >> 63) >> 1);
  };
  std::nth_element(lum.begin(), lum.begin() + index, lum.end(), [&](double a, double b) { return key(a) < key(b); });
  return 1e-3 * lum[index];
}

}  // namespace grt_api

extern "C" {

int grt_adaptive_min_luminance_device(int device, void* stream, const double* d_y, uint32_t stride, uint64_t n,
                                      const grt_adaptive_config* cfg, double* out) {
  if (!out || (n && (!d_y || stride == 0))) return fail(-EINVAL, "null argument");
  if (cfg && cfg->has_minimum_luminance) {
    *out = cfg->minimum_luminance;
    return 0;
  }
  if (n == 0) {
    *out = 0.0;
    return 0;
  }
  if (n > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "more than INT_MAX luminances");
  HIP_TRY(hipSetDevice(device));
  size_t bytes = 0;
  HIP_TRY(grt::luminance_order_stat(d_y, stride, n, floor_index(n), nullptr, &bytes, nullptr, (hipStream_t)stream));
  DevBuf b;
  int rc = b.alloc(bytes);
  if (rc) return rc;
  double v = 0.0;
  HIP_TRY(grt::luminance_order_stat(d_y, stride, n, floor_index(n), b.p, &bytes, &v, (hipStream_t)stream));
  *out = 1e-3 * v;
  return 0;
}

double grt_adaptive_min_luminance(const double* lum, uint64_t n, const grt_adaptive_config* cfg) {
  if (cfg && cfg->has_minimum_luminance) return cfg->minimum_luminance;
  if (!lum || n == 0) return 0.0;
  std::vector<double> v(lum, lum + n);
  return relative_min_luminance(v);
}

}  // extern "C"

GRT_API_NAMESPACE {

// The recorded failed sub-samples, sorted by (pixel, stratum): the reference logs them
// from a parallel loop (raytracer.rs:357-362), in no particular order.
int copy_failures(const grt::SubsampleFailures& f, uint64_t count, uint32_t spa, grt_subsample_failures* out) {
  const uint64_t m = std::min<uint64_t>(count, f.cap);
  if (m == 0) return 0;
  std::vector<uint64_t> key(m);
  std::vector<uint8_t> st(m), sp(f.stop ? m : 0);
  std::vector<uint32_t> ns(f.stop ? m : 0);
  HIP_TRY(hipMemcpy(key.data(), f.key, m * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(st.data(), f.status, m, hipMemcpyDeviceToHost));
  if (f.stop) {
    HIP_TRY(hipMemcpy(sp.data(), f.stop, m, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ns.data(), f.steps, m * 4, hipMemcpyDeviceToHost));
  }
  std::vector<uint64_t> order(m);
  for (uint64_t i = 0; i < m; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return key[a] < key[b]; });
  const uint64_t per = (uint64_t)spa * spa;
  for (uint64_t i = 0; i < m; ++i) {
    out->pixel[i] = (uint32_t)(key[order[i]] / per);
    if (out->sample) out->sample[i] = (uint32_t)(key[order[i]] % per);
    out->status[i] = st[order[i]];
    if (f.stop) {
      out->stop[i] = sp[order[i]];
      if (out->steps) out->steps[i] = ns[order[i]];
    }
  }
  return 0;
}

grt::AdaptiveParams adaptive_params(const grt_adaptive_config* cfg, uint32_t w, uint32_t h, double min_lum) {
  grt::AdaptiveParams ap;
  ap.w = w;
  ap.h = h;
  ap.exclude_background_contrast = cfg->exclude_background_contrast;
  ap._pad = 0;
  ap.min_lum = min_lum;
  ap.luminance_contrast_threshold = cfg->luminance_contrast_threshold;
  ap.opacity_contrast_threshold = cfg->opacity_contrast_threshold;
  return ap;
}

}  // namespace grt_api

extern "C" {

int grt_render_section_ex(grt_scene* s, int device, uint32_t from_row, uint32_t from_col, uint32_t to_row,
                          uint32_t to_col, const grt_adaptive_config* cfg, const double* mask_xyza, double* xyza_out,
                          uint8_t* class_out, uint64_t* n_supersampled, grt_stats* stats, uint8_t* status_out,
                          grt_subsample_failures* failures, uint8_t* stop_out, uint32_t* steps_out) {
  if (!s || !cfg || !xyza_out) return fail(-EINVAL, "null argument");
  if (to_row < from_row || to_col < from_col) return fail(-EINVAL, "empty section");
  if (cfg->samples_per_axis == 0) return fail(-EINVAL, "adaptive_sampling.samples_per_axis must be greater than zero");
  int rc = check_rect(s, from_row, from_col, to_row - from_row, to_col - from_col);
  if (rc) return rc;
  DeviceCopy* dc;
  rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  uint32_t w = to_col - from_col, h = to_row - from_row;
  uint64_t n = (uint64_t)w * h;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n_supersampled) *n_supersampled = 0;
  if (failures) failures->count = 0;
  if (n == 0) return 0;
  const bool supersampled = cfg->enabled || mask_xyza != nullptr;
  if (supersampled && n > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "section larger than INT_MAX pixels");
  AdaptivePlan P;
  P.n = n;
  P.w = w;
  P.h = h;
  P.spa = cfg->samples_per_axis;
  P.supersampled = supersampled;
  P.device_floor = supersampled && !cfg->has_minimum_luminance;
  P.ordered = P.sub_rays = supersampled && !mask_xyza;
  P.sec_stop = stop_out != nullptr;
  P.sec_steps = steps_out || P.ordered;
  if ((rc = P.plan(*dc, failures))) return rc;
  const SectionBufs& b = P.sec;
  const grt::AdaptiveParams ap = adaptive_params(cfg, w, h, cfg->minimum_luminance);
  hipStream_t st = nullptr;
  // the whole pass again, with the pool grown, while a trace of it lost candidates
  for (bool again = true; again;) {
    if ((rc = reset_counters(*dc, st))) return rc;
    if (supersampled) HIP_TRY(hipMemsetAsync(P.d_cnt, 0, 16, st));
    HIP_TRY(hipEventRecord(dc->ev0, st));
    if ((rc = enqueue_trace(s, *dc, rect_worklist(from_row, from_col, h, w), b.outputs(), dc->d_stats, st))) return rc;
    if (supersampled &&
        ((rc = P.enqueue_select(st, b.x64, b.cls, ap, P.d_cnt)) ||
         (rc = P.enqueue_tail(s, *dc, st, from_row, from_col, h, w, P.d_cnt, mask_xyza, b.x64, b.steps, dc->d_stats))))
      return rc;
    HIP_TRY(hipEventRecord(dc->ev1, st));
    HIP_TRY(hipEventSynchronize(dc->ev1));
    if ((rc = pool_check(*dc, &again))) return rc;
  }
  HIP_TRY(hipMemcpy(xyza_out, b.x64, n * 32, hipMemcpyDeviceToHost));
  if (class_out) HIP_TRY(hipMemcpy(class_out, b.cls, n, hipMemcpyDeviceToHost));
  if (status_out) HIP_TRY(hipMemcpy(status_out, b.status, n, hipMemcpyDeviceToHost));
  if (stop_out) HIP_TRY(hipMemcpy(stop_out, b.stop, n, hipMemcpyDeviceToHost));
  if (steps_out) HIP_TRY(hipMemcpy(steps_out, b.steps, n * 4, hipMemcpyDeviceToHost));
  if (supersampled && (rc = P.read(n_supersampled, failures))) return rc;
  if (stats) {  // the counters of the last attempt
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float ms = 0;
    if ((rc = read_counters(*dc, acc))) return rc;
    HIP_TRY(hipEventElapsedTime(&ms, dc->ev0, dc->ev1));
    stats_from(acc, ms, stats);
  }
  return 0;
}

int grt_render_section(grt_scene* s, int device, uint32_t from_row, uint32_t from_col, uint32_t to_row,
                       uint32_t to_col, const grt_adaptive_config* cfg, const double* mask_xyza,
                       double* xyza_out, uint8_t* class_out, uint64_t* n_supersampled, grt_stats* stats,
                       uint8_t* status_out) {
  return grt_render_section_ex(s, device, from_row, from_col, to_row, to_col, cfg, mask_xyza, xyza_out, class_out,
                               n_supersampled, stats, status_out, nullptr, nullptr, nullptr);
}

// ------------------------------------------------------------- camera sequences ----
// K cameras over one resident scene (grt_api.h).  The frames of a launch group are one
// stacked rectangle of kg * rows rows: its 1-spp trace is one work queue through the
// sequence unit (enqueue_trace with the group's camera table), and output slot
// R * cols + c of the stack is pixel (R % rows, c) of frame R / rows, so the stacked
// buffers are the frames back to back.
int grt_set_sequence_group(uint64_t rays) {
  g_seq_group.store(rays ? rays : SEQ_GROUP, std::memory_order_relaxed);
  return 0;
}

namespace {
struct SeqTimes {
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // as trace_sync's
  double trace_ms = 0.0, super_ms = 0.0;
};

// One launch group with supersampling (or the sampling mask): the stacked 1-spp trace,
// then frame by frame the passes of grt_render_section_ex on that frame's slice of the
// stacked buffers -- the luminance floor, the selection stencil (neither sees another
// frame), compaction, work order, and the sub-rays through the sequence unit as an offset
// list whose rows lie in the frame's part of the stack.  The per-frame scratch is reused
// from frame to frame (one stream).  Host outputs: the group's first frame onwards.
int sequence_group_super(grt_scene* s, DeviceCopy& dc, const grt::CamTable& ct, uint32_t rows, uint32_t cols,
                         const grt_adaptive_config* cfg, const double* mask_xyza, const grt_frame_out& out,
                         uint64_t* n_supersampled, grt_subsample_failures* failures, SeqTimes* T) {
  int rc;
  const uint32_t kg = ct.n_cams;
  const uint64_t per = (uint64_t)rows * cols, n = per * kg;
  AdaptivePlan P;
  P.n = per;
  P.w = cols;
  P.h = rows;
  P.frames = kg;
  P.spa = cfg->samples_per_axis;
  P.device_floor = !cfg->has_minimum_luminance;
  P.ordered = P.sub_rays = !mask_xyza;
  P.sec_stop = P.sec_steps = true;
  if ((rc = P.plan(dc, failures))) return rc;
  const SectionBufs& b = P.sec;
  hipStream_t st = nullptr;
  hipEvent_t ev_mid = nullptr;
  HIP_TRY(hipEventCreate(&ev_mid));
  struct EvGuard {
    hipEvent_t e;
    ~EvGuard() { (void)hipEventDestroy(e); }
  } guard{ev_mid};
  const grt::AdaptiveParams ap = adaptive_params(cfg, cols, rows, cfg->minimum_luminance);
  for (bool again = true; again;) {
    if ((rc = reset_counters(dc, st))) return rc;
    HIP_TRY(hipMemsetAsync(P.d_cnt, 0, P.cnt_bytes(), st));
    HIP_TRY(hipEventRecord(dc.ev0, st));
    if ((rc = enqueue_trace(s, dc, rect_worklist(0, 0, kg * rows, cols), b.outputs(), dc.d_stats, st, &ct))) return rc;
    HIP_TRY(hipEventRecord(ev_mid, st));
    for (uint32_t f = 0; f < kg; ++f) {  // the frame's slice of the stacked buffers, its own counts
      double* x64 = b.x64 + 4 * per * f;
      unsigned long long* cnt = P.d_cnt + 2 * f;
      if ((rc = P.enqueue_select(st, x64, b.cls + per * f, ap, cnt)) ||
          (rc = P.enqueue_tail(s, dc, st, 0, 0, rows, cols, cnt, mask_xyza, x64, b.steps + per * f, dc.d_stats, f, &ct)))
        return rc;
    }
    HIP_TRY(hipEventRecord(dc.ev1, st));
    HIP_TRY(hipEventSynchronize(dc.ev1));
    float t0 = 0, t1 = 0;
    HIP_TRY(hipEventElapsedTime(&t0, dc.ev0, ev_mid));
    HIP_TRY(hipEventElapsedTime(&t1, ev_mid, dc.ev1));
    T->trace_ms += t0;
    T->super_ms += t1;
    if ((rc = pool_check(dc, &again))) return rc;
    // as grt_render_section_ex: the counters of the attempt that stands
    if (!again && (rc = read_counters(dc, T->acc))) return rc;
  }
  HIP_TRY(hipMemcpy(out.xyza64, b.x64, n * 32, hipMemcpyDeviceToHost));
  if (out.ray_class) HIP_TRY(hipMemcpy(out.ray_class, b.cls, n, hipMemcpyDeviceToHost));
  if (out.status) HIP_TRY(hipMemcpy(out.status, b.status, n, hipMemcpyDeviceToHost));
  if (out.stop) HIP_TRY(hipMemcpy(out.stop, b.stop, n, hipMemcpyDeviceToHost));
  if (out.steps) HIP_TRY(hipMemcpy(out.steps, b.steps, n * 4, hipMemcpyDeviceToHost));
  return P.read(n_supersampled, failures);
}
}  // namespace

int grt_render_sequence(grt_scene* s, int device, uint32_t n_cameras, const grt_camera_desc* cameras,
                        const grt_adaptive_config* cfg, const double* mask_xyza, const grt_frame_out* out,
                        uint64_t* n_supersampled, grt_stats* stats, grt_subsample_failures* failures,
                        grt_sequence_report* report) {
  const auto wall0 = std::chrono::steady_clock::now();
  if (!s || !cameras || !out) return fail(-EINVAL, "null argument");
  if (n_cameras == 0) return fail(-EINVAL, "a sequence needs at least one camera");
  const int64_t rows64 = s->desc.camera.rows, cols64 = s->desc.camera.cols;
  for (uint32_t f = 0; f < n_cameras; ++f)
    if (cameras[f].rows != rows64 || cameras[f].cols != cols64)
      return fail(-EINVAL, "camera " + std::to_string(f) + " of the sequence has " + std::to_string(cameras[f].rows) +
                               " x " + std::to_string(cameras[f].cols) + " pixels, the scene's frame " +
                               std::to_string(rows64) + " x " + std::to_string(cols64));
  const bool supersampled = (cfg && cfg->enabled) || mask_xyza != nullptr;
  if (supersampled && !cfg) return fail(-EINVAL, "the sampling mask needs the adaptive configuration");
  if (supersampled && !out->xyza64) return fail(-EINVAL, "supersampling needs grt_frame_out.xyza64");
  if (supersampled && cfg->samples_per_axis == 0)
    return fail(-EINVAL, "adaptive_sampling.samples_per_axis must be greater than zero");
  const uint32_t rows = (uint32_t)rows64, cols = (uint32_t)cols64;
  const uint64_t per = (uint64_t)rows * cols;
  if (per > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "frame larger than INT_MAX pixels");
  // frames per launch group: whole frames within the group's rays, at least one; the
  // stack's slots and rows are 32-bit indices
  const uint64_t g = frames_per_group(per, n_cameras, INT_MAX, rows);
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  for (uint32_t f = 0; f < n_cameras; ++f) {
    if (n_supersampled) n_supersampled[f] = 0;
    if (failures) failures[f].count = 0;
  }
  // the camera table, in device form
  DevBuf b_cams;
  grt::CamTable all;
  if ((rc = upload_cam_table(cameras, n_cameras, rows, b_cams, &all))) return rc;
  SeqTimes T;
  uint32_t launches = 0;
  // 1 spp: run_to_host needs the f32 colour, class and status on the host even when the
  // caller does not ask for them (the re-trace of overflowed pixels reads the status)
  std::vector<float> tmp_xyza;
  std::vector<uint8_t> tmp_cls, tmp_status;
  for (uint32_t f0 = 0; f0 < n_cameras; f0 += (uint32_t)g, ++launches) {
    const uint32_t kg = (uint32_t)std::min<uint64_t>(g, n_cameras - f0);
    const uint64_t n = per * kg, at = per * f0;
    const grt::CamTable ct{all.cams + f0, rows, kg};
    if (supersampled) {
      grt_frame_out go{nullptr, out->xyza64 + 4 * at, out->ray_class ? out->ray_class + at : nullptr,
                       out->status ? out->status + at : nullptr, out->stop ? out->stop + at : nullptr,
                       out->steps ? out->steps + at : nullptr};
      if ((rc = sequence_group_super(s, *dc, ct, rows, cols, cfg, mask_xyza, go, n_supersampled ? n_supersampled + f0 : nullptr,
                                     failures ? failures + f0 : nullptr, &T)))
        return rc;
      continue;
    }
    if (!out->xyza) tmp_xyza.resize(n * 4);
    if (!out->ray_class) tmp_cls.resize(n);
    if (!out->status) tmp_status.resize(n);
    grt_aux_out aux;
    std::memset(&aux, 0, sizeof(aux));
    aux.xyza64 = out->xyza64 ? out->xyza64 + 4 * at : nullptr;
    aux.steps = out->steps ? out->steps + at : nullptr;
    aux.stop_reason = out->stop ? out->stop + at : nullptr;
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the group's own: its overflows are its last round's
    float ms = 0;
    const grt::WorkList wl = rect_worklist(0, 0, kg * rows, cols);
    if ((rc = trace_to_host(s, *dc, wl, n, nullptr, out->xyza ? out->xyza + 4 * at : tmp_xyza.data(),
                            out->ray_class ? out->ray_class + at : tmp_cls.data(),
                            out->status ? out->status + at : tmp_status.data(), &aux, acc, &ms, &ct)))
      return rc;
    for (int k = 0; k < 8; ++k) T.acc[k] += acc[k];
    T.trace_ms += ms;
  }
  if (stats) stats_from(T.acc, T.trace_ms + T.super_ms, stats);
  if (report) {
    std::memset(report, 0, sizeof(*report));
    report->n_frames = n_cameras;
    report->n_launches = launches;
    report->frames_per_launch = (uint32_t)g;
    report->trace_ms = T.trace_ms;
    report->supersample_ms = T.super_ms;
    report->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  }
  return 0;
}

}  // extern "C"

namespace grt_host {
// grt_supersample_shard_device; d_local_steps (nullable): the shard's 1-spp step counts in
// local order, for the sub-rays' longest-first work order (order_selection).
int supersample_shard(grt_scene* s, int device, void* stream, const grt_row_shard* sh,
                                const grt_adaptive_config* cfg, double min_lum, const double* d_min_lum,
                                const double* d_frame_ya, const uint8_t* d_frame_class,
                                const double* sampling_mask_xyza, double* d_xyza64, const uint32_t* d_local_steps,
                                uint64_t* d_n_supersampled, uint64_t* d_stats, grt_subsample_failures* failures) {
  if (!s || !cfg || !d_frame_ya || !d_frame_class || !d_xyza64 || !d_stats) return fail(-EINVAL, "null argument");
  if (cfg->samples_per_axis == 0) return fail(-EINVAL, "adaptive_sampling.samples_per_axis must be greater than zero");
  int rc = check_shard(sh);
  if (rc) return rc;
  if (failures) failures->count = 0;
  const uint32_t frame_rows = (uint32_t)s->desc.camera.rows, w = (uint32_t)s->desc.camera.cols;
  const uint32_t local_rows = grt_shard_row_count(frame_rows, sh);
  const uint64_t n_local = (uint64_t)local_rows * w;
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  if (n_local == 0) {
    if (d_n_supersampled) HIP_TRY(hipMemsetAsync(d_n_supersampled, 0, 8, st));
    return 0;
  }
  if (n_local > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "shard larger than INT_MAX pixels");
  AdaptivePlan P;
  P.n = n_local;
  P.w = w;
  P.h = local_rows;  // the work order's 3 x 3 neighbourhood lies in the shard's own rows
  P.spa = cfg->samples_per_axis;
  P.section = false;
  P.shard = true;
  P.ordered = d_local_steps && !sampling_mask_xyza;
  P.sub_rays = !sampling_mask_xyza;
  if ((rc = P.plan(*dc, failures))) return rc;
  if ((rc = stream_order(*dc, st))) return rc;
  HIP_TRY(hipMemsetAsync(P.d_cnt, 0, 16, st));
  // this shard's pixels with the whole frame's 1-spp buffer as the neighbourhood; selected
  // pixels in frame order (shard rows increase with local rows)
  const grt::AdaptiveParams ap = adaptive_params(cfg, w, frame_rows, min_lum);
  if ((rc = P.enqueue_select(st, d_frame_ya, d_frame_class, ap, P.d_cnt, sh, d_min_lum, local_rows)) ||
      (rc = P.enqueue_tail(s, *dc, st, 0, 0, frame_rows, w, P.d_cnt, sampling_mask_xyza, d_xyza64, d_local_steps,
                           (unsigned long long*)d_stats, 0, nullptr, sh)))
    return rc;
  if (d_n_supersampled) HIP_TRY(hipMemcpyAsync(d_n_supersampled, P.d_cnt, 8, hipMemcpyDeviceToDevice, st));
  if ((rc = stream_done(*dc, st))) return rc;
  if (failures) {
    unsigned long long cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, P.d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = P.fails[0].read(cnt[1], P.spa, failures))) return rc;
  }
  return 0;
}

}  // namespace grt_host

extern "C" {

int grt_supersample_shard_device(grt_scene* s, int device, void* stream, const grt_row_shard* sh,
                                 const grt_adaptive_config* cfg, double min_lum, const double* d_min_lum,
                                 const double* d_frame_ya, const uint8_t* d_frame_class,
                                 const double* sampling_mask_xyza, double* d_xyza64,
                                 uint64_t* d_n_supersampled, uint64_t* d_stats, grt_subsample_failures* failures) {
  return grt_host::supersample_shard(s, device, stream, sh, cfg, min_lum, d_min_lum, d_frame_ya, d_frame_class,
                                     sampling_mask_xyza, d_xyza64, nullptr, d_n_supersampled, d_stats, failures);
}

int grt_supersample_shard(grt_scene* s, int device, void* stream, const grt_row_shard* sh,
                          const grt_adaptive_config* cfg, double min_lum, const double* d_frame_ya,
                          const uint8_t* d_frame_class, const double* sampling_mask_xyza, double* d_xyza64,
                          uint64_t* n_supersampled, uint64_t* d_stats) {
  if (n_supersampled) *n_supersampled = 0;
  if (!s) return fail(-EINVAL, "null argument");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  DevBuf cnt;
  if ((rc = cnt.alloc(8))) return rc;
  HIP_TRY(hipMemsetAsync(cnt.p, 0, 8, (hipStream_t)stream));
  if ((rc = grt_supersample_shard_device(s, device, stream, sh, cfg, min_lum, nullptr, d_frame_ya, d_frame_class,
                                         sampling_mask_xyza, d_xyza64, (uint64_t*)cnt.p, d_stats, nullptr)))
    return rc;
  uint64_t v = 0;
  HIP_TRY(hipMemcpyAsync(&v, cnt.p, 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (n_supersampled) *n_supersampled = v;
  return 0;
}

// The luminance floor written to device memory (no host round trip): the multi-GPU
// adaptive pass hands it to grt_supersample_shard_device.  Scratch from the scene's
// grow-only arena on `device`, stream-ordered.
int grt_adaptive_floor_device(grt_scene* s, int device, void* stream, const double* d_y, uint32_t stride, uint64_t n,
                              double* d_min_lum) {
  if (!s || !d_min_lum || (n && (!d_y || stride == 0))) return fail(-EINVAL, "null argument");
  if (n > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "more than INT_MAX luminances");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(d_min_lum, 0, 8, st));  // +0.0
    return 0;
  }
  size_t bytes = 0;
  HIP_TRY(grt::luminance_floor_device(d_y, stride, n, floor_index(n), nullptr, &bytes, nullptr, st));
  if ((rc = ad_reserve(*dc, bytes))) return rc;
  if ((rc = stream_order(*dc, st))) return rc;
  HIP_TRY(grt::luminance_floor_device(d_y, stride, n, floor_index(n), dc->ad_mem, &bytes, d_min_lum, st));
  return stream_done(*dc, st);
}

}  // extern "C"
