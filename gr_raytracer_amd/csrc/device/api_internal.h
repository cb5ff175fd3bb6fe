// api_internal.h — what the units of the C ABI's device side share: api.hip (scenes, the
// trace, the plain entry points), api_adaptive.hip (the adaptive pass, camera sequences)
// and api_gbuffer.hip (geometry buffers).  Nothing here is part of the library's interface.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "grt_api.h"
#include "../host/host_internal.h"
#include "dev_scene.h"
#include "kernels.h"

// The shared items live in grt_api with hidden visibility, so that the library exports
// none of them.  The attribute holds for one namespace block only: every block that
// declares or defines a shared item opens with this.
#define GRT_API_NAMESPACE namespace grt_api __attribute__((visibility("hidden")))

GRT_API_NAMESPACE {

int fail(int code, const std::string& msg);  // sets grt_last_error, returns code
#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      (void)hipGetLastError(); /* clear it: a later launch check must not see it */    \
      return fail(-EIO, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    }                                                                                    \
  } while (0)

struct HostTexture {
  std::vector<uint32_t> rgba;
};

struct DeviceCopy {
  std::atomic<bool> ready{false};  // set (release) once the device copy below is complete
  grt::DevScene* d_scene = nullptr;
  std::vector<void*> allocations;
  unsigned long long* d_counter = nullptr;  // [0] work counter, [5..6] hit pool (HitPool::count)
  unsigned long long* d_stats = nullptr;    // [0..3] accepted, attempts, rays, overflows
  // [0] jobs, [1] job cursor, [2] samples, [3] jobs (cumulative), [4] noise samples,
  // [5] emitting samples, [8 + k] march_kernel's claim cursor of object k's pass
  unsigned long long* d_march = nullptr;
  bool vol = false;                         // the scene has VolumetricDiscs
  int cus = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::mutex mu;  // calls on one device are serialised
  // the last stream that enqueued work into the shared scratch below (stream_order)
  hipEvent_t ev_busy = nullptr;
  hipStream_t busy_stream = nullptr;
  bool busy = false;
  // integrate -> shade hand-off buffers, grown on demand (bytes per ray: ~1.1 KB)
  uint64_t ws_cap = 0;
  bool ws_vol = false;  // the arena holds the volumetric arrays
  void* ws_mem = nullptr;
  // tile-order scratch (probe counts, keys, indices, order, radix-sort temp), grow-only
  uint64_t sched_tiles = 0;
  void* sched_mem = nullptr;
  // adaptive-pass scratch (section buffers, flags, selection, sort and sub-ray buffers),
  // grow-only: no allocation (and no implicit device synchronisation) between passes
  uint64_t ad_bytes = 0;
  void* ad_mem = nullptr;
  // long-ray hand-off (Kerr-Schild): [0] live, [1] handed off, [2] claim cursor; entries, grow-only
  unsigned long long* d_tail_ctl = nullptr;  // 16 words (TailList::ctl)
  uint64_t tail_cap = 0;
  unsigned long long* tail_mem = nullptr;
  // hit pool: window candidates past a ray's GRT_WS_SLOTS workspace slots, grow-only
  uint64_t pool_cap = 0;
  bool pool_vol = false;
  void* pool_mem = nullptr;
  uint64_t ws_jobs_pool = 0;  // pool capacity the workspace's raymarch job list was sized for
  uint32_t *ws_head = nullptr, *ws_last = nullptr;  // per-ray list ends, carved from the workspace
  grt::HitPool* d_pool = nullptr;  // the descriptor the kernels read (device memory)
  grt::HitPool pool_desc{};        // what *d_pool holds
  // lapse traces only (grt_gbuffer_trace_lapse; the first one allocates them, ensure_hit_times):
  // the coordinate time of every candidate, beside the workspace slots and the pool records
  void* slot_time_mem = nullptr;  // f64[GRT_WS_SLOTS][slot_time_cap], slot_time_cap >= ws_cap
  uint64_t slot_time_cap = 0;
  void* pool_time_mem = nullptr;  // f64[pool_time_cap], pool_time_cap >= pool_cap
  uint64_t pool_time_cap = 0;
};

constexpr uint64_t POOL_MAX = (1ull << 31) - 1;      // job and list encodings hold 31 bits

}  // namespace grt_api

struct grt_scene {
  using HostTexture = grt_api::HostTexture;
  using DeviceCopy = grt_api::DeviceCopy;
  grt_scene_desc desc;
  HostTexture celestial;
  HostTexture obj_tex[GRT_MAX_OBJECTS];
  std::vector<double> lut_r[GRT_MAX_OBJECTS], lut_t[GRT_MAX_OBJECTS];
  std::vector<double> bb_log_t, bb_xyz;
  // one device copy per GPU, created on first use (ensure_device).  Fixed slots, so that a
  // host thread looking up its device never sees the table move under it while another
  // thread creates a copy for its own device.
  static constexpr int MAX_DEVICES = 64;
  std::atomic<DeviceCopy*> devices[MAX_DEVICES] = {};
  std::mutex mu;  // creation of the slots' copies
};

GRT_API_NAMESPACE {

// ---- api.hip ----
int ensure_device(grt_scene* s, int device, DeviceCopy** out);
int ensure_pool(DeviceCopy& dc, uint64_t want);
int ensure_workspace(DeviceCopy& dc, uint64_t n, grt::Workspace* ws);
int stream_order(DeviceCopy& dc, hipStream_t st);
int stream_done(DeviceCopy& dc, hipStream_t st);
void fill_dev_camera(const grt_camera_desc& c, grt::DevCamera& cam);
grt::WorkList rect_worklist(uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols);
// the offsets-mode list of n_items (pixel, dx, dy) items of the rectangle, all device arrays
grt::WorkList offsets_worklist(uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, uint64_t n_items,
                               const uint32_t* pix, const double* dx, const double* dy);
int check_rect(const grt_scene* s, uint64_t row0, uint64_t col0, uint64_t rows, uint64_t cols);
int check_shard(const grt_row_shard* sh);
// the rectangle work list of the shard's local rows, full width
grt::WorkList shard_worklist(const grt_scene* s, const grt_row_shard* sh);
// lapse (with exact, no ct, no VolumetricDisc): the lapse unit's kernels, which also record hit times
int enqueue_trace(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl_in, const grt::Outputs& o,
                  unsigned long long* d_stats, hipStream_t stream, const grt::CamTable* ct = nullptr,
                  bool exact = false, bool lapse = false);
int pool_check(DeviceCopy& dc, bool* again);
int reset_counters(DeviceCopy& dc, hipStream_t st);
int read_counters(DeviceCopy& dc, unsigned long long acc[8]);
void stats_from(const unsigned long long acc[8], double kernel_ms, grt_stats* stats);
int trace_sync(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, const grt::Outputs& o,
               unsigned long long acc[8], float* ms, unsigned long long* need, const grt::CamTable* ct = nullptr,
               bool exact = false, bool lapse = false);
int trace_to_host(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, uint64_t n, const grt_offsets* offs,
                  float* xyza_out, uint8_t* class_out, uint8_t* status_out, const grt_aux_out* aux,
                  unsigned long long acc[8], float* ms_out, const grt::CamTable* ct = nullptr);

// A device allocation and its owner: moved, never copied (a copy would free it twice).
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);  // o frees what this held
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  int alloc(size_t n) {
    if (n == 0) n = 16;
    HIP_TRY(hipMalloc(&p, n));
    return 0;
  }
};

// the cameras in device form, uploaded to `buf` (api.hip); *ct: the table over all of them
int upload_cam_table(const grt_camera_desc* cameras, uint32_t n, uint32_t rows, DevBuf& buf, grt::CamTable* ct);

// ---- api_adaptive.hip ----
// Bump allocator over the device's grow-only adaptive arena.  Plan the whole call's
// buffers first (ad_plan), then carve them (ad_take): growing the arena happens before
// any kernel of the call is enqueued.
struct AdArena {
  char* base = nullptr;
  uint64_t off = 0;
  void* take(uint64_t bytes) {
    void* r = base ? base + off : nullptr;
    off += (bytes + 255) & ~255ull;
    return r;
  }
};
int ad_reserve(DeviceCopy& dc, uint64_t bytes);

constexpr uint64_t SUB_CHUNK = 1ull << 21;  // sub-rays per supersample trace launch
extern std::atomic<uint64_t> g_sub_chunk;    // grt_set_sub_chunk (tests force several chunks)
extern std::atomic<uint64_t> g_seq_group;    // grt_set_sequence_group: rays per launch group
// Frames per launch group of a stack of n frames of `per` rays: whole frames within the
// group's rays, at least one; at most max_slots rays (0: no cap) and, where the stack's rows
// are 32-bit indices, 2^32 - 1 stacked rows of `rows` a frame (0: no cap).
uint64_t frames_per_group(uint64_t per, uint64_t n, uint64_t max_slots = 0, uint64_t rows = 0);

// Buffers of the supersample pass over at most n_max selected pixels.
struct SuperBufs {
  uint64_t chunk_pix = 0, cap = 0;
  uint32_t n_chunks = 0, per = 0;
  uint32_t* pix = nullptr;
  double *dx = nullptr, *dy = nullptr, *x64 = nullptr;
  float* xyza = nullptr;
  uint8_t *cls = nullptr, *status = nullptr, *stop = nullptr;
  uint32_t* steps = nullptr;
  unsigned long long* live = nullptr;
  // The chunking of at most n_max selected pixels: chunk_pix pixels (cap sub-rays) a chunk.
  void plan(uint64_t n_max, uint32_t spa) {
    per = spa * spa;
    chunk_pix = std::max<uint64_t>(1, std::min<uint64_t>(n_max, g_sub_chunk.load(std::memory_order_relaxed) / per));
    n_chunks = (uint32_t)((n_max + chunk_pix - 1) / chunk_pix);
    cap = chunk_pix * per;
  }
  // One chunk's sub-ray outputs (all the g-buffer's re-shade needs: it traces nothing).
  void carve_outputs(AdArena& A) {
    xyza = (float*)A.take(cap * 16);
    cls = (uint8_t*)A.take(cap);
    status = (uint8_t*)A.take(cap);
    x64 = (double*)A.take(cap * 32);
    stop = (uint8_t*)A.take(cap);
    steps = (uint32_t*)A.take(cap * 4);
  }
  void carve(AdArena& A) {
    pix = (uint32_t*)A.take(cap * 4);
    dx = (double*)A.take(cap * 8);
    dy = (double*)A.take(cap * 8);
    carve_outputs(A);
    live = (unsigned long long*)A.take((uint64_t)n_chunks * 8);
  }
};

int enqueue_supersample(grt_scene* s, DeviceCopy& dc, hipStream_t st, const SuperBufs& B, uint32_t row0, uint32_t col0,
                        uint32_t rows, uint32_t cols, const uint32_t* sel_px, const uint32_t* sel_out,
                        const unsigned long long* d_count, uint32_t spa, double* d_out64, unsigned long long* d_stats,
                        const grt::SubsampleFailures& fails_in, const grt::CamTable* ct = nullptr,
                        uint32_t stack_row0 = 0);
// resolve_minimum_luminance's index of the floor's element among n luminances
inline uint64_t floor_index(uint64_t n) { return (uint64_t)((double)(n - 1) * 0.99); }
int copy_failures(const grt::SubsampleFailures& f, uint64_t count, uint32_t spa, grt_subsample_failures* out);
grt::AdaptiveParams adaptive_params(const grt_adaptive_config* cfg, uint32_t w, uint32_t h, double min_lum);

// The device side of one grt_subsample_failures list (nullable: nothing is recorded).
struct FailBufs {
  grt::SubsampleFailures f{};
  bool events = false;  // NaN / no-terminal-event sub-rays too (scene.rs:178-183, :196-202)
  void plan(const grt_subsample_failures* out) {
    f.cap = (out && out->pixel && out->status) ? out->capacity : 0;
    events = f.cap && out->stop;
  }
  void carve(AdArena& A) {
    f.key = (uint64_t*)A.take(f.cap * 8);
    f.status = (uint8_t*)A.take(f.cap);
    f.stop = events ? (uint8_t*)A.take(f.cap) : nullptr;
    f.steps = events ? (uint32_t*)A.take(f.cap * 4) : nullptr;
  }
  // after the pass: `count` failed sub-samples (the pass's cnt[1]) to the caller's list
  int read(uint64_t count, uint32_t spa, grt_subsample_failures* out) const {
    if (!out) return 0;
    out->count = count;
    return copy_failures(f, count, spa, out);
  }
};

// The 1-spp buffers of a section of n pixels (stacked frames: n of them back to back).
struct SectionBufs {
  float* xyza = nullptr;
  uint8_t *cls = nullptr, *status = nullptr, *stop = nullptr;
  double* x64 = nullptr;
  uint32_t* steps = nullptr;
  void carve(AdArena& A, uint64_t n, bool want_stop, bool want_steps) {
    xyza = (float*)A.take(n * 16);
    cls = (uint8_t*)A.take(n);
    status = (uint8_t*)A.take(n);
    x64 = (double*)A.take(n * 32);
    if (want_stop) stop = (uint8_t*)A.take(n);
    if (want_steps) steps = (uint32_t*)A.take(n * 4);
  }
  grt::Outputs outputs() const { return grt::Outputs{xyza, cls, status, x64, steps, stop, nullptr}; }
};

// The adaptive pass (raytracer.rs:257-318) over a 1-spp buffer on the device: the
// luminance floor, the selection stencil and its compaction (enqueue_select), then the
// sampling mask painted over the selection, or the selection ordered and supersampled
// (enqueue_tail).  One plan holds the scratch of every entry point that runs the pass;
// what the caller sets decides which buffers exist:
//   grt_render_section_ex   the section's 1-spp buffers of n pixels
//   sequence_group_super    the stack's, `frames` x n pixels; the selection scratch is one
//                           frame's, reused from frame to frame, the counts are per frame
//   supersample_shard       `shard`: the caller's buffers, no floor (the caller's), and
//                           the frame indices of the selection beside the local ones
//   grt_gbuffer_shade_section  `held`: no trace, so no sub-ray offsets; the held / missing
//                           split of the selection, four counts
//   grt_gbuffer_shade_section_sequence  `held` and `stack`: the stack's 1-spp buffers; the
//                           selections of all `frames` kept side by side (frame f's at
//                           sel + f * n), one split and one sub-ray pass over all of them,
//                           four counts per frame and the two totals after them
struct AdaptivePlan {
  // set by the caller before plan()
  uint64_t n = 0;          // pixels of one selection
  uint32_t w = 0, h = 0;   // their rectangle (order_selection's neighbourhood)
  uint32_t frames = 1, spa = 1;
  bool section = true;     // SectionBufs (with stop / steps as asked for)
  bool sec_stop = false, sec_steps = false;
  bool supersampled = true, device_floor = false, ordered = false, sub_rays = false;
  bool shard = false, held = false, stack = false;
  std::vector<FailBufs> fails;  // one per frame
  // sizes (plan) and buffers (carve)
  size_t sort_bytes = 0, select_bytes = 0, order_bytes = 0, split_bytes = 0;
  SectionBufs sec;
  uint8_t *flags = nullptr, *split = nullptr;
  uint32_t *sel = nullptr, *sel_frame = nullptr, *order = nullptr, *held_px = nullptr, *missing_px = nullptr;
  uint32_t* stack_px = nullptr;              // stack: the selections as stacked indices f * n + pixel
  grt::GBufferFrame* frame_tab = nullptr;    // stack: device tables, one entry per frame
  grt::GBufferSubFrame* sub_tab = nullptr;
  grt::SubsampleFailures* fail_tab = nullptr;
  unsigned long long* d_cnt = nullptr;  // per frame: [0] selected pixels, [1] failed sub-samples (held: [2] held, [3] missing)
  double* d_floor = nullptr;
  void *sort = nullptr, *select = nullptr, *order_tmp = nullptr, *split_tmp = nullptr;
  SuperBufs B;

  uint64_t cnt_bytes() const { return (held ? 32ull : 16ull) * frames + (stack ? 32ull : 0ull); }
  uint64_t sel_n() const { return stack ? n * frames : n; }  // entries of the selection arrays
  unsigned long long* d_totals() const { return d_cnt + 4ull * frames; }  // stack: [0] held, [1] missing

  // The scratch sizes, then the buffers from the device's arena, grown first if need be.
  int plan(DeviceCopy& dc, const grt_subsample_failures* failures) {
    fails.assign(frames, FailBufs());
    for (uint32_t f = 0; f < frames && failures; ++f) fails[f].plan(&failures[f]);
    if (device_floor)
      HIP_TRY(grt::luminance_floor_device(nullptr, 4, n, floor_index(n), nullptr, &sort_bytes, nullptr, 0));
    if (supersampled) HIP_TRY(grt::compact_flags(nullptr, n, nullptr, nullptr, nullptr, &select_bytes, 0));
    // the supersample pass's work order (longest sub-rays first) reads the 1-spp step counts
    if (ordered) HIP_TRY(grt::order_selection(nullptr, nullptr, n, nullptr, w, h, nullptr, nullptr, &order_bytes, 0));
    if (held && sub_rays && !stack)
      HIP_TRY(grt::gbuffer_split(nullptr, nullptr, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 &split_bytes, 0));
    if (held && sub_rays && stack)
      HIP_TRY(grt::gbuffer_split_stack(nullptr, nullptr, frames, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, &split_bytes, 0));
    if (sub_rays) B.plan(sel_n(), spa);
    AdArena sizes;
    carve(sizes);
    if (int rc = ad_reserve(dc, sizes.off)) return rc;
    AdArena A{(char*)dc.ad_mem, 0};
    carve(A);
    return 0;
  }

  // A bump allocator: the order of the takes decides the addresses.  Every entry point
  // keeps the order it had when its pass was written on its own, so the shard path takes
  // its order arrays after the compaction scratch, the others before the flags.
  void carve(AdArena& A) {
    if (section) sec.carve(A, n * frames, sec_stop, sec_steps);
    if (stack) frame_tab = (grt::GBufferFrame*)A.take(frames * sizeof(grt::GBufferFrame));
    if (!supersampled) return;
    if (ordered && !shard) carve_order(A);
    flags = (uint8_t*)A.take(n);
    sel = (uint32_t*)A.take((sub_rays ? sel_n() : n) * 4);
    if (shard) sel_frame = (uint32_t*)A.take(n * 4);
    d_cnt = (unsigned long long*)A.take(cnt_bytes());
    if (!shard) {
      d_floor = (double*)A.take(8);
      sort = A.take(sort_bytes);
    }
    select = A.take(select_bytes);
    if (ordered && shard) carve_order(A);
    if (held && sub_rays) {
      split = (uint8_t*)A.take(2 * sel_n());
      held_px = (uint32_t*)A.take(sel_n() * 4);
      missing_px = (uint32_t*)A.take(sel_n() * 4);
      split_tmp = A.take(split_bytes);
      if (stack) stack_px = (uint32_t*)A.take(sel_n() * 4);
    }
    if (stack) {
      sub_tab = (grt::GBufferSubFrame*)A.take(frames * sizeof(grt::GBufferSubFrame));
      fail_tab = (grt::SubsampleFailures*)A.take(frames * sizeof(grt::SubsampleFailures));
    }
    if (sub_rays && held) B.carve_outputs(A);
    else if (sub_rays) B.carve(A);
    for (FailBufs& fb : fails) fb.carve(A);
  }
  void carve_order(AdArena& A) {
    order = (uint32_t*)A.take(n * 4);
    order_tmp = A.take(order_bytes);
  }

  // resolve_minimum_luminance (raytracer.rs:118-129): the exact 99th percentile in
  // f64::total_cmp order, selected on the device from the 1-spp buffer; then
  // collect_pixels_to_supersample (:386-458): the stencil, and the selected pixels in order
  // by a device stream compaction, their count in cnt[0].  sh: a row-band shard's pixels
  // (local_rows of them) with the whole frame (ya, cls) as the neighbourhood and the
  // caller's floor d_min_lum (nullable), else a section's x64 and class.  sel_to: where the
  // selection goes (stack: frame f's place, sel + f * n), else `sel`.
  int enqueue_select(hipStream_t st, const double* x64, const uint8_t* cls, const grt::AdaptiveParams& ap,
                     unsigned long long* cnt, const grt_row_shard* sh = nullptr, const double* d_min_lum = nullptr,
                     uint32_t local_rows = 0, uint32_t* sel_to = nullptr) {
    if (device_floor) HIP_TRY(grt::luminance_floor_device(x64 + 1, 4, n, floor_index(n), sort, &sort_bytes, d_floor, st));
    if (sh)
      HIP_TRY(grt::launch_select_shard(x64, cls, ap, d_min_lum, sh->band_rows, sh->shard, sh->n_shards, local_rows, flags,
                                       st));
    else
      HIP_TRY(grt::launch_select(x64, cls, ap, device_floor ? d_floor : nullptr, flags, st));
    HIP_TRY(grt::compact_flags(flags, n, sel_to ? sel_to : sel, cnt, select, &select_bytes, st));
    return 0;
  }

  // The selection of frame f (cnt = its counts) in the rect row0 / col0 / rows / cols:
  // painted with the mask (raytracer.rs:285-295), or ordered by the 1-spp `steps` and
  // supersampled into x64.  sh: the selection holds a shard's local indices, which are the
  // output's; the camera rays and the jitter hash take the frame's (launch_frame_index).
  int enqueue_tail(grt_scene* s, DeviceCopy& dc, hipStream_t st, uint32_t row0, uint32_t col0, uint32_t rows,
                   uint32_t cols, unsigned long long* cnt, const double* mask_xyza, double* x64, const uint32_t* steps,
                   unsigned long long* d_stats, uint32_t f = 0, const grt::CamTable* ct = nullptr,
                   const grt_row_shard* sh = nullptr) {
    const uint32_t* out = sel;
    if (ordered) {
      HIP_TRY(grt::order_selection(sel, cnt, n, steps, w, h, order, order_tmp, &order_bytes, st));
      out = order;
    }
    const uint32_t* px = out;
    if (sh) {
      HIP_TRY(grt::launch_frame_index(out, cnt, n, w, sh->band_rows, sh->shard, sh->n_shards, sel_frame, st));
      px = sel_frame;
    }
    if (mask_xyza) {
      HIP_TRY(grt::launch_paint(out, n, cnt, mask_xyza, x64, st));
      return 0;
    }
    grt::SubsampleFailures ff = fails[f].f;
    ff.count = cnt + 1;
    return enqueue_supersample(s, dc, st, B, row0, col0, rows, cols, px, out, cnt, spa, x64, d_stats, ff, ct,
                               ct ? f * rows : 0);
  }

  // After the pass has been waited for: the counts of every frame, the selected pixels
  // and the failure lists to the caller's (nullable) arrays.
  int read(uint64_t* n_supersampled, grt_subsample_failures* failures) const {
    std::vector<unsigned long long> cnt(cnt_bytes() / 8);
    HIP_TRY(hipMemcpy(cnt.data(), d_cnt, cnt_bytes(), hipMemcpyDeviceToHost));
    const size_t stride = held ? 4 : 2;
    for (uint32_t f = 0; f < frames; ++f) {
      if (n_supersampled) n_supersampled[f] = cnt[stride * f];
      if (int rc = fails[f].read(cnt[stride * f + 1], spa, failures ? &failures[f] : nullptr)) return rc;
    }
    return 0;
  }
};

// ---- api_gbuffer.hip: a row-band shard's buffer as one block (grt_gbuffer_trace_multi, multi.hip) ----
// The layout of the block: the twelve arrays of GRT_GBUFFER_FIELDS over n rays and `layers`
// layers, each 256-B aligned, the per-ray ones first, so that their places do not move when
// the layer total becomes known.
struct GBufferBlock {
  uint64_t n = 0, layers = 0;
  uint64_t off[grt_host::GB_N_FIELDS] = {};
  uint64_t ray_bytes = 0, bytes = 0;  // the per-ray arrays; the whole block
  GBufferBlock() = default;
  GBufferBlock(uint64_t n_, uint64_t layers_) : n(n_), layers(layers_) {
    for (int pass = 0; pass < 2; ++pass) {
      for (int k = 0; k < grt_host::GB_N_FIELDS; ++k) {
        const grt_host::GBufferField& f = grt_host::GBUFFER_FIELDS[k];
        if (f.layer != (pass == 1)) continue;
        off[k] = bytes;
        bytes += (f.bytes(n, layers) + 255) & ~255ull;
      }
      if (pass == 0) ray_bytes = bytes;
    }
  }
};
// What one rank made of its shard.
struct GBufferShard {
  GBufferBlock block;
  uint8_t* base = nullptr;
  uint32_t n_traces = 0;
  float trace_ms = 0, fill_ms = 0;
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // as trace_sync's
};
// The block's memory, the caller's: at least `bytes` at *base, the first `keep` bytes of what
// the last call returned kept; nothing is in flight on the block when it is called.
using GBufferReserve = std::function<int(uint64_t bytes, uint64_t keep, uint8_t** base)>;
// Trace and fill the shard `sh` of the scene's frame on `device` into one block: the exact
// trace (again with a larger pool while it loses candidates, 3 traces at most), the layer
// scan and the fill on `st`, under the device copy's mutex from the trace to the end of the
// fill.  `reserve` is called once before the trace (the per-ray arrays) and once when the
// layer total is known.  `st` is idle on return.  A shard without rows gives an empty block.
int gbuffer_trace_shard(grt_scene* s, int device, hipStream_t st, const grt_row_shard& sh,
                        const GBufferReserve& reserve, GBufferShard* out);
// An ordinary buffer of the scene's whole frame on `device` with n_layers layers, its arrays
// allocated and unwritten: p[k] is array k of GRT_GBUFFER_FIELDS.  Freed by grt_gbuffer_destroy.
int gbuffer_frame_alloc(const grt_scene* s, int device, uint64_t n_layers, grt_gbuffer** out,
                        void* p[grt_host::GB_N_FIELDS]);
void gbuffer_set_times(grt_gbuffer* gb, double trace_ms, double fill_ms);

}  // namespace grt_api
