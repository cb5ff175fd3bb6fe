// api.hip — C ABI of the device hot path (include/grt_api.h).
//
// grt_scene_create deep-copies the caller's POD descriptor (textures and LUTs
// included); each GPU receives its own device copy the first time it renders.
// grt_render_pixels replaces Raytracer::render_section_to_cie_buffer_raw
// (raytracer.rs:195-244) and supersample (:320-384); grt_render_section replaces
// render_section_to_cie_buffer[_supersampled] (:177-318).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "grt_api.h"
#include "../host/host_internal.h"
#include "dev_scene.h"
#include "kernels.h"

namespace {

// Process-wide tuning knobs (grt_set_*).  The library is called from one host thread per
// device (grt_render_frame_multi, or a host of its own), so a setter may run beside renders
// on other threads: the knobs are atomics, and a trace reads them once, into a Knobs
// snapshot, so that one call never sees two settings.
std::atomic<long long> g_launch{256};  // grt_set_launch_config: blocks per CU << 16 | threads per block
std::atomic<int> g_rkf_short{1};       // grt_debug_rkf_short: 0 = every Schwarzschild attempt with the full RKF sums, 2 = the fallback forced (tests)
std::atomic<int> g_range_free{1};      // grt_debug_range_free: 0 = every division and sqrt in its IEEE form (tests)
std::atomic<int> g_class_order{-1};    // grt_set_class_order: -1 auto, 0 off, 1 / 2 forced (tiles by sincos class)
std::atomic<int> g_schedule{-1};       // grt_set_schedule: -1 auto, 0 row-major tiles, 1 probe-ordered tiles
std::atomic<int> g_two_ended{1};       // grt_set_two_ended: probe-ordered traces take the queue from both ends
std::atomic<long long> g_tail{-1};     // grt_set_tail: -1 auto, 0 off, > 0 hand-off threshold (live rays)
std::atomic<int> g_arith{0};           // grt_set_arithmetic: 0 exact (reference bits), 1 fused (FMA contraction)
constexpr uint32_t PROBE_CAP = 32768;  // upper bound of the probe's step cap

struct Knobs {
  int blocks_per_cu, threads, schedule, two_ended;
  long long tail;
  int arith, class_order;
  static Knobs now() {
    const long long l = g_launch.load(std::memory_order_relaxed);
    return Knobs{(int)(l >> 16), (int)(l & 0xffff), g_schedule.load(std::memory_order_relaxed),
                 g_two_ended.load(std::memory_order_relaxed), g_tail.load(std::memory_order_relaxed),
                 g_arith.load(std::memory_order_relaxed), g_class_order.load(std::memory_order_relaxed)};
  }
};


int fail(int code, const std::string& msg) {
  grt_host::set_error(msg);
  return code;
}
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
};

constexpr uint64_t POOL_MIN = 1ull << 20;            // records
constexpr uint64_t POOL_MAX = (1ull << 31) - 1;      // job and list encodings hold 31 bits
std::atomic<uint64_t> g_pool_min{POOL_MIN};         // grt_set_hit_pool_min (tests force a full pool)
uint64_t pool_record_bytes(bool vol) { return 4 + 1 + 4 * 8 + 3 * 8 + 4 + 4 * 8 + 4 + (vol ? 3 * 8 + 4 * 8 : 0); }

// Grow the hit pool to at least `want` records (never shrinks).
int ensure_pool(DeviceCopy& dc, uint64_t want) {
  want = std::min(std::max(want, g_pool_min.load(std::memory_order_relaxed)), POOL_MAX);
  if (want <= dc.pool_cap && dc.pool_mem && (!dc.vol || dc.pool_vol)) return 0;
  want = std::max(want, dc.pool_cap);
  if (dc.pool_mem) {
    (void)hipDeviceSynchronize();  // earlier async launches may still use the old pool
    (void)hipFree(dc.pool_mem);
  }
  dc.pool_mem = nullptr;
  dc.pool_cap = 0;
  if (hipMalloc(&dc.pool_mem, want * pool_record_bytes(dc.vol) + 16 * 256) != hipSuccess) {
    (void)hipGetLastError();
    dc.pool_mem = nullptr;
    return fail(-ENOMEM, "cannot allocate the hit pool");
  }
  dc.pool_cap = want;
  dc.pool_vol = dc.vol;
  return 0;
}

// The scratch of a device (workspace, hit pool, tile order, tail list, adaptive arena) is
// one grow-only set per device and every call carves it from offset 0.  An async call
// on another stream than the previous one first waits for that stream's work in it
// (one event), so two streams never run in the same scratch at once; the call then
// records the event on its own stream (stream_done).
int stream_order(DeviceCopy& dc, hipStream_t st) {
  if (dc.busy && dc.busy_stream != st) HIP_TRY(hipStreamWaitEvent(st, dc.ev_busy, 0));
  return 0;
}
int stream_done(DeviceCopy& dc, hipStream_t st) {
  HIP_TRY(hipEventRecord(dc.ev_busy, st));
  dc.busy_stream = st;
  dc.busy = true;
  return 0;
}

grt::HitPool pool_view(const DeviceCopy& dc) {
  grt::HitPool hp;
  std::memset(&hp, 0, sizeof(hp));
  hp.head = dc.ws_head;
  hp.last = dc.ws_last;
  const uint64_t m = dc.pool_cap;
  char* p = (char*)dc.pool_mem;
  auto take = [&](uint64_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~255ull;
    return (void*)r;
  };
  hp.cap = m;
  hp.count = dc.d_counter + 5;
  hp.p = (double*)take(4 * 8 * m);
  hp.pt = (double*)take(3 * 8 * m);
  hp.hcol = (double*)take(4 * 8 * m);
  hp.win = (uint32_t*)take(4 * m);
  hp.next = (uint32_t*)take(4 * m);
  hp.hprev = (uint32_t*)take(4 * m);
  hp.obj = (uint8_t*)take(m);
  if (dc.pool_vol) {
    hp.dir = (double*)take(3 * 8 * m);
    hp.vcol = (double*)take(4 * 8 * m);
  }
  return hp;
}

// Carve a Workspace for n rays out of the device's grow-only arena.
int ensure_workspace(DeviceCopy& dc, uint64_t n, grt::Workspace* ws) {
  const uint64_t M = GRT_WS_SLOTS;
  const bool vol = dc.vol;
  // ray record (64 B), KerrBL's meta record (16 B), pool list ends (8 B), candidate slots;
  // volumetric scenes: the ray constants (48 B), chord directions, raymarched colours, jobs
  const uint64_t per_ray = 64 + 16 + 8 + M * 64 + (vol ? 6 * 8 + M * (3 * 8 + 4 * 8 + 8) : 0);
  // volumetric scenes: the raymarch job list also holds one job per pool record
  const uint64_t jobs_extra = vol ? dc.pool_cap : 0;
  if (n > dc.ws_cap || (vol && !dc.ws_vol) || jobs_extra > dc.ws_jobs_pool) {
    if (dc.ws_mem) {
      (void)hipDeviceSynchronize();  // earlier async launches may still use the old arena
      (void)hipFree(dc.ws_mem);
    }
    dc.ws_mem = nullptr;
    uint64_t cap = std::max<uint64_t>(n, 1 << 16);
    if (hipMalloc(&dc.ws_mem, cap * per_ray + jobs_extra * 8 + 32 * 256) != hipSuccess) {  // + per-array alignment
      (void)hipGetLastError();
      dc.ws_mem = nullptr;
      dc.ws_cap = 0;
      return fail(-ENOMEM, "cannot allocate the integrate/shade workspace");
    }
    dc.ws_cap = cap;
    dc.ws_vol = vol;
    dc.ws_jobs_pool = jobs_extra;
  }
  uint64_t cap = dc.ws_cap;
  char* p = (char*)dc.ws_mem;
  auto take = [&](uint64_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~255ull;
    return (void*)r;
  };
  ws->n = n;
  ws->fin = (double*)take(64 * cap);
  ws->meta = (uint32_t*)take(16 * cap);
  ws->steps = nullptr;  // launch_trace points it at Outputs::steps
  ws->rc = vol ? (double*)take(6 * 8 * cap) : nullptr;
  ws->rec = (grt::CandRec*)take(M * 64 * cap);
  dc.ws_head = (uint32_t*)take(4 * cap);
  dc.ws_last = (uint32_t*)take(4 * cap);
  ws->rec_dir = ws->vcol = nullptr;
  ws->jobs = nullptr;
  ws->march = dc.d_march;
  ws->n_live = nullptr;
  if (vol) {
    ws->rec_dir = (double*)take(3 * M * 8 * cap);
    ws->vcol = (double*)take(4 * M * 8 * cap);
    ws->jobs = (uint64_t*)take(M * 8 * cap + 8 * dc.ws_jobs_pool);
  }
  // the kernels index with the launch's n, which must not exceed the carved capacity
  if (n > cap) return fail(-ENOMEM, "workspace too small");
  return 0;
}

}  // namespace

struct grt_scene {
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

namespace {

void copy_texture(const grt_texture_desc& t, HostTexture& out) {
  if (t.kind == GRT_TEX_BITMAP && t.rgba && t.width && t.height) {
    size_t n = (size_t)t.width * t.height;
    out.rgba.resize(n);
    std::memcpy(out.rgba.data(), t.rgba, n * 4);
  }
}

template <class T>
int upload(DeviceCopy& dc, const T* src, size_t n, T** dst) {
  *dst = nullptr;
  if (n == 0) return 0;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, n * sizeof(T)));
  dc.allocations.push_back(p);
  HIP_TRY(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
  *dst = (T*)p;
  return 0;
}

void fill_dev_texture(const grt_texture_desc& t, grt::DevTexture& d) {
  d.kind = t.kind;
  d.width = t.width;
  d.height = t.height;
  d.beaming = t.beaming_exponent;
  d.rgba = nullptr;
  d.cw = t.checker_width;
  d.ch = t.checker_height;
  for (int k = 0; k < 4; ++k) {
    d.c1[k] = t.c1[k];
    d.c2[k] = t.c2[k];
  }
}

// The device form of a camera (DevScene::cam, or an entry of a sequence's CamTable).
void fill_dev_camera(const grt_camera_desc& c, grt::DevCamera& cam) {
  for (int k = 0; k < 4; ++k) {
    cam.pos[k] = c.position[k];
    cam.vel[k] = c.velocity[k];
    for (int j = 0; j < 4; ++j) cam.tet[k][j] = c.tetrad[k][j];
  }
  cam.tan_half_alpha = c.tan_half_alpha;
  cam.rows = (double)c.rows;
  cam.cols = (double)c.cols;
  cam.sig_s = c.spatial_signature;
  cam.hand = c.spatial_handedness;
  cam.sin_theta = c.sin_theta;
  cam.cos_theta = c.cos_theta;
}

int init_device_copy(grt_scene* s, int device, DeviceCopy& dc);

// The scene's copy on `device`, uploaded on first use.  Safe from one host thread per device
// (and from several threads on one device: the first uploads, the others wait for it).
int ensure_device(grt_scene* s, int device, DeviceCopy** out) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(-ENODEV, "invalid device ordinal");
  if (device >= grt_scene::MAX_DEVICES) return fail(-ENODEV, "device ordinal beyond the library's 64 slots");
  DeviceCopy* p = s->devices[device].load(std::memory_order_acquire);
  if (!p) {
    std::lock_guard<std::mutex> lk(s->mu);
    p = s->devices[device].load(std::memory_order_acquire);
    if (!p) {
      p = new DeviceCopy();
      s->devices[device].store(p, std::memory_order_release);
    }
  }
  DeviceCopy& dc = *p;
  *out = &dc;
  if (dc.ready.load(std::memory_order_acquire)) return 0;
  std::lock_guard<std::mutex> lk(dc.mu);
  if (dc.ready.load(std::memory_order_acquire)) return 0;
  return init_device_copy(s, device, dc);
}

// The device copy of a scene on `device` if one is complete, else nullptr.
DeviceCopy* find_device(const grt_scene* s, int device) {
  if (device < 0 || device >= grt_scene::MAX_DEVICES) return nullptr;
  DeviceCopy* p = s->devices[device].load(std::memory_order_acquire);
  return (p && p->ready.load(std::memory_order_acquire)) ? p : nullptr;
}

int init_device_copy(grt_scene* s, int device, DeviceCopy& dc) {
  HIP_TRY(hipSetDevice(device));
  const grt_scene_desc& d = s->desc;
  grt::DevScene ds;
  std::memset(&ds, 0, sizeof(ds));
  ds.geometry = d.geometry;
  ds.n_objects = d.n_objects;
  ds.radius = d.radius;
  ds.a = d.a;
  ds.horizon_epsilon = d.horizon_epsilon;
  // horizon thresholds exactly as schwarzschild.rs:181-183, kerr.rs:382-394, kerr_bl.rs:482-492
  if (d.geometry == GRT_GEOM_SCHWARZSCHILD) {
    ds.horizon_r = d.radius + d.horizon_epsilon;
    ds.has_horizon = 1;
  } else if (d.geometry == GRT_GEOM_KERR || d.geometry == GRT_GEOM_KERR_BL) {
    double m = d.geometry == GRT_GEOM_KERR ? 0.5 * d.radius : d.radius / 2.0;
    ds.has_horizon = !(std::fabs(d.a) > d.radius / 2.0);
    double disc = std::fmax(m * m - d.a * d.a, 0.0);
    double rp = m + std::sqrt(disc);
    ds.horizon_r = rp + d.horizon_epsilon;
  }
  ds.max_steps = d.max_steps;
  ds.max_radius_sq = d.max_radius * d.max_radius;
  ds.step_size = d.step_size;
  ds.epsilon = d.epsilon;
  ds.trapped_radius = 5.0 * d.radius;
  // Far-field filter bounds.  The margins (1e-9 relative) are ~1e6 x the rounding of
  // the Cartesian conversion and of the chord arithmetic, so every window the filter
  // skips would have been a miss in the reference too ("Exact skips").
  ds.far_ok = (d.geometry == GRT_GEOM_SCHWARZSCHILD || d.geometry == GRT_GEOM_KERR_BL ||
               d.geometry == GRT_GEOM_EUCLIDEAN_SPHERICAL) ? 1 : 0;
  ds.far_a = d.geometry == GRT_GEOM_KERR_BL ? std::fabs(d.a) : 0.0;
  ds.cel_lo2 = ds.max_radius_sq * (1.0 - 1e-9);
  ds.cel_hi2 = ds.max_radius_sq * (1.0 + 1e-9);
  if (!std::isfinite(ds.far_a) || !std::isfinite(ds.max_radius_sq)) ds.far_ok = 0;
  {
    int ex = 0;
    std::frexp(d.radius, &ex);
    ds.div_share = (std::fpclassify(d.radius) == FP_NORMAL && ex > -500 && ex < 500) ? 1 : 0;
    int ea = 0;
    std::frexp(d.a, &ea);
    // KerrBL: a normal |a| within 2^+-50; Kerr-Schild (ks_fd_ok): radius and a normal
    // within 2^+-20, or a == 0
    const int lim = d.geometry == GRT_GEOM_KERR ? 20 : 50;
    const bool a_mod = std::fpclassify(d.a) == FP_NORMAL && ea > -lim && ea < lim;
    const bool a_ok = d.geometry == GRT_GEOM_KERR_BL ? a_mod : (d.geometry != GRT_GEOM_KERR || a_mod || d.a == 0.0);
    ds.div_fast = (g_range_free.load(std::memory_order_relaxed) && std::fpclassify(d.radius) == FP_NORMAL && d.radius > 0.0 && ex > -lim && ex < lim &&
                   a_ok) ? 1 : 0;
    // radius == 1.0, the unit of every black-hole scene of the reference: the region-B
    // Schwarzschild quotients drop their multiplies by it (rcp_seed.h unit_radius_quotients)
    ds.unit_radius = (d.radius == 1.0 && ds.div_fast) ? 1 : 0;
    ds.rkf_short = g_rkf_short.load(std::memory_order_relaxed);
    // schw_div_ok_render's lower edge: radius (1 + 2^-40), moved up until schw_div_ok's own
    // test |r - radius| > 2^-40 radius holds at the edge itself; r - radius is monotone in r,
    // so it then holds for every r above the edge
    ds.div_r_lo = INFINITY;
    if (ds.div_fast) {
      double lo = d.radius * (1.0 + 0x1p-40);
      while (!(lo - d.radius > d.radius * 0x1p-40)) lo = std::nextafter(lo, INFINITY);
      ds.div_r_lo = lo;
    }
    // ks_fd_ok's coordinate bound: 2^ceil(log2(2 max_radius)) covers every state of a ray
    // (it stops one step beyond max_radius), within the proven 2^10 .. 2^32
    int em = 0;
    const double mr2 = 2.0 * d.max_radius;
    const double m = std::isfinite(mr2) && mr2 > 0.0 ? std::frexp(mr2, &em) : 0.0;
    if (m == 0.5) em -= 1;  // an exact power of two is its own bound
    ds.ks_cap = std::ldexp(1.0, !std::isfinite(mr2) ? 32 : std::min(32, std::max(10, em)));
  }
  {  // exact controller shortcuts (geodesic.hip step_control); off unless epsilon is a moderate normal
    int ex = 0;
    std::frexp(d.epsilon, &ex);
    const bool ok = std::fpclassify(d.epsilon) == FP_NORMAL && d.epsilon > 0.0 && ex > -900 && ex < 900;
    ds.pow_skip_err = ok ? d.epsilon / 1800.0 * (1.0 - 1e-9) : 0.0;
    ds.small_lo = ok ? d.epsilon * 1e-5 * (1.0 - 1e-9) : 0.0;
    ds.small_hi = ok ? d.epsilon * 1e-5 * (1.0 + 1e-9) : HUGE_VAL;
    const double t = std::fmin(ds.pow_skip_err, ds.small_lo);
    ds.tiny_err_sq = (ok && t >= 1e-150) ? t * t * (1.0 - 1e-9) : 0.0;  // t^2 stays a normal
  }
  fill_dev_camera(d.camera, ds.cam);
  fill_dev_texture(d.celestial, ds.celestial);
  ds.celestial_temperature = d.celestial_temperature;
  ds.hit_threshold = d.object_hit_opacity_threshold;
  ds.cos_half_pi = std::cos(1.57079632679489661923);
  ds.sin_half_pi = std::sin(1.57079632679489661923);
  int rc;
  uint32_t* tex = nullptr;
  if ((rc = upload(dc, s->celestial.rgba.data(), s->celestial.rgba.size(), &tex))) return rc;
  ds.celestial.rgba = tex;
  for (uint32_t k = 0; k < d.n_objects; ++k) {
    const grt_object_desc& o = d.objects[k];
    grt::DevObject& q = ds.obj[k];
    q.kind = o.kind;
    q.temp_kind = o.temp_kind;
    q.radius = o.radius;
    q.R2 = o.radius * o.radius;
    q.cx = o.center[0];
    q.cy = o.center[1];
    q.cz = o.center[2];
    q.temperature = o.temperature;
    q.rin = o.inner_radius;
    q.rout = o.outer_radius;
    q.rin2 = o.inner_radius * o.inner_radius;
    q.rout2 = o.outer_radius * o.outer_radius;
    {
      double cn = std::sqrt(o.center[0] * o.center[0] + o.center[1] * o.center[1] + o.center[2] * o.center[2]);
      double R = std::fabs(o.radius);
      q.shell_lo = (cn - R) * (1.0 - 1e-9) - 1e-9;
      q.shell_hi = (cn + R) * (1.0 + 1e-9) + 1e-9;
      if (!std::isfinite(q.shell_lo) || !std::isfinite(q.shell_hi)) ds.far_ok = 0;
    }
    q.temp_constant = o.temp_constant;
    q.r_isco = o.r_isco;
    q.lut_n = o.lut_n;
    double* lr = nullptr;
    double* lt = nullptr;
    if ((rc = upload(dc, s->lut_r[k].data(), s->lut_r[k].size(), &lr))) return rc;
    if ((rc = upload(dc, s->lut_t[k].data(), s->lut_t[k].size(), &lt))) return rc;
    q.lut_r = lr;
    q.lut_t = lt;
    if (o.kind == GRT_OBJ_VOLUMETRIC_DISC) {  // VolumetricDisc::new (volumetric_disc.rs:43-95)
      dc.vol = true;
      ds.has_vol = 1;
      grt_volumetric_frame(o.axis, q.ax, q.e1, q.e2);
      grt_perlin_permutation(o.perlin_seed, ds.perm[k]);
      q.perm_slot = k;
      q.thickness = o.thickness;
      q.cap_h = o.thickness * 3.0;
      q.m_step = o.march_step_size;
      q.m_max = o.march_max_steps;
      q.m_maxdist = o.march_step_size * (double)o.march_max_steps;
      q.dens_mult = o.density_multiplier;
      q.bref = o.brightness_reference_temperature;
      q.sig_a = o.absorption;
      q.sig_s = o.scattering;
      q.noff = o.noise_offset;
      q.g_fbm = std::exp2(-0.5);
      for (int i = 0; i < 3; ++i) q.ns[i] = o.noise_scale[i];
      q.octaves = o.num_octaves;
      // far-field filter bounds (geodesic.hip vol_far)
      const double corner = std::sqrt(o.outer_radius * o.outer_radius + q.cap_h * q.cap_h);
      q.vol_far_r = 2.0 * corner * (1.0 + 1e-6);
      q.vol_rmax = 1e6 * q.cap_h;
      q.vol_slab_h = q.cap_h * (1.0 + 1e-6) + 1e-12;
      q.vol_h_cut = std::sqrt(std::log(1000.0)) * o.thickness * (1.0 + 1e-6);  // exp(-(h/th)^2) < 0.001 beyond
      q.vol_slab_ok = (q.ax[0] == 0.0 && q.ax[1] == 0.0 && q.ax[2] == 1.0) ? 1 : 0;
      if (!std::isfinite(q.vol_far_r) || !std::isfinite(q.vol_rmax) || !(q.cap_h > 0.0)) {
        q.vol_far_r = HUGE_VAL;
        q.vol_rmax = 0.0;
        q.vol_slab_ok = 0;
      }
    }
    fill_dev_texture(o.texture, q.tex);
    uint32_t* ot = nullptr;
    if ((rc = upload(dc, s->obj_tex[k].rgba.data(), s->obj_tex[k].rgba.size(), &ot))) return rc;
    q.tex.rgba = ot;
  }
  double *bl = nullptr, *bx = nullptr, *sl = nullptr;
  if ((rc = upload(dc, s->bb_log_t.data(), s->bb_log_t.size(), &bl))) return rc;
  if ((rc = upload(dc, s->bb_xyz.data(), s->bb_xyz.size(), &bx))) return rc;
  if ((rc = upload(dc, d.srgb_to_linear, 256, &sl))) return rc;
  ds.bb_log_t = bl;
  ds.bb_xyz = bx;
  ds.bb_n = d.bb_n;
  ds.srgb_lin = sl;
  grt::DevScene* dsp = nullptr;
  if ((rc = upload(dc, &ds, 1, &dsp))) return rc;
  dc.d_scene = dsp;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, (16 + 8 + GRT_MAX_OBJECTS) * sizeof(unsigned long long)));
  dc.allocations.push_back(p);
  HIP_TRY(hipMemset(p, 0, (16 + 8 + GRT_MAX_OBJECTS) * sizeof(unsigned long long)));
  dc.d_counter = (unsigned long long*)p;
  dc.d_stats = dc.d_counter + 1;
  dc.d_march = dc.d_counter + 8;
  HIP_TRY(hipMalloc(&p, 16 * sizeof(unsigned long long)));
  dc.allocations.push_back(p);
  HIP_TRY(hipMemset(p, 0, 16 * sizeof(unsigned long long)));
  dc.d_tail_ctl = (unsigned long long*)p;
  HIP_TRY(hipMalloc(&p, sizeof(grt::HitPool)));
  dc.allocations.push_back(p);
  HIP_TRY(hipMemset(p, 0, sizeof(grt::HitPool)));
  dc.d_pool = (grt::HitPool*)p;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  dc.cus = prop.multiProcessorCount;
  int occ = 0;
  void (*kfn)() = nullptr;
  (void)kfn;
  HIP_TRY(hipEventCreate(&dc.ev0));
  HIP_TRY(hipEventCreate(&dc.ev1));
  HIP_TRY(hipEventCreateWithFlags(&dc.ev_busy, hipEventDisableTiming));
  (void)occ;
  dc.ready.store(true, std::memory_order_release);
  return 0;
}

grt::WorkList rect_worklist(uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols) {
  grt::WorkList wl;
  std::memset(&wl, 0, sizeof(wl));
  wl.row0 = row0;
  wl.col0 = col0;
  wl.rows = rows;
  wl.cols = cols;
  wl.tiles_x = (cols + 7) / 8;
  uint64_t tiles_y = (rows + 7) / 8;
  wl.n_items = (uint64_t)wl.tiles_x * tiles_y * 64;
  return wl;
}

// Step cap of the probe rays (scheduling only).  The pass lasts as long as its capped
// probes (horizon creepers) take to run the cap.  An escaping ray needs about max_radius
// accepted steps at H_MAX = 1 (C4: 15825-15900 for max_radius 15000), so the cap is
// 1.3 x max_radius, which tells them from the long rays.  A Kerr-Schild probe moving
// outward far from the hole ends at once with a key just below the cap (probe_escaped,
// round 5), so for Kerr-Schild the cap no longer has to outlast the escaping rays:
// 0.3 x max_radius (C4: 4,500 steps; C4 shard 2 0.51 -> 0.09 s before the integrate
// kernel, the integrate kernel's own time unchanged, profiles/r05aj, r05ak).  The other
// charts have no such shortcut and keep 1.3 x: with the short cap their escaping probes
// would end capped, keyed by their distance to the horizon, ahead of the long rays.
static uint32_t probe_cap(const grt_scene* s) {
  const double scale = s->desc.geometry == GRT_GEOM_KERR ? 0.3 : 1.3;
  const double c = scale * s->desc.max_radius;
  return c >= (double)PROBE_CAP ? PROBE_CAP : (c <= 4096.0 ? 4096u : (uint32_t)c);
}

// Probe-ordered tile queue (schedule.hip): worth its ~1/64 extra rays when a ray may run
// far longer than an escaping one (max_steps well above the probe cap) over many tiles,
// in the affine-parameter charts.  KerrBL integrates in Mino time, where even captured
// rays take ~1e3 steps (C3: max 1147), and Euclidean rays are straight lines: there the
// probe pass is pure overhead (measured +5% on C3), so automatic mode skips them.
bool schedule_wanted(const grt_scene* s, const grt::WorkList& wl, const Knobs& k) {
  if (wl.pixel_index || k.schedule == 0) return false;
  const uint64_t tiles = wl.n_items / 64;
  if (k.schedule == 1) return tiles > 1;
  const int g = s->desc.geometry;
  return (g == GRT_GEOM_KERR || g == GRT_GEOM_SCHWARZSCHILD) && s->desc.max_steps >= 8ull * PROBE_CAP &&
         tiles >= 1024;
}
// Schwarzschild frames the probe pass is not worth (automatic mode): the tile order from
// each tile's impact parameter instead (impact_key_kernel; no integration, ~0.1 ms).  C2
// one frame alone 1,280-1,282 -> 1,263-1,271 ms; two frames in flight unchanged
// (1,234-1,241 against 1,240 ms), and with the two-ended queue slower (1,253 ms); frames
// identical (profiles/r06x).
bool impact_wanted(const grt_scene* s, const grt::WorkList& wl, const Knobs& k) {
  return !wl.pixel_index && k.schedule == -1 && s->desc.geometry == GRT_GEOM_SCHWARZSCHILD &&
         wl.n_items / 64 >= 1024 && !schedule_wanted(s, wl, k);
}

// The impact-parameter order with the tiles grouped by the sincos case of their rays
// (schedule.hip tile_class; grt_set_class_order): automatic mode where impact_wanted
// holds; forced (1, 2) for any Schwarzschild rectangle of more than one tile that is not
// probe-ordered, whatever grt_set_schedule says.
bool class_order_wanted(const grt_scene* s, const grt::WorkList& wl, const Knobs& k) {
  if (k.class_order == 0 || wl.pixel_index || s->desc.geometry != GRT_GEOM_SCHWARZSCHILD) return false;
  if (k.class_order < 0) return impact_wanted(s, wl, k);
  return wl.n_items / 64 > 1 && !schedule_wanted(s, wl, k);
}

// Enqueue the probe pass and the sort; returns the device tile order in *order.
// quad: the Kerr-Schild probe on quads, -1 automatic, 0 never, 1 always (grt_debug_probe_keys).
// cls (with impact): the composite key, length bucket then sincos class; cls_out / corner_out
// (nullable) receive the device arrays of the tiles' classes and the corner predictions.
int enqueue_tile_order(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, hipStream_t stream,
                       const uint32_t** order, int quad_mode = -1, bool impact = false,
                       const grt::CamTable* ct = nullptr, bool cls = false, const uint8_t** cls_out = nullptr,
                       const float** corner_out = nullptr) {
  const uint32_t tiles_x = wl.tiles_x, tiles_y = (uint32_t)(wl.n_items / 64 / wl.tiles_x);
  const uint64_t n = (uint64_t)tiles_x * tiles_y;
  size_t temp_bytes = 0;
  HIP_TRY(grt::launch_tile_order(nullptr, tiles_x, tiles_y, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 &temp_bytes, stream));
  // the corner grid has (tiles_x + 1)(tiles_y + 1) <= 2 n + 2 entries whatever the frame's shape
  const uint64_t need = 5 * ((n * 4 + 255) & ~255ull) + temp_bytes + 256 + (((2 * n + 2) * 4 + 255) & ~255ull) +
                        ((n + 255) & ~255ull);
  if (n > dc.sched_tiles || !dc.sched_mem) {
    if (dc.sched_mem) {
      (void)hipDeviceSynchronize();
      (void)hipFree(dc.sched_mem);
      dc.sched_mem = nullptr;
    }
    dc.sched_tiles = 0;
    // room for a frame of the same tile count with a larger radix-sort temp
    HIP_TRY(hipMalloc(&dc.sched_mem, need + (need >> 2)));
    dc.sched_tiles = n;
  }
  char* p = (char*)dc.sched_mem;
  auto take = [&](uint64_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~255ull;
    return r;
  };
  uint32_t* probe = (uint32_t*)take(n * 4);
  uint32_t* keys = (uint32_t*)take(n * 4);
  uint32_t* keys_sorted = (uint32_t*)take(n * 4);
  uint32_t* idx = (uint32_t*)take(n * 4);
  uint32_t* ord = (uint32_t*)take(n * 4);
  void* temp = take(temp_bytes);
  float* corner_a = (float*)take((2 * n + 2) * 4);
  uint8_t* tile_cls = (uint8_t*)take(n);
  if (impact) {  // predicted lengths, no probe rays; no key counts as capped
    HIP_TRY(ct ? grt::seq::launch_impact_keys(dc.d_scene, wl, (uint32_t)n, probe, stream, *ct)
               : grt::launch_impact_keys(dc.d_scene, wl, (uint32_t)n, probe, stream));
    if (cls) {
      const uint32_t n_corners = (tiles_x + 1) * (tiles_y + 1);
      HIP_TRY(ct ? grt::seq::launch_class_keys(dc.d_scene, wl, tiles_x + 1, n_corners, corner_a, stream, *ct)
                 : grt::launch_class_keys(dc.d_scene, wl, tiles_x + 1, n_corners, corner_a, stream));
    }
    HIP_TRY(grt::launch_tile_order(probe, tiles_x, tiles_y, 0xffffffffu, keys, keys_sorted, idx, ord, temp, &temp_bytes,
                                   stream, cls ? corner_a : nullptr, cls ? tile_cls : nullptr));
    if (cls_out) *cls_out = tile_cls;
    if (corner_out) *corner_out = corner_a;
    *order = ord;
    return 0;
  }
  const uint32_t cap = probe_cap(s);
  // Kerr-Schild probe rays on quads when they fill at most 2 waves per SIMD that way
  // (probe_quad_kernel: a C4 1/8 shard's 32,768 probes); above that the one-lane probe,
  // whose pass is then bound by its work, not by one probe's latency
  const bool quad = quad_mode > 0 || (quad_mode < 0 && n <= (uint64_t)dc.cus * 128);
  HIP_TRY(ct ? grt::seq::launch_probe(s->desc.geometry, dc.d_scene, wl, (uint32_t)n, cap, probe, quad, stream, *ct)
             : grt::launch_probe(s->desc.geometry, dc.d_scene, wl, (uint32_t)n, cap, probe, quad, stream));
  HIP_TRY(grt::launch_tile_order(probe, tiles_x, tiles_y, cap, keys, keys_sorted, idx, ord, temp, &temp_bytes, stream));
  *order = ord;
  return 0;
}

// Long-ray hand-off of a Kerr-Schild trace (TailList, dev_scene.h): the tail kernel runs
// one block of 4 waves per CU per GRT_TAIL_WAVES, 64 rays per block (a quad each); by
// default the integrate kernel hands off once the queue is drained and no more rays are
// live than the tail kernel integrates at once.  A lane holds at most one ray, so the
// entry arena needs one entry per integrate lane whatever the threshold.
int tail_list(const grt_scene* s, DeviceCopy& dc, uint64_t lanes, long long tail, grt::TailList* tl,
              int* tail_blocks) {
  std::memset(tl, 0, sizeof(*tl));
  *tail_blocks = 0;
  if (s->desc.geometry != GRT_GEOM_KERR || tail == 0) return 0;
  const int blocks = dc.cus * GRT_TAIL_WAVES;
  const uint64_t threshold = tail > 0 ? (uint64_t)tail : (uint64_t)blocks * grt::TAIL_RAYS_PER_BLOCK;
  const uint64_t cap = lanes;
  if (cap > dc.tail_cap) {
    if (dc.tail_mem) {
      (void)hipDeviceSynchronize();
      (void)hipFree(dc.tail_mem);
      dc.tail_mem = nullptr;
    }
    dc.tail_cap = 0;
    HIP_TRY(hipMalloc(&dc.tail_mem, cap * 16 * sizeof(unsigned long long)));
    dc.tail_cap = cap;
  }
  tl->ctl = dc.d_tail_ctl;
  tl->cap = dc.tail_cap;
  tl->threshold = threshold;
  tl->st = dc.tail_mem;
  *tail_blocks = blocks;
  return 0;
}

#if GRT_RAY_TIMES
// Diagnostic builds: the per-ray schedule record of the last trace ([6][n] words,
// geodesic.hip), one process-wide buffer (single-device diagnostics).
unsigned long long* g_rt = nullptr;
uint64_t g_rt_cap = 0, g_rt_n = 0;
uint64_t g_rt_trace = 0, g_rt_only = 0;  // record only trace g_rt_only since grt_debug_ray_times_only (0: each)
int ray_times_reserve(uint64_t n, hipStream_t stream) {
  ++g_rt_trace;
  if (g_rt_only && g_rt_trace != g_rt_only) {  // another trace: it records nothing
    HIP_TRY(hipDeviceSynchronize());          // the recorded kernel may still be running
    HIP_TRY(grt::set_ray_times(nullptr));
    return 0;
  }
  if (n > g_rt_cap) {
    if (g_rt) {
      (void)hipDeviceSynchronize();
      (void)hipFree(g_rt);
    }
    g_rt = nullptr;
    g_rt_cap = 0;
    HIP_TRY(hipMalloc(&g_rt, n * 6 * 8));
    g_rt_cap = n;
  }
  g_rt_n = n;
  HIP_TRY(hipMemsetAsync(g_rt, 0, n * 6 * 8, stream));
  HIP_TRY(grt::set_ray_times(g_rt));
  return 0;
}
#endif

// Enqueue one trace over `wl` on `stream`; counters are zeroed first.
// ct (camera sequences): `wl` is over a stack of frames, each ray takes the camera of its
// frame from the table, and the sequence unit's exact kernels run (geodesic_seq.hip).
// exact (the geometry buffer): the exact kernels whatever grt_set_arithmetic says.
int enqueue_trace(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl_in, const grt::Outputs& o,
                  unsigned long long* d_stats, hipStream_t stream, const grt::CamTable* ct = nullptr,
                  bool exact = false) {
  grt::WorkList wl = wl_in;
  const Knobs k = Knobs::now();
  if (int rc0 = stream_order(dc, stream)) return rc0;
  if (schedule_wanted(s, wl, k)) {
    int rc0 = enqueue_tile_order(s, dc, wl, stream, &wl.tile_order, -1, false, ct);
    if (rc0) return rc0;
    // longest tiles to the priority wave of each SIMD, shortest to the others (WorkList)
    wl.two_ended = (k.two_ended != 0 && wl.n_items < (1ull << 31)) ? 1u : 0u;
  } else if (impact_wanted(s, wl, k) || class_order_wanted(s, wl, k)) {
    int rc0 = enqueue_tile_order(s, dc, wl, stream, &wl.tile_order, -1, true, ct, class_order_wanted(s, wl, k));
    if (rc0) return rc0;
  }
  HIP_TRY(hipMemsetAsync(dc.d_counter, 0, sizeof(unsigned long long), stream));
  if (dc.vol) {  // jobs, cursor; the march passes' cursors
    HIP_TRY(hipMemsetAsync(dc.d_march, 0, 2 * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(dc.d_march + 8, 0, GRT_MAX_OBJECTS * sizeof(unsigned long long), stream));
  }
  int threads = k.threads ? k.threads : 256;
  int blocks = k.blocks_per_cu > 0 ? dc.cus * k.blocks_per_cu
                                   : dc.cus * 2 * grt::integrate_waves(s->desc.geometry, dc.vol);
  // never launch more lanes than there is work for
  uint64_t max_blocks = (wl.n_items + threads - 1) / threads;
  if ((uint64_t)blocks > max_blocks) blocks = (int)std::max<uint64_t>(1, max_blocks);
  uint64_t n_out = wl.pixel_index ? wl.n_items : (uint64_t)wl.rows * wl.cols;
  grt::Workspace ws;
  // the pool starts at its minimum (grt_set_hit_pool_min) and only grows from a trace's
  // measured need: the synchronous calls' re-trace of flagged pixels, grt_hit_pool_reserve
  int rc = ensure_pool(dc, 0);
  if (rc) return rc;
  rc = ensure_workspace(dc, n_out, &ws);
  if (rc) return rc;
  ws.n_live = wl.n_live;
  {  // the pool descriptor changes only when the pool or the workspace arena moved
    const grt::HitPool hp = pool_view(dc);
    if (std::memcmp(&hp, &dc.pool_desc, sizeof(hp)) != 0) {
      HIP_TRY(hipDeviceSynchronize());  // no kernel in flight reads the old one
      HIP_TRY(hipMemcpy(dc.d_pool, &hp, sizeof(hp), hipMemcpyHostToDevice));
      dc.pool_desc = hp;
    }
  }
  ws.pool = dc.d_pool;
  HIP_TRY(hipMemsetAsync(dc.pool_desc.count, 0, sizeof(unsigned long long), stream));
#if GRT_RAY_TIMES
  if ((rc = ray_times_reserve(n_out, stream))) return rc;
#endif
  grt::TailList tl;
  int tail_blocks = 0;
  rc = tail_list(s, dc, blocks * (uint64_t)threads, k.tail, &tl, &tail_blocks);
  if (rc) return rc;
  if (tl.cap) HIP_TRY(hipMemsetAsync(dc.d_tail_ctl, 0, 16 * sizeof(unsigned long long), stream));
  // grt_set_arithmetic(1): the light charts' kernels built with FMA contraction
  // (geodesic_fused.hip); Kerr-Schild always runs the exact ones
  const bool fused = k.arith == 1 && !exact && s->desc.geometry != GRT_GEOM_KERR;
  const auto launch = fused ? grt::fused::launch_trace
                            : (s->desc.geometry == GRT_GEOM_KERR_BL ? grt::kerr_bl::launch_trace : grt::launch_trace);
  // the exact KerrBL kernels are a unit of their own (geodesic_kerr_bl.hip)
  if (ct)  // a camera sequence: always the exact sequence unit
    HIP_TRY(grt::seq::launch_trace(s->desc.geometry, dc.d_scene, wl, ws, o, dc.d_counter, d_stats, blocks, threads,
                                   dc.vol, tl, tail_blocks, stream, *ct));
  else
    HIP_TRY(launch(s->desc.geometry, dc.d_scene, wl, ws, o, dc.d_counter, d_stats, blocks, threads, dc.vol, tl,
                   tail_blocks, stream));
  return stream_done(dc, stream);
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t n) {
    if (n == 0) n = 16;
    HIP_TRY(hipMalloc(&p, n));
    return 0;
  }
};

int validate_desc(const grt_scene_desc* d) {
  if (!d) return fail(-EINVAL, "null scene descriptor");
  if (d->abi_version != GRT_ABI_VERSION) return fail(-EINVAL, "grt_scene_desc ABI version mismatch");
  if (d->geometry < GRT_GEOM_EUCLIDEAN || d->geometry > GRT_GEOM_EUCLIDEAN_SPHERICAL)
    return fail(-EINVAL, "unknown geometry");
  if (d->n_objects > GRT_MAX_OBJECTS) return fail(-EINVAL, "too many objects");
  auto check_tex = [&](const grt_texture_desc& t) -> int {
    if (t.kind == GRT_TEX_BITMAP && (!t.rgba || !t.width || !t.height)) return fail(-EINVAL, "bitmap texture without texels");
    if (t.kind == GRT_TEX_BLACKBODY && (d->bb_n < 2 || !d->bb_log_t || !d->bb_xyz))
      return fail(-EINVAL, "blackbody texture without LUT");
    if (t.kind < GRT_TEX_BITMAP || t.kind > GRT_TEX_BLACKBODY) return fail(-EINVAL, "unknown texture kind");
    return 0;
  };
  int rc;
  if ((rc = check_tex(d->celestial))) return rc;
  for (uint32_t k = 0; k < d->n_objects; ++k) {
    const grt_object_desc& o = d->objects[k];
    if (o.kind != GRT_OBJ_SPHERE && o.kind != GRT_OBJ_DISC && o.kind != GRT_OBJ_VOLUMETRIC_DISC)
      return fail(-EINVAL, "unknown object kind");
    if ((rc = check_tex(o.texture))) return rc;
    if (o.kind != GRT_OBJ_SPHERE && o.temp_kind == GRT_TEMP_KERR_LUT && (o.lut_n < 2 || !o.lut_r || !o.lut_t))
      return fail(-EINVAL, "disc temperature LUT missing");
    if (o.kind == GRT_OBJ_VOLUMETRIC_DISC &&
        (!(o.outer_radius > o.inner_radius) || !(o.thickness > 0.0) || o.march_max_steps == 0 ||
         !(o.march_step_size > 0.0) || !(o.brightness_reference_temperature > 0.0) || !(o.absorption >= 0.0) ||
         !(o.scattering >= 0.0)))
      return fail(-EINVAL, "invalid VolumetricDisc parameters (cli/shared.rs:238-284)");
  }
  if (d->camera.rows <= 0 || d->camera.cols <= 0) return fail(-EINVAL, "camera has no pixels");
  return 0;
}

}  // namespace

namespace grt_host {
void scene_frame_size(const grt_scene* s, int64_t* rows, int64_t* cols) {
  *rows = s->desc.camera.rows;
  *cols = s->desc.camera.cols;
}
}  // namespace grt_host

extern "C" {

int grt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int grt_set_launch_config(int blocks_per_cu, int threads_per_block) {
  if (blocks_per_cu < 0 || threads_per_block < 0 || threads_per_block % 64 != 0 || threads_per_block > 256)
    return fail(-EINVAL, "launch config: threads must be a multiple of 64 and <= 256");
  g_launch.store(((long long)blocks_per_cu << 16) | (threads_per_block ? threads_per_block : 256));
  return 0;
}

int grt_set_tail(long long threshold) {
  if (threshold < -1) return fail(-EINVAL, "tail threshold must be -1 (auto), 0 (off) or a ray count");
  g_tail.store(threshold);
  return 0;
}

int grt_tail_handoffs(grt_scene* scene, int device, uint64_t* handed_off) {
  return grt_tail_report(scene, device, handed_off, nullptr, nullptr, nullptr, 0);
}

int grt_tail_report(grt_scene* scene, int device, uint64_t* handed_off, double timeline_s[3], uint64_t* slot,
                    uint64_t* step, uint64_t capacity) {
  if (!scene || !handed_off) return fail(-EINVAL, "null argument");
  *handed_off = 0;
  if (timeline_s) timeline_s[0] = timeline_s[1] = timeline_s[2] = 0.0;
  DeviceCopy* dcp = find_device(scene, device);
  if (!dcp) return 0;
  DeviceCopy& dc = *dcp;
  std::lock_guard<std::mutex> lock(dc.mu);
  HIP_TRY(hipSetDevice(device));
  unsigned long long v[16];
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(v, dc.d_tail_ctl, sizeof(v), hipMemcpyDeviceToHost));
  *handed_off = v[1];
  if (timeline_s) {  // s_memrealtime ticks at 100 MHz
    auto since = [&](unsigned long long t) { return (t && v[3]) ? (double)(long long)(t - v[3]) * 1e-8 : 0.0; };
    timeline_s[0] = since(v[4]);
    timeline_s[1] = since(v[5]);
    timeline_s[2] = since(v[6]);
  }
  const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(v[1], dc.tail_cap), capacity);
  if (n && dc.tail_mem) {
    if (slot) HIP_TRY(hipMemcpy(slot, dc.tail_mem + 14 * dc.tail_cap, n * 8, hipMemcpyDeviceToHost));
    if (step) HIP_TRY(hipMemcpy(step, dc.tail_mem + 13 * dc.tail_cap, n * 8, hipMemcpyDeviceToHost));
  }
  return 0;
}

#if GRT_RAY_TIMES
// Diagnostic builds only (not in grt_api.h): the probe pass and tile order of a row-band
// shard, without the trace: probe keys (n_tiles) and the queue order (n_tiles).
int grt_debug_probe_order(grt_scene* s, int device, const grt_row_shard* sh, uint32_t* probe_out,
                          uint32_t* order_out, uint64_t n_tiles) {
  if (!s || !sh || !probe_out || !order_out) return fail(-EINVAL, "null argument");
  DeviceCopy* dc;
  int rc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  HIP_TRY(hipSetDevice(device));
  grt::WorkList wl = rect_worklist(0, 0, grt_shard_row_count((uint32_t)s->desc.camera.rows, sh),
                                   (uint32_t)s->desc.camera.cols);
  wl.band_rows = sh->band_rows;
  wl.shard = sh->shard;
  wl.n_shards = sh->n_shards;
  if (wl.n_items / 64 != n_tiles) return fail(-EINVAL, "tile count differs");
  const uint32_t* order = nullptr;
  if ((rc = enqueue_tile_order(s, *dc, wl, nullptr, &order))) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(probe_out, dc->sched_mem, n_tiles * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(order_out, order, n_tiles * 4, hipMemcpyDeviceToHost));
  return 0;
}

// Diagnostic builds only (not in grt_api.h): record the schedule of the k-th trace from
// now on (and of no other), or of every trace (k = 0): C5's supersample chunk is trace 2.
int grt_debug_ray_times_only(uint64_t k) {
  g_rt_only = k;
  g_rt_trace = 0;
  return 0;
}

// Diagnostic builds only (not in grt_api.h): the last trace's per-ray schedule record,
// [6][n] words (start, hand-off, end, hardware place, integrate / tail attempts), and
// the integrate kernel's start (s_memrealtime) in *t0.
int grt_debug_ray_times(grt_scene* scene, int device, uint64_t* out, uint64_t n, uint64_t* t0) {
  if (!scene || !out || !t0) return fail(-EINVAL, "null argument");
  if (n != g_rt_n || !g_rt) return fail(-EINVAL, "ray count differs from the last trace");
  DeviceCopy* dcp = find_device(scene, device);
  if (!dcp) return fail(-EINVAL, "no trace on this device");
  DeviceCopy& dc = *dcp;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, g_rt, n * 6 * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(t0, dc.d_tail_ctl + 3, 8, hipMemcpyDeviceToHost));
  return 0;
}
#endif

// Test hook (not in grt_api.h): the probe keys (probe_kernel / probe_quad_kernel) of a
// row-band shard with the probe forced onto quads (quad = 1) or onto one lane per ray (0),
// or the Schwarzschild impact-parameter keys (quad = 2, impact_key_kernel).
int grt_debug_probe_keys(grt_scene* s, int device, const grt_row_shard* sh, int quad, uint32_t* keys_out,
                         uint64_t n_tiles) {
  if (!s || !sh || !keys_out || quad < 0 || quad > 2) return fail(-EINVAL, "probe keys: bad argument");
  if (quad == 2 && s->desc.geometry != GRT_GEOM_SCHWARZSCHILD) return fail(-EINVAL, "impact keys: Schwarzschild only");
  DeviceCopy* dc;
  int rc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  grt::WorkList wl = rect_worklist(0, 0, grt_shard_row_count((uint32_t)s->desc.camera.rows, sh),
                                   (uint32_t)s->desc.camera.cols);
  wl.band_rows = sh->band_rows;
  wl.shard = sh->shard;
  wl.n_shards = sh->n_shards;
  if (wl.n_items / 64 != n_tiles || wl.n_items % 64 != 0) return fail(-EINVAL, "tile count differs");
  const uint32_t* order = nullptr;
  if ((rc = enqueue_tile_order(s, *dc, wl, nullptr, &order, quad == 2 ? -1 : quad, quad == 2))) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(keys_out, dc->sched_mem, n_tiles * 4, hipMemcpyDeviceToHost));
  return 0;
}

// Test hook (not in grt_api.h): the class-ordered tile queue of a row-band shard as a trace
// with grt_set_class_order(1) builds it, without the trace: the queue order (n_tiles), the
// tiles' sincos classes (n_tiles) and the predictor's pi/2 - theta_f at the corners of the
// tile grid (n_corners = (tiles_x + 1) * (tiles_y + 1)); any output nullable.
int grt_debug_class_order(grt_scene* s, int device, const grt_row_shard* sh, uint32_t* order_out, uint8_t* class_out,
                          float* corner_out, uint64_t n_tiles, uint64_t n_corners) {
  if (!s || !sh) return fail(-EINVAL, "class order: null argument");
  if (s->desc.geometry != GRT_GEOM_SCHWARZSCHILD) return fail(-EINVAL, "class order: Schwarzschild only");
  DeviceCopy* dc;
  int rc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  grt::WorkList wl = rect_worklist(0, 0, grt_shard_row_count((uint32_t)s->desc.camera.rows, sh),
                                   (uint32_t)s->desc.camera.cols);
  wl.band_rows = sh->band_rows;
  wl.shard = sh->shard;
  wl.n_shards = sh->n_shards;
  const uint64_t tiles_y = wl.n_items / 64 / wl.tiles_x;
  if (wl.n_items / 64 != n_tiles || (wl.tiles_x + 1ull) * (tiles_y + 1) != n_corners)
    return fail(-EINVAL, "class order: tile or corner count differs");
  const uint32_t* order = nullptr;
  const uint8_t* cls = nullptr;
  const float* corner = nullptr;
  if ((rc = enqueue_tile_order(s, *dc, wl, nullptr, &order, -1, true, nullptr, true, &cls, &corner))) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (order_out) HIP_TRY(hipMemcpy(order_out, order, n_tiles * 4, hipMemcpyDeviceToHost));
  if (class_out) HIP_TRY(hipMemcpy(class_out, cls, n_tiles, hipMemcpyDeviceToHost));
  if (corner_out) HIP_TRY(hipMemcpy(corner_out, corner, n_corners * 4, hipMemcpyDeviceToHost));
  return 0;
}

// Test hook (not in grt_api.h): the range-free divisions and square root (geodesic.hip
// div_inrange, div2_inrange, div_fx, sqrt_fx) against the compiler's over the exponent
// plane (arith_map_kernel): map[2047 * 2047], zmap[2047], smap[2047] flag bytes.
int grt_debug_arith_map(int device, uint32_t samples, uint64_t seed, uint8_t* map, uint8_t* zmap, uint8_t* smap) {
  if (!map || !zmap || !smap || samples == 0 || samples > 4096) return fail(-EINVAL, "arith map: 1 <= samples <= 4096");
  HIP_TRY(hipSetDevice(device));
  const size_t nm = 2047u * 2047u;
  DevBuf b;
  int rc = b.alloc(nm + 2 * 2047);
  if (rc) return rc;
  uint8_t* d = (uint8_t*)b.p;
  HIP_TRY(hipMemset(d, 0, nm + 2 * 2047));
  HIP_TRY(grt::launch_arith_map(samples, seed, d, d + nm, d + nm + 2047, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(map, d, nm, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(zmap, d + nm, 2047, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(smap, d + nm + 2047, 2047, hipMemcpyDeviceToHost));
  return 0;
}

// Test hook (not in grt_api.h): the seeded reciprocals of the region-B Schwarzschild RHS
// (rcp_seed.h) against the compiler's division on n host tuples (r, radius, a, sin, cos):
// flags[n], one bit per differing quotient (rcp_seed_check_kernel).
int grt_debug_rcp_seed(int device, uint64_t n, const double* tuples, uint8_t* flags) {
  if (!tuples || !flags || n == 0 || n > (1ull << 26)) return fail(-EINVAL, "rcp seed check: 1 <= n <= 2^26");
  HIP_TRY(hipSetDevice(device));
  DevBuf b_t, b_f;
  int rc;
  if ((rc = b_t.alloc(n * 40)) || (rc = b_f.alloc(n))) return rc;
  HIP_TRY(hipMemcpy(b_t.p, tuples, n * 40, hipMemcpyHostToDevice));
  HIP_TRY(grt::launch_rcp_seed_check(n, (const double*)b_t.p, (uint8_t*)b_f.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(flags, b_f.p, n, hipMemcpyDeviceToHost));
  return 0;
}

// Test hook (not in grt_api.h): the render's glibc wrappers as the device units compile
// them, on n host inputs x (pow: x, y; y unused otherwise).  unit 0: geodesic.hip's
// glibc_check_kernel, tables in LDS, blocks of threads_per_block (what grt_set_launch_config
// admits); unit 1: output.hip's opow (fn GLIBC_FN_POW only), tables in constant memory.
// fn, out0[n], out1[n], path[n]: glibc_check.h.  The host counterpart is
// grt_debug_glibc_host (host/glibc_check.cpp).
int grt_debug_glibc_device(int device, int unit, int fn, int threads_per_block, uint64_t n, const double* x,
                           const double* y, double* out0, double* out1, uint8_t* path) {
  if (!x || !out0 || !out1 || !path || n == 0 || n > (1ull << 26)) return fail(-EINVAL, "glibc check: 1 <= n <= 2^26");
  if (unit < 0 || unit > 1 || fn < 0 || fn >= grt::GLIBC_FN_COUNT || (unit == 1 && fn != grt::GLIBC_FN_POW))
    return fail(-EINVAL, "glibc check: unit 0 with fn 0..6, or unit 1 with fn 0 (pow)");
  if (fn == grt::GLIBC_FN_POW && !y) return fail(-EINVAL, "glibc check: pow needs y");
  if (threads_per_block != 64 && threads_per_block != 128 && threads_per_block != 192 && threads_per_block != 256)
    return fail(-EINVAL, "glibc check: 64, 128, 192 or 256 threads per block");
  HIP_TRY(hipSetDevice(device));
  DevBuf b_x, b_y, b_0, b_1, b_p;
  int rc;
  if ((rc = b_x.alloc(n * 8)) || (rc = b_y.alloc(n * 8)) || (rc = b_0.alloc(n * 8)) || (rc = b_1.alloc(n * 8)) ||
      (rc = b_p.alloc(n)))
    return rc;
  HIP_TRY(hipMemcpy(b_x.p, x, n * 8, hipMemcpyHostToDevice));
  if (y) HIP_TRY(hipMemcpy(b_y.p, y, n * 8, hipMemcpyHostToDevice));
  else HIP_TRY(hipMemset(b_y.p, 0, n * 8));
  HIP_TRY(unit == 0 ? grt::launch_glibc_check(fn, threads_per_block, n, (const double*)b_x.p, (const double*)b_y.p,
                                              (double*)b_0.p, (double*)b_1.p, (uint8_t*)b_p.p, nullptr)
                    : grt::launch_opow_check(threads_per_block, n, (const double*)b_x.p, (const double*)b_y.p,
                                             (double*)b_0.p, (double*)b_1.p, (uint8_t*)b_p.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out0, b_0.p, n * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out1, b_1.p, n * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(path, b_p.p, n, hipMemcpyDeviceToHost));
  return 0;
}

// Test hook (not in grt_api.h): the scene's RHS in its range-free and IEEE forms on n
// host states (8 doubles each; KerrBL: e, l_z, q per state in consts), out[16 n], pred[n]
// (rhs_check_kernel).
int grt_debug_rhs_check(grt_scene* s, int device, uint64_t n, const double* states, const double* consts,
                        double* out, uint8_t* pred) {
  if (!s || !states || !out || !pred || n == 0 || n > (1ull << 26)) return fail(-EINVAL, "rhs check: 1 <= n <= 2^26");
  const int g = s->desc.geometry;
  if (g != GRT_GEOM_SCHWARZSCHILD && g != GRT_GEOM_KERR && g != GRT_GEOM_KERR_BL)
    return fail(-EINVAL, "rhs check: Schwarzschild, Kerr-Schild or KerrBL");
  if (g == GRT_GEOM_KERR_BL && !consts) return fail(-EINVAL, "rhs check: KerrBL needs e, l_z, q per state");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  DevBuf b_st, b_c, b_out, b_pred;
  if ((rc = b_st.alloc(n * 64)) || (rc = b_c.alloc(n * 24)) || (rc = b_out.alloc(n * 128)) || (rc = b_pred.alloc(n)))
    return rc;
  HIP_TRY(hipMemcpy(b_st.p, states, n * 64, hipMemcpyHostToDevice));
  if (consts) HIP_TRY(hipMemcpy(b_c.p, consts, n * 24, hipMemcpyHostToDevice));
  HIP_TRY(grt::launch_rhs_check(g, dc->d_scene, (const double*)b_st.p, (const double*)b_c.p, n, (double*)b_out.p,
                                (uint8_t*)b_pred.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, b_out.p, n * 128, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(pred, b_pred.p, n, hipMemcpyDeviceToHost));
  return 0;
}

#if GRT_PATH_COUNT
// Diagnostic builds only (not in grt_api.h): the integrate kernels' path counters since the
// last reset (geodesic.hip path_count): out[28], [k] wave-level, [14 + k] lane-level.
int grt_debug_path_counts(uint64_t* out, int reset) {
  if (!out) return fail(-EINVAL, "null argument");
  HIP_TRY(grt::path_read((unsigned long long*)out, reset != 0));
  return 0;
}
#endif

// Test hook (not in grt_api.h): 0 makes the device copies of scenes created (first rendered)
// afterwards run every division and square root of the RHS in the compiler's IEEE form
// (DevScene::div_fast = 0), so a test can hold the range-free forms to them end to end.
int grt_debug_range_free(int on) {
  if (on != 0 && on != 1) return fail(-EINVAL, "range-free arithmetic: 0 or 1");
  g_range_free.store(on);
  return 0;
}

// Test hook (not in grt_api.h): 0 makes the device copies of scenes created (first rendered)
// afterwards take every attempt of the Schwarzschild integrate kernels with the full RKF
// sums (DevScene::rkf_short = 0), so a test can hold the short sums to them end to end;
// 2 keeps the short attempts and makes every attempt that leaves the quick step take the
// full form after them, which runs the fallback of a missed rkf_short_ok on ordinary rays.
int grt_debug_rkf_short(int on) {
  if (on < 0 || on > 2) return fail(-EINVAL, "short RKF sums: 0, 1 or 2");
  g_rkf_short.store(on);
  return 0;
}

// Test hook (not in grt_api.h): one RKF45 attempt per host state (8 doubles each) at step
// h[i] in the short and the full form (rkf_check_kernel): out_short[9 n] and out_full[9 n]
// hold yn[8] and err_sq, guard[i] whether rkf_short_ok admits the short result.
int grt_debug_rkf_check(grt_scene* s, int device, uint64_t n, const double* states, const double* h,
                        double* out_short, double* out_full, uint8_t* guard) {
  if (!s || !states || !h || !out_short || !out_full || !guard || n == 0 || n > (1ull << 26))
    return fail(-EINVAL, "rkf check: 1 <= n <= 2^26");
  if (s->desc.geometry != GRT_GEOM_SCHWARZSCHILD) return fail(-EINVAL, "rkf check: Schwarzschild only");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  DevBuf b_st, b_h, b_s, b_f, b_g;
  if ((rc = b_st.alloc(n * 64)) || (rc = b_h.alloc(n * 8)) || (rc = b_s.alloc(n * 72)) || (rc = b_f.alloc(n * 72)) ||
      (rc = b_g.alloc(n)))
    return rc;
  HIP_TRY(hipMemcpy(b_st.p, states, n * 64, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_h.p, h, n * 8, hipMemcpyHostToDevice));
  HIP_TRY(grt::launch_rkf_check(dc->d_scene, (const double*)b_st.p, (const double*)b_h.p, n, (double*)b_s.p,
                                (double*)b_f.p, (uint8_t*)b_g.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_short, b_s.p, n * 72, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_full, b_f.p, n * 72, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(guard, b_g.p, n, hipMemcpyDeviceToHost));
  return 0;
}

int grt_set_arithmetic(int mode) {
  if (mode != 0 && mode != 1) return fail(-EINVAL, "arithmetic: 0 (exact) or 1 (fused)");
  g_arith.store(mode);
  return 0;
}

int grt_get_arithmetic(void) { return g_arith.load(); }

int grt_set_two_ended(int on) {
  if (on != 0 && on != 1) return fail(-EINVAL, "two-ended queue: 0 or 1");
  g_two_ended.store(on);
  return 0;
}

int grt_set_class_order(int mode) {
  if (mode < -1 || mode > 2) return fail(-EINVAL, "class order mode must be -1 (auto), 0, 1 or 2");
  g_class_order.store(mode);
  return 0;
}

int grt_get_class_order(void) { return g_class_order.load(); }

int grt_set_schedule(int mode) {
  if (mode < -1 || mode > 1) return fail(-EINVAL, "schedule mode must be -1 (auto), 0 or 1");
  g_schedule.store(mode);
  return 0;
}

int grt_scene_create(const grt_scene_desc* desc, grt_scene** out) {
  if (!out) return fail(-EINVAL, "null output pointer");
  int rc = validate_desc(desc);
  if (rc) return rc;
  grt_scene* s = new grt_scene();
  s->desc = *desc;
  copy_texture(desc->celestial, s->celestial);
  for (uint32_t k = 0; k < desc->n_objects; ++k) {
    const grt_object_desc& o = desc->objects[k];
    copy_texture(o.texture, s->obj_tex[k]);
    if (o.lut_n) {
      s->lut_r[k].assign(o.lut_r, o.lut_r + o.lut_n);
      s->lut_t[k].assign(o.lut_t, o.lut_t + o.lut_n);
    }
  }
  if (desc->bb_n) {
    s->bb_log_t.assign(desc->bb_log_t, desc->bb_log_t + desc->bb_n);
    s->bb_xyz.assign(desc->bb_xyz, desc->bb_xyz + 3 * (size_t)desc->bb_n);
  }
  // the copy owns its arrays now
  s->desc.celestial.rgba = nullptr;
  for (uint32_t k = 0; k < desc->n_objects; ++k) {
    s->desc.objects[k].texture.rgba = nullptr;
    s->desc.objects[k].lut_r = nullptr;
    s->desc.objects[k].lut_t = nullptr;
  }
  s->desc.bb_log_t = nullptr;
  s->desc.bb_xyz = nullptr;
  *out = s;
  return 0;
}

int grt_scene_destroy(grt_scene* s) {
  if (!s) return 0;
  for (int dev = 0; dev < grt_scene::MAX_DEVICES; ++dev) {
    DeviceCopy* dc = s->devices[dev].load(std::memory_order_acquire);
    if (!dc) continue;
    (void)hipSetDevice((int)dev);
    for (void* p : dc->allocations) (void)hipFree(p);
    if (dc->ws_mem) (void)hipFree(dc->ws_mem);
    if (dc->sched_mem) (void)hipFree(dc->sched_mem);
    if (dc->ad_mem) (void)hipFree(dc->ad_mem);
    if (dc->tail_mem) (void)hipFree(dc->tail_mem);
    if (dc->pool_mem) (void)hipFree(dc->pool_mem);
    if (dc->ev0) (void)hipEventDestroy(dc->ev0);
    if (dc->ev1) (void)hipEventDestroy(dc->ev1);
    if (dc->ev_busy) (void)hipEventDestroy(dc->ev_busy);
    delete dc;
  }
  delete s;
  return 0;
}

static int check_rect(const grt_scene* s, uint64_t row0, uint64_t col0, uint64_t rows, uint64_t cols) {
  if (row0 + rows > (uint64_t)s->desc.camera.rows || col0 + cols > (uint64_t)s->desc.camera.cols)
    return fail(-EINVAL, "rectangle outside the camera frame");
  return 0;
}

// Synchronous calls: after the work has finished, whether some trace needed more hit-pool
// records than it had.  If so the pool is grown to that size (*again = true): the call
// traces again, and the deterministic trace then keeps every candidate.
static int pool_check(DeviceCopy& dc, bool* again) {
  unsigned long long need = 0;
  HIP_TRY(hipMemcpy(&need, dc.d_counter + 6, sizeof(need), hipMemcpyDeviceToHost));
  *again = need > dc.pool_cap && dc.pool_cap < POOL_MAX;
  if (*again) return ensure_pool(dc, need + need / 4);
  return 0;
}

// Device outputs of one synchronous trace of n slots (the aux ones when asked for).
struct HostTrace {
  DevBuf xyza, cls, status, x64, steps, stop, hits;
  grt::Outputs o{};
  int alloc(uint64_t n, const grt_aux_out* aux) {
    int rc;
    if ((rc = xyza.alloc(n * 16)) || (rc = cls.alloc(n)) || (rc = status.alloc(n))) return rc;
    if (aux && aux->xyza64 && (rc = x64.alloc(n * 32))) return rc;
    if (aux && aux->steps && (rc = steps.alloc(n * 4))) return rc;
    if (aux && aux->stop_reason && (rc = stop.alloc(n))) return rc;
    if (aux && aux->hits && (rc = hits.alloc(n * 4))) return rc;
    o = grt::Outputs{(float*)xyza.p, (uint8_t*)cls.p, (uint8_t*)status.p, (double*)x64.p, (uint32_t*)steps.p,
                     (uint8_t*)stop.p, (uint32_t*)hits.p};
    return 0;
  }
};

// One trace of `wl` on the null stream, waited for.  Adds its counters to acc ([0..3]
// accepted, attempts, rays, overflows; [4..7] march jobs, samples, noise, emitting
// samples) and its event time to *ms; *need = hit-pool records it asked for.
static int trace_sync(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, const grt::Outputs& o,
                      unsigned long long acc[8], float* ms, unsigned long long* need,
                      const grt::CamTable* ct = nullptr, bool exact = false) {
  hipStream_t st = nullptr;
  HIP_TRY(hipMemsetAsync(dc.d_stats, 0, 4 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(dc.d_march, 0, 8 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(dc.d_counter + 6, 0, sizeof(unsigned long long), st));
  HIP_TRY(hipEventRecord(dc.ev0, st));
  if (int rc = enqueue_trace(s, dc, wl, o, dc.d_stats, st, ct, exact)) return rc;
  HIP_TRY(hipEventRecord(dc.ev1, st));
  HIP_TRY(hipEventSynchronize(dc.ev1));
  unsigned long long h[4], m[8];
  HIP_TRY(hipMemcpy(h, dc.d_stats, sizeof(h), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(m, dc.d_march, sizeof(m), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(need, dc.d_counter + 6, sizeof(*need), hipMemcpyDeviceToHost));
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, dc.ev0, dc.ev1));
  for (int k = 0; k < 4; ++k) acc[k] += h[k];
  acc[4] += m[3];
  acc[5] += m[2];
  acc[6] += m[4];
  acc[7] += m[5];
  *ms += t;
  return 0;
}

// Trace `wl` (n output slots) into device scratch, wait, copy to the host arrays.  When the
// hit pool was too small (the trace asked for more records than it had), only the pixels
// that lost candidates (GRT_FLAG_HIT_OVERFLOW) are traced again, as a pixel list at their
// centres (get_ray_for_offset at (0.5, 0.5) is get_ray_for, camera.rs:338-363), with the
// pool grown once that subset alone does not fit; their outputs replace the flagged ones.
// `offs` (host, nullable): the offsets list wl was built from.  The stats count the work
// done, the re-traced rays included.  ct: a camera sequence (enqueue_trace), `wl` its stack.
static int run_to_host(grt_scene* s, DeviceCopy* dc_, const grt::WorkList& wl, uint64_t n, const grt_offsets* offs,
                       float* xyza_out, uint8_t* class_out, uint8_t* status_out, const grt_aux_out* aux,
                       grt_stats* stats, const grt::CamTable* ct = nullptr) {
  int rc;
  DeviceCopy& dc = *dc_;
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float ms = 0;
  unsigned long long need = 0;
  {
    HostTrace T;
    if ((rc = T.alloc(n, aux)) || (rc = trace_sync(s, dc, wl, T.o, acc, &ms, &need, ct))) return rc;
    HIP_TRY(hipMemcpy(xyza_out, T.xyza.p, n * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(class_out, T.cls.p, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(status_out, T.status.p, n, hipMemcpyDeviceToHost));
    if (T.o.xyza64) HIP_TRY(hipMemcpy(aux->xyza64, T.x64.p, n * 32, hipMemcpyDeviceToHost));
    if (T.o.steps) HIP_TRY(hipMemcpy(aux->steps, T.steps.p, n * 4, hipMemcpyDeviceToHost));
    if (T.o.stop) HIP_TRY(hipMemcpy(aux->stop_reason, T.stop.p, n, hipMemcpyDeviceToHost));
    if (T.o.hits) HIP_TRY(hipMemcpy(aux->hits, T.hits.p, n * 4, hipMemcpyDeviceToHost));
  }
  // the flagged pixels, traced again until none is left (a round either fits or grows the
  // pool to its own subset's need, which the next round's subset cannot exceed)
  for (int round = 0; need > dc.pool_cap && round < 8; ++round) {
    std::vector<uint64_t> lost;
    for (uint64_t k = 0; k < n; ++k)
      if (status_out[k] & GRT_FLAG_HIT_OVERFLOW) lost.push_back(k);
    if (lost.empty()) break;
    if (round > 0) {
      if (dc.pool_cap >= POOL_MAX) break;  // cannot grow: the pixels stay flagged
      if ((rc = ensure_pool(dc, need + need / 4))) return rc;
    }
    const uint64_t m = lost.size();
    std::vector<uint32_t> pix(m);
    std::vector<double> dx(m, 0.5), dy(m, 0.5);
    grt::WorkList wo;
    std::memset(&wo, 0, sizeof(wo));
    wo.col0 = wl.col0;
    wo.cols = wl.cols;
    wo.n_items = m;
    if (offs) {  // an offsets trace: the same (pixel, dx, dy) items
      wo.row0 = wl.row0;
      wo.rows = wl.rows;
      for (uint64_t j = 0; j < m; ++j) {
        pix[j] = offs->pixel_index[lost[j]];
        dx[j] = offs->dx[lost[j]];
        dy[j] = offs->dy[lost[j]];
      }
    } else if (wl.n_shards > 1) {  // a row-band shard: frame rows of the local ones
      wo.row0 = 0;
      wo.rows = (uint32_t)s->desc.camera.rows;
      for (uint64_t j = 0; j < m; ++j) {
        const uint32_t lr = (uint32_t)(lost[j] / wl.cols), c = (uint32_t)(lost[j] % wl.cols);
        pix[j] = grt::shard_frame_row(wl.band_rows, wl.shard, wl.n_shards, lr) * wl.cols + c;
      }
    } else {
      wo.row0 = wl.row0;
      wo.rows = wl.rows;
      for (uint64_t j = 0; j < m; ++j) pix[j] = (uint32_t)lost[j];
    }
    DevBuf b_pix, b_dx, b_dy;
    if ((rc = b_pix.alloc(m * 4)) || (rc = b_dx.alloc(m * 8)) || (rc = b_dy.alloc(m * 8))) return rc;
    HIP_TRY(hipMemcpy(b_pix.p, pix.data(), m * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_dx.p, dx.data(), m * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_dy.p, dy.data(), m * 8, hipMemcpyHostToDevice));
    wo.pixel_index = (const uint32_t*)b_pix.p;
    wo.dx = (const double*)b_dx.p;
    wo.dy = (const double*)b_dy.p;
    HostTrace T;
    acc[3] = 0;  // the overflows of the last round are the ones left
    if ((rc = T.alloc(m, aux)) || (rc = trace_sync(s, dc, wo, T.o, acc, &ms, &need, ct))) return rc;
    std::vector<float> x(m * 4);
    std::vector<uint8_t> c(m), st(m), sp(T.o.stop ? m : 0);
    std::vector<double> x64(T.o.xyza64 ? m * 4 : 0);
    std::vector<uint32_t> ns(T.o.steps ? m : 0), nh(T.o.hits ? m : 0);
    HIP_TRY(hipMemcpy(x.data(), T.xyza.p, m * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c.data(), T.cls.p, m, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st.data(), T.status.p, m, hipMemcpyDeviceToHost));
    if (T.o.xyza64) HIP_TRY(hipMemcpy(x64.data(), T.x64.p, m * 32, hipMemcpyDeviceToHost));
    if (T.o.steps) HIP_TRY(hipMemcpy(ns.data(), T.steps.p, m * 4, hipMemcpyDeviceToHost));
    if (T.o.stop) HIP_TRY(hipMemcpy(sp.data(), T.stop.p, m, hipMemcpyDeviceToHost));
    if (T.o.hits) HIP_TRY(hipMemcpy(nh.data(), T.hits.p, m * 4, hipMemcpyDeviceToHost));
    for (uint64_t j = 0; j < m; ++j) {
      const uint64_t k = lost[j];
      std::memcpy(xyza_out + 4 * k, &x[4 * j], 16);
      class_out[k] = c[j];
      status_out[k] = st[j];
      if (T.o.xyza64) std::memcpy(aux->xyza64 + 4 * k, &x64[4 * j], 32);
      if (T.o.steps) aux->steps[k] = ns[j];
      if (T.o.stop) aux->stop_reason[k] = sp[j];
      if (T.o.hits) aux->hits[k] = nh[j];
    }
  }
  if (stats) {
    stats->accepted_steps = acc[0];
    stats->attempts = acc[1];
    stats->rays = acc[2];
    stats->hit_overflows = acc[3];
    stats->kernel_ms = ms;
    stats->march_jobs = acc[4];
    stats->march_samples = acc[5];
    stats->march_noise_samples = acc[6];
    stats->march_emit_samples = acc[7];
  }
  return 0;
}

int grt_render_pixels_async(grt_scene* s, int device, void* stream, uint32_t row0, uint32_t col0,
                            uint32_t rows, uint32_t cols, float* d_xyza, uint8_t* d_class,
                            uint8_t* d_status, double* d_xyza64, uint32_t* d_steps, uint8_t* d_stop,
                            uint64_t* d_stats) {
  if (!s || !d_xyza || !d_class || !d_status || !d_stats) return fail(-EINVAL, "null argument");
  if (rows == 0 || cols == 0) return 0;
  int rc = check_rect(s, row0, col0, rows, cols);
  if (rc) return rc;
  DeviceCopy* dc;
  rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  grt::WorkList wl = rect_worklist(row0, col0, rows, cols);
  grt::Outputs o{d_xyza, d_class, d_status, d_xyza64, d_steps, d_stop};
  return enqueue_trace(s, *dc, wl, o, (unsigned long long*)d_stats, (hipStream_t)stream);
}

int grt_render_pixels(grt_scene* s, int device, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols,
                      const grt_offsets* offsets, float* xyza_out, uint8_t* class_out, uint8_t* status_out,
                      const grt_aux_out* aux, grt_stats* stats) {
  if (!s || !xyza_out || !class_out || !status_out) return fail(-EINVAL, "null argument");
  int rc = check_rect(s, row0, col0, rows, cols);
  if (rc) return rc;
  DeviceCopy* dc;
  rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  uint64_t n = offsets ? offsets->count : (uint64_t)rows * cols;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return 0;
  grt::WorkList wl;
  DevBuf b_pix, b_dx, b_dy;
  if (offsets) {
    if (!offsets->pixel_index || !offsets->dx || !offsets->dy) return fail(-EINVAL, "incomplete offsets");
    if (cols == 0) return fail(-EINVAL, "offsets need the rectangle width");
    for (uint64_t k = 0; k < n; ++k)
      if (offsets->pixel_index[k] >= (uint64_t)rows * cols) return fail(-EINVAL, "offset pixel outside rectangle");
    std::memset(&wl, 0, sizeof(wl));
    wl.row0 = row0;
    wl.col0 = col0;
    wl.rows = rows;
    wl.cols = cols;
    wl.n_items = n;
    if ((rc = b_pix.alloc(n * 4)) || (rc = b_dx.alloc(n * 8)) || (rc = b_dy.alloc(n * 8))) return rc;
    HIP_TRY(hipMemcpy(b_pix.p, offsets->pixel_index, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_dx.p, offsets->dx, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_dy.p, offsets->dy, n * 8, hipMemcpyHostToDevice));
    wl.pixel_index = (const uint32_t*)b_pix.p;
    wl.dx = (const double*)b_dx.p;
    wl.dy = (const double*)b_dy.p;
  } else {
    wl = rect_worklist(row0, col0, rows, cols);
  }
  return run_to_host(s, dc, wl, n, offsets, xyza_out, class_out, status_out, aux, stats);
}

// Shared body of grt_trace_pixels / grt_trace_rays: a, b are (row, col) or (pos, mom).
static int trace_common(grt_scene* s, int device, uint64_t n, bool camera, const double* a, const double* b,
                        uint64_t capacity, double* steps_out, uint64_t* n_steps, uint8_t* stop_out,
                        uint8_t* status_out) {
  if (!s || !n_steps || !stop_out || !status_out || (n && (!a || !b)) || (capacity && !steps_out))
    return fail(-EINVAL, "null argument");
  if (n == 0) return 0;
  if (capacity > (1ull << 40) / 72 / n) return fail(-EINVAL, "trajectory buffer too large");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  const uint64_t in_bytes = n * 8 * (camera ? 1 : 4);
  DevBuf b_a, b_b, b_steps, b_n, b_stop, b_status;
  if ((rc = b_a.alloc(in_bytes)) || (rc = b_b.alloc(in_bytes)) || (rc = b_steps.alloc(n * capacity * 72)) ||
      (rc = b_n.alloc(n * 8)) || (rc = b_stop.alloc(n)) || (rc = b_status.alloc(n)))
    return rc;
  HIP_TRY(hipMemcpy(b_a.p, a, in_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_b.p, b, in_bytes, hipMemcpyHostToDevice));
  grt::TrajectoryList tl;
  std::memset(&tl, 0, sizeof(tl));
  tl.n = n;
  if (camera) {
    tl.row = (const double*)b_a.p;
    tl.col = (const double*)b_b.p;
  } else {
    tl.pos = (const double*)b_a.p;
    tl.mom = (const double*)b_b.p;
  }
  tl.cap = capacity;
  tl.steps = (double*)b_steps.p;
  tl.n_steps = (uint64_t*)b_n.p;
  tl.stop = (uint8_t*)b_stop.p;
  tl.status = (uint8_t*)b_status.p;
  HIP_TRY(grt::launch_trajectories(s->desc.geometry, dc->d_scene, tl, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  if (capacity) HIP_TRY(hipMemcpy(steps_out, b_steps.p, n * capacity * 72, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_steps, b_n.p, n * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(stop_out, b_stop.p, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(status_out, b_status.p, n, hipMemcpyDeviceToHost));
  return 0;
}

int grt_health_pixels(grt_scene* s, int device, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols,
                      grt_health* out, double* per_ray) {
  if (!s || !out) return fail(-EINVAL, "null argument");
  std::memset(out, 0, sizeof(*out));
  out->n_constants = s->desc.geometry == GRT_GEOM_KERR_BL ? 3u : 2u;
  if ((uint64_t)row0 + rows > (uint64_t)s->desc.camera.rows || (uint64_t)col0 + cols > (uint64_t)s->desc.camera.cols)
    return fail(-EINVAL, "rectangle outside the frame");
  const uint64_t n = (uint64_t)rows * cols;
  if (n == 0) return 0;
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  DevBuf b_out, b_status;
  if ((rc = b_out.alloc(n * 5 * 8)) || (rc = b_status.alloc(n))) return rc;
  grt::WorkList wl = rect_worklist(row0, col0, rows, cols);
  HIP_TRY(grt::launch_health(s->desc.geometry, dc->d_scene, wl, n, (double*)b_out.p, (uint8_t*)b_status.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<double> v(n * 5);
  std::vector<uint8_t> st(n);
  HIP_TRY(hipMemcpy(v.data(), b_out.p, n * 5 * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(st.data(), b_status.p, n, hipMemcpyDeviceToHost));
  // scene.rs:116-124 (error above 1e-10 for every ray) and report_drifts (integrator.rs:176-201,
  // warnings above 1e-4 for the rays whose integration returned Ok)
  for (uint64_t k = 0; k < n; ++k) {
    const double* o = &v[k * 5];
    out->rays++;
    if (!(o[0] < 1e-10)) out->null_violations++;
    out->max_null = std::fmax(out->max_null, o[0]);
    if (st[k] != GRT_OK) {
      out->failed++;
      continue;
    }
    if (o[1] > 1e-4) out->kk_drift_rays++;
    out->max_kk_drift = std::fmax(out->max_kk_drift, o[1]);
    for (uint32_t c = 0; c < out->n_constants; ++c) {
      if (o[2 + c] > 1e-4) out->constant_drift_rays[c]++;
      out->max_constant_drift[c] = std::fmax(out->max_constant_drift[c], o[2 + c]);
    }
  }
  if (per_ray) std::memcpy(per_ray, v.data(), n * 5 * 8);
  return 0;
}

int grt_trace_pixels(grt_scene* s, int device, uint64_t n, const double* rows, const double* cols,
                     uint64_t capacity, double* steps_out, uint64_t* n_steps, uint8_t* stop_out,
                     uint8_t* status_out) {
  return trace_common(s, device, n, true, rows, cols, capacity, steps_out, n_steps, stop_out, status_out);
}

int grt_trace_rays(grt_scene* s, int device, uint64_t n, const double* positions, const double* momenta,
                   uint64_t capacity, double* steps_out, uint64_t* n_steps, uint8_t* stop_out,
                   uint8_t* status_out) {
  return trace_common(s, device, n, false, positions, momenta, capacity, steps_out, n_steps, stop_out,
                      status_out);
}

// ------------------------------------------------------------- adaptive pass ----
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
static int ad_reserve(DeviceCopy& dc, uint64_t bytes) {
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

constexpr uint64_t SUB_CHUNK = 1ull << 21;  // sub-rays per supersample trace launch
std::atomic<uint64_t> g_sub_chunk{SUB_CHUNK};  // grt_set_sub_chunk (tests force several chunks)

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
  // sub_chunk: grt_set_sub_chunk's value, read once per call (the plan and the carve of
  // one call must agree)
  void carve(AdArena& A, uint64_t n_max, uint32_t spa, uint64_t sub_chunk) {
    per = spa * spa;
    chunk_pix = std::max<uint64_t>(1, std::min<uint64_t>(n_max, sub_chunk / per));
    n_chunks = (uint32_t)((n_max + chunk_pix - 1) / chunk_pix);
    cap = chunk_pix * per;
    pix = (uint32_t*)A.take(cap * 4);
    dx = (double*)A.take(cap * 8);
    dy = (double*)A.take(cap * 8);
    xyza = (float*)A.take(cap * 16);
    cls = (uint8_t*)A.take(cap);
    status = (uint8_t*)A.take(cap);
    x64 = (double*)A.take(cap * 32);
    stop = (uint8_t*)A.take(cap);
    steps = (uint32_t*)A.take(cap * 4);
    live = (unsigned long long*)A.take((uint64_t)n_chunks * 8);
  }
};

// supersample (raytracer.rs:320-384) over a selection that lives on the device: entries
// j < *d_count <= n_max of sel_px (pixel index in the rect row0/col0/rows/cols: camera
// ray and jitter hash) and sel_out (index into d_out64).  The sub-rays go through the
// trace in chunks of g_sub_chunk; the integrate / shade kernels read each chunk's live
// count from the device, so nothing waits for the host between the passes.
static int enqueue_supersample(grt_scene* s, DeviceCopy& dc, hipStream_t st, const SuperBufs& B, uint32_t row0,
                        uint32_t col0, uint32_t rows, uint32_t cols, const uint32_t* sel_px, const uint32_t* sel_out,
                        const unsigned long long* d_count, uint32_t spa, double* d_out64, unsigned long long* d_stats,
                        const grt::SubsampleFailures& fails_in, const grt::CamTable* ct = nullptr,
                        uint32_t stack_row0 = 0) {
  grt::SubsampleFailures fails = fails_in;
  fails.ray_stop = B.stop;
  fails.ray_steps = B.steps;
  HIP_TRY(grt::launch_chunk_live(d_count, B.n_chunks, B.chunk_pix, B.per, B.live, st));
  for (uint32_t c = 0; c < B.n_chunks; ++c) {
    const uint64_t base = (uint64_t)c * B.chunk_pix;
    HIP_TRY(grt::launch_make_offsets(sel_px + base, B.chunk_pix, d_count, base, spa, row0, col0, cols, B.pix, B.dx,
                                     B.dy, st));
    grt::WorkList wo;
    std::memset(&wo, 0, sizeof(wo));
    // a camera sequence: the rect is a frame of the stack, stack_row0 its first stacked row
    // (the jitter above hashes the frame's own pixel coordinates, as a frame alone does)
    wo.row0 = row0 + stack_row0;
    wo.col0 = col0;
    wo.rows = rows;
    wo.cols = cols;
    wo.n_items = B.cap;
    wo.pixel_index = B.pix;
    wo.dx = B.dx;
    wo.dy = B.dy;
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

static uint64_t floor_index(uint64_t n) { return (uint64_t)((double)(n - 1) * 0.99); }

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

// The recorded failed sub-samples, sorted by (pixel, stratum): the reference logs them
// from a parallel loop (raytracer.rs:357-362), in no particular order.
static int copy_failures(const grt::SubsampleFailures& f, uint64_t count, uint32_t spa, grt_subsample_failures* out) {
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
  const bool device_floor = supersampled && !cfg->has_minimum_luminance;
  if (supersampled && n > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "section larger than INT_MAX pixels");
  const uint32_t spa = cfg->samples_per_axis;
  const uint64_t sub_chunk = g_sub_chunk.load(std::memory_order_relaxed);
  // plan: section buffers, selection, floor, sort / compaction scratch, sub-ray buffers
  size_t sort_bytes = 0, select_bytes = 0;
  if (device_floor) HIP_TRY(grt::luminance_floor_device(nullptr, 4, n, floor_index(n), nullptr, &sort_bytes, nullptr, 0));
  if (supersampled) HIP_TRY(grt::compact_flags(nullptr, n, nullptr, nullptr, nullptr, &select_bytes, 0));
  // the supersample pass's work order (longest sub-rays first) reads the 1-spp step counts
  const bool ordered = supersampled && !mask_xyza;
  size_t order_bytes = 0;
  if (ordered) HIP_TRY(grt::order_selection(nullptr, nullptr, n, nullptr, w, h, nullptr, nullptr, &order_bytes, 0));
  const uint64_t fail_cap = (failures && failures->pixel && failures->status) ? failures->capacity : 0;
  const bool want_events = fail_cap && failures->stop;
  grt::SubsampleFailures fails{nullptr, nullptr, nullptr, fail_cap};
  uint8_t* b_stop = nullptr;
  uint32_t *b_steps = nullptr, *b_order = nullptr;
  void* b_order_tmp = nullptr;
  auto carve = [&](AdArena& A, float** xyza, uint8_t** cls, uint8_t** status, double** x64, uint8_t** flags,
                   uint32_t** sel, unsigned long long** cnt, double** floor, void** sort, void** select,
                   SuperBufs* B) {
    *xyza = (float*)A.take(n * 16);
    *cls = (uint8_t*)A.take(n);
    *status = (uint8_t*)A.take(n);
    *x64 = (double*)A.take(n * 32);
    if (stop_out) b_stop = (uint8_t*)A.take(n);
    if (steps_out || ordered) b_steps = (uint32_t*)A.take(n * 4);
    if (!supersampled) return;
    if (ordered) {
      b_order = (uint32_t*)A.take(n * 4);
      b_order_tmp = A.take(order_bytes);
    }
    *flags = (uint8_t*)A.take(n);
    *sel = (uint32_t*)A.take(n * 4);
    *cnt = (unsigned long long*)A.take(16);  // [0] selected pixels, [1] failed sub-samples
    *floor = (double*)A.take(8);
    *sort = A.take(sort_bytes);
    *select = A.take(select_bytes);
    if (!mask_xyza) B->carve(A, n, spa, sub_chunk);
    fails.key = (uint64_t*)A.take(fail_cap * 8);
    fails.status = (uint8_t*)A.take(fail_cap);
    if (want_events) {  // NaN / no-terminal-event sub-rays too (scene.rs:178-183, :196-202)
      fails.stop = (uint8_t*)A.take(fail_cap);
      fails.steps = (uint32_t*)A.take(fail_cap * 4);
    }
  };
  float* b_xyza = nullptr;
  uint8_t *b_cls = nullptr, *b_status = nullptr, *b_flags = nullptr;
  double *b_x64 = nullptr, *d_floor = nullptr;
  uint32_t* b_sel = nullptr;
  unsigned long long* d_cnt = nullptr;
  void *b_sort = nullptr, *b_select = nullptr;
  SuperBufs B;
  {
    AdArena plan;
    carve(plan, &b_xyza, &b_cls, &b_status, &b_x64, &b_flags, &b_sel, &d_cnt, &d_floor, &b_sort, &b_select, &B);
    if ((rc = ad_reserve(*dc, plan.off))) return rc;
    AdArena A{(char*)dc->ad_mem, 0};
    carve(A, &b_xyza, &b_cls, &b_status, &b_x64, &b_flags, &b_sel, &d_cnt, &d_floor, &b_sort, &b_select, &B);
  }
  hipStream_t st = nullptr;
  for (bool again = true; again;) {
  HIP_TRY(hipMemsetAsync(dc->d_stats, 0, 4 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(dc->d_march, 0, 8 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(dc->d_counter + 6, 0, sizeof(unsigned long long), st));
  if (supersampled) HIP_TRY(hipMemsetAsync(d_cnt, 0, 16, st));
  HIP_TRY(hipEventRecord(dc->ev0, st));
  grt::WorkList wl = rect_worklist(from_row, from_col, h, w);
  grt::Outputs o{b_xyza, b_cls, b_status, b_x64, b_steps, b_stop};
  if ((rc = enqueue_trace(s, *dc, wl, o, dc->d_stats, st))) return rc;
  if (supersampled) {
    // resolve_minimum_luminance (raytracer.rs:118-129): the exact 99th percentile in
    // f64::total_cmp order, selected on the device from the 1-spp buffer
    if (device_floor)
      HIP_TRY(grt::luminance_floor_device(b_x64 + 1, 4, n, floor_index(n), b_sort, &sort_bytes, d_floor, st));
    grt::AdaptiveParams ap;
    ap.w = w;
    ap.h = h;
    ap.exclude_background_contrast = cfg->exclude_background_contrast;
    ap.min_lum = cfg->minimum_luminance;
    ap.luminance_contrast_threshold = cfg->luminance_contrast_threshold;
    ap.opacity_contrast_threshold = cfg->opacity_contrast_threshold;
    // collect_pixels_to_supersample (:386-458): stencil, then the selected pixels in
    // order by a device stream compaction
    HIP_TRY(grt::launch_select(b_x64, b_cls, ap, device_floor ? d_floor : nullptr, b_flags, st));
    HIP_TRY(grt::compact_flags(b_flags, n, b_sel, d_cnt, b_select, &select_bytes, st));
    if (mask_xyza) {  // raytracer.rs:285-295: paint instead of supersampling
      HIP_TRY(grt::launch_paint(b_sel, n, d_cnt, mask_xyza, b_x64, st));
    } else {
      fails.count = d_cnt + 1;
      HIP_TRY(grt::order_selection(b_sel, d_cnt, n, b_steps, w, h, b_order, b_order_tmp, &order_bytes, st));
      if ((rc = enqueue_supersample(s, *dc, st, B, from_row, from_col, h, w, b_order, b_order, d_cnt, spa, b_x64,
                                    dc->d_stats, fails)))
        return rc;
    }
  }
  HIP_TRY(hipEventRecord(dc->ev1, st));
  HIP_TRY(hipEventSynchronize(dc->ev1));
  if ((rc = pool_check(*dc, &again))) return rc;
  }
  HIP_TRY(hipMemcpy(xyza_out, b_x64, n * 32, hipMemcpyDeviceToHost));
  if (class_out) HIP_TRY(hipMemcpy(class_out, b_cls, n, hipMemcpyDeviceToHost));
  if (status_out) HIP_TRY(hipMemcpy(status_out, b_status, n, hipMemcpyDeviceToHost));
  if (stop_out) HIP_TRY(hipMemcpy(stop_out, b_stop, n, hipMemcpyDeviceToHost));
  if (steps_out) HIP_TRY(hipMemcpy(steps_out, b_steps, n * 4, hipMemcpyDeviceToHost));
  if (supersampled) {
    unsigned long long cnt[2] = {0, 0};
    HIP_TRY(hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    if (n_supersampled) *n_supersampled = cnt[0];
    if (failures) {
      failures->count = cnt[1];
      if (int frc = copy_failures(fails, cnt[1], spa, failures)) return frc;
    }
  }
  if (stats) {
    unsigned long long hs[4];
    HIP_TRY(hipMemcpy(hs, dc->d_stats, sizeof(hs), hipMemcpyDeviceToHost));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, dc->ev0, dc->ev1));
    stats->accepted_steps = hs[0];
    stats->attempts = hs[1];
    stats->rays = hs[2];
    stats->hit_overflows = hs[3];
    stats->kernel_ms = ms;
    unsigned long long m[8];
    HIP_TRY(hipMemcpy(m, dc->d_march, sizeof(m), hipMemcpyDeviceToHost));
    stats->march_jobs = m[3];
    stats->march_samples = m[2];
    stats->march_noise_samples = m[4];
    stats->march_emit_samples = m[5];
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
constexpr uint64_t SEQ_GROUP = 1ull << 22;            // rays per launch group
static std::atomic<uint64_t> g_seq_group{SEQ_GROUP};  // grt_set_sequence_group

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
  const bool device_floor = !cfg->has_minimum_luminance;
  const bool ordered = !mask_xyza;
  const uint32_t spa = cfg->samples_per_axis;
  const uint64_t sub_chunk = g_sub_chunk.load(std::memory_order_relaxed);
  size_t sort_bytes = 0, select_bytes = 0, order_bytes = 0;
  if (device_floor)
    HIP_TRY(grt::luminance_floor_device(nullptr, 4, per, floor_index(per), nullptr, &sort_bytes, nullptr, 0));
  HIP_TRY(grt::compact_flags(nullptr, per, nullptr, nullptr, nullptr, &select_bytes, 0));
  if (ordered)
    HIP_TRY(grt::order_selection(nullptr, nullptr, per, nullptr, cols, rows, nullptr, nullptr, &order_bytes, 0));
  std::vector<grt::SubsampleFailures> fails(kg, grt::SubsampleFailures{nullptr, nullptr, nullptr, 0});
  for (uint32_t f = 0; f < kg && failures; ++f)
    if (failures[f].pixel && failures[f].status) fails[f].cap = failures[f].capacity;
  float* b_xyza = nullptr;
  uint8_t *b_cls = nullptr, *b_status = nullptr, *b_stop = nullptr, *b_flags = nullptr;
  double *b_x64 = nullptr, *d_floor = nullptr;
  uint32_t *b_steps = nullptr, *b_order = nullptr, *b_sel = nullptr;
  unsigned long long* d_cnt = nullptr;  // per frame: [0] selected pixels, [1] failed sub-samples
  void *b_order_tmp = nullptr, *b_sort = nullptr, *b_select = nullptr;
  SuperBufs B;
  auto carve = [&](AdArena& A) {
    b_xyza = (float*)A.take(n * 16);
    b_cls = (uint8_t*)A.take(n);
    b_status = (uint8_t*)A.take(n);
    b_x64 = (double*)A.take(n * 32);
    b_stop = (uint8_t*)A.take(n);
    b_steps = (uint32_t*)A.take(n * 4);
    if (ordered) {
      b_order = (uint32_t*)A.take(per * 4);
      b_order_tmp = A.take(order_bytes);
    }
    b_flags = (uint8_t*)A.take(per);
    b_sel = (uint32_t*)A.take(per * 4);
    d_cnt = (unsigned long long*)A.take(16ull * kg);
    d_floor = (double*)A.take(8);
    b_sort = A.take(sort_bytes);
    b_select = A.take(select_bytes);
    if (!mask_xyza) B.carve(A, per, spa, sub_chunk);
    for (uint32_t f = 0; f < kg; ++f) {
      const bool events = fails[f].cap && failures[f].stop;
      fails[f].key = (uint64_t*)A.take(fails[f].cap * 8);
      fails[f].status = (uint8_t*)A.take(fails[f].cap);
      fails[f].stop = events ? (uint8_t*)A.take(fails[f].cap) : nullptr;
      fails[f].steps = events ? (uint32_t*)A.take(fails[f].cap * 4) : nullptr;
    }
  };
  {
    AdArena plan;
    carve(plan);
    if ((rc = ad_reserve(dc, plan.off))) return rc;
    AdArena A{(char*)dc.ad_mem, 0};
    carve(A);
  }
  hipStream_t st = nullptr;
  hipEvent_t ev_mid = nullptr;
  HIP_TRY(hipEventCreate(&ev_mid));
  struct EvGuard {
    hipEvent_t e;
    ~EvGuard() { (void)hipEventDestroy(e); }
  } guard{ev_mid};
  grt::AdaptiveParams ap;
  ap.w = cols;
  ap.h = rows;
  ap.exclude_background_contrast = cfg->exclude_background_contrast;
  ap._pad = 0;
  ap.min_lum = cfg->minimum_luminance;
  ap.luminance_contrast_threshold = cfg->luminance_contrast_threshold;
  ap.opacity_contrast_threshold = cfg->opacity_contrast_threshold;
  for (bool again = true; again;) {
    HIP_TRY(hipMemsetAsync(dc.d_stats, 0, 4 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(dc.d_march, 0, 8 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(dc.d_counter + 6, 0, sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 16ull * kg, st));
    HIP_TRY(hipEventRecord(dc.ev0, st));
    const grt::WorkList wl = rect_worklist(0, 0, kg * rows, cols);
    const grt::Outputs o{b_xyza, b_cls, b_status, b_x64, b_steps, b_stop};
    if ((rc = enqueue_trace(s, dc, wl, o, dc.d_stats, st, &ct))) return rc;
    HIP_TRY(hipEventRecord(ev_mid, st));
    for (uint32_t f = 0; f < kg; ++f) {
      double* x64 = b_x64 + 4 * per * f;
      unsigned long long* cnt = d_cnt + 2 * f;
      if (device_floor)
        HIP_TRY(grt::luminance_floor_device(x64 + 1, 4, per, floor_index(per), b_sort, &sort_bytes, d_floor, st));
      HIP_TRY(grt::launch_select(x64, b_cls + per * f, ap, device_floor ? d_floor : nullptr, b_flags, st));
      HIP_TRY(grt::compact_flags(b_flags, per, b_sel, cnt, b_select, &select_bytes, st));
      if (mask_xyza) {
        HIP_TRY(grt::launch_paint(b_sel, per, cnt, mask_xyza, x64, st));
      } else {
        grt::SubsampleFailures ff = fails[f];
        ff.count = cnt + 1;
        HIP_TRY(grt::order_selection(b_sel, cnt, per, b_steps + per * f, cols, rows, b_order, b_order_tmp, &order_bytes,
                                     st));
        if ((rc = enqueue_supersample(s, dc, st, B, 0, 0, rows, cols, b_order, b_order, cnt, spa, x64, dc.d_stats, ff,
                                      &ct, f * rows)))
          return rc;
      }
    }
    HIP_TRY(hipEventRecord(dc.ev1, st));
    HIP_TRY(hipEventSynchronize(dc.ev1));
    float t0 = 0, t1 = 0;
    HIP_TRY(hipEventElapsedTime(&t0, dc.ev0, ev_mid));
    HIP_TRY(hipEventElapsedTime(&t1, ev_mid, dc.ev1));
    T->trace_ms += t0;
    T->super_ms += t1;
    unsigned long long hs[4], m[8];
    HIP_TRY(hipMemcpy(hs, dc.d_stats, sizeof(hs), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(m, dc.d_march, sizeof(m), hipMemcpyDeviceToHost));
    if ((rc = pool_check(dc, &again))) return rc;
    if (again) continue;  // as grt_render_section_ex: the counters of the attempt that stands
    for (int k = 0; k < 4; ++k) T->acc[k] += hs[k];
    T->acc[4] += m[3];
    T->acc[5] += m[2];
    T->acc[6] += m[4];
    T->acc[7] += m[5];
  }
  HIP_TRY(hipMemcpy(out.xyza64, b_x64, n * 32, hipMemcpyDeviceToHost));
  if (out.ray_class) HIP_TRY(hipMemcpy(out.ray_class, b_cls, n, hipMemcpyDeviceToHost));
  if (out.status) HIP_TRY(hipMemcpy(out.status, b_status, n, hipMemcpyDeviceToHost));
  if (out.stop) HIP_TRY(hipMemcpy(out.stop, b_stop, n, hipMemcpyDeviceToHost));
  if (out.steps) HIP_TRY(hipMemcpy(out.steps, b_steps, n * 4, hipMemcpyDeviceToHost));
  std::vector<unsigned long long> cnt(2 * (size_t)kg);
  HIP_TRY(hipMemcpy(cnt.data(), d_cnt, 16ull * kg, hipMemcpyDeviceToHost));
  for (uint32_t f = 0; f < kg; ++f) {
    if (n_supersampled) n_supersampled[f] = cnt[2 * f];
    if (failures) {
      failures[f].count = cnt[2 * f + 1];
      if ((rc = copy_failures(fails[f], cnt[2 * f + 1], spa, &failures[f]))) return rc;
    }
  }
  return 0;
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
  uint64_t g = std::max<uint64_t>(1, g_seq_group.load(std::memory_order_relaxed) / per);
  g = std::min<uint64_t>(g, n_cameras);
  g = std::min<uint64_t>(g, std::max<uint64_t>(1, (uint64_t)INT_MAX / per));
  g = std::min<uint64_t>(g, std::max<uint64_t>(1, 0xffffffffull / rows));
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
  std::vector<grt::DevCamera> cams(n_cameras);
  for (uint32_t f = 0; f < n_cameras; ++f) fill_dev_camera(cameras[f], cams[f]);
  DevBuf b_cams;
  if ((rc = b_cams.alloc(n_cameras * sizeof(grt::DevCamera)))) return rc;
  HIP_TRY(hipMemcpy(b_cams.p, cams.data(), n_cameras * sizeof(grt::DevCamera), hipMemcpyHostToDevice));
  SeqTimes T;
  uint32_t launches = 0;
  // 1 spp: run_to_host needs the f32 colour, class and status on the host even when the
  // caller does not ask for them (the re-trace of overflowed pixels reads the status)
  std::vector<float> tmp_xyza;
  std::vector<uint8_t> tmp_cls, tmp_status;
  for (uint32_t f0 = 0; f0 < n_cameras; f0 += (uint32_t)g, ++launches) {
    const uint32_t kg = (uint32_t)std::min<uint64_t>(g, n_cameras - f0);
    const uint64_t n = per * kg, at = per * f0;
    const grt::CamTable ct{(const grt::DevCamera*)b_cams.p + f0, rows, kg};
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
    grt_stats gs;
    std::memset(&gs, 0, sizeof(gs));
    const grt::WorkList wl = rect_worklist(0, 0, kg * rows, cols);
    if ((rc = run_to_host(s, dc, wl, n, nullptr, out->xyza ? out->xyza + 4 * at : tmp_xyza.data(),
                          out->ray_class ? out->ray_class + at : tmp_cls.data(),
                          out->status ? out->status + at : tmp_status.data(), &aux, &gs, &ct)))
      return rc;
    T.acc[0] += gs.accepted_steps;
    T.acc[1] += gs.attempts;
    T.acc[2] += gs.rays;
    T.acc[3] += gs.hit_overflows;
    T.acc[4] += gs.march_jobs;
    T.acc[5] += gs.march_samples;
    T.acc[6] += gs.march_noise_samples;
    T.acc[7] += gs.march_emit_samples;
    T.trace_ms += gs.kernel_ms;
  }
  if (stats) {
    stats->accepted_steps = T.acc[0];
    stats->attempts = T.acc[1];
    stats->rays = T.acc[2];
    stats->hit_overflows = T.acc[3];
    stats->kernel_ms = T.trace_ms + T.super_ms;
    stats->march_jobs = T.acc[4];
    stats->march_samples = T.acc[5];
    stats->march_noise_samples = T.acc[6];
    stats->march_emit_samples = T.acc[7];
  }
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

// ------------------------------------------------------------- row-band shards ----
static int check_shard(const grt_row_shard* sh) {
  if (!sh) return fail(-EINVAL, "null shard");
  if (sh->n_shards == 0 || sh->shard >= sh->n_shards) return fail(-EINVAL, "shard index out of range");
  if (sh->band_rows == 0) return fail(-EINVAL, "band_rows must be >= 1");
  return 0;
}

uint32_t grt_shard_row_count(uint32_t frame_rows, const grt_row_shard* sh) {
  if (!sh || sh->n_shards == 0 || sh->band_rows == 0 || sh->shard >= sh->n_shards) return 0;
  if (sh->n_shards == 1) return frame_rows;
  uint64_t bands = ((uint64_t)frame_rows + sh->band_rows - 1) / sh->band_rows;
  uint64_t mine = bands > sh->shard ? (bands - sh->shard + sh->n_shards - 1) / sh->n_shards : 0;
  if (mine == 0) return 0;
  uint64_t last_band = sh->shard + (mine - 1) * sh->n_shards;
  uint64_t last_rows = std::min<uint64_t>(sh->band_rows, frame_rows - last_band * sh->band_rows);
  return (uint32_t)((mine - 1) * sh->band_rows + last_rows);
}

uint32_t grt_shard_frame_row(uint32_t local_row, const grt_row_shard* sh) {
  if (!sh) return local_row;
  return grt::shard_frame_row(sh->band_rows, sh->shard, sh->n_shards, local_row);
}

static grt::WorkList shard_worklist(const grt_scene* s, const grt_row_shard* sh) {
  uint32_t rows = grt_shard_row_count((uint32_t)s->desc.camera.rows, sh);
  grt::WorkList wl = rect_worklist(0, 0, rows, (uint32_t)s->desc.camera.cols);
  wl.band_rows = sh->band_rows;
  wl.shard = sh->shard;
  wl.n_shards = sh->n_shards;
  return wl;
}

int grt_render_shard(grt_scene* s, int device, const grt_row_shard* sh, float* xyza_out, uint8_t* class_out,
                     uint8_t* status_out, const grt_aux_out* aux, grt_stats* stats) {
  if (!s || !xyza_out || !class_out || !status_out) return fail(-EINVAL, "null argument");
  int rc = check_shard(sh);
  if (rc) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  grt::WorkList wl = shard_worklist(s, sh);
  uint64_t n = (uint64_t)wl.rows * wl.cols;
  if (n == 0) return 0;
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  return run_to_host(s, dc, wl, n, nullptr, xyza_out, class_out, status_out, aux, stats);
}

int grt_set_sub_chunk(uint64_t sub_rays) {
  if (sub_rays > (1ull << 31)) return fail(-EINVAL, "sub-ray chunk larger than 2^31");
  g_sub_chunk.store(sub_rays ? sub_rays : SUB_CHUNK);
  return 0;
}

int grt_set_hit_pool_min(uint64_t records) {
  if (records == 0 || records > POOL_MAX) return fail(-EINVAL, "hit pool minimum must be in [1, 2^31)");
  g_pool_min.store(records);
  return 0;
}

int grt_hit_pool_reserve(grt_scene* s, int device, uint64_t records, uint64_t* capacity) {
  if (!s) return fail(-EINVAL, "null argument");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  if (records == 0) {  // the largest need since the last reset, once the device is idle
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long need = 0;
    HIP_TRY(hipMemcpy(&need, dc->d_counter + 6, sizeof(need), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(dc->d_counter + 6, 0, sizeof(need)));
    records = need + need / 4;
  }
  if (records > POOL_MAX) return fail(-ENOMEM, "hit pool larger than 2^31 records");
  if ((rc = ensure_pool(*dc, records))) return rc;
  if (capacity) *capacity = dc->pool_cap;
  return 0;
}

int grt_render_shard_async(grt_scene* s, int device, void* stream, const grt_row_shard* sh, float* d_xyza,
                           uint8_t* d_class, uint8_t* d_status, double* d_xyza64, uint32_t* d_steps,
                           uint8_t* d_stop, uint64_t* d_stats) {
  if (!s || !d_xyza || !d_class || !d_status || !d_stats) return fail(-EINVAL, "null argument");
  int rc = check_shard(sh);
  if (rc) return rc;
  grt::WorkList wl = shard_worklist(s, sh);
  if ((uint64_t)wl.rows * wl.cols == 0) return 0;
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  grt::Outputs o{d_xyza, d_class, d_status, d_xyza64, d_steps, d_stop};
  return enqueue_trace(s, *dc, wl, o, (unsigned long long*)d_stats, (hipStream_t)stream);
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
  const uint32_t spa = cfg->samples_per_axis;
  const uint64_t sub_chunk = g_sub_chunk.load(std::memory_order_relaxed);
  const uint64_t fail_cap = (failures && failures->pixel && failures->status) ? failures->capacity : 0;
  const bool want_events = fail_cap && failures->stop;
  size_t select_bytes = 0, order_bytes = 0;
  HIP_TRY(grt::compact_flags(nullptr, n_local, nullptr, nullptr, nullptr, &select_bytes, 0));
  const bool ordered = d_local_steps && !sampling_mask_xyza;
  if (ordered)
    HIP_TRY(grt::order_selection(nullptr, nullptr, n_local, nullptr, w, local_rows, nullptr, nullptr, &order_bytes, 0));
  uint8_t* b_flags = nullptr;
  uint32_t *sel_local = nullptr, *sel_frame = nullptr, *sel_order = nullptr;
  unsigned long long* d_cnt = nullptr;
  void *b_select = nullptr, *b_order_tmp = nullptr;
  SuperBufs B;
  grt::SubsampleFailures fails{nullptr, nullptr, nullptr, fail_cap};
  auto carve = [&](AdArena& A) {
    b_flags = (uint8_t*)A.take(n_local);
    sel_local = (uint32_t*)A.take(n_local * 4);
    sel_frame = (uint32_t*)A.take(n_local * 4);
    d_cnt = (unsigned long long*)A.take(16);  // [0] selected pixels, [1] failed sub-samples
    b_select = A.take(select_bytes);
    if (ordered) {
      sel_order = (uint32_t*)A.take(n_local * 4);
      b_order_tmp = A.take(order_bytes);
    }
    if (!sampling_mask_xyza) B.carve(A, n_local, spa, sub_chunk);
    fails.key = (uint64_t*)A.take(fail_cap * 8);
    fails.status = (uint8_t*)A.take(fail_cap);
    if (want_events) {  // NaN / no-terminal-event sub-rays too (scene.rs:178-183, :196-202)
      fails.stop = (uint8_t*)A.take(fail_cap);
      fails.steps = (uint32_t*)A.take(fail_cap * 4);
    }
  };
  {
    AdArena plan;
    carve(plan);
    if ((rc = ad_reserve(*dc, plan.off))) return rc;
    AdArena A{(char*)dc->ad_mem, 0};
    carve(A);
  }
  if ((rc = stream_order(*dc, st))) return rc;
  HIP_TRY(hipMemsetAsync(d_cnt, 0, 16, st));
  // collect_pixels_to_supersample (raytracer.rs:386-458) over this shard's pixels, with
  // the whole frame's 1-spp buffer as the neighbourhood
  grt::AdaptiveParams ap;
  ap.w = w;
  ap.h = frame_rows;
  ap.exclude_background_contrast = cfg->exclude_background_contrast;
  ap.min_lum = min_lum;
  ap.luminance_contrast_threshold = cfg->luminance_contrast_threshold;
  ap.opacity_contrast_threshold = cfg->opacity_contrast_threshold;
  HIP_TRY(grt::launch_select_shard(d_frame_ya, d_frame_class, ap, d_min_lum, sh->band_rows, sh->shard, sh->n_shards,
                                   local_rows, b_flags, st));
  // selected pixels in frame order (shard rows increase with local rows): local index
  // for the output, frame index for the jitter hash and the camera ray
  HIP_TRY(grt::compact_flags(b_flags, n_local, sel_local, d_cnt, b_select, &select_bytes, st));
  if (ordered) {  // longest sub-rays first (the 3 x 3 neighbourhood in the shard's own rows)
    HIP_TRY(grt::order_selection(sel_local, d_cnt, n_local, d_local_steps, w, local_rows, sel_order, b_order_tmp,
                                 &order_bytes, st));
    sel_local = sel_order;
  }
  HIP_TRY(grt::launch_frame_index(sel_local, d_cnt, n_local, w, sh->band_rows, sh->shard, sh->n_shards, sel_frame,
                                  st));
  if (sampling_mask_xyza) {  // raytracer.rs:285-295: paint instead of supersampling
    HIP_TRY(grt::launch_paint(sel_local, n_local, d_cnt, sampling_mask_xyza, d_xyza64, st));
  } else {
    fails.count = d_cnt + 1;
    if ((rc = enqueue_supersample(s, *dc, st, B, 0, 0, frame_rows, w, sel_frame, sel_local, d_cnt, spa, d_xyza64,
                                  (unsigned long long*)d_stats, fails)))
      return rc;
  }
  if (d_n_supersampled) HIP_TRY(hipMemcpyAsync(d_n_supersampled, d_cnt, 8, hipMemcpyDeviceToDevice, st));
  if ((rc = stream_done(*dc, st))) return rc;
  if (failures) {
    unsigned long long cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    failures->count = cnt[1];
    if ((rc = copy_failures(fails, cnt[1], spa, failures))) return rc;
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
  if (b.p) (void)hipFree(b.p);
  b.p = p;
  return 0;
}

// The sub-sample set of a buffer (grt_api.h): append-only, capacities grow geometrically.
// Block b holds the per sub-rays of pixel sub_pixel[b] at rays [b * per, (b + 1) * per).
struct GBufferSub {
  uint32_t spa = 0;  // 0: no set
  uint64_t n_pix = 0, cap_pix = 0, n_layers = 0, cap_layers = 0;
  DevBuf sub_pixel;  // u32[cap_pix]
  DevBuf sub_block;  // u32[n_pixels], GBUFFER_NIL where a pixel has no block (derived, never stored)
  std::vector<uint32_t> h_block;  // host copy of sub_block
  DevBuf status, stop, steps, sky_u, sky_v, sky_z, layer_start, object, u, v, z, radius;
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
    const uint64_t cap = std::max<uint64_t>({want, 2 * cap_pix, 1024}), p = per(), r0 = n_rays(), r1 = cap * p;
    int rc;
    if ((rc = grow_buf(sub_pixel, 4 * n_pix, 4 * cap)) || (rc = grow_buf(status, r0, r1)) ||
        (rc = grow_buf(stop, r0, r1)) || (rc = grow_buf(steps, 4 * r0, 4 * r1)) ||
        (rc = grow_buf(sky_u, 8 * r0, 8 * r1)) || (rc = grow_buf(sky_v, 8 * r0, 8 * r1)) ||
        (rc = grow_buf(sky_z, 8 * r0, 8 * r1)))
      return rc;
    const bool first = layer_start.p == nullptr;
    if ((rc = grow_buf(layer_start, first ? 0 : 8 * (r0 + 1), 8 * (r1 + 1)))) return rc;
    if (first) HIP_TRY(hipMemset(layer_start.p, 0, 8));
    cap_pix = cap;
    return 0;
  }
  int reserve_layers(uint64_t want) {
    if (want <= cap_layers && object.p) return 0;
    const uint64_t cap = std::max<uint64_t>({want, 2 * cap_layers, 4096}), l = n_layers;
    int rc;
    if ((rc = grow_buf(object, l, cap)) || (rc = grow_buf(u, 8 * l, 8 * cap)) || (rc = grow_buf(v, 8 * l, 8 * cap)) ||
        (rc = grow_buf(z, 8 * l, 8 * cap)) || (rc = grow_buf(radius, 8 * l, 8 * cap)))
      return rc;
    cap_layers = cap;
    return 0;
  }
  // the rays from `first_ray` on (layer offsets stay the set's own)
  grt::GBufferArrays view(uint64_t first_ray, uint64_t n) const {
    return grt::GBufferArrays{n,
                              (const uint8_t*)status.p + first_ray,
                              (const uint8_t*)stop.p + first_ray,
                              (const uint64_t*)layer_start.p + first_ray,
                              (double*)sky_u.p + first_ray,
                              (double*)sky_v.p + first_ray,
                              (double*)sky_z.p + first_ray,
                              (uint8_t*)object.p,
                              (double*)u.p,
                              (double*)v.p,
                              (double*)z.p,
                              (double*)radius.p};
  }
};

struct grt_gbuffer {
  grt_gbuffer_info info;
  double times[2] = {0.0, 0.0};  // trace, scan + fill (ms)
  DevBuf status, stop, steps, sky_u, sky_v, sky_z, layer_start, object, u, v, z, radius;
  GBufferSub sub;
  grt_gbuffer() { std::memset(&info, 0, sizeof(info)); }
  int alloc_pixels() {
    const uint64_t n = info.n_pixels;
    int rc;
    if ((rc = status.alloc(n)) || (rc = stop.alloc(n)) || (rc = steps.alloc(4 * n)) || (rc = sky_u.alloc(8 * n)) ||
        (rc = sky_v.alloc(8 * n)) || (rc = sky_z.alloc(8 * n)) || (rc = layer_start.alloc(8 * (n + 1))))
      return rc;
    return 0;
  }
  int alloc_layers() {
    const uint64_t l = info.n_layers;
    int rc;
    if ((rc = object.alloc(l)) || (rc = u.alloc(8 * l)) || (rc = v.alloc(8 * l)) || (rc = z.alloc(8 * l)) ||
        (rc = radius.alloc(8 * l)))
      return rc;
    return 0;
  }
  grt::GBufferArrays view() const {
    return grt::GBufferArrays{info.n_pixels,      (const uint8_t*)status.p, (const uint8_t*)stop.p,
                              (const uint64_t*)layer_start.p, (double*)sky_u.p, (double*)sky_v.p,
                              (double*)sky_z.p,   (uint8_t*)object.p,       (double*)u.p,
                              (double*)v.p,       (double*)z.p,             (double*)radius.p};
  }
};

extern "C" {

int grt_gbuffer_trace(grt_scene* s, int device, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols,
                      grt_gbuffer** out, grt_stats* stats) {
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
  grt_gbuffer_shape_of(&s->desc, &info.shape);
  info.camera = s->desc.camera;
  info.max_steps = s->desc.max_steps;
  info.max_radius = s->desc.max_radius;
  info.step_size = s->desc.step_size;
  info.epsilon = s->desc.epsilon;
  info.horizon_epsilon = s->desc.horizon_epsilon;
  if ((rc = gb->alloc_pixels())) return rc;
  // the trace's other outputs, and the scan's scratch
  DevBuf xyza, cls, hits, counts, temp;
  if ((rc = xyza.alloc(16 * n)) || (rc = cls.alloc(n)) || (rc = hits.alloc(4 * n)) || (rc = counts.alloc(8 * (n + 1))))
    return rc;
  size_t temp_bytes = 0;
  HIP_TRY(grt::gbuffer_layer_scan(nullptr, nullptr, n, nullptr, nullptr, nullptr, &temp_bytes, nullptr));
  if ((rc = temp.alloc(temp_bytes))) return rc;
  const grt::WorkList wl = rect_worklist(row0, col0, rows, cols);
  const grt::Outputs o{(float*)xyza.p,          (uint8_t*)cls.p,         (uint8_t*)gb->status.p, nullptr,
                       (uint32_t*)gb->steps.p,  (uint8_t*)gb->stop.p,    (uint32_t*)hits.p};
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float ms = 0;
  // the whole rectangle again while a trace loses candidates: the workspace and pool the
  // fill reads must be one complete trace's
  for (int traces = 1;; ++traces) {
    unsigned long long need = 0;
    acc[3] = 0;
    if ((rc = trace_sync(s, *dc, wl, o, acc, &ms, &need, nullptr, true))) return rc;
    if (acc[3] == 0) break;
    if (traces == 3 || dc->pool_cap >= POOL_MAX)
      return fail(-ENOMEM, "the hit pool still overflows after " + std::to_string(traces) + " traces");
    if ((rc = ensure_pool(*dc, need + need / 4))) return rc;
  }
  hipStream_t st = nullptr;
  if ((rc = stream_order(*dc, st))) return rc;
  HIP_TRY(hipEventRecord(dc->ev0, st));
  HIP_TRY(grt::gbuffer_layer_scan((const uint8_t*)gb->status.p, (const uint32_t*)hits.p, n, (uint64_t*)counts.p,
                                  (uint64_t*)gb->layer_start.p, temp.p, &temp_bytes, st));
  uint64_t n_layers = 0;
  HIP_TRY(hipMemcpy(&n_layers, (const uint64_t*)gb->layer_start.p + n, 8, hipMemcpyDeviceToHost));
  info.n_layers = n_layers;
  if ((rc = gb->alloc_layers())) return rc;
  grt::Workspace ws;
  if ((rc = ensure_workspace(*dc, n, &ws))) return rc;  // the carving of the trace above
  ws.pool = dc->d_pool;
  const auto fill = s->desc.geometry == GRT_GEOM_KERR_BL ? grt::kerr_bl::launch_gbuffer_fill : grt::launch_gbuffer_fill;
  HIP_TRY(fill(s->desc.geometry, dc->d_scene, wl, ws, gb->view(), st));
  HIP_TRY(hipEventRecord(dc->ev1, st));
  HIP_TRY(hipEventSynchronize(dc->ev1));
  float fill_ms = 0;
  HIP_TRY(hipEventElapsedTime(&fill_ms, dc->ev0, dc->ev1));
  if ((rc = stream_done(*dc, st))) return rc;
  gb->times[0] = ms;
  gb->times[1] = fill_ms;
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->accepted_steps = acc[0];
    stats->attempts = acc[1];
    stats->rays = acc[2];
    stats->kernel_ms = ms;
  }
  *out = gb.release();
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
  if (!gb || !h || !h->status || !h->stop || !h->steps || !h->sky_u || !h->sky_v || !h->sky_redshift ||
      !h->layer_start)
    return fail(-EINVAL, "null argument");
  const uint64_t n = gb->info.n_pixels, l = gb->info.n_layers;
  if (l && (!h->object || !h->u || !h->v || !h->redshift || !h->radius)) return fail(-EINVAL, "null layer array");
  HIP_TRY(hipSetDevice(gb->info.device));
  HIP_TRY(hipMemcpy(h->status, gb->status.p, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->stop, gb->stop.p, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->steps, gb->steps.p, 4 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->sky_u, gb->sky_u.p, 8 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->sky_v, gb->sky_v.p, 8 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->sky_redshift, gb->sky_z.p, 8 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->layer_start, gb->layer_start.p, 8 * (n + 1), hipMemcpyDeviceToHost));
  if (l) {
    HIP_TRY(hipMemcpy(h->object, gb->object.p, l, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->u, gb->u.p, 8 * l, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->v, gb->v.p, 8 * l, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->redshift, gb->z.p, 8 * l, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->radius, gb->radius.p, 8 * l, hipMemcpyDeviceToHost));
  }
  return 0;
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
  if ((rc = gb->alloc_pixels()) || (rc = gb->alloc_layers())) return rc;
  HIP_TRY(hipMemcpy(gb->status.p, h->status, n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(gb->stop.p, h->stop, n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(gb->steps.p, h->steps, 4 * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(gb->sky_u.p, h->sky_u, 8 * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(gb->sky_v.p, h->sky_v, 8 * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(gb->sky_z.p, h->sky_redshift, 8 * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(gb->layer_start.p, h->layer_start, 8 * (n + 1), hipMemcpyHostToDevice));
  if (l) {
    HIP_TRY(hipMemcpy(gb->object.p, h->object, l, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(gb->u.p, h->u, 8 * l, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(gb->v.p, h->v, 8 * l, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(gb->z.p, h->redshift, 8 * l, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(gb->radius.p, h->radius, 8 * l, hipMemcpyHostToDevice));
  }
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
int gbuffer_sequence_group(grt_scene* s, DeviceCopy& dc, int device, const grt::CamTable& ct,
                           const grt_camera_desc* cameras, uint32_t rows, uint32_t cols,
                           std::vector<std::unique_ptr<grt_gbuffer>>& made, GbSeqTimes* T) {
  int rc;
  const uint32_t kg = ct.n_cams;
  const uint64_t per = (uint64_t)rows * cols, n = per * kg;
  DevBuf status, stop, steps, sky_u, sky_v, sky_z, layer_start, xyza, cls, hits, counts, temp;
  if ((rc = status.alloc(n)) || (rc = stop.alloc(n)) || (rc = steps.alloc(4 * n)) || (rc = sky_u.alloc(8 * n)) ||
      (rc = sky_v.alloc(8 * n)) || (rc = sky_z.alloc(8 * n)) || (rc = layer_start.alloc(8 * (n + 1))) ||
      (rc = xyza.alloc(16 * n)) || (rc = cls.alloc(n)) || (rc = hits.alloc(4 * n)) || (rc = counts.alloc(8 * (n + 1))))
    return rc;
  size_t temp_bytes = 0;
  HIP_TRY(grt::gbuffer_layer_scan(nullptr, nullptr, n, nullptr, nullptr, nullptr, &temp_bytes, nullptr));
  if ((rc = temp.alloc(temp_bytes))) return rc;
  const grt::WorkList wl = rect_worklist(0, 0, kg * rows, cols);
  const grt::Outputs o{(float*)xyza.p,     (uint8_t*)cls.p,  (uint8_t*)status.p, nullptr,
                       (uint32_t*)steps.p, (uint8_t*)stop.p, (uint32_t*)hits.p};
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float ms = 0;
  // the whole group again while its trace loses candidates (grt_gbuffer_trace)
  for (int traces = 1;; ++traces) {
    unsigned long long need = 0;
    acc[3] = 0;
    ++T->traces;
    if ((rc = trace_sync(s, dc, wl, o, acc, &ms, &need, &ct, true))) return rc;
    if (acc[3] == 0) break;
    if (traces == 3 || dc.pool_cap >= POOL_MAX)
      return fail(-ENOMEM, "the hit pool still overflows after " + std::to_string(traces) + " traces");
    if ((rc = ensure_pool(dc, need + need / 4))) return rc;
  }
  hipStream_t st = nullptr;
  if ((rc = stream_order(dc, st))) return rc;
  HIP_TRY(hipEventRecord(dc.ev0, st));
  HIP_TRY(grt::gbuffer_layer_scan((const uint8_t*)status.p, (const uint32_t*)hits.p, n, (uint64_t*)counts.p,
                                  (uint64_t*)layer_start.p, temp.p, &temp_bytes, st));
  // where each frame's layers begin in the stack's, and the total
  std::vector<uint64_t> base(kg + 1);
  for (uint32_t f = 0; f <= kg; ++f)
    HIP_TRY(hipMemcpy(&base[f], (const uint64_t*)layer_start.p + per * f, 8, hipMemcpyDeviceToHost));
  const uint64_t total = base[kg];
  DevBuf object, u, v, z, radius;
  if ((rc = object.alloc(total)) || (rc = u.alloc(8 * total)) || (rc = v.alloc(8 * total)) ||
      (rc = z.alloc(8 * total)) || (rc = radius.alloc(8 * total)))
    return rc;
  grt::Workspace ws;
  if ((rc = ensure_workspace(dc, n, &ws))) return rc;  // the carving of the trace above
  ws.pool = dc.d_pool;
  const grt::GBufferArrays stack{n,
                                 (const uint8_t*)status.p,
                                 (const uint8_t*)stop.p,
                                 (const uint64_t*)layer_start.p,
                                 (double*)sky_u.p,
                                 (double*)sky_v.p,
                                 (double*)sky_z.p,
                                 (uint8_t*)object.p,
                                 (double*)u.p,
                                 (double*)v.p,
                                 (double*)z.p,
                                 (double*)radius.p};
  HIP_TRY(grt::seq::launch_gbuffer_fill(s->desc.geometry, dc.d_scene, wl, ws, stack, st, ct));
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
    grt_gbuffer_shape_of(&s->desc, &info.shape);
    info.camera = cameras[f];
    info.max_steps = s->desc.max_steps;
    info.max_radius = s->desc.max_radius;
    info.step_size = s->desc.step_size;
    info.epsilon = s->desc.epsilon;
    info.horizon_epsilon = s->desc.horizon_epsilon;
    if ((rc = gb->alloc_pixels()) || (rc = gb->alloc_layers())) return rc;
    const uint64_t p0 = per * f, l0 = base[f], nl = info.n_layers;
    auto cut = [&](DevBuf& dst, const DevBuf& src, uint64_t at, uint64_t count, uint64_t size) {
      return count ? hipMemcpyAsync(dst.p, (const char*)src.p + at * size, count * size, hipMemcpyDeviceToDevice, st)
                   : hipSuccess;
    };
    HIP_TRY(cut(gb->status, status, p0, per, 1));
    HIP_TRY(cut(gb->stop, stop, p0, per, 1));
    HIP_TRY(cut(gb->steps, steps, p0, per, 4));
    HIP_TRY(cut(gb->sky_u, sky_u, p0, per, 8));
    HIP_TRY(cut(gb->sky_v, sky_v, p0, per, 8));
    HIP_TRY(cut(gb->sky_z, sky_z, p0, per, 8));
    HIP_TRY(cut(gb->object, object, l0, nl, 1));
    HIP_TRY(cut(gb->u, u, l0, nl, 8));
    HIP_TRY(cut(gb->v, v, l0, nl, 8));
    HIP_TRY(cut(gb->z, z, l0, nl, 8));
    HIP_TRY(cut(gb->radius, radius, l0, nl, 8));
    HIP_TRY(grt::gbuffer_rebase((const uint64_t*)layer_start.p + p0, per, (uint64_t*)gb->layer_start.p, st));
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
  uint64_t g = std::max<uint64_t>(1, g_seq_group.load(std::memory_order_relaxed) / per);
  g = std::min<uint64_t>(g, n_cameras);
  g = std::min<uint64_t>(g, std::max<uint64_t>(1, ((uint64_t)INT_MAX - 1) / per));
  g = std::min<uint64_t>(g, std::max<uint64_t>(1, 0xffffffffull / rows));
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  std::vector<grt::DevCamera> cams(n_cameras);
  for (uint32_t f = 0; f < n_cameras; ++f) fill_dev_camera(cameras[f], cams[f]);
  DevBuf b_cams;
  if ((rc = b_cams.alloc(n_cameras * sizeof(grt::DevCamera)))) return rc;
  HIP_TRY(hipMemcpy(b_cams.p, cams.data(), n_cameras * sizeof(grt::DevCamera), hipMemcpyHostToDevice));
  // the buffers die with `made` on any failure below
  std::vector<std::unique_ptr<grt_gbuffer>> made;
  made.reserve(n_cameras);
  GbSeqTimes T;
  uint32_t launches = 0;
  for (uint32_t f0 = 0; f0 < n_cameras; f0 += (uint32_t)g, ++launches) {
    const uint32_t kg = (uint32_t)std::min<uint64_t>(g, n_cameras - f0);
    const grt::CamTable ct{(const grt::DevCamera*)b_cams.p + f0, rows, kg};
    if ((rc = gbuffer_sequence_group(s, *dc, device, ct, cameras + f0, rows, cols, made, &T))) return rc;
  }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->accepted_steps = T.acc[0];
    stats->attempts = T.acc[1];
    stats->rays = T.acc[2];
    stats->kernel_ms = T.trace_ms;
  }
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
  for (uint32_t f = 0; f < n_buffers; ++f)
    if (!buffers[f]) return fail(-EINVAL, "frame " + std::to_string(f) + ": null buffer");
  const grt_gbuffer_info& i0 = buffers[0]->info;
  const int device = i0.device;
  for (uint32_t f = 0; f < n_buffers; ++f) {
    const grt_gbuffer_info& i = buffers[f]->info;
    if (i.device != device)
      return fail(-EINVAL, "frame " + std::to_string(f) + ": the g-buffer is on device " + std::to_string(i.device) +
                               ", frame 0's on device " + std::to_string(device));
    if (i.rows != i0.rows || i.cols != i0.cols)
      return fail(-EINVAL, "frame " + std::to_string(f) + ": the g-buffer has " + std::to_string(i.rows) + " x " +
                               std::to_string(i.cols) + " pixels, frame 0's " + std::to_string(i0.rows) + " x " +
                               std::to_string(i0.cols));
    if (int rc = grt_gbuffer_shape_compatible(&i.shape, &s->desc))
      return fail(rc, "frame " + std::to_string(f) + ": " + grt_last_error());
  }
  const uint64_t per = i0.n_pixels;
  if (per == 0 || per > (uint64_t)INT_MAX) return fail(-EINVAL, "frames of 0 or more than INT_MAX pixels");
  uint64_t g = std::max<uint64_t>(1, g_seq_group.load(std::memory_order_relaxed) / per);
  g = std::min<uint64_t>(g, n_buffers);
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  const uint64_t ng = per * g;  // slots of a full group
  DevBuf xyza, cls, status, x64, stop, steps, table;
  if ((rc = xyza.alloc(16 * ng)) || (rc = cls.alloc(ng)) || (rc = status.alloc(ng))) return rc;
  if (out->xyza64 && (rc = x64.alloc(32 * ng))) return rc;
  if (out->stop && (rc = stop.alloc(ng))) return rc;
  if (out->steps && (rc = steps.alloc(4 * ng))) return rc;
  std::vector<grt::GBufferFrame> frames(n_buffers);
  for (uint32_t f = 0; f < n_buffers; ++f) frames[f] = grt::GBufferFrame{buffers[f]->view(), (const uint32_t*)buffers[f]->steps.p};
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
// The sub-rays of a buffer belong to the frame it holds: the tracer's geometry (shape key),
// camera and integration parameters must be the recorded ones.
static int check_tracer(const grt_gbuffer* gb, const grt_scene* t) {
  if (int rc = grt_gbuffer_shape_compatible(&gb->info.shape, &t->desc)) return rc;
  auto differs = [](const char* field) {
    return fail(-EINVAL, std::string("g-buffer: the tracer differs from the traced scene in ") + field);
  };
  const grt_gbuffer_info& i = gb->info;
  if (std::memcmp(&i.camera, &t->desc.camera, sizeof(i.camera)) != 0) return differs("camera");
  if (i.max_steps != t->desc.max_steps) return differs("max_steps");
  if (std::memcmp(&i.max_radius, &t->desc.max_radius, 8) != 0) return differs("max_radius");
  if (std::memcmp(&i.step_size, &t->desc.step_size, 8) != 0) return differs("step_size");
  if (std::memcmp(&i.epsilon, &t->desc.epsilon, 8) != 0) return differs("epsilon");
  if (std::memcmp(&i.horizon_epsilon, &t->desc.horizon_epsilon, 8) != 0) return differs("horizon_epsilon");
  return 0;
}

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
static int sub_fill(grt_scene* tracer, grt_gbuffer* gb, uint32_t spa, const std::vector<uint32_t>& px,
                    unsigned long long acc[8], double ms[2]) {
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
  const uint64_t per = S.per();
  if ((S.n_pix + m) * per + 1 > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "more than INT_MAX - 1 sub-rays");
  const uint64_t chunk_pix = std::max<uint64_t>(1, std::min<uint64_t>(m, g_sub_chunk.load(std::memory_order_relaxed) / per));
  const uint64_t cap = chunk_pix * per;
  DevBuf d_px, pix, dx, dy, xyza, cls, hits, counts, local, temp;
  if ((rc = d_px.alloc(4 * m)) || (rc = pix.alloc(4 * cap)) || (rc = dx.alloc(8 * cap)) || (rc = dy.alloc(8 * cap)) ||
      (rc = xyza.alloc(16 * cap)) || (rc = cls.alloc(cap)) || (rc = hits.alloc(4 * cap)) ||
      (rc = counts.alloc(8 * (cap + 1))) || (rc = local.alloc(8 * (cap + 1))))
    return rc;
  size_t temp_bytes = 0;
  HIP_TRY(grt::gbuffer_layer_scan(nullptr, nullptr, cap, nullptr, nullptr, nullptr, &temp_bytes, nullptr));
  if ((rc = temp.alloc(temp_bytes))) return rc;
  HIP_TRY(hipMemcpy(d_px.p, px.data(), 4 * m, hipMemcpyHostToDevice));
  hipStream_t st = nullptr;
  const auto fill =
      tracer->desc.geometry == GRT_GEOM_KERR_BL ? grt::kerr_bl::launch_gbuffer_fill : grt::launch_gbuffer_fill;
  for (uint64_t base = 0; base < m; base += chunk_pix) {
    const uint64_t mc = std::min(chunk_pix, m - base), nr = mc * per;
    if ((rc = S.reserve_pixels(S.n_pix + mc))) return rc;
    const uint64_t off = S.n_rays();
    const uint32_t* d_chunk = (const uint32_t*)d_px.p + base;
    HIP_TRY(grt::launch_make_offsets(d_chunk, mc, nullptr, 0, spa, info.row0, info.col0, info.cols, (uint32_t*)pix.p,
                                     (double*)dx.p, (double*)dy.p, st));
    grt::WorkList wo;
    std::memset(&wo, 0, sizeof(wo));
    wo.row0 = info.row0;
    wo.col0 = info.col0;
    wo.rows = info.rows;
    wo.cols = info.cols;
    wo.n_items = nr;
    wo.pixel_index = (const uint32_t*)pix.p;
    wo.dx = (const double*)dx.p;
    wo.dy = (const double*)dy.p;
    const grt::Outputs o{(float*)xyza.p,
                         (uint8_t*)cls.p,
                         (uint8_t*)S.status.p + off,
                         nullptr,
                         (uint32_t*)S.steps.p + off,
                         (uint8_t*)S.stop.p + off,
                         (uint32_t*)hits.p};
    float t_ms = 0;
    // the chunk again while a trace loses candidates, as grt_gbuffer_trace does
    for (int traces = 1;; ++traces) {
      unsigned long long need = 0;
      acc[3] = 0;
      if ((rc = trace_sync(tracer, *dc, wo, o, acc, &t_ms, &need, nullptr, true))) return rc;
      if (acc[3] == 0) break;
      if (traces == 3 || dc->pool_cap >= POOL_MAX)
        return fail(-ENOMEM, "the hit pool still overflows after " + std::to_string(traces) + " traces");
      if ((rc = ensure_pool(*dc, need + need / 4))) return rc;
    }
    ms[0] += t_ms;
    if ((rc = stream_order(*dc, st))) return rc;
    HIP_TRY(hipEventRecord(dc->ev0, st));
    HIP_TRY(grt::gbuffer_layer_scan((const uint8_t*)S.status.p + off, (const uint32_t*)hits.p, nr, (uint64_t*)counts.p,
                                    (uint64_t*)local.p, temp.p, &temp_bytes, st));
    uint64_t n_new = 0;
    HIP_TRY(hipMemcpy(&n_new, (const uint64_t*)local.p + nr, 8, hipMemcpyDeviceToHost));
    if ((rc = S.reserve_layers(S.n_layers + n_new))) return rc;
    HIP_TRY(grt::gbuffer_sub_append((const uint64_t*)local.p, nr, S.n_layers, (uint64_t*)S.layer_start.p + off, d_chunk,
                                    mc, (uint32_t)S.n_pix, (uint32_t*)S.sub_block.p, (uint32_t*)S.sub_pixel.p, st));
    grt::Workspace ws;
    if ((rc = ensure_workspace(*dc, nr, &ws))) return rc;  // the carving of the trace above
    ws.pool = dc->d_pool;
    HIP_TRY(fill(tracer->desc.geometry, dc->d_scene, wo, ws, S.view(off, nr), st));
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

static void stats_from(const unsigned long long acc[8], double kernel_ms, grt_stats* stats) {
  std::memset(stats, 0, sizeof(*stats));
  stats->accepted_steps = acc[0];
  stats->attempts = acc[1];
  stats->rays = acc[2];
  stats->hit_overflows = acc[3];
  stats->kernel_ms = (float)kernel_ms;
  stats->march_jobs = acc[4];
  stats->march_samples = acc[5];
  stats->march_noise_samples = acc[6];
  stats->march_emit_samples = acc[7];
}

extern "C" {

int grt_gbuffer_supersample(grt_scene* tracer, grt_gbuffer* gb, uint32_t spa, uint64_t n, const uint32_t* pixels,
                            grt_stats* stats) {
  if (!tracer || !gb || (n && !pixels)) return fail(-EINVAL, "null argument");
  int rc;
  if ((rc = check_spa(gb, spa)) || (rc = check_tracer(gb, tracer))) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  std::vector<uint32_t> px;
  px.reserve(n);
  for (uint64_t k = 0; k < n; ++k) {
    if (pixels[k] >= gb->info.n_pixels)
      return fail(-EINVAL, "g-buffer: pixel " + std::to_string(pixels[k]) + " is outside the " +
                               std::to_string(gb->info.n_pixels) + " pixels of the buffer");
    if (gb->sub.h_block.empty() || gb->sub.h_block[pixels[k]] == grt::GBUFFER_NIL) px.push_back(pixels[k]);
  }
  // ascending pixel index: two runs append the same bytes
  std::sort(px.begin(), px.end());
  px.erase(std::unique(px.begin(), px.end()), px.end());
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double ms[2] = {0.0, 0.0};
  if ((rc = sub_fill(tracer, gb, spa, px, acc, ms))) return rc;
  if (stats) stats_from(acc, ms[0], stats);
  return 0;
}

int grt_gbuffer_shade_section(grt_scene* s, grt_gbuffer* gb, const grt_adaptive_config* cfg, const double* mask_xyza,
                              grt_scene* tracer, double* xyza_out, uint8_t* class_out, uint8_t* status_out,
                              uint64_t* n_supersampled, grt_subsample_failures* failures,
                              grt_gbuffer_section_report* report) {
  if (!s || !gb || !cfg || !xyza_out) return fail(-EINVAL, "null argument");
  if (cfg->samples_per_axis == 0) return fail(-EINVAL, "adaptive_sampling.samples_per_axis must be greater than zero");
  int rc = grt_gbuffer_shape_compatible(&gb->info.shape, &s->desc);
  if (rc) return rc;
  const bool supersampled = cfg->enabled || mask_xyza != nullptr;
  const bool sub_pass = supersampled && !mask_xyza;
  const uint32_t spa = cfg->samples_per_axis;
  if (sub_pass && (rc = check_spa(gb, spa))) return rc;
  if (sub_pass && tracer && (rc = check_tracer(gb, tracer))) return rc;
  if (report) std::memset(report, 0, sizeof(*report));
  if (n_supersampled) *n_supersampled = 0;
  if (failures) failures->count = 0;
  const int device = gb->info.device;
  const uint32_t w = gb->info.cols, h = gb->info.rows;
  const uint64_t n = gb->info.n_pixels, per = (uint64_t)spa * spa;
  if (n > (uint64_t)INT_MAX) return fail(-EOVERFLOW, "section larger than INT_MAX pixels");
  DeviceCopy* dc;
  if ((rc = ensure_device(s, device, &dc))) return rc;
  std::unique_lock<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  GBufferSub& S = gb->sub;
  if (sub_pass && (rc = S.ensure_map(n))) return rc;
  const bool device_floor = supersampled && !cfg->has_minimum_luminance;
  const uint64_t sub_chunk = g_sub_chunk.load(std::memory_order_relaxed);
  size_t sort_bytes = 0, select_bytes = 0, split_bytes = 0;
  if (device_floor) HIP_TRY(grt::luminance_floor_device(nullptr, 4, n, floor_index(n), nullptr, &sort_bytes, nullptr, 0));
  if (supersampled) HIP_TRY(grt::compact_flags(nullptr, n, nullptr, nullptr, nullptr, &select_bytes, 0));
  if (sub_pass)
    HIP_TRY(grt::gbuffer_split(nullptr, nullptr, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               &split_bytes, 0));
  const uint64_t fail_cap = (failures && failures->pixel && failures->status) ? failures->capacity : 0;
  const bool want_events = fail_cap && failures->stop;
  grt::SubsampleFailures fails{nullptr, nullptr, nullptr, fail_cap};
  // the section's buffers, then the selection's, then one chunk of sub-ray outputs
  float *b_xyza = nullptr, *c_xyza = nullptr;
  uint8_t *b_cls = nullptr, *b_status = nullptr, *b_flags = nullptr, *b_split = nullptr;
  uint8_t *c_cls = nullptr, *c_status = nullptr, *c_stop = nullptr;
  double *b_x64 = nullptr, *d_floor = nullptr, *c_x64 = nullptr;
  uint32_t *b_sel = nullptr, *b_held = nullptr, *b_missing = nullptr, *c_steps = nullptr;
  unsigned long long* d_cnt = nullptr;  // [0] selected, [1] failed sub-samples, [2] held, [3] missing
  void *b_sort = nullptr, *b_select = nullptr, *b_split_tmp = nullptr;
  const uint64_t chunk_pix = std::max<uint64_t>(1, std::min<uint64_t>(n, sub_chunk / per));
  const uint32_t n_chunks = (uint32_t)((n + chunk_pix - 1) / chunk_pix);
  const uint64_t cap = chunk_pix * per;
  auto carve = [&](AdArena& A) {
    b_xyza = (float*)A.take(n * 16);
    b_cls = (uint8_t*)A.take(n);
    b_status = (uint8_t*)A.take(n);
    b_x64 = (double*)A.take(n * 32);
    if (!supersampled) return;
    b_flags = (uint8_t*)A.take(n);
    b_sel = (uint32_t*)A.take(n * 4);
    d_cnt = (unsigned long long*)A.take(32);
    d_floor = (double*)A.take(8);
    b_sort = A.take(sort_bytes);
    b_select = A.take(select_bytes);
    if (!sub_pass) return;
    b_split = (uint8_t*)A.take(2 * n);
    b_held = (uint32_t*)A.take(n * 4);
    b_missing = (uint32_t*)A.take(n * 4);
    b_split_tmp = A.take(split_bytes);
    c_xyza = (float*)A.take(cap * 16);
    c_cls = (uint8_t*)A.take(cap);
    c_status = (uint8_t*)A.take(cap);
    c_x64 = (double*)A.take(cap * 32);
    c_stop = (uint8_t*)A.take(cap);
    c_steps = (uint32_t*)A.take(cap * 4);
    fails.key = (uint64_t*)A.take(fail_cap * 8);
    fails.status = (uint8_t*)A.take(fail_cap);
    if (want_events) {
      fails.stop = (uint8_t*)A.take(fail_cap);
      fails.steps = (uint32_t*)A.take(fail_cap * 4);
    }
  };
  {
    AdArena plan;
    carve(plan);
    if ((rc = ad_reserve(*dc, plan.off))) return rc;
    AdArena A{(char*)dc->ad_mem, 0};
    carve(A);
  }
  hipStream_t st = nullptr;
  float shade_ms = 0;
  unsigned long long cnt[4] = {0, 0, 0, 0};
  // split the selection by what the set holds, shade the held sub-rays, average them
  auto enqueue_sub_pass = [&]() -> int {
    HIP_TRY(hipMemsetAsync(d_cnt + 1, 0, 24, st));
    HIP_TRY(grt::gbuffer_split(b_sel, d_cnt, n, (const uint32_t*)S.sub_block.p, b_split, b_held, d_cnt + 2, b_missing,
                               d_cnt + 3, b_split_tmp, &split_bytes, st));
    if (S.n_pix == 0) return 0;  // nothing held: every selected pixel is missing
    fails.count = d_cnt + 1;
    fails.ray_stop = c_stop;
    fails.ray_steps = c_steps;
    const grt::Outputs so{c_xyza, c_cls, c_status, c_x64, c_steps, c_stop, nullptr};
    const grt::GBufferArrays sv = S.view(0, S.n_rays());
    for (uint32_t c = 0; c < n_chunks; ++c) {
      const uint64_t base = (uint64_t)c * chunk_pix;
      HIP_TRY(grt::launch_gbuffer_shade_sub(dc->d_scene, sv, (const uint32_t*)S.steps.p, (const uint32_t*)S.sub_block.p,
                                            b_held + base, chunk_pix, d_cnt + 2, base, spa, so, st));
      HIP_TRY(grt::launch_average(b_held + base, b_held + base, chunk_pix, d_cnt + 2, base, spa, c_x64, c_status, b_x64,
                                  fails, st));
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
  {
    const grt::Outputs o{b_xyza, b_cls, b_status, b_x64, nullptr, nullptr, nullptr};
    HIP_TRY(grt::launch_gbuffer_shade(dc->d_scene, gb->view(), o, st));
  }
  if (supersampled) {
    if (device_floor)
      HIP_TRY(grt::luminance_floor_device(b_x64 + 1, 4, n, floor_index(n), b_sort, &sort_bytes, d_floor, st));
    grt::AdaptiveParams ap;
    ap.w = w;
    ap.h = h;
    ap.exclude_background_contrast = cfg->exclude_background_contrast;
    ap._pad = 0;
    ap.min_lum = cfg->minimum_luminance;
    ap.luminance_contrast_threshold = cfg->luminance_contrast_threshold;
    ap.opacity_contrast_threshold = cfg->opacity_contrast_threshold;
    HIP_TRY(grt::launch_select(b_x64, b_cls, ap, device_floor ? d_floor : nullptr, b_flags, st));
    HIP_TRY(grt::compact_flags(b_flags, n, b_sel, d_cnt, b_select, &select_bytes, st));
    if (mask_xyza) HIP_TRY(grt::launch_paint(b_sel, n, d_cnt, mask_xyza, b_x64, st));
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
    HIP_TRY(hipMemcpy(px.data(), b_missing, 4 * n_missing, hipMemcpyDeviceToHost));
    lk.unlock();  // the tracer may be this scene: sub_fill takes its device's lock
    rc = sub_fill(tracer, gb, spa, px, acc, trace_ms);
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
      stats_from(acc, trace_ms[0], &report->top_up);
    }
  }
  HIP_TRY(hipMemcpy(xyza_out, b_x64, n * 32, hipMemcpyDeviceToHost));
  if (class_out) HIP_TRY(hipMemcpy(class_out, b_cls, n, hipMemcpyDeviceToHost));
  if (status_out) HIP_TRY(hipMemcpy(status_out, b_status, n, hipMemcpyDeviceToHost));
  if (supersampled) {
    if (n_supersampled) *n_supersampled = cnt[0];
    if (failures && sub_pass) {
      failures->count = cnt[1];
      if (int frc = copy_failures(fails, cnt[1], spa, failures)) return frc;
    }
  }
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
  if (!sub_pixel || !h || !h->status || !h->stop || !h->steps || !h->sky_u || !h->sky_v || !h->sky_redshift ||
      !h->layer_start)
    return fail(-EINVAL, "null argument");
  if (l && (!h->object || !h->u || !h->v || !h->redshift || !h->radius)) return fail(-EINVAL, "null layer array");
  HIP_TRY(hipSetDevice(gb->info.device));
  HIP_TRY(hipMemcpy(sub_pixel, S.sub_pixel.p, 4 * m, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->status, S.status.p, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->stop, S.stop.p, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->steps, S.steps.p, 4 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->sky_u, S.sky_u.p, 8 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->sky_v, S.sky_v.p, 8 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->sky_redshift, S.sky_z.p, 8 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->layer_start, S.layer_start.p, 8 * (n + 1), hipMemcpyDeviceToHost));
  if (l) {
    HIP_TRY(hipMemcpy(h->object, S.object.p, l, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->u, S.u.p, 8 * l, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->v, S.v.p, 8 * l, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->redshift, S.z.p, 8 * l, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->radius, S.radius.p, 8 * l, hipMemcpyDeviceToHost));
  }
  return 0;
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
    HIP_TRY(hipMemcpy(N->status.p, h->status, n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->stop.p, h->stop, n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->steps.p, h->steps, 4 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->sky_u.p, h->sky_u, 8 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->sky_v.p, h->sky_v, 8 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->sky_z.p, h->sky_redshift, 8 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->layer_start.p, h->layer_start, 8 * (n + 1), hipMemcpyHostToDevice));
    if (l) {
      HIP_TRY(hipMemcpy(N->object.p, h->object, l, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(N->u.p, h->u, 8 * l, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(N->v.p, h->v, 8 * l, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(N->z.p, h->redshift, 8 * l, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(N->radius.p, h->radius, 8 * l, hipMemcpyHostToDevice));
    }
    N->n_pix = m;
    N->n_layers = l;
    HIP_TRY(grt::gbuffer_sub_index((const uint32_t*)N->sub_pixel.p, m, gb->info.n_pixels, (uint32_t*)N->sub_block.p,
                                   nullptr));
    HIP_TRY(hipDeviceSynchronize());
    for (uint64_t j = 0; j < m; ++j) N->h_block[sub_pixel[j]] = (uint32_t)j;
  }
  // the old set's arrays are freed with N
  std::swap(gb->sub.spa, N->spa);
  std::swap(gb->sub.n_pix, N->n_pix);
  std::swap(gb->sub.cap_pix, N->cap_pix);
  std::swap(gb->sub.n_layers, N->n_layers);
  std::swap(gb->sub.cap_layers, N->cap_layers);
  std::swap(gb->sub.h_block, N->h_block);
  for (DevBuf GBufferSub::*f : {&GBufferSub::sub_pixel, &GBufferSub::sub_block, &GBufferSub::status, &GBufferSub::stop,
                                &GBufferSub::steps, &GBufferSub::sky_u, &GBufferSub::sky_v, &GBufferSub::sky_z,
                                &GBufferSub::layer_start, &GBufferSub::object, &GBufferSub::u, &GBufferSub::v,
                                &GBufferSub::z, &GBufferSub::radius})
    std::swap((gb->sub.*f).p, ((*N).*f).p);
  return 0;
}

int grt_gbuffer_destroy(grt_gbuffer* gb) {
  if (!gb) return 0;
  (void)hipSetDevice(gb->info.device);
  delete gb;
  return 0;
}

}  // extern "C"
