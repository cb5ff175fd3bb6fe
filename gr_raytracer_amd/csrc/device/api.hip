// api.hip — C ABI of the device hot path (include/grt_api.h): scenes and their device
// copies, the trace, and the plain render, trace, health and shard entry points.  The
// adaptive pass and camera sequences are api_adaptive.hip, geometry buffers api_gbuffer.hip;
// api_internal.h holds what the three share.
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
#include "api_internal.h"

using namespace grt_api;

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

}  // namespace

GRT_API_NAMESPACE {

int fail(int code, const std::string& msg) {
  grt_host::set_error(msg);
  return code;
}

constexpr uint64_t POOL_MIN = 1ull << 20;            // records
static std::atomic<uint64_t> g_pool_min{POOL_MIN};  // grt_set_hit_pool_min (tests force a full pool)
static uint64_t pool_record_bytes(bool vol) { return 4 + 1 + 4 * 8 + 3 * 8 + 4 + 4 * 8 + 4 + (vol ? 3 * 8 + 4 * 8 : 0); }

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

// The hit-time arrays of a lapse trace, as large as the workspace arena and the pool are now
// (after ensure_workspace and ensure_pool): 8 B per slot per ray and 8 B per pool record.
static int ensure_hit_times(DeviceCopy& dc) {
  auto grow = [&](void** mem, uint64_t* cap, uint64_t want, uint64_t per) -> int {
    if (*mem && *cap >= want) return 0;
    if (*mem) {
      (void)hipDeviceSynchronize();  // earlier async launches may still use the old array
      (void)hipFree(*mem);
    }
    *mem = nullptr;
    *cap = 0;
    if (hipMalloc(mem, std::max<uint64_t>(want * per, 16)) != hipSuccess) {
      (void)hipGetLastError();
      *mem = nullptr;
      return fail(-ENOMEM, "cannot allocate the hit times of a lapse trace");
    }
    *cap = want;
    return 0;
  };
  if (int rc = grow(&dc.slot_time_mem, &dc.slot_time_cap, dc.ws_cap, 8ull * GRT_WS_SLOTS)) return rc;
  return grow(&dc.pool_time_mem, &dc.pool_time_cap, dc.pool_cap, 8);
}

static grt::HitPool pool_view(const DeviceCopy& dc) {
  grt::HitPool hp;
  std::memset(&hp, 0, sizeof(hp));
  hp.head = dc.ws_head;
  hp.last = dc.ws_last;
  hp.slot_time = (double*)dc.slot_time_mem;
  hp.pool_time = (double*)dc.pool_time_mem;
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

static void copy_texture(const grt_texture_desc& t, HostTexture& out) {
  if (t.kind == GRT_TEX_BITMAP && t.rgba && t.width && t.height) {
    size_t n = (size_t)t.width * t.height;
    out.rgba.resize(n);
    std::memcpy(out.rgba.data(), t.rgba, n * 4);
  }
}

template <class T>
static int upload(DeviceCopy& dc, const T* src, size_t n, T** dst) {
  *dst = nullptr;
  if (n == 0) return 0;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, n * sizeof(T)));
  dc.allocations.push_back(p);
  HIP_TRY(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
  *dst = (T*)p;
  return 0;
}

static void fill_dev_texture(const grt_texture_desc& t, grt::DevTexture& d) {
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

static int init_device_copy(grt_scene* s, int device, DeviceCopy& dc);

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
static DeviceCopy* find_device(const grt_scene* s, int device) {
  if (device < 0 || device >= grt_scene::MAX_DEVICES) return nullptr;
  DeviceCopy* p = s->devices[device].load(std::memory_order_acquire);
  return (p && p->ready.load(std::memory_order_acquire)) ? p : nullptr;
}

static int init_device_copy(grt_scene* s, int device, DeviceCopy& dc) {
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

grt::WorkList offsets_worklist(uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols, uint64_t n_items,
                               const uint32_t* pix, const double* dx, const double* dy) {
  grt::WorkList wl;
  std::memset(&wl, 0, sizeof(wl));
  wl.row0 = row0;
  wl.col0 = col0;
  wl.rows = rows;
  wl.cols = cols;
  wl.n_items = n_items;
  wl.pixel_index = pix;
  wl.dx = dx;
  wl.dy = dy;
  return wl;
}

int upload_cam_table(const grt_camera_desc* cameras, uint32_t n, uint32_t rows, DevBuf& buf, grt::CamTable* ct) {
  std::vector<grt::DevCamera> cams(n);
  for (uint32_t f = 0; f < n; ++f) fill_dev_camera(cameras[f], cams[f]);
  if (int rc = buf.alloc(n * sizeof(grt::DevCamera))) return rc;
  HIP_TRY(hipMemcpy(buf.p, cams.data(), n * sizeof(grt::DevCamera), hipMemcpyHostToDevice));
  *ct = grt::CamTable{(const grt::DevCamera*)buf.p, rows, n};
  return 0;
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
static bool schedule_wanted(const grt_scene* s, const grt::WorkList& wl, const Knobs& k) {
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
static bool impact_wanted(const grt_scene* s, const grt::WorkList& wl, const Knobs& k) {
  return !wl.pixel_index && k.schedule == -1 && s->desc.geometry == GRT_GEOM_SCHWARZSCHILD &&
         wl.n_items / 64 >= 1024 && !schedule_wanted(s, wl, k);
}

// The impact-parameter order with the tiles grouped by the sincos case of their rays
// (schedule.hip tile_class; grt_set_class_order): automatic mode where impact_wanted
// holds; forced (1, 2) for any Schwarzschild rectangle of more than one tile that is not
// probe-ordered, whatever grt_set_schedule says.
static bool class_order_wanted(const grt_scene* s, const grt::WorkList& wl, const Knobs& k) {
  if (k.class_order == 0 || wl.pixel_index || s->desc.geometry != GRT_GEOM_SCHWARZSCHILD) return false;
  if (k.class_order < 0) return impact_wanted(s, wl, k);
  return wl.n_items / 64 > 1 && !schedule_wanted(s, wl, k);
}

// Enqueue the probe pass and the sort; returns the device tile order in *order.
// quad: the Kerr-Schild probe on quads, -1 automatic, 0 never, 1 always (grt_debug_probe_keys).
// cls (with impact): the composite key, length bucket then sincos class; cls_out / corner_out
// (nullable) receive the device arrays of the tiles' classes and the corner predictions.
static int enqueue_tile_order(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, hipStream_t stream,
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
static int tail_list(const grt_scene* s, DeviceCopy& dc, uint64_t lanes, long long tail, grt::TailList* tl,
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
static unsigned long long* g_rt = nullptr;
static uint64_t g_rt_cap = 0, g_rt_n = 0;
static uint64_t g_rt_trace = 0, g_rt_only = 0;  // record only trace g_rt_only since grt_debug_ray_times_only (0: each)
static int ray_times_reserve(uint64_t n, hipStream_t stream) {
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
                  unsigned long long* d_stats, hipStream_t stream, const grt::CamTable* ct, bool exact, bool lapse) {
  grt::WorkList wl = wl_in;
  if (lapse && (ct || !exact || dc.vol)) return fail(-EINVAL, "a lapse trace is exact, of one camera, without VolumetricDiscs");
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
  if (lapse && (rc = ensure_hit_times(dc))) return rc;
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
  // (geodesic_fused.hip); Kerr-Schild always runs the exact ones, and so does a scene with a
  // VolumetricDisc (contraction alone moves robust pixels of the stock KerrBL gas past 1e-4:
  // tests/test_fused.py)
  const bool fused = k.arith == 1 && !exact && s->desc.geometry != GRT_GEOM_KERR && !dc.vol;
  const auto launch = fused ? grt::fused::launch_trace
                            : (s->desc.geometry == GRT_GEOM_KERR_BL ? grt::kerr_bl::launch_trace : grt::launch_trace);
  // the exact KerrBL kernels are a unit of their own (geodesic_kerr_bl.hip)
  if (lapse)  // the buffer's trace that records hit times: the lapse unit and its KerrBL half
    HIP_TRY((s->desc.geometry == GRT_GEOM_KERR_BL ? grt::lapse_kerr_bl::launch_trace : grt::lapse::launch_trace)(
        s->desc.geometry, dc.d_scene, wl, ws, o, dc.d_counter, d_stats, blocks, threads, false, tl, tail_blocks, stream));
  else if (ct)  // a camera sequence: always the exact sequence unit
    HIP_TRY(grt::seq::launch_trace(s->desc.geometry, dc.d_scene, wl, ws, o, dc.d_counter, d_stats, blocks, threads,
                                   dc.vol, tl, tail_blocks, stream, *ct));
  else
    HIP_TRY(launch(s->desc.geometry, dc.d_scene, wl, ws, o, dc.d_counter, d_stats, blocks, threads, dc.vol, tl,
                   tail_blocks, stream));
  return stream_done(dc, stream);
}

static int validate_desc(const grt_scene_desc* d) {
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

}  // namespace grt_api

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

// Test hook (not in grt_api.h): the range-free divisions and square root (geodesic_rhs.h
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
// last reset (geodesic_rhs.h path_count): out[28], [k] wave-level, [14 + k] lane-level.
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

// object `obj` of the scene is a VolumetricDisc (the vdisc checks' argument test; no device needed)
static bool is_vdisc(const grt_scene* s, int64_t obj) {
  return obj >= 0 && obj < (int64_t)s->desc.n_objects && s->desc.objects[obj].kind == GRT_OBJ_VOLUMETRIC_DISC;
}

// Test hook (not in grt_api.h): the VolumetricDisc device functions of volumetric.h for object
// `obj` on n host inputs of 6 doubles each (vdisc_points_kernel; fn and the layout of in[6 n],
// out[8 n] and flag[n]: kernels.h VdiscCheckFn and the kernel's comment).  n == 0 does nothing.
int grt_debug_vdisc_points(grt_scene* s, int device, int obj, int fn, uint64_t n, const double* in, double* out,
                           uint8_t* flag) {
  if (!s) return fail(-EINVAL, "vdisc points: null scene");
  if (fn < 0 || fn >= grt::VDISC_FN_COUNT) return fail(-EINVAL, "vdisc points: fn 0..4");
  if (!is_vdisc(s, obj)) return fail(-EINVAL, "vdisc points: the object is not a VolumetricDisc of the scene");
  if (n == 0) return 0;
  if (!in || !out || !flag || n > (1ull << 24)) return fail(-EINVAL, "vdisc points: null buffer or n > 2^24");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  DevBuf b_in, b_out, b_f;
  if ((rc = b_in.alloc(n * 48)) || (rc = b_out.alloc(n * 64)) || (rc = b_f.alloc(n))) return rc;
  HIP_TRY(hipMemcpy(b_in.p, in, n * 48, hipMemcpyHostToDevice));
  HIP_TRY(grt::launch_vdisc_points(dc->d_scene, (uint32_t)obj, fn, n, (const double*)b_in.p, (double*)b_out.p,
                                   (uint8_t*)b_f.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, b_out.p, n * 64, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(flag, b_f.p, n, hipMemcpyDeviceToHost));
  return 0;
}

// Test hook (not in grt_api.h): the surface path's device functions on n host rows of 8 doubles
// each (surface_points_kernel; fn and the layout of in[8 n], out[8 n] and flag[n]: kernels.h
// SurfaceCheckFn and the kernel's comment).  obj: the Disc of DISC_CHORD, the Sphere of
// SPHERE_CHORD, the object whose table LUT_INDEX (a Kerr temperature table) and TEMPERATURE
// read and whose texture TEXTURE samples; -1 for LUT_INDEX over the blackbody table, the
// celestial TEXTURE, and every other request.  n == 0 does nothing.
int grt_debug_surface_points(grt_scene* s, int device, int obj, int fn, uint64_t n, const double* in, double* out,
                             uint8_t* flag) {
  if (!s) return fail(-EINVAL, "surface points: null scene");
  if (fn < 0 || fn >= grt::SURFACE_FN_COUNT) return fail(-EINVAL, "surface points: fn 0..7");
  const grt_scene_desc& d = s->desc;
  if (obj < -1 || obj >= (int64_t)d.n_objects) return fail(-EINVAL, "surface points: obj is -1 or an object of the scene");
  const grt_object_desc* o = obj < 0 ? nullptr : &d.objects[obj];
  const bool has_lut = o && o->temp_kind == GRT_TEMP_KERR_LUT && o->lut_n >= 2 && s->lut_r[obj].size() == o->lut_n;
  bool ok = true;
  switch (fn) {
    case grt::SURFACE_FN_DISC_CHORD: ok = o && o->kind == GRT_OBJ_DISC; break;
    case grt::SURFACE_FN_SPHERE_CHORD: ok = o && o->kind == GRT_OBJ_SPHERE; break;
    case grt::SURFACE_FN_LUT_INDEX: ok = o ? has_lut : d.bb_n >= 2; break;
    case grt::SURFACE_FN_TEMPERATURE: ok = o && o->kind != GRT_OBJ_SPHERE && (o->temp_kind == GRT_TEMP_CONSTANT || has_lut); break;
    case grt::SURFACE_FN_BLACKBODY: ok = !o && d.bb_n >= 2; break;
    case grt::SURFACE_FN_TEXTURE: break;  // every texture of a created scene is complete (validate_desc)
    default: ok = !o; break;              // WINDOW_FAR, BLEND: no object
  }
  if (!ok) return fail(-EINVAL, "surface points: obj does not fit the request");
  if (n == 0) return 0;
  if (!in || !out || !flag || n > (1ull << 24)) return fail(-EINVAL, "surface points: null buffer or n > 2^24");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  DevBuf b_in, b_out, b_f;
  if ((rc = b_in.alloc(n * 64)) || (rc = b_out.alloc(n * 64)) || (rc = b_f.alloc(n))) return rc;
  HIP_TRY(hipMemcpy(b_in.p, in, n * 64, hipMemcpyHostToDevice));
  HIP_TRY(grt::launch_surface_points(d.geometry, dc->d_scene, obj, fn, n, (const double*)b_in.p, (double*)b_out.p,
                                     (uint8_t*)b_f.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, b_out.p, n * 64, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(flag, b_f.p, n, hipMemcpyDeviceToHost));
  return 0;
}

// Test hook (not in grt_api.h): the production march_kernel over n host jobs.  Job i is a
// candidate of object obj[i] at ro[3 i ..] with the chord direction dir[3 i ..] of a ray whose
// frequency data is freq[3 i ..] = (observer energy, p_t, p_phi).  The workspace describes
// exactly these jobs: ray i holds job i as its slot-0 candidate (rec, rec_dir, rc, jobs), or,
// with as_pool, as record i of a HitPool (a JOB_POOL job); march[0] = n.  `blocks` blocks;
// arith 0 runs the exact kernel (grt::march_kernel, KerrBL: grt::kerr_bl's), 1 the fused one
// (grt::fused::march_kernel; refused for Kerr-Schild, as enqueue_trace never runs it there).
// col[4 n]: the colour per job; counters[4]: march jobs, samples, noise samples, emitting
// samples (grt_stats' march_* fields).  n == 0 launches nothing and zeroes the counters.
int grt_debug_vdisc_march(grt_scene* s, int device, uint64_t n, const uint32_t* obj, const double* ro,
                          const double* dir, const double* freq, int blocks, int arith, int as_pool, double* col,
                          uint64_t* counters) {
  if (!s) return fail(-EINVAL, "vdisc march: null scene");
  if (arith != 0 && arith != 1) return fail(-EINVAL, "vdisc march: arith 0 (exact) or 1 (fused)");
  if (arith == 1 && s->desc.geometry == GRT_GEOM_KERR)
    return fail(-EINVAL, "vdisc march: Kerr-Schild has no fused kernels");
  if (blocks < 1 || blocks > 4096) return fail(-EINVAL, "vdisc march: 1 <= blocks <= 4096");
  if (n == 0) {
    if (counters) std::fill(counters, counters + 4, 0ull);
    return 0;
  }
  if (!obj || !ro || !dir || !freq || !col || !counters || n > (1ull << 16))
    return fail(-EINVAL, "vdisc march: null buffer or n > 2^16");
  for (uint64_t i = 0; i < n; ++i)
    if (!is_vdisc(s, obj[i])) return fail(-EINVAL, "vdisc march: a job's object is not a VolumetricDisc of the scene");
  DeviceCopy* dc;
  int rc = ensure_device(s, device, &dc);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(dc->mu);
  HIP_TRY(hipSetDevice(device));
  const uint64_t MN = (uint64_t)GRT_WS_SLOTS * n;
  constexpr size_t MARCH_WORDS = 8 + GRT_MAX_OBJECTS;
  std::vector<grt::CandRec> rec(n);
  std::vector<double> rec_dir(3 * MN, 0.0), rcv(6 * n, 0.0), p_pt(3 * n), p_dir(3 * n);
  std::vector<uint64_t> jobs(n);
  std::vector<uint8_t> p_obj(n);
  for (uint64_t i = 0; i < n; ++i) {
    std::memset(&rec[i], 0, sizeof(grt::CandRec));
    rec[i].obj = obj[i];
    p_obj[i] = (uint8_t)obj[i];
    for (int k = 0; k < 3; ++k) {
      rec[i].pt[k] = p_pt[k * n + i] = ro[3 * i + k];
      rec_dir[k * MN + i] = p_dir[k * n + i] = dir[3 * i + k];
    }
    rcv[i] = freq[3 * i];
    rcv[4 * n + i] = freq[3 * i + 1];
    rcv[5 * n + i] = freq[3 * i + 2];
    jobs[i] = as_pool ? (grt::JOB_POOL | (i << 31) | i) : (i << 8);
  }
  DevBuf b_rec, b_dir, b_vcol, b_rc, b_jobs, b_march, b_pool, b_pobj, b_ppt, b_pdir, b_pvcol;
  if ((rc = b_rec.alloc(n * sizeof(grt::CandRec))) || (rc = b_dir.alloc(3 * MN * 8)) || (rc = b_vcol.alloc(4 * MN * 8)) ||
      (rc = b_rc.alloc(6 * n * 8)) || (rc = b_jobs.alloc(n * 8)) || (rc = b_march.alloc(MARCH_WORDS * 8)) ||
      (rc = b_pool.alloc(sizeof(grt::HitPool))) || (rc = b_pobj.alloc(n)) || (rc = b_ppt.alloc(3 * n * 8)) ||
      (rc = b_pdir.alloc(3 * n * 8)) || (rc = b_pvcol.alloc(4 * n * 8)))
    return rc;
  unsigned long long march[MARCH_WORDS] = {};
  march[0] = n;
  grt::HitPool hp;
  std::memset(&hp, 0, sizeof(hp));
  hp.cap = n;
  hp.obj = (uint8_t*)b_pobj.p;
  hp.pt = (double*)b_ppt.p;
  hp.dir = (double*)b_pdir.p;
  hp.vcol = (double*)b_pvcol.p;
  HIP_TRY(hipMemcpy(b_rec.p, rec.data(), n * sizeof(grt::CandRec), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_dir.p, rec_dir.data(), 3 * MN * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(b_vcol.p, 0xff, 4 * MN * 8));  // NaN: a job the kernel did not colour shows
  HIP_TRY(hipMemset(b_pvcol.p, 0xff, 4 * n * 8));
  HIP_TRY(hipMemcpy(b_rc.p, rcv.data(), 6 * n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_jobs.p, jobs.data(), n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_march.p, march, sizeof(march), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_pobj.p, p_obj.data(), n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_ppt.p, p_pt.data(), 3 * n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_pdir.p, p_dir.data(), 3 * n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b_pool.p, &hp, sizeof(hp), hipMemcpyHostToDevice));
  grt::Workspace ws;
  std::memset(&ws, 0, sizeof(ws));
  ws.n = n;
  ws.rc = (double*)b_rc.p;
  ws.rec = (grt::CandRec*)b_rec.p;
  ws.rec_dir = (double*)b_dir.p;
  ws.vcol = (double*)b_vcol.p;
  ws.jobs = (uint64_t*)b_jobs.p;
  ws.march = (unsigned long long*)b_march.p;
  ws.pool = (const grt::HitPool*)b_pool.p;
  const int g = s->desc.geometry;
  const auto launch = arith == 1 ? grt::fused::launch_march
                                 : (g == GRT_GEOM_KERR_BL ? grt::kerr_bl::launch_march : grt::launch_march);
  HIP_TRY(launch(g, dc->d_scene, ws, blocks, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  const uint64_t stride = as_pool ? n : MN;
  std::vector<double> vcol(4 * stride);
  HIP_TRY(hipMemcpy(vcol.data(), as_pool ? b_pvcol.p : b_vcol.p, 4 * stride * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(march, b_march.p, sizeof(march), hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < n; ++i)
    for (int q = 0; q < 4; ++q) col[4 * i + q] = vcol[q * stride + i];
  counters[0] = march[3];
  counters[1] = march[2];
  counters[2] = march[4];
  counters[3] = march[5];
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
    if (dc->slot_time_mem) (void)hipFree(dc->slot_time_mem);
    if (dc->pool_time_mem) (void)hipFree(dc->pool_time_mem);
    if (dc->ev0) (void)hipEventDestroy(dc->ev0);
    if (dc->ev1) (void)hipEventDestroy(dc->ev1);
    if (dc->ev_busy) (void)hipEventDestroy(dc->ev_busy);
    delete dc;
  }
  delete s;
  return 0;
}

}  // extern "C"

GRT_API_NAMESPACE {

int check_rect(const grt_scene* s, uint64_t row0, uint64_t col0, uint64_t rows, uint64_t cols) {
  if (row0 + rows > (uint64_t)s->desc.camera.rows || col0 + cols > (uint64_t)s->desc.camera.cols)
    return fail(-EINVAL, "rectangle outside the camera frame");
  return 0;
}

// Synchronous calls: after the work has finished, whether some trace needed more hit-pool
// records than it had.  If so the pool is grown to that size (*again = true): the call
// traces again, and the deterministic trace then keeps every candidate.
int pool_check(DeviceCopy& dc, bool* again) {
  unsigned long long need = 0;
  HIP_TRY(hipMemcpy(&need, dc.d_counter + 6, sizeof(need), hipMemcpyDeviceToHost));
  *again = need > dc.pool_cap && dc.pool_cap < POOL_MAX;
  if (*again) return ensure_pool(dc, need + need / 4);
  return 0;
}

namespace {
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
}  // namespace

// The counters of a call's traces, on the host: acc[0..3] accepted steps, attempts, rays,
// hit overflows (DeviceCopy::d_stats); acc[4..7] march jobs, samples, noise samples,
// emitting samples (DeviceCopy::d_march [3], [2], [4], [5]).
// reset_counters: zero the device's counters and the hit pool's recorded need, on `st`.
int reset_counters(DeviceCopy& dc, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(dc.d_stats, 0, 4 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(dc.d_march, 0, 8 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(dc.d_counter + 6, 0, sizeof(unsigned long long), st));
  return 0;
}
// read_counters: add the device's counters to acc (the work on them has been waited for).
int read_counters(DeviceCopy& dc, unsigned long long acc[8]) {
  unsigned long long h[4], m[8];
  HIP_TRY(hipMemcpy(h, dc.d_stats, sizeof(h), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(m, dc.d_march, sizeof(m), hipMemcpyDeviceToHost));
  for (int k = 0; k < 4; ++k) acc[k] += h[k];
  acc[4] += m[3];
  acc[5] += m[2];
  acc[6] += m[4];
  acc[7] += m[5];
  return 0;
}
void stats_from(const unsigned long long acc[8], double kernel_ms, grt_stats* stats) {
  std::memset(stats, 0, sizeof(*stats));
  stats->accepted_steps = acc[0];
  stats->attempts = acc[1];
  stats->rays = acc[2];
  stats->hit_overflows = acc[3];
  stats->kernel_ms = kernel_ms;
  stats->march_jobs = acc[4];
  stats->march_samples = acc[5];
  stats->march_noise_samples = acc[6];
  stats->march_emit_samples = acc[7];
}

// One trace of `wl` on the null stream, waited for.  Adds its counters to acc and its
// event time to *ms; *need = hit-pool records it asked for.
int trace_sync(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, const grt::Outputs& o,
               unsigned long long acc[8], float* ms, unsigned long long* need, const grt::CamTable* ct, bool exact,
               bool lapse) {
  hipStream_t st = nullptr;
  int rc;
  if ((rc = reset_counters(dc, st))) return rc;
  HIP_TRY(hipEventRecord(dc.ev0, st));
  if ((rc = enqueue_trace(s, dc, wl, o, dc.d_stats, st, ct, exact, lapse))) return rc;
  HIP_TRY(hipEventRecord(dc.ev1, st));
  HIP_TRY(hipEventSynchronize(dc.ev1));
  if ((rc = read_counters(dc, acc))) return rc;
  HIP_TRY(hipMemcpy(need, dc.d_counter + 6, sizeof(*need), hipMemcpyDeviceToHost));
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, dc.ev0, dc.ev1));
  *ms += t;
  return 0;
}

// Trace `wl` (n output slots) into device scratch, wait, copy to the host arrays.  When the
// hit pool was too small (the trace asked for more records than it had), only the pixels
// that lost candidates (GRT_FLAG_HIT_OVERFLOW) are traced again, as a pixel list at their
// centres (get_ray_for_offset at (0.5, 0.5) is get_ray_for, camera.rs:338-363), with the
// pool grown once that subset alone does not fit; their outputs replace the flagged ones.
// `offs` (host, nullable): the offsets list wl was built from.  acc (zero on entry) and *ms
// count the work done, the re-traced rays included; the overflows are those of the last
// round.  ct: a camera sequence (enqueue_trace), `wl` its stack.
int trace_to_host(grt_scene* s, DeviceCopy& dc, const grt::WorkList& wl, uint64_t n, const grt_offsets* offs,
                  float* xyza_out, uint8_t* class_out, uint8_t* status_out, const grt_aux_out* aux,
                  unsigned long long acc[8], float* ms_out, const grt::CamTable* ct) {
  int rc;
  float& ms = *ms_out;
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
    uint32_t row0 = wl.row0, rows = wl.rows;
    if (offs) {  // an offsets trace: the same (pixel, dx, dy) items
      for (uint64_t j = 0; j < m; ++j) {
        pix[j] = offs->pixel_index[lost[j]];
        dx[j] = offs->dx[lost[j]];
        dy[j] = offs->dy[lost[j]];
      }
    } else if (wl.n_shards > 1) {  // a row-band shard: frame rows of the local ones
      row0 = 0;
      rows = (uint32_t)s->desc.camera.rows;
      for (uint64_t j = 0; j < m; ++j) {
        const uint32_t lr = (uint32_t)(lost[j] / wl.cols), c = (uint32_t)(lost[j] % wl.cols);
        pix[j] = grt::shard_frame_row(wl.band_rows, wl.shard, wl.n_shards, lr) * wl.cols + c;
      }
    } else {
      for (uint64_t j = 0; j < m; ++j) pix[j] = (uint32_t)lost[j];
    }
    DevBuf b_pix, b_dx, b_dy;
    if ((rc = b_pix.alloc(m * 4)) || (rc = b_dx.alloc(m * 8)) || (rc = b_dy.alloc(m * 8))) return rc;
    HIP_TRY(hipMemcpy(b_pix.p, pix.data(), m * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_dx.p, dx.data(), m * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_dy.p, dy.data(), m * 8, hipMemcpyHostToDevice));
    const grt::WorkList wo = offsets_worklist(row0, wl.col0, rows, wl.cols, m, (const uint32_t*)b_pix.p,
                                              (const double*)b_dx.p, (const double*)b_dy.p);
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
  return 0;
}

// trace_to_host with the counters as grt_stats (nullable).
static int run_to_host(grt_scene* s, DeviceCopy* dc, const grt::WorkList& wl, uint64_t n, const grt_offsets* offs,
                       float* xyza_out, uint8_t* class_out, uint8_t* status_out, const grt_aux_out* aux,
                       grt_stats* stats) {
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float ms = 0;
  if (int rc = trace_to_host(s, *dc, wl, n, offs, xyza_out, class_out, status_out, aux, acc, &ms)) return rc;
  if (stats) stats_from(acc, ms, stats);
  return 0;
}

}  // namespace grt_api

extern "C" {

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
    if ((rc = b_pix.alloc(n * 4)) || (rc = b_dx.alloc(n * 8)) || (rc = b_dy.alloc(n * 8))) return rc;
    HIP_TRY(hipMemcpy(b_pix.p, offsets->pixel_index, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_dx.p, offsets->dx, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_dy.p, offsets->dy, n * 8, hipMemcpyHostToDevice));
    wl = offsets_worklist(row0, col0, rows, cols, n, (const uint32_t*)b_pix.p, (const double*)b_dx.p,
                          (const double*)b_dy.p);
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

}  // extern "C"

// ------------------------------------------------------------- row-band shards ----
GRT_API_NAMESPACE {
int check_shard(const grt_row_shard* sh) {
  if (!sh) return fail(-EINVAL, "null shard");
  if (sh->n_shards == 0 || sh->shard >= sh->n_shards) return fail(-EINVAL, "shard index out of range");
  if (sh->band_rows == 0) return fail(-EINVAL, "band_rows must be >= 1");
  return 0;
}
grt::WorkList shard_worklist(const grt_scene* s, const grt_row_shard* sh) {
  uint32_t rows = grt_shard_row_count((uint32_t)s->desc.camera.rows, sh);
  grt::WorkList wl = rect_worklist(0, 0, rows, (uint32_t)s->desc.camera.cols);
  wl.band_rows = sh->band_rows;
  wl.shard = sh->shard;
  wl.n_shards = sh->n_shards;
  return wl;
}
}  // namespace grt_api

extern "C" {

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
