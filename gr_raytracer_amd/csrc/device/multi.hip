// multi.hip — one frame over several GPUs of one process (grt_render_frame_multi,
// include/grt_api.h): the north-star layout behind the C ABI.  The frame's rows are cut
// into cyclic bands (band b -> device b mod N, grt_row_shard), one host thread per device
// traces its bands (grt_render_shard_async on the device's own stream), and ONE grouped
// RCCL send/recv moves every device's pixel records to devices[0] over xGMI, where
// deinterleave_kernel puts them in frame order.  With the reference's adaptive
// supersampling, one RCCL allgather of (Y, alpha, class) per pixel comes first: the
// selection stencil reads neighbours in other devices' bands and the luminance floor is a
// percentile of the whole frame (raytracer.rs:91-129, :386-458).
//
// The reference renders a frame in one process (render_section_to_cie_buffer_raw,
// raytracer.rs:195-244, called from main.rs:80-116 via Raytracer::render_section
// :460-497); every pixel here is identical to grt_render_pixels / grt_render_section of
// the same frame on one device (tests/test_multi.py).
//
// Two further transports (grt_set_multi_transport) move the same blocks without RCCL: the
// devices belong to one process, and after a trace's stream synchronise and the host
// barrier every block is complete in its owner's memory.  GRT_TRANSPORT_PEER maps the
// devices into each other (hipDeviceEnablePeerAccess) and gather_peer_kernel on the reading
// device dereferences the owners' blocks in place; GRT_TRANSPORT_PEER_STAGED copies each
// block into the reader's staging (hipMemcpyPeerAsync) and runs deinterleave_kernel as the
// RCCL path does.  Neither loads RCCL, and under both a device list may name one GPU
// several times: each entry is a rank with its own stream, events and arena, which runs
// the whole N > 1 host path on one GPU (tests/test_multi_peer.py).
//
// grt_gbuffer_trace_multi runs the same ranks, context, barrier and transports for the
// frame's geometry buffer: each rank traces and fills its shard into one block
// (gbuffer_trace_shard, api_gbuffer.hip), and devices[0] assembles the blocks into an
// ordinary grt_gbuffer with the two kernels of gbuffer.hip (gbuffer_gather.h).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "grt_api.h"
#include "../host/host_internal.h"
#include "dev_scene.h"
#include "api_internal.h"
#include "gbuffer_gather.h"

namespace grt {

// Fields of a pixel record, in the order they sit in a device's send block (8-byte fields
// first).  Bit f of a field mask selects field f.
enum RecField { RF_XYZA64 = 0, RF_XYZA32 = 1, RF_STEPS = 2, RF_CLASS = 3, RF_STATUS = 4, RF_STOP = 5, RF_N = 6 };
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr uint32_t rec_field_bytes(int f) { return f == RF_XYZA64 ? 32 : f == RF_XYZA32 ? 16 : f == RF_STEPS ? 4 : 1; }

constexpr int MULTI_MAX = GRT_MULTI_MAX_DEVICES;

// Where the gathered buffer holds each shard's fields, and the frame they go to.
struct GatherLayout {
  uint32_t cols, band_rows, n_shards, n_fields;
  uint64_t n_pixels;                 // frame pixels, rows x cols
  uint32_t elem[RF_N];               // bytes per pixel of gathered field k
  uint64_t src[MULTI_MAX][RF_N];     // byte offset of shard s's field k in the gathered buffer
};
struct GatherDst {
  uint8_t* p[RF_N];  // frame-order output of gathered field k
};

// Frame pixel p's field k: the shard that holds it, and its byte offset from the start of
// what L.src is relative to (the gathered buffer, or the shard's own block).
__host__ __device__ inline uint64_t gather_source_of(const GatherLayout& L, int k, uint64_t p, uint32_t* shard) {
  const uint32_t row = (uint32_t)(p / L.cols), col = (uint32_t)(p % L.cols);
  uint32_t lr;
  frame_row_source(L.band_rows, L.n_shards, row, shard, &lr);
  return L.src[*shard][k] + ((uint64_t)lr * L.cols + col) * L.elem[k];
}

// Byte offset in the gathered buffer of frame pixel p's field k.
__host__ __device__ inline uint64_t gather_source(const GatherLayout& L, int k, uint64_t p) {
  uint32_t s;
  return gather_source_of(L, k, p, &s);
}

// The peer transport's sources: shard s's block where its owner wrote it (another rank's
// arena, on this or a peer-mapped device); L.src is then relative to base[s].
struct GatherSrc {
  const uint8_t* base[MULTI_MAX];
};

// De-interleave: blockIdx.y = field, a grid-stride loop over the frame's pixels.  Reads
// are coalesced within a band row (consecutive pixels of one row are consecutive in their
// shard), writes always.  Every field offset is 256-B aligned, so the 32- and 16-B
// fields move as 16-B vectors.  An HBM stream: (read + write) x record bytes per pixel.
__global__ void __launch_bounds__(256) deinterleave_kernel(GatherLayout L, const uint8_t* __restrict__ g,
                                                           GatherDst d) {
  const int k = blockIdx.y;
  const uint32_t e = L.elem[k];
  uint8_t* __restrict__ out = d.p[k];
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < L.n_pixels;
       p += (uint64_t)gridDim.x * blockDim.x) {
    const uint8_t* s = g + gather_source(L, k, p);
    uint8_t* t = out + p * e;
    if (e == 32) {
      const uint4 a = ((const uint4*)s)[0], b = ((const uint4*)s)[1];
      ((uint4*)t)[0] = a;
      ((uint4*)t)[1] = b;
    } else if (e == 16) {
      *(uint4*)t = *(const uint4*)s;
    } else if (e == 4) {
      *(uint32_t*)t = *(const uint32_t*)s;
    } else {
      for (uint32_t b = 0; b < e; ++b) t[b] = s[b];
    }
  }
}

// The de-interleave with a base pointer per shard (GRT_TRANSPORT_PEER): the same grid,
// source function and moves as deinterleave_kernel, reading every block in its owner's
// memory.  Consecutive pixels of a band row are consecutive in their shard's block, so a
// wave's reads are contiguous runs of a row (or of the rows around a band edge); the
// blocks and their field offsets are 256-B aligned, so the 32- and 16-B fields move as
// 16-B vectors.  Reads of another GPU's block cross xGMI once per byte; writes are local.
__global__ void __launch_bounds__(256) gather_peer_kernel(GatherLayout L, GatherSrc S, GatherDst d) {
  const int k = blockIdx.y;
  const uint32_t e = L.elem[k];
  uint8_t* __restrict__ out = d.p[k];
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < L.n_pixels;
       p += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t sh;
    const uint64_t off = gather_source_of(L, k, p, &sh);
    const uint8_t* __restrict__ s = S.base[sh] + off;
    uint8_t* t = out + p * e;
    if (e == 32) {
      const uint4 a = ((const uint4*)s)[0], b = ((const uint4*)s)[1];
      ((uint4*)t)[0] = a;
      ((uint4*)t)[1] = b;
    } else if (e == 16) {
      *(uint4*)t = *(const uint4*)s;
    } else if (e == 4) {
      *(uint32_t*)t = *(const uint32_t*)s;
    } else {
      for (uint32_t b = 0; b < e; ++b) t[b] = s[b];
    }
  }
}

// The adaptive pass's neighbourhood record of each local pixel: (Y, alpha) of the 1-spp
// f64 XYZA, and the class (should_supersample_pair, raytracer.rs:91-108; the floor,
// resolve_minimum_luminance :118-129, reads Y).
__global__ void __launch_bounds__(256) pack_ya_kernel(const double* __restrict__ x64, const uint8_t* __restrict__ cls,
                                                      uint64_t n, double* __restrict__ ya, uint8_t* __restrict__ c_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const double y = x64[4 * i + 1], a = x64[4 * i + 3];
    ya[2 * i] = y;
    ya[2 * i + 1] = a;
    c_out[i] = cls[i];
  }
}

}  // namespace grt

namespace {

using grt_api::fail;  // and HIP_TRY (api_internal.h)

// RCCL is bound at the first multi-GPU frame (dlopen of librccl.so.1), not linked: a
// process that never renders over several GPUs (the single-GPU CLI, the Python host) does
// not load the 570 MB library at start-up, and libgrt.so loads where RCCL is absent.
struct Rccl {
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  std::string error;  // why binding failed, or empty
};
const Rccl& rccl() {
  static const Rccl r = [] {
    Rccl x;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      const char* e = dlerror();
      x.error = std::string("cannot load librccl.so.1: ") + (e ? e : "unknown error");
      return x;
    }
    auto get = [&](auto& fn, const char* name) {
      fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
      if (!fn && x.error.empty()) x.error = std::string("librccl.so.1 has no ") + name;
    };
    get(x.CommInitAll, "ncclCommInitAll");
    get(x.CommDestroy, "ncclCommDestroy");
    get(x.GetErrorString, "ncclGetErrorString");
    get(x.AllGather, "ncclAllGather");
    get(x.GroupStart, "ncclGroupStart");
    get(x.GroupEnd, "ncclGroupEnd");
    get(x.Send, "ncclSend");
    get(x.Recv, "ncclRecv");
    return x;
  }();
  return r;
}
#define NCCL_TRY(expr)                                                                   \
  do {                                                                                   \
    ncclResult_t _r = (expr);                                                            \
    if (_r != ncclSuccess) return fail(-EIO, std::string(#expr) + ": " + rccl().GetErrorString(_r)); \
  } while (0)

// grt_set_multi_transport: read once per frame.
std::atomic<int> g_transport{GRT_TRANSPORT_RCCL};
// grt_debug_multi_fail: rank * 4 + stage of the injected failure, -1 when none is armed.
std::atomic<int> g_inject{-1};

constexpr uint64_t align256(uint64_t b) { return (b + 255) & ~255ull; }

// Byte offset of field f in a block of n pixels holding the fields of `mask`; f = RF_N
// gives the block's size.  Each field starts 256-B aligned.
uint64_t field_offset(uint32_t mask, uint64_t n, int f) {
  uint64_t off = 0;
  for (int g = 0; g < f; ++g)
    if (mask & (1u << g)) off += align256(n * grt::rec_field_bytes(g));
  return off;
}

// Per device: its stream, events and a grow-only scratch arena.
struct MultiDev {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev[6] = {};  // trace start / end, allgather start / end, gather start / end
  void* mem = nullptr;
  uint64_t bytes = 0;
};

// One RCCL communicator per device of a device list (ncclCommInitAll), created on first
// use and cached for the process: a frame after the first pays no setup.  `mu` serialises
// frames on one device list (a communicator is driven by one thread at a time).
// RCCL's start-up takes seconds (1.6-5.8 s for one device on the pool's boxes, most of it
// loading its device code), and while it runs a kernel launch of the process can wait for
// it; so the communicators are created on a thread of their own (`comm_ready`) started
// once every device has enqueued its first frame's trace (note_launched), and a device
// waits for them only before its first collective.
struct MultiCtx {
  std::vector<int> devs;
  int transport = GRT_TRANSPORT_RCCL;  // the transport asked for (part of the cache key)
  // GRT_TRANSPORT_PEER: every pair of distinct devices is mapped both ways (a context
  // with a pair that cannot be runs its frames staged)
  bool peer_mapped = false;
  std::vector<ncclComm_t> comms;
  std::vector<MultiDev> d;
  std::mutex mu;
  std::mutex cm;  // the three below
  std::condition_variable cv;
  int launched = 0;
  bool started = false;
  std::shared_future<std::string> comm_ready;  // "" once the communicators exist, else the error

  // A device thread of the first frame has enqueued its trace (or failed before): the
  // last of them starts the communicators' creation.
  void note_launched() {
    std::lock_guard<std::mutex> lk(cm);
    if (started || ++launched < (int)devs.size()) return;
    started = true;
    MultiCtx* cp = this;
    comm_ready = std::async(std::launch::async, [cp]() -> std::string {
                   const Rccl& R = rccl();
                   if (!R.error.empty()) return R.error;
                   const ncclResult_t r = R.CommInitAll(cp->comms.data(), (int)cp->devs.size(), cp->devs.data());
                   return r == ncclSuccess ? std::string() : std::string("ncclCommInitAll: ") + R.GetErrorString(r);
                 }).share();
    cv.notify_all();
  }
};
std::mutex g_ctx_mu;
std::vector<std::unique_ptr<MultiCtx>> g_ctx;

// Map every pair of distinct devices of `devs` into each other, once per context and
// before any arena of it is allocated.  *mapped = false when some pair cannot be.
int enable_peer_access(const std::vector<int>& devs, bool* mapped) {
  *mapped = true;
  for (int a : devs)
    for (int b : devs) {
      if (a == b) continue;
      int can = 0;
      HIP_TRY(hipDeviceCanAccessPeer(&can, a, b));
      if (!can) {
        *mapped = false;
        continue;
      }
      HIP_TRY(hipSetDevice(a));
      const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
      if (e == hipErrorPeerAccessAlreadyEnabled) {
        (void)hipGetLastError();
      } else if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(-EIO, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
      }
    }
  return 0;
}

int get_ctx(const std::vector<int>& devs, int transport, MultiCtx** out) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  for (auto& c : g_ctx)
    if (c->devs == devs && c->transport == transport) {
      *out = c.get();
      return 0;
    }
  auto c = std::make_unique<MultiCtx>();
  c->devs = devs;
  c->transport = transport;
  if (transport == GRT_TRANSPORT_PEER)
    if (int rc = enable_peer_access(devs, &c->peer_mapped)) return rc;
  c->comms.resize(devs.size());
  c->d.resize(devs.size());
  for (size_t i = 0; i < devs.size(); ++i) {
    MultiDev& m = c->d[i];
    m.device = devs[i];
    HIP_TRY(hipSetDevice(devs[i]));
    HIP_TRY(hipStreamCreateWithFlags(&m.st, hipStreamNonBlocking));
    for (auto& e : m.ev) HIP_TRY(hipEventCreate(&e));
  }
  *out = c.get();
  g_ctx.push_back(std::move(c));
  return 0;
}

// A device list: 1..GRT_MULTI_MAX_DEVICES valid ordinals, distinct unless `repeats` (the
// peer transports: each entry is a rank of its own).  bad_ordinal: the code for an ordinal
// the machine does not have.
int check_devices(int n_devices, const int* devices, bool repeats, std::vector<int>* out, int bad_ordinal = -ENODEV) {
  if (!devices) return fail(-EINVAL, "null argument");
  if (n_devices < 1 || n_devices > grt::MULTI_MAX) return fail(-EINVAL, "n_devices must be in 1..GRT_MULTI_MAX_DEVICES");
  std::vector<int> devs(devices, devices + n_devices);
  for (int a = 0; a < n_devices && !repeats; ++a)
    for (int b = a + 1; b < n_devices; ++b)
      if (devs[a] == devs[b]) return fail(-EINVAL, "a device appears twice (one RCCL rank per GPU)");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  for (int d : devs)
    if (d < 0 || d >= ndev) return fail(bad_ordinal, "invalid device ordinal");
  *out = std::move(devs);
  return 0;
}

// The communicators of C, waited for (created beside the first frame's traces).
int comms_ready(MultiCtx& C) {
  std::shared_future<std::string> f;
  {
    std::unique_lock<std::mutex> lk(C.cm);
    C.cv.wait(lk, [&] { return C.started; });
    f = C.comm_ready;
  }
  const std::string err = f.get();
  return err.empty() ? 0 : fail(-EIO, err);
}

// A reusable barrier of the device threads.  arrive(ok) returns false on every thread
// when any thread arrived with ok == false: no thread then enters the next collective
// (a peer that never joins would leave the others waiting in RCCL).
struct Barrier {
  std::mutex mu;
  std::condition_variable cv;
  int n, waiting = 0;
  uint64_t gen = 0;
  bool failed = false;
  explicit Barrier(int n_) : n(n_) {}
  bool arrive(bool ok) {
    std::unique_lock<std::mutex> lk(mu);
    if (!ok) failed = true;
    const uint64_t g = gen;
    if (++waiting == n) {
      waiting = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g; });
    }
    return !failed;
  }
};

// The plan of one frame: which fields move, each device's rows and buffers.
struct Plan {
  uint32_t rows = 0, cols = 0, band = 0, n_dev = 0;
  uint32_t mask = 0;          // fields each device sends
  bool super = false;         // adaptive supersampling (or the sampling-mask paint)
  uint64_t n_local[grt::MULTI_MAX] = {};
  uint64_t block[grt::MULTI_MAX] = {};   // send block bytes
  uint64_t block_off[grt::MULTI_MAX + 1] = {};  // offsets in the gathered buffer
  uint64_t max_local = 0;
  uint64_t ag_bytes = 0;      // per-device allgather block: (Y, alpha) then class, padded to max_local
  int transport = GRT_TRANSPORT_RCCL;  // the transport this frame runs
};

// The peer transports: where each rank's allgather record and send block are this frame.
// A rank writes its own entries before the first barrier it arrives at with ok = true; the
// others read them after that barrier, and only when it let them pass.
struct PeerTable {
  const uint8_t* ag_send[grt::MULTI_MAX] = {};
  const uint8_t* block[grt::MULTI_MAX] = {};
};

// Failed sub-samples each device records before the merge truncates to the caller's
// capacity (14 B each in the device's adaptive scratch).
constexpr uint64_t FAIL_KEEP_MIN = 1ull << 16;

// grt_debug_multi_fail: true once, for the armed (rank, stage).
bool injected_failure(int rank, int stage) {
  int want = rank * 4 + stage;
  return g_inject.compare_exchange_strong(want, -1);
}

struct DevResult {
  int rc = 0;
  std::string err;
  unsigned long long stats[4] = {0, 0, 0, 0};
  uint64_t n_sel = 0;
  float trace_ms = 0, ag_ms = 0, gather_ms = 0;
  std::vector<uint32_t> f_pix, f_smp, f_steps;
  std::vector<uint8_t> f_status, f_stop;
  uint64_t f_count = 0;
};

// Carve a device's scratch (AdArena style: plan with base == nullptr, then carve).
struct Carve {
  char* base = nullptr;
  uint64_t off = 0;
  void* take(uint64_t b) {
    void* r = base ? base + off : nullptr;
    off += align256(b);
    return r;
  }
};
struct DevBufs {
  unsigned long long* stats = nullptr;  // [0..3] trace counters, [4] selected pixels
  double* floor = nullptr;
  uint8_t* block = nullptr;             // send block (fields of plan.mask)
  float* x32 = nullptr;                 // f32 XYZA when the plan does not send it
  double* x64 = nullptr;                // f64 XYZA when the plan does not send it (supersampling sends it)
  uint32_t* steps = nullptr;            // 1-spp step counts when supersampling and the plan does not send them
  uint8_t *ag_send = nullptr, *ag_recv = nullptr;
  double* frame_ya = nullptr;
  uint8_t* frame_cls = nullptr;
  uint8_t* gathered = nullptr;          // devices[0]: every block
  uint8_t* frame = nullptr;             // devices[0]: frame-order fields
};
void carve(Carve& A, const Plan& P, int i, DevBufs& B) {
  const uint64_t n = P.n_local[i];
  const uint64_t F = (uint64_t)P.rows * P.cols;
  B.stats = (unsigned long long*)A.take(8 * 8);
  B.floor = (double*)A.take(8);
  B.block = (uint8_t*)A.take(P.block[i]);
  if (!(P.mask & (1u << grt::RF_XYZA32))) B.x32 = (float*)A.take(n * 16);
  if (P.super) {
    if (!(P.mask & (1u << grt::RF_STEPS))) B.steps = (uint32_t*)A.take(n * 4);
    B.ag_send = (uint8_t*)A.take(P.ag_bytes);
    B.ag_recv = (uint8_t*)A.take(P.ag_bytes * P.n_dev);
    B.frame_ya = (double*)A.take(F * 16);
    B.frame_cls = (uint8_t*)A.take(F);
  }
  if (i == 0) {
    B.gathered = (uint8_t*)A.take(P.block_off[P.n_dev]);
    B.frame = (uint8_t*)A.take(field_offset(P.mask, F, grt::RF_N));
  }
}

uint8_t* field_ptr(uint8_t* block, uint32_t mask, uint64_t n, int f) {
  return (mask & (1u << f)) ? block + field_offset(mask, n, f) : nullptr;
}

// in_place: each shard's offsets from the start of its own block (gather_peer_kernel), not
// from the start of the gathered buffer.
grt::GatherLayout gather_layout(const Plan& P, bool in_place = false) {
  grt::GatherLayout L;
  std::memset(&L, 0, sizeof(L));
  L.cols = P.cols;
  L.band_rows = P.band;
  L.n_shards = P.n_dev;
  L.n_pixels = (uint64_t)P.rows * P.cols;
  for (int f = 0; f < grt::RF_N; ++f) {
    if (!(P.mask & (1u << f))) continue;
    const uint32_t k = L.n_fields++;
    L.elem[k] = grt::rec_field_bytes(f);
    for (uint32_t s = 0; s < P.n_dev; ++s)
      L.src[s][k] = (in_place ? 0 : P.block_off[s]) + field_offset(P.mask, P.n_local[s], f);
  }
  return L;
}

// The (Y, alpha, class) allgather's layout: every rank's record is ag_bytes long; stride
// is the distance between two ranks' records (0: each from its own base pointer).
grt::GatherLayout allgather_layout(const Plan& P, uint64_t stride) {
  grt::GatherLayout L;
  std::memset(&L, 0, sizeof(L));
  L.cols = P.cols;
  L.band_rows = P.band;
  L.n_shards = P.n_dev;
  L.n_pixels = (uint64_t)P.rows * P.cols;
  L.n_fields = 2;
  L.elem[0] = 16;
  L.elem[1] = 1;
  for (uint32_t s = 0; s < P.n_dev; ++s) {
    L.src[s][0] = s * stride;
    L.src[s][1] = s * stride + align256(P.max_local * 16);
  }
  return L;
}

int launch_gather_peer(const grt::GatherLayout& L, const grt::GatherSrc& S, const grt::GatherDst& d, hipStream_t st) {
  if (L.n_pixels == 0 || L.n_fields == 0) return 0;
  const uint64_t want = (L.n_pixels + 255) / 256;
  const unsigned gx = (unsigned)std::min<uint64_t>(want, 8192);
  hipLaunchKernelGGL(grt::gather_peer_kernel, dim3(gx, L.n_fields), dim3(256), 0, st, L, S, d);
  HIP_TRY(hipGetLastError());
  return 0;
}

// One block from its owner's arena into the reader's staging, on the reader's stream.
int copy_block(void* dst, int dst_dev, const void* src, int src_dev, uint64_t bytes, hipStream_t st) {
  if (bytes == 0) return 0;
  if (dst_dev == src_dev)
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
  else
    HIP_TRY(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st));
  return 0;
}

int launch_deinterleave(const grt::GatherLayout& L, const uint8_t* g, const grt::GatherDst& d, hipStream_t st) {
  if (L.n_pixels == 0 || L.n_fields == 0) return 0;
  const uint64_t want = (L.n_pixels + 255) / 256;
  const unsigned gx = (unsigned)std::min<uint64_t>(want, 8192);
  hipLaunchKernelGGL(grt::deinterleave_kernel, dim3(gx, L.n_fields), dim3(256), 0, st, L, g, d);
  HIP_TRY(hipGetLastError());
  return 0;
}

// One device's part of one frame.  Every collective is entered only after a barrier that
// all threads pass with no error so far.
//
// The peer transports (P.transport != GRT_TRANSPORT_RCCL; `i` is then a rank, and several
// ranks may share a GPU) keep the barriers where RCCL has them and replace each collective
// by reads of the other ranks' arenas on this rank's own stream.  What holds on every way
// out, errors included:
//  * a rank synchronises its stream before each barrier, so after one every rank's data
//    is complete and nothing of this frame is still writing it;
//  * an arena is written or regrown only by its own rank, before that rank's first
//    barrier of the frame; others read it only after a barrier, and the last reader
//    (devices[0]'s gather) is synchronised before its part returns, which is before the
//    frame's threads are joined and so before the next frame or trace may touch an arena;
//  * a part leaves its stream idle before it returns, on failure too (the wrapper below),
//    and a failed rank arrives at the barriers it has not reached with ok = false.
void device_part(grt_scene* scene, MultiCtx& C, const Plan& P, int i, const grt_adaptive_config* cfg,
                 const double* mask_xyza, const grt_frame_out* out, grt_subsample_failures* want_fail,
                 Barrier& bar, PeerTable& T, DevResult& R) {
  MultiDev& M = C.d[i];
  const int dev = M.device;
  const bool rccl_path = P.transport == GRT_TRANSPORT_RCCL;
  const bool direct = P.transport == GRT_TRANSPORT_PEER;
  // every thread arrives at each of the frame's barriers exactly once (a failed thread
  // arrives at the ones it has not reached with ok = false, below)
  const int n_barriers = P.super ? 2 : 1;
  int passed = 0;
  bool noted = false;  // C.note_launched() called
  auto barrier = [&]() -> bool {
    ++passed;
    return bar.arrive(true);
  };
  auto run = [&]() -> int {
    HIP_TRY(hipSetDevice(dev));
    if (!rccl_path && injected_failure(i, 1)) return fail(-EIO, "injected failure before the trace");
    Carve plan;
    DevBufs B;
    carve(plan, P, i, B);
    if (plan.off > M.bytes) {
      if (M.mem) {
        HIP_TRY(hipStreamSynchronize(M.st));
        HIP_TRY(hipFree(M.mem));
        M.mem = nullptr;
        M.bytes = 0;
      }
      HIP_TRY(hipMalloc(&M.mem, plan.off));
      M.bytes = plan.off;
    }
    Carve A{(char*)M.mem, 0};
    carve(A, P, i, B);
    T.ag_send[i] = B.ag_send;
    T.block[i] = B.block;
    const uint64_t n = P.n_local[i];
    const hipStream_t st = M.st;
    HIP_TRY(hipMemsetAsync(B.stats, 0, 8 * 8, st));
    HIP_TRY(hipEventRecord(M.ev[0], st));
    grt_row_shard sh{P.band, (uint32_t)i, P.n_dev};
    float* x32 = (P.mask & (1u << grt::RF_XYZA32)) ? (float*)field_ptr(B.block, P.mask, n, grt::RF_XYZA32) : B.x32;
    double* x64 = (double*)field_ptr(B.block, P.mask, n, grt::RF_XYZA64);
    uint8_t* cls = field_ptr(B.block, P.mask, n, grt::RF_CLASS);
    uint8_t* status = field_ptr(B.block, P.mask, n, grt::RF_STATUS);
    // the supersample pass orders its sub-rays by the 1-spp step counts: traced always then
    uint32_t* steps = (P.mask & (1u << grt::RF_STEPS)) ? (uint32_t*)field_ptr(B.block, P.mask, n, grt::RF_STEPS)
                                                       : B.steps;
    uint8_t* stop = field_ptr(B.block, P.mask, n, grt::RF_STOP);
    if (n) {
      int rc = grt_render_shard_async(scene, dev, st, &sh, x32, cls, status, x64, steps, stop, (uint64_t*)B.stats);
      if (rc) return rc;
    }
    noted = true;
    if (rccl_path) C.note_launched();
    if (P.super) {
      // (Y, alpha) and class of every local pixel, then ONE allgather: every device gets
      // the whole frame's neighbourhood records, de-interleaved into frame order
      if (n) {
        const unsigned gx = (unsigned)std::min<uint64_t>((n + 255) / 256, 8192);
        hipLaunchKernelGGL(grt::pack_ya_kernel, dim3(gx), dim3(256), 0, st, x64, cls, n, (double*)B.ag_send,
                           B.ag_send + align256(P.max_local * 16));
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipStreamSynchronize(st));
      if (rccl_path)
        if (int rc = comms_ready(C)) return rc;
      if (!barrier()) return fail(-ECANCELED, "another device failed");
      HIP_TRY(hipEventRecord(M.ev[2], st));
      grt::GatherLayout L = allgather_layout(P, direct ? 0 : P.ag_bytes);
      grt::GatherDst d{};
      d.p[0] = (uint8_t*)B.frame_ya;
      d.p[1] = B.frame_cls;
      if (direct) {  // every rank's record read where its owner packed it
        grt::GatherSrc S{};
        for (uint32_t s = 0; s < P.n_dev; ++s) S.base[s] = T.ag_send[s];
        if (int rc = launch_gather_peer(L, S, d, st)) return rc;
      } else {
        if (rccl_path) {
          NCCL_TRY(rccl().AllGather(B.ag_send, B.ag_recv, P.ag_bytes, ncclUint8, C.comms[i], st));
        } else {
          for (uint32_t s = 0; s < P.n_dev; ++s)
            if (int rc = copy_block(B.ag_recv + s * P.ag_bytes, dev, T.ag_send[s], C.d[s].device, P.ag_bytes, st))
              return rc;
        }
        if (int rc = launch_deinterleave(L, B.ag_recv, d, st)) return rc;
      }
      HIP_TRY(hipEventRecord(M.ev[3], st));
      if (!rccl_path && injected_failure(i, 2)) return fail(-EIO, "injected failure after the allgather");
      // the frame's exact 99th-percentile floor (or the configured minimum), then this
      // device's selection and sub-rays (grt_supersample_shard_device, longest first)
      const bool dev_floor = !cfg->has_minimum_luminance;
      if (dev_floor) {
        int rc = grt_adaptive_floor_device(scene, dev, st, B.frame_ya, 2, L.n_pixels, B.floor);
        if (rc) return rc;
      }
      grt_subsample_failures fl{};
      grt_subsample_failures* flp = nullptr;
      if (want_fail && want_fail->capacity && want_fail->pixel && want_fail->status) {
        // a device keeps whichever of its failures arrive first, so the merged list is the
        // frame's first `capacity` in (pixel, sample) order only while every device holds
        // all of its own: each keeps at least FAIL_KEEP_MIN, whatever the caller's capacity
        const uint64_t cap = std::max<uint64_t>(want_fail->capacity, FAIL_KEEP_MIN);
        R.f_pix.resize(cap);
        R.f_smp.resize(cap);
        R.f_status.resize(cap);
        fl.capacity = cap;
        fl.pixel = R.f_pix.data();
        fl.sample = R.f_smp.data();
        fl.status = R.f_status.data();
        if (want_fail->stop) {
          R.f_stop.resize(cap);
          R.f_steps.resize(cap);
          fl.stop = R.f_stop.data();
          fl.steps = R.f_steps.data();
        }
        flp = &fl;
      }
      int rc = grt_host::supersample_shard(scene, dev, st, &sh, cfg, cfg->minimum_luminance,
                                           dev_floor ? B.floor : nullptr, B.frame_ya, B.frame_cls, mask_xyza, x64,
                                           steps, (uint64_t*)(B.stats + 4), (uint64_t*)B.stats, flp);
      if (rc) return rc;
      R.f_count = flp ? fl.count : 0;
    }
    HIP_TRY(hipEventRecord(M.ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    // ONE gather: every device sends its block to devices[0] (grouped send / receive;
    // devices[0] sends to itself too, so every frame takes the same RCCL path)
    if (rccl_path)
      if (int rc = comms_ready(C)) return rc;
    if (!barrier()) return fail(-ECANCELED, "another device failed");
    if (!rccl_path && injected_failure(i, 3)) return fail(-EIO, "injected failure before the gather");
    HIP_TRY(hipEventRecord(M.ev[4], st));
    if (rccl_path) {
      NCCL_TRY(rccl().GroupStart());
      NCCL_TRY(rccl().Send(B.block, P.block[i], ncclUint8, 0, C.comms[i], st));
      if (i == 0)
        for (uint32_t s = 0; s < P.n_dev; ++s)
          NCCL_TRY(rccl().Recv(B.gathered + P.block_off[s], P.block[s], ncclUint8, (int)s, C.comms[i], st));
      NCCL_TRY(rccl().GroupEnd());
    } else if (i == 0 && !direct) {
      for (uint32_t s = 0; s < P.n_dev; ++s)
        if (int rc = copy_block(B.gathered + P.block_off[s], dev, T.block[s], C.d[s].device, P.block[s], st)) return rc;
    }
    if (i == 0) {
      const grt::GatherLayout L = gather_layout(P, direct);
      grt::GatherDst d{};
      const uint64_t F = L.n_pixels;
      for (int f = 0, k = 0; f < grt::RF_N; ++f)
        if (P.mask & (1u << f)) d.p[k++] = B.frame + field_offset(P.mask, F, f);
      if (direct) {  // rank 0 reads every rank's block in place
        grt::GatherSrc S{};
        for (uint32_t s = 0; s < P.n_dev; ++s) S.base[s] = T.block[s];
        if (int rc = launch_gather_peer(L, S, d, st)) return rc;
      } else if (int rc = launch_deinterleave(L, B.gathered, d, st)) {
        return rc;
      }
    }
    HIP_TRY(hipEventRecord(M.ev[5], st));
    if (i == 0) {  // frame-order fields to the caller
      const uint64_t F = (uint64_t)P.rows * P.cols;
      auto d2h = [&](void* host, int f) -> int {
        if (host && F) HIP_TRY(hipMemcpyAsync(host, B.frame + field_offset(P.mask, F, f), F * grt::rec_field_bytes(f),
                                              hipMemcpyDeviceToHost, st));
        return 0;
      };
      int rc;
      if ((rc = d2h(out->xyza64, grt::RF_XYZA64)) || (rc = d2h(out->xyza, grt::RF_XYZA32)) ||
          (rc = d2h(out->steps, grt::RF_STEPS)) || (rc = d2h(out->ray_class, grt::RF_CLASS)) ||
          (rc = d2h(out->status, grt::RF_STATUS)) || (rc = d2h(out->stop, grt::RF_STOP)))
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long h[5];
    HIP_TRY(hipMemcpy(h, B.stats, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) R.stats[k] = h[k];
    R.n_sel = h[4];
    HIP_TRY(hipEventElapsedTime(&R.trace_ms, M.ev[0], M.ev[1]));
    if (P.super) HIP_TRY(hipEventElapsedTime(&R.ag_ms, M.ev[2], M.ev[3]));
    HIP_TRY(hipEventElapsedTime(&R.gather_ms, M.ev[4], M.ev[5]));
    return 0;
  };
  R.rc = run();
  if (!noted && rccl_path) C.note_launched();  // failed before its trace: the others must not wait
  if (R.rc) {
    R.err = grt_last_error();
    // peer transports: what this rank enqueued may read other ranks' arenas, and its own
    // arena is read by the others once they pass a barrier; the stream is idle before
    // this thread arrives anywhere or returns
    if (!rccl_path && hipSetDevice(dev) == hipSuccess) (void)hipStreamSynchronize(M.st);
    // the barriers this thread has not reached: the other threads stop there instead of
    // entering a collective this device will not join
    for (; passed < n_barriers; ++passed) bar.arrive(false);
  }
}

// No communicator is still being created when a call returns (a frame that failed before its
// collectives has not waited for them).
void settle_comms(MultiCtx& C) {
  std::shared_future<std::string> f;
  {
    std::lock_guard<std::mutex> lk(C.cm);
    if (C.started) f = C.comm_ready;
  }
  if (f.valid()) (void)f.get();
}

// ---- grt_gbuffer_trace_multi: the frame's geometry buffer over the ranks ----
struct GbPlan {
  uint32_t rows = 0, cols = 0, band = 0, n_dev = 0;
  int transport = GRT_TRANSPORT_RCCL;  // the transport this call runs
};
// The frame's table: each rank's block where its owner left it, and its sizes.  A rank
// writes its own entries before it arrives at the first barrier with ok = true; the others
// read them after that barrier, and only when it let them pass.
struct GbTable {
  const uint8_t* base[grt::MULTI_MAX] = {};
  uint64_t n_local[grt::MULTI_MAX] = {}, layers[grt::MULTI_MAX] = {}, bytes[grt::MULTI_MAX] = {};
};
struct GbResult {
  int rc = 0;
  std::string err;
  grt_api::GBufferShard sh;
  float gather_ms = 0;
};

// A rank's arena grown to `bytes`, its first `keep` bytes kept (copied on the rank's stream
// and waited for).  Grow-only, as device_part's.
int arena_reserve(MultiDev& M, uint64_t bytes, uint64_t keep) {
  if (bytes <= M.bytes) return 0;
  HIP_TRY(hipStreamSynchronize(M.st));
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  if (keep && M.mem) {
    hipError_t e = hipMemcpyAsync(p, M.mem, keep, hipMemcpyDeviceToDevice, M.st);
    if (e == hipSuccess) e = hipStreamSynchronize(M.st);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(p);
      return fail(-EIO, std::string("cannot move a g-buffer block: ") + hipGetErrorString(e));
    }
  }
  if (M.mem) (void)hipFree(M.mem);
  M.mem = p;
  M.bytes = bytes;
  return 0;
}

// One rank's part of one buffer: its shard traced and filled into one block of its arena
// (gbuffer_trace_shard, api_gbuffer.hip), the block published, the first barrier, on
// devices[0] every allocation of the assembly (the sizes come from the table), the second
// barrier, then the transport, and on devices[0] the assembly (gbuffer.hip).  device_part's
// invariants hold: the transport, a collective under RCCL, is entered only after a barrier
// that all threads pass with no error so far, so a devices[0] that cannot allocate ends the
// call on every rank instead of leaving the others sending to it; a stream is idle before
// its rank reaches a barrier or returns; a failed rank arrives at every barrier it has not
// reached with ok = false; and devices[0]'s stream, the last reader of every block, is
// synchronised before its part returns.  The context enabled peer access when it was
// created, so every block is allocated after that.
void gbuffer_part(grt_scene* scene, MultiCtx& C, const GbPlan& P, int i, Barrier& bar, GbTable& T, GbResult& R,
                  grt_gbuffer** frame) {
  MultiDev& M = C.d[i];
  const int dev = M.device;
  const bool rccl_path = P.transport == GRT_TRANSPORT_RCCL;
  const bool direct = P.transport == GRT_TRANSPORT_PEER;
  const int n_barriers = 2;
  int passed = 0;
  bool noted = false;
  auto barrier = [&]() -> bool {
    ++passed;
    return bar.arrive(true);
  };
  // devices[0]'s staging (every block back to back) and scan scratch, and the buffer until
  // it is complete: freed after the stream is idle, on failure too
  grt_api::DevBuf staging, counts, temp;
  std::unique_ptr<grt_gbuffer, int (*)(grt_gbuffer*)> made(nullptr, grt_gbuffer_destroy);
  auto run = [&]() -> int {
    HIP_TRY(hipSetDevice(dev));
    if (!rccl_path && injected_failure(i, 1)) return fail(-EIO, "injected failure before the trace");
    const hipStream_t st = M.st;
    const grt_row_shard sh{P.band, (uint32_t)i, P.n_dev};
    int rc = grt_api::gbuffer_trace_shard(
        scene, dev, st, sh,
        [&](uint64_t bytes, uint64_t keep, uint8_t** base) -> int {
          if (int rc2 = arena_reserve(M, bytes, keep)) return rc2;
          *base = (uint8_t*)M.mem;
          return 0;
        },
        &R.sh);
    noted = true;
    if (rccl_path) C.note_launched();
    if (rc) return rc;
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(hipStreamSynchronize(st));
    T.base[i] = R.sh.base;
    T.n_local[i] = R.sh.block.n;
    T.layers[i] = R.sh.block.layers;
    T.bytes[i] = R.sh.block.bytes;
    if (rccl_path)
      if (int rc2 = comms_ready(C)) return rc2;
    if (!barrier()) return fail(-ECANCELED, "another device failed");
    if (!rccl_path && injected_failure(i, 3)) return fail(-EIO, "injected failure before the gather");
    // devices[0]: every allocation of the assembly, before the barrier that lets the ranks
    // into the transport.  The layer total is the sum of the ranks' totals, so the frame's
    // arrays need no read-back.
    const uint64_t F = (uint64_t)P.rows * P.cols;
    uint64_t off[grt::MULTI_MAX + 1] = {}, total = 0;
    size_t temp_bytes = 0;
    grt::GBufferGatherDst D{};
    if (i == 0) {
      for (uint32_t s = 0; s < P.n_dev; ++s) {
        off[s + 1] = off[s] + T.bytes[s];
        total += T.layers[s];
      }
      if (!direct)
        if (int rc2 = staging.alloc(off[P.n_dev])) return rc2;
      grt_gbuffer* gb = nullptr;
      void* fp[grt::GB_FIELDS];
      if (int rc2 = grt_api::gbuffer_frame_alloc(scene, dev, total, &gb, fp)) return rc2;
      made.reset(gb);
      for (int k = 0; k < grt::GB_FIELDS; ++k) D.p[k] = (uint8_t*)fp[k];
      HIP_TRY(grt::gbuffer_gather_scan(nullptr, F, nullptr, nullptr, &temp_bytes, st));
      int rc2;
      if ((rc2 = counts.alloc(8 * (F + 1))) || (rc2 = temp.alloc(temp_bytes))) return rc2;
    }
    if (!barrier()) return fail(-ECANCELED, "another device failed");
    HIP_TRY(hipEventRecord(M.ev[4], st));
    // ONE thing per rank moves: its block
    if (rccl_path) {
      NCCL_TRY(rccl().GroupStart());
      NCCL_TRY(rccl().Send(R.sh.base, T.bytes[i], ncclUint8, 0, C.comms[i], st));
      if (i == 0)
        for (uint32_t s = 0; s < P.n_dev; ++s)
          NCCL_TRY(rccl().Recv((uint8_t*)staging.p + off[s], T.bytes[s], ncclUint8, (int)s, C.comms[i], st));
      NCCL_TRY(rccl().GroupEnd());
    } else if (i == 0 && !direct) {
      for (uint32_t s = 0; s < P.n_dev; ++s)
        if (int rc2 = copy_block((uint8_t*)staging.p + off[s], dev, T.base[s], C.d[s].device, T.bytes[s], st))
          return rc2;
    }
    if (i == 0) {
      // the same two kernels under every transport: only the base pointers differ
      const grt::GBufferGatherShape G{P.rows, P.cols, P.band, P.n_dev, F, total};
      grt::GBufferGatherSrc S{};
      for (uint32_t s = 0; s < P.n_dev; ++s) {
        const grt_api::GBufferBlock B(T.n_local[s], T.layers[s]);
        const uint8_t* b = direct ? T.base[s] : (const uint8_t*)staging.p + off[s];
        for (int k = 0; k < grt::GB_FIELDS; ++k) S.p[k][s] = b + B.off[k];
      }
      HIP_TRY(grt::launch_gbuffer_gather_pixels(G, S, D, (uint64_t*)counts.p, st));
      uint64_t* frame_start = (uint64_t*)D.p[grt_host::GB_layer_start];
      HIP_TRY(grt::gbuffer_gather_scan((const uint64_t*)counts.p, F, frame_start, temp.p, &temp_bytes, st));
      // the offsets are the single-device ones only if they end at the ranks' total; the
      // layer kernel indexes by them, so it runs after the check
      uint64_t end = 0;
      HIP_TRY(hipMemcpyAsync(&end, frame_start + F, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (end != total)
        return fail(-EIO, "the frame's layer offsets end at " + std::to_string(end) + ", the ranks filled " +
                              std::to_string(total) + " layers");
      HIP_TRY(grt::launch_gbuffer_gather_layers(G, S, D, st));
    }
    HIP_TRY(hipEventRecord(M.ev[5], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&R.gather_ms, M.ev[4], M.ev[5]));
    if (i == 0) *frame = made.release();
    return 0;
  };
  R.rc = run();
  if (!noted && rccl_path) C.note_launched();  // failed before its trace: the others must not wait
  if (R.rc) {
    R.err = grt_last_error();
    // peer transports: what this rank enqueued may read other ranks' blocks, and its own is
    // read by devices[0] once it passes the second barrier; the stream is idle before this
    // thread arrives anywhere or returns (under RCCL a collective that failed part-way
    // would never let it become so)
    if (!rccl_path && hipSetDevice(dev) == hipSuccess) (void)hipStreamSynchronize(M.st);
    for (; passed < n_barriers; ++passed) bar.arrive(false);
  }
}

}  // namespace

extern "C" {

int grt_render_frame_multi(grt_scene* scene, int n_devices, const int* devices, uint32_t band_rows,
                           const grt_adaptive_config* cfg, const double* sampling_mask_xyza, const grt_frame_out* out,
                           uint64_t* n_supersampled, grt_stats* stats, grt_subsample_failures* failures,
                           grt_multi_report* report) {
  const auto t0 = std::chrono::steady_clock::now();
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n_supersampled) *n_supersampled = 0;
  if (failures) failures->count = 0;
  if (!scene || !devices || !out) return fail(-EINVAL, "null argument");
  if (band_rows == 0) return fail(-EINVAL, "band_rows must be >= 1");
  const int transport = g_transport.load();
  std::vector<int> devs;
  if (int rc = check_devices(n_devices, devices, transport != GRT_TRANSPORT_RCCL, &devs)) return rc;
  Plan P;
  P.n_dev = (uint32_t)n_devices;
  P.band = band_rows;
  {
    int64_t r = 0, c = 0;
    grt_host::scene_frame_size(scene, &r, &c);
    if (r <= 0 || c <= 0 || r > (int64_t)UINT32_MAX || c > (int64_t)UINT32_MAX)
      return fail(-EINVAL, "camera frame size out of range");
    P.rows = (uint32_t)r;
    P.cols = (uint32_t)c;
  }
  P.super = (cfg && cfg->enabled) || sampling_mask_xyza != nullptr;
  if (P.super) {
    if (!cfg) return fail(-EINVAL, "supersampling needs the adaptive configuration");
    if (cfg->samples_per_axis == 0) return fail(-EINVAL, "adaptive_sampling.samples_per_axis must be greater than zero");
    if (!out->xyza64) return fail(-EINVAL, "a supersampled frame is f64: pass out->xyza64");
    if (out->xyza) return fail(-EINVAL, "a supersampled frame has no f32 XYZA (pass out->xyza = NULL)");
  }
  P.mask = (1u << grt::RF_CLASS) | (1u << grt::RF_STATUS);
  if (out->xyza64 || P.super) P.mask |= 1u << grt::RF_XYZA64;
  if (out->xyza) P.mask |= 1u << grt::RF_XYZA32;
  if (out->steps) P.mask |= 1u << grt::RF_STEPS;
  if (out->stop) P.mask |= 1u << grt::RF_STOP;
  uint64_t off = 0;
  for (uint32_t s = 0; s < P.n_dev; ++s) {
    grt_row_shard sh{band_rows, s, P.n_dev};
    P.n_local[s] = (uint64_t)grt_shard_row_count(P.rows, &sh) * P.cols;
    P.max_local = std::max(P.max_local, P.n_local[s]);
    P.block[s] = field_offset(P.mask, P.n_local[s], grt::RF_N);
    P.block_off[s] = off;
    off += P.block[s];
  }
  P.block_off[P.n_dev] = off;
  P.ag_bytes = align256(P.max_local * 16) + align256(P.max_local);
  if (P.super && (uint64_t)P.rows * P.cols > (uint64_t)INT32_MAX) return fail(-EOVERFLOW, "frame larger than INT_MAX pixels");
  MultiCtx* C;
  if (int rc = get_ctx(devs, transport, &C)) return rc;
  std::lock_guard<std::mutex> lk(C->mu);
  // a device pair that cannot be mapped: the frame moves its blocks by copies
  P.transport = (transport == GRT_TRANSPORT_PEER && !C->peer_mapped) ? GRT_TRANSPORT_PEER_STAGED : transport;
  const bool ranks = P.transport != GRT_TRANSPORT_RCCL;
  std::vector<DevResult> R;
  uint32_t attempt = 0;
  // a trace that lost hit candidates (a device's hit pool too small) grows that device's
  // pool from the trace's measured need and the frame is traced again, at most 3 times
  for (;;) {
    ++attempt;
    R.assign(P.n_dev, DevResult());
    Barrier bar(n_devices);
    PeerTable T;
    std::vector<std::thread> th;
    for (int i = 1; i < n_devices; ++i)
      th.emplace_back(device_part, scene, std::ref(*C), std::cref(P), i, cfg, sampling_mask_xyza, out, failures,
                      std::ref(bar), std::ref(T), std::ref(R[i]));
    device_part(scene, *C, P, 0, cfg, sampling_mask_xyza, out, failures, bar, T, R[0]);
    for (auto& t : th) t.join();
    settle_comms(*C);
    for (uint32_t i = 0; i < P.n_dev; ++i)
      if (R[i].rc && R[i].rc != -ECANCELED)
        return fail(R[i].rc, (ranks ? "rank " + std::to_string(i) + " (device " + std::to_string(devs[i]) + ")"
                                    : "device " + std::to_string(devs[i])) +
                                 ": " + R[i].err);
    for (uint32_t i = 0; i < P.n_dev; ++i)
      if (R[i].rc) return fail(R[i].rc, R[i].err);
    uint64_t lost = 0;
    for (uint32_t i = 0; i < P.n_dev; ++i) lost += R[i].stats[3];
    if (lost == 0 || attempt == 3) break;
    for (uint32_t i = 0; i < P.n_dev; ++i)
      if (R[i].stats[3])
        if (int rc = grt_hit_pool_reserve(scene, devs[i], 0, nullptr)) return rc;
  }
  uint64_t nsel = 0;
  if (stats) {
    for (uint32_t i = 0; i < P.n_dev; ++i) {
      stats->accepted_steps += R[i].stats[0];
      stats->attempts += R[i].stats[1];
      stats->rays += R[i].stats[2];
      stats->hit_overflows += R[i].stats[3];
      stats->kernel_ms = std::max(stats->kernel_ms, (double)R[i].trace_ms);
    }
  }
  for (uint32_t i = 0; i < P.n_dev; ++i) nsel += R[i].n_sel;
  if (n_supersampled) *n_supersampled = nsel;
  if (failures && failures->capacity && failures->pixel && failures->status) {
    // every device's failed sub-samples (frame pixel indices), sorted by (pixel, sample)
    struct E {
      uint32_t pix, smp, steps;
      uint8_t status, stop;
    };
    std::vector<E> all;
    uint64_t count = 0;
    for (uint32_t i = 0; i < P.n_dev; ++i) {
      count += R[i].f_count;
      const uint64_t m = std::min<uint64_t>(R[i].f_count, R[i].f_pix.size());
      for (uint64_t k = 0; k < m; ++k)
        all.push_back(E{R[i].f_pix[k], R[i].f_smp[k], R[i].f_steps.empty() ? 0u : R[i].f_steps[k], R[i].f_status[k],
                        R[i].f_stop.empty() ? (uint8_t)0 : R[i].f_stop[k]});
    }
    std::sort(all.begin(), all.end(), [](const E& a, const E& b) { return a.pix != b.pix ? a.pix < b.pix : a.smp < b.smp; });
    const uint64_t m = std::min<uint64_t>(all.size(), failures->capacity);
    for (uint64_t k = 0; k < m; ++k) {
      failures->pixel[k] = all[k].pix;
      if (failures->sample) failures->sample[k] = all[k].smp;
      failures->status[k] = all[k].status;
      if (failures->stop) failures->stop[k] = all[k].stop;
      if (failures->steps) failures->steps[k] = all[k].steps;
    }
    failures->count = count;
  }
  if (report) {
    std::memset(report, 0, sizeof(*report));
    report->n_devices = P.n_dev;
    uint32_t rb = 0;
    for (int f = 0; f < grt::RF_N; ++f)
      if (P.mask & (1u << f)) rb += grt::rec_field_bytes(f);
    report->record_bytes = rb;
    report->attempts = attempt;
    report->transport = (uint32_t)P.transport;
    report->gather_ms = R[0].gather_ms;
    for (uint32_t i = 0; i < P.n_dev; ++i) {
      report->trace_ms[i] = R[i].trace_ms;
      report->accepted_steps[i] = R[i].stats[0];
      report->rows[i] = P.cols ? P.n_local[i] / P.cols : 0;
      report->allgather_ms = std::max(report->allgather_ms, (double)R[i].ag_ms);
    }
    report->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return 0;
}

int grt_gbuffer_trace_multi(grt_scene* scene, int n_devices, const int* devices, uint32_t band_rows,
                            grt_gbuffer** out, grt_stats* stats, grt_gbuffer_multi_report* report) {
  const auto t0 = std::chrono::steady_clock::now();
  if (out) *out = nullptr;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (report) std::memset(report, 0, sizeof(*report));
  if (!scene || !devices || !out) return fail(-EINVAL, "null argument");
  if (band_rows == 0) return fail(-EINVAL, "band_rows must be >= 1");
  const int transport = g_transport.load();
  std::vector<int> devs;
  if (int rc = check_devices(n_devices, devices, transport != GRT_TRANSPORT_RCCL, &devs, -EINVAL)) return rc;
  for (uint32_t k = 0; k < scene->desc.n_objects; ++k)
    if (scene->desc.objects[k].kind == GRT_OBJ_VOLUMETRIC_DISC)
      return fail(-ENOTSUP, "a VolumetricDisc's colour is raymarched: the scene has no geometry buffer");
  GbPlan P;
  P.n_dev = (uint32_t)n_devices;
  P.band = band_rows;
  {
    const int64_t r = scene->desc.camera.rows, c = scene->desc.camera.cols;
    if (r <= 0 || c <= 0 || r > (int64_t)UINT32_MAX || c > (int64_t)UINT32_MAX)
      return fail(-EINVAL, "camera frame size out of range");
    P.rows = (uint32_t)r;
    P.cols = (uint32_t)c;
  }
  if ((uint64_t)P.rows * P.cols + 1 > (uint64_t)INT32_MAX) return fail(-EOVERFLOW, "more than INT_MAX - 1 pixels");
  MultiCtx* C;
  if (int rc = get_ctx(devs, transport, &C)) return rc;
  std::lock_guard<std::mutex> lk(C->mu);
  // a device pair that cannot be mapped: the blocks move by copies
  P.transport = (transport == GRT_TRANSPORT_PEER && !C->peer_mapped) ? GRT_TRANSPORT_PEER_STAGED : transport;
  std::vector<GbResult> R(P.n_dev);
  grt_gbuffer* frame = nullptr;
  {
    Barrier bar(n_devices);
    GbTable T;
    std::vector<std::thread> th;
    for (int i = 1; i < n_devices; ++i)
      th.emplace_back(gbuffer_part, scene, std::ref(*C), std::cref(P), i, std::ref(bar), std::ref(T), std::ref(R[i]),
                      &frame);
    gbuffer_part(scene, *C, P, 0, bar, T, R[0], &frame);
    for (auto& t : th) t.join();
    settle_comms(*C);
  }
  int failed = -1;  // the first rank with an error of its own, else the first that was cancelled
  for (uint32_t i = 0; i < P.n_dev && failed < 0; ++i)
    if (R[i].rc && R[i].rc != -ECANCELED) failed = (int)i;
  for (uint32_t i = 0; i < P.n_dev && failed < 0; ++i)
    if (R[i].rc) failed = (int)i;
  if (failed >= 0) {
    if (frame) (void)grt_gbuffer_destroy(frame);
    return fail(R[failed].rc,
                "rank " + std::to_string(failed) + " (device " + std::to_string(devs[failed]) + "): " + R[failed].err);
  }
  double trace_ms = 0, fill_ms = 0;
  for (uint32_t i = 0; i < P.n_dev; ++i) {
    trace_ms = std::max(trace_ms, (double)R[i].sh.trace_ms);
    fill_ms = std::max(fill_ms, (double)R[i].sh.fill_ms);
  }
  grt_api::gbuffer_set_times(frame, trace_ms, fill_ms + R[0].gather_ms);
  if (stats) {
    for (uint32_t i = 0; i < P.n_dev; ++i) {
      stats->accepted_steps += R[i].sh.acc[0];
      stats->attempts += R[i].sh.acc[1];
      stats->rays += R[i].sh.acc[2];
      stats->hit_overflows += R[i].sh.acc[3];
    }
    stats->kernel_ms = trace_ms;
  }
  if (report) {
    report->n_devices = P.n_dev;
    report->transport = (uint32_t)P.transport;
    report->gather_ms = R[0].gather_ms;
    for (uint32_t i = 0; i < P.n_dev; ++i) {
      report->n_traces[i] = R[i].sh.n_traces;
      report->rows[i] = R[i].sh.block.n / P.cols;
      report->layers[i] = R[i].sh.block.layers;
      report->block_bytes[i] = R[i].sh.block.bytes;
      report->trace_ms[i] = R[i].sh.trace_ms;
      report->fill_ms[i] = R[i].sh.fill_ms;
    }
    report->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  *out = frame;
  return 0;
}

void grt_multi_release(void) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  for (auto& c : g_ctx) {
    std::lock_guard<std::mutex> l2(c->mu);
    const bool have_comms = c->started && c->comm_ready.get().empty();
    for (auto& m : c->d) {
      (void)hipSetDevice(m.device);
      if (m.st) (void)hipStreamSynchronize(m.st);
      if (m.mem) (void)hipFree(m.mem);
      for (auto& e : m.ev)
        if (e) (void)hipEventDestroy(e);
      if (m.st) (void)hipStreamDestroy(m.st);
    }
    if (have_comms)
      for (auto& cm : c->comms) (void)rccl().CommDestroy(cm);
  }
  g_ctx.clear();
}

int grt_set_multi_transport(int mode) {
  if (mode != GRT_TRANSPORT_RCCL && mode != GRT_TRANSPORT_PEER && mode != GRT_TRANSPORT_PEER_STAGED)
    return fail(-EINVAL, "multi-GPU transport must be 0 (RCCL), 1 (peer) or 2 (peer, staged)");
  g_transport.store(mode);
  return 0;
}

int grt_get_multi_transport(void) { return g_transport.load(); }

// Test hook (not in grt_api.h): the next frame of a peer transport fails on `rank` with
// -EIO from host code, before it enqueues anything of `stage` (1: its trace, 2: the
// supersample pass after the allgather, 3: devices[0]'s gather after the last barrier).
// grt_gbuffer_trace_multi honours stages 1 (before the rank's trace) and 3 (after its first
// barrier, before devices[0]'s allocations, the second barrier, the transport and the assembly).
// One-shot: it clears itself when it fires; rank < 0 disarms it.  No GPU state is touched.
int grt_debug_multi_fail(int rank, int stage) {
  if (rank < 0) {
    g_inject.store(-1);
    return 0;
  }
  if (rank >= grt::MULTI_MAX || stage < 1 || stage > 3) return fail(-EINVAL, "multi_fail: bad rank or stage");
  g_inject.store(rank * 4 + stage);
  return 0;
}

// Test hook (not in grt_api.h): the de-interleave of deinterleave_kernel run on the host
// with the same per-pixel source function (gather_source), so that a CPU test can hold
// the frame-order assembly of n_shards gathered blocks to distributed.shard_frame_rows.
// gathered: the blocks of shards 0..n-1 back to back, each laid out for `mask`
// (grt_debug_gather_block_bytes); dst[f] (nullable): frame-order output of field f.
int grt_debug_deinterleave_host(uint32_t rows, uint32_t cols, uint32_t band_rows, uint32_t n_shards, uint32_t mask,
                                const uint8_t* gathered, uint8_t* const* dst) {
  if (!gathered || !dst || n_shards == 0 || n_shards > (uint32_t)grt::MULTI_MAX || band_rows == 0 || mask >= 64u)
    return fail(-EINVAL, "deinterleave: bad argument");
  Plan P;
  P.rows = rows;
  P.cols = cols;
  P.band = band_rows;
  P.n_dev = n_shards;
  P.mask = mask;
  uint64_t off = 0;
  for (uint32_t s = 0; s < n_shards; ++s) {
    grt_row_shard sh{band_rows, s, n_shards};
    P.n_local[s] = (uint64_t)grt_shard_row_count(rows, &sh) * cols;
    P.block[s] = field_offset(mask, P.n_local[s], grt::RF_N);
    P.block_off[s] = off;
    off += P.block[s];
  }
  P.block_off[n_shards] = off;
  const grt::GatherLayout L = gather_layout(P);
  for (int f = 0, k = 0; f < grt::RF_N; ++f) {
    if (!(mask & (1u << f))) continue;
    const uint32_t e = L.elem[k];
    if (dst[f])
      for (uint64_t p = 0; p < L.n_pixels; ++p) std::memcpy(dst[f] + p * e, gathered + grt::gather_source(L, k, p), e);
    ++k;
  }
  return 0;
}

// Test hook (not in grt_api.h): gather_peer_kernel's assembly run on the host with the
// same per-pixel source function (gather_source_of) and layout (gather_layout, in place):
// blocks[s] is shard s's block as its owner holds it, an allocation of its own (unused for
// a shard without rows); dst[f] as for grt_debug_deinterleave_host.
int grt_debug_gather_peer_host(uint32_t rows, uint32_t cols, uint32_t band_rows, uint32_t n_shards, uint32_t mask,
                               const uint8_t* const* blocks, uint8_t* const* dst) {
  if (!blocks || !dst || n_shards == 0 || n_shards > (uint32_t)grt::MULTI_MAX || band_rows == 0 || mask >= 64u)
    return fail(-EINVAL, "gather_peer: bad argument");
  Plan P;
  P.rows = rows;
  P.cols = cols;
  P.band = band_rows;
  P.n_dev = n_shards;
  P.mask = mask;
  for (uint32_t s = 0; s < n_shards; ++s) {
    grt_row_shard sh{band_rows, s, n_shards};
    P.n_local[s] = (uint64_t)grt_shard_row_count(rows, &sh) * cols;
    if (P.n_local[s] && !blocks[s]) return fail(-EINVAL, "gather_peer: a shard with rows has no block");
  }
  const grt::GatherLayout L = gather_layout(P, true);
  for (int f = 0, k = 0; f < grt::RF_N; ++f) {
    if (!(mask & (1u << f))) continue;
    const uint32_t e = L.elem[k];
    if (dst[f])
      for (uint64_t p = 0; p < L.n_pixels; ++p) {
        uint32_t s;
        const uint64_t off = grt::gather_source_of(L, k, p, &s);
        std::memcpy(dst[f] + p * e, blocks[s] + off, e);
      }
    ++k;
  }
  return 0;
}

// Test hook (not in grt_api.h): the assembly of grt_gbuffer_trace_multi run on the host with
// the two kernels' index functions (gbuffer_gather_pixel, gbuffer_gather_layer) in plain
// loops, the counterpart of grt_debug_gather_peer_host.  shards[s]: shard s's twelve arrays
// as its rank holds them, local order, n_local[s] pixels (unused for a shard without rows);
// frame: the frame's arrays, rows * cols pixels and as many layers as the shards hold.
int grt_debug_gbuffer_gather_host(uint32_t rows, uint32_t cols, uint32_t band_rows, uint32_t n_shards,
                                  const grt_gbuffer_arrays* shards, const uint64_t* n_local,
                                  const grt_gbuffer_arrays* frame) {
  if (!shards || !n_local || !frame || n_shards == 0 || n_shards > (uint32_t)grt::MULTI_MAX || band_rows == 0)
    return fail(-EINVAL, "gbuffer_gather: bad argument");
  const grt_host::GBufferPtrs F(*frame);
  grt::GBufferGatherShape G{rows, cols, band_rows, n_shards, (uint64_t)rows * cols, 0};
  grt::GBufferGatherSrc S{};
  for (uint32_t s = 0; s < n_shards; ++s) {
    grt_row_shard sh{band_rows, s, n_shards};
    if (n_local[s] != (uint64_t)grt_shard_row_count(rows, &sh) * cols)
      return fail(-EINVAL, "gbuffer_gather: n_local is not the shard's pixel count");
    if (n_local[s] == 0) continue;
    const grt_host::GBufferPtrs P(shards[s]);
    if (P.missing(false)) return fail(-EINVAL, "gbuffer_gather: a shard with rows has a null array");
    for (int k = 0; k < grt::GB_FIELDS; ++k) S.p[k][s] = (const uint8_t*)P.p[k];
    G.n_layers += shards[s].layer_start[n_local[s]];
  }
  if (F.missing(false) || (G.n_layers && F.missing(true))) return fail(-EINVAL, "gbuffer_gather: null frame array");
  uint64_t* start = frame->layer_start;
  uint64_t sum = 0;
  for (uint64_t p = 0; p < G.n_pixels; ++p) {  // gbuffer_gather_pixels_kernel, then the scan
    uint32_t s;
    const uint64_t lp = grt::gbuffer_gather_pixel(G, p, &s);
    for (int k = 0; k < grt::GB_FIELDS; ++k) {
      const grt_host::GBufferField& f = grt_host::GBUFFER_FIELDS[k];
      if (f.layer || k == grt_host::GB_layer_start) continue;
      std::memcpy((uint8_t*)F.p[k] + p * f.size, S.p[k][s] + lp * f.size, f.size);
    }
    const uint64_t* ls = (const uint64_t*)S.p[grt_host::GB_layer_start][s];
    start[p] = sum;
    sum += ls[lp + 1] - ls[lp];
  }
  start[G.n_pixels] = sum;
  if (sum != G.n_layers) return fail(-EIO, "gbuffer_gather: the frame's layer offsets do not end at the shards' total");
  for (int y = 0; y < grt::GB_GATHER_LAYER_FIELDS; ++y) {  // gbuffer_gather_layers_kernel
    const int k = grt::gbuffer_gather_layer_field(y);
    const uint32_t e = grt_host::GBUFFER_FIELDS[k].size;
    for (uint64_t q = 0; q < G.n_layers; ++q) {
      uint32_t s;
      const uint64_t j = grt::gbuffer_gather_layer(G, start, S, q, &s);
      std::memcpy((uint8_t*)F.p[k] + q * e, S.p[k][s] + j * e, e);
    }
  }
  return 0;
}

// Test hook (not in grt_api.h): bytes of a device's send block of n pixels for `mask`,
// and each field's offset in it (offsets[6], ~0 for a field not in the mask).
uint64_t grt_debug_gather_block_bytes(uint32_t mask, uint64_t n, uint64_t* offsets) {
  for (int f = 0; f < grt::RF_N; ++f)
    if (offsets) offsets[f] = (mask & (1u << f)) ? field_offset(mask, n, f) : ~0ull;
  return field_offset(mask, n, grt::RF_N);
}

}  // extern "C"
