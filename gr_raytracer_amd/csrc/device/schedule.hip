// schedule.hip — tile queue order for the persistent integrate kernel.
//
// Pixels cost very different amounts: in Kerr-Schild (C4) the rays that fall into the
// horizon take ~5e5 accepted steps and the trapped ones the full max_steps (1e6),
// while an escaping ray takes ~1.6e4.  The integrate kernel hands out 8x8 tiles from
// one counter, so a long tile queued late ends the frame on a single busy lane.  The
// probe kernel (geodesic_probe.h) traces one ray per tile for a capped number of steps (a
// probe still going at the cap gets a key above the cap from its state there); here each
// tile's key is the largest probe key in its 3x3 tile neighbourhood (a shadow edge can
// cut a tile whose probe pixel escapes; edge tiles get more, below), and the tiles are sorted by
// key, descending and stable (row-major among equals), with hipCUB's radix sort.  The
// order changes which lane traces a pixel, never its result.
//
// Schwarzschild frames ordered by impact parameter (impact_key_kernel) also group their
// tiles by the case the RHS's sincos takes in the far field (tile_class below), so that
// the 64 lanes of a wave, which hold rays of a few consecutive queue tiles, agree on it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "kernels.h"

namespace grt {

// Edge tiles (own probe finished, a neighbour's capped: the tile straddles the border of
// a long-ray region) get twice the neighbour's excess over the cap.  The rays that graze
// that border run longer than the ones inside it: in a C4 shard the edge tiles' longest
// rays reach 0.9-1.9x the neighbour's prediction at the 90th-99th percentile, and a tile
// of 6e5-step rays queued by its neighbour's key ended the shard 2 s after the rest
// (profiles/r04d); most edge tiles are short, so queueing them early costs little.
__global__ void __launch_bounds__(256) dilate_kernel(const uint32_t* __restrict__ probe, uint32_t tiles_x,
                                                     uint32_t tiles_y, uint32_t cap, uint32_t* __restrict__ keys,
                                                     uint32_t* __restrict__ idx) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tiles_x * tiles_y) return;
  const int tr = (int)(t / tiles_x), tc = (int)(t % tiles_x);
  uint32_t k = 0;
  for (int dr = -1; dr <= 1; ++dr)
    for (int dc = -1; dc <= 1; ++dc) {
      const int r = tr + dr, c = tc + dc;
      if (r >= 0 && r < (int)tiles_y && c >= 0 && c < (int)tiles_x) k = max(k, probe[(uint32_t)r * tiles_x + c]);
    }
  if (probe[t] < cap && k > cap) {
    const uint64_t boosted = (uint64_t)cap + 2ull * (uint64_t)(k - cap);
    k = boosted > 0xffffffffull ? 0xffffffffu : (uint32_t)boosted;
  }
  keys[t] = k;
  idx[t] = t;
}

// Sincos class of a tile, from the predicted pi/2 - theta_f of its four corner pixels
// (class_key_kernel, geodesic_probe.h): the case the RHS's sincos takes over the ~97% of an
// escaping ray's steps that lie in the far field.
//   0: every corner in the Taylor case (|pi/2 - theta_f| < TAYLOR_MAX);
//   2: every corner in region B's table case, all on one side of the Taylor band;
//   3: every corner captured or outside region B (theta_f below 0x3feb6000's 0.855469 or
//      from 0x400368fd's 2.426265 on);
//   1: anything else, the tiles that straddle a border.
// The margin is two pixels' worth of angle: a quarter of the spread of theta_f over the
// tile's 8 pixels (lensing stretches it, so it is taken from the corners themselves).
constexpr float CLASS_TAYLOR_MAX = 0.126f;  // glibc_tables.h TAYLOR_MAX
constexpr float CLASS_B_HI = 0.71532758f, CLASS_B_LO = -0.85546748f;  // pi/2 - 0.85546875, pi/2 - 2.42626381
__device__ inline uint32_t tile_class(const float* __restrict__ a, uint32_t tr, uint32_t tc, uint32_t tiles_x) {
  const uint32_t cx = tiles_x + 1;
  const float v[4] = {a[tr * cx + tc], a[tr * cx + tc + 1], a[(tr + 1) * cx + tc], a[(tr + 1) * cx + tc + 1]};
  float lo = 1e30f, hi = -1e30f;  // over the escaping corners inside region B
  int n_out = 0;
  for (int k = 0; k < 4; ++k) {
    if (v[k] != v[k]) return 1;  // undecided corner
    if (v[k] > CLASS_B_LO && v[k] < CLASS_B_HI) {
      lo = fminf(lo, v[k]);
      hi = fmaxf(hi, v[k]);
    } else {
      ++n_out;
    }
  }
  if (n_out == 4) return 3;
  if (n_out != 0) return 1;
  const float m = 0.25f * (hi - lo);
  if (lo - m <= CLASS_B_LO || hi + m >= CLASS_B_HI) return 1;
  if (fmaxf(fabsf(lo), fabsf(hi)) + m < CLASS_TAYLOR_MAX) return 0;
  if (lo - m > CLASS_TAYLOR_MAX || hi + m < -CLASS_TAYLOR_MAX) return 2;
  return 1;
}

// The composite key: the dilated length in LEN_BUCKET steps as the major part, so that
// the near-critical tiles (hundreds to thousands of steps more than an escaping ray's
// max_radius) still come first, longest first; below it the class, 0 first.  Lengths
// closer than a bucket (a fifteenth of a C2 ray) are told apart by class alone: the
// impact keys of the tiles with b < 2 b_c differ by a few steps from ring to ring round
// the shadow, and a ring crosses every class.  Row-major among equals (the sort is stable).
constexpr uint32_t LEN_BUCKET_SHIFT = 10;
__global__ void __launch_bounds__(256) class_compose_kernel(const float* __restrict__ corner_a, uint32_t tiles_x,
                                                            uint32_t tiles_y, uint32_t* __restrict__ keys,
                                                            uint8_t* __restrict__ cls_out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tiles_x * tiles_y) return;
  const uint32_t cls = tile_class(corner_a, t / tiles_x, t % tiles_x, tiles_x);
  keys[t] = ((keys[t] >> LEN_BUCKET_SHIFT) << 2) | (3u - cls);
  if (cls_out) cls_out[t] = (uint8_t)cls;
}

hipError_t launch_tile_order(const uint32_t* d_probe, uint32_t tiles_x, uint32_t tiles_y, uint32_t cap, uint32_t* d_keys,
                             uint32_t* d_keys_sorted, uint32_t* d_idx, uint32_t* d_order, void* temp,
                             size_t* temp_bytes, hipStream_t stream, const float* d_corner_a, uint8_t* d_class) {
  const uint32_t n = tiles_x * tiles_y;
  if (temp == nullptr)
    return hipcub::DeviceRadixSort::SortPairsDescending(nullptr, *temp_bytes, d_keys, d_keys_sorted, d_idx, d_order,
                                                        (int)n, 0, 32, stream);
  hipLaunchKernelGGL(dilate_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_probe, tiles_x, tiles_y, cap,
                     d_keys, d_idx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (d_corner_a) {
    hipLaunchKernelGGL(class_compose_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_corner_a, tiles_x, tiles_y,
                       d_keys, d_class);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipcub::DeviceRadixSort::SortPairsDescending(temp, *temp_bytes, d_keys, d_keys_sorted, d_idx, d_order, (int)n,
                                                      0, 32, stream);
}

}  // namespace grt
