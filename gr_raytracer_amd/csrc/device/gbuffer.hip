// gbuffer.hip — layer offsets of a geometry buffer (grt_gbuffer_trace), and the bookkeeping
// of its sub-sample set (grt_gbuffer_supersample, grt_gbuffer_shade_section): the split of
// a selection into held and missing pixels (of one buffer, or of a stack of buffers at once:
// grt_gbuffer_shade_section_sequence), the append of a traced chunk, the pixel -> block map
// of an uploaded set; and the assembly of a frame's buffer from the buffers of its row-band
// shards (grt_gbuffer_trace_multi).
//
// A pixel's layers are the window-nearest hits that enter its blend: the trace's own
// `hits` output, and none for a pixel the trace aborted (status != 0).  The offsets are
// the exclusive prefix sum of those counts (hipCUB), over n + 1 entries so that the last
// one is the total.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>

#include "kernels.h"
#include "gbuffer_gather.h"

namespace grt {

__global__ void __launch_bounds__(256) gbuffer_count_kernel(const uint8_t* __restrict__ status,
                                                            const uint32_t* __restrict__ hits, uint64_t n,
                                                            uint64_t* __restrict__ counts) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  counts[i] = (i < n && status[i] == 0) ? (uint64_t)hits[i] : 0ull;
}

hipError_t gbuffer_layer_scan(const uint8_t* d_status, const uint32_t* d_hits, uint64_t n, uint64_t* d_counts,
                              uint64_t* d_layer_start, void* d_temp, size_t* temp_bytes, hipStream_t stream) {
  if (n + 1 > (uint64_t)INT_MAX) return hipErrorInvalidValue;
  if (d_temp == nullptr)
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *temp_bytes, d_counts, d_layer_start, (int)(n + 1), stream);
  hipLaunchKernelGGL(gbuffer_count_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, d_status, d_hits,
                     n, d_counts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceScan::ExclusiveSum(d_temp, *temp_bytes, d_counts, d_layer_start, (int)(n + 1), stream);
}

// ---- a stacked buffer cut into its frames (grt_gbuffer_trace_sequence) ----
// The scan above runs over the whole stack; a frame's own offsets start at 0 at its first
// pixel.
__global__ void __launch_bounds__(256) gbuffer_rebase_kernel(const uint64_t* __restrict__ stack_start, uint64_t n,
                                                             uint64_t* __restrict__ frame_start) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) frame_start[i] = stack_start[i] - stack_start[0];
}

hipError_t gbuffer_rebase(const uint64_t* d_stack_start, uint64_t n, uint64_t* d_frame_start, hipStream_t stream) {
  hipLaunchKernelGGL(gbuffer_rebase_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, d_stack_start,
                     n, d_frame_start);
  return hipGetLastError();
}

// ---- the sub-sample set (grt_gbuffer_supersample, grt_gbuffer_shade_section) ----
// held[j] / missing[j]: whether selected pixel j has a block; 0 past the selection's end.
__global__ void __launch_bounds__(256) gbuffer_split_flags_kernel(const uint32_t* __restrict__ sel,
                                                                  const unsigned long long* __restrict__ d_count,
                                                                  uint64_t n_max, const uint32_t* __restrict__ sub_block,
                                                                  uint8_t* __restrict__ held,
                                                                  uint8_t* __restrict__ missing) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_max) return;
  const bool live = j < *d_count;
  const bool has = live && sub_block[sel[j]] != GBUFFER_NIL;
  held[j] = has ? 1 : 0;
  missing[j] = (live && !has) ? 1 : 0;
}

// An ordered compaction of each flag array (DeviceSelect::Flagged, as compact_flags): the
// lists keep the selection's ascending pixel order, so a top-up appends the same bytes
// every time.
hipError_t gbuffer_split(const uint32_t* d_sel, const unsigned long long* d_count, uint64_t n_max,
                         const uint32_t* d_sub_block, uint8_t* d_flags, uint32_t* d_held,
                         unsigned long long* d_n_held, uint32_t* d_missing, unsigned long long* d_n_missing,
                         void* d_temp, size_t* temp_bytes, hipStream_t stream) {
  if (n_max > (uint64_t)INT_MAX) return hipErrorInvalidValue;
  if (d_temp == nullptr)
    return hipcub::DeviceSelect::Flagged(nullptr, *temp_bytes, d_sel, d_flags, d_held, d_n_held, (int)n_max, stream);
  if (n_max == 0) return hipSuccess;
  hipLaunchKernelGGL(gbuffer_split_flags_kernel, dim3((unsigned)((n_max + 255) / 256)), dim3(256), 0, stream, d_sel,
                     d_count, n_max, d_sub_block, d_flags, d_flags + n_max);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipcub::DeviceSelect::Flagged(d_temp, *temp_bytes, d_sel, d_flags, d_held, d_n_held, (int)n_max, stream);
  if (e != hipSuccess) return e;
  return hipcub::DeviceSelect::Flagged(d_temp, *temp_bytes, d_sel, d_flags + n_max, d_missing, d_n_missing, (int)n_max,
                                       stream);
}

// The same over the selections of a stack of buffers (grt_gbuffer_shade_section_sequence):
// slot i = f * npix + j is entry j of frame f's selection, live while j < cnt[4 f], and is
// looked up in that frame's own sub_block.  stack[i] is the entry as a stacked index
// f * npix + pixel; cnt[4 f + 2] / cnt[4 f + 3] count the frame's held / missing pixels.
__global__ void __launch_bounds__(256) gbuffer_split_stack_flags_kernel(const uint32_t* __restrict__ sel,
                                                                        unsigned long long* __restrict__ cnt,
                                                                        uint32_t n_frames, uint64_t npix,
                                                                        const GBufferSubFrame* __restrict__ frames,
                                                                        uint8_t* __restrict__ held,
                                                                        uint8_t* __restrict__ missing,
                                                                        uint32_t* __restrict__ stack) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_frames * npix) return;
  const uint64_t f = i / npix, j = i - f * npix;
  const bool live = j < cnt[4 * f];
  const uint32_t p = live ? sel[i] : 0u;
  const bool has = live && p < npix && frames[f].sub_block[p] != GBUFFER_NIL;
  held[i] = has ? 1 : 0;
  missing[i] = (live && !has) ? 1 : 0;
  stack[i] = (uint32_t)(f * npix + p);
  if (live) atomicAdd(&cnt[4 * f + (has ? 2 : 3)], 1ull);
}

// Two ordered compactions, as gbuffer_split: slot order is frame-major and a frame's
// selection ascends, so each list ascends in the stacked index.
hipError_t gbuffer_split_stack(const uint32_t* d_sel, unsigned long long* d_cnt, uint32_t n_frames, uint64_t npix,
                               const GBufferSubFrame* d_frames, uint8_t* d_flags, uint32_t* d_stack, uint32_t* d_held,
                               unsigned long long* d_n_held, uint32_t* d_missing, unsigned long long* d_n_missing,
                               void* d_temp, size_t* temp_bytes, hipStream_t stream) {
  const uint64_t m = (uint64_t)n_frames * npix;
  if (m > (uint64_t)INT_MAX) return hipErrorInvalidValue;
  if (d_temp == nullptr)
    return hipcub::DeviceSelect::Flagged(nullptr, *temp_bytes, d_stack, d_flags, d_held, d_n_held, (int)m, stream);
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(gbuffer_split_stack_flags_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, d_sel,
                     d_cnt, n_frames, npix, d_frames, d_flags, d_flags + m, d_stack);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipcub::DeviceSelect::Flagged(d_temp, *temp_bytes, d_stack, d_flags, d_held, d_n_held, (int)m, stream);
  if (e != hipSuccess) return e;
  return hipcub::DeviceSelect::Flagged(d_temp, *temp_bytes, d_stack, d_flags + m, d_missing, d_n_missing, (int)m,
                                       stream);
}

__global__ void __launch_bounds__(256) gbuffer_sub_append_kernel(const uint64_t* __restrict__ local, uint64_t n_rays,
                                                                 uint64_t layer_base, uint64_t* __restrict__ layer_start,
                                                                 const uint32_t* __restrict__ pixels, uint64_t n_pixels,
                                                                 uint32_t first_block, uint32_t* __restrict__ sub_block,
                                                                 uint32_t* __restrict__ sub_pixel) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n_rays) layer_start[i] = local[i] + layer_base;
  if (i < n_pixels) {
    const uint32_t p = pixels[i];
    sub_block[p] = first_block + (uint32_t)i;
    sub_pixel[first_block + i] = p;
  }
}

hipError_t gbuffer_sub_append(const uint64_t* d_local, uint64_t n_rays, uint64_t layer_base, uint64_t* d_layer_start,
                              const uint32_t* d_pixels, uint64_t n_pixels, uint32_t first_block, uint32_t* d_sub_block,
                              uint32_t* d_sub_pixel, hipStream_t stream) {
  const uint64_t n = (n_rays + 1 > n_pixels) ? n_rays + 1 : n_pixels;
  hipLaunchKernelGGL(gbuffer_sub_append_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_local, n_rays,
                     layer_base, d_layer_start, d_pixels, n_pixels, first_block, d_sub_block, d_sub_pixel);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) gbuffer_sub_index_kernel(const uint32_t* __restrict__ sub_pixel, uint64_t n_sub,
                                                                uint32_t* __restrict__ sub_block) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_sub) sub_block[sub_pixel[j]] = (uint32_t)j;
}

hipError_t gbuffer_sub_index(const uint32_t* d_sub_pixel, uint64_t n_sub_pixels, uint64_t n_pixels,
                             uint32_t* d_sub_block, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_sub_block, 0xff, 4 * n_pixels, stream);  // GBUFFER_NIL
  if (e != hipSuccess || n_sub_pixels == 0) return e;
  hipLaunchKernelGGL(gbuffer_sub_index_kernel, dim3((unsigned)((n_sub_pixels + 255) / 256)), dim3(256), 0, stream,
                     d_sub_pixel, n_sub_pixels, d_sub_block);
  return hipGetLastError();
}

// ---- a frame's buffer from its row-band shards (grt_gbuffer_trace_multi, gbuffer_gather.h) ----
// Frame order from local order, a grid-stride loop over the frame's pixels: consecutive
// pixels of a band row are consecutive in their shard, so a wave reads contiguous runs of a
// row of each array (another GPU's, over xGMI, under the peer transport) and writes
// contiguous ones.  The pixel's layer count is the difference of its owner's offsets; entry
// n_pixels of the counts is the scan's extra 0.
using grt_host::GB_layer_start;
using grt_host::GB_object;
using grt_host::GB_sky_redshift;
using grt_host::GB_sky_u;
using grt_host::GB_sky_v;
using grt_host::GB_status;
using grt_host::GB_steps;
using grt_host::GB_stop;

__global__ void __launch_bounds__(256) gbuffer_gather_pixels_kernel(GBufferGatherShape G, GBufferGatherSrc S,
                                                                    GBufferGatherDst D,
                                                                    uint64_t* __restrict__ counts) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= G.n_pixels;
       p += (uint64_t)gridDim.x * blockDim.x) {
    if (p == G.n_pixels) {
      counts[p] = 0;
      continue;
    }
    uint32_t s;
    const uint64_t lp = gbuffer_gather_pixel(G, p, &s);
    D.p[GB_status][p] = S.p[GB_status][s][lp];
    D.p[GB_stop][p] = S.p[GB_stop][s][lp];
    ((uint32_t*)D.p[GB_steps])[p] = ((const uint32_t*)S.p[GB_steps][s])[lp];
    ((uint64_t*)D.p[GB_sky_u])[p] = ((const uint64_t*)S.p[GB_sky_u][s])[lp];
    ((uint64_t*)D.p[GB_sky_v])[p] = ((const uint64_t*)S.p[GB_sky_v][s])[lp];
    ((uint64_t*)D.p[GB_sky_redshift])[p] = ((const uint64_t*)S.p[GB_sky_redshift][s])[lp];
    const uint64_t* ls = (const uint64_t*)S.p[GB_layer_start][s];
    counts[p] = ls[lp + 1] - ls[lp];
  }
}

hipError_t launch_gbuffer_gather_pixels(const GBufferGatherShape& G, const GBufferGatherSrc& S,
                                        const GBufferGatherDst& D, uint64_t* d_counts, hipStream_t stream) {
  const unsigned gx = (unsigned)((G.n_pixels + 1 + 255) / 256 < 8192 ? (G.n_pixels + 1 + 255) / 256 : 8192);
  hipLaunchKernelGGL(gbuffer_gather_pixels_kernel, dim3(gx), dim3(256), 0, stream, G, S, D, d_counts);
  return hipGetLastError();
}

hipError_t gbuffer_gather_scan(const uint64_t* d_counts, uint64_t n_pixels, uint64_t* d_layer_start, void* d_temp,
                               size_t* temp_bytes, hipStream_t stream) {
  if (n_pixels + 1 > (uint64_t)INT_MAX) return hipErrorInvalidValue;
  return hipcub::DeviceScan::ExclusiveSum(d_temp, *temp_bytes, d_counts, d_layer_start, (int)(n_pixels + 1), stream);
}

// One lane per frame layer and array (blockIdx.y: u, v, redshift, radius, then object), a
// grid-stride loop.  The lanes of a wave lie in one band or in a few consecutive ones, so
// they read and write consecutive elements (8 B each, 1 B for `object`); the bisection's
// probes are the same for most of a wave (at most log2 of the band count, 12 at 4096 bands).
__global__ void __launch_bounds__(256) gbuffer_gather_layers_kernel(GBufferGatherShape G, GBufferGatherSrc S,
                                                                    GBufferGatherDst D) {
  const int k = gbuffer_gather_layer_field((int)blockIdx.y);
  const uint64_t* __restrict__ frame_start = (const uint64_t*)D.p[GB_layer_start];
  uint8_t* __restrict__ out = D.p[k];
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < G.n_layers;
       q += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t s;
    const uint64_t j = gbuffer_gather_layer(G, frame_start, S, q, &s);
    const uint8_t* __restrict__ src = S.p[k][s];
    if (k == GB_object) out[q] = src[j];
    else ((uint64_t*)out)[q] = ((const uint64_t*)src)[j];
  }
}

hipError_t launch_gbuffer_gather_layers(const GBufferGatherShape& G, const GBufferGatherSrc& S,
                                        const GBufferGatherDst& D, hipStream_t stream) {
  if (G.n_layers == 0) return hipSuccess;
  const uint64_t want = (G.n_layers + 255) / 256;
  const unsigned gx = (unsigned)(want < 8192 ? want : 8192);
  hipLaunchKernelGGL(gbuffer_gather_layers_kernel, dim3(gx, GB_GATHER_LAYER_FIELDS), dim3(256), 0, stream, G, S, D);
  return hipGetLastError();
}

}  // namespace grt
