// gbuffer_gather.h — a frame's geometry buffer assembled from the buffers of its row-band
// shards (grt_gbuffer_trace_multi, multi.hip): the shapes the two kernels of gbuffer.hip
// take, and their index arithmetic, which the host twin (grt_debug_gbuffer_gather_host)
// runs in plain loops.
//
// Shard s holds the frame's bands s, s + N, ... (grt_row_shard) local-row-major, each with
// its own layer_start from 0.  A band's pixels are contiguous in the frame and in their
// owner, and layers are pixel-major, so a band's layers are one contiguous run in both: a
// frame pixel is found from its row (frame_row_source), a frame layer from its band.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/host_internal.h"
#include "dev_scene.h"

namespace grt {

constexpr int GB_FIELDS = grt_host::GB_N_FIELDS;
constexpr int GB_GATHER_MAX = GRT_MULTI_MAX_DEVICES;

struct GBufferGatherShape {
  uint32_t rows, cols, band_rows, n_shards;
  uint64_t n_pixels, n_layers;  // of the frame
};
// p[k][s]: array k (GRT_GBUFFER_FIELDS' order) of shard s, where its owner left it or in the
// reader's staging; unused for a shard without rows.
struct GBufferGatherSrc {
  const uint8_t* p[GB_FIELDS][GB_GATHER_MAX];
};
struct GBufferGatherDst {
  uint8_t* p[GB_FIELDS];  // the frame's arrays
};

// The layer arrays in the order of gbuffer_gather_layers_kernel's blockIdx.y, and their
// element sizes: the 8-byte ones, then `object`.
constexpr int GB_GATHER_LAYER_FIELDS = 5;
__host__ __device__ constexpr int gbuffer_gather_layer_field(int y) {
  return y == 0   ? (int)grt_host::GB_u
         : y == 1 ? (int)grt_host::GB_v
         : y == 2 ? (int)grt_host::GB_redshift
         : y == 3 ? (int)grt_host::GB_radius
                  : (int)grt_host::GB_object;
}
constexpr bool gbuffer_gather_fields_ok() {
  int layer = 0;
  for (int k = 0; k < GB_FIELDS; ++k) layer += grt_host::GBUFFER_FIELDS[k].layer ? 1 : 0;
  if (layer != GB_GATHER_LAYER_FIELDS) return false;
  for (int y = 0; y < GB_GATHER_LAYER_FIELDS; ++y) {
    const grt_host::GBufferField f = grt_host::GBUFFER_FIELDS[gbuffer_gather_layer_field(y)];
    if (!f.layer || f.size != (y < 4 ? 8u : 1u)) return false;
  }
  return true;
}
static_assert(gbuffer_gather_fields_ok(), "the layer arrays of GRT_GBUFFER_FIELDS are u, v, redshift, radius and object");

// Frame pixel p: the shard that holds it, and its index in that shard's per-pixel arrays.
__host__ __device__ inline uint64_t gbuffer_gather_pixel(const GBufferGatherShape& G, uint64_t p, uint32_t* shard) {
  const uint32_t row = (uint32_t)(p / G.cols), col = (uint32_t)(p % G.cols);
  uint32_t lr;
  frame_row_source(G.band_rows, G.n_shards, row, shard, &lr);
  return (uint64_t)lr * G.cols + col;
}

// Frame layer q < n_layers: the shard that holds it, and its index in that shard's layer
// arrays.  frame_start is the frame's layer_start; q's band b is the one with
// frame_start[first pixel of b] <= q < frame_start[first pixel of b + 1], found by bisecting
// over the band-first pixels (a band without layers is never the answer); the source is
// shard b % N, at its own layer_start of the band's first local pixel plus q's place in the band.
__host__ __device__ inline uint64_t gbuffer_gather_layer(const GBufferGatherShape& G, const uint64_t* frame_start,
                                                         const GBufferGatherSrc& S, uint64_t q, uint32_t* shard) {
  if (G.n_shards <= 1) {
    *shard = 0;
    return q;
  }
  const uint64_t band_px = (uint64_t)G.band_rows * G.cols;
  uint64_t lo = 0, hi = ((uint64_t)G.rows + G.band_rows - 1) / G.band_rows;  // frame_start[n_pixels] > q
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (frame_start[mid * band_px] <= q) lo = mid;
    else hi = mid;
  }
  const uint32_t s = (uint32_t)(lo % G.n_shards);
  *shard = s;
  const uint64_t* local_start = (const uint64_t*)S.p[grt_host::GB_layer_start][s];
  return local_start[(lo / G.n_shards) * band_px] + (q - frame_start[lo * band_px]);
}

// gbuffer_gather_pixels_kernel on `stream`: the six per-pixel arrays of the frame from the
// shards', and d_counts[p] = the pixel's layer count, d_counts[n_pixels] = 0.
hipError_t launch_gbuffer_gather_pixels(const GBufferGatherShape& G, const GBufferGatherSrc& S,
                                        const GBufferGatherDst& D, uint64_t* d_counts, hipStream_t stream);
// The frame's layer_start from those counts (n_pixels + 1 entries, n_pixels < INT_MAX):
// hipCUB's exclusive sum.  Call with d_temp == NULL for *temp_bytes.
hipError_t gbuffer_gather_scan(const uint64_t* d_counts, uint64_t n_pixels, uint64_t* d_layer_start, void* d_temp,
                               size_t* temp_bytes, hipStream_t stream);
// gbuffer_gather_layers_kernel on `stream`: the five layer arrays of the frame, G.n_layers
// entries each, by the frame's finished layer_start (D.p[GB_layer_start]).
hipError_t launch_gbuffer_gather_layers(const GBufferGatherShape& G, const GBufferGatherSrc& S,
                                        const GBufferGatherDst& D, hipStream_t stream);

}  // namespace grt
