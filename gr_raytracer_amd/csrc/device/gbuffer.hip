// gbuffer.hip — layer offsets of a geometry buffer (grt_gbuffer_trace).
//
// A pixel's layers are the window-nearest hits that enter its blend: the trace's own
// `hits` output, and none for a pixel the trace aborted (status != 0).  The offsets are
// the exclusive prefix sum of those counts (hipCUB), over n + 1 entries so that the last
// one is the total.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>

#include "kernels.h"

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

}  // namespace grt
