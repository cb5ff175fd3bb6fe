// gbuffer_shade.hip — the deferred shade of a geometry buffer on gfx950.
//
// shade_kernel's window colours, terminal colour and composite from a geometry buffer and
// the appearance scene S (textures, LUTs, temperatures, the celestial sphere, the hit
// threshold) -- no chart, workspace or integrator, one lane per ray.  The operations and
// their order are shade_kernel's (geodesic.hip), through the same helpers (appearance.h), so
// the pixel has its bits.  One ray body (gbuffer_shade_ray) serves every kernel here; a
// kernel finds its ray (`src` in a buffer's arrays), its output slot (`dst`) and, for the
// disc's orbital motion, its time.
//
// Compiled with the flags of the exact build (no contraction).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grt_api.h"
#include "dev_scene.h"
#ifndef GRT_GLIBC_LDS
#define GRT_GLIBC_LDS 1  // glibc tables staged in LDS per workgroup, as in geodesic.hip
#endif
#include "glibc_math.h"
#include "kernels.h"

namespace grt {

#ifndef GDEV
#define GDEV __device__ __forceinline__
#endif

#include "appearance.h"

// ---- the disc's orbital motion (grt_gbuffer_shade_times, grt_gbuffer_shade_section_at) ----
// shade_record's disc emitter moves on a circular orbit with killing_coefficients' omega, so
// a disc texture that orbits at that rate is the animation of the scene being shaded: at
// coordinate time t the matter seen at in-plane angle phi sat at phi - omega t at time 0, and
// disc uv is 0.5 + 0.5 rho (cos phi, sin phi), so the lookup point turns about (0.5, 0.5) by
// -omega t.  "Fast light": every layer of a frame is shaded at the same t, and light-travel delay
// is ignored.  Retarded (grt_gbuffer_shade_times_retarded): a buffer traced with its lapse holds,
// per layer, the coordinate time its light took to the camera, negated, and the layer is shaded
// at its emission time t + lapse.
// The rule is restated on the host with the same operations in the same order
// (host/orbit.cpp: grt_orbit_rate, grt_gbuffer_orbit_uv, grt_gbuffer_orbit_uv_retarded).
//
// d(phi)/dt of the emitter at radius r: killing_coefficients' omega (geodesic.hip), as a
// function of the appearance scene alone; the flat charts' emitter is at rest.
GDEV double orbit_rate(const DevScene& S, double r) {
  if (S.geometry == GRT_GEOM_EUCLIDEAN || S.geometry == GRT_GEOM_EUCLIDEAN_SPHERICAL) return 0.0;
  const double m = 0.5 * S.radius;
  const double sqrt_m = sqrt(m);
  return sqrt_m / (rpow(r, 1.5) + S.a * sqrt_m);
}

GDEV void orbit_uv(double omega, double t, double* u, double* v) {
  const double th = omega * t;
  if (th == 0.0 || !isfinite(th)) return;  // (u, v) unchanged, bit for bit
  double s, c;
  rsincos(th, &s, &c);
  const double du = *u - 0.5, dv = *v - 0.5;
  *u = 0.5 + (du * c + dv * s);
  *v = 0.5 + (dv * c - du * s);
}

// How a shade treats time.  SHADE_STATIC: the buffer as traced (no orbit code at all).
// SHADE_AT: at time t, a disc layer's rate computed where it is used.  SHADE_AT_CACHED: at
// time t, the rate read from omega[k] (gbuffer_orbit_rate_kernel wrote it): the same
// expression either way, so the same bits.  SHADE_RETARDED: SHADE_AT_CACHED with layer k at
// its emission time t + lapse[k] (grt_gbuffer_shade_times_retarded): one add, then orbit_uv.
// SHADE_RETARDED_AT: SHADE_RETARDED with the rate computed where it is used, as SHADE_AT does
// (grt_gbuffer_shade_section_at_retarded): the same expression, so the cached form's bits.
enum ShadeMode { SHADE_STATIC, SHADE_AT, SHADE_AT_CACHED, SHADE_RETARDED, SHADE_RETARDED_AT };

// The colour of layer k.  In the two time modes a disc layer's (u, v) goes through orbit_uv
// before the texture lookup; t and omega are unused in SHADE_STATIC, lapse in every mode but
// the two retarded ones.
template <ShadeMode MODE>
GDEV int gbuffer_layer_color(const DevScene& S, const GBufferArrays& gb, uint64_t k, double t,
                             const double* __restrict__ omega, const double* __restrict__ lapse, XYZA* col) {
  const DevObject& o = S.obj[gb.object[k]];
  double temperature;
  if (o.kind != GRT_OBJ_SPHERE) {
    int e = compute_temperature(o, gb.radius[k], &temperature);
    if (e != GRT_OK) return e;
  } else {
    temperature = o.temperature;
  }
  double u = gb.u[k], v = gb.v[k];
  if constexpr (MODE == SHADE_RETARDED) {
    if (o.kind == GRT_OBJ_DISC) orbit_uv(omega[k], t + lapse[k], &u, &v);
  } else if constexpr (MODE == SHADE_RETARDED_AT) {
    if (o.kind == GRT_OBJ_DISC) orbit_uv(orbit_rate(S, gb.radius[k]), t + lapse[k], &u, &v);
  } else if constexpr (MODE != SHADE_STATIC) {
    if (o.kind == GRT_OBJ_DISC) orbit_uv(MODE == SHADE_AT_CACHED ? omega[k] : orbit_rate(S, gb.radius[k]), t, &u, &v);
  }
  *col = texture_color(S, o.tex, u, v, gb.redshift[k], temperature);
  return GRT_OK;
}

// One ray of a buffer (`src` in gb's arrays) shaded into output slot `dst`.  Two passes over
// the ray's layers: front to back for the opacity, back to front for the blend (each layer's
// colour is evaluated in both; a ray may have any number of layers).
template <ShadeMode MODE>
GDEV void gbuffer_shade_ray(const DevScene& S, const GBufferArrays& gb, uint64_t src, const Outputs& out, uint64_t dst,
                            double t = 0.0, const double* __restrict__ omega = nullptr,
                            const double* __restrict__ lapse = nullptr) {
  const int status = gb.status[src];
  const int stop = gb.stop[src];
  const XYZA fail{0.0, 0.0, 0.0, 1.0};
  if (status != GRT_OK) {
    write_out(out, dst, fail, GRT_CLASS_ESCAPED, status, stop, 0u);
    return;
  }
  const uint64_t l0 = gb.layer_start[src], l1 = gb.layer_start[src + 1];
  double opacity = 0.0;
  for (uint64_t k = l0; k < l1; ++k) {
    XYZA col;
    int e = gbuffer_layer_color<MODE>(S, gb, k, t, omega, lapse, &col);
    if (e != GRT_OK) {  // a temperature error the traced scene did not have: the window error's pixel
      write_out(out, dst, fail, GRT_CLASS_ESCAPED, e, stop, (uint32_t)(k - l0));
      return;
    }
    double alpha = rclamp(col.a, 0.0, 1.0);
    opacity = alpha + opacity * (1.0 - alpha);
  }
  XYZA result{0.0, 0.0, 0.0, 1.0};
  int cls = GRT_CLASS_CAPTURED;
  if (stop == GRT_STOP_HORIZON || stop == GRT_STOP_CLOSED_ORBIT) {
    result = blend(result, XYZA{0.0, 0.0, 0.0, 1.0});
  } else if (stop == GRT_STOP_CELESTIAL) {
    result = blend(result, texture_color(S, S.celestial, gb.sky_u[src], gb.sky_v[src], gb.sky_redshift[src],
                                         S.celestial_temperature));
    cls = GRT_CLASS_ESCAPED;
  }
  for (uint64_t k = l1; k > l0; --k) {
    XYZA col{0.0, 0.0, 0.0, 0.0};
    (void)gbuffer_layer_color<MODE>(S, gb, k - 1, t, omega, lapse, &col);
    result = blend(result, col);
  }
  if (opacity >= S.hit_threshold) cls = GRT_CLASS_HIT;
  write_out(out, dst, result, cls, status, stop, (uint32_t)(l1 - l0));
}

// One lane per pixel of a buffer (grt_gbuffer_shade, the 1-spp pass of grt_gbuffer_shade_section).
__global__ void __launch_bounds__(256) gbuffer_shade_kernel(const DevScene* __restrict__ Sp, GBufferArrays gb,
                                                            Outputs out) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= gb.n) return;
  gbuffer_shade_ray<SHADE_STATIC>(S, gb, idx, out, idx);
}

// gbuffer_shade_kernel at one time (the 1-spp pass of grt_gbuffer_shade_section_at).
__global__ void __launch_bounds__(256) gbuffer_shade_at_kernel(const DevScene* __restrict__ Sp, GBufferArrays gb,
                                                               double t, Outputs out) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= gb.n) return;
  gbuffer_shade_ray<SHADE_AT>(S, gb, idx, out, idx, t);
}

// The supersample pass of an adaptive re-shade (grt_gbuffer_shade_section): one lane per
// (held selected pixel j, stratum s) of a chunk of the list `sel` (entries base + j <
// *d_count).  Sub-ray sub_block[sel[j]] * per + s of the buffer's sub-sample set `sub` is
// shaded as gbuffer_shade_kernel shades a pixel, into slot j * per + s: the layout
// average_kernel reads, with the sub-ray's step count beside it.
__global__ void __launch_bounds__(256) gbuffer_shade_sub_kernel(const DevScene* __restrict__ Sp, GBufferArrays sub,
                                                                const uint32_t* __restrict__ sub_steps,
                                                                const uint32_t* __restrict__ sub_block,
                                                                const uint32_t* __restrict__ sel, uint64_t n_sel,
                                                                const unsigned long long* __restrict__ d_count,
                                                                uint64_t base, uint32_t per, Outputs out) {
  const DevScene& S = *Sp;
  // a block past the held pixels (the empty chunks of a pass) has nothing to do
  if (base + (uint64_t)blockIdx.x * blockDim.x / per >= *d_count) return;
  glibc::tables_to_lds();  // whole block, before the per-lane early return
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t j = k / per;
  if (j >= n_sel || base + j >= *d_count) return;
  const uint64_t src = (uint64_t)sub_block[sel[j]] * per + k % per;
  if (src >= sub.n) return;  // a pixel the set does not hold: the split never lists one
  if (out.steps) out.steps[k] = sub_steps[src];
  gbuffer_shade_ray<SHADE_STATIC>(S, sub, src, out, k);
}

// gbuffer_shade_sub_kernel at one time (the supersample pass of grt_gbuffer_shade_section_at):
// the set's numbers are the unrotated ones; the time enters at the texture lookup only.
__global__ void __launch_bounds__(256) gbuffer_shade_sub_at_kernel(const DevScene* __restrict__ Sp, GBufferArrays sub,
                                                                   const uint32_t* __restrict__ sub_steps,
                                                                   const uint32_t* __restrict__ sub_block,
                                                                   const uint32_t* __restrict__ sel, uint64_t n_sel,
                                                                   const unsigned long long* __restrict__ d_count,
                                                                   uint64_t base, uint32_t per, double t, Outputs out) {
  const DevScene& S = *Sp;
  // a block past the held pixels (the empty chunks of a pass) has nothing to do
  if (base + (uint64_t)blockIdx.x * blockDim.x / per >= *d_count) return;
  glibc::tables_to_lds();  // whole block, before the per-lane early return
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t j = k / per;
  if (j >= n_sel || base + j >= *d_count) return;
  const uint64_t src = (uint64_t)sub_block[sel[j]] * per + k % per;
  if (src >= sub.n) return;  // a pixel the set does not hold: the split never lists one
  if (out.steps) out.steps[k] = sub_steps[src];
  gbuffer_shade_ray<SHADE_AT>(S, sub, src, out, k, t);
}

// The supersample pass of an adaptive re-shade of a stack of buffers
// (grt_gbuffer_shade_section_sequence): gbuffer_shade_sub_kernel with the set found per lane.
// `sel` holds stacked indices P = frame * npix + pixel of held selected pixels (entries
// base + j < *d_count); the frame's entry of the device table gives its set, the set's step
// counts and its sub_block.  Sub-ray sub_block[pixel] * per + s of that set is shaded into
// the chunk's slot j * per + s, the layout average_kernel reads.
__global__ void __launch_bounds__(256) gbuffer_shade_sub_stack_kernel(const DevScene* __restrict__ Sp,
                                                                      const GBufferSubFrame* __restrict__ frames,
                                                                      uint32_t n_frames, uint64_t npix,
                                                                      const uint32_t* __restrict__ sel, uint64_t n_sel,
                                                                      const unsigned long long* __restrict__ d_count,
                                                                      uint64_t base, uint32_t per, Outputs out) {
  const DevScene& S = *Sp;
  // a block past the held pixels (the empty chunks of a pass) has nothing to do
  if (base + (uint64_t)blockIdx.x * blockDim.x / per >= *d_count) return;
  glibc::tables_to_lds();  // whole block, before the per-lane early return
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t j = k / per;
  if (j >= n_sel || base + j >= *d_count) return;
  const uint64_t p = sel[j], f = p / npix;
  if (f >= n_frames) return;  // an index past the stack: the split never lists one
  const GBufferSubFrame fr = frames[f];
  const uint64_t src = (uint64_t)fr.sub_block[p - f * npix] * per + k % per;
  if (src >= fr.sub.n) return;  // a pixel the set does not hold: the split never lists one
  if (out.steps) out.steps[k] = fr.steps[src];
  gbuffer_shade_ray<SHADE_STATIC>(S, fr.sub, src, out, k);
}

// The deferred shade of a stack of equally sized buffers (grt_gbuffer_shade_sequence): one
// lane per (frame, pixel) of a launch group, the frame's arrays from a device table, the
// pixel shaded as gbuffer_shade_kernel shades it into slot frame * per + pixel of the
// stacked outputs, with the recorded step count beside it when asked for.
__global__ void __launch_bounds__(256) gbuffer_shade_stack_kernel(const DevScene* __restrict__ Sp,
                                                                  const GBufferFrame* __restrict__ frames,
                                                                  uint32_t n_frames, uint64_t per, Outputs out) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (uint64_t)n_frames * per) return;
  const uint64_t f = idx / per, src = idx - f * per;
  const GBufferFrame fr = frames[f];
  if (src >= fr.gb.n) return;  // a frame of another size: the host refuses such a stack
  if (out.steps) out.steps[idx] = fr.steps[src];
  gbuffer_shade_ray<SHADE_STATIC>(S, fr.gb, src, out, idx);
}

// One buffer at n_times times in one launch (grt_gbuffer_shade_times): one lane per (frame,
// pixel) of a launch group, frame k at times[k], into slot k * gb.n + pixel of the stacked
// outputs (gbuffer_shade_stack_kernel's layout), the recorded step count beside it when asked.
// The layers' rates come from omega[], written once per call by the pre-pass below: the
// n_times * 2 colour evaluations of a layer read 8 bytes instead of redoing pow, sqrt and a
// division (measured against the inline form: DESIGN.md section 15).
__global__ void __launch_bounds__(256) gbuffer_shade_times_kernel(const DevScene* __restrict__ Sp, GBufferArrays gb,
                                                                  const uint32_t* __restrict__ steps,
                                                                  const double* __restrict__ times, uint32_t n_times,
                                                                  const double* __restrict__ omega, Outputs out) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (uint64_t)n_times * gb.n) return;
  const uint64_t f = idx / gb.n, src = idx - f * gb.n;
  if (out.steps) out.steps[idx] = steps[src];
  gbuffer_shade_ray<SHADE_AT_CACHED>(S, gb, src, out, idx, times[f], omega);
}

// gbuffer_shade_times_kernel under the retarded rule (grt_gbuffer_shade_times_retarded): the
// same launch shape and output layout, each disc layer at times[f] + lapse[layer].
__global__ void __launch_bounds__(256) gbuffer_shade_times_retarded_kernel(
    const DevScene* __restrict__ Sp, GBufferArrays gb, const uint32_t* __restrict__ steps,
    const double* __restrict__ times, uint32_t n_times, const double* __restrict__ omega,
    const double* __restrict__ lapse, Outputs out) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (uint64_t)n_times * gb.n) return;
  const uint64_t f = idx / gb.n, src = idx - f * gb.n;
  if (out.steps) out.steps[idx] = steps[src];
  gbuffer_shade_ray<SHADE_RETARDED>(S, gb, src, out, idx, times[f], omega, lapse);
}

// The pre-pass of grt_gbuffer_shade_times: orbit_rate of every disc layer, once per call (the
// entry of another layer is never read).
__global__ void __launch_bounds__(256) gbuffer_orbit_rate_kernel(const DevScene* __restrict__ Sp, GBufferArrays gb,
                                                                 uint64_t n_layers, double* __restrict__ omega) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_layers) return;
  omega[k] = S.obj[gb.object[k]].kind == GRT_OBJ_DISC ? orbit_rate(S, gb.radius[k]) : 0.0;
}

// gbuffer_shade_at_kernel under the retarded rule (the 1-spp pass of
// grt_gbuffer_shade_section_at_retarded): each disc layer at t + lapse[layer], the buffer's lapse.
__global__ void __launch_bounds__(256) gbuffer_shade_at_retarded_kernel(const DevScene* __restrict__ Sp,
                                                                        GBufferArrays gb, double t,
                                                                        const double* __restrict__ lapse,
                                                                        Outputs out) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= gb.n) return;
  gbuffer_shade_ray<SHADE_RETARDED_AT>(S, gb, idx, out, idx, t, nullptr, lapse);
}

// gbuffer_shade_sub_at_kernel under the retarded rule (the supersample pass of
// grt_gbuffer_shade_section_at_retarded): sub_lapse is the set's lapse, one entry per
// sub-layer, indexed as the set's layer arrays are.
__global__ void __launch_bounds__(256) gbuffer_shade_sub_at_retarded_kernel(
    const DevScene* __restrict__ Sp, GBufferArrays sub, const uint32_t* __restrict__ sub_steps,
    const uint32_t* __restrict__ sub_block, const uint32_t* __restrict__ sel, uint64_t n_sel,
    const unsigned long long* __restrict__ d_count, uint64_t base, uint32_t per, double t,
    const double* __restrict__ sub_lapse, Outputs out) {
  const DevScene& S = *Sp;
  // a block past the held pixels (the empty chunks of a pass) has nothing to do
  if (base + (uint64_t)blockIdx.x * blockDim.x / per >= *d_count) return;
  glibc::tables_to_lds();  // whole block, before the per-lane early return
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t j = k / per;
  if (j >= n_sel || base + j >= *d_count) return;
  const uint64_t src = (uint64_t)sub_block[sel[j]] * per + k % per;
  if (src >= sub.n) return;  // a pixel the set does not hold: the split never lists one
  if (out.steps) out.steps[k] = sub_steps[src];
  gbuffer_shade_ray<SHADE_RETARDED_AT>(S, sub, src, out, k, t, nullptr, sub_lapse);
}

hipError_t launch_gbuffer_orbit_rate(const DevScene* d_scene, const GBufferArrays& gb, uint64_t n_layers,
                                     double* d_omega, hipStream_t stream) {
  if (n_layers == 0) return hipSuccess;
  hipLaunchKernelGGL(gbuffer_orbit_rate_kernel, dim3((unsigned)((n_layers + 255) / 256)), dim3(256), 0, stream, d_scene,
                     gb, n_layers, d_omega);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade_times(const DevScene* d_scene, const GBufferArrays& gb, const uint32_t* d_steps,
                                      const double* d_times, uint32_t n_times, const double* d_omega,
                                      const double* d_lapse, bool retarded, const Outputs& out, hipStream_t stream) {
  const uint64_t n = (uint64_t)n_times * gb.n;
  if (n == 0) return hipSuccess;
  if (n > 0xffffffffull * 256) return hipErrorInvalidValue;
  if (!d_omega || (retarded && !d_lapse)) return hipErrorInvalidValue;
  if (retarded) {
    hipLaunchKernelGGL(gbuffer_shade_times_retarded_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       d_scene, gb, d_steps, d_times, n_times, d_omega, d_lapse, out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(gbuffer_shade_times_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_scene, gb,
                     d_steps, d_times, n_times, d_omega, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade_at(const DevScene* d_scene, const GBufferArrays& gb, double t, const Outputs& out,
                                   hipStream_t stream) {
  if (gb.n == 0) return hipSuccess;
  hipLaunchKernelGGL(gbuffer_shade_at_kernel, dim3((unsigned)((gb.n + 255) / 256)), dim3(256), 0, stream, d_scene, gb, t,
                     out);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade_sub_at(const DevScene* d_scene, const GBufferArrays& sub, const uint32_t* d_sub_steps,
                                       const uint32_t* d_sub_block, const uint32_t* d_sel, uint64_t n_sel,
                                       const unsigned long long* d_count, uint64_t base, uint32_t spa, double t,
                                       const Outputs& out, hipStream_t stream) {
  const uint64_t n = n_sel * spa * spa;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gbuffer_shade_sub_at_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_scene, sub,
                     d_sub_steps, d_sub_block, d_sel, n_sel, d_count, base, spa * spa, t, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade_stack(const DevScene* d_scene, const GBufferFrame* d_frames, uint32_t n_frames,
                                      uint64_t per, const Outputs& out, hipStream_t stream) {
  const uint64_t n = (uint64_t)n_frames * per;
  if (n == 0) return hipSuccess;
  if (n > 0xffffffffull * 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gbuffer_shade_stack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_scene,
                     d_frames, n_frames, per, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade(const DevScene* d_scene, const GBufferArrays& gb, const Outputs& out,
                                hipStream_t stream) {
  if (gb.n == 0) return hipSuccess;
  hipLaunchKernelGGL(gbuffer_shade_kernel, dim3((unsigned)((gb.n + 255) / 256)), dim3(256), 0, stream, d_scene, gb, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade_sub(const DevScene* d_scene, const GBufferArrays& sub, const uint32_t* d_sub_steps,
                                    const uint32_t* d_sub_block, const uint32_t* d_sel, uint64_t n_sel,
                                    const unsigned long long* d_count, uint64_t base, uint32_t spa, const Outputs& out,
                                    hipStream_t stream) {
  const uint64_t n = n_sel * spa * spa;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gbuffer_shade_sub_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_scene, sub,
                     d_sub_steps, d_sub_block, d_sel, n_sel, d_count, base, spa * spa, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade_sub_stack(const DevScene* d_scene, const GBufferSubFrame* d_frames, uint32_t n_frames,
                                          uint64_t npix, const uint32_t* d_sel, uint64_t n_sel,
                                          const unsigned long long* d_count, uint64_t base, uint32_t spa,
                                          const Outputs& out, hipStream_t stream) {
  const uint64_t n = n_sel * spa * spa;
  if (n == 0) return hipSuccess;
  if (npix == 0 || n_frames == 0 || n > 0xffffffffull * 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gbuffer_shade_sub_stack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_scene,
                     d_frames, n_frames, npix, d_sel, n_sel, d_count, base, spa * spa, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade_at_retarded(const DevScene* d_scene, const GBufferArrays& gb, double t,
                                            const double* d_lapse, const Outputs& out, hipStream_t stream) {
  if (gb.n == 0) return hipSuccess;
  if (!d_lapse) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gbuffer_shade_at_retarded_kernel, dim3((unsigned)((gb.n + 255) / 256)), dim3(256), 0, stream,
                     d_scene, gb, t, d_lapse, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer_shade_sub_at_retarded(const DevScene* d_scene, const GBufferArrays& sub,
                                                const uint32_t* d_sub_steps, const uint32_t* d_sub_block,
                                                const uint32_t* d_sel, uint64_t n_sel,
                                                const unsigned long long* d_count, uint64_t base, uint32_t spa,
                                                double t, const double* d_sub_lapse, const Outputs& out,
                                                hipStream_t stream) {
  const uint64_t n = n_sel * spa * spa;
  if (n == 0) return hipSuccess;
  if (!d_sub_lapse) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gbuffer_shade_sub_at_retarded_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     d_scene, sub, d_sub_steps, d_sub_block, d_sel, n_sel, d_count, base, spa * spa, t, d_sub_lapse, out);
  return hipGetLastError();
}

}  // namespace grt
