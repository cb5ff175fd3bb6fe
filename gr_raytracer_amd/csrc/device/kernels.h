// kernels.h — launch entry points of the gfx950 kernels (geodesic.hip and its geodesic_*.h layers,
// gbuffer_shade.hip, adaptive.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "dev_scene.h"
#include "glibc_check.h"

namespace grt {

// integrate_kernel (persistent, lane refill) then shade_kernel, all on `stream`.  With
// `vol` (the scene has VolumetricDiscs): integrate, job gathering, march_kernel and the
// composite; the workspace then needs its volumetric arrays, ws.march zeroed.
// `tl.cap` != 0 (every Kerr-Schild trace, volumetric or not): long rays are handed to
// tail_kernel (launched between integrate and shade on `stream`, `tail_blocks` blocks of
// 256 threads); tl.ctl must be zeroed.
hipError_t launch_trace(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                        const Outputs& out, unsigned long long* d_counter, unsigned long long* d_stats,
                        int blocks, int threads, bool vol, const TailList& tl, int tail_blocks,
                        hipStream_t stream);
// Diagnostic builds (-DGRT_RAY_TIMES=1): the per-ray schedule record ([6][n] words, see
// geodesic.hip), or NULL.
hipError_t set_ray_times(unsigned long long* p);
// Tail kernel's quad capacity per block (rays integrated at once).
constexpr int TAIL_RAYS_PER_BLOCK = 256 / 4;

// Work-order probe: steps of one ray per 8x8 tile of `wl` (rectangle mode), capped.
// quad (Kerr-Schild only): each probe ray on a quad of lanes (probe_quad_kernel), same keys.
hipError_t launch_probe(int geometry, const DevScene* d_scene, const WorkList& wl, uint32_t n_tiles, uint32_t cap,
                        uint32_t* d_steps, bool quad, hipStream_t stream);
// Schwarzschild work-order keys without a probe pass: predicted steps per 8x8 tile of
// `wl` from the impact parameter of the tile's probe pixel (impact_key_kernel).
hipError_t launch_impact_keys(const DevScene* d_scene, const WorkList& wl, uint32_t n_tiles, uint32_t* d_keys,
                              hipStream_t stream);
// Schwarzschild sincos-case predictor (class_key_kernel): pi/2 - theta_f of the asymptotic
// direction of the ray through pixel (8i, 8j) of `wl`, clamped to the frame, for the
// corners_x x (n_corners / corners_x) corners of the tile grid; CLASS_CAPTURED-large for
// a captured ray, NaN for an undecided one.
hipError_t launch_class_keys(const DevScene* d_scene, const WorkList& wl, uint32_t corners_x, uint32_t n_corners,
                             float* d_a, hipStream_t stream);
// Tile queue order from the probe keys (schedule.hip): 3x3-dilated keys (edge tiles of a
// region of probes that reached `cap` boosted), sorted descending (stable).  `temp` /
// `temp_bytes`: scratch, query with temp == NULL.
// d_corner_a (launch_class_keys' output, NULL = none): the composite key, the predicted
// length in LEN_BUCKET steps as the major part and the tile's sincos class as the minor
// one (schedule.hip tile_class); d_class (nullable) receives the classes.
hipError_t launch_tile_order(const uint32_t* d_probe, uint32_t tiles_x, uint32_t tiles_y, uint32_t cap, uint32_t* d_keys,
                             uint32_t* d_keys_sorted, uint32_t* d_idx, uint32_t* d_order, void* temp,
                             size_t* temp_bytes, hipStream_t stream, const float* d_corner_a = nullptr,
                             uint8_t* d_class = nullptr);

// Whole trajectories (render-ray / render-ray-at): camera pixels (row, col) or explicit
// native-chart (position, momentum) pairs; record layout in trajectory_kernel.
struct TrajectoryList {
  uint64_t n;
  const double* row;  // camera mode: pixel coordinates (offsets allowed), both non-null
  const double* col;
  const double* pos;  // explicit mode: n x 4 each
  const double* mom;
  uint64_t cap;       // records stored per ray
  double* steps;      // n x cap x 9
  uint64_t* n_steps;  // steps produced per ray (step 0 included), even beyond cap
  uint8_t* stop;
  uint8_t* status;
};
// test hook: div_inrange / div2_inrange against the compiler's division on n random pairs
hipError_t launch_arith_map(uint32_t samples, uint64_t seed, uint8_t* d_map, uint8_t* d_zmap, uint8_t* d_smap,
                            hipStream_t stream);
// test hook: the seeded reciprocals of rcp_seed.h against the compiler's division on n tuples
hipError_t launch_rcp_seed_check(uint64_t n, const double* d_tuples, uint8_t* d_flags, hipStream_t stream);
// test hook: the render's glibc wrappers on n inputs (glibc_check.h): unit 0, tables in LDS
// (geodesic.hip glibc_check_kernel), `threads` per block; unit 1, opow with the tables in
// constant memory (output.hip opow_check_kernel)
hipError_t launch_glibc_check(int fn, int threads, uint64_t n, const double* d_x, const double* d_y, double* d_out0,
                              double* d_out1, uint8_t* d_path, hipStream_t stream);
hipError_t launch_opow_check(int threads, uint64_t n, const double* d_x, const double* d_y, double* d_out0,
                             double* d_out1, uint8_t* d_path, hipStream_t stream);
hipError_t launch_rhs_check(int geometry, const DevScene* d_scene, const double* d_states, const double* d_consts,
                            uint64_t n, double* d_out, uint8_t* d_pred, hipStream_t stream);
hipError_t launch_rkf_check(const DevScene* d_scene, const double* d_states, const double* d_h, uint64_t n,
                            double* d_short, double* d_full, uint8_t* d_guard, hipStream_t stream);
// test hook: the VolumetricDisc device functions (volumetric.h) of object `obj` on n inputs
// of 6 doubles each, 8 doubles and a flag byte out per input (vdisc_points_kernel says which)
enum VdiscCheckFn {
  VDISC_FN_PERLIN = 0,   // perlin3 with the object's permutation table
  VDISC_FN_DENSITY = 1,  // vdisc_density
  VDISC_FN_CHORD = 2,    // vdisc_chord
  VDISC_FN_EXIT = 3,     // vdisc_exit_distance
  VDISC_FN_NO_MORE = 4,  // vdisc_no_more_density
  VDISC_FN_COUNT = 5,
};
hipError_t launch_vdisc_points(const DevScene* d_scene, uint32_t obj, int fn, uint64_t n, const double* d_in,
                               double* d_out, uint8_t* d_flag, hipStream_t stream);
// test hook: the surface path's pieces (geodesic.hip chord tests and window filter,
// appearance.h lookups) on n rows of 8 doubles each, 8 doubles and a flag byte out per row
// (surface_points_kernel says which); obj: an object of the scene, -1 where a request takes
// the celestial texture or the blackbody table
enum SurfaceCheckFn {
  SURFACE_FN_DISC_CHORD = 0,    // disc_chord
  SURFACE_FN_SPHERE_CHORD = 1,  // sphere_chord
  SURFACE_FN_WINDOW_FAR = 2,    // window_far<G, VOL> of the scene's chart
  SURFACE_FN_LUT_INDEX = 3,     // lut_index over the object's lut_r, or bb_log_t
  SURFACE_FN_TEMPERATURE = 4,   // compute_temperature
  SURFACE_FN_BLACKBODY = 5,     // sample_blackbody
  SURFACE_FN_TEXTURE = 6,       // texture_color of the object's texture, or the celestial one
  SURFACE_FN_BLEND = 7,         // blend
  SURFACE_FN_COUNT = 8,
};
hipError_t launch_surface_points(int geometry, const DevScene* d_scene, int obj, int fn, uint64_t n, const double* d_in,
                                 double* d_out, uint8_t* d_flag, hipStream_t stream);
// test hook: march_kernel<geometry> alone, `blocks` blocks of 256 threads, over the jobs the
// caller filed in `ws` (jobs, march[0] = their count, the march cursors zeroed): the exact
// unit's (every chart but KerrBL), the exact KerrBL unit's and the fused unit's (every chart
// but Kerr-Schild); hipErrorInvalidValue for a chart the unit does not build
hipError_t launch_march(int geometry, const DevScene* d_scene, const Workspace& ws, int blocks, hipStream_t stream);
namespace kerr_bl {
hipError_t launch_march(int geometry, const DevScene* d_scene, const Workspace& ws, int blocks, hipStream_t stream);
}
namespace fused {
hipError_t launch_march(int geometry, const DevScene* d_scene, const Workspace& ws, int blocks, hipStream_t stream);
}
#if GRT_PATH_COUNT
hipError_t path_read(unsigned long long* out, bool reset);  // 2 * 14 words
#endif
// The same trace compiled with FMA contraction (geodesic_fused.hip, grt_set_arithmetic(1)):
// every geometry but Kerr-Schild (hipErrorInvalidValue for it).
namespace fused {
hipError_t launch_trace(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                        const Outputs& out, unsigned long long* d_counter, unsigned long long* d_stats,
                        int blocks, int threads, bool vol, const TailList& tl, int tail_blocks,
                        hipStream_t stream);
}  // namespace fused
// The exact KerrBL trace (geodesic_kerr_bl.hip: the same code compiled without machine
// loop-invariant code motion, which hoisted ~100 VGPRs of polynomial constants out of the
// loops and made the 3-wave integrate kernel spill; C3 -2%, its raymarch -7%, profiles/r06p).
namespace kerr_bl {
hipError_t launch_trace(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                        const Outputs& out, unsigned long long* d_counter, unsigned long long* d_stats,
                        int blocks, int threads, bool vol, const TailList& tl, int tail_blocks,
                        hipStream_t stream);
hipError_t set_ray_times(unsigned long long* p);
#if GRT_PATH_COUNT
hipError_t path_read(unsigned long long* out, bool reset);
#endif
}  // namespace kerr_bl
// The exact trace over a stack of frames that share the scene but not the camera
// (geodesic_seq.hip, grt_render_sequence).  `wl` describes the stack as one rectangle of
// n_cams * cam_rows rows (or an offset list over it); row R of the stack is row
// R % cam_rows of frame R / cam_rows, traced with cams[R / cam_rows] in place of the
// scene's camera.  The table is a kernel parameter of this unit's kernels only: WorkList,
// Workspace and DevScene are the tuned units' arguments and stay as they are.
struct CamTable {
  const DevCamera* cams;  // device memory, n_cams entries
  uint32_t cam_rows;      // rows of one frame
  uint32_t n_cams;
};
namespace seq {
hipError_t launch_trace(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                        const Outputs& out, unsigned long long* d_counter, unsigned long long* d_stats,
                        int blocks, int threads, bool vol, const TailList& tl, int tail_blocks,
                        hipStream_t stream, CamTable ct);
hipError_t launch_probe(int geometry, const DevScene* d_scene, const WorkList& wl, uint32_t n_tiles, uint32_t cap,
                        uint32_t* d_steps, bool quad, hipStream_t stream, CamTable ct);
hipError_t launch_impact_keys(const DevScene* d_scene, const WorkList& wl, uint32_t n_tiles, uint32_t* d_keys,
                              hipStream_t stream, CamTable ct);
hipError_t launch_class_keys(const DevScene* d_scene, const WorkList& wl, uint32_t corners_x, uint32_t n_corners,
                             float* d_a, hipStream_t stream, CamTable ct);
}  // namespace seq
hipError_t launch_trajectories(int geometry, const DevScene* d_scene, const TrajectoryList& tl, hipStream_t stream);

// The geometry buffer of a traced rectangle (grt_gbuffer_*), device arrays, structure of
// arrays.  Per pixel, in output-slot order: the trace's status and stop reason, the
// celestial sphere's texture arguments, and layer_start (n + 1 entries, the exclusive
// prefix sum of the layer counts).  Per layer (a window-nearest hit), pixel-major and front
// to back: the object and texture_color's / compute_temperature's arguments.
struct GBufferArrays {
  uint64_t n;
  const uint8_t* status;
  const uint8_t* stop;
  const uint64_t* layer_start;
  double *sky_u, *sky_v, *sky_redshift;
  uint8_t* object;
  double *u, *v, *redshift, *radius;
};
// Layer counts (the trace's `hits`, 0 where status != 0; counts[n] = 0) and their exclusive
// prefix sum over n + 1 entries, so layer_start[n] is the total (gbuffer.hip; n < INT_MAX).
// Call with d_temp == NULL for *temp_bytes.
hipError_t gbuffer_layer_scan(const uint8_t* d_status, const uint32_t* d_hits, uint64_t n, uint64_t* d_counts,
                              uint64_t* d_layer_start, void* d_temp, size_t* temp_bytes, hipStream_t stream);
// Fill `gb` from the workspace and hit pool a 1-spp rectangle trace of `wl` left behind
// (gbuffer_fill_kernel: geodesic_fill.h for every chart but KerrBL, whose exact unit has its own).
hipError_t launch_gbuffer_fill(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                               const GBufferArrays& gb, hipStream_t stream);
namespace kerr_bl {
hipError_t launch_gbuffer_fill(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                               const GBufferArrays& gb, hipStream_t stream);
}
// The same after a stacked trace (seq::launch_trace), every chart; `wl` is the stack from
// (0, 0): its whole rectangle, `gb` spanning it in slot order, frame after frame
// (grt_gbuffer_trace_sequence), or an offset list over it, `gb` spanning the list's
// n_items slots (grt_gbuffer_supersample_sequence).  A ray's camera is its frame's entry
// of the table, found from its stacked row; hipErrorInvalidValue for any other work list.
namespace seq {
hipError_t launch_gbuffer_fill(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                               const GBufferArrays& gb, hipStream_t stream, CamTable ct);
}
// The exact trace and fill of a buffer that holds its lapse (geodesic_lapse.hip,
// grt_gbuffer_trace_lapse), every chart but KerrBL, scenes without VolumetricDiscs (hipErrorInvalidValue
// for `vol`).  The trace is launch_trace's and leaves the same workspace, pool and outputs;
// it also writes the coordinate time of every candidate to ws.pool->slot_time / pool_time,
// which must be there.  The fill is launch_gbuffer_fill's and also writes d_lapse[layer] = the
// layer's candidate's time - the camera's, over the buffer's layers.
namespace lapse {
hipError_t launch_trace(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                        const Outputs& out, unsigned long long* d_counter, unsigned long long* d_stats,
                        int blocks, int threads, bool vol, const TailList& tl, int tail_blocks,
                        hipStream_t stream);
hipError_t launch_gbuffer_fill(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                               const GBufferArrays& gb, hipStream_t stream, double* d_lapse);
}  // namespace lapse
namespace lapse_kerr_bl {  // KerrBL's (geodesic_lapse_kerr_bl.hip), as kerr_bl is to the exact build
hipError_t launch_trace(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                        const Outputs& out, unsigned long long* d_counter, unsigned long long* d_stats,
                        int blocks, int threads, bool vol, const TailList& tl, int tail_blocks,
                        hipStream_t stream);
hipError_t launch_gbuffer_fill(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                               const GBufferArrays& gb, hipStream_t stream, double* d_lapse);
}  // namespace lapse_kerr_bl
// A stacked buffer cut into its frames (gbuffer.hip): frame_start[i] = stack_start[i] -
// stack_start[0] for i <= n, where stack_start points at the frame's first pixel.
hipError_t gbuffer_rebase(const uint64_t* d_stack_start, uint64_t n, uint64_t* d_frame_start, hipStream_t stream);
// Deferred shade of `gb` under the appearance scene (gbuffer_shade_kernel, gbuffer_shade.hip).
hipError_t launch_gbuffer_shade(const DevScene* d_scene, const GBufferArrays& gb, const Outputs& out,
                                hipStream_t stream);
// Deferred shade of n_frames buffers of `per` pixels each in one launch
// (gbuffer_shade_stack_kernel, gbuffer_shade.hip): d_frames is a device table of the buffers'
// views and recorded step counts; out spans n_frames * per slots, frame-major.
struct GBufferFrame {
  GBufferArrays gb;
  const uint32_t* steps;
};
hipError_t launch_gbuffer_shade_stack(const DevScene* d_scene, const GBufferFrame* d_frames, uint32_t n_frames,
                                      uint64_t per, const Outputs& out, hipStream_t stream);
// The sub-sample set of a buffer (grt_gbuffer_supersample): for some pixels, the spa^2
// jittered sub-rays, each reduced as a 1-spp ray is; sub-ray b * spa^2 + s is stratum s of
// block b, and sub_block[pixel] is the pixel's block or GBUFFER_NIL.
constexpr uint32_t GBUFFER_NIL = 0xffffffffu;
// Supersample pass of the adaptive re-shade (gbuffer_shade_sub_kernel, gbuffer_shade.hip): a
// chunk of n_sel entries at position `base` of the held list d_sel (*d_count entries),
// shaded into out at j * spa^2 + s (out.steps takes the sub-rays' step counts).
hipError_t launch_gbuffer_shade_sub(const DevScene* d_scene, const GBufferArrays& sub, const uint32_t* d_sub_steps,
                                    const uint32_t* d_sub_block, const uint32_t* d_sel, uint64_t n_sel,
                                    const unsigned long long* d_count, uint64_t base, uint32_t spa, const Outputs& out,
                                    hipStream_t stream);
// The same for the buffers of a stack (gbuffer_shade_sub_stack_kernel, gbuffer_shade.hip): d_sel
// holds stacked indices P = frame * npix + pixel of held selected pixels, and entry P / npix
// of the device table d_frames gives the frame's set, its step counts and its sub_block.
struct GBufferSubFrame {
  GBufferArrays sub;  // the set's rays, n = n_sub_rays (0: the buffer holds none)
  const uint32_t* steps;
  const uint32_t* sub_block;
};
hipError_t launch_gbuffer_shade_sub_stack(const DevScene* d_scene, const GBufferSubFrame* d_frames, uint32_t n_frames,
                                          uint64_t npix, const uint32_t* d_sel, uint64_t n_sel,
                                          const unsigned long long* d_count, uint64_t base, uint32_t spa,
                                          const Outputs& out, hipStream_t stream);
// The disc's orbital motion (gbuffer_shade.hip): `gb` shaded at d_times[0..n_times) in one launch
// (gbuffer_shade_times_kernel), frame k into slots [k * gb.n, (k + 1) * gb.n) of out, d_steps
// the buffer's recorded step counts; and launch_gbuffer_shade / launch_gbuffer_shade_sub at one
// time t (gbuffer_shade_at_kernel, gbuffer_shade_sub_at_kernel).  The K-times kernel reads each
// layer's rate from d_omega (n_layers doubles), which launch_gbuffer_orbit_rate writes once per
// call; the single-time kernels compute it where a layer is coloured.
hipError_t launch_gbuffer_orbit_rate(const DevScene* d_scene, const GBufferArrays& gb, uint64_t n_layers,
                                     double* d_omega, hipStream_t stream);
// retarded (gbuffer_shade_times_retarded_kernel): layer k of a frame at its time + d_lapse[k]
// (n_layers doubles; unread otherwise).
hipError_t launch_gbuffer_shade_times(const DevScene* d_scene, const GBufferArrays& gb, const uint32_t* d_steps,
                                      const double* d_times, uint32_t n_times, const double* d_omega,
                                      const double* d_lapse, bool retarded, const Outputs& out, hipStream_t stream);
hipError_t launch_gbuffer_shade_at(const DevScene* d_scene, const GBufferArrays& gb, double t, const Outputs& out,
                                   hipStream_t stream);
hipError_t launch_gbuffer_shade_sub_at(const DevScene* d_scene, const GBufferArrays& sub, const uint32_t* d_sub_steps,
                                       const uint32_t* d_sub_block, const uint32_t* d_sel, uint64_t n_sel,
                                       const unsigned long long* d_count, uint64_t base, uint32_t spa, double t,
                                       const Outputs& out, hipStream_t stream);
// The two single-time launches under the retarded rule (gbuffer_shade_at_retarded_kernel,
// gbuffer_shade_sub_at_retarded_kernel): layer k at t + d_lapse[k], the buffer's lapse over its
// layers, the set's over the set's.  hipErrorInvalidValue for a null lapse.
hipError_t launch_gbuffer_shade_at_retarded(const DevScene* d_scene, const GBufferArrays& gb, double t,
                                            const double* d_lapse, const Outputs& out, hipStream_t stream);
hipError_t launch_gbuffer_shade_sub_at_retarded(const DevScene* d_scene, const GBufferArrays& sub,
                                                const uint32_t* d_sub_steps, const uint32_t* d_sub_block,
                                                const uint32_t* d_sel, uint64_t n_sel,
                                                const unsigned long long* d_count, uint64_t base, uint32_t spa,
                                                double t, const double* d_sub_lapse, const Outputs& out,
                                                hipStream_t stream);
// The selected pixels d_sel (*d_count of them, ascending) split by sub_block into the ones
// the set holds and the ones it misses, each in ascending order, with their counts
// (gbuffer.hip; n_max <= INT_MAX entries of room).  d_flags: 2 * n_max bytes of scratch.
// Call with d_temp == NULL for *temp_bytes.
hipError_t gbuffer_split(const uint32_t* d_sel, const unsigned long long* d_count, uint64_t n_max,
                         const uint32_t* d_sub_block, uint8_t* d_flags, uint32_t* d_held,
                         unsigned long long* d_n_held, uint32_t* d_missing, unsigned long long* d_n_missing,
                         void* d_temp, size_t* temp_bytes, hipStream_t stream);
// gbuffer_split over the selections of n_frames buffers of npix pixels at once: frame f's
// selection is d_sel[f * npix + j], j < d_cnt[4 f], looked up in its own buffer's sub_block
// (d_frames[f]).  The lists hold stacked indices f * npix + pixel, ascending, so frame-major;
// d_cnt[4 f + 2] and [4 f + 3] (zero on entry) take the frame's held and missing counts,
// *d_n_held and *d_n_missing the totals.  d_flags: 2 * n_frames * npix bytes, d_stack:
// n_frames * npix entries of scratch (n_frames * npix <= INT_MAX).
hipError_t gbuffer_split_stack(const uint32_t* d_sel, unsigned long long* d_cnt, uint32_t n_frames, uint64_t npix,
                               const GBufferSubFrame* d_frames, uint8_t* d_flags, uint32_t* d_stack, uint32_t* d_held,
                               unsigned long long* d_n_held, uint32_t* d_missing, unsigned long long* d_n_missing,
                               void* d_temp, size_t* temp_bytes, hipStream_t stream);
// Appending a chunk to the set: d_layer_start[i] = d_local[i] + layer_base for i <= n_rays,
// and sub_block[d_pixels[j]] = first_block + j, sub_pixel[first_block + j] = d_pixels[j].
hipError_t gbuffer_sub_append(const uint64_t* d_local, uint64_t n_rays, uint64_t layer_base, uint64_t* d_layer_start,
                              const uint32_t* d_pixels, uint64_t n_pixels, uint32_t first_block, uint32_t* d_sub_block,
                              uint32_t* d_sub_pixel, hipStream_t stream);
// sub_block of an uploaded set: GBUFFER_NIL everywhere, then block j at d_sub_pixel[j].
hipError_t gbuffer_sub_index(const uint32_t* d_sub_pixel, uint64_t n_sub_pixels, uint64_t n_pixels,
                             uint32_t* d_sub_block, hipStream_t stream);

// Invariant monitors of the n = rows x cols rays of a rectangle (health_kernel):
// d_out n x 5 doubles, d_status n bytes.
hipError_t launch_health(int geometry, const DevScene* d_scene, const WorkList& wl, uint64_t n, double* d_out,
                         uint8_t* d_status, hipStream_t stream);

// Adaptive supersampling helpers (raytracer.rs:91-159, :320-458).
struct AdaptiveParams {
  uint32_t w, h;  // section size
  int32_t exclude_background_contrast;
  int32_t _pad;
  double min_lum;
  double luminance_contrast_threshold;
  double opacity_contrast_threshold;
};
// d_min_lum (nullable): the luminance floor on the device, else p.min_lum.
hipError_t launch_select(const double* d_xyza64, const uint8_t* d_cls, const AdaptiveParams& p,
                         const double* d_min_lum, uint8_t* d_flags, hipStream_t stream);
// The index-th of n luminances d_y[stride * i] in f64::total_cmp order, on the device
// (radix sort; n <= INT_MAX).  Call with d_mem == NULL for the scratch size.
// luminance_order_stat returns the value to the host; luminance_floor_device writes
// 1e-3 x the value (resolve_minimum_luminance) to *d_min_lum without a host copy.
hipError_t luminance_order_stat(const double* d_y, uint32_t stride, uint64_t n, uint64_t index, void* d_mem,
                                size_t* mem_bytes, double* value, hipStream_t stream);
hipError_t luminance_floor_device(const double* d_y, uint32_t stride, uint64_t n, uint64_t index, void* d_mem,
                                  size_t* mem_bytes, double* d_min_lum, hipStream_t stream);
// Indices i < n with d_flags[i] != 0, in order, and their count (n <= INT_MAX).
// Call with d_temp == NULL for *temp_bytes.
hipError_t compact_flags(const uint8_t* d_flags, uint64_t n, uint32_t* d_out, unsigned long long* d_count, void* d_temp,
                         size_t* temp_bytes, hipStream_t stream);
hipError_t launch_select_shard(const double* d_ya, const uint8_t* d_cls, const AdaptiveParams& p,
                               const double* d_min_lum, uint32_t band_rows, uint32_t shard, uint32_t n_shards,
                               uint32_t local_rows, uint8_t* d_flags, hipStream_t stream);
// The supersample helpers take a chunk of the selected list: n_sel entries starting at
// position `base` of a list of *d_count entries (d_count NULL: all n_sel present).
hipError_t launch_make_offsets(const uint32_t* d_sel, uint64_t n_sel, const unsigned long long* d_count, uint64_t base,
                               uint32_t spa, uint32_t row0, uint32_t col0, uint32_t w, uint32_t* d_pix, double* d_dx,
                               double* d_dy, hipStream_t stream);
// The same for n_sel entries of a list over a stack of frames of `rows` x `w` pixels
// (offsets_stack_kernel): entry P = frame * rows * w + pixel; the jitter hashes the frame's
// own (row, col) = ((P / w) % rows, P % w), as the frame alone does, and d_pix takes P.
hipError_t launch_make_offsets_stack(const uint32_t* d_sel, uint64_t n_sel, uint32_t spa, uint32_t rows, uint32_t w,
                                     uint32_t* d_pix, double* d_dx, double* d_dy, hipStream_t stream);
// Failed sub-samples of the supersample pass (device side; count NULL: not recorded).
struct SubsampleFailures {
  unsigned long long* count;
  uint64_t* key;      // pixel * spa^2 + stratum
  uint8_t* status;
  uint64_t cap;
  // with `stop` set, the list also takes the sub-rays without an error that ended on NaN
  // coordinates or without a terminal event (status 0), with their stop reason and steps
  uint8_t* stop;
  uint32_t* steps;
  const uint8_t* ray_stop;    // the sub-ray trace's stop reasons / step counts
  const uint32_t* ray_steps;
};
hipError_t launch_average(const uint32_t* d_sel_out, const uint32_t* d_sel_px, uint64_t n_sel,
                          const unsigned long long* d_count, uint64_t base, uint32_t spa, const double* d_samples,
                          const uint8_t* d_status, double* d_out, const SubsampleFailures& f, hipStream_t stream);
// average_kernel's failure records for a chunk whose pixels belong to several frames
// (failures_stack_kernel): d_sel holds stacked indices P = frame * npix + pixel, the chunk's
// sub-ray j * spa^2 + s has status d_status[...], and a failed sub-sample (or, where the
// frame's list has `stop`, an event) goes to list P / npix of the device table d_frames
// with the key (P % npix) * spa^2 + s; each list's count counts them all.
hipError_t launch_failures_stack(const uint32_t* d_sel, uint64_t n_sel, const unsigned long long* d_count, uint64_t base,
                                 uint32_t spa, uint64_t npix, uint32_t n_frames, const uint8_t* d_status,
                                 const SubsampleFailures* d_frames, hipStream_t stream);
hipError_t launch_paint(const uint32_t* d_sel, uint64_t n_sel, const unsigned long long* d_count, const double* mask,
                        double* d_out, hipStream_t stream);
// live[c] = sub-rays of chunk c (P selected pixels per chunk, `per` sub-rays each)
hipError_t launch_chunk_live(const unsigned long long* d_count, uint32_t n_chunks, uint64_t P, uint32_t per,
                             unsigned long long* d_live, hipStream_t stream);
hipError_t launch_frame_index(const uint32_t* d_sel_local, const unsigned long long* d_count, uint64_t n_max, uint32_t w,
                              uint32_t band_rows, uint32_t shard, uint32_t n_shards, uint32_t* d_sel_frame,
                              hipStream_t stream);
// Work order of the supersample pass: the first *d_count of d_sel (pixel indices of a
// w x h rect, n_max entries of room) into d_out, longest expected sub-rays first -- by
// the 1-spp step counts d_steps (rect order) around each pixel -- ties in selection
// order.  Call with d_temp == NULL for *temp_bytes (n_max <= INT_MAX).
hipError_t order_selection(const uint32_t* d_sel, const unsigned long long* d_count, uint64_t n_max,
                           const uint32_t* d_steps, uint32_t w, uint32_t h, uint32_t* d_out, void* d_temp,
                           size_t* temp_bytes, hipStream_t stream);

}  // namespace grt
