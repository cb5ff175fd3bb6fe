// geodesic_lapse.hip — the exact trace kernels (integrate, tail, shade) and the geometry
// buffer fill of every chart but KerrBL (geodesic_lapse_kerr_bl.hip), built once more for grt_gbuffer_trace_lapse: the trace of a
// geometry buffer that also records each layer's light-travel time.  Same source, same flags
// and the same arithmetic as geodesic.hip (-ffp-contract=off), so the twelve arrays of the
// buffer have the bits grt_gbuffer_trace gives them.  The one difference: window_pass keeps
// the coordinate time of every candidate it records, y[0] lerped over the window by the
// chord parameter, in two arrays beside the candidates (HitPool::slot_time, pool_time), and
// this unit's gbuffer_fill_kernel writes lapse[layer] = that time - the camera's.  The lapse
// array is an extra parameter of this unit's fill kernel, and the two arrays are named at
// the end of the pool's descriptor in device memory, so the kernels of the other units are
// compiled from unchanged code and keep their argument layouts.
// No fused, volumetric, probe or trajectory kernels: the buffer's trace needs none.
#define GRT_LAPSE 1
#include "geodesic.hip"
