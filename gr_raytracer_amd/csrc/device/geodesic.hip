// geodesic.hip — gfx950 kernels for the per-pixel geodesic hot path.
//
// One lane traces one camera ray from creation to final colour, entirely in VGPRs:
//   camera ray (camera.rs:214-254) -> RKF45 attempts (runge_kutta.rs:86-182)
//   -> for every accepted step: chord window test against every object
//      (objects.rs:65-120, disc.rs:41-88, sphere.rs:37-128), emitter redshift +
//      temperature + texture (redshift.rs, temperature.rs, texture.rs), then the
//      stop test (integrator.rs:203-268)
//   -> terminal colour + back-to-front blend (scene.rs:153-219).
// The reference stores the whole trajectory (Vec<Step>, 112 B/step) and runs the
// window pass afterwards; here the window test is fused into the step loop, which
// visits exactly the same windows in the same order, so no trajectory ever leaves
// the register file.
//
// The grid is persistent: each wave claims work items from one global
// counter, and whenever lanes finish their ray a wave ballot hands them the next
// items (lane refill), so long (near-photon-sphere) and short (captured) rays never
// leave lanes idle until the queue is empty.
//
// Floating point follows the reference's evaluation order (Rust, no contraction);
// the library is compiled with -ffp-contract=off.  Per-frame constants that need
// libm (sin/cos of the camera position, tan(alpha/2), LUTs) are evaluated on the
// host.  pow() is glibc's own algorithm restated bit-exactly (glibc_math.h); the
// remaining per-step transcendentals (sin/cos/atan2/acos) use the device libm (OCML).
//
// Layers in their own files, each on the ones before it (the include sites below say
// which unit builds which):
//   geodesic_rhs.h    range-free division / sqrt, metrics, the sincos dispatch, the RHS   every unit
//   geodesic_rkf.h    RKF45 attempts, LDS stage parking                                   every unit
//   geodesic_probe.h  work-order kernels (probes, impact and class keys)                  exact build, sequence
//   geodesic_fill.h   gbuffer_fill_kernel                                                 exact build, KerrBL, sequence, lapse
// Still here, between them and in this order: chart helpers, chord tests and the camera
// ray; the trace (integrate_kernel, tail_kernel); the exact build's trajectory kernel,
// device checks and invariant monitors; shade_kernel.  The unit macros and every GRT_*
// knob are in this file (tools/build_variant.sh edits them here), and so is every launch
// function.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grt_api.h"
#include "dev_scene.h"
#ifndef GRT_GLIBC_LDS
#define GRT_GLIBC_LDS 1  // glibc tables staged in LDS per workgroup (measured -1..2%)
#endif
#include "glibc_math.h"
#include "rcp_seed.h"
#include "rkf_weights.h"
#include "kernels.h"

// GRT_FUSED: this file compiled a second time, by geodesic_fused.hip, with FMA contraction
// (-ffp-contract=fast) into namespace grt::fused: the trace kernels of the light charts
// for grt_set_arithmetic(1).  Only launch_trace is defined there (Kerr-Schild excluded).
#ifndef GRT_FUSED
#define GRT_FUSED 0
#endif
// GRT_KERR_BL_TU: this file compiled a second time, by geodesic_kerr_bl.hip, without the
// machine-level loop-invariant code motion, into namespace grt::kerr_bl: the KerrBL trace
// kernels (launch_trace for GRT_GEOM_KERR_BL only; the exact build leaves them out).
#ifndef GRT_KERR_BL_TU
#define GRT_KERR_BL_TU 0
#endif
// GRT_SEQ: this file compiled a fourth time, by geodesic_seq.hip, into namespace grt::seq:
// the exact trace and probe kernels of every chart over a stack of frames that share the
// scene but not the camera (grt_render_sequence).  Each ray takes its camera from a table
// (CamTable, an extra kernel parameter of this unit's kernels only) by the frame its
// stacked row lies in; everything else is the code of the other units.
#ifndef GRT_SEQ
#define GRT_SEQ 0
#endif
// GRT_LAPSE: this file compiled a fifth time, by geodesic_lapse.hip, into namespace
// grt::lapse: the exact trace and geometry buffer fill of every chart but KerrBL, which also
// keep the coordinate time y[0] of every recorded hit (grt_gbuffer_trace_lapse).  Everything
// else is the code of the exact units; the time goes to two arrays named at the end of HitPool.
// GRT_LAPSE_KERR_BL: and a sixth time, by geodesic_lapse_kerr_bl.hip, into namespace
// grt::lapse_kerr_bl: the same for KerrBL, built as grt::kerr_bl is (without the machine-level
// loop-invariant code motion; with it the integrate kernel spills 96 B per lane).
#ifndef GRT_LAPSE
#define GRT_LAPSE 0
#endif
#ifndef GRT_LAPSE_KERR_BL
#define GRT_LAPSE_KERR_BL 0
#endif
#define GRT_MAIN_TU (!GRT_FUSED && !GRT_KERR_BL_TU && !GRT_SEQ && !GRT_LAPSE)

namespace grt {
#if GRT_FUSED
namespace fused {
#elif GRT_KERR_BL_TU
namespace kerr_bl {
#elif GRT_SEQ
namespace seq {
#elif GRT_LAPSE && GRT_LAPSE_KERR_BL
namespace lapse_kerr_bl {
#elif GRT_LAPSE
namespace lapse {
#endif

// The camera of a ray.  The other units read the scene's; the sequence unit hands its
// camera table down to the places that create a camera ray (CAMS_*), and those pass the
// entry of the ray's frame on (CAM_*).
#if GRT_SEQ
#define CAMS_PARAM , CamTable ct
#define CAMS_ARG , ct
#define CAM_PARAM , const DevCamera& ray_cam
#define CAM_ARG(c) , c
#define CAM_OF(S) ray_cam
#else
#define CAMS_PARAM
#define CAMS_ARG
#define CAM_PARAM
#define CAM_ARG(c)
#define CAM_OF(S) (S).cam
#endif

// The lapse unit: the coordinate time of a recorded hit, handed to hit_append (HIT_TIME_*),
// and the buffer's lapse array, handed to gbuffer_fill_kernel (LAPSE_*).
#if GRT_LAPSE
#define HIT_TIME_PARAM , double th
#define HIT_TIME_ARG , th
#define LAPSE_PARAM , double* __restrict__ lapse
#define LAPSE_ARG , lapse
#else
#define HIT_TIME_PARAM
#define HIT_TIME_ARG
#define LAPSE_PARAM
#define LAPSE_ARG
#endif

#ifndef GDEV
#define GDEV __device__ __forceinline__
#endif

#ifndef GRT_SHARED_DIV
#define GRT_SHARED_DIV 1
#endif
#ifndef GRT_UNIT_H
#define GRT_UNIT_H 1  // far-field attempts of a wave with h == 1 everywhere skip h * o
#endif
#ifndef GRT_KLDS_GEOMS
#define GRT_KLDS_GEOMS (1 << GRT_GEOM_KERR)  // integrate kernels whose RKF stages k1..k4 live in LDS
#endif
#ifndef GRT_SINCOS_B
#define GRT_SINCOS_B 1  // Schwarzschild / KerrBL RHS: wave-uniform straight-line sincos (region B)
#endif
#ifndef GRT_FAST_DIV
#define GRT_FAST_DIV 1  // Schwarzschild / KerrBL region-B RHS: divisions without range steps when the operands allow
#endif
#ifndef GRT_FAST_DIV_KS
#define GRT_FAST_DIV_KS 1  // Kerr-Schild RHS: metric quotients without v_div_scale when the state allows
#endif
#ifndef GRT_FAST_SQRT_KS
#define GRT_FAST_SQRT_KS 1  // and its square roots without the range steps (sqrt_fx)
#endif
#ifndef GRT_FAST_DIV_BL
// KerrBL too: C3 is no faster with it (165-172 ms either way), but its 3-wave kernel's
// spills land elsewhere: 1.71 GB written per frame with it, 20.9 GB without
// (profiles/r04n_c3_pmc.json, r04o_c3_pmc.json)
#define GRT_FAST_DIV_BL 1
#endif
#ifndef GRT_UNIT_RADIUS
#define GRT_UNIT_RADIUS 1  // Schwarzschild region-B RHS: the quotients of radius == 1.0 without their multiplies (rcp_seed.h)
#endif
#ifndef GRT_DIV_OK_CHEAP
#define GRT_DIV_OK_CHEAP 1  // Schwarzschild RHS: the render's division predicate as two compares (schw_div_ok_render)
#endif
#ifndef GRT_RKF_SHORT
#define GRT_RKF_SHORT 1  // Schwarzschild integrate kernels: attempts without the zero-weight CH2 / CT2 terms (rkf_short_ok)
#endif
#ifndef GRT_QUICK_STEP
#define GRT_QUICK_STEP 1  // Schwarzschild: the far-field accepted step as one straight-line block
#endif
#ifndef GRT_STEADY_LOOP
#define GRT_STEADY_LOOP 1  // Schwarzschild: quick steps of a wave with h == 1 everywhere in a loop of their own (steady_step_mask)
#endif
#ifndef GRT_SCALAR_VOTES
#define GRT_SCALAR_VOTES 1  // Schwarzschild: wave votes compared as lane masks on the scalar side (wave_all)
#endif
#ifndef GRT_KL_STAGES
#define GRT_KL_STAGES 4  // how many leading stages (k1, k2, ...) those kernels park in LDS
#endif
#ifndef GRT_TAIL_PRIO
#define GRT_TAIL_PRIO 1  // light charts: issue priority by steps left once the queue drains (C5 -1.2%, profiles/r05i)
#endif
#ifndef GRT_RAY_TIMES
#define GRT_RAY_TIMES 0  // diagnostic builds only: per-ray schedule record (tools/c4_ray_times.py)
#endif
#ifndef GRT_PATH_COUNT
#define GRT_PATH_COUNT 0  // diagnostic builds only: count code paths per wave and per lane
#endif
#ifndef GRT_RK_FOLD
#define GRT_RK_FOLD 1  // running RKF sums (rkf_attempt_fold) for every chart but Kerr-Schild
#endif
#ifndef GRT_PROBE_ESCAPE
#define GRT_PROBE_ESCAPE 1  // end an outward-bound Kerr-Schild probe far from the hole at once
#endif

#include "appearance.h"

// The charts this unit builds kernels for, one bit per GRT_GEOM_*: the trace
// (launch_trace), the exact-only kernels (geometry buffer fill, work-order probes) and
// the exact build's diagnostics.
constexpr unsigned ALL_CHARTS = 0x1f, KERR_CHART = 1u << GRT_GEOM_KERR, KERR_BL_CHART = 1u << GRT_GEOM_KERR_BL;
#if GRT_MAIN_TU
constexpr unsigned TRACE_CHARTS = ALL_CHARTS & ~KERR_BL_CHART;  // the exact KerrBL trace is grt::kerr_bl's
constexpr unsigned FILL_CHARTS = TRACE_CHARTS;                  // and so is its geometry buffer fill
constexpr unsigned PROBE_CHARTS = ALL_CHARTS;
constexpr unsigned DIAG_CHARTS = ALL_CHARTS;  // trajectories, invariant monitors
constexpr unsigned RHS_CHECK_CHARTS = 1u << GRT_GEOM_SCHWARZSCHILD | KERR_CHART | KERR_BL_CHART;  // the range-free forms
#elif GRT_FUSED
constexpr unsigned TRACE_CHARTS = ALL_CHARTS & ~KERR_CHART;  // Kerr-Schild always runs exact (grt_set_arithmetic)
#elif GRT_KERR_BL_TU
constexpr unsigned TRACE_CHARTS = KERR_BL_CHART, FILL_CHARTS = KERR_BL_CHART;
#elif GRT_SEQ
constexpr unsigned TRACE_CHARTS = ALL_CHARTS, FILL_CHARTS = ALL_CHARTS, PROBE_CHARTS = ALL_CHARTS;
#elif GRT_LAPSE_KERR_BL
constexpr unsigned TRACE_CHARTS = KERR_BL_CHART, FILL_CHARTS = KERR_BL_CHART;
#else  // GRT_LAPSE
constexpr unsigned TRACE_CHARTS = ALL_CHARTS & ~KERR_BL_CHART, FILL_CHARTS = TRACE_CHARTS;
#endif

// f(std::integral_constant<int, G>()) for G = geometry when CHARTS has that chart;
// hipErrorInvalidValue otherwise.  f is instantiated for the charts of CHARTS only.
template <unsigned CHARTS, int G = 0, class F>
static hipError_t with_chart(int geometry, const F& f) {
  if constexpr ((CHARTS >> G) == 0) {
    return hipErrorInvalidValue;
  } else {
    if constexpr ((CHARTS >> G) & 1u) {
      if (geometry == G) return f(std::integral_constant<int, G>());
    }
    return with_chart<CHARTS, G + 1>(geometry, f);
  }
}

#include "geodesic_rhs.h"
#include "geodesic_rkf.h"

// ---- chart helpers ----
// Cartesian spatial position of a state (scene.rs:48-69 get_position / point.rs:125-154).
template <int G>
GDEV void to_cart(const DevScene& S, const double* y, double* c) {
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD || G == GRT_GEOM_EUCLIDEAN_SPHERICAL) {
    double st, ct, sp, cp;
    rsincos(y[2], &st, &ct);
    rsincos(y[3], &sp, &cp);
    double r = y[1];
    c[0] = r * st * cp;
    c[1] = r * st * sp;
    c[2] = r * ct;
  } else if constexpr (G == GRT_GEOM_KERR_BL) {
    double a = S.a, r = y[1];
    double st, ct, sp, cp;
    rsincos(y[2], &st, &ct);
    rsincos(y[3], &sp, &cp);
    c[0] = (r * cp - a * sp) * st;
    c[1] = (r * sp + a * cp) * st;
    c[2] = r * ct;
  } else {
    c[0] = y[1];
    c[1] = y[2];
    c[2] = y[3];
  }
}

// cartesian_to_spherical (spherical_coordinates_helper.rs:5-26): r, theta, phi
GDEV void cart_to_sph(double x, double y, double z, double* r_o, double* th_o, double* ph_o) {
  double r = sqrt(x * x + y * y + z * z);
  if (r == 0.0) {
    *r_o = 0.0;
    *th_o = 0.0;
    *ph_o = 0.0;
    return;
  }
  *r_o = r;
  *th_o = acos(z / r);
  *ph_o = atan2(y, x);
}
// cartesian_to_boyer_lindquist (spherical_coordinates_helper.rs:44-61)
GDEV void cart_to_bl(double a, double x, double y, double z, double* r_o, double* th_o, double* ph_o) {
  double rho_sqr = x * x + y * y + z * z;
  double d = rho_sqr - a * a;
  double r_sqr = 0.5 * (rho_sqr - a * a + sqrt(d * d + 4.0 * a * a * z * z));
  double r = sqrt(r_sqr);
  *r_o = r;
  *th_o = (r == 0.0) ? 0.0 : acos(rclamp(z / r, -1.0, 1.0));
  *ph_o = atan2(r * y - a * x, r * x + a * y);
}

// momentum_from_state (geometry.rs:29-31; kerr_bl.rs:225-249; kerr.rs:262-273)
template <int G>
GDEV void momentum(const DevScene& S, const RayConst& rc, const double* y, double* p) {
  if constexpr (G == GRT_GEOM_KERR_BL) {
    double a = S.a, e = rc.e, l_z = rc.lz;
    double r = y[1], theta = y[2], v_r = y[4], v_theta = y[5];
    double st, ct;
    rsincos(theta, &st, &ct);
    double del = bl_delta(r, S.radius, a);
    double sig = r * r + a * a * (ct * ct);
    double sin2 = st * st;
    double p_r_term = (r * r + a * a) * e - a * l_z;
    double dt = (r * r + a * a) / del * p_r_term + a * (l_z - a * e * sin2);
    double dphi = a / del * p_r_term + l_z / sin2 - a * e;
    p[0] = dt / sig;
    p[1] = v_r / sig;
    p[2] = v_theta / sig;
    p[3] = dphi / sig;
  } else if constexpr (G == GRT_GEOM_KERR) {
    double Gc[4][4];
    ks_metric_contra(S.radius, S.a, y[1], y[2], y[3], Gc);
    mat_vec(Gc, y + 4, p);
  } else {
    p[0] = y[4];
    p[1] = y[5];
    p[2] = y[6];
    p[3] = y[7];
  }
}

// x unchanged, through an empty volatile asm: the compiler can neither hoist what is
// computed from the result out of the branch it sits in nor merge it with the same
// computation on x elsewhere.
GDEV double opaque(double x) {
  asm volatile("" : "+v"(x));
  return x;
}
// The window pass's lerped momentum of a hit, sw p(ya) + t p(yb) (objects.rs:27-44).
// KerrBL reads the momentum's inputs through opaque(): otherwise both momenta, invariant
// in the object loop, have their sincos-free parts computed before the loop for every
// near-field window and kept live across it, and the 3-wave kernel spills them (the
// scratch stores of C3: 1.75 GB written per frame).  Now they are computed only for a
// recorded hit (1.55M of 1.79e9 C3 steps), with the same operations on the same values.
// (An out-of-line function does the same for the spills, but the call makes the kernel
// rematerialise its SGPR constants around it: +20% scalar instructions, +1.5% time.)
template <int G>
GDEV void lerp_momentum(const DevScene& S, const RayConst& rc, const double* ya, const double* yb, double t,
                        double* ph) {
  double pa[4], pb[4];
  if constexpr (G == GRT_GEOM_KERR_BL) {
    const double a8[8] = {0.0, opaque(ya[1]), opaque(ya[2]), 0.0, opaque(ya[4]), opaque(ya[5]), 0.0, 0.0};
    const double b8[8] = {0.0, opaque(yb[1]), opaque(yb[2]), 0.0, opaque(yb[4]), opaque(yb[5]), 0.0, 0.0};
    momentum<G>(S, rc, a8, pa);
    momentum<G>(S, rc, b8, pb);
  } else {
    momentum<G>(S, rc, ya, pa);
    momentum<G>(S, rc, yb, pb);
  }
  const double sw = 1.0 - t;
#pragma unroll
  for (int q = 0; q < 4; ++q) ph[q] = sw * pa[q] + t * pb[q];
}

// inner_product at a native-chart point whose polar-angle sin/cos are given.
template <int G>
GDEV double inner(const DevScene& S, const double* pos, double st, double ct, const double* v,
                  const double* w) {
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD) {  // schwarzschild.rs:90-102
    double r = pos[1];
    double a = 1.0 - S.radius / r;
    return a * v[0] * w[0] - v[1] * w[1] / a - r * r * v[2] * w[2] - r * r * st * st * v[3] * w[3];
  } else if constexpr (G == GRT_GEOM_EUCLIDEAN_SPHERICAL) {  // euclidean_spherical.rs:80-91
    double r = pos[1];
    return 1.0 * v[0] * w[0] - v[1] * w[1] - r * r * v[2] * w[2] - r * r * st * st * v[3] * w[3];
  } else if constexpr (G == GRT_GEOM_KERR_BL) {  // kerr_bl.rs:338-359
    double g[4][4];
    metric_bl(S.radius, S.a, pos[1], st, ct, g);
    double result = 0.0;
#pragma unroll
    for (int mu = 0; mu < 4; ++mu)
#pragma unroll
      for (int nu = 0; nu < 4; ++nu) result += g[mu][nu] * v[mu] * w[nu];
    return result;
  } else if constexpr (G == GRT_GEOM_KERR) {  // kerr.rs:283-287
    double g[4][4];
    ks_metric(S.radius, S.a, pos[1], pos[2], pos[3], g);
    return quad_form(v, g, w);
  } else {  // euclidean.rs:62-67
    return 1.0 * v[0] * w[0] + -v[1] * w[1] + -v[2] * w[2] + -v[3] * w[3];
  }
}
template <int G>
GDEV double signature0() {
  return (G == GRT_GEOM_KERR || G == GRT_GEOM_KERR_BL) ? -1.0 : 1.0;
}

// get_stationary_velocity_at (schwarzschild.rs:237-240; kerr.rs:449-455; kerr_bl.rs:362-371)
template <int G>
GDEV void stationary_velocity(const DevScene& S, const double* pos, double* u) {
  u[1] = 0.0;
  u[2] = 0.0;
  u[3] = 0.0;
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD) {
    double a = 1.0 - S.radius / pos[1];
    u[0] = 1.0 / sqrt(a);
  } else if constexpr (G == GRT_GEOM_KERR_BL) {
    double r = pos[1];
    double ct = rcos(pos[2]);  // kerr_bl.rs:362-371 evaluates sigma alone: a lone cos()
    double sig = r * r + S.a * S.a * (ct * ct);
    u[0] = 1.0 / sqrt(1.0 - S.radius * r / sig);
  } else if constexpr (G == GRT_GEOM_KERR) {
    double a = S.a, z = pos[3];
    double r_sqr = ks_r_sqr(a, pos[1], pos[2], pos[3]);
    double r = sqrt(r_sqr);
    double f = (r * r * r * S.radius) / (r * r * r * r + a * a * z * z);
    u[0] = 1.0 / sqrt(1.0 - f);
  } else {
    u[0] = 1.0;
  }
}

// circular_orbit::killing_coefficients (circular_orbit.rs:76-108)
GDEV bool killing_coefficients(const DevScene& S, double r, double* u_t, double* u_phi) {
  double r_s = S.radius, a = S.a;
  double m = 0.5 * r_s;
  double sqrt_m = sqrt(m);
  double omega = sqrt_m / (rpow(r, 1.5) + a * sqrt_m);
  double c = S.cos_half_pi, s = S.sin_half_pi;
  double sig = r * r + a * a * (c * c);
  double sin2 = s * s;
  double g_tt = -(1.0 - r_s * r / sig);
  double g_tphi = -a * r_s * r * sin2 / sig;
  double g_phiphi = (r * r + a * a + a * a * r_s * r * sin2 / sig) * sin2;
  double ut_pre = g_tt + 2.0 * omega * g_tphi + omega * omega * g_phiphi;
  if (ut_pre >= 0.0) return false;
  double ut = 1.0 / sqrt(-ut_pre);
  *u_t = ut;
  *u_phi = omega * ut;
  return true;
}

#include "volumetric.h"

// ====================================================== window (chord) tests ======
// Geometry only: the integrate kernel decides hit / no hit, the chord parameter t and
// the hit point; everything that needs the emitter (energy, temperature, colour) is
// evaluated later by the shade kernel from the recorded point and momentum.

// disc.rs:41-88.  The sign / magnitude pre-filter only skips divisions whose quotient
// is provably outside [0, 1] (and cannot underflow to -0); every accepted t is the
// same correctly rounded p1 / p2 the reference computes.
GDEV bool disc_chord(const DevObject& o, const double* s, const double* e, double* t_out, double* ip) {
  double d0 = e[0] - s[0], d1 = e[1] - s[1], d2 = e[2] - s[2];
  double p1 = (0.0 - s[0]) * 0.0 + (0.0 - s[1]) * 0.0 + (0.0 - s[2]) * 1.0;
  double p2 = d0 * 0.0 + d1 * 0.0 + d2 * 1.0;
  double a1 = fabs(p1), a2 = fabs(p2);
  if (a1 > 1e-200 && a2 < 1e100 && ((p1 > 0.0 && p2 < 0.0) || (p1 < 0.0 && p2 > 0.0))) return false;  // t < 0
  if (a1 > 2.0 * a2) return false;                                                                    // t > 2
  double t = p1 / p2;
  if (!(0.0 <= t && t <= 1.0)) return false;
  double ix = s[0] + t * d0, iy = s[1] + t * d1, iz = s[2] + t * d2;
  double rr = ix * ix + iy * iy + iz * iz;
  if (!(rr >= o.rin2 && rr <= o.rout2)) return false;
  *t_out = t;
  ip[0] = ix;
  ip[1] = iy;
  ip[2] = iz;
  return true;
}

// sphere.rs:37-128; returns the hit point in the sphere's local frame.
GDEV bool sphere_chord(const DevObject& o, const double* s_w, const double* e_w, double* t_out, double* lp) {
  double s0 = s_w[0] + -o.cx, s1 = s_w[1] + -o.cy, s2 = s_w[2] + -o.cz;
  double e0 = e_w[0] + -o.cx, e1 = e_w[1] + -o.cy, e2 = e_w[2] + -o.cz;
  double r_start = s0 * s0 + s1 * s1 + s2 * s2;
  double r_end = e0 * e0 + e1 * e1 + e2 * e2;
  double R2 = o.R2;
  if (!((r_start >= R2 && r_end <= R2) || (r_start <= R2 && r_end >= R2))) return false;
  double d0 = e0 - s0, d1 = e1 - s1, d2 = e2 - s2;
  double a = d0 * d0 + d1 * d1 + d2 * d2;
  double b = 2.0 * (s0 * d0 + s1 * d1 + s2 * d2);
  double c = (s0 * s0 + s1 * s1 + s2 * s2) - o.radius * o.radius;
  double disc = b * b - 4.0 * a * c;
  if (disc < 0.0) return false;
  double sq = sqrt(disc);
  double t1 = (-b + sq) / (2.0 * a);
  double t2 = (-b - sq) / (2.0 * a);
  double t;
  if (0.0 <= t1 && t1 <= 1.0) t = t1;
  else if (0.0 <= t2 && t2 <= 1.0) t = t2;
  else return false;
  *t_out = t;
  lp[0] = s0 + t * d0;
  lp[1] = s1 + t * d1;
  lp[2] = s2 + t * d2;
  return true;
}

// ======================================================== integrate kernel =======
// camera.rs:214-232 get_direction_for, then momentum = direction - e_t (:243, :252)
GDEV void camera_momentum(const DevCamera& c, double row, double column, double* p) {
  double shifted_column = column + 1.0;
  double shifted_row = row + 1.0;
  double tha = c.tan_half_alpha;
  double i_prime = c.hand * (2.0 * tha / c.rows) * (shifted_column - (c.cols + 1.0) / 2.0);
  double j_prime = (2.0 * tha / c.rows) * (shifted_row - (c.rows + 1.0) / 2.0);
  double w_squared = c.sig_s * (1.0 + i_prime * i_prime + j_prime * j_prime);
  double denom = c.sig_s * w_squared;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double w = c.tet[3][k] + i_prime * c.tet[1][k] + j_prime * c.tet[2][k];
    double dir = -c.tet[3][k] + 2.0 * w / denom;
    p[k] = dir + (-c.tet[0][k]);
  }
}

// Initial ODE state of a ray at native-chart position `pos` with contravariant momentum
// `p` (integrator.rs:82-99 + the geometry's get_geodesic_solver / create_initial_state);
// st, ct = sin / cos of pos[2] (KerrBL only).  Fills the KerrBL constants E, L_z, Q.
template <int G>
GDEV void init_state(const DevScene& S, const double* pos, double st, double ct, const double* p, double* y,
                     RayConst& rc) {
  rc.e = 0.0;
  rc.lz = 0.0;
  rc.q = 0.0;
  if constexpr (G == GRT_GEOM_KERR_BL) {  // kerr_bl.rs:505-577, :176-223 (BL ray)
    double a = S.a, radius = S.radius;
    double r = pos[1];
    double g[4][4];
    metric_bl(radius, a, r, st, ct, g);
    double pc[4];
    mat_vec(g, p, pc);
    double e = -pc[0], l_z = pc[3], p_theta = pc[2];
    double sin2 = st * st;
    double q = p_theta * p_theta + ct * ct * (l_z * l_z / fmax(sin2, 1e-28) - a * a * e * e);
    rc.e = e;
    rc.lz = l_z;
    rc.q = q;
    double sign_r = p[1] >= 0.0 ? 1.0 : -1.0;
    double sign_theta = p[2] >= 0.0 ? 1.0 : -1.0;
    double del = bl_delta(r, radius, a);
    double p_r = (r * r + a * a) * e - a * l_z;
    double le = l_z - a * e;
    double r_pot = p_r * p_r - del * (le * le + q);
    double th_pot = q + a * a * e * e * ct * ct - l_z * l_z * ct * ct / (st * st);
    y[0] = pos[0];
    y[1] = r;
    y[2] = pos[2];
    y[3] = pos[3];
    y[4] = sign_r * sqrt(fmax(r_pot, 0.0));
    y[5] = sign_theta * sqrt(fmax(th_pot, 0.0));
    y[6] = 0.0;
    y[7] = 0.0;
  } else if constexpr (G == GRT_GEOM_KERR) {  // kerr.rs:243-260
    double g[4][4];
    ks_metric(S.radius, S.a, pos[1], pos[2], pos[3], g);
    double pc[4];
    mat_vec(g, p, pc);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      y[k] = pos[k];
      y[4 + k] = pc[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      y[k] = pos[k];
      y[4 + k] = p[k];
    }
  }
}

// The camera of integer row *R of a work list, and *R as a row of that camera's frame.
// The scene's camera, and *R as it is; in the sequence unit, over stacked frames: integer
// row R of the stack is row R % cam_rows of frame R / cam_rows.  Always from the integer
// row, before any sub-pixel jitter (a jittered row may leave its frame by half a pixel).
// A row past the table (the host never makes one) takes the last camera, so that no load
// leaves the table.
GDEV const DevCamera& frame_camera(const DevScene& S, uint32_t* R CAMS_PARAM) {
#if GRT_SEQ
  const uint32_t f = min(*R / ct.cam_rows, ct.n_cams - 1u);
  *R -= f * ct.cam_rows;
  return ct.cams[f];
#else
  return S.cam;
#endif
}
// The pixel (r, c) of a work list's rectangle / row-band shard (local row r mapped to its
// frame row): its image coordinates within its frame, and its camera.
GDEV const DevCamera& rect_pixel(const DevScene& S, const WorkList& wl, uint32_t r, uint32_t c, double* row,
                                 double* col CAMS_PARAM) {
  uint32_t ri = wl.row0 + shard_frame_row(wl.band_rows, wl.shard, wl.n_shards, r);
  const DevCamera& cam = frame_camera(S, &ri CAMS_ARG);
  *row = (double)ri;
  *col = (double)(wl.col0 + c);
  return cam;
}
// The same of the ray in output slot idx of a work list: an offset list's jittered pixel
// (get_ray_for_offset, camera.rs:247-254), or rectangle pixel (idx / cols, idx % cols).
GDEV const DevCamera& ray_pixel(const DevScene& S, const WorkList& wl, uint64_t idx, double* row,
                                double* col CAMS_PARAM) {
  if (wl.pixel_index) {
    const uint32_t pix = wl.pixel_index[idx];
    uint32_t ri = wl.row0 + pix / wl.cols;
    const DevCamera& cam = frame_camera(S, &ri CAMS_ARG);
    const double r = (double)ri, cc = (double)(wl.col0 + pix % wl.cols);
    *row = r + (wl.dy[idx] - 0.5);
    *col = cc + (wl.dx[idx] - 0.5);
    return cam;
  }
  return rect_pixel(S, wl, (uint32_t)(idx / wl.cols), (uint32_t)(idx % wl.cols), row, col CAMS_ARG);
}

// Create a camera ray's state (camera.rs:234-254 + init_state); also the observer
// energy the redshift needs (redshift.rs:40-43).
template <int G, bool FREQ = false>
GDEV void init_ray(const DevScene& S, double row, double col, double* y, RayConst& rc CAM_PARAM) {
  const DevCamera& cam = CAM_OF(S);
  double p[4];
  camera_momentum(cam, row, col, p);
  init_state<G>(S, cam.pos, cam.sin_theta, cam.cos_theta, p, y, rc);
  rc.obs = inner<G>(S, cam.pos, cam.sin_theta, cam.cos_theta, cam.vel, p);  // = observer_energy
  rc.pt = 0.0;
  rc.pphi = 0.0;
  if constexpr (FREQ) {  // get_ray_frequency_data: <e_t, p> and <axial Killing vector, p>
    const double et[4] = {1.0, 0.0, 0.0, 0.0};
    double ax[4] = {0.0, 0.0, 0.0, 1.0};  // d_phi (schwarzschild.rs:256, kerr_bl.rs:394, ...)
    if constexpr (G == GRT_GEOM_EUCLIDEAN || G == GRT_GEOM_KERR) {  // (0, -y, x, 0), kerr.rs:482-485
      ax[1] = -cam.pos[2];
      ax[2] = cam.pos[1];
      ax[3] = 0.0;
    }
    rc.pt = inner<G>(S, cam.pos, cam.sin_theta, cam.cos_theta, et, p);
    rc.pphi = inner<G>(S, cam.pos, cam.sin_theta, cam.cos_theta, ax, p);
  }
}
// The camera ray of rectangle pixel (r, c) of a work list.
template <int G>
GDEV void init_rect_ray(const DevScene& S, const WorkList& wl, uint32_t r, uint32_t c, double* y,
                        RayConst& rc CAMS_PARAM) {
  double row, col;
  [[maybe_unused]] const DevCamera& cam = rect_pixel(S, wl, r, c, &row, &col CAMS_ARG);
  init_ray<G>(S, row, col, y, rc CAM_ARG(cam));
}

// integrator.rs:203-268
template <int G>
GDEV int should_stop(const DevScene& S, const double* y, double* c, bool& c_valid, uint64_t i) {
  if (!(isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]) && isfinite(y[3]))) return GRT_STOP_NAN;
  bool last = (i == S.max_steps - 1);
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD || G == GRT_GEOM_KERR_BL) {
    if (G == GRT_GEOM_SCHWARZSCHILD || S.has_horizon) {
      if (y[1] <= S.horizon_r) return GRT_STOP_HORIZON;
    }
    if (last && y[1] < S.trapped_radius) return GRT_STOP_CLOSED_ORBIT;
  } else if constexpr (G == GRT_GEOM_KERR) {
    double r = sqrt(ks_r_sqr(S.a, y[1], y[2], y[3]));
    if (S.has_horizon && r <= S.horizon_r) return GRT_STOP_HORIZON;
    if (last && r < S.trapped_radius) return GRT_STOP_CLOSED_ORBIT;
  }
  // celestial test |x_cart|^2 > max_radius^2 (integrator.rs:203-268).  |x_cart| lies in
  // [|r|, |r| + far_a] in the curvilinear charts, so away from the celestial shell the
  // answer follows from r and the conversion is skipped.
  bool escaped = false, decided = false;
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD || G == GRT_GEOM_KERR_BL || G == GRT_GEOM_EUCLIDEAN_SPHERICAL) {
    if (!c_valid && S.far_ok) {
      double ar = fabs(y[1]), hi = ar + S.far_a;
      if (hi * hi < S.cel_lo2) decided = true;
      else if (ar * ar > S.cel_hi2) decided = escaped = true;
    }
  }
  if (!decided) {
    if (!c_valid) {
      to_cart<G>(S, y, c);
      c_valid = true;
    }
    escaped = c[0] * c[0] + c[1] * c[1] + c[2] * c[2] > S.max_radius_sq;
  }
  if (escaped) return GRT_STOP_CELESTIAL;
  if (!(isfinite(y[4]) && isfinite(y[5]) && isfinite(y[6]) && isfinite(y[7]))) return GRT_STOP_NAN;
  return GRT_STOP_NONE;
}

// Exact far-field window filter (curvilinear charts).  True when neither end of the
// window (ya -> yb) can produce a hit in the reference's chord tests, decided from r and
// theta alone, so the Cartesian conversion and the chord arithmetic can be skipped:
//  * Disc (disc.rs:41-88): z = r cos(theta) keeps one strict sign, with |z| >= 1e-9 r at
//    both ends and r_a / r_b within [1e-3, 1e3], so t = -z_a / (z_b - z_a) is outside
//    [0, 1] by a factor ~1e-12, far above rounding (theta within 1e-9 of a zero of cos,
//    or outside (-pi/2, 3pi/2), is always converted).
//  * Sphere (sphere.rs:37-128): a hit needs |x - c|^2 - R^2 to change sign over the
//    window; |x| in [r, r + far_a] outside the host's shell [shell_lo, shell_hi]
//    (1e-9 margins) keeps both ends strictly outside.
//  * VolumetricDisc (volumetric_disc.rs:442-494): every hit lies in the capture region
//    |x.axis| <= cap_h, |x x axis| <= rout.  Skipped when (1) the chord stays farther than
//    vol_far_r = 2 |capture corner| (1 + 1e-6) from the origin: |x| >= r at both ends and
//    the chord is no longer than the chart path, |dr| + (r_max + far_a)(|dtheta| + |dphi|)
//    (the map's partial derivatives are bounded by 1, r + |a|, r + |a|); or (2) for the z
//    axis, both ends in one hemisphere with |z| = r |cos theta| >= r (2/pi) x (Jordan's
//    inequality, x = distance of theta to the equator) beyond cap_h (1 + 1e-6): z is
//    linear along the chord, so it never enters the slab.  Only for radii below
//    vol_rmax = 1e6 cap_h, where the chord arithmetic's rounding is far below the margins.
GDEV bool vol_far(const DevScene& S, const DevObject& o, const double* ya, const double* yb) {
  const double ra = ya[1], rb = yb[1];
  if (!(ra > 0.0 && rb > 0.0)) return false;
  const double rmax = fmax(ra, rb);
  if (!(rmax < o.vol_rmax)) return false;
  const double L = fabs(rb - ra) + (rmax + S.far_a) * (fabs(yb[2] - ya[2]) + fabs(yb[3] - ya[3]));
  if (fmin(ra, rb) > o.vol_far_r + L * (1.0 + 1e-9)) return true;
  if (!o.vol_slab_ok) return false;
  constexpr double N_LO = -1.5707963257948966, N_HI = 1.5707963257948966;  // (-pi/2, pi/2) -/+ 1e-9
  constexpr double S_LO = 1.5707963277948966, S_HI = 4.7123889793846899;   // (pi/2, 3pi/2) +/- 1e-9
  constexpr double HALF_PI = 1.5707963267948966, TWO_OVER_PI = 0.63661977236758134;
  const double ta = ya[2], tb = yb[2];
  double xa, xb;
  if (ta > N_LO && ta < N_HI && tb > N_LO && tb < N_HI) {
    xa = HALF_PI - fabs(ta);
    xb = HALF_PI - fabs(tb);
  } else if (ta > S_LO && ta < S_HI && tb > S_LO && tb < S_HI) {
    xa = HALF_PI - fabs(ta - PI);
    xb = HALF_PI - fabs(tb - PI);
  } else {
    return false;
  }
  const double za = ra * TWO_OVER_PI * (xa - 1e-15) * (1.0 - 1e-9);
  const double zb = rb * TWO_OVER_PI * (xb - 1e-15) * (1.0 - 1e-9);
  return za > o.vol_slab_h && zb > o.vol_slab_h;
}

template <int G, bool VOL>
GDEV bool window_far(const DevScene& S, const double* ya, const double* yb) {
  if constexpr (G != GRT_GEOM_SCHWARZSCHILD && G != GRT_GEOM_KERR_BL && G != GRT_GEOM_EUCLIDEAN_SPHERICAL) {
    return false;
  } else {
    if (!S.far_ok) return false;
    const double ra = ya[1], rb = yb[1], ta = ya[2], tb = yb[2];
    constexpr double N_LO = -1.5707963257948966, N_HI = 1.5707963257948966;  // (-pi/2, pi/2) -/+ 1e-9
    constexpr double S_LO = 1.5707963277948966, S_HI = 4.7123889793846899;   // (pi/2, 3pi/2) +/- 1e-9
    for (uint32_t k = 0; k < S.n_objects; ++k) {
      const DevObject& o = S.obj[k];
      if (o.kind == GRT_OBJ_DISC) {
        bool north = ta > N_LO && ta < N_HI && tb > N_LO && tb < N_HI;
        bool south = ta > S_LO && ta < S_HI && tb > S_LO && tb < S_HI;
        if (!(north || south)) return false;
        if (!(ra >= 1e-3 * rb && rb >= 1e-3 * ra && ra > 0.0)) return false;
      } else if (VOL && o.kind == GRT_OBJ_VOLUMETRIC_DISC) {
        if (!vol_far(S, o, ya, yb)) return false;
      } else {
        bool out_a = ra > o.shell_hi || fabs(ra) + S.far_a < o.shell_lo;
        bool out_b = rb > o.shell_hi || fabs(rb) + S.far_a < o.shell_lo;
        if (!(out_a && out_b)) return false;
      }
    }
    return true;
  }
}

// The premise of rkf_attempt_fold's lemma for the result of a short attempt: every yn[k]
// finite and not -0 (one v_cmp_class_f64 each: -normal, -subnormal, +0, +subnormal,
// +normal), and err_sq finite.  Where it holds, the full attempt has the same bits.
constexpr int FINITE_NOT_NEG_ZERO = 0x008 | 0x010 | 0x040 | 0x080 | 0x100;
GDEV bool finite_not_neg_zero8(const double* yn) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) ok = ok & __builtin_amdgcn_class(yn[k], FINITE_NOT_NEG_ZERO);
  return ok;
}
GDEV bool rkf_short_ok(double err_sq, const double* yn) {
  return finite_not_neg_zero8(yn) & (bool)isfinite(err_sq);
}

// The commonest accepted step of a curvilinear chart as one predicate, evaluated without
// branches over the lanes (integrate_kernel's quick step): step_control's first case
// (err_sq < tiny_err_sq: accepted, next h = clamp(4h)), window_far for every object (no
// chord test, c_valid = false) and should_stop's checks all passing on yn with the
// celestial test decided by r (finite, outside the horizon, inside the celestial shell,
// not the last step).  True only where the general path does exactly the quick step's
// updates; every other case takes the general path.
// SHORT: yn and err_sq come from a short attempt (rkf_attempt_fold).  The finiteness
// tests on yn become "finite and not -0", which with err_sq < tiny_err_sq is rkf_short_ok:
// a wave on the quick path holds the full attempt's bits at no extra cost, and a ray with a
// +0 component stays on it.
template <int G, bool SHORT = false>
GDEV bool quick_step_ok(const DevScene& S, double err_sq, const double* y, const double* yn, uint64_t i_next) {
  static_assert(G == GRT_GEOM_SCHWARZSCHILD, "quick step: Schwarzschild only");
  constexpr double N_LO = -1.5707963257948966, N_HI = 1.5707963257948966;
  constexpr double S_LO = 1.5707963277948966, S_HI = 4.7123889793846899;
  const double ra = y[1], rb = yn[1], ta = y[2], tb = yn[2];
  bool ok = (err_sq < S.tiny_err_sq) & (S.far_ok != 0);
  const bool north = (ta > N_LO) & (ta < N_HI) & (tb > N_LO) & (tb < N_HI);
  const bool south = (ta > S_LO) & (ta < S_HI) & (tb > S_LO) & (tb < S_HI);
  const bool ratio = (ra >= 1e-3 * rb) & (rb >= 1e-3 * ra) & (ra > 0.0);
  for (uint32_t k = 0; k < S.n_objects; ++k) {
    const DevObject& o = S.obj[k];
    const bool out_a = (ra > o.shell_hi) | (fabs(ra) + S.far_a < o.shell_lo);
    const bool out_b = (rb > o.shell_hi) | (fabs(rb) + S.far_a < o.shell_lo);
    ok = ok & ((o.kind == GRT_OBJ_DISC) ? ((north | south) & ratio) : (out_a & out_b));
  }
  bool fin = true;
  if constexpr (SHORT) {
    fin = finite_not_neg_zero8(yn);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) fin = fin & (bool)isfinite(yn[k]);
  }
  const double ar = fabs(rb), hi = ar + S.far_a;
  return ok & fin & (rb > S.horizon_r) & (hi * hi < S.cel_lo2) & (i_next != S.max_steps - 1);
}

// The scene constants of quick_step_ok that integrate_kernel's steady loop reads, taken
// once at the loop's entry (a scene of at most STEADY_OBJECTS objects: every Schwarzschild
// scene of the reference has at most two).  Wave-uniform flags are lane masks, all or none.
constexpr uint32_t STEADY_OBJECTS = 2;
struct SteadyScene {
  double tiny_err_sq, horizon_r, cel_lo2;
  uint64_t last;  // max_steps - 1
  double shell_lo[STEADY_OBJECTS], shell_hi[STEADY_OBJECTS];
  uint64_t off[STEADY_OBJECTS], disc[STEADY_OBJECTS];  // no object k; object k is a disc
};
GDEV SteadyScene steady_scene(const DevScene& S) {
  SteadyScene q;
  q.tiny_err_sq = S.tiny_err_sq;
  q.horizon_r = S.horizon_r;
  q.cel_lo2 = S.cel_lo2;
  q.last = S.max_steps - 1;
#pragma unroll
  for (uint32_t k = 0; k < STEADY_OBJECTS; ++k) {
    const DevObject& o = S.obj[k];  // obj[] has 8 slots
    q.off[k] = k < S.n_objects ? 0ull : ~0ull;
    q.disc[k] = o.kind == GRT_OBJ_DISC ? ~0ull : 0ull;
    q.shell_lo[k] = o.shell_lo;
    q.shell_hi[k] = o.shell_hi;
  }
  return q;
}
// Whether the steady loop may run for this scene: the objects fit SteadyScene;
// horizon_r >= 0, so that rb > horizon_r of one step proves ra > 0 on the next; and
// far_a == 0 (every Schwarzschild scene: api.hip), so that |rb| + far_a is |rb| (|rb| is
// never -0, and x + 0.0 is x for every other x).
GDEV bool steady_scene_ok(const DevScene& S) {
  return S.n_objects <= STEADY_OBJECTS && S.horizon_r >= 0.0 && S.far_a == 0.0;
}

// The lanes that pass quick_step_ok<G, true> in integrate_kernel's steady loop, where y is
// the yn of a step that passed quick_step_ok (or this) on the same lanes with the same
// scene.  The tests on (ra, ta) that the b-side tests of that step imply are dropped
// (DESIGN section 4): far_ok; ta inside one of the two theta bands, so one compare against a
// bound between them says which; ra > 0.0 (ra > horizon_r >= 0, steady_scene_ok); out_a of
// every object (out_b of that step, the same expression on the same values).  Every compare
// is voted on by itself and the votes are combined as masks (wave_all's reason): the result
// equals the executing lanes' mask iff quick_step_ok holds on all of them.
template <int G>
GDEV uint64_t steady_step_mask(const SteadyScene& q, double err_sq, const double* y, const double* yn, uint64_t i_next) {
  static_assert(G == GRT_GEOM_SCHWARZSCHILD, "quick step: Schwarzschild only");
  constexpr double N_LO = -1.5707963257948966, N_HI = 1.5707963257948966;
  constexpr double S_LO = 1.5707963277948966, S_HI = 4.7123889793846899;
  const double ra = y[1], rb = yn[1], ta = y[2], tb = yn[2];
  const uint64_t a_north = __ballot(ta < N_HI);  // ta < N_HI (north band) or ta > S_LO > N_HI (south band)
  const uint64_t north = a_north & __ballot(tb > N_LO) & __ballot(tb < N_HI);
  const uint64_t south = ~a_north & __ballot(tb > S_LO) & __ballot(tb < S_HI);
  const uint64_t disc_ok = (north | south) & __ballot(ra >= 1e-3 * rb) & __ballot(rb >= 1e-3 * ra);
  const double hi = fabs(rb);
  uint64_t ok = __ballot(err_sq < q.tiny_err_sq);
#pragma unroll
  for (uint32_t k = 0; k < STEADY_OBJECTS; ++k) {
    const uint64_t out_b = __ballot(rb > q.shell_hi[k]) | __ballot(hi < q.shell_lo[k]);
    ok &= q.off[k] | (q.disc[k] & disc_ok) | (~q.disc[k] & out_b);
  }
  // one vote for the eight class tests: a v_cmp_class result is not taken as a lane mask
  ok &= __ballot(finite_not_neg_zero8(yn));
  return ok & __ballot(rb > q.horizon_r) & __ballot(hi * hi < q.cel_lo2) & __ballot(i_next != q.last);
}

// The step-size controller of rkf45 (runge_kutta.rs:148-178) after one attempt with
// error norm `err` at step h_cur.  Accepted: h_next is the next step's h.  Rejected:
// h_cur is the retry's step (STEP_RETRY), or the 100th retry failed (STEP_FAILED,
// Err(MaxStepsReached)).
enum { STEP_ACCEPTED = 0, STEP_RETRY = 1, STEP_FAILED = 2 };
GDEV int step_control(const DevScene& S, double err_sq, double& h_cur, int& retries, double& h_next) {
  // err_sq < tiny_err_sq (host: min(pow_skip_err, small_lo)^2 * (1 - 1e-9)) proves
  // err = sqrt(err_sq) < both thresholds (and < eps): accepted with h_next = clamp(4h),
  // the outcome of every branch below, without the sqrt (the far-field steps)
  if (err_sq < S.tiny_err_sq) {
    h_next = rclamp(h_cur * H_GROWTH, H_MIN, H_MAX);
    return STEP_ACCEPTED;
  }
  const double err = sqrt(err_sq);
  // h_prop = err > 0 ? BETA*h*(eps/err)^(1/5) : 4h, then min(., 4h).  For eps/err >= 1800,
  // BETA*1800^(1/5) = 4.0308 > 4, so the min is 4h whatever pow's last ulp: pow is
  // skipped there (the far-field steps), which leaves every result bit-identical.
  // err < pow_skip_err (host: eps/1800 * (1 - 1e-9)) proves eps/err > 1800: the division
  // is skipped with the pow.
  double h_prop = h_cur * H_GROWTH;
  if (err > 0.0 && !(err < S.pow_skip_err)) {
    const double ratio = S.epsilon / err;
    if (ratio < POW_SATURATED) h_prop = BETA * h_cur * rpow(ratio, INV_ORDER);
  }
  h_prop = rclamp(fmin(h_prop, h_cur * H_GROWTH), H_MIN, H_MAX);
  if (err > S.epsilon) {
    if (h_cur <= H_MIN) {
      h_next = h_cur;
      return STEP_ACCEPTED;
    }
    h_cur = rclamp(h_prop / 2.0, H_MIN, H_MAX);
    return (++retries >= MAX_RETRY) ? STEP_FAILED : STEP_RETRY;
  }
  // err / eps < 1e-5, decided without the division away from the threshold (1e-9 margins)
  const bool small = err < S.small_lo || (!(err > S.small_hi) && err / S.epsilon < SMALL_ERR);
  h_next = small ? rclamp(h_cur * H_GROWTH, H_MIN, H_MAX) : h_prop;
  return STEP_ACCEPTED;
}

#if GRT_RAY_TIMES
// Per-ray schedule record of a diagnostic build, [6][n] words at output slot idx: start,
// hand-off and end (s_memrealtime, 100 MHz), the starting lane's hardware place
// (XCC_ID << 32 | HW_ID), attempts in the integrate kernel, attempts in the tail kernel.
__device__ unsigned long long* g_ray_times;
GDEV void ray_time(uint64_t n, uint64_t idx, int k, unsigned long long v) {
  if (g_ray_times) g_ray_times[(uint64_t)k * n + idx] = v;
}
GDEV unsigned long long hw_place() {
  const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_REG_HW_ID
  const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));  // HW_REG_XCC_ID
  return ((unsigned long long)xcc << 32) | hw;
}
#if GRT_MAIN_TU  // the KerrBL unit's kernels record too
hipError_t set_ray_times(unsigned long long* p) {
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_ray_times), &p, sizeof(p));
  return e != hipSuccess ? e : kerr_bl::set_ray_times(p);
}
#elif GRT_KERR_BL_TU
hipError_t set_ray_times(unsigned long long* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_ray_times), &p, sizeof(p)); }
#endif
#define RAY_TIME(n, idx, k, v) ray_time(n, idx, k, v)
#else
#define RAY_TIME(n, idx, k, v) ((void)0)
#endif
#if GRT_KERR_BL_TU && GRT_PATH_COUNT
hipError_t path_read(unsigned long long* out, bool reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_path), sizeof(g_path));
  if (e == hipSuccess && reset) {
    const unsigned long long z[2 * NPATH] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_path), z, sizeof(z));
  }
  return e;
}
#endif

// The observer energy of the camera ray in output slot idx (init_ray's rc.obs, recomputed
// by the shade kernels instead of stored).
template <int G>
GDEV double observer_energy(const DevScene& S, const WorkList& wl, uint64_t idx CAMS_PARAM) {
  double row, col, p[4];
  const DevCamera& cam = ray_pixel(S, wl, idx, &row, &col CAMS_ARG);
  camera_momentum(cam, row, col, p);
  return inner<G>(S, cam.pos, cam.sin_theta, cam.cos_theta, cam.vel, p);
}

// The record of a ray (Workspace::fin, 8 doubles = one 64-B line, written whole by the
// lane that ends it): what the shade kernel reads of the final state and the ray
// constants, and the ray's counts.
//   Schwarzschild, Kerr-Schild, flat charts: y[1..7] (y[0] is not read; Kerr-Schild's
//   momentum needs none of E, L_z, Q), then the candidate count (low 32 bits), stop
//   reason and status (bits 32-39, 40-47).  The observer energy is not stored: the shade
//   kernel recomputes it from the ray's pixel (observer_energy: init_ray's operations on
//   the same operands, hence the same bits), and the step count goes straight to the
//   optional per-pixel output (Workspace::steps).
//   KerrBL: r, theta, phi, v_r, v_theta, observer energy, E, L_z (y[6], y[7] are
//   identically 0, Q only drives the RHS), and the counts in a 16-B meta record.  The
//   one-record layout measured C3 +8% (its 3-wave kernel's spills moved into the
//   accepted-step path: profiles/r04r), so KerrBL keeps this one.
struct RayMeta {
  uint32_t nrec, steps;
  int stop, status;
};
template <int G>
GDEV void fin_put(const Workspace& ws, uint64_t idx, const double* y, const RayConst& rc, uint32_t nrec, int stop,
                  int status) {
  double v[8];
  if constexpr (G == GRT_GEOM_KERR_BL) {
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = y[1 + k];
    v[5] = rc.obs;
    v[6] = rc.e;
    v[7] = rc.lz;
  } else {
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = y[1 + k];
    v[7] = __hiloint2double((int)((uint32_t)(stop & 0xff) | ((uint32_t)(status & 0xff) << 8)), (int)nrec);
  }
  double2* d = reinterpret_cast<double2*>(ws.fin + idx * 8);
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = make_double2(v[2 * k], v[2 * k + 1]);
}
// rc.obs: KerrBL's from the record, else 0 (the caller sets observer_energy)
template <int G>
GDEV RayMeta fin_get(const Workspace& ws, uint64_t idx, double* y, RayConst& rc) {
  const double2* d = reinterpret_cast<const double2*>(ws.fin + idx * 8);
  double v[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double2 w = d[k];
    v[2 * k] = w.x;
    v[2 * k + 1] = w.y;
  }
  y[0] = 0.0;
  rc.q = 0.0;
  rc.pt = 0.0;
  rc.pphi = 0.0;
  if constexpr (G == GRT_GEOM_KERR_BL) {
#pragma unroll
    for (int k = 0; k < 5; ++k) y[1 + k] = v[k];
    y[6] = 0.0;
    y[7] = 0.0;
    rc.obs = v[5];
    rc.e = v[6];
    rc.lz = v[7];
    const uint4 m = reinterpret_cast<const uint4*>(ws.meta)[idx];
    return RayMeta{m.y, m.x, (int)(m.z & 0xffu), (int)((m.z >> 8) & 0xffu)};
  } else {
#pragma unroll
    for (int k = 0; k < 7; ++k) y[1 + k] = v[k];
    rc.obs = 0.0;
    rc.e = 0.0;
    rc.lz = 0.0;
    const uint64_t m = (uint64_t)__double_as_longlong(v[7]);
    return RayMeta{(uint32_t)m, 0u, (int)((m >> 32) & 0xffu), (int)((m >> 40) & 0xffu)};
  }
}

// End of a ray: its record goes to the workspace for the shade kernel.
template <int G>
GDEV void store_ray(const Workspace& ws, uint64_t idx, const double* y, const RayConst& rc, int stop, int status,
                    uint32_t nrec, uint32_t steps) {
  RAY_TIME(ws.n, idx, 2, __builtin_amdgcn_s_memrealtime());
  fin_put<G>(ws, idx, y, rc, nrec, stop, status);
  if constexpr (G == GRT_GEOM_KERR_BL) {
    reinterpret_cast<uint4*>(ws.meta)[idx] =
        make_uint4(steps, nrec, (uint32_t)(stop & 0xff) | ((uint32_t)(status & 0xff) << 8), 0u);
  } else {
    if (ws.steps) ws.steps[idx] = steps;
  }
}

// Candidate nrec >= GRT_WS_SLOTS of ray idx: one record appended to the hit pool and
// linked after the ray's previous one.  Once a record does not fit, the ray's list is
// marked lost (ovf_last = HIT_NIL) and nothing more is linked; the count keeps growing so
// that the host learns the size the trace needed.
GDEV void hit_append(const Workspace& ws, uint64_t idx, uint32_t nrec, uint32_t win, uint32_t obj,
                     const double* p, const double* pt, const double* dir HIT_TIME_PARAM) {
  const HitPool& hp = *ws.pool;
  const unsigned long long pos = atomicAdd(hp.count, 1ull);
  const bool first = nrec == GRT_WS_SLOTS;
  const uint32_t prev = first ? HIT_NIL : ws.pool->last[idx];
  if (pos >= hp.cap || (!first && prev == HIT_NIL)) {
    if (first) ws.pool->head[idx] = HIT_NIL;
    ws.pool->last[idx] = HIT_NIL;
    return;
  }
  const uint64_t m = hp.cap;
  hp.win[pos] = win;
  hp.obj[pos] = (uint8_t)obj;
#pragma unroll
  for (int q = 0; q < 4; ++q) hp.p[q * m + pos] = p[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) hp.pt[q * m + pos] = pt[q];
  if (dir) {
#pragma unroll
    for (int q = 0; q < 3; ++q) hp.dir[q * m + pos] = dir[q];
  }
#if GRT_LAPSE
  hp.pool_time[pos] = th;
#endif
  if (first) ws.pool->head[idx] = (uint32_t)pos;
  else hp.next[prev] = (uint32_t)pos;
  ws.pool->last[idx] = (uint32_t)pos;
}

// The window (y -> yn) of accepted step i against every object in config order
// (objects.rs:81); a hit nearer than the current nearest (objects.rs:86-88) is recorded
// as candidate nrec: its object, window index, hit point and the lerped momentum
// (objects.rs:27-44).  `writer`: this lane stores the candidate (one lane of a quad in
// tail_kernel; every lane computes the same decisions).  c / c_valid follow yn.
template <int G, bool VOL>
GDEV void window_pass(const DevScene& S, const Workspace& ws, const RayConst& rc, uint64_t idx, const double* y,
                      const double* yn, double* c, bool& c_valid, uint64_t i, uint32_t& nrec, bool writer) {
  const uint64_t n = ws.n;
  if (!window_far<G, VOL>(S, y, yn)) {
    PATH_COUNT(4);
    if (!c_valid) to_cart<G>(S, y, c);
    double cn[3];
    to_cart<G>(S, yn, cn);
    double shortest = 1.7976931348623157e308;
    for (uint32_t k = 0; k < S.n_objects; ++k) {
      const DevObject& o = S.obj[k];
      double t, pt[3];
      bool hit;
      if (VOL && o.kind == GRT_OBJ_VOLUMETRIC_DISC) hit = vdisc_chord(o, c, cn, &t, pt);
      else hit = (o.kind == GRT_OBJ_DISC) ? disc_chord(o, c, cn, &t, pt) : sphere_chord(o, c, cn, &t, pt);
      if (!hit) continue;
      double wx = pt[0], wy = pt[1], wz = pt[2];
      if (o.kind == GRT_OBJ_SPHERE) {
        wx = pt[0] + o.cx;
        wy = pt[1] + o.cy;
        wz = pt[2] + o.cz;
      }
      double dx = wx - c[0], dy = wy - c[1], dz = wz - c[2];
      double distance = sqrt(dx * dx + dy * dy + dz * dz);
      if (!(distance < shortest)) continue;
      shortest = distance;
      double ph[4];
      if (writer) lerp_momentum<G>(S, rc, y, yn, t, ph);
#if GRT_LAPSE
      // the hit's coordinate time, lerped over the window as the momentum is
      [[maybe_unused]] double th = 0.0;
      if (writer) th = y[0] + t * (yn[0] - y[0]);
#endif
      if (writer && nrec < GRT_WS_SLOTS) {
        const uint64_t slot = (uint64_t)nrec * n + idx;
#if GRT_LAPSE
        ws.pool->slot_time[slot] = th;
#endif
        double2* d = reinterpret_cast<double2*>(ws.rec + slot);
        d[0] = make_double2(ph[0], ph[1]);
        d[1] = make_double2(ph[2], ph[3]);
        d[2] = make_double2(pt[0], pt[1]);
        d[3] = make_double2(pt[2], __hiloint2double((int)k, (int)(uint32_t)i));
        if constexpr (VOL) {  // chord direction for the raymarch (volumetric_disc.rs:576, :589-594)
          ws.rec_dir[slot] = cn[0] - c[0];
          ws.rec_dir[(uint64_t)GRT_WS_SLOTS * n + slot] = cn[1] - c[1];
          ws.rec_dir[(uint64_t)2 * GRT_WS_SLOTS * n + slot] = cn[2] - c[2];
        }
      } else if (writer) {  // beyond the workspace slots: the hit pool
        double dir[3] = {cn[0] - c[0], cn[1] - c[1], cn[2] - c[2]};
        hit_append(ws, idx, nrec, (uint32_t)i, k, ph, pt, VOL ? dir : nullptr HIT_TIME_ARG);
      }
      nrec++;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = cn[k];
    c_valid = true;
  } else {
    c_valid = false;
  }
}

// A ray's loop state at the top of integrate_kernel's loop, in entry e of the tail list.
struct LoopState {
  double y[8], c[3];
  double h, h_cur;
  uint64_t i, idx;
  uint32_t nrec;
  int retries;
  bool c_valid;
};
// Entry e of an entry arena `st` of m entries ([16][m] words: TailList::st).
GDEV void tail_save(unsigned long long* st, uint64_t m, uint64_t e, const LoopState& s) {
  unsigned long long* w = st + e;
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k * m] = (unsigned long long)__double_as_longlong(s.y[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) w[(8 + k) * m] = (unsigned long long)__double_as_longlong(s.c[k]);
  w[11 * m] = (unsigned long long)__double_as_longlong(s.h);
  w[12 * m] = (unsigned long long)__double_as_longlong(s.h_cur);
  w[13 * m] = s.i;
  w[14 * m] = s.idx;
  w[15 * m] = (unsigned long long)s.nrec | ((unsigned long long)(uint32_t)s.retries << 32) |
              ((unsigned long long)(s.c_valid ? 1 : 0) << 48);
}
GDEV void tail_load(const unsigned long long* st, uint64_t m, uint64_t e, LoopState& s) {
  const unsigned long long* w = st + e;
#pragma unroll
  for (int k = 0; k < 8; ++k) s.y[k] = __longlong_as_double((long long)w[k * m]);
#pragma unroll
  for (int k = 0; k < 3; ++k) s.c[k] = __longlong_as_double((long long)w[(8 + k) * m]);
  s.h = __longlong_as_double((long long)w[11 * m]);
  s.h_cur = __longlong_as_double((long long)w[12 * m]);
  s.i = w[13 * m];
  s.idx = w[14 * m];
  const unsigned long long f = w[15 * m];
  s.nrec = (uint32_t)f;
  s.retries = (int)((f >> 32) & 0xffffu);
  s.c_valid = ((f >> 48) & 1u) != 0;
}
GDEV unsigned long long load_agent(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Items claimed so far from the work counter (both ends of a two-ended queue).
GDEV uint64_t items_claimed(unsigned long long w, bool two_ended) {
  return two_ended ? (w & 0xffffffffull) + (w >> 32) : w;
}
// This wave's hardware slot on its SIMD (HW_REG_HW_ID bits 3:0, gfx9).
GDEV unsigned hw_wave_slot() { return __builtin_amdgcn_s_getreg(4 | (3 << 11)); }
// One lane integrates one ray at a time: RKF45 attempts, and after every accepted
// step the chord test of window (previous step, step) against every object in config
// order (objects.rs:81) and the stop test (window_pass, should_stop).
// Kerr-Schild with tl.cap != 0: once the tile queue is drained and at most tl.threshold
// rays are live, each wave hands its rays to tail_kernel (tail_save) and exits.
template <int G, bool VOL>
__global__ void __launch_bounds__(256, integrate_waves(G, VOL)) integrate_kernel(
    const DevScene* __restrict__ Sp, WorkList wl, Workspace ws, unsigned long long* __restrict__ counter,
    unsigned long long* __restrict__ stats, TailList tl CAMS_PARAM) {
  const DevScene& S = *Sp;
  // items present: the capacity, or the count the adaptive pass decided on the device
  const uint64_t n_items = wl.n_live ? (uint64_t)min((unsigned long long)wl.n_items, *wl.n_live) : wl.n_items;
  if (n_items == 0) return;  // an empty chunk of a supersample pass
#if GRT_PATH_COUNT
  if (threadIdx.x < 2 * NPATH) path_lds[threadIdx.x] = 0;  // ordered before use by the tables' barrier
#endif
  glibc::tables_to_lds();  // whole block, before any lookup
  const int lane = threadIdx.x & 63;
  const uint64_t lanemask_lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  constexpr uint64_t CHUNK = 64;
  const uint64_t n = ws.n;
  constexpr bool TAIL = (G == GRT_GEOM_KERR);
  const bool tail_on = TAIL && tl.cap != 0;
  constexpr int NKL = (((GRT_KLDS_GEOMS) >> G) & 1) ? GRT_KL_STAGES : 0;
  if (tail_on && blockIdx.x == 0 && threadIdx.x == 0) tl.ctl[3] = __builtin_amdgcn_s_memrealtime();

  // Two-ended queue (WorkList::two_ended).  The issue arbiter of a SIMD serves the oldest
  // wave first: with two Kerr-Schild waves per SIMD the older one runs an attempt in
  // ~31 us and the younger one in ~130 us while both are busy (per-ray record of a C4
  // shard, profiles/r04a).  So one wave per SIMD (even hardware slot) takes the items
  // with the longest predicted rays from the front and holds the issue priority
  // explicitly (s_setprio), and the others take the shortest items from the back.  Both
  // ends advance one packed counter, so a claim sees every earlier claim of either end:
  // with (front, back) its snapshot, rank r is item front + r or n - 1 - (back + r), and
  // exists while front + back + r < n.
  const bool two_ended = wl.two_ended != 0;
  const bool from_back = two_ended && (hw_wave_slot() & 1u);
  if (two_ended && !from_back) __builtin_amdgcn_s_setprio(1);
  uint64_t chunk_next = 0, chunk_end = 0;  // wave-uniform work cursor
  bool active = false, done = false;
  bool started = false, ended = false;  // since the last live-count update (tail_on)
  uint32_t poll = 0;
  bool q_drained = false;  // this wave has seen the tile queue drained (it stays drained)
  uint64_t idx = 0;      // output slot of the current ray
  double y[8];           // state
  double c[3];           // Cartesian position of the last accepted step (when c_valid)
  bool c_valid = false;
  double h = 0.0, h_cur = 0.0;
  uint64_t i = 0;        // accepted step index
  int retries = 0;
  uint32_t nrec = 0;
  RayConst rc;
  // per-lane counters in 32 bits (one VGPR each): a lane integrates far fewer than 2^32
  // steps in one launch (C4 whole frame: ~5e6 per lane)
  uint32_t n_acc = 0, n_att = 0;
  uint64_t w_rays = 0;  // rays started by this wave: counted in wave-uniform control flow (an SGPR)
#if GRT_RAY_TIMES
  uint32_t ray_att = 0;
#endif

  while (true) {
    // ---------------- lane refill: ballot, one atomic per claim ------------------
    bool need = !active && !done;
    uint64_t need_mask = __ballot(need);
    if (need_mask) {
      bool fresh = false;  // this lane started a ray in this refill
      uint64_t cnt = __popcll(need_mask);
      uint64_t remaining = chunk_end - chunk_next;
      uint64_t new_base = 0;
      // Claims are exact: a wave takes exactly the items it starts now.  A wave holding
      // unstarted items of a 64-item chunk when the queue drains starts them one ray
      // lifetime late, on its own lanes, while other waves have emptied (C5's supersample
      // pass, ~2.5 sub-rays per lane: its last ray started at 0.375 s of a 0.47 s pass with
      // chunks, at 0.21 s of 0.39 s with exact claims; C2 -2.5%; profiles/r05d, r05e).
      // KerrBL claims 64-item chunks until its view of the counter is within two grids'
      // worth of lanes of the end: its 2.25M short rays end ~13M times a second, and an
      // atomic on one address per refill cost C3 +16% (profiles/r05l, r05m).
      const uint64_t grid_lanes = (uint64_t)gridDim.x * blockDim.x;
      const bool exact = TAIL || two_ended || G != GRT_GEOM_KERR_BL || chunk_end + 2 * grid_lanes >= n_items;
      const uint64_t take = exact ? cnt - remaining : CHUNK;
      if (cnt > remaining) {
        unsigned long long b = 0;
        if (lane == 0) b = atomicAdd(counter, from_back ? (unsigned long long)take << 32 : (unsigned long long)take);
        new_base = __shfl(b, 0);
      }
      if (need) {
        uint64_t rank = __popcll(need_mask & lanemask_lt);
        uint64_t item = rank < remaining ? chunk_next + rank : new_base + (rank - remaining);
        if (two_ended) {  // new_base is the counter's snapshot (front | back << 32)
          const uint64_t f = new_base & 0xffffffffull, bk = new_base >> 32;
          item = (f + bk + rank >= n_items) ? n_items : (from_back ? n_items - 1 - (bk + rank) : f + rank);
        }
        if (item >= n_items) {
          if (TAIL && tail_on && !done && tl.ctl[4] == 0ull)
            atomicCAS(&tl.ctl[4], 0ull, (unsigned long long)__builtin_amdgcn_s_memrealtime());
          done = true;
        } else {
          double row, col;
          bool valid = true;
          [[maybe_unused]] const DevCamera* cam;  // this lane's camera: in the sequence unit the frame of its ray (a per-lane load)
          if (wl.pixel_index) {  // offset list (get_ray_for_offset, camera.rs:247-254)
            idx = item;
            cam = &ray_pixel(S, wl, idx, &row, &col CAMS_ARG);
          } else {  // 8x8 pixel tiles, row-major tiles: a wave starts on a compact patch
            uint64_t tile = item >> 6;
            if (wl.tile_order) tile = wl.tile_order[tile];  // longest-predicted tiles first
            uint32_t w = (uint32_t)(item & 63);
            uint32_t tr = (uint32_t)(tile / wl.tiles_x), tc = (uint32_t)(tile % wl.tiles_x);
            uint32_t r = tr * 8 + (w >> 3), cc = tc * 8 + (w & 7);
            valid = (r < wl.rows) && (cc < wl.cols);
            // rect_pixel(r, cc), written out: through the call, KerrBL's volumetric kernel changes its
            // code in one unit or another
#if GRT_SEQ
            uint32_t ri = wl.row0 + shard_frame_row(wl.band_rows, wl.shard, wl.n_shards, r);
            cam = &frame_camera(S, &ri CAMS_ARG);
            row = (double)ri;
#else
            row = (double)(wl.row0 + shard_frame_row(wl.band_rows, wl.shard, wl.n_shards, r));
#endif
            col = (double)(wl.col0 + cc);
            idx = (uint64_t)r * wl.cols + cc;
          }
          if (valid) {
            init_ray<G, VOL>(S, row, col, y, rc CAM_ARG(*cam));
            if constexpr (VOL) {  // the raymarch's frequency data (march_kernel)
              ws.rc[0 * n + idx] = rc.obs;
              ws.rc[1 * n + idx] = rc.e;
              ws.rc[2 * n + idx] = rc.lz;
              ws.rc[3 * n + idx] = rc.q;
              ws.rc[4 * n + idx] = rc.pt;
              ws.rc[5 * n + idx] = rc.pphi;
            }
            c_valid = false;
            h = S.step_size;
            h_cur = rclamp(h, H_MIN, H_MAX);
            i = 0;
            retries = 0;
            nrec = 0;
            active = true;
            started = true;
            fresh = true;
#if GRT_RAY_TIMES
            ray_att = 0;
            RAY_TIME(n, idx, 0, __builtin_amdgcn_s_memrealtime());
            RAY_TIME(n, idx, 3, hw_place());
#endif
            if (S.max_steps <= 1) {  // `for i in 1..max_steps` never runs
              store_ray<G>(ws, idx, y, rc, GRT_STOP_NONE, GRT_OK, 0, 0);
              active = false;
              ended = true;
            }
          }
        }
      }
      w_rays += __popcll(__ballot(fresh));
#if GRT_TAIL_PRIO
      // KerrBL's rays are all short: measured no gain there
      if constexpr (!TAIL && G != GRT_GEOM_KERR_BL) {
        // After the queue has drained for this wave (one of its lanes found no item), the
        // pass ends on the rays with the most steps left, so the waves holding them get the
        // SIMD's issue slots first (s_setprio; the arbiter otherwise serves the oldest wave):
        // the estimate of what is left is max_radius unit steps (a ray escapes after about
        // that many) minus the wave's fewest accepted steps.  Scheduling only, never results.
        if (!two_ended && __ballot(done) != 0) {
          uint32_t mi = active ? (uint32_t)i : 0xffffffffu;
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) mi = min(mi, (uint32_t)__shfl_xor((int)mi, off));
          const double len = sqrt(S.max_radius_sq);
          const double left = len - (double)mi;
          if (left > 0.67 * len) __builtin_amdgcn_s_setprio(3);
          else if (left > 0.33 * len) __builtin_amdgcn_s_setprio(2);
          else __builtin_amdgcn_s_setprio(1);
        }
      }
#endif
      if (cnt > remaining) {
        chunk_next = new_base + (cnt - remaining);
        chunk_end = new_base + take;
      } else {
        chunk_next += cnt;
      }
    }
    if constexpr (TAIL) {
      if (tail_on) {
        // live-ray count: one atomic per wave when rays started or ended
        const uint64_t st_mask = __ballot(started), en_mask = __ballot(ended);
        started = ended = false;
        const long long d = (long long)__popcll(st_mask) - (long long)__popcll(en_mask);
        if (d != 0 && lane == 0) atomicAdd(&tl.ctl[0], (unsigned long long)d);
        // hand-off: queue drained (and nothing left in this wave's chunk), few rays left.
        // Kerr-Schild claims exactly what it starts, so its chunk is always used up: the
        // drained test (an agent-scope load, served beyond this XCD's L2) runs every 256
        // attempts until the wave has seen the queue drained, then the live count every 16
        if ((chunk_next >= chunk_end || chunk_next >= n_items) && ((++poll & (q_drained ? 15u : 255u)) == 0u) &&
            (q_drained || (q_drained = items_claimed(load_agent(counter), two_ended) >= n_items)) &&
            (long long)load_agent(&tl.ctl[0]) <= (long long)tl.threshold) {
          const uint64_t ev = __ballot(active);
          if (ev) {
            unsigned long long b = 0;
            if (lane == 0) {
              b = atomicAdd(&tl.ctl[1], (unsigned long long)__popcll(ev));
              if (b == 0) tl.ctl[5] = __builtin_amdgcn_s_memrealtime();
            }
            b = __shfl(b, 0);
            if (active) {
              const uint64_t e = b + __popcll(ev & lanemask_lt);
              if (e < tl.cap) {
                LoopState s;
#pragma unroll
                for (int k = 0; k < 8; ++k) s.y[k] = y[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) s.c[k] = c[k];
                s.h = h;
                s.h_cur = h_cur;
                s.i = i;
                s.idx = idx;
                s.nrec = nrec;
                s.retries = retries;
                s.c_valid = c_valid;
                tail_save(tl.st, tl.cap, e, s);
                RAY_TIME(n, idx, 1, __builtin_amdgcn_s_memrealtime());
                RAY_TIME(n, idx, 4, ray_att);
                active = false;
                done = true;
              }
            }
          }
        }
      }
    }
    if (__ballot(!done) == 0) break;
    if (!active) continue;

    // ---------------- one RKF45 attempt (runge_kutta.rs:148-178) ----------------
    double yn[8];
    double err_sq = 0.0;
    // Kerr-Schild: the RHS dwarfs the saved products, and a second copy of its attempt
    // (+80 KB of code) is not worth them
    constexpr bool UNIT_H_COPY = GRT_UNIT_H && G != GRT_GEOM_KERR;
    constexpr bool QUICK = GRT_QUICK_STEP && G == GRT_GEOM_SCHWARZSCHILD && !VOL;
    // Schwarzschild: the attempt without its zero-weight k2 terms (rkf_attempt_fold's lemma)
    constexpr bool SHORT = GRT_RKF_SHORT && GRT_RK_FOLD && G == GRT_GEOM_SCHWARZSCHILD;
    // grt_debug_rkf_short: 0 every attempt in the full form; 2 the short attempt, then on the
    // general path always the full one after it, as if a lane had missed rkf_short_ok (tests)
    bool full = false, again = false;
    if constexpr (SHORT) {
      full = S.rkf_short == 0;
      again = S.rkf_short == 2;
    }
    // The steady loop: the general iteration takes the attempt without
    // UNIT_H (h * o with h == 1 is o), and a wave whose quick step leaves every lane at
    // h_cur == 1.0 stays in a loop of unit attempts and reduced tests (steady_step_mask) until a
    // lane misses the test; then it goes on below with yn and err_sq of that attempt, as it
    // does from the quick step.  Two copies of the attempt, as before.
    constexpr bool STEADY = GRT_STEADY_LOOP && QUICK && UNIT_H_COPY && SHORT;
    while (!full) {
      if constexpr (STEADY) {
        err_sq = rkf_attempt<G, false, false, NKL, SHORT>(S, rc, y, h_cur, yn);
      } else {
        err_sq = (UNIT_H_COPY && __ballot(active && h_cur != 1.0) == 0)
                     ? rkf_attempt<G, UNIT_H_COPY, false, NKL, SHORT>(S, rc, y, h_cur, yn)
                     : rkf_attempt<G, false, false, NKL, SHORT>(S, rc, y, h_cur, yn);
      }
      n_att++;
      PATH_COUNT(6);
#if GRT_RAY_TIMES
      ray_att++;
#endif
      if constexpr (QUICK) {
        // every lane of the wave on the commonest accepted step (quick_step_ok): the
        // general path's updates in one straight-line block, then straight on to the next
        // attempt (no ray ended, so no lane needs a refill)
        const bool q_ok = quick_step_ok<G, SHORT>(S, err_sq, y, yn, i + 1);
        if (GRT_SCALAR_VOTES ? wave_all(q_ok) : __ballot(!q_ok) == 0) {
          h = rclamp(h_cur * H_GROWTH, H_MIN, H_MAX);
          i++;
          n_acc++;
          c_valid = false;
#pragma unroll
          for (int k = 0; k < 8; ++k) y[k] = yn[k];
          retries = 0;
          h_cur = rclamp(h, H_MIN, H_MAX);
          if constexpr (STEADY) {
            // h_cur == 1.0 on every lane: each step of the loop would set h = clamp(4 * 1.0) =
            // 1.0 and h_cur = 1.0 again, so both stay as they are, with retries and c_valid
            if (steady_scene_ok(S) && wave_all(h_cur == 1.0)) {
              const SteadyScene q = steady_scene(S);
              while (true) {
                err_sq = rkf_attempt<G, true, false, NKL, SHORT>(S, rc, y, 1.0, yn);
                n_att++;
                PATH_COUNT(6);
#if GRT_RAY_TIMES
                ray_att++;
#endif
                if (steady_step_mask<G>(q, err_sq, y, yn, i + 1) != __ballot(true)) break;
                i++;
                n_acc++;
#pragma unroll
                for (int k = 0; k < 8; ++k) y[k] = yn[k];
              }
              break;
            }
          }
          continue;
        }
      }
      break;
    }
    if constexpr (SHORT) {
      // The quick step tested the lemma's premise itself (quick_step_ok); on this, the
      // general path, the wave tests it here and, if a lane misses it, takes the attempt
      // again in the full form: a ray with a persistent -0 component (v_phi = -0 in a
      // meridional plane) or one going non-finite; lanes that met the premise get their bits
      // again.  One copy, without UNIT_H (h * o with h == 1 is o), inlined: out of line it
      // cost the kernel 464 B of scratch per lane for the call's saves, against 112 B.
      if (full || again || (GRT_SCALAR_VOTES ? !wave_all(rkf_short_ok(err_sq, yn)) : __ballot(!rkf_short_ok(err_sq, yn)) != 0)) {
        PATH_COUNT(7);
        err_sq = rkf_attempt<G, false, false, NKL>(S, rc, y, h_cur, yn);
        if (full) {
          n_att++;
          PATH_COUNT(6);
#if GRT_RAY_TIMES
          ray_att++;
#endif
        }
      }
    }
    double h_next;
    const int ctl = step_control(S, err_sq, h_cur, retries, h_next);
    if (ctl != STEP_ACCEPTED) {
      if (ctl == STEP_FAILED) {  // Err(MaxStepsReached)
        store_ray<G>(ws, idx, y, rc, GRT_STOP_NONE, GRT_ERR_MAX_STEPS_REACHED, 0, (uint32_t)i);
        RAY_TIME(n, idx, 4, ray_att);
        active = false;
        ended = true;
      }
      continue;
    }

    // ---------------- accepted step i (integrator.rs:100-162) --------------------
    PATH_COUNT(5);
    h = h_next;
    i++;
    n_acc++;
    window_pass<G, VOL>(S, ws, rc, idx, y, yn, c, c_valid, i, nrec, true);
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = yn[k];

    int stop = should_stop<G>(S, y, c, c_valid, i);
    if (stop != GRT_STOP_NONE || i == S.max_steps - 1) {
      store_ray<G>(ws, idx, y, rc, stop, GRT_OK, nrec, (uint32_t)i);
      RAY_TIME(n, idx, 4, ray_att);
      active = false;
      ended = true;
      continue;
    }
    retries = 0;
    h_cur = rclamp(h, H_MIN, H_MAX);
  }

  // per-wave reduction of the counters, one atomic per wave
  uint64_t w_acc = n_acc, w_att = n_att;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    w_acc += __shfl_down(w_acc, off);
    w_att += __shfl_down(w_att, off);
  }
  if (lane == 0) {
    atomicAdd(stats + 0, (unsigned long long)w_acc);
    atomicAdd(stats + 1, (unsigned long long)w_att);
    atomicAdd(stats + 2, (unsigned long long)w_rays);
  }
#if GRT_PATH_COUNT
  __syncthreads();  // every wave of the block has left its loop
  if (threadIdx.x < 2 * NPATH) atomicAdd(&g_path[threadIdx.x], path_lds[threadIdx.x]);
#endif
}

// ============================================================= tail kernel =======
// One attempt of a handed-off ray on the 4 lanes of its quad: the loop body of
// integrate_kernel with the RHS split over the quad (rhs_ks_quad); lane 0 of the quad
// writes.  Returns true when the ray has ended (its outputs are stored).
template <int G, bool VOL>
GDEV bool quad_attempt(const DevScene& S, const Workspace& ws, const RayConst& rc, LoopState& s, int sub,
                       bool writer, uint64_t& n_acc, uint64_t& n_att) {
  double yn[8];
  const double err_sq = rkf_attempt<G, false, true>(S, rc, s.y, s.h_cur, yn, sub);
  n_att++;
  double h_next;
  const int ctl = step_control(S, err_sq, s.h_cur, s.retries, h_next);
  if (ctl != STEP_ACCEPTED) {
    if (ctl == STEP_FAILED) {  // Err(MaxStepsReached)
      if (writer) store_ray<G>(ws, s.idx, s.y, rc, GRT_STOP_NONE, GRT_ERR_MAX_STEPS_REACHED, 0, (uint32_t)s.i);
      return true;
    }
    return false;
  }
  s.h = h_next;
  s.i++;
  n_acc++;
  window_pass<G, VOL>(S, ws, rc, s.idx, s.y, yn, s.c, s.c_valid, s.i, s.nrec, writer);
#pragma unroll
  for (int k = 0; k < 8; ++k) s.y[k] = yn[k];
  const int stop = should_stop<G>(S, s.y, s.c, s.c_valid, s.i);
  if (stop != GRT_STOP_NONE || s.i == S.max_steps - 1) {
    if (writer) store_ray<G>(ws, s.idx, s.y, rc, stop, GRT_OK, s.nrec, (uint32_t)s.i);
    return true;
  }
  s.retries = 0;
  s.h_cur = rclamp(s.h, H_MIN, H_MAX);
  return false;
}

// The rays integrate_kernel handed off (Kerr-Schild): the 4 lanes of a quad carry one
// ray, splitting each RHS evaluation (rhs_ks_quad), and repeat the rest of the loop of
// integrate_kernel in lockstep (identical values in all four lanes; lane 0 of the quad
// writes).  A quad claims the next handed-off ray when its ray ends.  With one wave per
// SIMD a long ray no longer shares issue slots with another wave.
template <int G, bool VOL>
__global__ void __launch_bounds__(256, GRT_TAIL_WAVES) tail_kernel(const DevScene* __restrict__ Sp, Workspace ws,
                                                                   TailList tl,
                                                                   unsigned long long* __restrict__ stats) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before any lookup
  const int lane = threadIdx.x & 63;
  const int sub = lane & 3;
  const bool writer = sub == 0;
  const uint64_t below_quad = (lane < 4) ? 0ull : (~0ull >> (64 - (lane & ~3)));
  const uint64_t n = ws.n;
  const unsigned long long handed = load_agent(&tl.ctl[1]);
  const uint64_t n_tail = handed < tl.cap ? handed : tl.cap;  // final: integrate_kernel has ended

  bool active = false, done = false;
  LoopState s;
  RayConst rc;
  uint64_t n_acc = 0, n_att = 0;
#if GRT_RAY_TIMES
  uint64_t att0 = 0;
#endif

  while (true) {
    const bool need = !active && !done;  // uniform within a quad
    const uint64_t leaders = __ballot(need && writer);
    if (leaders) {
      unsigned long long b = 0;
      if (lane == 0) b = atomicAdd(&tl.ctl[2], (unsigned long long)__popcll(leaders));
      b = __shfl(b, 0);
      if (need) {
        const uint64_t e = b + __popcll(leaders & below_quad);
        if (e >= n_tail) {
          done = true;
        } else {
          tail_load(tl.st, tl.cap, e, s);
          rc.obs = 0.0;  // Kerr-Schild: the RHS, the momentum and fin_put read no ray constant
          rc.e = 0.0;
          rc.lz = 0.0;
          rc.q = 0.0;
          rc.pt = VOL ? ws.rc[4 * n + s.idx] : 0.0;
          rc.pphi = VOL ? ws.rc[5 * n + s.idx] : 0.0;
          active = true;
#if GRT_RAY_TIMES
          att0 = n_att;
#endif
        }
      }
    }
    if (__ballot(!done) == 0) break;
    if (!active) continue;
    if (quad_attempt<G, VOL>(S, ws, rc, s, sub, writer, n_acc, n_att)) {
      active = false;
#if GRT_RAY_TIMES
      if (writer) RAY_TIME(n, s.idx, 5, n_att - att0);
#endif
    }
  }

  if (lane == 0) atomicMax(&tl.ctl[6], (unsigned long long)__builtin_amdgcn_s_memrealtime());
  if (!writer) n_acc = n_att = 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_acc += __shfl_down(n_acc, off);
    n_att += __shfl_down(n_att, off);
  }
  if (lane == 0) {
    atomicAdd(stats + 0, (unsigned long long)n_acc);
    atomicAdd(stats + 1, (unsigned long long)n_att);
  }
}

#if GRT_MAIN_TU  // trajectories, monitors and test hooks: exact build only
// Device check of div_inrange / div2_inrange / div_fx / sqrt_fx against the compiler's
// division and sqrt over the whole exponent plane (tests/test_gpu_parity.py
// ::test_range_free_arithmetic_map): thread (ex, ey), ex, ey biased exponents 0 .. 2046
// (0: subnormals), runs `samples` operand pairs x = +-m_x 2^(ex-1023), y = +-m_y 2^(ey-1023)
// -- the first four with extreme mantissas (0 / all ones), the rest splitmix64-random, and
// a second numerator x2 of the same exponent for div2_inrange -- and sets in map[ex][ey]:
//   1 div_inrange(x, y) != x / y      2 div2_inrange(x, x2, y) != (x / y, x2 / y)
//   4 div_fx(x, y) != x / y
// Threads with ex == 0 also set zmap[ey] |= 8 when div_fx(+-0, y) != +-0 / y, and threads
// with ey == 0 set smap[ex] |= 16 when sqrt_fx(x) != sqrt(x) for positive x of exponent ex.
__global__ void arith_map_kernel(uint32_t samples, uint64_t seed, uint8_t* map, uint8_t* zmap, uint8_t* smap) {
  const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= 2047u * 2047u) return;
  const uint32_t ex = cell / 2047u, ey = cell % 2047u;
  auto mix = [](uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  };
  constexpr uint64_t MANT = 0x000fffffffffffffull;
  auto bits = [](double v) { return (uint64_t)__double_as_longlong(v); };
  auto make = [](uint64_t sign, uint64_t e, uint64_t m) {
    return __longlong_as_double((long long)((sign << 63) | (e << 52) | m));
  };
  uint32_t flags = 0, zflags = 0, sflags = 0;
  for (uint32_t k = 0; k < samples; ++k) {
    const uint64_t u = mix(seed ^ ((uint64_t)cell * 64 + 3 * k + 1)), v = mix(seed ^ ((uint64_t)cell * 64 + 3 * k + 2)),
                   w = mix(seed ^ ((uint64_t)cell * 64 + 3 * k + 3));
    const uint64_t mx = k < 4 ? ((k & 1) ? MANT : 0) : (u & MANT);
    const uint64_t my = k < 4 ? ((k & 2) ? MANT : 0) : (v & MANT);
    const double x = make(u >> 63, ex, mx), y = make(v >> 63, ey, my), x2 = make(w >> 63, ex, w & MANT);
    volatile double vx = x, vy = y, vx2 = x2;  // keep the reference divisions as divisions
    const double ref1 = vx / vy, ref2 = vx2 / vy;
    double q1, q2;
    div2_inrange(x, x2, y, &q1, &q2);
    if (bits(div_inrange(x, y)) != bits(ref1)) flags |= 1u;
    if (bits(q1) != bits(ref1) || bits(q2) != bits(ref2)) flags |= 2u;
    if (bits(div_fx(x, y)) != bits(ref1)) flags |= 4u;
    if (ex == 0) {
      const double z0 = (u >> 62) & 1 ? -0.0 : 0.0;
      volatile double vz = z0;
      if (bits(div_fx(z0, y)) != bits(vz / vy)) zflags |= 8u;
    }
    if (ey == 0) {
      const double sx = fabs(x);
      volatile double vsx = sx;
      if (bits(sqrt_fx(sx)) != bits(sqrt(vsx))) sflags |= 16u;
    }
  }
  map[cell] = (uint8_t)flags;
  if (ex == 0) zmap[ey] = (uint8_t)zflags;
  if (ey == 0) smap[ex] = (uint8_t)sflags;
}

// Device check of the seeded reciprocals of the region-B Schwarzschild RHS (rcp_seed.h)
// against the compiler's division (tests/test_gpu_rcp_seed.py): tuple i = (r, radius, a,
// sin, cos) in t[5 i ..]; flags[i] gets bit
//   1 radius / r   2 2 / r   4 radius / (r r)   8 (radius / (r r)) / a   16 (2 cos) / sin
// for each quotient whose bits differ.  a comes from the tuple, not from r, so that the
// test can put it on the predicate's edge.
__global__ void rcp_seed_check_kernel(uint64_t n, const double* __restrict__ t, uint8_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double r = t[5 * i], radius = t[5 * i + 1], a = t[5 * i + 2], st = t[5 * i + 3], ct = t[5 * i + 4];
  auto bits = [](double v) { return (uint64_t)__double_as_longlong(v); };
  auto hw_rcp = [](double v) { return __builtin_amdgcn_rcp(v); };
  const double rr = r * r, two_ct = 2.0 * ct;
  double Yr, Yrr, Ya, Yst;
  rcpseed::rcp_r_rr(r, rr, hw_rcp, &Yr, &Yrr);
  rcpseed::rcp_pair(a, st, hw_rcp, &Ya, &Yst);
  const double a_prime = rcpseed::div_by_rcp(radius, rr, Yrr);
  volatile double v_r = r, v_radius = radius, v_a = a, v_st = st, v_rr = rr, v_two = 2.0, v_two_ct = two_ct,
                  v_a_prime = a_prime;  // keep the reference divisions as divisions
  uint32_t f = 0;
  if (bits(rcpseed::div_by_rcp(radius, r, Yr)) != bits(v_radius / v_r)) f |= 1u;
  if (bits(rcpseed::div_by_rcp(2.0, r, Yr)) != bits(v_two / v_r)) f |= 2u;
  if (bits(a_prime) != bits(v_radius / v_rr)) f |= 4u;
  if (bits(rcpseed::div_by_rcp(a_prime, a, Ya)) != bits(v_a_prime / v_a)) f |= 8u;
  if (bits(rcpseed::div_by_rcp(two_ct, st, Yst)) != bits(v_two_ct / v_st)) f |= 16u;
  flags[i] = (uint8_t)f;
}

// ======================================================= trajectory kernel =======
// Integrator::integrate with the whole Vec<Step> kept (integrator.rs:78-174), the path
// of `render-ray` / `render-ray-at` (main.rs:117-171, ray.rs:35-54).  One lane per ray;
// step 0 is the initial state.  Each record is (t, x^0..x^3, p^0..p^3): the affine
// parameter, the native-chart position and momentum_from_state.  Steps beyond the
// caller's capacity are counted but not stored.
template <int G>
__global__ void __launch_bounds__(64) trajectory_kernel(const DevScene* __restrict__ Sp, TrajectoryList tl) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= tl.n) return;
  double y[8];
  RayConst rc;
  if (tl.row) {
    init_ray<G>(S, tl.row[r], tl.col[r], y, rc);
  } else {
    double st = 0.0, ct = 0.0;
    if constexpr (G == GRT_GEOM_KERR_BL) rsincos(tl.pos[4 * r + 2], &st, &ct);
    init_state<G>(S, tl.pos + 4 * r, st, ct, tl.mom + 4 * r, y, rc);
  }
  uint64_t count = 0;
  auto record = [&](double t) {
    if (count < tl.cap) {
      double* o = tl.steps + (r * tl.cap + count) * 9;
      o[0] = t;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[1 + k] = y[k];
      momentum<G>(S, rc, y, o + 5);
    }
    count++;
  };
  record(0.0);
  int stop = GRT_STOP_NONE, status = GRT_OK;
  double t = 0.0, h = S.step_size;
  for (uint64_t i = 1; i < S.max_steps; ++i) {
    double h_cur = rclamp(h, H_MIN, H_MAX), h_next = 0.0, yn[8];
    int retries = 0, ctl;
    do {
      const double err_sq = rkf_attempt<G>(S, rc, y, h_cur, yn);
      ctl = step_control(S, err_sq, h_cur, retries, h_next);
    } while (ctl == STEP_RETRY);
    if (ctl == STEP_FAILED) {
      status = GRT_ERR_MAX_STEPS_REACHED;
      break;
    }
    t += h_cur;
    h = h_next;
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = yn[k];
    record(t);
    double c[3];
    bool c_valid = false;
    stop = should_stop<G>(S, y, c, c_valid, i);
    if (stop != GRT_STOP_NONE) break;
  }
  tl.n_steps[r] = count;
  tl.stop[r] = (uint8_t)stop;
  tl.status[r] = (uint8_t)status;
}

hipError_t launch_arith_map(uint32_t samples, uint64_t seed, uint8_t* d_map, uint8_t* d_zmap, uint8_t* d_smap,
                            hipStream_t stream) {
  hipLaunchKernelGGL(arith_map_kernel, dim3((2047u * 2047u + 255u) / 256u), dim3(256), 0, stream, samples, seed, d_map,
                     d_zmap, d_smap);
  return hipGetLastError();
}

hipError_t launch_rcp_seed_check(uint64_t n, const double* d_tuples, uint8_t* d_flags, hipStream_t stream) {
  hipLaunchKernelGGL(rcp_seed_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, d_tuples, d_flags);
  return hipGetLastError();
}

// Device check of the glibc restatement (glibc_math.h) as this unit compiles and runs it
// (tests/test_gpu_glibc_math.py): the tables staged in LDS as the trace kernels stage them,
// then the wrappers the render calls -- rpow, rsin, rcos, rsincos, vdisc_density's sincos
// line, glibc::exp_ and the region-B straight-line pair -- on x[i] (pow: x[i], y[i]).  fn,
// out0 / out1 / path: glibc_check.h.  Blocks of 64, 128, 192 or 256 threads.
__global__ void __launch_bounds__(256) glibc_check_kernel(int fn, uint64_t n, const double* __restrict__ x,
                                                          const double* __restrict__ y, double* __restrict__ out0,
                                                          double* __restrict__ out1, uint8_t* __restrict__ path) {
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double xi = x[i];
  double o0 = 0.0, o1 = 0.0, t0, t1;
  uint32_t p = 0;
  switch (fn) {
    case GLIBC_FN_POW: {
      const double yi = y[i];
      o0 = rpow(xi, yi);
      p = glibc::pow_fast(xi, yi, &t0) ? 1u : 0u;
      break;
    }
    case GLIBC_FN_SIN:
      o0 = rsin(xi);
      p = glibc::sin_fast(xi, &t0) ? 1u : 0u;
      break;
    case GLIBC_FN_COS:
      o0 = rcos(xi);
      p = glibc::cos_fast(xi, &t0) ? 1u : 0u;
      break;
    case GLIBC_FN_SINCOS:
      rsincos(xi, &o0, &o1);
      p = glibc::sincos_fast(xi, &t0, &t1) ? 1u : 0u;
      break;
    case GLIBC_FN_VDISC_SINCOS:  // vdisc_density's line, restated (volumetric.h)
      if (!glibc::sincos_fast_uniform(xi, &o0, &o1)) sincos(xi, &o0, &o1);
      p = glibc::sincos_fast_uniform(xi, &t0, &t1) ? 1u : 0u;
      break;
    case GLIBC_FN_EXP:
      o0 = glibc::exp_(xi);
      p = 1u;
      break;
    case GLIBC_FN_SINCOS_B:
      if (glibc::sincos_b_table_ok(xi)) {
        glibc::sincos_b_table(xi, &o0, &o1);
        p = 1u;
      } else if (glibc::sincos_b_taylor_ok(xi)) {
        glibc::sincos_b_taylor(xi, &o0, &o1);
        p = 2u;
      }
      break;
    default: break;
  }
  out0[i] = o0;
  out1[i] = o1;
  path[i] = (uint8_t)p;
}

hipError_t launch_glibc_check(int fn, int threads, uint64_t n, const double* d_x, const double* d_y, double* d_out0,
                              double* d_out1, uint8_t* d_path, hipStream_t stream) {
  hipLaunchKernelGGL(glibc_check_kernel, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, stream, fn, n,
                     d_x, d_y, d_out0, d_out1, d_path);
  return hipGetLastError();
}

// Device check of the range-free RHS forms (tests/test_gpu_parity.py
// ::test_rhs_fast_forms_match_ieee): for state i (y[8]; KerrBL: e, l_z, q in consts[3 i ..])
// out[16 i ..] = the range-free form (rhs MODE 1), out[16 i + 8 ..] = the IEEE form (MODE 2),
// pred[i] = whether the render's predicate admits the range-free form there.
template <int G>
__global__ void __launch_bounds__(64) rhs_check_kernel(const DevScene* __restrict__ Sp, const double* __restrict__ states,
                                                      const double* __restrict__ consts, uint64_t n, double* out,
                                                      uint8_t* pred) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double y[8], of[8], oi[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) y[k] = states[8 * i + k];
  RayConst rc{};
  if constexpr (G == GRT_GEOM_KERR_BL) {
    rc.e = consts[3 * i];
    rc.lz = consts[3 * i + 1];
    rc.q = consts[3 * i + 2];
  }
  rhs<G, 1>(S, rc, y, of);
  rhs<G, 2>(S, rc, y, oi);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out[16 * i + k] = of[k];
    out[16 * i + 8 + k] = oi[k];
  }
  bool p = false;
  const bool region_b = glibc::sincos_b_table_ok(y[2]) || glibc::sincos_b_taylor_ok(y[2]);
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD) p = S.div_share && region_b && schw_div_ok(S, y[1]);
  if constexpr (G == GRT_GEOM_KERR_BL) p = region_b && bl_div_ok(S, y[1], bl_delta(y[1], S.radius, S.a), rc.lz);
  if constexpr (G == GRT_GEOM_KERR) p = S.div_fast && ks_fd_ok(S.a, y[1], y[2], y[3], S.ks_cap);
  pred[i] = p ? 1 : 0;
}

hipError_t launch_rhs_check(int geometry, const DevScene* d_scene, const double* d_states, const double* d_consts,
                            uint64_t n, double* d_out, uint8_t* d_pred, hipStream_t stream) {
  const unsigned blocks = (unsigned)((n + 63) / 64);
  return with_chart<RHS_CHECK_CHARTS>(geometry, [&](auto g) {
    hipLaunchKernelGGL(rhs_check_kernel<decltype(g)::value>, dim3(blocks), dim3(64), 0, stream, d_scene, d_states,
                       d_consts, n, d_out, d_pred);
    return hipGetLastError();
  });
}

// Device check of the short RKF sums (tests/test_gpu_rkf_short.py): one Schwarzschild attempt
// from state i (y[8]) at step h[i] in both forms, out_short[9 i ..] and out_full[9 i ..] =
// yn[8], err_sq; guard[i] = rkf_short_ok of the short result (rkf_attempt_fold's lemma).
__global__ void __launch_bounds__(64) rkf_check_kernel(const DevScene* __restrict__ Sp, const double* __restrict__ states,
                                                      const double* __restrict__ hs, uint64_t n, double* out_short,
                                                      double* out_full, uint8_t* guard) {
  constexpr int G = GRT_GEOM_SCHWARZSCHILD;
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double y[8], ys[8], yf[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) y[k] = states[8 * i + k];
  const double h = hs[i];
  const RayConst rc{};
  const double es = rkf_attempt<G, false, false, 0, GRT_RKF_SHORT && GRT_RK_FOLD>(S, rc, y, h, ys);
  const double ef = rkf_attempt<G>(S, rc, y, h, yf);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out_short[9 * i + k] = ys[k];
    out_full[9 * i + k] = yf[k];
  }
  out_short[9 * i + 8] = es;
  out_full[9 * i + 8] = ef;
  guard[i] = rkf_short_ok(es, ys) ? 1 : 0;
}

hipError_t launch_rkf_check(const DevScene* d_scene, const double* d_states, const double* d_h, uint64_t n,
                            double* d_short, double* d_full, uint8_t* d_guard, hipStream_t stream) {
  hipLaunchKernelGGL(rkf_check_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_scene, d_states, d_h, n,
                     d_short, d_full, d_guard);
  return hipGetLastError();
}

// Device check of the VolumetricDisc arithmetic (tests/test_gpu_volumetric_checks.py): one
// lane per input, object `obj` of the scene, the production functions of volumetric.h
// unchanged, the permutation tables and gradient rows staged as march_kernel stages them.
// Input i is in[6 i ..], its results out[8 i ..] and flag[i]; per request (VdiscCheckFn):
//   PERLIN   (x, y, z)      out[0] = perlin3
//   DENSITY  p              out[0] = density, out[1..4] = PlaneAngle x, y, sp, cp, out[5] = phi
//                           (atan2 of the returned y, x: vdisc_density's own line), flag = noise
//   CHORD    from, to       flag = hit, out[0] = t, out[1..3] = the point
//   EXIT     ro, rd         flag = found, out[0] = the distance
//   NO_MORE  p, rd          flag = vdisc_no_more_density
__global__ void __launch_bounds__(256) vdisc_points_kernel(const DevScene* __restrict__ Sp, uint32_t obj, int fn,
                                                           uint64_t n, const double* __restrict__ in,
                                                           double* __restrict__ out, uint8_t* __restrict__ flag) {
  const DevScene& S = *Sp;
  __shared__ uint8_t lds_perm[GRT_MAX_OBJECTS * 256];
  __shared__ double lds_grad[16 * 4];
  if (threadIdx.x < 64) lds_grad[threadIdx.x] = (threadIdx.x & 3u) == 3u ? 0.0 : grad_coef(threadIdx.x >> 2, threadIdx.x & 3u);
  for (unsigned i = threadIdx.x; i < GRT_MAX_OBJECTS * 256u; i += blockDim.x) lds_perm[i] = S.perm[i >> 8][i & 255u];
  glibc::tables_to_lds();  // whole block, before the early return; includes the block barrier
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevObject& o = S.obj[obj];
  const uint8_t* P = lds_perm + o.perm_slot * 256u;
  const double* q = in + 6 * i;
  const V3 a{q[0], q[1], q[2]}, b{q[3], q[4], q[5]};
  double r[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool f = false;
  switch (fn) {
    case VDISC_FN_PERLIN: r[0] = perlin3(P, lds_grad, a.x, a.y, a.z); break;
    case VDISC_FN_DENSITY: {
      PlaneAngle pa{0.0, 0.0, 0.0, 0.0};
      r[0] = vdisc_density(o, P, lds_grad, a, &pa, &f);
      if (f) {
        r[1] = pa.x;
        r[2] = pa.y;
        r[3] = pa.sp;
        r[4] = pa.cp;
        r[5] = atan2(pa.y, pa.x);
      }
      break;
    }
    case VDISC_FN_CHORD: f = vdisc_chord(o, q, q + 3, &r[0], &r[1]); break;
    case VDISC_FN_EXIT: f = vdisc_exit_distance(o, a, b, &r[0]); break;
    case VDISC_FN_NO_MORE: f = vdisc_no_more_density(o, a, b); break;
    default: break;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) out[8 * i + k] = r[k];
  flag[i] = f ? 1 : 0;
}

hipError_t launch_vdisc_points(const DevScene* d_scene, uint32_t obj, int fn, uint64_t n, const double* d_in,
                               double* d_out, uint8_t* d_flag, hipStream_t stream) {
  hipLaunchKernelGGL(vdisc_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_scene, obj, fn, n,
                     d_in, d_out, d_flag);
  return hipGetLastError();
}

// Device check of the surface path's pieces (tests/test_gpu_surface_checks.py): one lane per
// input row, the production functions of this file and of appearance.h unchanged.  Row i is
// in[8 i ..], its results out[8 i ..] and flag[i]; `obj` is an object of the scene, or -1 for
// the celestial texture / the blackbody table.  Per request (SurfaceCheckFn):
//   DISC_CHORD    from xyz, to xyz           flag = hit, out[0] = t, out[1..3] = the point
//   SPHERE_CHORD  from xyz, to xyz (world)   flag = hit, out[0] = t, out[1..3] = the local point
//   WINDOW_FAR    ya[1..3], yb[1..3]         flag = window_far<G, VOL>, VOL = the scene has a gas
//   LUT_INDEX     x                          out[0] = lut_index over obj's lut_r (-1: bb_log_t)
//   TEMPERATURE   radius                     out[0] = status, out[1] = the temperature
//   BLACKBODY     temperature                out[0..3] = sample_blackbody, out[4] = its own
//                                            log10(fmax(T, 10)) (texture.rs:150, OCML's log10)
//   TEXTURE       u, v, redshift, T          out[0..3] = texture_color, out[4] = 1 where the
//                                            beaming factor is glibc's (pow_fast took it, or the
//                                            exponent is 0), 0 where rpow fell back to OCML
//   BLEND         self xyza, other xyza      out[0..3] = blend(self, other)
// Only WINDOW_FAR reads the chart G.
template <int G>
__global__ void __launch_bounds__(256) surface_points_kernel(const DevScene* __restrict__ Sp, int obj, int fn,
                                                             uint64_t n, const double* __restrict__ in,
                                                             double* __restrict__ out, uint8_t* __restrict__ flag) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return; includes the block barrier
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* q = in + 8 * i;
  const DevObject& o = S.obj[obj < 0 ? 0 : obj];
  const DevTexture& tex = obj < 0 ? S.celestial : o.tex;
  double r[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool f = false;
  switch (fn) {
    case SURFACE_FN_DISC_CHORD: f = disc_chord(o, q, q + 3, &r[0], &r[1]); break;
    case SURFACE_FN_SPHERE_CHORD: f = sphere_chord(o, q, q + 3, &r[0], &r[1]); break;
    case SURFACE_FN_WINDOW_FAR: {
      const double ya[4] = {0.0, q[0], q[1], q[2]}, yb[4] = {0.0, q[3], q[4], q[5]};
      f = S.has_vol ? window_far<G, true>(S, ya, yb) : window_far<G, false>(S, ya, yb);
      break;
    }
    case SURFACE_FN_LUT_INDEX: {
      const double* a = obj < 0 ? S.bb_log_t : o.lut_r;
      const uint32_t m = obj < 0 ? S.bb_n : o.lut_n;
      r[0] = (double)lut_index(a, m, a[0], a[m - 1], q[0]);
      break;
    }
    case SURFACE_FN_TEMPERATURE: r[0] = (double)compute_temperature(o, q[0], &r[1]); break;
    case SURFACE_FN_BLACKBODY: {
      const XYZA c = sample_blackbody(S, q[0]);
      r[0] = c.x, r[1] = c.y, r[2] = c.z, r[3] = c.a;
      r[4] = log10(fmax(q[0], 10.0));
      break;
    }
    case SURFACE_FN_TEXTURE: {
      const XYZA c = texture_color(S, tex, q[0], q[1], q[2], q[3]);
      r[0] = c.x, r[1] = c.y, r[2] = c.z, r[3] = c.a;
      double p;
      r[4] = (tex.beaming == 0.0 || glibc::pow_fast(q[2], tex.beaming, &p)) ? 1.0 : 0.0;
      break;
    }
    case SURFACE_FN_BLEND: {
      const XYZA c = blend(XYZA{q[0], q[1], q[2], q[3]}, XYZA{q[4], q[5], q[6], q[7]});
      r[0] = c.x, r[1] = c.y, r[2] = c.z, r[3] = c.a;
      break;
    }
    default: break;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) out[8 * i + k] = r[k];
  flag[i] = f ? 1 : 0;
}

hipError_t launch_surface_points(int geometry, const DevScene* d_scene, int obj, int fn, uint64_t n, const double* d_in,
                                 double* d_out, uint8_t* d_flag, hipStream_t stream) {
  return with_chart<DIAG_CHARTS>(geometry, [&](auto g) {
    hipLaunchKernelGGL(surface_points_kernel<decltype(g)::value>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       d_scene, obj, fn, n, d_in, d_out, d_flag);
    return hipGetLastError();
  });
}

#if GRT_PATH_COUNT
// this unit's counters plus the KerrBL unit's
hipError_t path_read(unsigned long long* out, bool reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_path), sizeof(g_path));
  if (e == hipSuccess && reset) {
    const unsigned long long z[2 * NPATH] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_path), z, sizeof(z));
  }
  unsigned long long bl[2 * NPATH];
  if (e == hipSuccess) e = kerr_bl::path_read(bl, reset);
  for (int k = 0; e == hipSuccess && k < 2 * NPATH; ++k) out[k] += bl[k];
  return e;
}
#endif

hipError_t launch_trajectories(int geometry, const DevScene* d_scene, const TrajectoryList& tl, hipStream_t stream) {
  if (tl.n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((tl.n + 63) / 64);
  return with_chart<DIAG_CHARTS>(geometry, [&](auto g) {
    hipLaunchKernelGGL(trajectory_kernel<decltype(g)::value>, dim3(blocks), dim3(64), 0, stream, d_scene, tl);
    return hipGetLastError();
  });
}

// ====================================================== invariant monitors =======
// The reference's per-ray health checks, off the render path:
//  * the null condition of the camera ray, |k.k| < 1e-10 (scene.rs:116-124, logged as an
//    error otherwise);
//  * in debug builds, the largest |k.k| over the accepted steps and the largest drift of
//    each constant of motion from its value at step 0, relative when |initial| > 1e-12
//    (integrator.rs:91-146), warned above 1e-4 (report_drifts, :176-201).  A ray whose
//    rkf45 fails returns Err before report_drifts: it reports no drift.
// health_kernel re-integrates the rays (one lane per ray) with these monitors.

// get_constants_of_motion at (x, p): E, L_z and, for KerrBL, Carter's Q.  Returns the count.
template <int G>
GDEV int constants_of_motion(const DevScene& S, const double* x, const double* p, double* c) {
  if constexpr (G == GRT_GEOM_EUCLIDEAN) {  // euclidean.rs:160-182
    const double p_x = -p[1], p_y = -p[2];
    c[0] = p[0];
    c[1] = x[1] * p_y - x[2] * p_x;
    return 2;
  } else if constexpr (G == GRT_GEOM_EUCLIDEAN_SPHERICAL) {  // euclidean_spherical.rs:147-166
    const double r = x[1], st = rsin(x[2]);
    c[0] = p[0];
    c[1] = -r * r * st * st * p[3];
    return 2;
  } else if constexpr (G == GRT_GEOM_SCHWARZSCHILD) {  // schwarzschild.rs:213-233
    const double r = x[1], st = rsin(x[2]);
    const double a = 1.0 - S.radius / r;
    c[0] = a * p[0];
    c[1] = -r * r * st * st * p[3];
    return 2;
  } else if constexpr (G == GRT_GEOM_KERR) {  // kerr.rs:421-445
    double g[4][4], pc[4];
    ks_metric(S.radius, S.a, x[1], x[2], x[3], g);
    mat_vec(g, p, pc);
    c[0] = -pc[0];
    c[1] = -x[2] * pc[1] + x[1] * pc[2];
    return 2;
  } else {  // KerrBL, kerr_bl.rs:596-625 (metric_bl's and this sin / cos of one theta: one sincos)
    double st, ct;
    rsincos(x[2], &st, &ct);
    double g[4][4], pc[4];
    metric_bl(S.radius, S.a, x[1], st, ct, g);
    mat_vec(g, p, pc);
    const double e = -pc[0], l_z = pc[3], p_theta = pc[2];
    const double sin2 = st * st;
    c[0] = e;
    c[1] = l_z;
    c[2] = p_theta * p_theta + ct * ct * (l_z * l_z / fmax(sin2, 1e-28) - S.a * S.a * e * e);
    return 3;
  }
}
// inner_product(x, v, v) at a native-chart point
template <int G>
GDEV double inner_at(const DevScene& S, const double* x, const double* v) {
  double st = 0.0, ct = 0.0;
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD || G == GRT_GEOM_EUCLIDEAN_SPHERICAL) st = rsin(x[2]);
  else if constexpr (G == GRT_GEOM_KERR_BL) rsincos(x[2], &st, &ct);
  return inner<G>(S, x, st, ct, v, v);
}
GDEV double drift_of(double cur, double init) {  // integrator.rs:127-134
  return fabs(init) > 1e-12 ? fabs(cur - init) / fabs(init) : fabs(cur - init);
}

// Per ray k (pixel (row0 + k / cols, col0 + k % cols)): out[k * 5 + 0] |k.k| of the camera
// ray, [1] the largest |k.k| over the accepted steps, [2..4] the largest drift of E, L_z, Q;
// status[k] = GRT_ERR_MAX_STEPS_REACHED when rkf45 failed (no drift report).
template <int G>
__global__ void __launch_bounds__(64) health_kernel(const DevScene* __restrict__ Sp, WorkList wl, uint64_t n,
                                                    double* __restrict__ out, uint8_t* __restrict__ status) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double row = (double)(wl.row0 + (uint32_t)(k / wl.cols)), col = (double)(wl.col0 + (uint32_t)(k % wl.cols));
  double pcam[4];
  camera_momentum(S.cam, row, col, pcam);
  const double null_kk = fabs(inner<G>(S, S.cam.pos, S.cam.sin_theta, S.cam.cos_theta, pcam, pcam));
  double y[8];
  RayConst rc;
  init_ray<G>(S, row, col, y, rc);
  double p[4], c0[3] = {0.0, 0.0, 0.0}, c1[3];
  momentum<G>(S, rc, y, p);
  const int nc = constants_of_motion<G>(S, y, p, c0);
  double max_kk = 0.0, max_d[3] = {0.0, 0.0, 0.0};
  int st_out = GRT_OK;
  double h = S.step_size;
  for (uint64_t i = 1; i < S.max_steps; ++i) {
    double h_cur = rclamp(h, H_MIN, H_MAX), h_next = 0.0, yn[8];
    int retries = 0, ctl;
    do {
      const double err_sq = rkf_attempt<G>(S, rc, y, h_cur, yn);
      ctl = step_control(S, err_sq, h_cur, retries, h_next);
    } while (ctl == STEP_RETRY);
    if (ctl == STEP_FAILED) {
      st_out = GRT_ERR_MAX_STEPS_REACHED;
      break;
    }
    h = h_next;
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = yn[q];
    momentum<G>(S, rc, y, p);
    const double kk = fabs(inner_at<G>(S, y, p));
    if (kk > max_kk) max_kk = kk;
    constants_of_motion<G>(S, y, p, c1);
    for (int q = 0; q < nc; ++q) {
      const double d = drift_of(c1[q], c0[q]);
      if (d > max_d[q]) max_d[q] = d;
    }
    double c[3];
    bool c_valid = false;
    if (should_stop<G>(S, y, c, c_valid, i) != GRT_STOP_NONE) break;
  }
  double* o = out + k * 5;
  o[0] = null_kk;
  o[1] = max_kk;
  o[2] = max_d[0];
  o[3] = max_d[1];
  o[4] = max_d[2];
  status[k] = (uint8_t)st_out;
}

hipError_t launch_health(int geometry, const DevScene* d_scene, const WorkList& wl, uint64_t n, double* d_out,
                         uint8_t* d_status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((n + 63) / 64);
  return with_chart<DIAG_CHARTS>(geometry, [&](auto g) {
    hipLaunchKernelGGL(health_kernel<decltype(g)::value>, dim3(blocks), dim3(64), 0, stream, d_scene, wl, n, d_out,
                       d_status);
    return hipGetLastError();
  });
}

#endif  // GRT_MAIN_TU
#if GRT_MAIN_TU || GRT_SEQ  // the work-order probes: the exact builds of every chart
#include "geodesic_probe.h"

hipError_t launch_impact_keys(const DevScene* d_scene, const WorkList& wl, uint32_t n_tiles, uint32_t* d_keys,
                              hipStream_t stream CAMS_PARAM) {
  if (n_tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(impact_key_kernel, dim3((n_tiles + 63) / 64), dim3(64), 0, stream, d_scene, wl, n_tiles,
                     d_keys CAMS_ARG);
  return hipGetLastError();
}

hipError_t launch_class_keys(const DevScene* d_scene, const WorkList& wl, uint32_t corners_x, uint32_t n_corners,
                             float* d_a, hipStream_t stream CAMS_PARAM) {
  if (n_corners == 0) return hipSuccess;
  hipLaunchKernelGGL(class_key_kernel, dim3((n_corners + 63) / 64), dim3(64), 0, stream, d_scene, wl, corners_x,
                     n_corners, d_a CAMS_ARG);
  return hipGetLastError();
}

hipError_t launch_probe(int geometry, const DevScene* d_scene, const WorkList& wl, uint32_t n_tiles, uint32_t cap,
                        uint32_t* d_steps, bool quad, hipStream_t stream CAMS_PARAM) {
  if (n_tiles == 0) return hipSuccess;
  if (quad && geometry == GRT_GEOM_KERR) {
    hipLaunchKernelGGL(probe_quad_kernel, dim3((n_tiles * 4ull + 255) / 256), dim3(256), 0, stream, d_scene, wl,
                       n_tiles, cap, d_steps CAMS_ARG);
    return hipGetLastError();
  }
  const unsigned blocks = (n_tiles + 63) / 64;
  return with_chart<PROBE_CHARTS>(geometry, [&](auto g) {
    hipLaunchKernelGGL(probe_kernel<decltype(g)::value>, dim3(blocks), dim3(64), 0, stream, d_scene, wl, n_tiles, cap,
                       d_steps CAMS_ARG);
    return hipGetLastError();
  });
}
#endif  // GRT_MAIN_TU || GRT_SEQ
// ============================================================ shade kernel =======
// Evaluate one recorded candidate: the emitter step at the intersection
// (objects.rs:27-44 + :95-115), its redshift, temperature and texture colour.
// A VolumetricDisc candidate gets its energy and temperature (and their errors) here;
// its colour is the raymarch of march_kernel (volumetric_disc.rs:580-601), so *col is
// left untouched.  color = false: errors only (the job-gathering pass).
// geo (nullable, the geometry buffer's fill): the appearance-independent numbers the colour
// is a function of -- texture_color's (u, v, redshift) and compute_temperature's radius
// (+0.0 for a sphere, whose temperature is a constant of the object).
template <int G>
GDEV int shade_record(const DevScene& S, const RayConst& rc, const DevObject& o, const double* p,
                      const double* pt, XYZA* col, bool color = true, double* geo = nullptr) {
  double u_tex = 0.0, v_tex = 0.0, wx, wy, wz;
  if (o.kind == GRT_OBJ_VOLUMETRIC_DISC) {  // world hit point (its uv is not used for colour)
    wx = pt[0];
    wy = pt[1];
    wz = pt[2];
  } else if (o.kind == GRT_OBJ_DISC) {  // disc.rs:60-76 uv from the in-plane point
    wx = pt[0];
    wy = pt[1];
    wz = pt[2];
    double rr = wx * wx + wy * wy + wz * wz;
    double phi = atan2(wy - 0.0, wx - 0.0);
    double r = (sqrt(rr) - o.rin) / (o.rout - o.rin);
    double sp, cp;
    rsincos(phi, &sp, &cp);
    u_tex = 0.5 + 0.5 * r * cp;
    v_tex = 0.5 + 0.5 * r * sp;
  } else {  // sphere.rs:92-117 uv from the sphere-local point, world point for physics
    double rr, theta, phi;
    cart_to_sph(pt[0], pt[1], pt[2], &rr, &theta, &phi);
    double u = (PI + phi) / TWO_PI;
    u_tex = 1.0 - u;
    v_tex = theta / PI;
    wx = pt[0] + o.cx;
    wy = pt[1] + o.cy;
    wz = pt[2] + o.cz;
  }
  double x[4];  // step.x = intersection point converted to the native chart
  double st = 0.0, ct = 0.0;
  x[0] = 0.0;
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD || G == GRT_GEOM_EUCLIDEAN_SPHERICAL) {
    cart_to_sph(wx, wy, wz, &x[1], &x[2], &x[3]);
    st = rsin(x[2]);  // the only trig of the spherical inner products (ct unused)
  } else if constexpr (G == GRT_GEOM_KERR_BL) {
    cart_to_bl(S.a, wx, wy, wz, &x[1], &x[2], &x[3]);
    rsincos(x[2], &st, &ct);
  } else {
    x[1] = wx;
    x[2] = wy;
    x[3] = wz;
  }
  double u[4];
  if (o.kind != GRT_OBJ_SPHERE) {  // disc.rs:101-110, volumetric_disc.rs:603-612: circular-orbit emitter
    if constexpr (G == GRT_GEOM_EUCLIDEAN || G == GRT_GEOM_EUCLIDEAN_SPHERICAL) {  // at rest in flat space
      u[0] = 1.0; u[1] = 0.0; u[2] = 0.0; u[3] = 0.0;
    } else {
      double r;
      if constexpr (G == GRT_GEOM_KERR) r = sqrt(ks_r_sqr(S.a, x[1], x[2], x[3]));
      else r = x[1];
      double ut, uphi;
      if (!killing_coefficients(S, r, &ut, &uphi)) return GRT_ERR_NO_CIRCULAR_ORBIT;
      if constexpr (G == GRT_GEOM_KERR) {
        double ax[4] = {0.0, -x[2], x[1], 0.0};
        double et[4] = {1.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = ut * et[q] + uphi * ax[q];
      } else {
        u[0] = ut; u[1] = 0.0; u[2] = 0.0; u[3] = uphi;
      }
    }
  } else {  // sphere.rs:141-150: static emitter
    stationary_velocity<G>(S, x, u);
  }
  double em = inner<G>(S, x, st, ct, u, p);
  double sig0 = signature0<G>();
  double redshift = (sig0 * rc.obs) / (sig0 * em);  // redshift.rs:36-38
  double temperature;
  if (geo) {
    geo[0] = u_tex;
    geo[1] = v_tex;
    geo[2] = redshift;
    geo[3] = 0.0;
  }
  if (o.kind != GRT_OBJ_SPHERE) {  // disc.rs:112-120, volumetric_disc.rs:614-622
    double rad;  // get_radial_coordinate of the Cartesian intersection point
    if constexpr (G == GRT_GEOM_KERR || G == GRT_GEOM_KERR_BL) {
      rad = sqrt(ks_r_sqr(S.a, wx, wy, wz));
    } else {
      rad = sqrt(wx * wx + wy * wy + wz * wz);
    }
    if (geo) geo[3] = rad;
    int e = compute_temperature(o, rad, &temperature);
    if (e != GRT_OK) return e;
  } else {
    temperature = o.temperature;
  }
  if (color && o.kind != GRT_OBJ_VOLUMETRIC_DISC) *col = texture_color(S, o.tex, u_tex, v_tex, redshift, temperature);
  return GRT_OK;
}

// ---- a ray's candidates in window order: workspace slots 0..GRT_WS_SLOTS-1, then the
// hit pool's list (HitPool).
struct RecRef {
  bool pool;
  uint64_t s;  // workspace slot j * n + idx, or pool record
};
// Candidates a ray can replay in order: all of them, unless its pool list was lost
// (the pool was full), in which case only the workspace slots (*lost = true).
GDEV uint32_t rec_count(const Workspace& ws, uint64_t idx, uint32_t nrec, bool* lost) {
  *lost = nrec > GRT_WS_SLOTS && ws.pool->last[idx] == HIT_NIL;
  return *lost ? GRT_WS_SLOTS : nrec;
}
// Candidate j, for j = 0, 1, 2, ... in turn (*pos carries the position in the pool list).
GDEV RecRef rec_at(const Workspace& ws, uint64_t idx, uint32_t j, uint32_t* pos) {
  if (j < GRT_WS_SLOTS) return RecRef{false, (uint64_t)j * ws.n + idx};
  *pos = (j == GRT_WS_SLOTS) ? ws.pool->head[idx] : ws.pool->next[*pos];
  return RecRef{true, *pos};
}
GDEV uint32_t rec_win(const Workspace& ws, const RecRef& r) { return r.pool ? ws.pool->win[r.s] : ws.rec[r.s].win; }
// The window of candidate j + 1 (which exists), given candidate j.
GDEV uint32_t rec_next_win(const Workspace& ws, uint64_t idx, uint32_t j, const RecRef& r) {
  if (j + 1 < GRT_WS_SLOTS) return ws.rec[r.s + ws.n].win;
  if (j + 1 == GRT_WS_SLOTS) return ws.pool->win[ws.pool->head[idx]];
  return ws.pool->win[ws.pool->next[r.s]];
}
GDEV uint32_t rec_read(const Workspace& ws, const RecRef& r, double* p, double* pt) {
  if (!r.pool) {
    const double2* d = reinterpret_cast<const double2*>(ws.rec + r.s);
    const double2 a = d[0], b = d[1], c = d[2], e = d[3];
    p[0] = a.x;
    p[1] = a.y;
    p[2] = b.x;
    p[3] = b.y;
    pt[0] = c.x;
    pt[1] = c.y;
    pt[2] = e.x;
    return (uint32_t)__double2hiint(e.y);
  }
  const uint64_t m = ws.pool->cap;
#pragma unroll
  for (int q = 0; q < 4; ++q) p[q] = ws.pool->p[q * m + r.s];
#pragma unroll
  for (int q = 0; q < 3; ++q) pt[q] = ws.pool->pt[q * m + r.s];
  return ws.pool->obj[r.s];
}

// Volumetric scenes, pass 1: the candidate slots whose raymarched colour the composite
// needs -- the window-nearest VolumetricDisc hits of a ray whose window pass raises no
// error (an error aborts the pixel, scene.rs:146, so its marches would be wasted).
// Workspace slots come back as a mask; pool records get their jobs appended here.
template <int G>
GDEV uint32_t march_slots(const DevScene& S, const WorkList& wl, const Workspace& ws, uint64_t idx CAMS_PARAM) {
  RayConst rc;
  double y[8];
  const RayMeta mt = fin_get<G>(ws, idx, y, rc);
  if (mt.status != GRT_OK) return 0u;
  if constexpr (G != GRT_GEOM_KERR_BL) rc.obs = observer_energy<G>(S, wl, idx CAMS_ARG);
  bool lost;
  const uint32_t nr = rec_count(ws, idx, mt.nrec, &lost);
  uint32_t mask = 0u, pool_jobs = 0u, pos = HIT_NIL;
  for (uint32_t j = 0; j < nr; ++j) {
    const RecRef r = rec_at(ws, idx, j, &pos);
    const uint32_t win = rec_win(ws, r);
    double p[4], pt[3];
    const DevObject& o = S.obj[rec_read(ws, r, p, pt)];
    XYZA col;
    if (shade_record<G>(S, rc, o, p, pt, &col, false) != GRT_OK) return 0u;
    bool last_in_window = (j + 1 == nr) || (rec_next_win(ws, idx, j, r) != win);
    if (last_in_window && o.kind == GRT_OBJ_VOLUMETRIC_DISC) {
      if (!r.pool) mask |= 1u << j;
      else pool_jobs++;
    }
  }
  if (pool_jobs) {  // the rare rays with more than GRT_WS_SLOTS candidates: no error, append
    unsigned long long at = atomicAdd(ws.march, (unsigned long long)pool_jobs);
    pos = HIT_NIL;
    for (uint32_t j = GRT_WS_SLOTS; j < nr; ++j) {
      const RecRef r = rec_at(ws, idx, j, &pos);
      bool last_in_window = (j + 1 == nr) || (rec_next_win(ws, idx, j, r) != rec_win(ws, r));
      if (last_in_window && S.obj[ws.pool->obj[r.s]].kind == GRT_OBJ_VOLUMETRIC_DISC)
        ws.jobs[at++] = JOB_POOL | (idx << 31) | r.s;
    }
  }
  return mask;
}

// The celestial sphere's texture arguments of a ray that ended on it (scene.rs:184-195):
// get_as_spherical of the final position (point.rs:172-188) as (1 - u, v), and the redshift
// against a static emitter there.
template <int G>
GDEV void celestial_args(const DevScene& S, const RayConst& rc, const double* y, double* u_tex, double* v_tex,
                         double* redshift) {
  double th, ph;
  double st = 0.0, ct = 0.0;
  if constexpr (G == GRT_GEOM_SCHWARZSCHILD || G == GRT_GEOM_KERR_BL || G == GRT_GEOM_EUCLIDEAN_SPHERICAL) {
    th = rem_euclid(y[2], PI);
    ph = rem_euclid(y[3] + PI, TWO_PI) - PI;
    if constexpr (G != GRT_GEOM_KERR_BL) st = rsin(y[2]);  // inner_product: sin only
    else rsincos(y[2], &st, &ct);
  } else {
    double rr;
    cart_to_sph(y[1], y[2], y[3], &rr, &th, &ph);
  }
  double u = (PI + ph) / TWO_PI;
  double v = th / PI;
  double vel[4], p[4];
  stationary_velocity<G>(S, y, vel);
  momentum<G>(S, rc, y, p);
  double em = inner<G>(S, y, st, ct, vel, p);
  double sig0 = signature0<G>();
  *redshift = (sig0 * rc.obs) / (sig0 * em);
  *u_tex = 1.0 - u;
  *v_tex = v;
}

// Scene::color_of_ray's window pass, terminal colour and composite (scene.rs:141-219),
// one lane per ray, over the candidates the integrate kernel recorded.
//   MODE 0: scenes without volumetric objects.
//   MODE 1: volumetric scenes, pass 1 -- append the raymarch jobs (wave-aggregated).
//   MODE 2: volumetric scenes, pass 3 -- composite with the raymarched colours (ws.vcol).
template <int G, int MODE>
__global__ void __launch_bounds__(256) shade_kernel(const DevScene* __restrict__ Sp, WorkList wl, Workspace ws,
                                                    Outputs out, unsigned long long* __restrict__ stats CAMS_PARAM) {
  const DevScene& S = *Sp;
  const uint64_t n = ws.n;
  const uint64_t n_live = ws.n_live ? (uint64_t)min((unsigned long long)n, *ws.n_live) : n;
  // a block past the live rays (the empty chunks of a supersample pass) has nothing to do;
  // block 0 stays for the pool high-water mark below
  if (blockIdx.x != 0 && (uint64_t)blockIdx.x * blockDim.x >= n_live) return;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (MODE == 1) {
    const uint32_t mask = idx < n_live ? march_slots<G>(S, wl, ws, idx CAMS_ARG) : 0u;
    const int lane = threadIdx.x & 63;
    const uint32_t c = __popc(mask);
    uint32_t incl = c;  // inclusive wave prefix sum of the job counts
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    const uint32_t total = __shfl(incl, 63);
    unsigned long long base = 0;
    if (lane == 63 && total) base = atomicAdd(ws.march, (unsigned long long)total);
    base = __shfl(base, 63);
    uint64_t pos = base + incl - c;
    for (uint32_t m = mask; m; m &= m - 1u) ws.jobs[pos++] = (idx << 8) | (uint64_t)__ffs(m) - 1u;
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(ws.pool->count + 1, *ws.pool->count);
  if (idx >= n_live) return;
  RayConst rc;
  double y[8];
  const RayMeta mt = fin_get<G>(ws, idx, y, rc);
  int status = mt.status;
  const int stop = mt.stop;
  if constexpr (G == GRT_GEOM_KERR_BL) {
    if (out.steps) out.steps[idx] = mt.steps;  // the other charts: written by store_ray
  }
  const XYZA fail{0.0, 0.0, 0.0, 1.0};
  if (status != GRT_OK) {  // integrate error: reference default pixel (raytracer.rs:204-210)
    write_out(out, idx, fail, GRT_CLASS_ESCAPED, status, stop, 0u);
    return;
  }
  if constexpr (G != GRT_GEOM_KERR_BL) rc.obs = observer_energy<G>(S, wl, idx CAMS_ARG);
  bool lost;
  const uint32_t nr = rec_count(ws, idx, mt.nrec, &lost);
  // window-nearest hits: the first ones in registers, the later ones (pool records of
  // rays with more than GRT_WS_SLOTS candidates) next to their record, linked backwards
  XYZA hits[GRT_WS_SLOTS];
  uint32_t nh = 0, n_pool_hits = 0, pos = HIT_NIL, last_pool_hit = HIT_NIL;
  double opacity = 0.0;
  for (uint32_t j = 0; j < nr; ++j) {
    const RecRef r = rec_at(ws, idx, j, &pos);
    const uint32_t win = rec_win(ws, r);
    double p[4], pt[3];
    const DevObject& o = S.obj[rec_read(ws, r, p, pt)];
    XYZA col{0.0, 0.0, 0.0, 0.0};
    int e = shade_record<G>(S, rc, o, p, pt, &col);
    if (e != GRT_OK) {  // any window error aborts the pixel (scene.rs:146, objects.rs:96-102)
      write_out(out, idx, fail, GRT_CLASS_ESCAPED, e | (lost ? GRT_FLAG_HIT_OVERFLOW : 0), stop, nh + n_pool_hits);
      if (lost) atomicAdd(stats + 3, 1ull);
      return;
    }
    bool last_in_window = (j + 1 == nr) || (rec_next_win(ws, idx, j, r) != win);
    if constexpr (MODE == 2) {
      if (last_in_window && o.kind == GRT_OBJ_VOLUMETRIC_DISC) {
        const double* vc = r.pool ? ws.pool->vcol : ws.vcol;
        const uint64_t m = r.pool ? ws.pool->cap : (uint64_t)GRT_WS_SLOTS * n;
        col = XYZA{vc[r.s], vc[m + r.s], vc[2 * m + r.s], vc[3 * m + r.s]};
      }
    }
    if (last_in_window) {  // the window's nearest hit
      if (!r.pool) {
        hits[nh++] = col;
      } else {
        const uint64_t m = ws.pool->cap;
        ws.pool->hcol[r.s] = col.x;
        ws.pool->hcol[m + r.s] = col.y;
        ws.pool->hcol[2 * m + r.s] = col.z;
        ws.pool->hcol[3 * m + r.s] = col.a;
        ws.pool->hprev[r.s] = last_pool_hit;
        last_pool_hit = (uint32_t)r.s;
        n_pool_hits++;
      }
      double alpha = rclamp(col.a, 0.0, 1.0);
      opacity = alpha + opacity * (1.0 - alpha);
    }
  }
  // terminal colour (scene.rs:157-205) and back-to-front blend (:206-210)
  XYZA result{0.0, 0.0, 0.0, 1.0};
  int cls = GRT_CLASS_CAPTURED;
  if (stop == GRT_STOP_HORIZON || stop == GRT_STOP_CLOSED_ORBIT) {
    result = blend(result, XYZA{0.0, 0.0, 0.0, 1.0});
  } else if (stop == GRT_STOP_CELESTIAL) {
    double u_tex, v_tex, redshift;
    celestial_args<G>(S, rc, y, &u_tex, &v_tex, &redshift);
    result = blend(result, texture_color(S, S.celestial, u_tex, v_tex, redshift, S.celestial_temperature));
    cls = GRT_CLASS_ESCAPED;
  }
  // back to front: the pool's hits (the farthest windows), then the first ones
  for (uint32_t q = last_pool_hit; q != HIT_NIL; q = ws.pool->hprev[q]) {
    const uint64_t m = ws.pool->cap;
    result = blend(result, XYZA{ws.pool->hcol[q], ws.pool->hcol[m + q], ws.pool->hcol[2 * m + q], ws.pool->hcol[3 * m + q]});
  }
  for (int k = (int)nh - 1; k >= 0; --k) result = blend(result, hits[k]);
  if (opacity >= S.hit_threshold) cls = GRT_CLASS_HIT;
  if (lost) {  // the pool was full: candidates past the workspace slots are missing
    status |= GRT_FLAG_HIT_OVERFLOW;
    atomicAdd(stats + 3, 1ull);
  }
  write_out(out, idx, result, cls, status, stop, nh + n_pool_hits);
}

#if !GRT_FUSED  // the geometry buffer: the exact units only
#include "geodesic_fill.h"

hipError_t launch_gbuffer_fill(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                               const GBufferArrays& gb, hipStream_t stream CAMS_PARAM LAPSE_PARAM) {
  if (gb.n == 0) return hipSuccess;
#if GRT_LAPSE
  if (!lapse) return hipErrorInvalidValue;
#endif
#if GRT_SEQ  // the stack from (0, 0): whole frames, one camera each, or an offset list over them (a slot per entry)
  if (!ct.cams || ct.cam_rows == 0 || ct.n_cams == 0 || wl.row0 != 0 || wl.col0 != 0 ||
      (uint64_t)wl.rows != (uint64_t)ct.cam_rows * ct.n_cams || (wl.pixel_index && (!wl.dx || !wl.dy)) ||
      gb.n != (wl.pixel_index ? wl.n_items : (uint64_t)wl.rows * wl.cols))
    return hipErrorInvalidValue;
#endif
  return with_chart<FILL_CHARTS>(geometry, [&](auto g) {
    hipLaunchKernelGGL(gbuffer_fill_kernel<decltype(g)::value>, dim3((unsigned)((gb.n + 255) / 256)), dim3(256), 0,
                       stream, d_scene, wl, ws, gb CAMS_ARG LAPSE_ARG);
    return hipGetLastError();
  });
}
#endif  // !GRT_FUSED

// ------------------------------------------------------------------ launch -------
// Plain scenes: integrate [-> tail] -> shade.  Volumetric scenes (VOL): integrate [-> tail] ->
// gather raymarch jobs -> march (persistent, lane refill) -> composite; ws.march must be
// zeroed.  The tail (Kerr-Schild) continues the long rays the integrate kernel handed off.
template <int G, bool VOL>
static hipError_t launch_g(const DevScene* d_scene, const WorkList& wl, const Workspace& ws_in, const Outputs& out,
                           unsigned long long* d_counter, unsigned long long* d_stats, int blocks, int threads,
                           const TailList& tl_in, int tail_blocks, hipStream_t stream CAMS_PARAM) {
  const unsigned nb = (unsigned)((ws_in.n + 255) / 256);
  Workspace ws = ws_in;
  ws.steps = G == GRT_GEOM_KERR_BL ? nullptr : out.steps;  // store_ray writes the per-pixel step counts
  TailList tl = tl_in;
  if (G != GRT_GEOM_KERR || tail_blocks <= 0) tl.cap = 0;
  if (VOL && (!ws.rec_dir || !ws.vcol || !ws.jobs || !ws.march)) return hipErrorInvalidValue;
#if GRT_LAPSE
  if (VOL) return hipErrorInvalidValue;  // no raymarch kernels in this unit (VolumetricDisc scenes have no buffer)
#endif
  hipLaunchKernelGGL((integrate_kernel<G, VOL>), dim3(blocks), dim3(threads), 0, stream, d_scene, wl, ws, d_counter,
                     d_stats, tl CAMS_ARG);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if constexpr (G == GRT_GEOM_KERR) {
    if (tl.cap) {
      hipLaunchKernelGGL((tail_kernel<G, VOL>), dim3(tail_blocks), dim3(256), 0, stream, d_scene, ws, tl, d_stats);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  hipLaunchKernelGGL((shade_kernel<G, VOL ? 1 : 0>), dim3(nb), dim3(256), 0, stream, d_scene, wl, ws, out,
                     d_stats CAMS_ARG);
  e = hipGetLastError();
#if !GRT_LAPSE
  if constexpr (VOL) {
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((march_kernel<G>), dim3(blocks), dim3(256), 0, stream, d_scene, ws);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((shade_kernel<G, 2>), dim3(nb), dim3(256), 0, stream, d_scene, wl, ws, out, d_stats CAMS_ARG);
    e = hipGetLastError();
  }
#endif
  return e;
}

hipError_t launch_trace(int geometry, const DevScene* d_scene, const WorkList& wl, const Workspace& ws,
                        const Outputs& out, unsigned long long* d_counter, unsigned long long* d_stats, int blocks,
                        int threads, bool vol, const TailList& tl, int tail_blocks, hipStream_t stream CAMS_PARAM) {
  if (ws.n == 0) return hipSuccess;
#if GRT_SEQ
  if (!ct.cams || ct.cam_rows == 0 || ct.n_cams == 0) return hipErrorInvalidValue;
#endif
#if GRT_LAPSE
  if (vol) return hipErrorInvalidValue;
  return with_chart<TRACE_CHARTS>(geometry, [&](auto g) {
    return launch_g<decltype(g)::value, false>(d_scene, wl, ws, out, d_counter, d_stats, blocks, threads, tl,
                                               tail_blocks, stream);
  });
#else
  return with_chart<TRACE_CHARTS>(geometry, [&](auto g) {
    constexpr int G = decltype(g)::value;
    return vol ? launch_g<G, true>(d_scene, wl, ws, out, d_counter, d_stats, blocks, threads, tl, tail_blocks,
                                   stream CAMS_ARG)
               : launch_g<G, false>(d_scene, wl, ws, out, d_counter, d_stats, blocks, threads, tl, tail_blocks,
                                    stream CAMS_ARG);
  });
#endif
}

#if GRT_MAIN_TU || GRT_FUSED || GRT_KERR_BL_TU
// Test hook (grt_debug_vdisc_march): this unit's march_kernel alone, as launch_g launches it.
hipError_t launch_march(int geometry, const DevScene* d_scene, const Workspace& ws, int blocks, hipStream_t stream) {
  if (blocks <= 0 || !ws.rec || !ws.rec_dir || !ws.vcol || !ws.jobs || !ws.march || !ws.rc || !ws.pool)
    return hipErrorInvalidValue;
  return with_chart<TRACE_CHARTS>(geometry, [&](auto g) {
    hipLaunchKernelGGL((march_kernel<decltype(g)::value>), dim3(blocks), dim3(256), 0, stream, d_scene, ws);
    return hipGetLastError();
  });
}
#endif

#if GRT_FUSED || GRT_KERR_BL_TU || GRT_SEQ || GRT_LAPSE
}  // namespace fused / kerr_bl / seq / lapse / lapse_kerr_bl
#endif
}  // namespace grt
