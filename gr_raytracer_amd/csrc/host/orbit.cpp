// orbit.cpp — host restatement of the disc's orbital motion (grt_api.h: grt_orbit_rate,
// grt_gbuffer_orbit_uv, grt_gbuffer_orbit_uv_retarded).  The rule is the device's (device/gbuffer_shade.hip: orbit_rate, orbit_uv)
// with the same operations in the same order, compiled without contraction, over the host
// build of device/glibc_math.h: pow_fast / sincos_fast, and the host libm outside their fast
// paths.  Device and host agree bit for bit for |omega t| < 105414350, the range of the exact
// sincos; beyond it the device takes the fallback the render takes (within 1 ulp of libm).
// No device code: the file is what a CPU-only sanitizer build links (tools/orbit_uv_main.cpp).
#include <cerrno>
#include <cmath>
#include <cstdint>

#include "../device/glibc_math.h"
#include "grt_api.h"
#include "host_internal.h"

namespace {

int fail(int code, const char* msg) {
  grt_host::set_error(msg);
  return code;
}

double pow_(double x, double y) {
  double r;
  if (grt::glibc::pow_fast(x, y, &r)) return r;
  return std::pow(x, y);
}

// killing_coefficients' omega (host/setup.cpp, device/geodesic.hip); +0.0 where shade_record's
// emitter is at rest.  false: unknown geometry.
bool orbit_rate(int32_t geometry, double r_s, double a, double r, double* omega) {
  switch (geometry) {
    case GRT_GEOM_EUCLIDEAN:
    case GRT_GEOM_EUCLIDEAN_SPHERICAL:
      *omega = 0.0;
      return true;
    case GRT_GEOM_SCHWARZSCHILD:
    case GRT_GEOM_KERR:
    case GRT_GEOM_KERR_BL: {
      const double m = 0.5 * r_s;
      const double sqrt_m = std::sqrt(m);
      *omega = sqrt_m / (pow_(r, 1.5) + a * sqrt_m);
      return true;
    }
    default:
      return false;
  }
}

void orbit_uv(double omega, double t, double* u, double* v) {
  const double th = omega * t;
  if (th == 0.0 || !std::isfinite(th)) return;  // (u, v) unchanged, bit for bit
  double s, c;
  if (!grt::glibc::sincos_fast(th, &s, &c)) {
    s = std::sin(th);
    c = std::cos(th);
  }
  const double du = *u - 0.5, dv = *v - 0.5;
  *u = 0.5 + (du * c + dv * s);
  *v = 0.5 + (dv * c - du * s);
}

}  // namespace

extern "C" {

int grt_orbit_rate(int32_t geometry, double radius, double a, double r, double* omega) {
  if (!omega) return fail(-EINVAL, "grt_orbit_rate: null output");
  if (!orbit_rate(geometry, radius, a, r, omega)) return fail(-EINVAL, "grt_orbit_rate: unknown geometry");
  return 0;
}

// grt_gbuffer_orbit_uv (lapse NULL: every layer at `time`) and grt_gbuffer_orbit_uv_retarded
// (a disc layer at time + lapse[k]).
static int orbit_uv_layers(const grt_gbuffer_shape* shape, uint64_t n_layers, const uint8_t* object, const double* u,
                           const double* v, const double* radius, const double* lapse, double time, double* u_out,
                           double* v_out) {
  if (!shape || !object || !u || !v || !radius || !u_out || !v_out)
    return fail(-EINVAL, "grt_gbuffer_orbit_uv: null argument");
  if (!std::isfinite(time)) return fail(-EINVAL, "grt_gbuffer_orbit_uv: the time is not finite");
  if (shape->n_objects > GRT_MAX_OBJECTS) return fail(-EINVAL, "grt_gbuffer_orbit_uv: more than GRT_MAX_OBJECTS objects");
  double probe;
  if (!orbit_rate(shape->geometry, shape->radius, shape->a, 1.0, &probe))
    return fail(-EINVAL, "grt_gbuffer_orbit_uv: unknown geometry");
  // nothing is written before every index is known to be in range
  for (uint64_t k = 0; k < n_layers; ++k)
    if (object[k] >= shape->n_objects) return fail(-EINVAL, "grt_gbuffer_orbit_uv: an object index is out of range");
  for (uint64_t k = 0; lapse && k < n_layers; ++k)
    if (!std::isfinite(lapse[k])) return fail(-EINVAL, "grt_gbuffer_orbit_uv_retarded: a lapse is not finite");
  for (uint64_t k = 0; k < n_layers; ++k) {
    double uk = u[k], vk = v[k];
    if (shape->objects[object[k]].kind == GRT_OBJ_DISC) {
      double omega;
      orbit_rate(shape->geometry, shape->radius, shape->a, radius[k], &omega);
      const double te = lapse ? time + lapse[k] : time;  // the emission time
      orbit_uv(omega, te, &uk, &vk);
    }
    u_out[k] = uk;
    v_out[k] = vk;
  }
  return 0;
}

int grt_gbuffer_orbit_uv(const grt_gbuffer_shape* shape, uint64_t n_layers, const uint8_t* object, const double* u,
                         const double* v, const double* radius, double time, double* u_out, double* v_out) {
  return orbit_uv_layers(shape, n_layers, object, u, v, radius, nullptr, time, u_out, v_out);
}

int grt_gbuffer_orbit_uv_retarded(const grt_gbuffer_shape* shape, uint64_t n_layers, const uint8_t* object,
                                  const double* u, const double* v, const double* radius, const double* lapse,
                                  double time, double* u_out, double* v_out) {
  if (!lapse) return fail(-EINVAL, "grt_gbuffer_orbit_uv_retarded: null lapse");
  return orbit_uv_layers(shape, n_layers, object, u, v, radius, lapse, time, u_out, v_out);
}

}  // extern "C"
