// glibc_check.cpp — host side of the glibc test hooks (not in grt_api.h).
//
// grt_debug_glibc_host evaluates device/glibc_math.h, compiled for the host without
// contraction, through the same wrappers and with the same path byte as
// grt_debug_glibc_device (api.hip; fn and outputs: device/glibc_check.h).  It is the
// restatement tests/test_glibc_math.py ties to glibc bit for bit, and the expectation
// tests/test_gpu_glibc_math.py holds the device to.  Lanes the fast paths refuse get the
// host libm's value; fn | GLIBC_FN_LIBM gives the host libm's own function on every lane.
// libm is called through pointers from dlsym, so the compiler can neither fold a call
// nor fuse sin and cos of one operand into sincos.
#include <dlfcn.h>

#include <cerrno>
#include <string>

#include "../device/glibc_check.h"
#include "../device/glibc_math.h"
#include "host_internal.h"

namespace {

struct Libm {
  double (*pow)(double, double) = nullptr;
  double (*exp)(double) = nullptr;
  double (*sin)(double) = nullptr;
  double (*cos)(double) = nullptr;
  void (*sincos)(double, double*, double*) = nullptr;
  bool ok = false;
  Libm() {
    void* h = dlopen("libm.so.6", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    pow = reinterpret_cast<double (*)(double, double)>(dlsym(h, "pow"));
    exp = reinterpret_cast<double (*)(double)>(dlsym(h, "exp"));
    sin = reinterpret_cast<double (*)(double)>(dlsym(h, "sin"));
    cos = reinterpret_cast<double (*)(double)>(dlsym(h, "cos"));
    sincos = reinterpret_cast<void (*)(double, double*, double*)>(dlsym(h, "sincos"));
    ok = pow && exp && sin && cos && sincos;
  }
};

}  // namespace

extern "C" int grt_debug_glibc_host(int fn, uint64_t n, const double* x, const double* y, double* out0, double* out1,
                                    uint8_t* path) {
  namespace g = grt::glibc;
  static const Libm m;
  const bool libm_only = (fn & grt::GLIBC_FN_LIBM) != 0;
  fn &= ~(int)grt::GLIBC_FN_LIBM;
  if (!x || !out0 || !out1 || !path || fn < 0 || fn >= grt::GLIBC_FN_COUNT || (fn == grt::GLIBC_FN_POW && !y)) {
    grt_host::set_error("glibc host check: bad argument");
    return -EINVAL;
  }
  if (!m.ok) {
    grt_host::set_error("glibc host check: libm.so.6 lacks pow / exp / sin / cos / sincos");
    return -ENOSYS;
  }
  for (uint64_t i = 0; i < n; ++i) {
    const double xi = x[i];
    double o0 = 0.0, o1 = 0.0;
    uint8_t p = 0;
    switch (fn) {
      case grt::GLIBC_FN_POW:
        if (!libm_only && g::pow_fast(xi, y[i], &o0)) p = 1;
        else o0 = m.pow(xi, y[i]);
        break;
      case grt::GLIBC_FN_SIN:
        if (!libm_only && g::sin_fast(xi, &o0)) p = 1;
        else o0 = m.sin(xi);
        break;
      case grt::GLIBC_FN_COS:
        if (!libm_only && g::cos_fast(xi, &o0)) p = 1;
        else o0 = m.cos(xi);
        break;
      case grt::GLIBC_FN_SINCOS:
        if (!libm_only && g::sincos_fast(xi, &o0, &o1)) p = 1;
        else m.sincos(xi, &o0, &o1);
        break;
      case grt::GLIBC_FN_VDISC_SINCOS:
        if (!libm_only && g::sincos_fast_uniform(xi, &o0, &o1)) p = 1;
        else m.sincos(xi, &o0, &o1);
        break;
      case grt::GLIBC_FN_EXP:
        if (!libm_only) {
          o0 = g::exp_(xi);
          p = 1;
        } else {
          o0 = m.exp(xi);
        }
        break;
      default:  // GLIBC_FN_SINCOS_B
        if (libm_only) {
          m.sincos(xi, &o0, &o1);
        } else if (g::sincos_b_table_ok(xi)) {
          g::sincos_b_table(xi, &o0, &o1);
          p = 1;
        } else if (g::sincos_b_taylor_ok(xi)) {
          g::sincos_b_taylor(xi, &o0, &o1);
          p = 2;
        }
        break;
    }
    out0[i] = o0;
    out1[i] = o1;
    path[i] = p;
  }
  return 0;
}
