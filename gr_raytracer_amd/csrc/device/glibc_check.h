// glibc_check.h — what the glibc test hooks evaluate (grt_debug_glibc_device in api.hip,
// grt_debug_glibc_host in host/glibc_check.cpp; tests/glibc_inputs.py carries the same
// numbers).  Per lane i the hooks write out0[i], out1[i] (the cosine of the sincos forms,
// else 0) and path[i]: 0 the wrapper fell back to the platform's libm (OCML on the device)
// or the region-B form did not claim x, 1 glibc_math.h's fast / table path, 2 region B's
// Taylor path.
#pragma once

namespace grt {

enum GlibcCheckFn {
  GLIBC_FN_POW = 0,           // rpow / opow: pow_fast, else pow          (x, y)
  GLIBC_FN_SIN = 1,           // rsin: sin_fast, else sin
  GLIBC_FN_COS = 2,           // rcos: cos_fast, else cos
  GLIBC_FN_SINCOS = 3,        // rsincos: sincos_fast, else sincos
  GLIBC_FN_VDISC_SINCOS = 4,  // volumetric.h vdisc_density: sincos_fast_uniform, else sincos
  GLIBC_FN_EXP = 5,           // glibc::exp_ (every lane on path 1)
  GLIBC_FN_SINCOS_B = 6,      // sincos_b_table where sincos_b_table_ok (1), sincos_b_taylor
                              // where sincos_b_taylor_ok (2), else unclaimed: (0, 0), path 0
  GLIBC_FN_COUNT = 7,
  // host hook only: fn | GLIBC_FN_LIBM is the host libm's own pow / sin / cos / sincos /
  // exp on every lane (path 0)
  GLIBC_FN_LIBM = 16,
};

}  // namespace grt
