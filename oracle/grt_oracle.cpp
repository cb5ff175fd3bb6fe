// grt_oracle.cpp — CPU restatement of mdreem/gr_raytracer's per-pixel hot path.
//
// TEST INFRASTRUCTURE ONLY.  This file is the parity checker for the HIP kernels in
// gr_raytracer_amd/csrc.  Only tests/, __graft_entry__.smoke() and bench.py's
// cpu_baseline leg may load it; the product never links or calls it.
//
// It restates, in the reference's own structure and floating-point evaluation order,
//   * rkf45 / rkf45_step                        src/rendering/runge_kutta.rs:86-182
//   * Integrator::integrate + should_stop       src/rendering/integrator.rs:78-268
//   * Scene::color_of_ray, get_uv_coordinates   src/rendering/scene.rs:114-231
//   * Objects::intersects, step_at_intersection src/scene_objects/objects.rs:27-120
//   * Disc / Sphere intersections + emitters    src/scene_objects/{disc,sphere}.rs
//   * VolumetricDisc (capture cylinder, Perlin fBm density, constant-step raymarch)
//                                               src/scene_objects/volumetric_disc.rs
//   * Schwarzschild / Kerr / KerrBL / Euclidean / EuclideanSpherical
//                                               src/geometry/*.rs (RHS, metrics, stops)
//   * redshift, textures, temperature lookup    src/rendering/{redshift,texture,temperature}.rs
//   * camera ray generation                     src/rendering/camera.rs:214-254
//   * frame driver + adaptive supersampling     src/rendering/raytracer.rs:91-458
// It keeps the reference's algorithm literally: the whole trajectory is stored
// (Vec<Step>) and the window pass runs after integration, every object is tested
// on every window, errors abort the pixel.
//
// Evaluation order follows Rust semantics (no FMA contraction, left-to-right +,
// powi(2)=x*x, powi(3)=x*(x*x)).  nalgebra 0.35.0 arithmetic is restated from its
// published source (NOT vendored here): 4x4 matrix*vector and matrix*matrix
// accumulate column by column (gemv/axcpy: y = A[:,k]*x[k] + y, k = 0..3), Vector3
// dot = a + b + c, and the 8-vector norm uses the 8-accumulator unrolled dot
// ((a0+a4) + (a1+a5)) + (a2+a6) + (a3+a7).  libm is glibc (the same libm the Rust
// x86_64-unknown-linux-gnu build calls).  Parity of transcendental functions at the
// ulp level against the Rust binary is unpinned: no reference test fixes them.
//
// Build: oracle/Makefile (g++ -O2 -ffp-contract=off -fopenmp).

#include <cerrno>
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../include/grt_api.h"

namespace oracle {

static const double PI = 3.14159265358979323846;
static const double FRAC_PI_2 = 1.57079632679489661923;

// ---------------------------------------------------------------- basic types ----
enum class CS { Cartesian, Spherical, BoyerLindquist };

struct Point {  // geometry/point.rs:36-40
  CS cs;
  double a;  // BL spin (only meaningful for BoyerLindquist)
  double v[4];
  double operator[](int i) const { return v[i]; }
};
struct FourVector {  // geometry/four_vector.rs:5-9
  CS cs;
  double v[4];
  double operator[](int i) const { return v[i]; }
};
struct Vec3 {
  double x, y, z;
};
using Vec8 = double[8];
struct Mat4 {
  double m[4][4];
};

struct XYZA {  // color.rs:23-29 CIETristimulus
  double x, y, z, alpha;
};

enum Err {
  OK = GRT_OK,
  MaxStepsReached = GRT_ERR_MAX_STEPS_REACHED,
  NoCircularOrbitPossible = GRT_ERR_NO_CIRCULAR_ORBIT,
  BelowRISCO = GRT_ERR_BELOW_RISCO,
  NonFiniteRadius = GRT_ERR_NON_FINITE_RADIUS,
};

static inline double rust_clamp(double v, double lo, double hi) {  // f64::clamp
  if (v < lo) v = lo;
  if (v > hi) v = hi;
  return v;
}
static inline double rem_euclid(double x, double m) {  // f64::rem_euclid
  double r = std::fmod(x, m);
  return r < 0.0 ? r + std::fabs(m) : r;
}
static inline uint64_t sat_u64(double v) {  // `as usize` / `as u32` saturating cast
  if (!(v > 0.0)) return 0;                 // NaN and negatives -> 0
  if (v >= 18446744073709551616.0) return UINT64_MAX;
  return (uint64_t)v;
}
static inline uint32_t sat_u32(double v) {
  if (!(v > 0.0)) return 0;
  if (v >= 4294967296.0) return UINT32_MAX;
  return (uint32_t)v;
}
static inline double dot3(const Vec3& a, const Vec3& b) {  // nalgebra U3 dot: a + b + c
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
static inline double norm3(const Vec3& a) { return std::sqrt(dot3(a, a)); }

// nalgebra gemv: y_i = A_i0 x_0; y_i = A_ik x_k + y_i
static inline void mat_vec(const Mat4& A, const double* x, double* y) {
  for (int i = 0; i < 4; ++i) {
    double s = A.m[i][0] * x[0];
    for (int k = 1; k < 4; ++k) s = A.m[i][k] * x[k] + s;
    y[i] = s;
  }
}
// nalgebra gemm = gemv per column of B
static inline Mat4 mat_mul(const Mat4& A, const Mat4& B) {
  Mat4 C;
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < 4; ++i) {
      double s = A.m[i][0] * B.m[0][j];
      for (int k = 1; k < 4; ++k) s = A.m[i][k] * B.m[k][j] + s;
      C.m[i][j] = s;
    }
  return C;
}
// (v^T * M) * w, both products as nalgebra gemm/gemv
static inline double quad_form(const double* v, const Mat4& M, const double* w) {
  double row[4];
  for (int j = 0; j < 4; ++j) {
    double s = v[0] * M.m[0][j];
    for (int k = 1; k < 4; ++k) s = v[k] * M.m[k][j] + s;
    row[j] = s;
  }
  double s = row[0] * w[0];
  for (int j = 1; j < 4; ++j) s = row[j] * w[j] + s;
  return s;
}

// ------------------------------------------------------ chart conversions ----
// Sensitivity probes (tests only).  Bit mask: 1 = controller pow() one ulp up,
// 2 = one ulp down, 4 = the RHS's sin() one ulp up and cos() one ulp down, 8 / 16 =
// shading angles one ulp up / down (see shade_angle), 32 / 64 = the VolumetricDisc's two
// in-plane angles (compute_density and get_uv) one ulp up / down (see vdisc_angle).  Used to
// measure how strongly a last-ulp libm difference propagates on a scene; a pixel that
// moves under any probe is "libm-sensitive" (tests/test_gpu_parity.py).
static int g_libm_probe = 0;
static inline double controller_pow(double x, double e) {
  double p = std::pow(x, e);
  if (g_libm_probe & 1) return std::nextafter(p, INFINITY);
  if (g_libm_probe & 2) return std::nextafter(p, -INFINITY);
  return p;
}
// Which glibc entry point each site calls, as the reference's compiled code does:
// LLVM fuses f64::sin and f64::cos of one operand in one function into a single
// sincos() libcall, and glibc 2.35's sincos is the baseline (non-FMA) build while
// sin / cos / pow are the ifunc'd FMA builds -- their last bits differ.  The oracle
// spells the choice out (g_sincos / g_sin) and is compiled with -fno-builtin-sin
// -fno-builtin-cos -fno-builtin-sincos so GCC does not fuse on its own.
static inline void g_sincos(double x, double* s, double* c) { ::sincos(x, s, c); }
static inline double g_sin(double x) { return ::sin(x); }
static inline double g_cos(double x) { return ::cos(x); }
// the RHS's sin/cos pair, with probe bit 4 (sin one ulp up, cos one ulp down)
static inline void rhs_sincos(double x, double* s, double* c) {
  g_sincos(x, s, c);
  if (g_libm_probe & 4) {
    *s = std::nextafter(*s, INFINITY);
    *c = std::nextafter(*c, -INFINITY);
  }
}
// probe bits 8 / 16: shading angles (atan2 / acos of hit points and of the final
// direction, which feed texture coordinates) one ulp up / down
static inline double shade_angle(double v) {
  if (g_libm_probe & 8) return std::nextafter(v, INFINITY);
  if (g_libm_probe & 16) return std::nextafter(v, -INFINITY);
  return v;
}

// probe bits 32 / 64: the VolumetricDisc's in-plane angle (atan2 in compute_density and in
// get_uv, which feeds the noise coordinates and the texture coordinates) one ulp up / down
static inline double vdisc_angle(double v) {
  if (g_libm_probe & 32) return std::nextafter(v, INFINITY);
  if (g_libm_probe & 64) return std::nextafter(v, -INFINITY);
  return v;
}

// spherical_coordinates_helper.rs:5-26
static Point cartesian_to_spherical(const Point& c) {
  double t = c[0], x = c[1], y = c[2], z = c[3];
  double r = std::sqrt(x * x + y * y + z * z);
  if (r == 0.0) return Point{CS::Spherical, 0.0, {t, 0.0, 0.0, 0.0}};
  double theta = shade_angle(std::acos(z / r));
  double phi = shade_angle(std::atan2(y, x));
  return Point{CS::Spherical, 0.0, {t, r, theta, phi}};
}
// :28-39
static Point spherical_to_cartesian(const Point& s) {
  double t = s[0], r = s[1], theta = s[2], phi = s[3];
  double st, ct, sp, cp;
  g_sincos(theta, &st, &ct);
  g_sincos(phi, &sp, &cp);
  double x = r * st * cp;
  double y = r * st * sp;
  double z = r * ct;
  return Point{CS::Cartesian, 0.0, {t, x, y, z}};
}
// :44-61
static Point cartesian_to_boyer_lindquist(double a, const Point& c) {
  double t = c[0], x = c[1], y = c[2], z = c[3];
  double rho_sqr = x * x + y * y + z * z;
  double d = rho_sqr - a * a;
  double r_sqr = 0.5 * (rho_sqr - a * a + std::sqrt(d * d + 4.0 * a * a * z * z));
  double r = std::sqrt(r_sqr);
  double theta = (r == 0.0) ? 0.0 : shade_angle(std::acos(rust_clamp(z / r, -1.0, 1.0)));
  double phi = shade_angle(std::atan2(r * y - a * x, r * x + a * y));
  return Point{CS::BoyerLindquist, a, {t, r, theta, phi}};
}
// point.rs:139-154
static Point to_cartesian(const Point& p) {
  switch (p.cs) {
    case CS::Cartesian:
      return p;
    case CS::Spherical:
      return spherical_to_cartesian(p);
    case CS::BoyerLindquist: {
      double a = p.a, t = p[0], r = p[1], theta = p[2], phi = p[3];
      double st, ct, sp, cp;
      g_sincos(theta, &st, &ct);
      g_sincos(phi, &sp, &cp);
      double x = (r * cp - a * sp) * st;
      double y = (r * sp + a * cp) * st;
      double z = r * ct;
      return Point{CS::Cartesian, 0.0, {t, x, y, z}};
    }
  }
  return p;
}
// point.rs:125-137
static Vec3 spatial_cartesian(const Point& p) {
  Point c = to_cartesian(p);
  return Vec3{c[1], c[2], c[3]};
}
// point.rs:160-169
static Point to_coordinate_system(const Point& p, CS target, double a) {
  if (p.cs == target && (target != CS::BoyerLindquist || p.a == a)) return p;
  switch (target) {
    case CS::Cartesian:
      return to_cartesian(p);
    case CS::Spherical:
      return cartesian_to_spherical(to_cartesian(p));
    case CS::BoyerLindquist:
      return cartesian_to_boyer_lindquist(a, to_cartesian(p));
  }
  return p;
}
// point.rs:79-86 + :172-188
static Vec3 get_as_spherical(const Point& p) {
  if (p.cs == CS::Cartesian) {
    Point s = cartesian_to_spherical(p);
    return Vec3{s[1], s[2], s[3]};
  }
  return Vec3{p[1], rem_euclid(p[2], PI), rem_euclid(p[3] + PI, 2.0 * PI) - PI};
}
// point.rs:190-200
static double radial_distance_spatial_part_squared(const Point& p) {
  if (p.cs == CS::Cartesian) return p[1] * p[1] + p[2] * p[2] + p[3] * p[3];
  return p[1] * p[1];
}

// ------------------------------------------------------------ circular orbits ----
struct Killing {
  double u_t, u_phi;
};
// circular_orbit.rs:76-80
static double angular_velocity(double r_s, double a, double r) {
  double m = 0.5 * r_s;
  double sqrt_m = std::sqrt(m);
  return sqrt_m / (std::pow(r, 1.5) + a * sqrt_m);
}
// circular_orbit.rs:39-51 at theta = pi/2
static void metric_components_eq(double r_s, double a, double r, double* g_tt, double* g_tphi,
                                 double* g_phiphi) {
  double c = std::cos(FRAC_PI_2), s = std::sin(FRAC_PI_2);
  double sig = r * r + a * a * (c * c);
  double sin2 = s * s;
  *g_tt = -(1.0 - r_s * r / sig);
  *g_tphi = -a * r_s * r * sin2 / sig;
  *g_phiphi = (r * r + a * a + a * a * r_s * r * sin2 / sig) * sin2;
}
// circular_orbit.rs:84-108
static Err killing_coefficients(double r_s, double a, double r, Killing* out) {
  double omega = angular_velocity(r_s, a, r);
  double g_tt, g_tphi, g_phiphi;
  metric_components_eq(r_s, a, r, &g_tt, &g_tphi, &g_phiphi);
  double ut_pre = g_tt + 2.0 * omega * g_tphi + omega * omega * g_phiphi;
  if (ut_pre >= 0.0) return NoCircularOrbitPossible;
  double u_t = 1.0 / std::sqrt(-ut_pre);
  out->u_t = u_t;
  out->u_phi = omega * u_t;
  return OK;
}

// ------------------------------------------------------------------ geometry ----
struct Ray {  // rendering/ray.rs:16-23
  int64_t row, col;
  Point position;
  FourVector momentum;
};


struct GeodesicSolver {  // geometry.rs:15-32
  virtual ~GeodesicSolver() {}
  virtual void apply(const double* y, double* out) const = 0;
  virtual void create_initial_state(const Ray& ray, double* y) const {
    for (int i = 0; i < 4; ++i) y[i] = ray.position[i];
    for (int i = 0; i < 4; ++i) y[4 + i] = ray.momentum[i];
  }
  virtual FourVector momentum_from_state(const double* y) const = 0;
};

struct Geometry {  // geometry.rs:108-121 + SupportQuantities :49-81
  double radius = 0, a = 0, horizon_epsilon = 0;
  virtual ~Geometry() {}
  virtual CS cs() const = 0;
  virtual double signature0() const = 0;
  virtual double inner_product(const Point& p, const FourVector& v, const FourVector& w) const = 0;
  virtual bool inside_horizon(const Point& p) const = 0;
  virtual bool closed_orbit(const Point& p, uint64_t step, uint64_t max_steps) const = 0;
  virtual std::unique_ptr<GeodesicSolver> solver(const Ray& ray) const = 0;
  virtual double radial_coordinate(const Point& p) const = 0;
  virtual FourVector stationary_velocity(const Point& p) const = 0;
  virtual Err circular_orbit_velocity(const Point& p, FourVector* out) const = 0;
  // get_constants_of_motion (geometry.rs:119-120): E, L_z (+ Q); returns the count
  virtual int constants_of_motion(const Point& p, const FourVector& m, double* c) const = 0;
  Point make_point(const double* y) const { return Point{cs(), a, {y[0], y[1], y[2], y[3]}}; }
};

// ---- Euclidean (geometry/euclidean.rs) ----
struct EuclideanSolver : GeodesicSolver {
  void apply(const double* y, double* o) const override {  // :47-53
    o[0] = y[4]; o[1] = y[5]; o[2] = y[6]; o[3] = y[7];
    o[4] = 0.0; o[5] = 0.0; o[6] = 0.0; o[7] = 0.0;
  }
  FourVector momentum_from_state(const double* y) const override {
    return FourVector{CS::Cartesian, {y[4], y[5], y[6], y[7]}};
  }
};
struct Euclidean : Geometry {
  CS cs() const override { return CS::Cartesian; }
  double signature0() const override { return 1.0; }
  double inner_product(const Point&, const FourVector& v, const FourVector& w) const override {
    return 1.0 * v[0] * w[0] + -v[1] * w[1] + -v[2] * w[2] + -v[3] * w[3];  // :62-67
  }
  bool inside_horizon(const Point&) const override { return false; }
  bool closed_orbit(const Point&, uint64_t, uint64_t) const override { return false; }
  std::unique_ptr<GeodesicSolver> solver(const Ray&) const override {
    return std::unique_ptr<GeodesicSolver>(new EuclideanSolver());
  }
  double radial_coordinate(const Point& p) const override { return get_as_spherical(p).x; }
  FourVector stationary_velocity(const Point&) const override {
    return FourVector{CS::Cartesian, {1.0, 0.0, 0.0, 0.0}};
  }
  Err circular_orbit_velocity(const Point&, FourVector* out) const override {
    *out = FourVector{CS::Cartesian, {1.0, 0.0, 0.0, 0.0}};
    return OK;
  }
  int constants_of_motion(const Point& p, const FourVector& m, double* c) const override {  // :160-182
    double p_x = -m[1], p_y = -m[2];
    c[0] = m[0];
    c[1] = p[1] * p_y - p[2] * p_x;
    return 2;
  }
};

// ---- Schwarzschild (geometry/schwarzschild.rs) ----
struct SchwarzschildSolver : GeodesicSolver {
  double radius;
  explicit SchwarzschildSolver(double r) : radius(r) {}
  void apply(const double* y, double* o) const override {  // :54-80
    double r = y[1], theta = y[2];
    double v_t = y[4], v_r = y[5], v_theta = y[6], v_phi = y[7];
    double st, ct;
    rhs_sincos(theta, &st, &ct);
    double a = 1.0 - radius / r;
    double a_prime = radius / (r * r);
    double aprime_over_a = a_prime / a;
    double a_t = -(aprime_over_a)*v_t * v_r;
    double a_r = -0.5 * a * a_prime * v_t * v_t + 0.5 * (aprime_over_a)*v_r * v_r +
                 a * r * (v_theta * v_theta + v_phi * v_phi * st * st);
    double a_theta = -(2.0 / r) * v_r * v_theta + st * ct * v_phi * v_phi;
    double a_phi =
        -(2.0 / r) * v_phi * v_r - 2.0 * ct / st * v_theta * v_phi;
    o[0] = v_t; o[1] = v_r; o[2] = v_theta; o[3] = v_phi;
    o[4] = a_t; o[5] = a_r; o[6] = a_theta; o[7] = a_phi;
  }
  FourVector momentum_from_state(const double* y) const override {
    return FourVector{CS::Spherical, {y[4], y[5], y[6], y[7]}};
  }
};
struct Schwarzschild : Geometry {
  CS cs() const override { return CS::Spherical; }
  double signature0() const override { return 1.0; }
  double inner_product(const Point& p, const FourVector& v, const FourVector& w) const override {
    double r = p[1], theta = p[2];  // :90-102
    double a = 1.0 - radius / r;
    return a * v[0] * w[0] - v[1] * w[1] / a - r * r * v[2] * w[2] -
           r * r * g_sin(theta) * g_sin(theta) * v[3] * w[3];
  }
  bool inside_horizon(const Point& p) const override {  // :181-183
    return p[1] <= radius + horizon_epsilon;
  }
  bool closed_orbit(const Point& p, uint64_t i, uint64_t max_steps) const override {
    return i == max_steps - 1 && p[1] < 5.0 * radius;  // :185-193
  }
  std::unique_ptr<GeodesicSolver> solver(const Ray&) const override {
    return std::unique_ptr<GeodesicSolver>(new SchwarzschildSolver(radius));
  }
  double radial_coordinate(const Point& p) const override {  // :201-211
    if (p.cs == CS::Cartesian) return get_as_spherical(p).x;
    return p[1];
  }
  FourVector stationary_velocity(const Point& p) const override {  // :237-240
    double a = 1.0 - radius / p[1];
    return FourVector{CS::Spherical, {1.0 / std::sqrt(a), 0.0, 0.0, 0.0}};
  }
  Err circular_orbit_velocity(const Point& p, FourVector* out) const override {  // :248-254
    Killing c;
    Err e = killing_coefficients(radius, 0.0, radial_coordinate(p), &c);
    if (e != OK) return e;
    *out = FourVector{CS::Spherical, {c.u_t, 0.0, 0.0, c.u_phi}};
    return OK;
  }
  int constants_of_motion(const Point& p, const FourVector& m, double* c) const override {  // :213-233
    double r = p[1], theta = p[2];  // a lone sin in this function
    double a = 1.0 - radius / r;
    c[0] = a * m[0];
    c[1] = -r * r * g_sin(theta) * g_sin(theta) * m[3];
    return 2;
  }
};

// ---- EuclideanSpherical: flat space in the spherical chart (geometry/euclidean_spherical.rs) ----
struct EuclideanSphericalSolver : GeodesicSolver {
  void apply(const double* y, double* o) const override {  // :48-70
    double r = y[1], theta = y[2];
    double v_t = y[4], v_r = y[5], v_theta = y[6], v_phi = y[7];
    double st, ct;
    rhs_sincos(theta, &st, &ct);
    double a_t = 0.0;
    double a_r = r * (v_theta * v_theta + v_phi * v_phi * st * st);
    double a_theta = -(2.0 / r) * v_r * v_theta + st * ct * v_phi * v_phi;
    double a_phi = -(2.0 / r) * v_phi * v_r - 2.0 * ct / st * v_theta * v_phi;
    o[0] = v_t; o[1] = v_r; o[2] = v_theta; o[3] = v_phi;
    o[4] = a_t; o[5] = a_r; o[6] = a_theta; o[7] = a_phi;
  }
  FourVector momentum_from_state(const double* y) const override {
    return FourVector{CS::Spherical, {y[4], y[5], y[6], y[7]}};
  }
};
struct EuclideanSpherical : Geometry {
  CS cs() const override { return CS::Spherical; }
  double signature0() const override { return 1.0; }
  double inner_product(const Point& p, const FourVector& v, const FourVector& w) const override {
    double r = p[1], theta = p[2];  // :80-91
    return 1.0 * v[0] * w[0] - v[1] * w[1] - r * r * v[2] * w[2] -
           r * r * g_sin(theta) * g_sin(theta) * v[3] * w[3];
  }
  bool inside_horizon(const Point&) const override { return false; }                  // :124-126
  bool closed_orbit(const Point&, uint64_t, uint64_t) const override { return false; }  // :128-130
  std::unique_ptr<GeodesicSolver> solver(const Ray&) const override {
    return std::unique_ptr<GeodesicSolver>(new EuclideanSphericalSolver());
  }
  double radial_coordinate(const Point& p) const override {  // :136-146
    if (p.cs == CS::Cartesian) return get_as_spherical(p).x;
    return p[1];
  }
  FourVector stationary_velocity(const Point&) const override {  // :168-170
    return FourVector{CS::Spherical, {1.0, 0.0, 0.0, 0.0}};
  }
  Err circular_orbit_velocity(const Point&, FourVector* out) const override {  // :177-183
    *out = FourVector{CS::Spherical, {1.0, 0.0, 0.0, 0.0}};
    return OK;
  }
  int constants_of_motion(const Point& p, const FourVector& m, double* c) const override {  // :147-166
    double r = p[1], theta = p[2];
    c[0] = m[0];
    c[1] = -r * r * g_sin(theta) * g_sin(theta) * m[3];
    return 2;
  }
};

// ---- Kerr, Kerr-Schild Cartesian chart (geometry/kerr.rs) ----
static double ks_r_sqr(double a, double x, double y, double z) {  // :31-34
  double rho_sqr = x * x + y * y + z * z;
  return 0.5 * (rho_sqr - a * a + std::sqrt((rho_sqr - a * a) * (rho_sqr - a * a) + 4.0 * a * a * z * z));
}
static void k_covector(double a, double x, double y, double z, double* k) {  // :36-46
  double r_sqr = ks_r_sqr(a, x, y, z);
  double r = std::sqrt(r_sqr);
  k[0] = 1.0;
  k[1] = (r * x + a * y) / (r_sqr + a * a);
  k[2] = (r * y - a * x) / (r_sqr + a * a);
  k[3] = z / r;
}
static Mat4 ks_metric(double radius, double a, double x, double y, double z) {  // :49-84
  double r_sqr = ks_r_sqr(a, x, y, z);
  double r = std::sqrt(r_sqr);
  double f = (r * r * r * radius) / (r * r * r * r + a * a * z * z);
  double k[4];
  k_covector(a, x, y, z, k);
  double k_0 = k[0], k_x = k[1], k_y = k[2], k_z = k[3];
  Mat4 g;
  g.m[0][0] = k_0 * k_0 * f - 1.0;
  g.m[0][1] = k_0 * k_x * f;
  g.m[0][2] = k_0 * k_y * f;
  g.m[0][3] = k_0 * k_z * f;
  g.m[1][0] = g.m[0][1];
  g.m[1][1] = k_x * k_x * f + 1.0;
  g.m[1][2] = k_x * k_y * f;
  g.m[1][3] = k_x * k_z * f;
  g.m[2][0] = g.m[0][2];
  g.m[2][1] = g.m[1][2];
  g.m[2][2] = k_y * k_y * f + 1.0;
  g.m[2][3] = k_y * k_z * f;
  g.m[3][0] = g.m[0][3];
  g.m[3][1] = g.m[1][3];
  g.m[3][2] = g.m[2][3];
  g.m[3][3] = k_z * k_z * f + 1.0;
  return g;
}
static Mat4 ks_metric_contravariant(double radius, double a, double x, double y, double z) {
  double r_sqr = ks_r_sqr(a, x, y, z);  // :88-110
  double r = std::sqrt(r_sqr);
  double f = (r * r * r * radius) / (r * r * r * r + a * a * z * z);
  double k[4];
  k_covector(a, x, y, z, k);
  double kc[4] = {-k[0], k[1], k[2], k[3]};
  Mat4 g;
  std::memset(&g, 0, sizeof(g));
  g.m[0][0] = -1.0;
  g.m[1][1] = 1.0;
  g.m[2][2] = 1.0;
  g.m[3][3] = 1.0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) g.m[i][j] -= f * kc[i] * kc[j];
  return g;
}
struct KerrSolver : GeodesicSolver {
  double radius, a;
  KerrSolver(double r, double a_) : radius(r), a(a_) {}
  Mat4 d_covariant(int index, double x, double y, double z) const {  // :162-186
    double base = 1e-10;
    double h = base * (index == 1 ? std::fmax(std::fabs(x), 1.0)
                                  : index == 2 ? std::fmax(std::fabs(y), 1.0)
                                               : std::fmax(std::fabs(z), 1.0));
    double dx = index == 1 ? h : 0.0, dy = index == 2 ? h : 0.0, dz = index == 3 ? h : 0.0;
    Mat4 mp = ks_metric(radius, a, x + dx, y + dy, z + dz);
    Mat4 mm = ks_metric(radius, a, x - dx, y - dy, z - dz);
    Mat4 d;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) d.m[i][j] = (mp.m[i][j] - mm.m[i][j]) / (2.0 * h);
    return d;
  }
  Mat4 d_contravariant(int index, double x, double y, double z, const Mat4& gc) const {
    Mat4 d = d_covariant(index, x, y, z);  // :149-159
    Mat4 t = mat_mul(mat_mul(gc, d), gc);
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) t.m[i][j] = -t.m[i][j];
    return t;
  }
  void apply(const double* ys, double* o) const override {  // :200-241
    double x = ys[1], y = ys[2], z = ys[3];
    double p[4] = {ys[4], ys[5], ys[6], ys[7]};
    Mat4 gc = ks_metric_contravariant(radius, a, x, y, z);
    double xdot[4];
    mat_vec(gc, p, xdot);
    Mat4 dx = d_contravariant(1, x, y, z, gc);
    Mat4 dy = d_contravariant(2, x, y, z, gc);
    Mat4 dz = d_contravariant(3, x, y, z, gc);
    o[0] = xdot[0]; o[1] = xdot[1]; o[2] = xdot[2]; o[3] = xdot[3];
    o[4] = 0.0;
    o[5] = -0.5 * quad_form(p, dx, p);
    o[6] = -0.5 * quad_form(p, dy, p);
    o[7] = -0.5 * quad_form(p, dz, p);
  }
  void create_initial_state(const Ray& ray, double* y) const override {  // :243-260
    Mat4 g = ks_metric(radius, a, ray.position[1], ray.position[2], ray.position[3]);
    double pc[4];
    mat_vec(g, ray.momentum.v, pc);
    for (int i = 0; i < 4; ++i) y[i] = ray.position[i];
    for (int i = 0; i < 4; ++i) y[4 + i] = pc[i];
  }
  FourVector momentum_from_state(const double* y) const override {  // :262-273
    Mat4 gc = ks_metric_contravariant(radius, a, y[1], y[2], y[3]);
    FourVector f{CS::Cartesian, {0, 0, 0, 0}};
    mat_vec(gc, y + 4, f.v);
    return f;
  }
};
struct Kerr : Geometry {
  CS cs() const override { return CS::Cartesian; }
  double signature0() const override { return -1.0; }
  double inner_product(const Point& p, const FourVector& v, const FourVector& w) const override {
    Mat4 g = ks_metric(radius, a, p[1], p[2], p[3]);  // :283-287
    return quad_form(v.v, g, w.v);
  }
  bool inside_horizon(const Point& p) const override {  // :382-394
    if (std::fabs(a) > radius / 2.0) return false;
    double r = std::sqrt(ks_r_sqr(a, p[1], p[2], p[3]));
    double m = 0.5 * radius;
    double disc = std::fmax(m * m - a * a, 0.0);
    double rp = m + std::sqrt(disc);
    return r <= rp + horizon_epsilon;
  }
  bool closed_orbit(const Point& p, uint64_t i, uint64_t max_steps) const override {
    double r = radial_coordinate(p);  // :396-407
    return i == max_steps - 1 && r < 5.0 * radius;
  }
  std::unique_ptr<GeodesicSolver> solver(const Ray&) const override {
    return std::unique_ptr<GeodesicSolver>(new KerrSolver(radius, a));
  }
  double radial_coordinate(const Point& p) const override {  // :416-419
    return std::sqrt(ks_r_sqr(a, p[1], p[2], p[3]));
  }
  FourVector stationary_velocity(const Point& p) const override {  // :449-455
    double x = p[1], y = p[2], z = p[3];
    (void)x; (void)y;
    double r_sqr = ks_r_sqr(a, p[1], p[2], p[3]);
    double r = std::sqrt(r_sqr);
    double f = (r * r * r * radius) / (r * r * r * r + a * a * z * z);
    return FourVector{CS::Cartesian, {1.0 / std::sqrt(1.0 - f), 0.0, 0.0, 0.0}};
  }
  Err circular_orbit_velocity(const Point& p, FourVector* out) const override {  // :473-480
    Killing c;
    Err e = killing_coefficients(radius, a, radial_coordinate(p), &c);
    if (e != OK) return e;
    double ax[4] = {0.0, -p[2], p[1], 0.0};  // axial_killing_vector :482-485
    double et[4] = {1.0, 0.0, 0.0, 0.0};
    FourVector u{CS::Cartesian, {0, 0, 0, 0}};
    for (int i = 0; i < 4; ++i) u.v[i] = c.u_t * et[i] + c.u_phi * ax[i];
    *out = u;
    return OK;
  }
  int constants_of_motion(const Point& p, const FourVector& m, double* c) const override {  // :421-445
    Mat4 g = ks_metric(radius, a, p[1], p[2], p[3]);
    double pc[4];
    mat_vec(g, m.v, pc);  // nalgebra Matrix4 * Vector4
    c[0] = -pc[0];
    c[1] = -p[2] * pc[1] + p[1] * pc[2];
    return 2;
  }
};

// ---- KerrBL, Boyer-Lindquist with Carter constant (geometry/kerr_bl.rs) ----
static double bl_sigma(double r, double a, double cos_t) {  // :62-64 (cos theta passed in)
  return r * r + a * a * (cos_t * cos_t);
}
static double bl_delta(double r, double r_s, double a) { return r * r - r_s * r + a * a; }
static Mat4 metric_bl(double r_s, double a, double r, double theta) {  // :253-272
  double sin_t, cos_t;  // sigma's cos and this sin of one theta: one sincos
  g_sincos(theta, &sin_t, &cos_t);
  double sig = bl_sigma(r, a, cos_t);
  double sin2 = sin_t * sin_t;
  Mat4 g;
  std::memset(&g, 0, sizeof(g));
  g.m[0][0] = -(1.0 - r_s * r / sig);
  g.m[1][1] = sig / bl_delta(r, r_s, a);
  g.m[2][2] = sig;
  g.m[3][3] = (r * r + a * a + a * a * r_s * r * sin2 / sig) * sin2;
  double g_tph = -a * r_s * r * sin2 / sig;
  g.m[0][3] = g_tph;
  g.m[3][0] = g_tph;
  return g;
}
struct KerrBLSolver : GeodesicSolver {
  double radius, a, e, l_z, q;
  void apply(const double* y, double* o) const override {  // :141-174
    double r = y[1], theta = y[2], v_r = y[4], v_theta = y[5];
    double del = bl_delta(r, radius, a);
    double p_r = (r * r + a * a) * e - a * l_z;
    double sin_t, cos_t;  // geodesic + potential_theta_derivative: one sincos
    rhs_sincos(theta, &sin_t, &cos_t);
    double sin2 = sin_t * sin_t;
    double dt = (r * r + a * a) / del * p_r + a * (l_z - a * e * sin2);
    double dphi = a / del * p_r + l_z / sin2 - a * e;
    // potential_r_derivative :85-89
    double p_r2 = (r * r + a * a) * e - a * l_z;
    double le = l_z - a * e;
    double carter = le * le + q;
    double dv_r = (4.0 * r * e * p_r2 - (2.0 * r - radius) * carter) / 2.0;
    // potential_theta_derivative :114-118
    double sin_t2 = sin_t;
    double dv_theta = (-2.0 * a * a * e * e * cos_t * sin_t2 +
                       2.0 * l_z * l_z * cos_t / (sin_t2 * (sin_t2 * sin_t2))) /
                      2.0;
    o[0] = dt; o[1] = v_r; o[2] = v_theta; o[3] = dphi;
    o[4] = dv_r; o[5] = dv_theta; o[6] = 0.0; o[7] = 0.0;
  }
  void create_initial_state(const Ray& ray, double* y) const override {  // :176-223 (BL ray)
    double r = ray.position[1], theta = ray.position[2], phi = ray.position[3];
    double t = ray.position[0];
    double sign_r = ray.momentum[1] >= 0.0 ? 1.0 : -1.0;
    double sign_theta = ray.momentum[2] >= 0.0 ? 1.0 : -1.0;
    // potential_r :78-82
    double del = bl_delta(r, radius, a);
    double p_r = (r * r + a * a) * e - a * l_z;
    double le = l_z - a * e;
    double r_pot = p_r * p_r - del * (le * le + q);
    // potential_theta :101-105
    double cos_t, sin_t;
    g_sincos(theta, &sin_t, &cos_t);
    double th_pot = q + a * a * e * e * cos_t * cos_t - l_z * l_z * cos_t * cos_t / (sin_t * sin_t);
    y[0] = t; y[1] = r; y[2] = theta; y[3] = phi;
    y[4] = sign_r * std::sqrt(std::fmax(r_pot, 0.0));
    y[5] = sign_theta * std::sqrt(std::fmax(th_pot, 0.0));
    y[6] = 0.0; y[7] = 0.0;
  }
  FourVector momentum_from_state(const double* y) const override {  // :225-249
    double r = y[1], theta = y[2], v_r = y[4], v_theta = y[5];
    double del = bl_delta(r, radius, a);
    double s, c;  // sigma's cos and this sin: one sincos
    g_sincos(theta, &s, &c);
    double sig = bl_sigma(r, a, c);
    double sin2 = s * s;
    double p_r_term = (r * r + a * a) * e - a * l_z;
    double dt = (r * r + a * a) / del * p_r_term + a * (l_z - a * e * sin2);
    double dphi = a / del * p_r_term + l_z / sin2 - a * e;
    return FourVector{CS::BoyerLindquist, {dt / sig, v_r / sig, v_theta / sig, dphi / sig}};
  }
};
struct KerrBL : Geometry {
  CS cs() const override { return CS::BoyerLindquist; }
  double signature0() const override { return -1.0; }
  double inner_product(const Point& p, const FourVector& v, const FourVector& w) const override {
    Mat4 g = metric_bl(radius, a, p[1], p[2]);  // :338-359
    double result = 0.0;
    for (int mu = 0; mu < 4; ++mu)
      for (int nu = 0; nu < 4; ++nu) result += g.m[mu][nu] * v[mu] * w[nu];
    return result;
  }
  bool inside_horizon(const Point& p) const override {  // :482-492
    double m = radius / 2.0;
    if (std::fabs(a) > m) return false;
    double disc = std::fmax(m * m - a * a, 0.0);
    double r_plus = m + std::sqrt(disc);
    return p[1] <= r_plus + horizon_epsilon;
  }
  bool closed_orbit(const Point& p, uint64_t i, uint64_t max_steps) const override {
    return i == max_steps - 1 && p[1] < 5.0 * radius;  // :494-503
  }
  std::unique_ptr<GeodesicSolver> solver(const Ray& ray) const override {  // :505-577 BL branch
    double r = ray.position[1], theta = ray.position[2];
    Mat4 g = metric_bl(radius, a, r, theta);
    double pc[4];
    mat_vec(g, ray.momentum.v, pc);
    double e = -pc[0], l_z = pc[3], p_theta = pc[2];
    double cos_t, sin_t;
    g_sincos(theta, &sin_t, &cos_t);
    double sin2 = sin_t * sin_t;
    double q = p_theta * p_theta + cos_t * cos_t * (l_z * l_z / std::fmax(sin2, 1e-28) - a * a * e * e);
    KerrBLSolver* s = new KerrBLSolver();
    s->radius = radius; s->a = a; s->e = e; s->l_z = l_z; s->q = q;
    return std::unique_ptr<GeodesicSolver>(s);
  }
  double radial_coordinate(const Point& p) const override {  // :579-594
    if (p.cs == CS::BoyerLindquist) return p[1];
    double x = p[1], y = p[2], z = p[3];
    double rho_sqr = x * x + y * y + z * z;
    double d = rho_sqr - a * a;
    return std::sqrt(0.5 * (rho_sqr - a * a + std::sqrt(d * d + 4.0 * a * a * z * z)));
  }
  FourVector stationary_velocity(const Point& p) const override {  // :362-371
    double r = p[1], theta = p[2];
    double sig = bl_sigma(r, a, g_cos(theta));  // sigma alone: a lone cos()
    double ut = 1.0 / std::sqrt(1.0 - radius * r / sig);
    return FourVector{CS::BoyerLindquist, {ut, 0.0, 0.0, 0.0}};
  }
  Err circular_orbit_velocity(const Point& p, FourVector* out) const override {  // :384-392
    Killing c;
    Err e = killing_coefficients(radius, a, radial_coordinate(p), &c);
    if (e != OK) return e;
    *out = FourVector{CS::BoyerLindquist, {c.u_t, 0.0, 0.0, c.u_phi}};
    return OK;
  }
  int constants_of_motion(const Point& p, const FourVector& m, double* c) const override {  // :596-625
    double r = p[1], theta = p[2];
    Mat4 g = metric_bl(radius, a, r, theta);
    double pc[4];
    mat_vec(g, m.v, pc);
    double e = -pc[0], l_z = pc[3], p_theta_cov = pc[2];
    double sin_t, cos_t;  // theta.cos() and theta.sin() in one function: one sincos
    g_sincos(theta, &sin_t, &cos_t);
    double sin2 = sin_t * sin_t;  // powi(2)
    c[0] = e;
    c[1] = l_z;
    c[2] = p_theta_cov * p_theta_cov + cos_t * cos_t * (l_z * l_z / std::fmax(sin2, 1e-28) - a * a * e * e);
    return 3;
  }
};

// --------------------------------------------------------------- RKF45 ---------
// runge_kutta.rs:16-84
static const double B21 = 2.0 / 9.0;
static const double B31 = 1.0 / 12.0, B32 = 1.0 / 4.0;
static const double B41 = 69.0 / 128.0, B42 = -243.0 / 128.0, B43 = 135.0 / 64.0;
static const double B51 = -17.0 / 12.0, B52 = 27.0 / 4.0, B53 = -27.0 / 5.0, B54 = 16.0 / 15.0;
static const double B61 = 65.0 / 432.0, B62 = -5.0 / 16.0, B63 = 13.0 / 16.0, B64 = 4.0 / 27.0,
                    B65 = 5.0 / 144.0;
static const double CH1 = 47.0 / 450.0, CH2 = 0.0, CH3 = 12.0 / 25.0, CH4 = 32.0 / 225.0,
                    CH5 = 1.0 / 30.0, CH6 = 6.0 / 25.0;
static const double CT1 = 1.0 / 150.0, CT2 = 0.0, CT3 = -3.0 / 100.0, CT4 = 16.0 / 75.0,
                    CT5 = 1.0 / 20.0, CT6 = -6.0 / 25.0;
static const double BETA = 0.9, CONVERGENCY_ORDER = 5.0, ERROR_RATIO_SMALL_ERROR = 1e-5;
static const int MAX_RETRY_STEP = 100;
static const double H_MAX = 1.0, H_MIN = 1e-12, H_GROWTH_CAP = 4.0;

template <int D, class F>
static double rkf45_step(const double* y, double h, const F& f, double* y_new) {  // :86-125
  double k1[D], k2[D], k3[D], k4[D], k5[D], k6[D], tmp[D], o[D];
  f(y, o);
  for (int i = 0; i < D; ++i) k1[i] = h * o[i];
  for (int i = 0; i < D; ++i) tmp[i] = y[i] + B21 * k1[i];
  f(tmp, o);
  for (int i = 0; i < D; ++i) k2[i] = h * o[i];
  for (int i = 0; i < D; ++i) tmp[i] = y[i] + B31 * k1[i] + B32 * k2[i];
  f(tmp, o);
  for (int i = 0; i < D; ++i) k3[i] = h * o[i];
  for (int i = 0; i < D; ++i) tmp[i] = y[i] + B41 * k1[i] + B42 * k2[i] + B43 * k3[i];
  f(tmp, o);
  for (int i = 0; i < D; ++i) k4[i] = h * o[i];
  for (int i = 0; i < D; ++i) tmp[i] = y[i] + B51 * k1[i] + B52 * k2[i] + B53 * k3[i] + B54 * k4[i];
  f(tmp, o);
  for (int i = 0; i < D; ++i) k5[i] = h * o[i];
  for (int i = 0; i < D; ++i)
    tmp[i] = y[i] + B61 * k1[i] + B62 * k2[i] + B63 * k3[i] + B64 * k4[i] + B65 * k5[i];
  f(tmp, o);
  for (int i = 0; i < D; ++i) k6[i] = h * o[i];
  double e[D];
  for (int i = 0; i < D; ++i) {
    y_new[i] = y[i] + CH1 * k1[i] + CH2 * k2[i] + CH3 * k3[i] + CH4 * k4[i] + CH5 * k5[i] + CH6 * k6[i];
    e[i] = CT1 * k1[i] + CT2 * k2[i] + CT3 * k3[i] + CT4 * k4[i] + CT5 * k5[i] + CT6 * k6[i];
  }
  // nalgebra norm(): 8-accumulator unrolled dot for D >= 8, sequential otherwise
  double res = 0.0;
  if (D == 8) {
    res += e[0] * e[0] + e[4] * e[4];
    res += e[1] * e[1] + e[5] * e[5];
    res += e[2] * e[2] + e[6] * e[6];
    res += e[3] * e[3] + e[7] * e[7];
  } else if (D == 2) {
    res = e[0] * e[0] + e[1] * e[1];
  } else {
    for (int i = 0; i < D; ++i) res += e[i] * e[i];
  }
  return std::sqrt(res);
}

struct StepResult {
  double h_taken, h_next;
  int attempts;
};
template <int D, class F>
static Err rkf45(const double* y, double h, double epsilon, const F& f, double* y_new,
                 StepResult* sr) {  // :138-182
  double h_cur = rust_clamp(h, H_MIN, H_MAX);
  sr->attempts = 0;
  for (int it = 0; it < MAX_RETRY_STEP; ++it) {
    double err = rkf45_step<D>(y, h_cur, f, y_new);
    sr->attempts++;
    double h_prop = err > 0.0 ? BETA * h_cur * controller_pow(epsilon / err, 1.0 / CONVERGENCY_ORDER)
                              : h_cur * H_GROWTH_CAP;
    h_prop = rust_clamp(std::fmin(h_prop, h_cur * H_GROWTH_CAP), H_MIN, H_MAX);
    if (err > epsilon) {
      if (h_cur <= H_MIN) {
        sr->h_taken = h_cur;
        sr->h_next = h_cur;
        return OK;
      }
      h_cur = rust_clamp(h_prop / 2.0, H_MIN, H_MAX);
    } else {
      sr->h_taken = h_cur;
      sr->h_next = (err / epsilon < ERROR_RATIO_SMALL_ERROR)
                       ? rust_clamp(h_cur * H_GROWTH_CAP, H_MIN, H_MAX)
                       : h_prop;
      return OK;
    }
  }
  return MaxStepsReached;
}

// ------------------------------------------------------------- integrator -------
struct Step {  // integrator.rs:14-19
  Point x;
  FourVector p;
  double t;
  uint64_t step;
};

struct IntegrationConfig {
  uint64_t max_steps;
  double max_radius_sq, step_size, epsilon;
};

// scene.rs:48-69
static Point get_position(const double* y, const Geometry& g) {
  return to_cartesian(g.make_point(y));
}

static int should_stop(const Geometry& g, const IntegrationConfig& cfg, const double* cur,
                       uint64_t i) {  // integrator.rs:203-268
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(cur[k])) return GRT_STOP_NAN;
  Point p = g.make_point(cur);
  if (g.inside_horizon(p)) return GRT_STOP_HORIZON;
  if (g.closed_orbit(p, i, cfg.max_steps)) return GRT_STOP_CLOSED_ORBIT;
  if (radial_distance_spatial_part_squared(get_position(cur, g)) > cfg.max_radius_sq)
    return GRT_STOP_CELESTIAL;
  for (int k = 4; k < 8; ++k)
    if (!std::isfinite(cur[k])) return GRT_STOP_NAN;
  return GRT_STOP_NONE;
}

struct Counters {
  uint64_t accepted = 0, attempts = 0, march_samples = 0;
};

// integrator.rs:78-174.  Returns the stop reason in *stop.
static Err integrate(const Geometry& g, const IntegrationConfig& cfg, const Ray& ray,
                     std::vector<Step>& result, int* stop, Counters* cnt) {
  double t = 0.0;
  std::unique_ptr<GeodesicSolver> solver = g.solver(ray);
  double y[8];
  solver->create_initial_state(ray, y);
  result.clear();
  result.reserve(1024);
  result.push_back(Step{g.make_point(y), solver->momentum_from_state(y), t, 0});
  double h = cfg.step_size;
  auto f = [&](const double* s, double* o) { solver->apply(s, o); };
  *stop = GRT_STOP_NONE;
  for (uint64_t i = 1; i < cfg.max_steps; ++i) {
    double y_new[8];
    StepResult sr;
    Err e = rkf45<8>(y, h, cfg.epsilon, f, y_new, &sr);
    cnt->attempts += sr.attempts;
    if (e != OK) return e;
    std::memcpy(y, y_new, sizeof(y));
    t += sr.h_taken;
    h = sr.h_next;
    cnt->accepted++;
    result.push_back(Step{g.make_point(y), solver->momentum_from_state(y), t, i});
    int s = should_stop(g, cfg, y, i);
    if (s != GRT_STOP_NONE) {
      *stop = s;
      return OK;
    }
  }
  return OK;
}

// ----------------------------------------------------------------- colours -------
static XYZA blend(const XYZA& self, const XYZA& other) {  // color.rs:49-69
  double ab = rust_clamp(self.alpha, 0.0, 1.0);
  double af = rust_clamp(other.alpha, 0.0, 1.0);
  double ao = af + ab * (1.0 - af);
  if (ao <= 0.0) return XYZA{0.0, 0.0, 0.0, 0.0};
  double x = (other.x * af + self.x * ab * (1.0 - af)) / ao;
  double y = (other.y * af + self.y * ab * (1.0 - af)) / ao;
  double z = (other.z * af + self.z * ab * (1.0 - af)) / ao;
  return XYZA{x, y, z, ao};
}
static XYZA apply_beaming(const XYZA& c, double redshift, double exponent) {  // :72-80
  double f = std::pow(redshift, exponent);
  return XYZA{c.x * f, c.y * f, c.z * f, c.alpha};
}
static double inv_compand_srgb(double u) {  // :301-308
  if (u <= 0.04045) return u / 12.92;
  return std::pow((u + 0.055) / 1.055, 2.4);
}
static XYZA srgb_to_xyz_alpha(uint8_t r8, uint8_t g8, uint8_t b8, uint8_t a8) {  // :310-332
  double r = inv_compand_srgb((double)r8 / 255.0);
  double g = inv_compand_srgb((double)g8 / 255.0);
  double b = inv_compand_srgb((double)b8 / 255.0);
  static const double M[3][3] = {{0.4124564, 0.3575761, 0.1804375},
                                 {0.2126729, 0.7151522, 0.0721750},
                                 {0.0193339, 0.1191920, 0.9503041}};
  double v[3] = {r, g, b}, o[3];
  for (int i = 0; i < 3; ++i) {
    double s = M[i][0] * v[0];
    s = M[i][1] * v[1] + s;
    s = M[i][2] * v[2] + s;
    o[i] = s;
  }
  return XYZA{o[0], o[1], o[2], (double)a8 / 255.0};  // CIETristimulus::from_color
}

// ---------------------------------------------------------------- textures -------
struct TextureMap {
  const grt_texture_desc* d;
  const grt_scene_desc* scene;
  XYZA texel(uint32_t x, uint32_t y) const {
    const uint8_t* p = d->rgba + 4 * ((size_t)y * d->width + x);
    return srgb_to_xyz_alpha(p[0], p[1], p[2], p[3]);
  }
  XYZA bilinear(double u, double v) const {  // texture.rs:62-90
    uint32_t width = d->width, height = d->height;
    double p_x = (double)width * u;
    double p_y = (double)height * v;
    uint32_t xf = std::min(sat_u32(std::floor(p_x)), width - 1);
    uint32_t yf = std::min(sat_u32(std::floor(p_y)), height - 1);
    uint32_t xc = std::min(sat_u32(std::ceil(p_x)), width - 1);
    uint32_t yc = std::min(sat_u32(std::ceil(p_y)), height - 1);
    XYZA c00 = texel(xf, yf), c01 = texel(xf, yc), c11 = texel(xc, yc), c10 = texel(xc, yf);
    double dx = p_x - (double)xf;
    double dy = p_y - (double)yf;
    double w00 = (1.0 - dx) * (1.0 - dy);
    double w01 = (1.0 - dx) * dy;
    double w10 = dx * (1.0 - dy);
    double w11 = dx * dy;
    auto mul = [](double w, const XYZA& c) { return XYZA{w * c.x, w * c.y, w * c.z, w * c.alpha}; };
    auto add = [](const XYZA& a, const XYZA& b) {
      return XYZA{a.x + b.x, a.y + b.y, a.z + b.z, a.alpha + b.alpha};
    };
    return add(add(add(mul(w00, c00), mul(w10, c10)), mul(w01, c01)), mul(w11, c11));
  }
  // log_t_in: log10(max(temperature, 10)) given by the caller in place of std::log10
  // (oracle_blackbody_n, oracle_texture_color_n: the one operation of the lookup whose bits
  // depend on the platform's libm)
  XYZA sample_blackbody(double temperature, const double* log_t_in = nullptr) const {  // texture.rs:149-195
    uint32_t n = scene->bb_n;
    const double* lt = scene->bb_log_t;
    const double* c = scene->bb_xyz;
    XYZA first{c[0], c[1], c[2], 1.0}, last{c[3 * (n - 1)], c[3 * (n - 1) + 1], c[3 * (n - 1) + 2], 1.0};
    double log_t = log_t_in ? *log_t_in : std::log10(std::fmax(temperature, 10.0));
    if (!std::isfinite(log_t)) return first;
    if (log_t <= lt[0]) return first;
    if (log_t >= lt[n - 1]) return last;
    // binary_search_by(total_cmp): index of the last entry <= log_t (strictly increasing LUT)
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
      uint32_t mid = lo + (hi - lo) / 2;
      if (lt[mid] <= log_t) lo = mid + 1; else hi = mid;
    }
    uint32_t idx = lo == 0 ? 0 : lo - 1;
    double lt0 = lt[idx], lt1 = lt[idx + 1];
    const double* c0 = c + 3 * idx;
    const double* c1 = c + 3 * (idx + 1);
    double t = (log_t - lt0) / (lt1 - lt0);
    return XYZA{c0[0] + t * (c1[0] - c0[0]), c0[1] + t * (c1[1] - c0[1]), c0[2] + t * (c1[2] - c0[2]), 1.0};
  }
  XYZA color_at_uv(double u, double v, double redshift, double temperature, const double* log_t_in = nullptr) const {
    switch (d->kind) {
      case GRT_TEX_BITMAP:  // texture.rs:93-102
        return apply_beaming(bilinear(u, v), redshift, d->beaming_exponent);
      case GRT_TEX_CHECKER: {  // texture.rs:240-257
        uint64_t ut = sat_u64(std::floor(u * d->checker_width));
        uint64_t vt = sat_u64(std::floor(v * d->checker_height));
        const double* c = ((ut + vt) % 2 == 0) ? d->c1 : d->c2;
        return apply_beaming(XYZA{c[0], c[1], c[2], c[3]}, redshift, d->beaming_exponent);
      }
      default:  // GRT_TEX_BLACKBODY, texture.rs:198-210
        return apply_beaming(sample_blackbody(temperature * redshift, log_t_in), redshift, d->beaming_exponent);
    }
  }
};

// --------------------------------------------------------------- objects --------
struct Intersection {  // hittable.rs:7-12
  double u, v;
  Point point;
  double t;
};

static Err compute_temperature(const grt_object_desc& o, double radius, double* out) {
  if (o.temp_kind == GRT_TEMP_CONSTANT) {  // temperature.rs:22-26
    *out = o.temp_constant;
    return OK;
  }
  // temperature.rs:198-253
  if (!std::isfinite(radius)) return NonFiniteRadius;
  if (radius < o.r_isco) return BelowRISCO;
  uint32_t n = o.lut_n;
  if (radius <= o.lut_r[0]) { *out = o.lut_t[0]; return OK; }
  if (radius >= o.lut_r[n - 1]) { *out = o.lut_t[n - 1]; return OK; }
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = lo + (hi - lo) / 2;
    if (o.lut_r[mid] <= radius) lo = mid + 1; else hi = mid;
  }
  uint32_t idx = lo == 0 ? 0 : lo - 1;
  double r0 = o.lut_r[idx], t0 = o.lut_t[idx], r1 = o.lut_r[idx + 1], t1 = o.lut_t[idx + 1];
  double t = (radius - r0) / (r1 - r0);
  *out = t0 + t * (t1 - t0);
  return OK;
}

// disc.rs:41-88
static bool disc_intersects(const grt_object_desc& o, const Point& ys, const Point& ye, Intersection* out) {
  Vec3 s = spatial_cartesian(ys);
  Vec3 e = spatial_cartesian(ye);
  Vec3 d{e.x - s.x, e.y - s.y, e.z - s.z};
  Vec3 normal{0.0, 0.0, 1.0};
  Vec3 cms{0.0 - s.x, 0.0 - s.y, 0.0 - s.z};
  double p1 = dot3(cms, normal);
  double p2 = dot3(d, normal);
  double t = p1 / p2;
  if (!(0.0 <= t && t <= 1.0)) return false;
  Vec3 ip{s.x + t * d.x, s.y + t * d.y, s.z + t * d.z};
  double rr = dot3(ip, ip);
  double rin = o.inner_radius, rout = o.outer_radius;
  if (rr >= rin * rin && rr <= rout * rout) {
    double vx = ip.x - 0.0, vy = ip.y - 0.0;
    double phi = shade_angle(std::atan2(vy, vx));
    double r = (std::sqrt(rr) - rin) / (rout - rin);
    double sp, cp;
    g_sincos(phi, &sp, &cp);
    out->u = 0.5 + 0.5 * r * cp;
    out->v = 0.5 + 0.5 * r * sp;
    out->point = Point{CS::Cartesian, 0.0, {0.0, ip.x, ip.y, ip.z}};
    out->t = t;
    return true;
  }
  return false;
}
// sphere.rs:37-58
static bool solve_for_t(const Vec3& s, const Vec3& d, double r, double* t_out) {
  double a = dot3(d, d);
  double b = 2.0 * dot3(s, d);
  double c = dot3(s, s) - r * r;
  double disc = b * b - 4.0 * a * c;
  if (disc < 0.0) return false;
  double sq = std::sqrt(disc);
  double t1 = (-b + sq) / (2.0 * a);
  double t2 = (-b - sq) / (2.0 * a);
  if (0.0 <= t1 && t1 <= 1.0) { *t_out = t1; return true; }
  if (0.0 <= t2 && t2 <= 1.0) { *t_out = t2; return true; }
  return false;
}
// sphere.rs:62-128
static bool sphere_intersects(const grt_object_desc& o, const Point& ys, const Point& ye, Intersection* out) {
  Point sc = to_cartesian(ys), ec = to_cartesian(ye);
  double neg[4] = {-0.0, -o.center[0], -o.center[1], -o.center[2]};
  double ss[4], es[4];
  for (int i = 0; i < 4; ++i) { ss[i] = sc.v[i] + neg[i]; es[i] = ec.v[i] + neg[i]; }
  double r_start = ss[1] * ss[1] + ss[2] * ss[2] + ss[3] * ss[3];
  double r_end = es[1] * es[1] + es[2] * es[2] + es[3] * es[3];
  double R2 = o.radius * o.radius;
  if ((r_start >= R2 && r_end <= R2) || (r_start <= R2 && r_end >= R2)) {
    Vec3 s{ss[1], ss[2], ss[3]}, e{es[1], es[2], es[3]};
    Vec3 d{e.x - s.x, e.y - s.y, e.z - s.z};
    double t;
    if (!solve_for_t(s, d, o.radius, &t)) return false;
    Vec3 p{s.x + t * d.x, s.y + t * d.y, s.z + t * d.z};
    Point local = cartesian_to_spherical(Point{CS::Cartesian, 0.0, {0.0, p.x, p.y, p.z}});
    double theta = local[2], phi = local[3];
    double u = (PI + phi) / (2.0 * PI);
    double v = theta / PI;
    out->u = 1.0 - u;
    out->v = v;
    out->point = Point{CS::Cartesian, 0.0, {0.0, p.x + o.center[0], p.y + o.center[1], p.z + o.center[2]}};
    out->t = t;
    return true;
  }
  return false;
}

// ------------------------------------------------------------ volumetric disc ----
// scene_objects/volumetric_disc.rs.  Its noise is Perlin of the `noise` crate 0.9.0
// (Cargo.lock; with rand 0.8.7 and rand_xorshift 0.3.0), which is NOT vendored under
// /root/reference: perlin_3d, PermutationTable and the RNG below restate the crates'
// published algorithms, so the noise values are "parity unpinned" (no reference test
// fixes them; the volumetric_disc.rs tests pin the rest, tests/test_oracle_kats.py).
namespace noise09 {
struct XorShift {  // rand_xorshift 0.3.0 XorShiftRng::next_u32
  uint32_t x, y, z, w;
  uint32_t next_u32() {
    uint32_t t = x ^ (x << 11);
    x = y;
    y = z;
    z = w;
    w = w ^ (w >> 19) ^ (t ^ (t >> 8));
    return w;
  }
};
// rand 0.8 Rng::gen_range(0..n) for u32 = UniformInt::sample_single_inclusive(0, n - 1)
static uint32_t gen_range(XorShift& rng, uint32_t n) {
  uint32_t range = n;
  uint32_t zone = (range << __builtin_clz(range)) - 1u;  // `(range << lz).wrapping_sub(1)`
  while (true) {
    uint64_t m = (uint64_t)rng.next_u32() * (uint64_t)range;  // wmul
    if ((uint32_t)m <= zone) return (uint32_t)(m >> 32);
  }
}
// permutationtable.rs PermutationTable::new(seed) + Distribution<PermutationTable>
static void permutation_table(uint32_t seed, uint8_t* values) {
  uint8_t real[16] = {0};
  real[0] = 1;
  for (int i = 1; i < 4; ++i) {
    real[i * 4] = (uint8_t)seed;
    real[i * 4 + 1] = (uint8_t)(seed >> 8);
    real[i * 4 + 2] = (uint8_t)(seed >> 16);
    real[i * 4 + 3] = (uint8_t)(seed >> 24);
  }
  uint32_t w[4];
  for (int i = 0; i < 4; ++i)  // XorShiftRng::from_seed: little-endian words
    w[i] = (uint32_t)real[4 * i] | (uint32_t)real[4 * i + 1] << 8 | (uint32_t)real[4 * i + 2] << 16 |
           (uint32_t)real[4 * i + 3] << 24;
  XorShift rng{w[0], w[1], w[2], w[3]};
  for (int i = 0; i < 256; ++i) values[i] = (uint8_t)i;
  for (int i = 255; i >= 1; --i) {  // SliceRandom::shuffle
    uint32_t j = gen_range(rng, (uint32_t)i + 1);
    std::swap(values[i], values[j]);
  }
}
// NoiseHasher for PermutationTable: fold (a & 0xff) with values[a] ^ b, then values[.]
static inline size_t hash3(const uint8_t* P, int64_t x, int64_t y, int64_t z) {
  size_t i = (size_t)(x & 0xff);
  i = (size_t)P[i] ^ (size_t)(y & 0xff);
  i = (size_t)P[i] ^ (size_t)(z & 0xff);
  return P[i];
}
static inline double gradient_dot_v(size_t perm, double x, double y, double z) {  // core/perlin.rs
  switch (perm & 15) {
    case 0: return x + y;
    case 1: return -x + y;
    case 2: return x - y;
    case 3: return -x - y;
    case 4: return x + z;
    case 5: return -x + z;
    case 6: return x - z;
    case 7: return -x - z;
    case 8: return y + z;
    case 9: return -y + z;
    case 10: return y - z;
    case 11: return -y - z;
    case 12: return x + y;
    case 13: return -x + y;
    case 14: return -y + z;
    default: return -y - z;
  }
}
static inline double s_curve5(double x) { return x * x * x * (x * (x * 6.0 - 15.0) + 10.0); }
// core/perlin.rs perlin_3d (Perlin::get)
static double perlin_3d(const uint8_t* P, double px, double py, double pz) {
  const double SCALE_FACTOR = 1.1547005383792515;
  double fx = std::floor(px), fy = std::floor(py), fz = std::floor(pz);
  int64_t cx = (int64_t)fx, cy = (int64_t)fy, cz = (int64_t)fz;
  double dx = px - fx, dy = py - fy, dz = pz - fz;
  auto g = [&](int ox, int oy, int oz) {
    return gradient_dot_v(hash3(P, cx + ox, cy + oy, cz + oz), dx - (double)ox, dy - (double)oy, dz - (double)oz);
  };
  double g000 = g(0, 0, 0), g100 = g(1, 0, 0), g010 = g(0, 1, 0), g110 = g(1, 1, 0);
  double g001 = g(0, 0, 1), g101 = g(1, 0, 1), g011 = g(0, 1, 1), g111 = g(1, 1, 1);
  double a = s_curve5(dx), b = s_curve5(dy), c = s_curve5(dz);
  double k0 = g000;
  double k1 = g100 - g000;
  double k2 = g010 - g000;
  double k3 = g001 - g000;
  double k4 = g000 + g110 - g100 - g010;
  double k5 = g000 + g101 - g100 - g001;
  double k6 = g000 + g011 - g010 - g001;
  double k7 = g100 + g010 + g001 + g111 - g000 - g110 - g101 - g011;
  double result = k0 + k1 * a + k2 * b + k3 * c + k4 * a * b + k5 * a * c + k6 * b * c + k7 * a * b * c;
  return rust_clamp(result * SCALE_FACTOR, -1.0, 1.0);
}
}  // namespace noise09

static inline Vec3 cross3(const Vec3& a, const Vec3& b) {  // nalgebra Vector3::cross
  return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
static inline Vec3 normalize3(const Vec3& v) {  // nalgebra normalize = v / |v|
  double n = norm3(v);
  return Vec3{v.x / n, v.y / n, v.z / n};
}
static inline double rust_max(double a, double b) { return std::fmax(a, b); }  // f64::max

enum CylKind { NoIntersection, Parallel, OneIntersection, TwoIntersections };
struct Cyl {
  CylKind k;
  double t1, t2;
};

struct VDisc {  // volumetric_disc.rs:21-95
  const grt_object_desc* o = nullptr;
  Vec3 axis, e1, e2;
  uint8_t perm[256];
  double g_fbm;  // (-h).exp2() with h = 0.5 (fbm's only call, :130)
  void init(const grt_object_desc* od) {
    o = od;
    Vec3 ax{od->axis[0], od->axis[1], od->axis[2]};
    axis = dot3(ax, ax) <= 2.220446049250313e-16 ? Vec3{0.0, 0.0, 1.0} : normalize3(ax);
    Vec3 seed = std::fabs(axis.x) > 0.9 ? Vec3{0.0, 1.0, 0.0} : Vec3{1.0, 0.0, 0.0};
    e1 = normalize3(cross3(seed, axis));
    e2 = normalize3(cross3(axis, e1));
    noise09::permutation_table(od->perlin_seed, perm);
    g_fbm = std::exp2(-0.5);
  }
  double noise(double x, double y, double z) const { return noise09::perlin_3d(perm, x, y, z); }
  double fbm(const Vec3& x) const {  // :330-342
    double frequency = 4.0, amplitude = 1.0, t = 0.0;
    for (uint32_t i = 0; i < o->num_octaves; ++i) {
      t += amplitude * noise(x.x * frequency, x.y * frequency, x.z * frequency);
      frequency *= 2.0;
      amplitude *= g_fbm;
    }
    return t;
  }
  // phi_in: the in-plane angle given by the caller in place of atan2 (oracle_vdisc_density_phi:
  // the one operation of the density whose bits depend on the platform's libm)
  // plane_out (x_local, y_local) and *noise_out = whether the noise was evaluated (the point passed both
  // early returns): oracle_vdisc_plane_n, for the device check of the same three values
  double compute_density(const Vec3& p, const double* phi_in = nullptr, double* plane_out = nullptr,
                         bool* noise_out = nullptr) const {  // :97-138
    double h = std::fabs(dot3(p, axis));
    double r = norm3(cross3(p, axis));
    double rin = o->inner_radius, rout = o->outer_radius;
    if (r <= rin || r >= rout) return 0.0;
    double q = h / o->thickness;
    double vertical_falloff = std::exp(-(q * q));
    if (vertical_falloff < 0.001) return 0.0;
    double radial_base = std::pow(rin / r, 1.5);
    double boundary_falloff = 1.0;
    double d1 = rout - r, d2 = r - rin;
    boundary_falloff *= std::exp(-1.0 / rust_max(d1 * d1, 0.0001));
    boundary_falloff *= std::exp(-1.0 / rust_max(d2 * d2, 0.0001));
    double x_local = dot3(p, e1);
    double y_local = dot3(p, e2);
    if (plane_out) { plane_out[0] = x_local; plane_out[1] = y_local; }
    if (noise_out) *noise_out = true;
    double phi = phi_in ? *phi_in : vdisc_angle(std::atan2(y_local, x_local));
    double sp, cp;
    g_sincos(phi, &sp, &cp);  // phi.cos() and phi.sin() in one block: one sincos
    double noise_phi_x = cp * o->noise_scale[1];
    double noise_phi_y = sp * o->noise_scale[1];
    double n = fbm(Vec3{r * o->noise_scale[0], noise_phi_x, noise_phi_y});
    n += noise(r * 0.5, h * o->noise_scale[2], cp) * 0.5;
    double n2 = rust_max(n + o->noise_offset, 0.0) * o->density_multiplier;
    return n2 * radial_base * vertical_falloff * boundary_falloff;
  }
  void get_uv(const Vec3& p, double* u, double* v) const {  // :140-152
    double x = dot3(p, e1), y = dot3(p, e2);
    double rr = std::sqrt(x * x + y * y);
    double phi = vdisc_angle(std::atan2(y, x));
    double r = (rr - o->inner_radius) / (o->outer_radius - o->inner_radius);
    double sp, cp;
    g_sincos(phi, &sp, &cp);
    *u = 0.5 + 0.5 * r * cp;
    *v = 0.5 + 0.5 * r * sp;
  }
  Cyl clipped_cylinder(const Vec3& from, const Vec3& to, double radius, double half_height) const {  // :348-405
    Vec3 sv{to.x - from.x, to.y - from.y, to.z - from.z};
    double len = norm3(sv);
    if (len < 1e-12) return Cyl{NoIntersection, 0, 0};
    Vec3 d{sv.x / len, sv.y / len, sv.z / len};
    Vec3 v = cross3(from, axis);
    Vec3 w = cross3(d, axis);
    double a = dot3(w, w);
    double b = 2.0 * dot3(v, w);
    double c = dot3(v, v) - radius * radius;
    if (a < 1e-10) {
      if (dot3(v, v) > radius * radius) return Cyl{NoIntersection, 0, 0};
      return Cyl{Parallel, 0, 0};
    }
    double disc = b * b - 4.0 * a * c;
    if (disc < 0.0) return Cyl{NoIntersection, 0, 0};
    double sq = std::sqrt(disc);
    double dists[2] = {(-b - sq) / (2.0 * a), (-b + sq) / (2.0 * a)};
    double hits[2];
    int nh = 0;
    for (double dist : dists) {
      double t = dist / len;
      if (0.0 <= t && t <= 1.0) {
        Vec3 p{from.x + t * sv.x, from.y + t * sv.y, from.z + t * sv.z};
        if (std::fabs(dot3(p, axis)) <= half_height) hits[nh++] = t;
      }
    }
    if (nh == 0) return Cyl{NoIntersection, 0, 0};
    if (nh == 1) return Cyl{OneIntersection, hits[0], 0};
    return Cyl{TwoIntersections, std::fmin(hits[0], hits[1]), std::fmax(hits[0], hits[1])};
  }
  bool cap(const Vec3& from, const Vec3& to, double radius, double pos, double* t_out) const {  // :407-440
    Vec3 sv{to.x - from.x, to.y - from.y, to.z - from.z};
    double len = norm3(sv);
    if (len < 1e-12) return false;
    Vec3 n{sv.x / len, sv.y / len, sv.z / len};
    double denom = dot3(n, axis);
    if (std::fabs(denom) < 1e-10) return false;
    double t = (pos - dot3(from, axis)) / dot3(sv, axis);
    if (!(0.0 <= t && t <= 1.0)) return false;
    Vec3 p{from.x + t * sv.x, from.y + t * sv.y, from.z + t * sv.z};
    Vec3 c = cross3(p, axis);
    if (dot3(c, c) > radius * radius) return false;
    *t_out = t;
    return true;
  }
  Cyl cylinder(const Vec3& from, const Vec3& to) const {  // intersects_cylinder :442-494
    double rin = o->inner_radius, rout = o->outer_radius;
    std::vector<double> hits;
    Vec3 dir{to.x - from.x, to.y - from.y, to.z - from.z};
    double capture_height = o->thickness * 3.0;
    for (double radius : {rout, rin}) {
      Cyl c = clipped_cylinder(from, to, radius, capture_height);
      if (c.k == OneIntersection) hits.push_back(c.t1);
      else if (c.k == TwoIntersections) { hits.push_back(c.t1); hits.push_back(c.t2); }
    }
    for (double pos : {capture_height, -capture_height}) {
      double t;
      if (cap(from, to, rout, pos, &t)) {
        Vec3 p{from.x + t * dir.x, from.y + t * dir.y, from.z + t * dir.z};
        Vec3 c = cross3(p, axis);
        if (dot3(c, c) >= rin * rin) hits.push_back(t);
      }
    }
    auto total_key = [](double x) {  // f64::total_cmp order
      uint64_t u;
      std::memcpy(&u, &x, 8);
      return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    };
    std::stable_sort(hits.begin(), hits.end(), [&](double a, double b) { return total_key(a) < total_key(b); });
    if (hits.empty()) return Cyl{NoIntersection, 0, 0};
    if (hits.size() == 1) return Cyl{OneIntersection, hits[0], 0};
    return Cyl{TwoIntersections, hits[0], hits[1]};
  }
  // Hittable::intersects (:506-578): first capture-boundary crossing with t > 1e-9
  bool intersects(const Vec3& s, const Vec3& e, double* t_out, Vec3* point, Vec3* direction) const {
    Vec3 dir{e.x - s.x, e.y - s.y, e.z - s.z};
    Cyl c = cylinder(s, e);
    double t;
    const double MIN_T = 1e-9;
    if (c.k == NoIntersection || c.k == Parallel) return false;
    if (c.k == OneIntersection) {
      if (!(c.t1 > MIN_T)) return false;
      t = c.t1;
    } else {
      if (c.t1 > MIN_T) t = c.t1;
      else if (c.t2 > MIN_T) t = c.t2;
      else return false;
    }
    if (!(0.0 <= t && t <= 1.0)) return false;  // error! + None
    *t_out = t;
    *point = Vec3{s.x + t * dir.x, s.y + t * dir.y, s.z + t * dir.z};
    *direction = dir;
    return true;
  }
  bool precompute_exit_distance(const Vec3& ro, const Vec3& rd, double* out) const {  // :172-196
    double max_distance = o->march_step_size * (double)o->march_max_steps;
    Vec3 to{ro.x + rd.x * max_distance, ro.y + rd.y * max_distance, ro.z + rd.z * max_distance};
    Cyl c = cylinder(ro, to);
    const double MIN_T = 1e-9;
    if (c.k == OneIntersection) {
      if (c.t1 > MIN_T) { *out = c.t1 * max_distance; return true; }
      return false;
    }
    if (c.k == TwoIntersections) {
      if (c.t1 > MIN_T) { *out = c.t1 * max_distance; return true; }
      if (c.t2 > MIN_T) { *out = c.t2 * max_distance; return true; }
    }
    return false;
  }
  bool does_exit(const Vec3& p, const Vec3& rd, double t) const {  // :154-170
    Vec3 to{p.x + rd.x * t, p.y + rd.y * t, p.z + rd.z * t};
    double ti;
    Vec3 ip, dir;
    if (!intersects(p, to, &ti, &ip, &dir)) return false;
    return ti > 1e-9;
  }
};

struct FrequencyData {  // redshift.rs RayFrequencyData
  double observer_energy, p_t, p_phi;
};

// Geometry::circular_orbit_killing_coefficients of a Cartesian point (euclidean.rs:207-217,
// euclidean_spherical.rs:191-201, schwarzschild.rs:260-265, kerr.rs:487-496, kerr_bl.rs:398-410)
static Err killing_at(const Geometry& g, int32_t geometry, const Point& cart, Killing* k) {
  if (geometry == GRT_GEOM_EUCLIDEAN || geometry == GRT_GEOM_EUCLIDEAN_SPHERICAL) {
    k->u_t = 1.0;
    k->u_phi = 0.0;
    return OK;
  }
  double spin = geometry == GRT_GEOM_SCHWARZSCHILD ? 0.0 : g.a;
  return killing_coefficients(g.radius, spin, g.radial_coordinate(cart), k);
}

// raymarch_constant_step_internal (:209-328).  Returns the error that the reference's
// `?` would propagate (color_at_uv then substitutes (0,0,0,0), :596-600).
static Err vdisc_raymarch(const VDisc& V, const TextureMap& tex, const Geometry& g, int32_t geometry,
                          const Vec3& ro, const Vec3& rd, const FrequencyData& f, bool use_cached_exit,
                          XYZA* out, uint64_t* samples) {
  const grt_object_desc& o = *V.o;
  double sigma_a = o.absorption, sigma_s = o.scattering;
  XYZA acc{0.0, 0.0, 0.0, 0.0};
  double transparency = 1.0, alpha_weighted_sum = 0.0, alpha_weight_total = 0.0;
  double d_s = o.march_step_size, d_o = 0.0;
  double exit_distance = 0.0;
  bool cached = use_cached_exit && V.precompute_exit_distance(ro, rd, &exit_distance);
  for (uint64_t i = 0; i < o.march_max_steps; ++i) {
    Vec3 p{ro.x + rd.x * d_o, ro.y + rd.y * d_o, ro.z + rd.z * d_o};
    d_o += d_s;
    if (samples) ++*samples;
    double density = V.compute_density(p);
    if (density > 0.0) {
      double sample_attenuation = std::exp(-d_s * density * (sigma_a + sigma_s));
      transparency *= sample_attenuation;
      Killing k;
      if (killing_at(g, geometry, Point{CS::Cartesian, 0.0, {0.0, p.x, p.y, p.z}}, &k) == OK) {
        double emitter_energy = k.u_t * f.p_t + k.u_phi * f.p_phi;
        double redshift = f.observer_energy / emitter_energy;
        double r_dist = norm3(cross3(p, V.axis));
        double temperature;
        Err e = compute_temperature(o, r_dist, &temperature);
        if (e != OK) return e;
        double u, v;
        V.get_uv(p, &u, &v);
        XYZA light = tex.color_at_uv(u, v, redshift, temperature);
        double travel_density = d_s;
        double light_attenuation = std::exp(-density * travel_density * (sigma_a + sigma_s));
        double ratio = temperature / o.brightness_reference_temperature;
        double r2 = ratio * ratio;
        double intensity_factor = r2 * r2;  // powi(4)
        double emission_weight = transparency * light_attenuation * sigma_s * density * d_s;
        double wgt = emission_weight * intensity_factor;
        double alpha_sample_weight = density * d_s;
        alpha_weighted_sum += rust_clamp(light.alpha, 0.0, 1.0) * alpha_sample_weight;
        alpha_weight_total += alpha_sample_weight;
        acc.x += light.x * wgt;
        acc.y += light.y * wgt;
        acc.z += light.z * wgt;
      }
    }
    bool exited = cached ? d_o >= exit_distance : V.does_exit(p, rd, d_s);
    if (exited) break;
  }
  double physical_opacity = 1.0 - transparency;
  double texture_alpha = alpha_weight_total > 0.0 ? alpha_weighted_sum / alpha_weight_total : 1.0;
  acc.alpha = physical_opacity * texture_alpha;
  *out = acc;
  return OK;
}

struct SceneCtx {
  const grt_scene_desc* d;
  std::unique_ptr<Geometry> g;
  IntegrationConfig cfg;
  FourVector cam_velocity;
  Point cam_position;
  TextureMap celestial;
  TextureMap obj_tex[GRT_MAX_OBJECTS];
  VDisc vd[GRT_MAX_OBJECTS];  // VolumetricDisc frames + permutation tables
};

// objects.rs:27-44
static Step step_at_intersection(const Geometry& g, const Step& a, const Step& b, const Point& ip, double t) {
  double s = 1.0 - t;
  Step st;
  st.t = s * a.t + t * b.t;
  st.step = a.step;
  st.x = to_coordinate_system(ip, a.x.cs, g.a);
  st.p.cs = a.p.cs;
  for (int i = 0; i < 4; ++i) st.p.v[i] = s * a.p.v[i] + t * b.p.v[i];
  return st;
}

// objects.rs:65-120
static Err objects_intersects(const SceneCtx& S, const Step& ys, const Step& ye, const FrequencyData& freq,
                              bool* has, XYZA* color, uint64_t* march_samples) {
  const double observer_energy = freq.observer_energy;
  const Geometry& g = *S.g;
  *has = false;
  double shortest = std::numeric_limits<double>::max();
  Vec3 ysc = spatial_cartesian(ys.x);
  for (uint32_t k = 0; k < S.d->n_objects; ++k) {
    const grt_object_desc& o = S.d->objects[k];
    Intersection in;
    Vec3 vdir{0.0, 0.0, 0.0};
    bool hit;
    if (o.kind == GRT_OBJ_VOLUMETRIC_DISC) {  // volumetric_disc.rs:506-578
      Vec3 vp{0.0, 0.0, 0.0};
      hit = S.vd[k].intersects(spatial_cartesian(ys.x), spatial_cartesian(ye.x), &in.t, &vp, &vdir);
      in.point = Point{CS::Cartesian, 0.0, {0.0, vp.x, vp.y, vp.z}};
    } else {
      hit = o.kind == GRT_OBJ_DISC ? disc_intersects(o, ys.x, ye.x, &in) : sphere_intersects(o, ys.x, ye.x, &in);
    }
    if (!hit) continue;
    Vec3 ip = spatial_cartesian(in.point);
    Vec3 dv{ip.x - ysc.x, ip.y - ysc.y, ip.z - ysc.z};
    double distance = norm3(dv);
    if (distance < shortest) {
      shortest = distance;
      Step st = step_at_intersection(g, ys, ye, in.point, in.t);
      FourVector vel;
      if (o.kind != GRT_OBJ_SPHERE) {  // disc.rs:101-110, volumetric_disc.rs:603-612
        Err e = g.circular_orbit_velocity(st.x, &vel);
        if (e != OK) return e;
      } else {  // sphere.rs:141-150
        vel = g.stationary_velocity(st.x);
      }
      double emitter_energy = g.inner_product(st.x, vel, st.p);
      double sig0 = g.signature0();
      double redshift = (sig0 * observer_energy) / (sig0 * emitter_energy);  // redshift.rs:36-38
      double temperature;
      if (o.kind != GRT_OBJ_SPHERE) {  // disc.rs:112-120, volumetric_disc.rs:614-622
        Err e = compute_temperature(o, g.radial_coordinate(in.point), &temperature);
        if (e != OK) return e;
      } else {
        temperature = o.temperature;
      }
      if (o.kind == GRT_OBJ_VOLUMETRIC_DISC) {  // color_at_uv (:580-601): raymarch from the hit
        Vec3 rd = normalize3(vdir);
        XYZA c;
        if (vdisc_raymarch(S.vd[k], S.obj_tex[k], g, S.d->geometry, ip, rd, freq, true, &c, march_samples) != OK)
          c = XYZA{0.0, 0.0, 0.0, 0.0};  // unwrap_or_else
        *color = c;
      } else {
        *color = S.obj_tex[k].color_at_uv(in.u, in.v, redshift, temperature);
      }
      *has = true;
    }
  }
  return OK;
}

// RedshiftComputer::get_ray_frequency_data (redshift.rs:45-60) with the geometries'
// axial_killing_vector (euclidean.rs:203-205, kerr.rs:482-485: (0, -y, x, 0);
// schwarzschild.rs:256-258, euclidean_spherical.rs:187-189, kerr_bl.rs:394-396: d_phi)
static FrequencyData ray_frequency_data(const SceneCtx& S, const Ray& ray, double observer_energy) {
  const Geometry& g = *S.g;
  FrequencyData f;
  f.observer_energy = observer_energy;
  FourVector e_t{ray.momentum.cs, {1.0, 0.0, 0.0, 0.0}};
  f.p_t = g.inner_product(ray.position, e_t, ray.momentum);
  int32_t geo = S.d->geometry;
  FourVector ax = (geo == GRT_GEOM_EUCLIDEAN || geo == GRT_GEOM_KERR)
                      ? FourVector{CS::Cartesian, {0.0, -ray.position[2], ray.position[1], 0.0}}
                      : FourVector{g.cs(), {0.0, 0.0, 0.0, 1.0}};
  f.p_phi = g.inner_product(ray.position, ax, ray.momentum);
  return f;
}

// camera.rs:214-232
static FourVector get_direction_for(const grt_camera_desc& c, double row, double column) {
  double shifted_column = column + 1.0;
  double shifted_row = row + 1.0;
  double tha = c.tan_half_alpha;
  double rows = (double)c.rows, cols = (double)c.cols;
  double i_prime = c.spatial_handedness * (2.0 * tha / rows) * (shifted_column - (cols + 1.0) / 2.0);
  double j_prime = (2.0 * tha / rows) * (shifted_row - (rows + 1.0) / 2.0);
  double w[4];
  for (int k = 0; k < 4; ++k) w[k] = c.tetrad[3][k] + i_prime * c.tetrad[1][k] + j_prime * c.tetrad[2][k];
  double w_squared = c.spatial_signature * (1.0 + i_prime * i_prime + j_prime * j_prime);
  FourVector dir{CS::Cartesian, {0, 0, 0, 0}};
  for (int k = 0; k < 4; ++k) dir.v[k] = -c.tetrad[3][k] + 2.0 * w[k] / (c.spatial_signature * w_squared);
  return dir;
}

static Ray make_ray(const SceneCtx& S, int64_t row, int64_t col, bool offset, double dx, double dy) {
  const grt_camera_desc& c = S.d->camera;
  FourVector dir = offset ? get_direction_for(c, (double)row + (dy - 0.5), (double)col + (dx - 0.5))
                          : get_direction_for(c, (double)row, (double)col);  // camera.rs:234-254
  Ray ray;
  ray.row = row;
  ray.col = col;
  ray.position = S.cam_position;
  ray.momentum.cs = S.g->cs();
  for (int k = 0; k < 4; ++k) ray.momentum.v[k] = dir.v[k] + (-c.tetrad[0][k]);
  return ray;
}

struct Sample {
  XYZA color;
  int ray_class;
  int status;
  int stop;
  uint64_t steps;
  uint32_t hits;  // windows with an intersection (intersections.len() before the terminal colour)
};

// scene.rs:114-220
static Err color_of_ray(const SceneCtx& S, const Ray& ray, Sample* out, Counters* cnt) {
  const Geometry& g = *S.g;
  std::vector<Step> steps;
  int stop;
  Counters local;
  Err e = integrate(g, S.cfg, ray, steps, &stop, &local);
  cnt->accepted += local.accepted;
  cnt->attempts += local.attempts;
  out->steps = local.accepted;
  out->stop = stop;
  out->hits = 0;
  if (e != OK) return e;
  double observer_energy = g.inner_product(ray.position, S.cam_velocity, ray.momentum);  // redshift.rs:40-43
  FrequencyData freq = ray_frequency_data(S, ray, observer_energy);
  double object_opacity = 0.0;
  std::vector<XYZA> intersections;
  for (size_t w = 0; w + 1 < steps.size(); ++w) {
    bool has;
    XYZA c;
    Err ie = objects_intersects(S, steps[w], steps[w + 1], freq, &has, &c, &cnt->march_samples);
    if (ie != OK) return ie;
    if (has) {
      intersections.push_back(c);
      out->hits++;
      double alpha = rust_clamp(c.alpha, 0.0, 1.0);
      object_opacity = alpha + object_opacity * (1.0 - alpha);
    }
  }
  const Step& last = steps.back();
  int ray_class = GRT_CLASS_CAPTURED;
  if (stop == GRT_STOP_HORIZON || stop == GRT_STOP_CLOSED_ORBIT) {
    intersections.push_back(XYZA{0.0, 0.0, 0.0, 1.0});
  } else if (stop == GRT_STOP_CELESTIAL) {
    Vec3 sph = get_as_spherical(last.x);  // get_uv_coordinates :222-231
    double u = (PI + sph.z) / (2.0 * PI);
    double v = sph.y / PI;
    FourVector vel = g.stationary_velocity(last.x);  // redshift.rs:31-34, :62-67
    double em = g.inner_product(last.x, vel, last.p);
    double sig0 = g.signature0();
    double redshift = (sig0 * observer_energy) / (sig0 * em);
    intersections.push_back(S.celestial.color_at_uv(1.0 - u, v, redshift, S.d->celestial_temperature));
    ray_class = GRT_CLASS_ESCAPED;
  }
  XYZA result{0.0, 0.0, 0.0, 1.0};
  for (size_t k = intersections.size(); k-- > 0;) result = blend(result, intersections[k]);
  if (object_opacity >= S.d->object_hit_opacity_threshold) ray_class = GRT_CLASS_HIT;
  out->color = result;
  out->ray_class = ray_class;
  return OK;
}

static void init_ctx(SceneCtx& S, const grt_scene_desc* d) {
  S.d = d;
  switch (d->geometry) {
    case GRT_GEOM_EUCLIDEAN: S.g.reset(new Euclidean()); break;
    case GRT_GEOM_SCHWARZSCHILD: S.g.reset(new Schwarzschild()); break;
    case GRT_GEOM_KERR: S.g.reset(new Kerr()); break;
    case GRT_GEOM_EUCLIDEAN_SPHERICAL: S.g.reset(new EuclideanSpherical()); break;
    default: S.g.reset(new KerrBL()); break;
  }
  S.g->radius = d->radius;
  S.g->a = d->a;
  S.g->horizon_epsilon = d->horizon_epsilon;
  S.cfg.max_steps = d->max_steps;
  S.cfg.max_radius_sq = d->max_radius * d->max_radius;
  S.cfg.step_size = d->step_size;
  S.cfg.epsilon = d->epsilon;
  S.cam_position = Point{S.g->cs(), d->a, {d->camera.position[0], d->camera.position[1], d->camera.position[2], d->camera.position[3]}};
  S.cam_velocity = FourVector{S.g->cs(), {d->camera.velocity[0], d->camera.velocity[1], d->camera.velocity[2], d->camera.velocity[3]}};
  S.celestial = TextureMap{&d->celestial, d};
  for (uint32_t k = 0; k < d->n_objects && k < GRT_MAX_OBJECTS; ++k) {
    S.obj_tex[k] = TextureMap{&d->objects[k].texture, d};
    if (d->objects[k].kind == GRT_OBJ_VOLUMETRIC_DISC) S.vd[k].init(&d->objects[k]);
  }
}

static void default_sample(Sample* s) {
  s->color = XYZA{0.0, 0.0, 0.0, 1.0};
  s->ray_class = GRT_CLASS_ESCAPED;
}

static void trace_one(const SceneCtx& S, int64_t row, int64_t col, bool offset, double dx, double dy,
                      Sample* s, Counters* cnt) {
  Ray ray = make_ray(S, row, col, offset, dx, dy);
  Sample tmp;
  tmp.steps = 0;
  tmp.stop = 0;
  Err e = color_of_ray(S, ray, &tmp, cnt);
  if (e != OK) {
    default_sample(s);  // raytracer.rs:204-210, :232-239
    s->status = e;
    s->steps = tmp.steps;
    s->stop = tmp.stop;
    s->hits = tmp.hits;
  } else {
    *s = tmp;
    s->status = OK;
  }
}

// ------------------------------------------------ adaptive supersampling -------
static uint64_t mix64(uint64_t z) {  // raytracer.rs:132-136
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
static double hash_pixel_samples(int64_t row, int64_t col, uint64_t k) {  // :138-143
  uint64_t z = mix64((uint64_t)row + mix64((uint64_t)col + mix64(k)));
  return (double)(z >> 11) * (1.0 / (double)(1ULL << 53));
}
static void stratified_sample_offset(int64_t row, int64_t col, uint64_t sr, uint64_t sc, uint64_t n,
                                     double* dx, double* dy) {  // :145-159
  uint64_t idx = sr * n + sc;
  *dx = ((double)sc + hash_pixel_samples(row, col, 2 * idx)) / (double)n;
  *dy = ((double)sr + hash_pixel_samples(row, col, 2 * idx + 1)) / (double)n;
}
static bool should_supersample_pair(const Sample& p, const Sample& q, const grt_adaptive_config& c,
                                    double min_lum) {  // :91-108
  if (p.ray_class != q.ray_class) return true;
  if (c.exclude_background_contrast && p.ray_class == GRT_CLASS_ESCAPED) return false;
  bool visible = std::fmax(p.color.y, q.color.y) > min_lum;
  double lc = std::fabs(p.color.y - q.color.y) / (p.color.y + q.color.y + 1e-4);
  double oc = std::fabs(p.color.alpha - q.color.alpha);
  return visible && (lc > c.luminance_contrast_threshold || oc > c.opacity_contrast_threshold);
}
static int total_cmp(double a, double b) {  // f64::total_cmp
  int64_t ia, ib;
  std::memcpy(&ia, &a, 8);
  std::memcpy(&ib, &b, 8);
  ia ^= (int64_t)((uint64_t)(ia >> 63) >> 1);
  ib ^= (int64_t)((uint64_t)(ib >> 63) >> 1);
  return ia < ib ? -1 : (ia > ib ? 1 : 0);
}

// resolve_minimum_luminance (raytracer.rs:118-129) + collect_pixels_to_supersample
// (:386-458) over a w x h section buffer (row-major): the serial stencil, first trigger
// wins.  Returns the luminance floor; `sel` gets the selected section indices in order.
static double select_pixels(const std::vector<Sample>& buf, uint32_t w, uint32_t hgt,
                            const grt_adaptive_config& cfg, std::vector<uint64_t>* sel) {
  const uint64_t n = (uint64_t)w * hgt;
  double min_lum;
  if (cfg.has_minimum_luminance) min_lum = cfg.minimum_luminance;
  else if (n == 0) min_lum = 0.0;
  else {
    std::vector<double> lum(n);
    for (uint64_t i = 0; i < n; ++i) lum[i] = buf[i].color.y;
    uint64_t index = (uint64_t)((double)(n - 1) * 0.99);
    std::nth_element(lum.begin(), lum.begin() + index, lum.end(),
                     [](double a, double b) { return total_cmp(a, b) < 0; });
    min_lum = 1e-3 * lum[index];
  }
  static const int shifts[8][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};
  for (uint32_t row = 0; row < hgt; ++row)
    for (uint32_t col = 0; col < w; ++col) {
      uint64_t pi = (uint64_t)row * w + col;
      for (int s = 0; s < 8; ++s) {
        int64_t nr = (int64_t)row + shifts[s][0], nc = (int64_t)col + shifts[s][1];
        if (nr < 0 || nr >= (int64_t)hgt || nc < 0 || nc >= (int64_t)w) continue;
        uint64_t ni = (uint64_t)nr * w + (uint64_t)nc;
        if (should_supersample_pair(buf[pi], buf[ni], cfg, min_lum)) {
          sel->push_back(pi);
          break;
        }
      }
    }
  return min_lum;
}

#include "host_setup.inc"  // Camera::new, KerrTemperatureComputer::new, BlackBodyMapper::new

}  // namespace oracle

// =================================================================== C ABI =====
using namespace oracle;

extern "C" {

int oracle_abi_version(void) { return GRT_ABI_VERSION; }
void oracle_set_libm_perturbation(int mode) { g_libm_probe = mode; }

// One ray through Scene::color_of_ray.  use_offset selects get_ray_for_offset.
int oracle_color_of_ray(const grt_scene_desc* d, int64_t row, int64_t col, int use_offset, double dx,
                        double dy, double* xyza, uint8_t* ray_class, uint8_t* status, uint8_t* stop,
                        uint64_t* steps, uint64_t* attempts) {
  SceneCtx S;
  init_ctx(S, d);
  Sample s;
  Counters cnt;
  trace_one(S, row, col, use_offset != 0, dx, dy, &s, &cnt);
  xyza[0] = s.color.x; xyza[1] = s.color.y; xyza[2] = s.color.z; xyza[3] = s.color.alpha;
  if (ray_class) *ray_class = (uint8_t)s.ray_class;
  if (status) *status = (uint8_t)s.status;
  if (stop) *stop = (uint8_t)s.stop;
  if (steps) *steps = cnt.accepted;
  if (attempts) *attempts = cnt.attempts;
  return 0;
}

// The reference's invariant monitors per camera ray of a rectangle (scene.rs:116-124,
// integrator.rs:91-146): out[k * 5] |k.k| of the camera ray, [1] the largest |k.k| over the
// accepted steps, [2..4] the largest drift of each constant of motion from step 0
// (relative when |initial| > 1e-12); status[k] = the integration error (no drift report).
void oracle_health_pixels(const grt_scene_desc* d, uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols,
                          int threads, double* out, uint8_t* status) {
  SceneCtx S;
  init_ctx(S, d);
  const uint64_t n = (uint64_t)rows * cols;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads > 0 ? threads : 1)
  for (int64_t k = 0; k < (int64_t)n; ++k) {
    const Geometry& g = *S.g;
    Ray ray = make_ray(S, row0 + k / cols, col0 + k % cols, false, 0.0, 0.0);
    double* o = out + k * 5;
    for (int q = 0; q < 5; ++q) o[q] = 0.0;
    o[0] = std::fabs(g.inner_product(ray.position, ray.momentum, ray.momentum));
    std::vector<Step> steps;
    int stop;
    Counters cnt;
    Err e = integrate(g, S.cfg, ray, steps, &stop, &cnt);
    status[k] = (uint8_t)e;
    if (e != OK) continue;
    double c0[3] = {0, 0, 0}, c1[3];
    const int nc = g.constants_of_motion(steps[0].x, steps[0].p, c0);
    for (size_t i = 1; i < steps.size(); ++i) {
      double kk = std::fabs(g.inner_product(steps[i].x, steps[i].p, steps[i].p));
      if (kk > o[1]) o[1] = kk;
      g.constants_of_motion(steps[i].x, steps[i].p, c1);
      for (int q = 0; q < nc; ++q) {
        double drift = std::fabs(c0[q]) > 1e-12 ? std::fabs(c1[q] - c0[q]) / std::fabs(c0[q])
                                                 : std::fabs(c1[q] - c0[q]);
        if (drift > o[2 + q]) o[2 + q] = drift;
      }
    }
  }
}

// render_section_to_cie_buffer_raw (raytracer.rs:195-244) over a rectangle, or over an
// offset list when pixel_index != NULL (sample k = pixel pixel_index[k] at dx[k], dy[k]).
// OpenMP schedule(dynamic) mirrors rayon work stealing.  Returns wall seconds.
double oracle_render_pixels(const grt_scene_desc* d, uint32_t row0, uint32_t col0, uint32_t rows,
                            uint32_t cols, uint64_t n_offsets, const uint32_t* pixel_index,
                            const double* odx, const double* ody, const uint32_t* row_list,
                            uint32_t n_row_list, double* xyza, uint8_t* cls, uint8_t* status,
                            uint8_t* stop, uint32_t* steps, int threads, uint64_t* total_accepted,
                            uint64_t* total_attempts, uint32_t* hits) {
  SceneCtx S;
  init_ctx(S, d);
  // Work list: rectangle rows (or an explicit subset of rectangle rows) x cols, or offsets.
  uint64_t n;
  if (pixel_index) n = n_offsets;
  else if (row_list) n = (uint64_t)n_row_list * cols;
  else n = (uint64_t)rows * cols;
  std::atomic<uint64_t> acc(0), att(0);
  auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads > 0 ? threads : 1)
  for (int64_t i = 0; i < (int64_t)n; ++i) {
    int64_t row, col;
    bool off = false;
    double dx = 0, dy = 0;
    if (pixel_index) {
      row = row0 + pixel_index[i] / cols;
      col = col0 + pixel_index[i] % cols;
      off = true;
      dx = odx[i];
      dy = ody[i];
    } else if (row_list) {
      row = row0 + row_list[i / cols];
      col = col0 + i % cols;
    } else {
      row = row0 + i / cols;
      col = col0 + i % cols;
    }
    Sample s;
    Counters cnt;
    trace_one(S, row, col, off, dx, dy, &s, &cnt);
    acc += cnt.accepted;
    att += cnt.attempts;
    xyza[4 * i + 0] = s.color.x; xyza[4 * i + 1] = s.color.y;
    xyza[4 * i + 2] = s.color.z; xyza[4 * i + 3] = s.color.alpha;
    if (cls) cls[i] = (uint8_t)s.ray_class;
    if (status) status[i] = (uint8_t)s.status;
    if (stop) stop[i] = (uint8_t)s.stop;
    if (steps) steps[i] = (uint32_t)s.steps;
    if (hits) hits[i] = s.hits;
  }
  auto t1 = std::chrono::steady_clock::now();
  if (total_accepted) *total_accepted = acc.load();
  if (total_attempts) *total_attempts = att.load();
  return std::chrono::duration<double>(t1 - t0).count();
}

// render_section_to_cie_buffer[_supersampled] (raytracer.rs:177-318), whole pipeline.
// Returns the number of supersampled pixels.
uint64_t oracle_render_section(const grt_scene_desc* d, uint32_t from_row, uint32_t from_col,
                               uint32_t to_row, uint32_t to_col, const grt_adaptive_config* cfg,
                               const double* mask_xyza, double* out, uint8_t* cls_out, int threads) {
  SceneCtx S;
  init_ctx(S, d);
  uint32_t w = to_col - from_col, hgt = to_row - from_row;
  uint64_t n = (uint64_t)w * hgt;
  std::vector<Sample> buf(n);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads > 0 ? threads : 1)
  for (int64_t i = 0; i < (int64_t)n; ++i) {
    Counters c;
    trace_one(S, from_row + i / w, from_col + i % w, false, 0, 0, &buf[i], &c);
  }
  bool supersampled = cfg->enabled || mask_xyza != nullptr;
  for (uint64_t i = 0; i < n; ++i) {
    out[4 * i] = buf[i].color.x; out[4 * i + 1] = buf[i].color.y;
    out[4 * i + 2] = buf[i].color.z; out[4 * i + 3] = buf[i].color.alpha;
    if (cls_out) cls_out[i] = (uint8_t)buf[i].ray_class;
  }
  if (!supersampled) return 0;
  std::vector<uint64_t> sel;
  (void)select_pixels(buf, w, hgt, *cfg, &sel);
  if (mask_xyza) {
    for (uint64_t pi : sel) for (int k = 0; k < 4; ++k) out[4 * pi + k] = mask_xyza[k];
    return sel.size();
  }
  uint64_t spa = cfg->samples_per_axis;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads > 0 ? threads : 1)
  for (int64_t j = 0; j < (int64_t)sel.size(); ++j) {  // supersample :320-384
    uint64_t pi = sel[j];
    int64_t row = from_row + pi / w, col = from_col + pi % w;
    XYZA acc{0.0, 0.0, 0.0, 0.0};
    uint32_t valid = 0;
    for (uint64_t sr = 0; sr < spa; ++sr)
      for (uint64_t sc = 0; sc < spa; ++sc) {
        double dx, dy;
        stratified_sample_offset(row, col, sr, sc, spa, &dx, &dy);
        Sample s;
        Counters c;
        Ray ray = make_ray(S, row, col, true, dx, dy);
        Sample tmp;
        tmp.steps = 0;
        if (color_of_ray(S, ray, &tmp, &c) == OK) {
          acc = XYZA{acc.x + tmp.color.x, acc.y + tmp.color.y, acc.z + tmp.color.z, acc.alpha + tmp.color.alpha};
          valid++;
        }
        (void)s;
      }
    if (valid > 0) {
      double inv = 1.0 / (double)valid;
      out[4 * pi] = acc.x * inv; out[4 * pi + 1] = acc.y * inv;
      out[4 * pi + 2] = acc.z * inv; out[4 * pi + 3] = acc.alpha * inv;
    }
  }
  return sel.size();
}

// Reference unit test runge_kutta.rs:214-239 (d^2y/dt^2 = 2): integrate to t > t_end.
void oracle_rk_analytic(double t_end, double* y_out, double* t_out) {
  double y[2] = {1.0, 2.0};
  double t = 0.0, h = 0.0000001;
  auto f = [](const double* s, double* o) { o[0] = s[1]; o[1] = 2.0; };
  while (t <= t_end) {
    double yn[2];
    StepResult sr{0.0, 0.0, 0};
    rkf45<2>(y, h, 1e-10, f, yn, &sr);
    y[0] = yn[0]; y[1] = yn[1];
    t += sr.h_taken;
    h = sr.h_next;
  }
  y_out[0] = y[0]; y_out[1] = y[1];
  *t_out = t;
}

// Integrate one explicit ray (position/momentum in the native chart) — the
// integrator-level reference tests (schwarzschild.rs:874-939, kerr_bl.rs:1215-1344).
// Writes up to max_out steps of (t, x0..x3, p0..p3) and returns the step count.
int64_t oracle_integrate_ray(const grt_scene_desc* d, const double* position, const double* momentum,
                             double* out, int64_t max_out, int32_t* stop, int32_t* status) {
  SceneCtx S;
  init_ctx(S, d);
  Ray ray;
  ray.row = ray.col = 0;
  ray.position = Point{S.g->cs(), d->a, {position[0], position[1], position[2], position[3]}};
  ray.momentum = FourVector{S.g->cs(), {momentum[0], momentum[1], momentum[2], momentum[3]}};
  std::vector<Step> steps;
  int st = 0;
  Counters c;
  Err e = integrate(*S.g, S.cfg, ray, steps, &st, &c);
  *stop = st;
  *status = e;
  int64_t n = (int64_t)steps.size();
  for (int64_t i = 0; i < n && i < max_out; ++i) {
    out[9 * i] = steps[i].t;
    for (int k = 0; k < 4; ++k) out[9 * i + 1 + k] = steps[i].x.v[k];
    for (int k = 0; k < 4; ++k) out[9 * i + 5 + k] = steps[i].p.v[k];
  }
  return n;
}

// Camera ray (camera.rs:234-254): momentum of the traced ray.
void oracle_camera_ray(const grt_scene_desc* d, double row, double col, int use_offset, double dx,
                       double dy, double* momentum) {
  FourVector dir = use_offset ? get_direction_for(d->camera, row + (dy - 0.5), col + (dx - 0.5))
                              : get_direction_for(d->camera, row, col);
  for (int k = 0; k < 4; ++k) momentum[k] = dir.v[k] + (-d->camera.tetrad[0][k]);
}
void oracle_camera_direction(const grt_scene_desc* d, double row, double col, double* dir_out) {
  FourVector dir = get_direction_for(d->camera, row, col);
  for (int k = 0; k < 4; ++k) dir_out[k] = dir.v[k];
}
double oracle_inner_product(const grt_scene_desc* d, const double* position, const double* v, const double* w) {
  SceneCtx S;
  init_ctx(S, d);
  Point p{S.g->cs(), d->a, {position[0], position[1], position[2], position[3]}};
  FourVector fv{S.g->cs(), {v[0], v[1], v[2], v[3]}}, fw{S.g->cs(), {w[0], w[1], w[2], w[3]}};
  return S.g->inner_product(p, fv, fw);
}
void oracle_stratified_offset(int64_t row, int64_t col, uint64_t sr, uint64_t sc, uint64_t n, double* dx,
                              double* dy) {
  stratified_sample_offset(row, col, sr, sc, n, dx, dy);
}
void oracle_blend(const double* self_c, const double* other, double* out) {
  XYZA r = blend(XYZA{self_c[0], self_c[1], self_c[2], self_c[3]}, XYZA{other[0], other[1], other[2], other[3]});
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.alpha;
}
void oracle_texture_color(const grt_scene_desc* d, int object /* -1 = celestial */, double u, double v,
                          double redshift, double temperature, double* out) {
  TextureMap tm{object < 0 ? &d->celestial : &d->objects[object].texture, d};
  XYZA c = tm.color_at_uv(u, v, redshift, temperature);
  out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.alpha;
}
int oracle_killing_coefficients(double r_s, double a, double r, double* u_t, double* u_phi) {
  Killing k;
  Err e = killing_coefficients(r_s, a, r, &k);
  *u_t = k.u_t;
  *u_phi = k.u_phi;
  return e;
}
// Disc / sphere window test on two Cartesian points (sphere.rs:188-246 tests).
int oracle_object_intersects(const grt_scene_desc* d, int object, const double* a, const double* b,
                             double* point_out, double* t_out) {
  const grt_object_desc& o = d->objects[object];
  Point pa{CS::Cartesian, 0.0, {a[0], a[1], a[2], a[3]}}, pb{CS::Cartesian, 0.0, {b[0], b[1], b[2], b[3]}};
  Intersection in;
  bool hit;
  if (o.kind == GRT_OBJ_VOLUMETRIC_DISC) {
    VDisc V;
    V.init(&o);
    Vec3 vp{0.0, 0.0, 0.0}, dir;
    hit = V.intersects(spatial_cartesian(pa), spatial_cartesian(pb), &in.t, &vp, &dir);
    in.point = Point{CS::Cartesian, 0.0, {0.0, vp.x, vp.y, vp.z}};
  } else {
    hit = o.kind == GRT_OBJ_DISC ? disc_intersects(o, pa, pb, &in) : sphere_intersects(o, pa, pb, &in);
  }
  if (hit) {
    for (int k = 0; k < 4; ++k) point_out[k] = in.point.v[k];
    *t_out = in.t;
  }
  return hit ? 1 : 0;
}

// Array forms of the surface path's pieces (tests/surface_cases.py): n rows per call.
// a and b are n x 3 Cartesian points; object is a Disc or a Sphere; hit[n], t[n], point[n x 3]
// (the world point, as disc_intersects and sphere_intersects return it); 0 where no hit
void oracle_object_intersects_n(const grt_scene_desc* d, int object, uint64_t n, const double* a, const double* b,
                                uint8_t* hit, double* t, double* point) {
  const grt_object_desc& o = d->objects[object];
  for (uint64_t i = 0; i < n; ++i) {
    Point pa{CS::Cartesian, 0.0, {0.0, a[3 * i], a[3 * i + 1], a[3 * i + 2]}};
    Point pb{CS::Cartesian, 0.0, {0.0, b[3 * i], b[3 * i + 1], b[3 * i + 2]}};
    Intersection in;
    bool h = o.kind == GRT_OBJ_DISC ? disc_intersects(o, pa, pb, &in) : sphere_intersects(o, pa, pb, &in);
    hit[i] = h ? 1 : 0;
    t[i] = h ? in.t : 0.0;
    for (int k = 0; k < 3; ++k) point[3 * i + k] = h ? in.point.v[k + 1] : 0.0;
  }
}
// to_cartesian (point.rs:125-154) of n native-chart positions (r, theta, phi) -- (x, y, z) on the
// Cartesian charts: xyz[n x 3]
void oracle_to_cartesian_n(const grt_scene_desc* d, uint64_t n, const double* pos, double* xyz) {
  SceneCtx S;
  init_ctx(S, d);
  for (uint64_t i = 0; i < n; ++i) {
    const double p[4] = {0.0, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    Point c = to_cartesian(S.g->make_point(p));
    for (int k = 0; k < 3; ++k) xyz[3 * i + k] = c.v[k + 1];
  }
}
// compute_temperature of the object per radius: status[n] (grt_status), value[n] (0 where not OK)
void oracle_compute_temperature_n(const grt_scene_desc* d, int object, uint64_t n, const double* radius,
                                  int32_t* status, double* value) {
  for (uint64_t i = 0; i < n; ++i) {
    double v = 0.0;
    Err e = compute_temperature(d->objects[object], radius[i], &v);
    status[i] = e;
    value[i] = e == OK ? v : 0.0;
  }
}
// sample_blackbody per temperature, out[n x 4]; log_t == NULL: std::log10, else log_t[i] in its place
void oracle_blackbody_n(const grt_scene_desc* d, uint64_t n, const double* temperature, const double* log_t,
                        double* out) {
  TextureMap tm{&d->celestial, d};
  for (uint64_t i = 0; i < n; ++i) {
    XYZA c = tm.sample_blackbody(temperature[i], log_t ? log_t + i : nullptr);
    out[4 * i] = c.x; out[4 * i + 1] = c.y; out[4 * i + 2] = c.z; out[4 * i + 3] = c.alpha;
  }
}
// color_at_uv per row uvzt[4 i ..] = (u, v, redshift, temperature), object -1 = celestial; log_t as
// in oracle_blackbody_n (of temperature * redshift; read by a blackbody texture only)
void oracle_texture_color_n(const grt_scene_desc* d, int object, uint64_t n, const double* uvzt, const double* log_t,
                            double* out) {
  TextureMap tm{object < 0 ? &d->celestial : &d->objects[object].texture, d};
  for (uint64_t i = 0; i < n; ++i) {
    const double* q = uvzt + 4 * i;
    XYZA c = tm.color_at_uv(q[0], q[1], q[2], q[3], log_t ? log_t + i : nullptr);
    out[4 * i] = c.x; out[4 * i + 1] = c.y; out[4 * i + 2] = c.z; out[4 * i + 3] = c.alpha;
  }
}
void oracle_blend_n(uint64_t n, const double* self_c, const double* other, double* out) {
  for (uint64_t i = 0; i < n; ++i) oracle_blend(self_c + 4 * i, other + 4 * i, out + 4 * i);
}

// ---- VolumetricDisc pieces (volumetric_disc.rs tests, :693-786) ----
void oracle_perlin_table(uint32_t seed, uint8_t* out) { noise09::permutation_table(seed, out); }
double oracle_perlin(uint32_t seed, double x, double y, double z) {
  uint8_t P[256];
  noise09::permutation_table(seed, P);
  return noise09::perlin_3d(P, x, y, z);
}
double oracle_vdisc_density(const grt_scene_desc* d, int object, const double* p) {
  VDisc V;
  V.init(&d->objects[object]);
  return V.compute_density(Vec3{p[0], p[1], p[2]});
}
// raymarch_constant_step_internal with frequency (observer_energy, p_t, p_phi); returns
// the propagated error (0 = Ok) and the colour in out4.
int oracle_vdisc_raymarch(const grt_scene_desc* d, int object, const double* ro, const double* rd,
                          const double* freq3, int use_cached_exit, double* out4, uint64_t* samples) {
  SceneCtx S;
  init_ctx(S, d);
  FrequencyData f{freq3[0], freq3[1], freq3[2]};
  XYZA c{0.0, 0.0, 0.0, 0.0};
  uint64_t n = 0;
  Err e = vdisc_raymarch(S.vd[object], S.obj_tex[object], *S.g, d->geometry, Vec3{ro[0], ro[1], ro[2]},
                         Vec3{rd[0], rd[1], rd[2]}, f, use_cached_exit != 0, &c, &n);
  out4[0] = c.x;
  out4[1] = c.y;
  out4[2] = c.z;
  out4[3] = c.alpha;
  if (samples) *samples = n;
  return e;
}

// compute_density with the in-plane angle phi given by the caller in place of std::atan2.
double oracle_vdisc_density_phi(const grt_scene_desc* d, int object, const double* p, double phi) {
  VDisc V;
  V.init(&d->objects[object]);
  return V.compute_density(Vec3{p[0], p[1], p[2]}, &phi);
}
// precompute_exit_distance alone: 1 and *out when a crossing lies within max_steps * step_size.
int oracle_vdisc_exit_distance(const grt_scene_desc* d, int object, const double* ro, const double* rd, double* out) {
  VDisc V;
  V.init(&d->objects[object]);
  double e = 0.0;
  bool f = V.precompute_exit_distance(Vec3{ro[0], ro[1], ro[2]}, Vec3{rd[0], rd[1], rd[2]}, &e);
  *out = f ? e : 0.0;
  return f ? 1 : 0;
}
// Array forms: n inputs per call (xyz / p / ro / rd are n x 3, row-major).
void oracle_perlin_n(uint32_t seed, uint64_t n, const double* xyz, double* out) {
  uint8_t P[256];
  noise09::permutation_table(seed, P);
  for (uint64_t i = 0; i < n; ++i) out[i] = noise09::perlin_3d(P, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}
// phi == NULL: oracle_vdisc_density; else oracle_vdisc_density_phi with phi[i]
void oracle_vdisc_density_n(const grt_scene_desc* d, int object, uint64_t n, const double* p, const double* phi,
                            double* out) {
  VDisc V;
  V.init(&d->objects[object]);
  for (uint64_t i = 0; i < n; ++i)
    out[i] = V.compute_density(Vec3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}, phi ? phi + i : nullptr);
}
// compute_density's in-plane coordinates xy[2 i ..] = (x_local, y_local) and noise[i] = whether the point
// reached the noise (inside rin .. rout with a vertical falloff >= 0.001); xy is (0, 0) where it did not
void oracle_vdisc_plane_n(const grt_scene_desc* d, int object, uint64_t n, const double* p, double* xy, uint8_t* noise) {
  VDisc V;
  V.init(&d->objects[object]);
  for (uint64_t i = 0; i < n; ++i) {
    bool f = false;
    xy[2 * i] = xy[2 * i + 1] = 0.0;
    V.compute_density(Vec3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}, nullptr, xy + 2 * i, &f);
    noise[i] = f ? 1 : 0;
  }
}
// the density at p + k * step * rd for k = 0 .. steps (steps + 1 samples): nonzero[i] = any of them > 0
void oracle_vdisc_density_along_n(const grt_scene_desc* d, int object, uint64_t n, const double* p, const double* rd,
                                  double step, uint64_t steps, uint8_t* nonzero) {
  VDisc V;
  V.init(&d->objects[object]);
  for (uint64_t i = 0; i < n; ++i) {
    uint8_t any = 0;
    for (uint64_t k = 0; k <= steps && !any; ++k) {
      double t = (double)k * step;
      Vec3 q{p[3 * i] + rd[3 * i] * t, p[3 * i + 1] + rd[3 * i + 1] * t, p[3 * i + 2] + rd[3 * i + 2] * t};
      any = V.compute_density(q) > 0.0;
    }
    nonzero[i] = any;
  }
}
void oracle_vdisc_exit_distance_n(const grt_scene_desc* d, int object, uint64_t n, const double* ro, const double* rd,
                                  uint8_t* found, double* out) {
  for (uint64_t i = 0; i < n; ++i) found[i] = (uint8_t)oracle_vdisc_exit_distance(d, object, ro + 3 * i, rd + 3 * i, out + i);
}
// a and b are n x 3 Cartesian points; hit[n], t[n], point[n x 3]
void oracle_vdisc_intersects_n(const grt_scene_desc* d, int object, uint64_t n, const double* a, const double* b,
                               uint8_t* hit, double* t, double* point) {
  VDisc V;
  V.init(&d->objects[object]);
  for (uint64_t i = 0; i < n; ++i) {
    Vec3 vp{0.0, 0.0, 0.0}, dir;
    double ti = 0.0;
    bool h = V.intersects(Vec3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}, Vec3{b[3 * i], b[3 * i + 1], b[3 * i + 2]}, &ti, &vp, &dir);
    hit[i] = h ? 1 : 0;
    t[i] = h ? ti : 0.0;
    point[3 * i] = h ? vp.x : 0.0;
    point[3 * i + 1] = h ? vp.y : 0.0;
    point[3 * i + 2] = h ? vp.z : 0.0;
  }
}
// oracle_vdisc_raymarch over n jobs (one scene context): object[n], ro / rd / freq n x 3, err[n], out n x 4, samples[n]
void oracle_vdisc_raymarch_n(const grt_scene_desc* d, uint64_t n, const uint32_t* object, const double* ro,
                             const double* rd, const double* freq, int use_cached_exit, int32_t* err, double* out,
                             uint64_t* samples) {
  SceneCtx S;
  init_ctx(S, d);
  for (uint64_t i = 0; i < n; ++i) {
    FrequencyData f{freq[3 * i], freq[3 * i + 1], freq[3 * i + 2]};
    XYZA c{0.0, 0.0, 0.0, 0.0};
    uint64_t ns = 0;
    const uint32_t k = object[i];
    err[i] = vdisc_raymarch(S.vd[k], S.obj_tex[k], *S.g, d->geometry, Vec3{ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]},
                            Vec3{rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]}, f, use_cached_exit != 0, &c, &ns);
    out[4 * i] = c.x;
    out[4 * i + 1] = c.y;
    out[4 * i + 2] = c.z;
    out[4 * i + 3] = c.alpha;
    samples[i] = ns;
  }
}

// ---- output stage (color.rs:193-298), as Raytracer::render_section calls it for
// non-HDR files (raytracer.rs:481-487): xyz_to_linear_srgb_buffer, then
// linear_srgb_to_srgb_buffer(.., exposure, tone_mapping).
static double out_compand_srgb(double linear) {  // color.rs:193-202
  double sign = linear < 0.0 ? -1.0 : 1.0;
  double a = std::fabs(linear);
  double encoded = a <= 0.003'130'8 ? 12.92 * a : 1.055 * std::pow(a, 1.0 / 2.4) - 0.055;
  double v = sign * encoded;
  return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);  // f64::clamp
}
static uint8_t out_round_u8(double v) {  // (v * 255.0).round() as u8
  double r = std::round(v * 255.0);
  if (std::isnan(r) || r <= 0.0) return 0;
  return r >= 255.0 ? 255 : (uint8_t)r;
}
void oracle_xyz_to_srgb8(const double* xyza, uint64_t n, int tone, double exposure, uint8_t* rgb) {
  static const double M[3][3] = {{3.240'625'5, -1.537'208'0, -0.498'628'6},
                                 {-0.968'930'7, 1.875'756'1, 0.041'517'5},
                                 {0.055'710'1, -0.204'021'1, 1.056'995'9}};
  std::vector<std::array<double, 3>> lin(n);
  for (uint64_t i = 0; i < n; ++i)  // m * v: nalgebra gemv, column by column
    for (int r = 0; r < 3; ++r) {
      double acc = M[r][0] * xyza[4 * i];
      acc = M[r][1] * xyza[4 * i + 1] + acc;
      acc = M[r][2] * xyza[4 * i + 2] + acc;
      lin[i][r] = acc;
    }
  double scale = 1.0;
  if (tone == 1) {  // GlobalLinear: fold(0.0, f64::max) per channel
    double mx[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k)
      for (uint64_t i = 0; i < n; ++i) mx[k] = std::fmax(mx[k], lin[i][k] * exposure);
    double max_component = std::fmax(std::fmax(mx[0], mx[1]), mx[2]);
    scale = max_component > 0.0 ? 1.0 / max_component : 1.0;
  }
  for (uint64_t i = 0; i < n; ++i) {
    double c[3] = {lin[i][0] * exposure, lin[i][1] * exposure, lin[i][2] * exposure};
    if (tone == 0) {  // Reinhard on luminance
      double l_in = 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2];
      if (l_in > 0.0) {
        double l_out = l_in / (1.0 + l_in);
        double f = l_out / l_in;
        for (int k = 0; k < 3; ++k) c[k] = c[k] * f;
      }
    } else {
      for (int k = 0; k < 3; ++k) c[k] = scale * c[k];
    }
    for (int k = 0; k < 3; ++k) rgb[3 * i + k] = out_round_u8(out_compand_srgb(std::fmax(c[k], 0.0)));
  }
}


// ---- geometry probes for the reference's unit tests (tests/test_reference_kats.py) ----
// Each builds the scene's Geometry from the descriptor (geometry, radius, a,
// horizon_epsilon) and calls one of the functions the path uses.
int oracle_should_stop(const grt_scene_desc* d, const double* y, uint64_t i) {  // integrator.rs:203-268
  SceneCtx S;
  init_ctx(S, d);
  return should_stop(*S.g, S.cfg, y, i);
}
int oracle_inside_horizon(const grt_scene_desc* d, const double* pos) {
  SceneCtx S;
  init_ctx(S, d);
  return S.g->inside_horizon(S.g->make_point(pos)) ? 1 : 0;
}
// radial_coordinate of a native-chart point, or of a Cartesian one (cartesian != 0)
double oracle_radial_coordinate(const grt_scene_desc* d, const double* pos, int cartesian) {
  SceneCtx S;
  init_ctx(S, d);
  Point p = cartesian ? Point{CS::Cartesian, d->a, {pos[0], pos[1], pos[2], pos[3]}} : S.g->make_point(pos);
  return S.g->radial_coordinate(p);
}
void oracle_to_cartesian(const grt_scene_desc* d, const double* pos, double* out) {  // point.rs:125-154
  SceneCtx S;
  init_ctx(S, d);
  Point c = to_cartesian(S.g->make_point(pos));
  for (int k = 0; k < 4; ++k) out[k] = c.v[k];
}
void oracle_stationary_velocity(const grt_scene_desc* d, const double* pos, double* out) {
  SceneCtx S;
  init_ctx(S, d);
  FourVector u = S.g->stationary_velocity(S.g->make_point(pos));
  for (int k = 0; k < 4; ++k) out[k] = u.v[k];
}
int oracle_circular_orbit_velocity(const grt_scene_desc* d, const double* pos, double* out) {
  SceneCtx S;
  init_ctx(S, d);
  FourVector u{S.g->cs(), {0, 0, 0, 0}};
  Err e = S.g->circular_orbit_velocity(S.g->make_point(pos), &u);
  for (int k = 0; k < 4; ++k) out[k] = u.v[k];
  return e;
}
// The solver of the ray (pos, mom): create_initial_state -> y0, apply(y_in or y0) ->
// rhs, momentum_from_state(y_in or y0) -> p.  y_in may be NULL.
void oracle_geodesic_rhs(const grt_scene_desc* d, const double* pos, const double* mom, const double* y_in,
                         double* y0, double* rhs, double* p) {
  SceneCtx S;
  init_ctx(S, d);
  Ray ray;
  ray.row = ray.col = 0;
  ray.position = S.g->make_point(pos);
  ray.momentum = FourVector{S.g->cs(), {mom[0], mom[1], mom[2], mom[3]}};
  std::unique_ptr<GeodesicSolver> sol = S.g->solver(ray);
  sol->create_initial_state(ray, y0);
  const double* y = y_in ? y_in : y0;
  sol->apply(y, rhs);
  FourVector f = sol->momentum_from_state(y);
  for (int k = 0; k < 4; ++k) p[k] = f.v[k];
}
// kerr.rs:49-110 metric / metric_contravariant; kerr_bl.rs:253-272 metric_bl
void oracle_ks_metric(double radius, double a, double x, double y, double z, int contravariant, double* g) {
  Mat4 m = contravariant ? ks_metric_contravariant(radius, a, x, y, z) : ks_metric(radius, a, x, y, z);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) g[4 * i + j] = m.m[i][j];
}
void oracle_bl_metric(double r_s, double a, double r, double theta, double* g) {
  Mat4 m = metric_bl(r_s, a, r, theta);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) g[4 * i + j] = m.m[i][j];
}
// RedshiftComputer::compute_redshift (redshift.rs:31-38, :62-73): static emitter at pos
double oracle_redshift_static(const grt_scene_desc* d, const double* pos, const double* mom, double observer_energy) {
  SceneCtx S;
  init_ctx(S, d);
  Point p = S.g->make_point(pos);
  FourVector m{S.g->cs(), {mom[0], mom[1], mom[2], mom[3]}};
  double emitter_energy = S.g->inner_product(p, S.g->stationary_velocity(p), m);
  double sig0 = S.g->signature0();
  return (sig0 * observer_energy) / (sig0 * emitter_energy);
}
// KerrBLSolver::geodesic (kerr_bl.rs:141-174) with explicit constants of motion
void oracle_kerr_bl_rhs(double r_s, double a, double e, double l_z, double q, const double* y, double* out) {
  KerrBLSolver sol;
  sol.radius = r_s;
  sol.a = a;
  sol.e = e;
  sol.l_z = l_z;
  sol.q = q;
  sol.apply(y, out);
}
// should_supersample_pair (raytracer.rs:91-108) on two (XYZA, class) samples
int oracle_should_supersample_pair(const double* p, int pc, const double* q, int qc, const grt_adaptive_config* c,
                                   double min_lum) {
  Sample a, b;
  a.color = XYZA{p[0], p[1], p[2], p[3]};
  a.ray_class = pc;
  b.color = XYZA{q[0], q[1], q[2], q[3]};
  b.ray_class = qc;
  return should_supersample_pair(a, b, *c, min_lum) ? 1 : 0;
}
// collect_pixels_to_supersample applied to a given 1-spp section buffer (f64 XYZA + class,
// row-major w x h): flags_out[i] = 1 for the selected pixels.  Returns the luminance floor.
double oracle_select_pixels(const double* xyza, const uint8_t* cls, uint32_t w, uint32_t h,
                            const grt_adaptive_config* cfg, uint8_t* flags_out) {
  const uint64_t n = (uint64_t)w * h;
  std::vector<Sample> buf(n);
  for (uint64_t i = 0; i < n; ++i) {
    buf[i].color = XYZA{xyza[4 * i], xyza[4 * i + 1], xyza[4 * i + 2], xyza[4 * i + 3]};
    buf[i].ray_class = cls[i];
  }
  std::vector<uint64_t> sel;
  double min_lum = select_pixels(buf, w, h, *cfg, &sel);
  std::memset(flags_out, 0, n);
  for (uint64_t pi : sel) flags_out[pi] = 1;
  return min_lum;
}
// ---- host setup, restated (host_setup.inc) ----
int oracle_camera_setup(int32_t geometry, double radius, double a, const double* cart, int velocity_mode,
                        const double* explicit_velocity, double alpha, int64_t rows, int64_t cols, double phi,
                        double theta, double psi, grt_camera_desc* out) {
  return setup::camera_setup(geometry, radius, a, cart, velocity_mode, explicit_velocity, alpha, rows, cols, phi,
                             theta, psi, out);
}
int oracle_kerr_temperature_lut(double temperature, double outer_radius, double a, double radius, uint32_t n,
                                double* lut_r, double* lut_t, double* r_isco) {
  if (n < 2) return -EINVAL;
  return setup::kerr_temperature_lut(temperature, outer_radius, a, radius, n, lut_r, lut_t, r_isco);
}
double oracle_r_isco(double radius, double a) { return setup::r_isco(radius, a); }
int oracle_blackbody_lut(uint32_t n, double* log_t, double* xyz) {
  if (n < 2) return -EINVAL;
  setup::blackbody_lut(n, log_t, xyz);
  return 0;
}
void oracle_blackbody_xyz(double temperature, double redshift, double* out) {
  setup::blackbody_xyz(temperature, redshift, out);
}
}  // extern "C"

