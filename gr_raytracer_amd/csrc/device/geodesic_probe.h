// geodesic_probe.h — a layer of geodesic.hip: the work-order kernels, which only decide the
// order of the tile queue (schedule.hip), never a result: the step probes (probe_kernel,
// probe_quad_kernel) and the Schwarzschild keys without a probe (impact_key_kernel,
// class_key_kernel).  Included by the exact build and the sequence unit, after
// the trace kernels.

// ============================================================ probe kernel =======
// Work-order probe (scheduling only, never an output): one ray per 8x8 tile, the
// tile's pixel (3, 3), integrated for at most `cap` accepted steps.  A frame's cost is
// heavy-tailed where rays spiral into the horizon or orbit near the photon sphere
// (C4: 6% of the rays carry 60% of the steps, up to max_steps each); with the counts
// the host queues the long tiles first, so the frame does not end on a lone ray that
// started late.  Writes the steps taken, or for a probe still going at the cap a key
// above every finished count: cap + 2^30 (r - r_stop) / r_stop, r its radial coordinate
// there and r_stop the horizon test's radius (cap alone without a horizon).  The capped
// probes of a C4 shard all creep towards the horizon with steps of ~1e-8, and the
// distance they have left predicts the ray's length (log-log correlation 0.98 with the
// probe pixel's own count; the 300 tiles with a ray past 8e5 steps are among the 311
// largest keys but 11; tools/c4_probe_features.py), so the longest tiles are queued first.
//
// GRT_PROBE_ESCAPE: a Kerr-Schild probe moving outward beyond min(10 radius,
// max_radius / 2) escapes (no turning point outside the photon orbits); its key becomes
// cap - 1: below every capped probe's key (those rays are longer), above the rays that
// fell in early, and "finished" for the edge-tile rule (schedule.hip).  So the cap
// (api.hip probe_cap) need not outlast the escaping rays, and the pass ends sooner.
// Scheduling only, never an output.
template <int G>
GDEV bool probe_escaped(const DevScene& S, const double* y, double& r_prev, uint32_t cap, uint32_t* key) {
  if constexpr (G != GRT_GEOM_KERR || !GRT_PROBE_ESCAPE) {
    return false;
  } else {
    const double r = sqrt(ks_r_sqr(S.a, y[1], y[2], y[3]));
    const bool out = r > fmin(10.0 * S.radius, 0.5 * sqrt(S.max_radius_sq)) && r > r_prev;
    r_prev = r;
    if (out) *key = cap - 1;
    return out;
  }
}

// The probe's radial coordinate at its initial state, so that the first accepted step's
// "moving outward" test compares against where the ray started (a camera far from the
// hole, beyond the escape radius, must not end its inward probes at step 1).
template <int G>
GDEV double probe_r0(const DevScene& S, const double* y) {
  if constexpr (G != GRT_GEOM_KERR || !GRT_PROBE_ESCAPE) {
    return 0.0;
  } else {
    return sqrt(ks_r_sqr(S.a, y[1], y[2], y[3]));
  }
}

template <int G>
__global__ void __launch_bounds__(64) probe_kernel(const DevScene* __restrict__ Sp, WorkList wl, uint32_t n_tiles,
                                                   uint32_t cap, uint32_t* __restrict__ steps_out CAMS_PARAM) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles) return;
  const uint32_t tr = t / wl.tiles_x, tc = t % wl.tiles_x;
  const uint32_t r = min(tr * 8 + 3, wl.rows - 1), c = min(tc * 8 + 3, wl.cols - 1);
  double y[8];
  RayConst rc;
  init_rect_ray<G>(S, wl, r, c, y, rc CAMS_ARG);
  const uint64_t end = S.max_steps < (uint64_t)cap ? S.max_steps : (uint64_t)cap;
  uint64_t i = 1;
  double h = S.step_size;
  double r_prev = probe_r0<G>(S, y);
  uint32_t key = 0;
  bool escaped = false;
  for (; i < end; ++i) {
    double h_cur = rclamp(h, H_MIN, H_MAX), h_next = 0.0, yn[8];
    int retries = 0, ctl;
    do {
      const double err_sq = rkf_attempt<G>(S, rc, y, h_cur, yn);
      ctl = step_control(S, err_sq, h_cur, retries, h_next);
    } while (ctl == STEP_RETRY);
    if (ctl == STEP_FAILED) break;
    h = h_next;
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = yn[k];
    double cc[3];
    bool c_valid = false;
    if (should_stop<G>(S, y, cc, c_valid, i) != GRT_STOP_NONE) break;
    if ((escaped = probe_escaped<G>(S, y, r_prev, cap, &key))) break;
  }
  if (!escaped) key = (uint32_t)i;
  if (!escaped && i >= end) {
    key = cap;
    const bool horizon = G == GRT_GEOM_SCHWARZSCHILD || ((G == GRT_GEOM_KERR || G == GRT_GEOM_KERR_BL) && S.has_horizon);
    if (horizon && S.horizon_r > 0.0) {
      const double rad = (G == GRT_GEOM_KERR) ? sqrt(ks_r_sqr(S.a, y[1], y[2], y[3])) : y[1];
      const double d = (rad - S.horizon_r) / S.horizon_r * 1073741824.0;
      if (d > 0.0) key = cap + (uint32_t)fmin(d, (double)(0xffffffffu - cap));  // NaN: stays cap
    }
  }
  steps_out[t] = key;
}

// Work-order key of a Schwarzschild tile without integrating: the predicted steps of its
// probe pixel's ray from the impact parameter b = L / E of its initial momentum (E =
// (1 - r_s / r) dt/dl, L = r^2 sqrt((dtheta/dl)^2 + sin^2 theta (dphi/dl)^2)).  A ray with
// b above the photon orbit's b_c = (3 sqrt 3 / 2) r_s escapes to the celestial sphere
// (~max_radius unit steps), one below it falls in (a few hundred steps), and near b_c
// both wind round the photon sphere for ~ln(1 / |b / b_c - 1|) more turns.  Only the
// queue order depends on it, never a result.
__global__ void __launch_bounds__(64) impact_key_kernel(const DevScene* __restrict__ Sp, WorkList wl,
                                                        uint32_t n_tiles, uint32_t* __restrict__ keys_out CAMS_PARAM) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles) return;
  const uint32_t tr = t / wl.tiles_x, tc = t % wl.tiles_x;
  const uint32_t r = min(tr * 8 + 3, wl.rows - 1), c = min(tc * 8 + 3, wl.cols - 1);
  double y[8];
  RayConst rc;
  init_rect_ray<GRT_GEOM_SCHWARZSCHILD>(S, wl, r, c, y, rc CAMS_ARG);
  const double rs = S.radius, rr = y[1], sn = sin(y[2]);
  const double e = fabs((1.0 - rs / rr) * y[4]);
  const double l = rr * rr * sqrt(y[6] * y[6] + sn * sn * y[7] * y[7]);
  const double bc = 2.598076211353316 * rs;
  const double b = l / e;
  const double x = fmax(fabs(b - bc) / bc, 1e-12);
  const double len = (b > bc ? sqrt(S.max_radius_sq) : 300.0) + 700.0 * fmax(0.0, -log(x));
  keys_out[t] = (len > 0.0 && len < 4.0e9) ? (uint32_t)len : (len >= 4.0e9 ? 4000000000u : 0u);  // NaN: 0
}

// Where a Schwarzschild camera ray ends up, without the chart integration: pi/2 - theta_f
// of its asymptotic direction, for the corner pixels (8i, 8j) of the tile grid (clamped to
// the frame).  In the far field a ray's theta is constant to O(b / r), so for nearly all
// of its steps the RHS's sincos takes the case theta_f falls in (glibc_math.h: Taylor
// within TAYLOR_MAX of pi/2, table elsewhere in region B), and a wave whose lanes agree
// on the case runs one straight-line form (rhs path 12 / 13) instead of the general one.
// schedule.hip groups the tiles by it.  The ray moves in the plane of its position and
// its tangential momentum; with psi the angle swept in that plane, u = 1 / r obeys
// u'' = -u + 1.5 r_s u^2 (fixed-step RK4 here), u(0) = 1 / r_0, u'(0) = -(dr/dl) / L with
// L = r^2 dpsi/dl.  The direction after psi is cos(psi) n_0 + sin(psi) t_0 (n_0 the
// camera's position direction, t_0 the tangential momentum's), hence theta_f.
// Out: pi/2 - theta_f; CLASS_CAPTURED for a ray that reaches the horizon; NaN for one
// still winding after CLASS_STEPS steps.  Only the queue order depends on it, never a result.
constexpr float CLASS_CAPTURED = 1.0e30f;
constexpr int CLASS_STEPS = 400;
constexpr double CLASS_DPSI = 0.03125;  // 400 steps: 12.5 rad, two turns round the hole
__global__ void __launch_bounds__(64) class_key_kernel(const DevScene* __restrict__ Sp, WorkList wl,
                                                       uint32_t corners_x, uint32_t n_corners,
                                                       float* __restrict__ a_out CAMS_PARAM) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_corners) return;
  const uint32_t r = min((t / corners_x) * 8, wl.rows - 1), c = min((t % corners_x) * 8, wl.cols - 1);
  double y[8];
  RayConst rc;
  init_rect_ray<GRT_GEOM_SCHWARZSCHILD>(S, wl, r, c, y, rc CAMS_ARG);
  const double rs = S.radius, st0 = sin(y[2]), ct0 = cos(y[2]);
  const double tang = sqrt(y[6] * y[6] + st0 * st0 * y[7] * y[7]);  // dpsi/dl
  const double l = y[1] * y[1] * tang;
  const double u_hor = 1.0 / rs;
  double u = 1.0 / y[1], v = -y[5] / l, psi = 0.0;
  float a = __builtin_nanf("");
  if (!(l > 0.0) || !isfinite(v)) {  // a radial ray keeps its direction, or falls in
    a_out[t] = y[5] > 0.0 ? (float)(1.5707963267948966 - y[2]) : CLASS_CAPTURED;
    return;
  }
  auto acc = [rs](double uu) { return -uu + 1.5 * rs * uu * uu; };
  for (int k = 0; k < CLASS_STEPS; ++k) {
    const double h = CLASS_DPSI;
    const double k1u = v, k1v = acc(u);
    const double k2u = v + 0.5 * h * k1v, k2v = acc(u + 0.5 * h * k1u);
    const double k3u = v + 0.5 * h * k2v, k3v = acc(u + 0.5 * h * k2u);
    const double k4u = v + h * k3v, k4v = acc(u + h * k3u);
    const double un = u + h / 6.0 * (k1u + 2.0 * k2u + 2.0 * k3u + k4u);
    const double vn = v + h / 6.0 * (k1v + 2.0 * k2v + 2.0 * k3v + k4v);
    if (!(un > 0.0)) {  // escaped within this step: psi where u crosses 0
      psi += h * u / (u - un);
      // t_0's z component: the theta part of the tangential momentum, e_theta . z = -sin(theta)
      const double tz = -st0 * (y[6] / tang);
      const double nz = fmin(1.0, fmax(-1.0, cos(psi) * ct0 + sin(psi) * tz));
      a = (float)(1.5707963267948966 - acos(nz));
      break;
    }
    if (un >= u_hor) {
      a = CLASS_CAPTURED;
      break;
    }
    u = un;
    v = vn;
    psi += h;
  }
  a_out[t] = a;
}

// probe_kernel<KERR> with each probe ray on the 4 lanes of a quad (rhs_ks_quad, as in
// tail_kernel): the same operations on the same values, so the same keys (GPU test
// tests/test_gpu_schedule.py).  For a pass of few probe rays (a 1/8 row-band shard of
// C4: 32,768 tiles, 0.5 waves per SIMD as one lane each) the pass lasts as long as its
// capped probes take to run `cap` steps at one wave's latency; splitting each RHS over a
// quad cuts that latency, at 4x the lanes (2 waves per SIMD here).
// The loop and the key rules are probe_kernel's, written out a second time: shared through
// a device function both kernels compile to other code, and as one kernel template they
// get other names and places in the code object.
__global__ void __launch_bounds__(256, 2) probe_quad_kernel(const DevScene* __restrict__ Sp, WorkList wl,
                                                            uint32_t n_tiles, uint32_t cap,
                                                            uint32_t* __restrict__ steps_out CAMS_PARAM) {
  constexpr int G = GRT_GEOM_KERR;
  const DevScene& S = *Sp;
  glibc::tables_to_lds();
  const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;  // the quad's tile
  const int sub = threadIdx.x & 3;
  if (t >= n_tiles) return;  // the whole quad
  const uint32_t tr = t / wl.tiles_x, tc = t % wl.tiles_x;
  const uint32_t r = min(tr * 8 + 3, wl.rows - 1), c = min(tc * 8 + 3, wl.cols - 1);
  double y[8];
  RayConst rc;
  init_rect_ray<G>(S, wl, r, c, y, rc CAMS_ARG);
  const uint64_t end = S.max_steps < (uint64_t)cap ? S.max_steps : (uint64_t)cap;
  uint64_t i = 1;
  double h = S.step_size;
  double r_prev = probe_r0<G>(S, y);
  uint32_t key = 0;
  bool escaped = false;
  for (; i < end; ++i) {  // identical decisions in the quad's four lanes
    double h_cur = rclamp(h, H_MIN, H_MAX), h_next = 0.0, yn[8];
    int retries = 0, ctl;
    do {
      const double err_sq = rkf_attempt<G, false, true>(S, rc, y, h_cur, yn, sub);
      ctl = step_control(S, err_sq, h_cur, retries, h_next);
    } while (ctl == STEP_RETRY);
    if (ctl == STEP_FAILED) break;
    h = h_next;
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = yn[k];
    double cc[3];
    bool c_valid = false;
    if (should_stop<G>(S, y, cc, c_valid, i) != GRT_STOP_NONE) break;
    if ((escaped = probe_escaped<G>(S, y, r_prev, cap, &key))) break;
  }
  if (!escaped) key = (uint32_t)i;
  if (!escaped && i >= end) {
    key = cap;
    if (S.has_horizon && S.horizon_r > 0.0) {
      const double d = (sqrt(ks_r_sqr(S.a, y[1], y[2], y[3])) - S.horizon_r) / S.horizon_r * 1073741824.0;
      if (d > 0.0) key = cap + (uint32_t)fmin(d, (double)(0xffffffffu - cap));  // NaN: stays cap
    }
  }
  if (sub == 0) steps_out[t] = key;
}
