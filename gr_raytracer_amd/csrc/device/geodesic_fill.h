// geodesic_fill.h — a layer of geodesic.hip: the geometry buffer's fill.  Included by the
// exact units (the exact build, the KerrBL unit, the sequence unit, the lapse unit; not the fused one),
// after the shade kernel.

// ============================================================ geometry buffer =====
// After a 1-spp trace of a rectangle whose outputs (status, stop) are gb's: the numbers
// shade_kernel<G, 0> reduces each ray to before any texture or temperature is applied --
// per window-nearest hit (a "layer", front to back) its object and shade_record's (u, v,
// redshift, radius), at layer_start[idx] + k; per ray that ended on the celestial sphere
// celestial_args' (1 - u, v, redshift).  The same record walk as shade_kernel; one lane per
// ray.  A ray whose status is not 0 has no layers (layer_start is the scan of the trace's
// own hit counts, zeroed for those rays).  The sequence unit's (grt_gbuffer_trace_sequence)
// fills the buffer of a whole stack: slot idx is a ray of frame idx / (rows * cols), and its
// camera is that frame's (observer_energy).  The lapse unit's (grt_gbuffer_trace_lapse) also
// writes each layer's lapse: the coordinate time the trace kept beside the layer's record
// (window_pass) minus the camera's, the y[0] the ray started from.
template <int G>
__global__ void __launch_bounds__(256) gbuffer_fill_kernel(const DevScene* __restrict__ Sp, WorkList wl, Workspace ws,
                                                           GBufferArrays gb CAMS_PARAM LAPSE_PARAM) {
  const DevScene& S = *Sp;
  glibc::tables_to_lds();  // whole block, before the early return
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= gb.n) return;
  double sky_u = 0.0, sky_v = 0.0, sky_z = 0.0;
  if (gb.status[idx] == GRT_OK) {
    RayConst rc;
    double y[8];
    const RayMeta mt = fin_get<G>(ws, idx, y, rc);
    if constexpr (G != GRT_GEOM_KERR_BL) rc.obs = observer_energy<G>(S, wl, idx CAMS_ARG);
    bool lost;
    const uint32_t nr = rec_count(ws, idx, mt.nrec, &lost);
    uint64_t at = gb.layer_start[idx];
    const uint64_t end = gb.layer_start[idx + 1];
    uint32_t pos = HIT_NIL;
    for (uint32_t j = 0; j < nr; ++j) {
      const RecRef r = rec_at(ws, idx, j, &pos);
      const uint32_t win = rec_win(ws, r);
      double p[4], pt[3], geo[4];
      const uint32_t oi = rec_read(ws, r, p, pt);
      XYZA col;
      if (shade_record<G>(S, rc, S.obj[oi], p, pt, &col, false, geo) != GRT_OK) break;  // status would not be 0
      const bool last_in_window = (j + 1 == nr) || (rec_next_win(ws, idx, j, r) != win);
      if (last_in_window && at < end) {
        gb.object[at] = (uint8_t)oi;
        gb.u[at] = geo[0];
        gb.v[at] = geo[1];
        gb.redshift[at] = geo[2];
        gb.radius[at] = geo[3];
#if GRT_LAPSE
        lapse[at] = (r.pool ? ws.pool->pool_time[r.s] : ws.pool->slot_time[r.s]) - S.cam.pos[0];
#endif
        ++at;
      }
    }
    if (mt.stop == GRT_STOP_CELESTIAL) celestial_args<G>(S, rc, y, &sky_u, &sky_v, &sky_z);
  }
  gb.sky_u[idx] = sky_u;
  gb.sky_v[idx] = sky_v;
  gb.sky_redshift[idx] = sky_z;
}
