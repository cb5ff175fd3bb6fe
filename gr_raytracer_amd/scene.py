"""Host-side mirror of the reference's scene/render surface, over the C ABI.

Names follow mdreem/gr_raytracer:
  * GlobalOpts                 src/cli/cli.rs:5-47
  * load_scene                 main.rs:74-116 + cli/<geometry>.rs + cli/shared.rs:131-321
  * Scene.render_section       Raytracer::render_section_to_cie_buffer (raytracer.rs:177-318)
  * Scene.render_pixels        render_section_to_cie_buffer_raw (raytracer.rs:195-244)
  * Scene.color_of_ray         Scene::color_of_ray (scene.rs:114-220) for one camera pixel
  * SceneBuilder               scene.rs::test_scene::create_scene_with_camera (scene.rs:250-369)
Every call runs the HIP kernels in libgrt.so; there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
import errno
import math
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib as L


# ------------------------------------------------------------------ options -------
@dataclass
class GlobalOpts:
    """clap GlobalOpts (cli.rs:5-47) with the reference defaults."""
    width: int = 500
    height: int = 500
    step_size: float = 0.01
    max_steps: int = 20000
    max_radius: float = 15000.0
    epsilon: float = 0.00001
    camera_position: Sequence[float] = (18.0, 0.0, 0.8)
    phi: float = 0.0
    theta: float = 0.0
    psi: float = 0.0
    tone_mapping: str = "reinhard"
    show_sampling_mask: bool = False
    sampling_mask_color: Sequence[int] = (255, 0, 255)

    def to_c(self) -> L.GlobalOpts:
        o = L.GlobalOpts()
        L.lib().grt_default_global_opts(C.byref(o))
        o.width, o.height = int(self.width), int(self.height)
        o.step_size, o.max_steps, o.max_radius = float(self.step_size), int(self.max_steps), float(self.max_radius)
        o.epsilon = float(self.epsilon)
        for k in range(3):
            o.camera_position[k] = float(self.camera_position[k])
            o.sampling_mask_color[k] = int(self.sampling_mask_color[k])
        o.phi, o.theta, o.psi = float(self.phi), float(self.theta), float(self.psi)
        o.tone_mapping = {"reinhard": 0, "global-linear": 1}[self.tone_mapping]
        o.show_sampling_mask = int(bool(self.show_sampling_mask))
        return o


def default_adaptive() -> L.AdaptiveConfig:
    c = L.AdaptiveConfig()
    L.lib().grt_default_adaptive_config(C.byref(c))
    return c


def device_count() -> int:
    return int(L.lib().grt_device_count())


# ------------------------------------------------------------------ scenes --------
class HostScene:
    """A TOML scene built on the host (textures decoded, camera tetrad, LUTs)."""

    def __init__(self, config_file: str, opts: GlobalOpts, resource_root: Optional[str] = None):
        self._h = C.c_void_p()
        rr = None if resource_root is None else str(resource_root).encode()
        L.check(L.lib().grt_host_scene_load(str(config_file).encode(), rr, C.byref(opts.to_c()), C.byref(self._h)),
                f"load_scene({config_file})")
        self.opts = opts

    @property
    def desc(self) -> L.SceneDesc:
        return L.lib().grt_host_scene_desc(self._h).contents

    def desc_ptr(self):
        return L.lib().grt_host_scene_desc(self._h)

    @property
    def info_log(self) -> list:
        """The reference's info-level lines of the scene setup, in order (grt_host_scene_log:
        the temperature LUT's, temperature.rs:55-102)."""
        return [x for x in (L.lib().grt_host_scene_log(self._h) or b"").decode().split("\n") if x]

    @property
    def adaptive(self) -> L.AdaptiveConfig:
        c = L.AdaptiveConfig()
        L.lib().grt_host_scene_adaptive(self._h, C.byref(c))
        return c

    def camera(self, position, phi: float = 0.0, theta: float = 0.0, psi: float = 0.0) -> L.CameraDesc:
        """The camera a load of this scene with these --camera-position / --phi / --theta /
        --psi values would have built (grt_host_scene_camera): the cameras of
        Scene.render_sequence."""
        pos = (C.c_double * 3)(*[float(x) for x in position])
        cam = L.CameraDesc()
        L.check(L.lib().grt_host_scene_camera(self._h, pos, float(phi), float(theta), float(psi), C.byref(cam)),
                "grt_host_scene_camera")
        return cam

    def close(self) -> None:
        if self._h:
            L.lib().grt_host_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_scene(config_file: str, opts: Optional[GlobalOpts] = None, resource_root: Optional[str] = None) -> "Scene":
    """Parse a scene TOML + options and upload it (main.rs:74-116, cli/shared.rs:131-321)."""
    hs = HostScene(config_file, opts or GlobalOpts(), resource_root)
    return Scene(hs.desc_ptr(), keepalive=hs, adaptive=hs.adaptive)


@dataclass
class RenderResult:
    xyza: np.ndarray                 # float32 (n, 4)
    ray_class: np.ndarray            # uint8 (n,)
    status: np.ndarray               # uint8 (n,)
    xyza64: Optional[np.ndarray] = None
    steps: Optional[np.ndarray] = None
    stop_reason: Optional[np.ndarray] = None
    hits: Optional[np.ndarray] = None  # uint32 (n,): windows with an intersection (scene.rs:141-152)
    stats: dict = field(default_factory=dict)


@dataclass
class SectionResult:
    xyza64: np.ndarray          # float64 (n, 4)
    ray_class: np.ndarray       # uint8 (n,)
    status: np.ndarray          # uint8 (n,): the 1-spp ray's status
    n_supersampled: int
    stats: dict
    n_failed_subsamples: int
    failed_subsamples: np.ndarray  # (m, 3) uint32: section pixel, stratum, status (m <= capacity)
    # log_events=True: the 1-spp rays' stop reasons and accepted steps, and the supersample
    # sub-rays that ended on NaN coordinates or without a terminal event (no error):
    # (k, 4) uint32 section pixel, stratum, stop reason, accepted steps (scene.rs:178-202)
    stop: Optional[np.ndarray] = None
    steps: Optional[np.ndarray] = None
    subsample_events: Optional[np.ndarray] = None


def _stats_dict(st: L.Stats) -> dict:
    return {"accepted_steps": int(st.accepted_steps), "attempts": int(st.attempts), "rays": int(st.rays),
            "hit_overflows": int(st.hit_overflows), "kernel_ms": float(st.kernel_ms),
            "march_jobs": int(st.march_jobs), "march_samples": int(st.march_samples),
            "march_noise_samples": int(st.march_noise_samples), "march_emit_samples": int(st.march_emit_samples)}


class Scene:
    """Device-resident scene (grt_scene); one device copy per GPU, created lazily."""

    def __init__(self, desc_ptr, keepalive=None, adaptive: Optional[L.AdaptiveConfig] = None):
        self._s = C.c_void_p()
        L.check(L.lib().grt_scene_create(desc_ptr, C.byref(self._s)), "grt_scene_create")
        self._keep = keepalive
        self.desc = desc_ptr.contents
        self.adaptive = adaptive if adaptive is not None else default_adaptive()

    @property
    def rows(self) -> int:
        return int(self.desc.camera.rows)

    @property
    def cols(self) -> int:
        return int(self.desc.camera.cols)

    def close(self) -> None:
        if self._s:
            L.lib().grt_scene_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_pixels(self, row0: int = 0, col0: int = 0, rows: Optional[int] = None, cols: Optional[int] = None,
                      device: int = 0, offsets=None, aux: bool = True) -> RenderResult:
        """1-spp trace of a rectangle, or of an offset list (pixel_index, dx, dy)."""
        rows = self.rows - row0 if rows is None else rows
        cols = self.cols - col0 if cols is None else cols
        off = None
        keep = []
        if offsets is not None:
            pix, dx, dy = (np.ascontiguousarray(offsets[0], np.uint32), np.ascontiguousarray(offsets[1], np.float64),
                           np.ascontiguousarray(offsets[2], np.float64))
            keep += [pix, dx, dy]
            off = L.Offsets(len(pix), L.ptr(pix, C.c_uint32), L.dptr(dx), L.dptr(dy))
            n = len(pix)
        else:
            n = rows * cols
        xyza = np.zeros((n, 4), np.float32)
        cls = np.zeros(n, np.uint8)
        status = np.zeros(n, np.uint8)
        res = RenderResult(xyza, cls, status)
        a = None
        if aux:
            res.xyza64 = np.zeros((n, 4), np.float64)
            res.steps = np.zeros(n, np.uint32)
            res.stop_reason = np.zeros(n, np.uint8)
            res.hits = np.zeros(n, np.uint32)
            a = L.AuxOut(L.dptr(res.xyza64), L.ptr(res.steps, C.c_uint32), L.ptr(res.stop_reason, C.c_uint8),
                         L.ptr(res.hits, C.c_uint32))
        st = L.Stats()
        L.check(L.lib().grt_render_pixels(self._s, device, row0, col0, rows, cols,
                                          C.byref(off) if off is not None else None,
                                          L.ptr(xyza, C.c_float), L.ptr(cls, C.c_uint8), L.ptr(status, C.c_uint8),
                                          C.byref(a) if a is not None else None, C.byref(st)), "grt_render_pixels")
        res.stats = _stats_dict(st)
        return res

    def trace_gbuffer(self, row0: int = 0, col0: int = 0, rows: Optional[int] = None, cols: Optional[int] = None,
                      device: int = 0, adaptive: Optional[L.AdaptiveConfig] = None, lapse: bool = False) -> "GBuffer":
        """1-spp exact trace of a rectangle that keeps its geometry buffer (grt_gbuffer_trace):
        shade it again under any scene with the same shape key without integrating.  With
        `adaptive`, one `shade_section` with the scene as its own tracer follows, so the
        buffer also holds the sub-rays of the pixels this scene's adaptive frame selects.
        With `lapse`, the trace also records each layer's light-travel time
        (grt_gbuffer_trace_lapse): the same arrays byte for byte, and `GBuffer.lapse()`; with
        both, the sub-rays are filled with theirs (a timed set, `GBuffer.sub_lapse()`)."""
        rows = self.rows - row0 if rows is None else rows
        cols = self.cols - col0 if cols is None else cols
        h = C.c_void_p()
        st = L.Stats()
        name = "grt_gbuffer_trace_lapse" if lapse else "grt_gbuffer_trace"
        L.check(getattr(L.lib(), name)(self._s, device, row0, col0, rows, cols, C.byref(h), C.byref(st)), name)
        gb = GBuffer(h, _stats_dict(st))
        if adaptive is not None and lapse:
            # the static frame's own selection (what `adaptive` alone fills), traced timed: the
            # mask pass paints the selected pixels and traces nothing, and no shaded pixel has
            # the mask's alpha of -1
            if adaptive.enabled:
                res, _ = gb.shade_section(self, adaptive=adaptive, sampling_mask_xyza=(-1.0, -1.0, -1.0, -1.0))
                gb.supersample(self, np.flatnonzero(res.xyza64[:, 3] == -1.0), adaptive.samples_per_axis, lapse=True)
        elif adaptive is not None:
            gb.shade_section(self, adaptive=adaptive, tracer=self)
        return gb

    def trace_gbuffer_multi(self, devices=(0,), band_rows: int = 16, transport=None) -> "GBuffer":
        """The whole frame's geometry buffer traced over `devices` (grt_gbuffer_trace_multi: the
        cyclic row bands of `render_frame_multi`, one host thread per rank, every rank's part
        gathered and assembled on devices[0]).  The result is the ordinary GBuffer of
        `trace_gbuffer(device=devices[0])`, byte for byte, with the summed `stats` and the
        call's `report` (GBufferMultiReport) as attributes.  transport: as
        `render_frame_multi`'s, set for this call and restored afterwards; under the peer
        transports `devices` may repeat an ordinal (one rank per entry)."""
        devs = (C.c_int * max(len(devices), 1))(*devices)
        h = C.c_void_p()
        st = L.Stats()
        rep = L.GBufferMultiReport()
        lib = L.lib()
        before = None
        if transport is not None:
            mode = L.MULTI_TRANSPORTS[transport] if isinstance(transport, str) else int(transport)
            before = lib.grt_get_multi_transport()
            L.check(lib.grt_set_multi_transport(mode), "grt_set_multi_transport")
        try:
            rc = lib.grt_gbuffer_trace_multi(self._s, len(devices), devs, band_rows, C.byref(h), C.byref(st),
                                             C.byref(rep))
        finally:
            if before is not None:
                lib.grt_set_multi_transport(before)
        L.check(rc, "grt_gbuffer_trace_multi")
        gb = GBuffer(h, _stats_dict(st))
        gb.report = rep
        return gb

    def trace_gbuffer_sequence(self, cameras, device: int = 0,
                               adaptive: Optional[L.AdaptiveConfig] = None) -> "GBufferSequence":
        """K cameras (CameraDesc, each with the scene's rows and cols) over this scene, traced
        stacked at 1 spp with the exact kernels, one geometry buffer per frame
        (grt_gbuffer_trace_sequence).  Buffer k is the ordinary GBuffer of a scene with camera
        k, byte for byte.  Returns a list of GBuffer with the call's `stats` and `report`
        (GBufferSequenceReport) as attributes.  With `adaptive`, one `shade_section_sequence`
        with the scene as appearance and as tracer follows, so each buffer also holds the
        sub-rays of the pixels this scene's adaptive frame of its camera selects (its report
        dict: the attribute `adaptive_report`)."""
        cams = list(cameras)
        k = len(cams)
        table = (L.CameraDesc * max(k, 1))(*cams)
        handles = (C.c_void_p * max(k, 1))()
        st = L.Stats()
        rep = L.GBufferSequenceReport()
        L.check(L.lib().grt_gbuffer_trace_sequence(self._s, device, k, table, handles, C.byref(st), C.byref(rep)),
                "grt_gbuffer_trace_sequence")
        stats = _stats_dict(st)
        out = GBufferSequence(GBuffer(C.c_void_p(handles[f]), stats) for f in range(k))
        out.stats, out.report = stats, rep
        if adaptive is not None:
            out.adaptive_report = shade_section_sequence(out, self, adaptive=adaptive, tracer=self)[1]
        return out

    def render_shard(self, band_rows: int, shard: int, n_shards: int, device: int = 0,
                     aux: bool = True) -> RenderResult:
        """The local rows of one cyclic row-band shard (grt_render_shard), full width."""
        sh = L.RowShard(band_rows, shard, n_shards)
        n = int(L.lib().grt_shard_row_count(self.rows, C.byref(sh))) * self.cols
        xyza, cls, status = np.zeros((n, 4), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        res = RenderResult(xyza, cls, status)
        a = None
        if aux:
            res.xyza64, res.steps, res.stop_reason = np.zeros((n, 4)), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
            res.hits = np.zeros(n, np.uint32)
            a = L.AuxOut(L.dptr(res.xyza64), L.ptr(res.steps, C.c_uint32), L.ptr(res.stop_reason, C.c_uint8),
                         L.ptr(res.hits, C.c_uint32))
        st = L.Stats()
        L.check(L.lib().grt_render_shard(self._s, device, C.byref(sh), L.ptr(xyza, C.c_float), L.ptr(cls, C.c_uint8),
                                         L.ptr(status, C.c_uint8), C.byref(a) if a is not None else None,
                                         C.byref(st)), "grt_render_shard")
        res.stats = _stats_dict(st)
        return res

    def render_frame_multi(self, devices=(0,), band_rows: int = 16, adaptive: Optional[L.AdaptiveConfig] = None,
                           supersample: bool = False, sampling_mask_xyza=None, fields=("xyza", "class", "status"),
                           fail_capacity: int = 0, transport=None) -> dict:
        """The whole frame over `devices` (grt_render_frame_multi: cyclic row bands, one host
        thread per device, one gather to devices[0]).  transport: "rccl", "peer" or
        "peer-staged" (or the grt_multi_transport number) sets grt_set_multi_transport for
        this call and restores it afterwards; None leaves the knob as it is.  Under the peer
        transports `devices` may repeat an ordinal (one rank per entry).  fields: which of
        "xyza" (f32), "xyza64", "class", "status", "stop", "steps" to return (frame order).  supersample:
        the adaptive pass with `adaptive` (default: the scene's own configuration).
        Returns a dict of the fields plus "stats", "n_supersampled", "report" and, with
        fail_capacity, "failures" (pixel, sample, status, stop, steps arrays)."""
        n = self.rows * self.cols
        want = set(fields)
        arrays = {}
        if "xyza" in want:
            arrays["xyza"] = np.zeros((n, 4), np.float32)
        if "xyza64" in want or supersample or sampling_mask_xyza is not None:
            arrays["xyza64"] = np.zeros((n, 4), np.float64)
        for k, dt in (("class", np.uint8), ("status", np.uint8), ("stop", np.uint8), ("steps", np.uint32)):
            if k in want:
                arrays[k] = np.zeros(n, dt)
        out = L.FrameOut(L.ptr(arrays["xyza"], C.c_float) if "xyza" in arrays else None,
                         L.dptr(arrays["xyza64"]) if "xyza64" in arrays else None,
                         L.ptr(arrays["class"], C.c_uint8) if "class" in arrays else None,
                         L.ptr(arrays["status"], C.c_uint8) if "status" in arrays else None,
                         L.ptr(arrays["stop"], C.c_uint8) if "stop" in arrays else None,
                         L.ptr(arrays["steps"], C.c_uint32) if "steps" in arrays else None)
        cfg = None
        if supersample or sampling_mask_xyza is not None:
            cfg = L.AdaptiveConfig()
            C.memmove(C.byref(cfg), C.byref(adaptive if adaptive is not None else self.adaptive), C.sizeof(cfg))
            cfg.enabled = 1 if supersample else cfg.enabled
        mask = None
        if sampling_mask_xyza is not None:
            mask = np.ascontiguousarray(sampling_mask_xyza, np.float64)
        devs = (C.c_int * len(devices))(*devices)
        fails = None
        farr = {}
        if fail_capacity:
            farr = {"pixel": np.zeros(fail_capacity, np.uint32), "sample": np.zeros(fail_capacity, np.uint32),
                    "status": np.zeros(fail_capacity, np.uint8), "stop": np.zeros(fail_capacity, np.uint8),
                    "steps": np.zeros(fail_capacity, np.uint32)}
            fails = L.SubsampleFailures(fail_capacity, L.ptr(farr["pixel"], C.c_uint32),
                                        L.ptr(farr["sample"], C.c_uint32), L.ptr(farr["status"], C.c_uint8), 0,
                                        L.ptr(farr["stop"], C.c_uint8), L.ptr(farr["steps"], C.c_uint32))
        nsel = C.c_uint64(0)
        st = L.Stats()
        rep = L.MultiReport()
        lib = L.lib()
        before = None
        if transport is not None:
            mode = L.MULTI_TRANSPORTS[transport] if isinstance(transport, str) else int(transport)
            before = lib.grt_get_multi_transport()
            L.check(lib.grt_set_multi_transport(mode), "grt_set_multi_transport")
        try:
            rc = lib.grt_render_frame_multi(self._s, len(devices), devs, band_rows,
                                            C.byref(cfg) if cfg is not None else None,
                                            L.dptr(mask) if mask is not None else None, C.byref(out),
                                            C.byref(nsel), C.byref(st), C.byref(fails) if fails is not None else None,
                                            C.byref(rep))
        finally:
            if before is not None:
                lib.grt_set_multi_transport(before)
        L.check(rc, "grt_render_frame_multi")
        arrays["stats"] = _stats_dict(st)
        arrays["n_supersampled"] = int(nsel.value)
        arrays["report"] = rep
        if fails is not None:
            m = min(int(fails.count), fail_capacity)
            arrays["failures"] = {k: v[:m] for k, v in farr.items()}
            arrays["failures"]["count"] = int(fails.count)
        return arrays

    def render_sequence(self, cameras, adaptive: Optional[L.AdaptiveConfig] = None, mask=None, device: int = 0,
                        supersample: bool = False, fields=("xyza", "xyza64", "class", "status", "stop", "steps"),
                        failure_capacity: int = 1 << 16) -> dict:
        """K cameras (CameraDesc, each with the scene's rows and cols) over this scene in
        stacked launches (grt_render_sequence); every frame is bit-identical to rendering
        its camera alone.  supersample: the adaptive pass with `adaptive` (default: the
        scene's own configuration), per frame; mask: paint the selected pixels instead.
        Returns a dict of the `fields` as arrays with a leading frame axis ("xyza" only at
        1 spp), plus "stats", "report" (SequenceReport) and, with supersampling,
        "n_supersampled" (K,) and "failures": per frame an (m, 3) uint32 array of (pixel,
        stratum, status) and "n_failed" the counts."""
        cams = list(cameras)
        k, n = len(cams), self.rows * self.cols
        table = (L.CameraDesc * max(k, 1))(*cams)
        ss = supersample or mask is not None
        want = set(fields)
        arrays = {}
        if "xyza" in want and not ss:
            arrays["xyza"] = np.zeros((k, n, 4), np.float32)
        if "xyza64" in want or ss:
            arrays["xyza64"] = np.zeros((k, n, 4), np.float64)
        for name, dt in (("class", np.uint8), ("status", np.uint8), ("stop", np.uint8), ("steps", np.uint32)):
            if name in want:
                arrays[name] = np.zeros((k, n), dt)
        out = L.FrameOut(L.ptr(arrays["xyza"], C.c_float) if "xyza" in arrays else None,
                         L.dptr(arrays["xyza64"]) if "xyza64" in arrays else None,
                         L.ptr(arrays["class"], C.c_uint8) if "class" in arrays else None,
                         L.ptr(arrays["status"], C.c_uint8) if "status" in arrays else None,
                         L.ptr(arrays["stop"], C.c_uint8) if "stop" in arrays else None,
                         L.ptr(arrays["steps"], C.c_uint32) if "steps" in arrays else None)
        cfg = None
        if ss:
            cfg = L.AdaptiveConfig()
            C.memmove(C.byref(cfg), C.byref(adaptive if adaptive is not None else self.adaptive), C.sizeof(cfg))
            cfg.enabled = 1 if supersample else cfg.enabled
        m = np.ascontiguousarray(mask, np.float64) if mask is not None else None
        nsel = (C.c_uint64 * max(k, 1))()
        fails, farr = None, []
        if ss and failure_capacity:
            fails = (L.SubsampleFailures * max(k, 1))()
            for f in range(k):
                a = (np.zeros(failure_capacity, np.uint32), np.zeros(failure_capacity, np.uint32),
                     np.zeros(failure_capacity, np.uint8))
                farr.append(a)
                fails[f] = L.SubsampleFailures(failure_capacity, L.ptr(a[0], C.c_uint32), L.ptr(a[1], C.c_uint32),
                                               L.ptr(a[2], C.c_uint8), 0, None, None)
        st = L.Stats()
        rep = L.SequenceReport()
        L.check(L.lib().grt_render_sequence(self._s, device, k, table, C.byref(cfg) if cfg is not None else None,
                                            L.dptr(m) if m is not None else None, C.byref(out), nsel, C.byref(st),
                                            fails, C.byref(rep)), "grt_render_sequence")
        arrays["stats"] = _stats_dict(st)
        arrays["report"] = rep
        if ss:
            arrays["n_supersampled"] = np.array([int(nsel[f]) for f in range(k)], np.uint64)
            if fails is not None:
                arrays["n_failed"] = [int(fails[f].count) for f in range(k)]
                arrays["failures"] = []
                for f in range(k):
                    c = min(int(fails[f].count), failure_capacity)
                    a = farr[f]
                    arrays["failures"].append(np.stack([a[0][:c], a[1][:c], a[2][:c].astype(np.uint32)], axis=1))
        return arrays

    def render_section(self, from_row: int = 0, from_col: int = 0, to_row: Optional[int] = None,
                       to_col: Optional[int] = None, adaptive: Optional[L.AdaptiveConfig] = None,
                       sampling_mask_xyza=None, device: int = 0):
        """render_section_to_cie_buffer (raytracer.rs:177-318): f64 XYZA per pixel.
        Returns (xyza64, class, n_supersampled, stats)."""
        r = self.render_section_ex(from_row, from_col, to_row, to_col, adaptive, sampling_mask_xyza, device)
        return r.xyza64, r.ray_class, r.n_supersampled, r.stats

    def render_section_ex(self, from_row: int = 0, from_col: int = 0, to_row: Optional[int] = None,
                          to_col: Optional[int] = None, adaptive: Optional[L.AdaptiveConfig] = None,
                          sampling_mask_xyza=None, device: int = 0, failure_capacity: int = 1 << 16,
                          log_events: bool = False):
        """render_section plus each pixel's 1-spp status and the failed supersample
        sub-rays ((pixel, stratum, status), sorted; raytracer.rs:232-239, :357-362); with
        log_events, also what color_of_ray's NaN / no-terminal-event log lines need."""
        to_row = self.rows if to_row is None else to_row
        to_col = self.cols if to_col is None else to_col
        n = (to_row - from_row) * (to_col - from_col)
        out = np.zeros((n, 4), np.float64)
        cls = np.zeros(n, np.uint8)
        status = np.zeros(n, np.uint8)
        nsel = C.c_uint64(0)
        st = L.Stats()
        mask = None
        if sampling_mask_xyza is not None:
            mask = np.ascontiguousarray(sampling_mask_xyza, np.float64)
        fp = np.zeros(failure_capacity, np.uint32)
        fs = np.zeros(failure_capacity, np.uint32)
        fst = np.zeros(failure_capacity, np.uint8)
        fsp = np.zeros(failure_capacity, np.uint8)
        fn = np.zeros(failure_capacity, np.uint32)
        fails = L.SubsampleFailures(failure_capacity, L.ptr(fp, C.c_uint32), L.ptr(fs, C.c_uint32),
                                    L.ptr(fst, C.c_uint8), 0, L.ptr(fsp, C.c_uint8) if log_events else None,
                                    L.ptr(fn, C.c_uint32) if log_events else None)
        stop = np.zeros(n, np.uint8) if log_events else None
        steps = np.zeros(n, np.uint32) if log_events else None
        L.check(L.lib().grt_render_section_ex(self._s, device, from_row, from_col, to_row, to_col,
                                              C.byref(adaptive or self.adaptive),
                                              L.dptr(mask) if mask is not None else None, L.dptr(out),
                                              L.ptr(cls, C.c_uint8), C.byref(nsel), C.byref(st),
                                              L.ptr(status, C.c_uint8), C.byref(fails),
                                              L.ptr(stop, C.c_uint8) if log_events else None,
                                              L.ptr(steps, C.c_uint32) if log_events else None),
                "grt_render_section_ex")
        m = min(int(fails.count), failure_capacity)
        rows = np.stack([fp[:m], fs[:m], fst[:m].astype(np.uint32)], axis=1)
        if not log_events:
            return SectionResult(out, cls, status, int(nsel.value), _stats_dict(st), int(fails.count), rows)
        failed = fst[:m] != 0
        events = np.stack([fp[:m], fs[:m], fsp[:m].astype(np.uint32), fn[:m]], axis=1)[~failed]
        return SectionResult(out, cls, status, int(nsel.value), _stats_dict(st), int(fails.count) - len(events),
                             rows[failed], stop, steps, events)

    def _trace(self, fn, a, b, width: int, capacity: int, device: int):
        a = np.ascontiguousarray(a, np.float64).reshape(-1, width)
        b = np.ascontiguousarray(b, np.float64).reshape(-1, width)
        n = a.shape[0]
        steps = np.zeros((n, capacity, 9), np.float64)
        n_steps = np.zeros(n, np.uint64)
        stop, status = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        L.check(fn(self._s, device, n, L.dptr(a), L.dptr(b), capacity, L.dptr(steps), L.ptr(n_steps, C.c_uint64),
                   L.ptr(stop, C.c_uint8), L.ptr(status, C.c_uint8)), "grt_trace")
        return Trajectories(steps, n_steps.astype(np.int64), stop, status)

    def trace_pixels(self, rows, cols, capacity: Optional[int] = None, device: int = 0) -> "Trajectories":
        """Whole trajectories of camera rays (Raytracer::integrate_ray_at_point,
        raytracer.rs:499-507; `render-ray`).  capacity defaults to max_steps records."""
        cap = int(self.desc.max_steps) if capacity is None else capacity
        return self._trace(L.lib().grt_trace_pixels, np.atleast_1d(rows), np.atleast_1d(cols), 1, cap, device)

    def trace_rays(self, positions, momenta, capacity: Optional[int] = None, device: int = 0) -> "Trajectories":
        """Whole trajectories from native-chart positions / contravariant momenta (n x 4)."""
        cap = int(self.desc.max_steps) if capacity is None else capacity
        return self._trace(L.lib().grt_trace_rays, positions, momenta, 4, cap, device)

    def color_of_ray(self, row: int, col: int, device: int = 0):
        """Colour, class and status of one camera pixel (Scene::color_of_ray)."""
        r = self.render_pixels(row, col, 1, 1, device=device)
        return r.xyza64[0], int(r.ray_class[0]), int(r.status[0])

    def health(self, row0: int = 0, col0: int = 0, rows: Optional[int] = None, cols: Optional[int] = None,
               device: int = 0, per_ray: bool = False) -> dict:
        """The reference's invariant monitors over a rectangle (grt_health_pixels): camera-ray
        null condition (scene.rs:116-124) and k.k / constants-of-motion drifts
        (integrator.rs:91-201).  per_ray adds an (n, 5) array: |k.k| at the camera, largest
        |k.k| along the path, largest drift of E, L_z, Q."""
        rows = self.rows - row0 if rows is None else rows
        cols = self.cols - col0 if cols is None else cols
        h = L.Health()
        arr = np.zeros((rows * cols, 5)) if per_ray else None
        L.check(L.lib().grt_health_pixels(self._s, device, row0, col0, rows, cols, C.byref(h),
                                          L.ptr(arr, C.c_double) if per_ray else None), "grt_health_pixels")
        nc = h.n_constants
        out = {"rays": h.rays, "failed": h.failed, "null_violations": h.null_violations, "max_null": h.max_null,
               "kk_drift_rays": h.kk_drift_rays, "max_kk_drift": h.max_kk_drift, "n_constants": nc,
               "constant_drift_rays": list(h.constant_drift_rays)[:nc],
               "max_constant_drift": list(h.max_constant_drift)[:nc]}
        if per_ray:
            out["per_ray"] = arr
        return out

    def tail_handoffs(self, device: int = 0) -> int:
        """Rays the last Kerr-Schild trace on `device` handed to the tail kernel."""
        n = C.c_uint64()
        L.check(L.lib().grt_tail_handoffs(self._s, device, C.byref(n)), "grt_tail_handoffs")
        return n.value

    def tail_report(self, device: int = 0, capacity: int = 0) -> dict:
        """Hand-off diagnostics of the last Kerr-Schild trace: count, timeline (s since the
        integrate kernel started) and the handed-off rays' output slots and step counts."""
        n = C.c_uint64()
        tl = (C.c_double * 3)()
        slot = np.zeros(capacity, np.uint64)
        step = np.zeros(capacity, np.uint64)
        L.check(L.lib().grt_tail_report(self._s, device, C.byref(n), tl, L.ptr(slot, C.c_uint64),
                                        L.ptr(step, C.c_uint64), capacity), "grt_tail_report")
        k = min(n.value, capacity)
        return {"handed_off": n.value, "drained_s": tl[0], "handoff_s": tl[1], "tail_end_s": tl[2],
                "slot": slot[:k], "step": step[:k]}


_GB_PIXEL = (("status", np.uint8), ("stop", np.uint8), ("steps", np.uint32), ("sky_u", np.float64),
             ("sky_v", np.float64), ("sky_redshift", np.float64))
_GB_LAYER = (("object", np.uint8), ("u", np.float64), ("v", np.float64), ("redshift", np.float64),
             ("radius", np.float64))
_GB_CTYPE = {np.uint8: C.c_uint8, np.uint32: C.c_uint32, np.uint64: C.c_uint64, np.float64: C.c_double}


def _gbuffer_host_arrays(info: L.GBufferInfo, arrays: Optional[dict] = None):
    """(dict of numpy arrays sized by `info`, the grt_gbuffer_arrays over them); `arrays`
    given: those, made contiguous and of the right type, after a length check."""
    n, nl = int(info.n_pixels), int(info.n_layers)
    spec = [(k, t, n) for k, t in _GB_PIXEL] + [("layer_start", np.uint64, n + 1)] + [(k, t, nl) for k, t in _GB_LAYER]
    out = {}
    for k, t, m in spec:
        if arrays is None:
            out[k] = np.zeros(m, t)
        else:
            out[k] = np.ascontiguousarray(arrays[k], t)
            if out[k].shape != (m,):
                raise L.GrtError(f"g-buffer array {k}: shape {out[k].shape}, expected ({m},)")
    c = L.GBufferArrays(**{k: L.ptr(out[k], _GB_CTYPE[t]) for k, t, _ in spec})
    return out, c


def _gbuffer_sub_host_arrays(sub: L.GBufferSubInfo, arrays: Optional[dict] = None):
    """_gbuffer_host_arrays for a sub-sample set: the twelve arrays over its sub-rays and
    layers, and sub_pixel; returns (dict, grt_gbuffer_arrays, sub_pixel pointer)."""
    sized = L.GBufferInfo(n_pixels=int(sub.n_sub_rays), n_layers=int(sub.n_sub_layers))
    out, c = _gbuffer_host_arrays(sized, arrays)
    m = int(sub.n_sub_pixels)
    if arrays is None:
        out["sub_pixel"] = np.zeros(m, np.uint32)
    else:
        out["sub_pixel"] = np.ascontiguousarray(arrays["sub_pixel"], np.uint32)
        if out["sub_pixel"].shape != (m,):
            raise L.GrtError(f"g-buffer array sub_pixel: shape {out['sub_pixel'].shape}, expected ({m},)")
    return out, c, L.ptr(out["sub_pixel"], C.c_uint32)


def _frame_out_arrays(k: int, n: int, fields):
    """(dict of zeroed [k, n(, 4)] arrays for `fields`, the grt_frame_out over them)."""
    want = set(fields)
    arrays = {}
    for name, shape, dt in (("xyza", (k, n, 4), np.float32), ("xyza64", (k, n, 4), np.float64),
                            ("class", (k, n), np.uint8), ("status", (k, n), np.uint8), ("stop", (k, n), np.uint8),
                            ("steps", (k, n), np.uint32)):
        if name in want:
            arrays[name] = np.zeros(shape, dt)
    out = L.FrameOut(L.ptr(arrays["xyza"], C.c_float) if "xyza" in arrays else None,
                     L.dptr(arrays["xyza64"]) if "xyza64" in arrays else None,
                     L.ptr(arrays["class"], C.c_uint8) if "class" in arrays else None,
                     L.ptr(arrays["status"], C.c_uint8) if "status" in arrays else None,
                     L.ptr(arrays["stop"], C.c_uint8) if "stop" in arrays else None,
                     L.ptr(arrays["steps"], C.c_uint32) if "steps" in arrays else None)
    return arrays, out


class GBufferMissing(L.GrtError):
    """shade_section without a tracer met selected pixels the sub-sample set does not hold
    (-ENODATA); `report` is the call's report (n_missing)."""

    def __init__(self, msg: str, report: dict):
        super().__init__(msg)
        self.report = report


class GBuffer:
    """Device-resident geometry buffer of a traced rectangle (grt_gbuffer): per pixel the
    trace's status, stop reason, steps and the celestial sphere's texture arguments; per
    layer (a window's nearest hit, front to back) the object and its texture / temperature
    arguments.  `shade(scene)` is bit-identical to `scene.render_pixels` of the rectangle
    for any scene with the traced shape key, camera and integration parameters."""

    def __init__(self, handle, stats: Optional[dict] = None):
        self._h = handle
        self.stats = stats or {}

    @property
    def info(self) -> L.GBufferInfo:
        out = L.GBufferInfo()
        L.check(L.lib().grt_gbuffer_info_get(self._h, C.byref(out)), "grt_gbuffer_info_get")
        return out

    @property
    def trace_times(self) -> dict:
        """Event times of the trace that filled the buffer, ms (zeros for a loaded one)."""
        ms = (C.c_double * 2)()
        L.check(L.lib().grt_gbuffer_trace_times(self._h, ms), "grt_gbuffer_trace_times")
        return {"trace_ms": float(ms[0]), "fill_ms": float(ms[1])}

    def arrays(self) -> dict:
        """The buffer's arrays, downloaded: numpy arrays by the names of grt_gbuffer_arrays."""
        out, c = _gbuffer_host_arrays(self.info)
        L.check(L.lib().grt_gbuffer_download(self._h, C.byref(c)), "grt_gbuffer_download")
        return out

    def shade(self, scene: "Scene", device: Optional[int] = None) -> RenderResult:
        """Shade under `scene`'s appearance on the buffer's device.  `device`, when given,
        must be that device (a scene has a copy per GPU; the buffer lives on one)."""
        info = self.info
        if device is not None and device != info.device:
            raise L.GrtError(f"grt_gbuffer_shade failed (-22): the g-buffer is on device {info.device}, not {device}")
        n = int(info.n_pixels)
        res = RenderResult(np.zeros((n, 4), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8),
                           xyza64=np.zeros((n, 4), np.float64))
        ms = C.c_float()
        L.check(L.lib().grt_gbuffer_shade(scene._s, self._h, L.ptr(res.xyza, C.c_float), L.ptr(res.ray_class, C.c_uint8),
                                          L.ptr(res.status, C.c_uint8), L.dptr(res.xyza64), C.byref(ms)),
                "grt_gbuffer_shade")
        res.stats = {"kernel_ms": float(ms.value)}
        return res

    def lapse(self):
        """Each layer's light-travel time, downloaded (grt_gbuffer_lapse_download): n_layers
        doubles <= 0, the chart's coordinate time of the hit minus the camera's; None for a
        buffer that holds none."""
        out = np.zeros(int(self.info.n_layers), np.float64)
        rc = L.lib().grt_gbuffer_lapse_download(self._h, L.dptr(out))
        if rc == -errno.ENODATA:
            return None
        L.check(rc, "grt_gbuffer_lapse_download")
        return out

    def set_lapse(self, lapse) -> None:
        """Give the buffer a lapse, one finite double per layer (grt_gbuffer_lapse_upload)."""
        a = np.ascontiguousarray(lapse, np.float64).reshape(-1)
        L.check(L.lib().grt_gbuffer_lapse_upload(self._h, L.dptr(a), len(a)), "grt_gbuffer_lapse_upload")

    def shade_orbit(self, scene: "Scene", times, fields=("xyza", "xyza64", "class", "status", "stop", "steps"),
                    device: Optional[int] = None, retarded: bool = False) -> dict:
        """The buffer under `scene`'s appearance at each of `times`, the disc's texture
        orbiting at the emitter's own rate (grt_gbuffer_shade_times; "fast light": one
        coordinate time per frame, no light-travel delay).  Frame k is `shade` of the buffer
        whose (u, v) went through gbuffer_orbit_uv at times[k], bit for bit.  Returns what
        shade_sequence returns: the `fields` with a leading frame axis, plus "stats".
        `retarded` (grt_gbuffer_shade_times_retarded; the buffer must hold a lapse): every
        disc layer at its emission time times[k] + lapse, gbuffer_orbit_uv_retarded's rule."""
        name = "grt_gbuffer_shade_times_retarded" if retarded else "grt_gbuffer_shade_times"
        info = self.info
        if device is not None and device != info.device:
            raise L.GrtError(f"{name} failed (-22): the g-buffer is on device {info.device}, not {device}")
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        arrays, out = _frame_out_arrays(len(t), int(info.n_pixels), fields)
        ms = C.c_float()
        L.check(getattr(L.lib(), name)(scene._s, self._h, len(t), L.dptr(t), C.byref(out), C.byref(ms)), name)
        arrays["stats"] = {"kernel_ms": float(ms.value)}
        return arrays

    @property
    def sub_info(self) -> L.GBufferSubInfo:
        """Sizes of the sub-sample set (samples_per_axis 0: the buffer holds none)."""
        out = L.GBufferSubInfo()
        L.check(L.lib().grt_gbuffer_sub_info_get(self._h, C.byref(out)), "grt_gbuffer_sub_info_get")
        return out

    def sub_arrays(self) -> dict:
        """The sub-sample set, downloaded: sub_pixel (block -> pixel) and the arrays of
        grt_gbuffer_arrays over the sub-rays (block b, stratum s at b * spa^2 + s)."""
        out, c, px = _gbuffer_sub_host_arrays(self.sub_info)
        L.check(L.lib().grt_gbuffer_sub_download(self._h, px, C.byref(c)), "grt_gbuffer_sub_download")
        return out

    def set_sub_arrays(self, sub: L.GBufferSubInfo, arrays: dict) -> None:
        """Replace the sub-sample set by host arrays (grt_gbuffer_sub_upload; checked)."""
        held, c, px = _gbuffer_sub_host_arrays(sub, arrays)
        L.check(L.lib().grt_gbuffer_sub_upload(self._h, C.byref(sub), px, C.byref(c)), "grt_gbuffer_sub_upload")

    def supersample(self, tracer: "Scene", pixels, samples_per_axis: int, lapse: bool = False) -> dict:
        """Trace the sub-rays of `pixels` (indices into the rectangle) under `tracer` and
        append them to the set; pixels already held are skipped.  Returns the traces' stats.
        With `lapse` the set is a timed one (grt_gbuffer_supersample_lapse): each sub-layer's
        light-travel time beside the same arrays."""
        px = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        st = L.Stats()
        name = "grt_gbuffer_supersample_lapse" if lapse else "grt_gbuffer_supersample"
        L.check(getattr(L.lib(), name)(tracer._s, self._h, samples_per_axis, len(px), L.ptr(px, C.c_uint32),
                                       C.byref(st)), name)
        return _stats_dict(st)

    @property
    def sub_has_lapse(self) -> bool:
        """Whether the sub-sample set is a timed one (grt_gbuffer_sub_has_lapse)."""
        rc = L.lib().grt_gbuffer_sub_has_lapse(self._h)
        if rc < 0:
            L.check(rc, "grt_gbuffer_sub_has_lapse")
        return rc == 1

    def sub_lapse(self):
        """The set's lapse, downloaded (grt_gbuffer_sub_lapse_download): n_sub_layers doubles,
        indexed as the set's layer arrays; None for an untimed or absent set."""
        out = np.zeros(int(self.sub_info.n_sub_layers), np.float64)
        rc = L.lib().grt_gbuffer_sub_lapse_download(self._h, L.dptr(out))
        if rc == -errno.ENODATA:
            return None
        L.check(rc, "grt_gbuffer_sub_lapse_download")
        return out

    def set_sub_lapse(self, lapse) -> None:
        """Give the set a lapse, one finite double per sub-layer, and so make it timed
        (grt_gbuffer_sub_lapse_upload)."""
        a = np.ascontiguousarray(lapse, np.float64).reshape(-1)
        L.check(L.lib().grt_gbuffer_sub_lapse_upload(self._h, L.dptr(a), len(a)), "grt_gbuffer_sub_lapse_upload")

    def clear_sub(self) -> None:
        """Drop the sub-sample set, whatever its kind (grt_gbuffer_sub_clear)."""
        L.check(L.lib().grt_gbuffer_sub_clear(self._h), "grt_gbuffer_sub_clear")

    def shade_section(self, scene: "Scene", adaptive: Optional[L.AdaptiveConfig] = None,
                      tracer: Optional["Scene"] = None, sampling_mask_xyza=None, failure_capacity: int = 0,
                      log_events: bool = False, time: Optional[float] = None, retarded: bool = False):
        """The adaptive frame of the buffer under `scene`'s appearance
        (grt_gbuffer_shade_section): bit-identical to `render_section_ex` of a scene with
        this appearance and the traced geometry, camera and integration parameters.
        Selected pixels whose sub-rays the buffer does not hold are traced under `tracer`
        and appended; without a tracer they raise GBufferMissing.  With `time` the disc's
        texture has orbited for that coordinate time (grt_gbuffer_shade_section_at; the set
        keeps unrotated numbers).  With `retarded` as well every disc layer is shaded at its
        emission time `time` + lapse (grt_gbuffer_shade_section_at_retarded): the buffer must
        hold a lapse and the set be timed or empty; a top-up fills an empty set timed.
        Returns (SectionResult, report dict); the result's stats are the top-up's."""
        if retarded and time is None:
            raise ValueError("shade_section: retarded=True needs a time")
        n = int(self.info.n_pixels)
        out = np.zeros((n, 4), np.float64)
        cls = np.zeros(n, np.uint8)
        status = np.zeros(n, np.uint8)
        nsel = C.c_uint64(0)
        mask = None
        if sampling_mask_xyza is not None:
            mask = np.ascontiguousarray(sampling_mask_xyza, np.float64)
        cap = max(failure_capacity, 1)
        fp, fs, fn = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        fst, fsp = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        fails = L.SubsampleFailures(failure_capacity, L.ptr(fp, C.c_uint32), L.ptr(fs, C.c_uint32),
                                    L.ptr(fst, C.c_uint8), 0, L.ptr(fsp, C.c_uint8) if log_events else None,
                                    L.ptr(fn, C.c_uint32) if log_events else None)
        rep = L.GBufferSectionReport()
        what = "grt_gbuffer_shade_section" if time is None else "grt_gbuffer_shade_section_at"
        if retarded:
            what = "grt_gbuffer_shade_section_at_retarded"
        args = (scene._s, self._h, C.byref(adaptive or scene.adaptive), L.dptr(mask) if mask is not None else None,
                tracer._s if tracer is not None else None, L.dptr(out), L.ptr(cls, C.c_uint8),
                L.ptr(status, C.c_uint8), C.byref(nsel), C.byref(fails), C.byref(rep))
        if time is None:
            rc = L.lib().grt_gbuffer_shade_section(*args)
        else:
            rc = getattr(L.lib(), what)(*args, float(time))
        report = {"n_selected": int(rep.n_selected), "n_held": int(rep.n_held), "n_traced": int(rep.n_traced),
                  "n_missing": int(rep.n_missing), "shade_ms": float(rep.shade_ms), "trace_ms": float(rep.trace_ms),
                  "top_up": _stats_dict(rep.top_up)}
        if rc == -errno.ENODATA:
            msg = L.lib().grt_last_error().decode(errors="replace")
            raise GBufferMissing(f"{what} failed ({rc}): {msg}", report)
        L.check(rc, what)
        m = min(int(fails.count), failure_capacity)
        rows = np.stack([fp[:m], fs[:m], fst[:m].astype(np.uint32)], axis=1)
        if not log_events:
            return SectionResult(out, cls, status, int(nsel.value), report["top_up"], int(fails.count), rows), report
        failed = fst[:m] != 0
        events = np.stack([fp[:m], fs[:m], fsp[:m].astype(np.uint32), fn[:m]], axis=1)[~failed]
        a = self.arrays()  # the 1-spp rays' stop reasons and steps are the buffer's
        return SectionResult(out, cls, status, int(nsel.value), report["top_up"], int(fails.count) - len(events),
                             rows[failed], a["stop"], a["steps"], events), report

    def save_sub(self, path) -> None:
        """Write the sub-sample set's sidecar (grt_gbuffer_sub_write_file), and beside it
        `<path>.lapse` when the set is timed."""
        info, sub = self.info, self.sub_info
        out, c, px = _gbuffer_sub_host_arrays(sub)
        L.check(L.lib().grt_gbuffer_sub_download(self._h, px, C.byref(c)), "grt_gbuffer_sub_download")
        L.check(L.lib().grt_gbuffer_sub_write_file(str(path).encode(), C.byref(info), C.byref(sub), px, C.byref(c)),
                "grt_gbuffer_sub_write_file")
        lapse = self.sub_lapse()
        if lapse is not None:
            self.write_sub_lapse_file(str(path) + ".lapse", info, sub, lapse)

    @staticmethod
    def write_sub_lapse_file(path, info: L.GBufferInfo, sub: L.GBufferSubInfo, lapse) -> None:
        a = np.ascontiguousarray(lapse, np.float64).reshape(-1)
        L.check(L.lib().grt_gbuffer_sub_lapse_write_file(str(path).encode(), C.byref(info), C.byref(sub), L.dptr(a),
                                                         len(a)), "grt_gbuffer_sub_lapse_write_file")

    @staticmethod
    def read_sub_lapse_file(path, info: L.GBufferInfo, sub: L.GBufferSubInfo) -> np.ndarray:
        """The lapse of a sidecar bound to the buffer `info` and its set `sub`, on the host."""
        out = np.zeros(int(sub.n_sub_layers), np.float64)
        L.check(L.lib().grt_gbuffer_sub_lapse_read_file(str(path).encode(), C.byref(info), C.byref(sub), L.dptr(out)),
                "grt_gbuffer_sub_lapse_read_file")
        return out

    @staticmethod
    def read_sub_file(path, info: L.GBufferInfo):
        """(sub info, dict of arrays) of a sidecar bound to the buffer `info`, on the host."""
        sub = L.GBufferSubInfo()
        L.check(L.lib().grt_gbuffer_sub_read_file(str(path).encode(), C.byref(info), C.byref(sub), None, None),
                "grt_gbuffer_sub_read_file")
        out, c, px = _gbuffer_sub_host_arrays(sub)
        L.check(L.lib().grt_gbuffer_sub_read_file(str(path).encode(), C.byref(info), C.byref(sub), px, C.byref(c)),
                "grt_gbuffer_sub_read_file")
        return sub, out

    @staticmethod
    def write_sub_file(path, info: L.GBufferInfo, sub: L.GBufferSubInfo, arrays: dict) -> None:
        held, c, px = _gbuffer_sub_host_arrays(sub, arrays)
        L.check(L.lib().grt_gbuffer_sub_write_file(str(path).encode(), C.byref(info), C.byref(sub), px, C.byref(c)),
                "grt_gbuffer_sub_write_file")

    def load_sub(self, path) -> None:
        """Read a sidecar written for this buffer and make it the buffer's set: a timed one
        when `<path>.lapse` is there (a sidecar of another or of a since-grown set is refused)."""
        info = self.info
        sub, arrays = self.read_sub_file(path, info)
        lapse = None
        if os.path.exists(str(path) + ".lapse"):
            lapse = self.read_sub_lapse_file(str(path) + ".lapse", info, sub)
        self.set_sub_arrays(sub, arrays)
        if lapse is not None:
            self.set_sub_lapse(lapse)

    def save(self, path) -> None:
        """Write the buffer's file, and beside it `<path>.lapse` when the buffer holds a lapse."""
        info = self.info
        out, c = _gbuffer_host_arrays(info)
        L.check(L.lib().grt_gbuffer_download(self._h, C.byref(c)), "grt_gbuffer_download")
        L.check(L.lib().grt_gbuffer_write_file(str(path).encode(), C.byref(info), C.byref(c)), "grt_gbuffer_write_file")
        lapse = self.lapse()
        if lapse is not None:
            self.write_lapse_file(str(path) + ".lapse", info, lapse)

    @staticmethod
    def write_lapse_file(path, info: L.GBufferInfo, lapse) -> None:
        a = np.ascontiguousarray(lapse, np.float64).reshape(-1)
        L.check(L.lib().grt_gbuffer_lapse_write_file(str(path).encode(), C.byref(info), L.dptr(a), len(a)),
                "grt_gbuffer_lapse_write_file")

    @staticmethod
    def read_lapse_file(path, info: L.GBufferInfo) -> np.ndarray:
        """The lapse of a sidecar bound to the buffer `info`, on the host (no GPU needed)."""
        out = np.zeros(int(info.n_layers), np.float64)
        L.check(L.lib().grt_gbuffer_lapse_read_file(str(path).encode(), C.byref(info), L.dptr(out)),
                "grt_gbuffer_lapse_read_file")
        return out

    @staticmethod
    def read_file(path):
        """(info, dict of arrays) of a g-buffer file, on the host (no GPU needed)."""
        info = L.GBufferInfo()
        L.check(L.lib().grt_gbuffer_read_file(str(path).encode(), C.byref(info), None), "grt_gbuffer_read_file")
        out, c = _gbuffer_host_arrays(info)
        L.check(L.lib().grt_gbuffer_read_file(str(path).encode(), C.byref(info), C.byref(c)), "grt_gbuffer_read_file")
        return info, out

    @staticmethod
    def write_file(path, info: L.GBufferInfo, arrays: dict) -> None:
        held, c = _gbuffer_host_arrays(info, arrays)  # `held`: the converted arrays `c` points into
        L.check(L.lib().grt_gbuffer_write_file(str(path).encode(), C.byref(info), C.byref(c)), "grt_gbuffer_write_file")

    @classmethod
    def from_arrays(cls, info: L.GBufferInfo, arrays: dict, device: int = 0) -> "GBuffer":
        held, c = _gbuffer_host_arrays(info, arrays)  # `held`: the converted arrays `c` points into
        h = C.c_void_p()
        L.check(L.lib().grt_gbuffer_upload(C.byref(info), C.byref(c), device, C.byref(h)), "grt_gbuffer_upload")
        return cls(h)

    @classmethod
    def load(cls, path, device: int = 0) -> "GBuffer":
        """The buffer of a file, with the lapse of `<path>.lapse` when that file is there."""
        info, arrays = cls.read_file(path)
        gb = cls.from_arrays(info, arrays, device)
        if os.path.exists(str(path) + ".lapse"):
            gb.set_lapse(cls.read_lapse_file(str(path) + ".lapse", info))
        return gb

    def close(self) -> None:
        if self._h:
            L.lib().grt_gbuffer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GBufferSequence(list):
    """The buffers of Scene.trace_gbuffer_sequence, frame by frame: a list of GBuffer with
    the call's `stats` (dict) and `report` (GBufferSequenceReport)."""
    stats: dict = {}
    report = None
    adaptive_report = None


def shade_sequence(buffers, scene: "Scene", fields=("xyza", "xyza64", "class", "status", "stop", "steps")) -> dict:
    """Shade the buffers (equal rows x cols, one device) under `scene`'s appearance in
    stacked launches (grt_gbuffer_shade_sequence): frame k is `buffers[k].shade(scene)` bit
    for bit.  Returns a dict of the `fields` as arrays with a leading frame axis, as
    Scene.render_sequence returns them at 1 spp ("stop" and "steps" are the buffers'
    recorded ones), plus "stats" ({"kernel_ms"})."""
    bufs = list(buffers)
    k = len(bufs)
    n = int(bufs[0].info.n_pixels) if k else 0
    arrays, out = _frame_out_arrays(k, n, fields)
    handles = (C.c_void_p * max(k, 1))(*[b._h for b in bufs])
    ms = C.c_float()
    L.check(L.lib().grt_gbuffer_shade_sequence(scene._s, k, handles, C.byref(out), C.byref(ms)),
            "grt_gbuffer_shade_sequence")
    arrays["stats"] = {"kernel_ms": float(ms.value)}
    return arrays


def supersample_sequence(buffers, tracer: "Scene", pixels_per_buffer, samples_per_axis: int) -> dict:
    """GBuffer.supersample for several whole-frame buffers at once, the traces stacked
    (grt_gbuffer_supersample_sequence): the sub-rays of `pixels_per_buffer[k]` are appended to
    `buffers[k]`'s set, byte for byte what `buffers[k].supersample` leaves with a tracer that
    has frame k's camera.  `tracer` needs the buffers' shape key, integration parameters and
    frame size; its camera is not used (each ray takes the camera its buffer recorded).
    Returns the traces' stats with the call's `report` (GBufferSequenceReport: n_launches
    chunks, n_traces traces) under "report"."""
    bufs = list(buffers)
    k = len(bufs)
    lists = [np.ascontiguousarray(p, np.uint32).reshape(-1) for p in pixels_per_buffer]
    if len(lists) != k:
        raise L.GrtError(f"grt_gbuffer_supersample_sequence failed (-22): {len(lists)} pixel lists for {k} buffers")
    handles = (C.c_void_p * max(k, 1))(*[b._h for b in bufs])
    counts = (C.c_uint64 * max(k, 1))(*[len(p) for p in lists])
    ptrs = (C.POINTER(C.c_uint32) * max(k, 1))(*[L.ptr(p, C.c_uint32) for p in lists])
    st = L.Stats()
    rep = L.GBufferSequenceReport()
    L.check(L.lib().grt_gbuffer_supersample_sequence(tracer._s, k, handles, samples_per_axis, counts, ptrs,
                                                     C.byref(st), C.byref(rep)), "grt_gbuffer_supersample_sequence")
    stats = _stats_dict(st)
    stats["report"] = rep
    return stats


def shade_section_sequence(buffers, scene: "Scene", adaptive: Optional[L.AdaptiveConfig] = None, mask=None,
                           tracer: Optional["Scene"] = None, failure_capacity: int = 0, log_events: bool = False):
    """The adaptive frames of several whole-frame buffers under `scene`'s appearance in stacked
    launches (grt_gbuffer_shade_section_sequence): frame k is `buffers[k].shade_section(scene,
    ...)` with a tracer that has frame k's camera, bit for bit.  `mask` (XYZA) paints the
    selected pixels instead.  Selected pixels the sets do not hold are traced in one stacked
    top-up under `tracer` (its camera is not used; it may be `scene`); without a tracer they
    raise GBufferMissing, whose report carries the per-frame counts.  Returns (dict, report):
    the dict holds "xyza64", "class", "status", "stop" and "steps" with a leading frame axis,
    "n_supersampled" [K], and per frame the failure lists "failed_subsamples" (rows pixel,
    stratum, status), "n_failed_subsamples" and, with log_events, "subsample_events" (rows
    pixel, stratum, stop, steps); the report dict has the totals, the times, "top_up" and
    "per_frame" ([K, 4]: selected, held, traced, missing)."""
    bufs = list(buffers)
    k = len(bufs)
    n = int(bufs[0].info.n_pixels) if k else 0
    arrays = {"xyza64": np.zeros((k, n, 4), np.float64), "class": np.zeros((k, n), np.uint8),
              "status": np.zeros((k, n), np.uint8), "stop": np.zeros((k, n), np.uint8),
              "steps": np.zeros((k, n), np.uint32)}
    out = L.FrameOut(None, L.dptr(arrays["xyza64"]), L.ptr(arrays["class"], C.c_uint8), L.ptr(arrays["status"], C.c_uint8),
                     L.ptr(arrays["stop"], C.c_uint8), L.ptr(arrays["steps"], C.c_uint32))
    handles = (C.c_void_p * max(k, 1))(*[b._h for b in bufs])
    nsel = np.zeros(max(k, 1), np.uint64)
    per_frame = np.zeros((max(k, 1), 4), np.uint64)
    cap = max(failure_capacity, 1)
    held = [[np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8),
             np.zeros(cap, np.uint32)] for _ in range(max(k, 1))]
    fails = (L.SubsampleFailures * max(k, 1))(*[
        L.SubsampleFailures(failure_capacity, L.ptr(h[0], C.c_uint32), L.ptr(h[1], C.c_uint32), L.ptr(h[2], C.c_uint8), 0,
                            L.ptr(h[3], C.c_uint8) if log_events else None,
                            L.ptr(h[4], C.c_uint32) if log_events else None) for h in held])
    m = None if mask is None else np.ascontiguousarray(mask, np.float64)
    rep = L.GBufferSectionSequenceReport()
    cfg = adaptive or scene.adaptive
    rc = L.lib().grt_gbuffer_shade_section_sequence(scene._s, k, handles, C.byref(cfg),
                                                    L.dptr(m) if m is not None else None,
                                                    tracer._s if tracer is not None else None, C.byref(out),
                                                    L.ptr(nsel, C.c_uint64), fails, L.ptr(per_frame, C.c_uint64),
                                                    C.byref(rep))
    report = {"n_frames": int(rep.n_frames), "n_launches": int(rep.n_launches), "n_selected": int(rep.n_selected),
              "n_held": int(rep.n_held), "n_traced": int(rep.n_traced), "n_missing": int(rep.n_missing),
              "wall_ms": float(rep.wall_ms), "shade_ms": float(rep.shade_ms), "trace_ms": float(rep.trace_ms),
              "top_up": _stats_dict(rep.top_up), "per_frame": per_frame[:k].astype(np.int64)}
    if rc == -errno.ENODATA:
        msg = L.lib().grt_last_error().decode(errors="replace")
        raise GBufferMissing(f"grt_gbuffer_shade_section_sequence failed ({rc}): {msg}", report)
    L.check(rc, "grt_gbuffer_shade_section_sequence")
    arrays["n_supersampled"] = nsel[:k].astype(np.int64)
    arrays["failed_subsamples"], arrays["n_failed_subsamples"], arrays["subsample_events"] = [], [], []
    for f in range(k):
        fp, fs, fst, fsp, fn = held[f]
        got = min(int(fails[f].count), failure_capacity)
        rows = np.stack([fp[:got], fs[:got], fst[:got].astype(np.uint32)], axis=1)
        if not log_events:
            arrays["failed_subsamples"].append(rows)
            arrays["n_failed_subsamples"].append(int(fails[f].count))
            arrays["subsample_events"].append(None)
            continue
        failed = fst[:got] != 0
        events = np.stack([fp[:got], fs[:got], fsp[:got].astype(np.uint32), fn[:got]], axis=1)[~failed]
        arrays["failed_subsamples"].append(rows[failed])
        arrays["n_failed_subsamples"].append(int(fails[f].count) - len(events))
        arrays["subsample_events"].append(events)
    return arrays, report


def orbit_rate(geometry: int, radius: float, a: float, r: float) -> float:
    """d(phi)/dt of the shade pass's disc emitter at radius r (grt_orbit_rate): sqrt(M) /
    (r^1.5 + a sqrt(M)) with M = radius / 2; +0.0 for the flat charts."""
    out = C.c_double()
    L.check(L.lib().grt_orbit_rate(int(geometry), float(radius), float(a), float(r), C.byref(out)), "grt_orbit_rate")
    return float(out.value)


def gbuffer_orbit_uv(shape: L.GBufferShape, object, u, v, radius, time: float):
    """(u', v') of layer arrays (a buffer's or a sub-sample set's) at coordinate time `time`:
    the host restatement of the rule GBuffer.shade_orbit applies on the device
    (grt_gbuffer_orbit_uv).  Disc layers turn about (0.5, 0.5) by -Omega(radius) * time; every
    other layer is returned unchanged."""
    obj = np.ascontiguousarray(object, np.uint8).reshape(-1)
    n = len(obj)
    arr = [np.ascontiguousarray(x, np.float64).reshape(-1) for x in (u, v, radius)]
    if any(len(x) != n for x in arr):
        raise L.GrtError("grt_gbuffer_orbit_uv failed (-22): object, u, v and radius differ in length")
    uo, vo = np.zeros(n, np.float64), np.zeros(n, np.float64)
    L.check(L.lib().grt_gbuffer_orbit_uv(C.byref(shape), n, L.ptr(obj, C.c_uint8), L.dptr(arr[0]), L.dptr(arr[1]),
                                         L.dptr(arr[2]), float(time), L.dptr(uo), L.dptr(vo)), "grt_gbuffer_orbit_uv")
    return uo, vo


def gbuffer_compatible(traced: L.SceneDesc, appearance: L.SceneDesc) -> None:
    """Raise GrtError (-EINVAL, naming the first differing field) unless a g-buffer traced
    under `traced` can be shaded under `appearance`: equal shape keys (grt_gbuffer_compatible)."""
    L.check(L.lib().grt_gbuffer_compatible(C.byref(traced), C.byref(appearance)), "grt_gbuffer_compatible")


def set_two_ended(on: bool = True) -> None:
    """Probe-ordered traces take the tile queue from both ends (grt_set_two_ended): the
    priority wave of each SIMD the longest tiles, the others the shortest.  Scheduling
    only; results are identical in both modes."""
    L.check(L.lib().grt_set_two_ended(1 if on else 0), "grt_set_two_ended")


def set_sequence_group(rays: int = 0) -> None:
    """Rays per launch group of Scene.render_sequence (grt_set_sequence_group; 0 = the
    default 2^22).  A group holds whole frames, at least one.  Scheduling only."""
    L.check(L.lib().grt_set_sequence_group(int(rays)), "grt_set_sequence_group")


def gbuffer_orbit_uv_retarded(shape: L.GBufferShape, object, u, v, radius, lapse, time: float):
    """gbuffer_orbit_uv with every disc layer at its emission time `time + lapse[k]`: the host
    restatement of the rule GBuffer.shade_orbit(retarded=True) applies on the device
    (grt_gbuffer_orbit_uv_retarded).  Returns new (u, v)."""
    obj = np.ascontiguousarray(object, np.uint8).reshape(-1)
    arr = [np.ascontiguousarray(x, np.float64).reshape(-1) for x in (u, v, radius, lapse)]
    n = len(obj)
    if any(len(x) != n for x in arr):
        raise L.GrtError("grt_gbuffer_orbit_uv_retarded failed (-22): object, u, v, radius and lapse differ in length")
    uo, vo = np.empty(n, np.float64), np.empty(n, np.float64)
    L.check(L.lib().grt_gbuffer_orbit_uv_retarded(C.byref(shape), n, L.ptr(obj, C.c_uint8), L.dptr(arr[0]),
                                                  L.dptr(arr[1]), L.dptr(arr[2]), L.dptr(arr[3]), float(time),
                                                  L.dptr(uo), L.dptr(vo)), "grt_gbuffer_orbit_uv_retarded")
    return uo, vo


def load_camera_path(path) -> np.ndarray:
    """A camera-path file: one camera per line, `x,y,z,phi,theta,psi` -- the values
    --camera-position, --phi, --theta and --psi take; blank lines and lines starting with
    `#` are skipped.  Returns an (n, 6) float64 array; ValueError names the bad line."""
    rows = []
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            t = line.strip()
            if not t or t.startswith("#"):
                continue
            parts = [x.strip() for x in t.split(",")]
            if len(parts) != 6:
                raise ValueError(f"{path}:{no}: expected 6 values `x,y,z,phi,theta,psi`, found {len(parts)}")
            try:
                vals = [float(x) for x in parts]
            except ValueError:
                raise ValueError(f"{path}:{no}: `{t}` is not six numbers") from None
            rows.append(vals)
    if not rows:
        raise ValueError(f"{path}:1: the camera path holds no camera")
    return np.array(rows, np.float64)


ARITH_EXACT, ARITH_FUSED = 0, 1


def set_arithmetic(mode) -> None:
    """grt_set_arithmetic: "exact" / 0 (the reference's roundings, default) or "fused" / 1
    (FMA contraction in the light charts' kernels; Kerr-Schild stays exact)."""
    m = {"exact": 0, "fused": 1}.get(mode, mode)
    L.check(L.lib().grt_set_arithmetic(int(m)), "grt_set_arithmetic")


def get_arithmetic() -> int:
    return int(L.lib().grt_get_arithmetic())


def set_tail(threshold: int = -1) -> None:
    """Long-ray hand-off of Kerr-Schild traces (grt_set_tail): -1 auto, 0 off, > 0 the
    live-ray threshold.  Scheduling only; results are identical in every mode."""
    L.check(L.lib().grt_set_tail(int(threshold)), "grt_set_tail")


# --------------------------------------------------------- programmatic scenes ----
@dataclass
class Checker:
    """CheckerMapper (texture.rs:212-257)."""
    beaming_exponent: float
    width: float
    height: float
    color1: Sequence[int]
    color2: Sequence[int]


@dataclass
class Bitmap:
    """TextureMapper (texture.rs:41-102): RGBA8 array (H, W, 4)."""
    beaming_exponent: float
    rgba: np.ndarray


@dataclass
class BlackBody:
    """BlackBodyMapper (texture.rs:104-210)."""
    beaming_exponent: float = 0.0


def srgb_to_xyza(r: int, g: int, b: int, a: int = 255) -> np.ndarray:
    out = np.zeros(4, np.float64)
    L.lib().grt_srgb_to_xyza(r, g, b, a, L.dptr(out))
    return out


def xyz_to_srgb8(xyza, tone_mapping: int = 0, exposure: float = 1.0, device: Optional[int] = None) -> np.ndarray:
    """Output stage (color.rs:204-298): (n,4) f64 XYZA -> (n,3) u8 sRGB.  device=None
    runs the host C++ path (grt_xyz_to_srgb8), an ordinal runs the HIP kernels
    (grt_xyz_to_srgb8_device); both return the reference's bytes."""
    x = np.ascontiguousarray(xyza, np.float64).reshape(-1, 4)
    out = np.zeros((x.shape[0], 3), np.uint8)
    if device is None:
        L.check(L.lib().grt_xyz_to_srgb8(L.dptr(x), x.shape[0], tone_mapping, exposure, L.ptr(out, C.c_uint8)),
                "grt_xyz_to_srgb8")
    else:
        L.check(L.lib().grt_xyz_to_srgb8_device(device, L.dptr(x), x.shape[0], tone_mapping, exposure,
                                                 L.ptr(out, C.c_uint8)), "grt_xyz_to_srgb8_device")
    return out


@dataclass
class Trajectories:
    """steps[k, i] = (t, x^0..x^3, p^0..p^3) of ray k's step i, i < min(n_steps[k], capacity)."""
    steps: np.ndarray
    n_steps: np.ndarray
    stop_reason: np.ndarray
    status: np.ndarray

    def ray(self, k: int) -> np.ndarray:
        return self.steps[k, : min(int(self.n_steps[k]), self.steps.shape[1])]


def ray_at(geometry: int, radius: float, a: float, position, direction):
    """render_ray_at's initial (position, momentum) in the geometry's chart (grt_ray_at)."""
    p, d = np.ascontiguousarray(position, np.float64), np.ascontiguousarray(direction, np.float64)
    po, mo = np.zeros(4), np.zeros(4)
    L.check(L.lib().grt_ray_at(geometry, radius, a, L.dptr(p), L.dptr(d), L.dptr(po), L.dptr(mo)), "grt_ray_at")
    return po, mo


def write_trajectory_csv(path: str, geometry: int, a: float, records) -> None:
    """IntegratedRay::save (ray.rs:35-54) of (n, 9) records."""
    r = np.ascontiguousarray(records, np.float64).reshape(-1, 9)
    L.check(L.lib().grt_write_trajectory_csv(str(path).encode(), geometry, a, L.dptr(r), r.shape[0]),
            "grt_write_trajectory_csv")


def format_f64(v: float) -> str:
    """Rust's Display of an f64 (shortest round-trip digits, positional)."""
    buf = C.create_string_buffer(1200)
    L.lib().grt_format_f64(float(v), buf, 1200)
    return buf.value.decode()


def format_f64_debug(v: float) -> str:
    """Rust's Debug of an f64 ({:?}): Display's digits with ".0" on integral values, and
    exponential notation outside 1e-4 <= |v| < 1e16."""
    import math
    if math.isnan(v) or math.isinf(v):
        return format_f64(v)
    if v != 0.0 and (abs(v) < 1e-4 or abs(v) >= 1e16):
        m, e = repr(float(v)).lower().split("e") if "e" in repr(float(v)).lower() else (repr(float(v)), "0")
        return f"{m.rstrip('0').rstrip('.') if '.' in m else m}e{int(e)}"
    d = format_f64(v)
    return d if "." in d else d + ".0"


def coordinate_system_debug(geometry: int, a: float) -> str:
    """CoordinateSystem's Debug form for a geometry (geometry/*.rs coordinate_system, point.rs:11)."""
    if geometry in (L.GEOM_SCHWARZSCHILD, L.GEOM_EUCLIDEAN_SPHERICAL):
        return "Spherical"
    if geometry == L.GEOM_KERR_BL:
        return f"BoyerLindquist {{ a: {format_f64_debug(a)} }}"
    return "Cartesian"


def duration_debug_2(secs: float) -> str:
    """A Duration's Debug form with two decimals ({:.2?}): the largest of s / ms / us / ns
    with a non-zero integer part, the dropped digits rounded half up."""
    ns = int(round(secs * 1e9))
    for div, unit in ((10 ** 9, "s"), (10 ** 6, "ms"), (10 ** 3, "\u00b5s")):
        if ns >= div:
            h = (ns * 100 + div // 2) // div
            return f"{h // 100}.{h % 100:02d}{unit}"
    return f"{ns}.00ns"


def r_isco(radius: float, a: float) -> float:
    return float(L.lib().grt_r_isco(radius, a))


def blackbody_xyz(temperature: float, redshift: float = 1.0) -> np.ndarray:
    out = np.zeros(3, np.float64)
    L.lib().grt_blackbody_xyz(temperature, redshift, L.dptr(out))
    return out


def kerr_temperature_lut(temperature: float, outer_radius: float, a: float, radius: float, n: int = 1000):
    lr, lt, ri = np.zeros(n), np.zeros(n), C.c_double(0.0)
    L.check(L.lib().grt_kerr_temperature_lut(temperature, outer_radius, a, radius, n, L.dptr(lr), L.dptr(lt),
                                             C.byref(ri)), "KerrTemperatureComputer::new")
    return lr, lt, float(ri.value)


def cartesian_to_spherical(p) -> np.ndarray:
    i, o = np.ascontiguousarray(p, np.float64), np.zeros(4)
    L.lib().grt_cartesian_to_spherical(L.dptr(i), L.dptr(o))
    return o


def cartesian_to_boyer_lindquist(a: float, p) -> np.ndarray:
    i, o = np.ascontiguousarray(p, np.float64), np.zeros(4)
    L.lib().grt_cartesian_to_boyer_lindquist(a, L.dptr(i), L.dptr(o))
    return o


def build_camera(geometry: int, radius: float, a: float, position, velocity, alpha: float, rows: int, cols: int,
                 phi: float = 0.0, theta: float = 0.0, psi: float = 0.0) -> L.CameraDesc:
    """Camera::new (camera.rs:151-196)."""
    cam = L.CameraDesc()
    p, v = np.ascontiguousarray(position, np.float64), np.ascontiguousarray(velocity, np.float64)
    L.check(L.lib().grt_camera_build(geometry, radius, a, L.dptr(p), L.dptr(v), alpha, rows, cols, phi, theta, psi,
                                     C.byref(cam)), "Camera::new")
    return cam


def stationary_velocity(geometry: int, radius: float, a: float, position) -> np.ndarray:
    p, o = np.ascontiguousarray(position, np.float64), np.zeros(4)
    L.lib().grt_stationary_velocity(geometry, radius, a, L.dptr(p), L.dptr(o))
    return o


class SceneBuilder:
    """Assemble a grt_scene_desc in Python, as the reference tests do with
    `create_scene_with_camera` (scene.rs:281-369)."""

    def __init__(self, geometry: int, radius: float = 0.0, a: float = 0.0, horizon_epsilon: float = 0.0):
        self.d = L.SceneDesc()
        self.d.abi_version = L.GRT_ABI_VERSION
        self.d.geometry, self.d.radius, self.d.a, self.d.horizon_epsilon = geometry, radius, a, horizon_epsilon
        self.d.object_hit_opacity_threshold = 0.5
        self._fill_srgb()
        self._keep = []
        self._need_bb = False

    def _fill_srgb(self):
        # inv_compand_srgb (color.rs:301-308) of each 8-bit code; math.pow is the C libm pow
        for i in range(256):
            u = i / 255.0
            self.d.srgb_to_linear[i] = u / 12.92 if u <= 0.04045 else math.pow((u + 0.055) / 1.055, 2.4)

    def integration(self, max_steps: int, max_radius: float, step_size: float, epsilon: float) -> "SceneBuilder":
        self.d.max_steps, self.d.max_radius, self.d.step_size, self.d.epsilon = max_steps, max_radius, step_size, epsilon
        return self

    def camera(self, position, velocity, alpha: float, rows: int, cols: int, phi=0.0, theta=0.0, psi=0.0):
        self.d.camera = build_camera(self.d.geometry, self.d.radius, self.d.a, position, velocity, alpha, rows, cols,
                                     phi, theta, psi)
        return self

    def _texture(self, t) -> L.TextureDesc:
        d = L.TextureDesc()
        d.beaming_exponent = t.beaming_exponent
        if isinstance(t, Checker):
            d.kind = L.TEX_CHECKER
            d.checker_width, d.checker_height = t.width, t.height
            c1, c2 = srgb_to_xyza(*t.color1, 255), srgb_to_xyza(*t.color2, 255)
            c1[3] = c2[3] = 1.0
            for k in range(4):
                d.c1[k], d.c2[k] = c1[k], c2[k]
        elif isinstance(t, Bitmap):
            arr = np.ascontiguousarray(t.rgba, np.uint8)
            assert arr.ndim == 3 and arr.shape[2] == 4
            self._keep.append(arr)
            d.kind = L.TEX_BITMAP
            d.rgba = L.ptr(arr, C.c_uint8)
            d.height, d.width = arr.shape[0], arr.shape[1]
        else:
            d.kind = L.TEX_BLACKBODY
            self._need_bb = True
        return d

    def celestial(self, texture, temperature: float = 0.0) -> "SceneBuilder":
        self.d.celestial = self._texture(texture)
        self.d.celestial_temperature = temperature
        return self

    def add_sphere(self, radius: float, center, texture, temperature: float = 0.0) -> "SceneBuilder":
        o = self.d.objects[self.d.n_objects]
        o.kind, o.radius, o.temperature = L.OBJ_SPHERE, radius, temperature
        for k in range(3):
            o.center[k] = center[k]
        o.texture = self._texture(texture)
        self.d.n_objects += 1
        return self

    def add_disc(self, inner_radius: float, outer_radius: float, texture, temperature: float = 0.0,
                 constant_temperature: Optional[bool] = None) -> "SceneBuilder":
        """Disc with geometry.get_temperature_computer(temperature, inner, outer)."""
        o = self.d.objects[self.d.n_objects]
        o.kind, o.inner_radius, o.outer_radius = L.OBJ_DISC, inner_radius, outer_radius
        const = (self.d.geometry in (L.GEOM_EUCLIDEAN, L.GEOM_EUCLIDEAN_SPHERICAL) if constant_temperature is None
                 else constant_temperature)
        if const:
            o.temp_kind, o.temp_constant = L.TEMP_CONSTANT, temperature
        else:
            spin = 0.0 if self.d.geometry == L.GEOM_SCHWARZSCHILD else self.d.a
            lr, lt, ri = kerr_temperature_lut(temperature, outer_radius, spin, self.d.radius)
            self._keep += [lr, lt]
            o.temp_kind, o.r_isco, o.lut_n = L.TEMP_KERR_LUT, ri, len(lr)
            o.lut_r, o.lut_t = L.dptr(lr), L.dptr(lt)
        o.texture = self._texture(texture)
        self.d.n_objects += 1
        return self

    def add_volumetric_disc(self, inner_radius: float, outer_radius: float, texture, temperature: float = 0.0, *,
                            axis=(0.0, 0.0, 1.0), num_octaves: int = 8, perlin_seed: int = 1,
                            max_steps: int = 50000, step_size: float = 0.002, thickness: float = 0.1,
                            density_multiplier: float = 500.0, brightness_reference_temperature: float = 1000.0,
                            absorption: float = 0.3, scattering: float = 0.4, noise_scale=(1.0, 1.0, 1.0),
                            noise_offset: float = 0.0,
                            constant_temperature: Optional[bool] = None) -> "SceneBuilder":
        """VolumetricDisc::new (volumetric_disc.rs:43-95) with the Disc temperature model."""
        self.add_disc(inner_radius, outer_radius, texture, temperature, constant_temperature)
        o = self.d.objects[self.d.n_objects - 1]
        o.kind = L.OBJ_VOLUMETRIC_DISC
        for k in range(3):
            o.axis[k], o.noise_scale[k] = axis[k], noise_scale[k]
        o.num_octaves, o.perlin_seed, o.march_max_steps, o.march_step_size = num_octaves, perlin_seed, max_steps, step_size
        o.thickness, o.density_multiplier = thickness, density_multiplier
        o.brightness_reference_temperature = brightness_reference_temperature
        o.absorption, o.scattering, o.noise_offset = absorption, scattering, noise_offset
        return self

    def build(self) -> L.SceneDesc:
        if self._need_bb and not self.d.bb_n:
            lt, xyz = np.zeros(1000), np.zeros(3000)
            L.check(L.lib().grt_blackbody_lut(1000, L.dptr(lt), L.dptr(xyz)), "BlackBodyMapper::new")
            self._keep += [lt, xyz]
            self.d.bb_log_t, self.d.bb_xyz, self.d.bb_n = L.dptr(lt), L.dptr(xyz), 1000
        self.d._keepalive = self._keep  # type: ignore[attr-defined]
        return self.d

    def scene(self) -> Scene:
        d = self.build()
        return Scene(C.pointer(d), keepalive=(self, d))
