"""Host side of the adaptive frames of g-buffer sequences (grt_gbuffer_supersample_sequence,
grt_gbuffer_shade_section_sequence): the exported entry points, the kernels the library
carries for them, the new report's layout, the refusals that need no device, the usage errors
of `--adaptive-stacked` and the recorded kernel hashes.  CPU only.
"""
import ctypes as C
import errno
import json
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT

GRT = ROOT / "gr_raytracer_amd" / "lib" / "grt"


def test_entry_points_are_exported(grt):
    from gr_raytracer_amd import _lib as L

    for name in ("grt_gbuffer_supersample_sequence", "grt_gbuffer_shade_section_sequence"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)
    assert callable(grt.supersample_sequence) and callable(grt.shade_section_sequence)


def test_library_carries_the_stacked_kernels(grt):
    from gr_raytracer_amd import _lib as L

    syms = L.kernel_symbols()
    for kernel in ("gbuffer_shade_sub_stack_kernel", "offsets_stack_kernel", "failures_stack_kernel",
                   "gbuffer_split_stack_flags_kernel"):
        hits = [s for s in syms if s.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1, (kernel, hits)
        assert len(L.kernel_code_sha256(hits[0])) == 64


def test_section_sequence_report_layout_matches_header(grt, tmp_path):
    from gr_raytracer_amd import _lib as L

    fields = ("n_frames", "n_launches", "n_selected", "n_held", "n_traced", "n_missing", "wall_ms", "shade_ms",
              "trace_ms", "top_up")
    src = tmp_path / "size.c"
    offs = "".join(f'  printf("%zu\\n", offsetof(grt_gbuffer_section_sequence_report, {f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grt_api.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(grt_gbuffer_section_sequence_report));\n' + offs + '  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    R = L.GBufferSectionSequenceReport
    assert [int(v) for v in out] == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    assert [f for f, _ in R._fields_] == list(fields)


def test_refusals_that_need_no_device(grt):
    """n = 0 and null arguments are refused before any buffer or device is looked at."""
    from gr_raytracer_amd import _lib as L

    lib = L.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below ends on its arguments
    handles = (C.c_void_p * 1)(None)
    counts = (C.c_uint64 * 1)(0)
    lists = (C.POINTER(C.c_uint32) * 1)()
    ad = grt.default_adaptive()
    x64 = np.zeros(4)
    out = L.FrameOut(None, L.dptr(x64), None, None, None, None)

    def last():
        return lib.grt_last_error().decode()

    assert lib.grt_gbuffer_supersample_sequence(None, 1, handles, 4, counts, lists, None, None) == -errno.EINVAL
    assert "null argument" in last()
    assert lib.grt_gbuffer_supersample_sequence(fake, 1, None, 4, counts, lists, None, None) == -errno.EINVAL
    assert lib.grt_gbuffer_supersample_sequence(fake, 1, handles, 4, None, lists, None, None) == -errno.EINVAL
    assert lib.grt_gbuffer_supersample_sequence(fake, 1, handles, 4, counts, None, None, None) == -errno.EINVAL
    assert lib.grt_gbuffer_supersample_sequence(fake, 0, handles, 4, counts, lists, None, None) == -errno.EINVAL
    assert "at least one buffer" in last()
    assert lib.grt_gbuffer_supersample_sequence(fake, 1, handles, 4, counts, lists, None, None) == -errno.EINVAL
    assert "frame 0: null buffer" in last()
    args = (C.byref(ad), None, None, C.byref(out), None, None, None, None)
    assert lib.grt_gbuffer_shade_section_sequence(None, 1, handles, *args) == -errno.EINVAL and "null argument" in last()
    assert lib.grt_gbuffer_shade_section_sequence(fake, 1, None, *args) == -errno.EINVAL
    assert lib.grt_gbuffer_shade_section_sequence(fake, 1, handles, None, *args[1:]) == -errno.EINVAL
    assert lib.grt_gbuffer_shade_section_sequence(fake, 1, handles, args[0], None, None, None, None, None, None,
                                                  None) == -errno.EINVAL
    assert lib.grt_gbuffer_shade_section_sequence(fake, 0, handles, *args) == -errno.EINVAL
    assert "at least one buffer" in last()
    assert lib.grt_gbuffer_shade_section_sequence(fake, 1, handles, *args) == -errno.EINVAL
    assert "frame 0: null buffer" in last()
    no64 = L.FrameOut(None, None, None, None, None, None)
    assert lib.grt_gbuffer_shade_section_sequence(fake, 1, handles, C.byref(ad), None, None, C.byref(no64), None, None,
                                                  None, None) == -errno.EINVAL
    assert "xyza64" in last()
    with pytest.raises(grt.GrtError, match="at least one buffer"):
        grt.supersample_sequence([], SimpleNamespace(_s=fake), [], 4)


@pytest.mark.parametrize("args,needle", [
    # a missing path or pattern
    (["gbuffer-sequence", "--filename-pattern", "a-%04d.grtg", "--adaptive-stacked"], "--camera-path"),
    (["gbuffer-sequence", "--camera-path", "PATH", "--adaptive-stacked"], "--filename-pattern"),
    (["reshade-sequence", "--frames", "3", "--adaptive-stacked"], "--gbuffer-pattern"),
    (["reshade-sequence", "--adaptive-stacked", "--gbuffer-pattern", "a-%04d.grtg"], "--frames"),
    # no frames
    (["reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg", "--frames", "0", "--adaptive-stacked"], "--frames"),
    # one GPU
    (["--gpus", "2", "gbuffer-sequence", "--camera-path", "PATH", "--filename-pattern", "a-%04d.grtg",
      "--adaptive-stacked"], "--gpus"),
    (["--gpus", "2", "reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg", "--frames", "3", "--adaptive-stacked"],
     "--gpus"),
    (["--devices", "0,1", "reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg", "--frames", "3",
      "--adaptive-stacked"], "--devices"),
    # the flag belongs to the two sequence subcommands
    (["reshade", "--gbuffer", "a.grtg", "--adaptive-stacked"], "--adaptive-stacked"),
])
def test_usage_errors_come_before_the_scene_and_the_gpu(tmp_path, args, needle):
    """Neither the config file nor the .grtg files exist: the run ends on its arguments."""
    p = tmp_path / "path.txt"
    p.write_text("-16,0,3.5,0,-3.142,0\n")
    args = [str(p) if a == "PATH" else a for a in args]
    r = subprocess.run([str(GRT), "--config-file", str(tmp_path / "missing.toml")] + args, capture_output=True,
                       text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert needle in r.stderr.splitlines()[0] and "usage:" in r.stderr, r.stderr
    assert not list(tmp_path.glob("*.png")) and not list(tmp_path.glob("*.grtg")) and not list(tmp_path.glob("*.sub"))


def test_adaptive_names_the_stacked_flag(tmp_path):
    r = subprocess.run([str(GRT), "--config-file", str(tmp_path / "missing.toml"), "reshade-sequence", "--gbuffer-pattern",
                        "a-%d.grtg", "--frames", "2", "--adaptive"], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert r.returncode == 2 and "--adaptive-stacked" in r.stderr.splitlines()[0], r.stderr


def _frame_file(grt, path, rows, cols, max_steps):
    """A hand-written whole-frame .grtg file without layers."""
    L = grt._lib
    n = rows * cols
    info = L.GBufferInfo()
    info.rows, info.cols, info.n_pixels, info.n_layers = rows, cols, n, 0
    info.shape.geometry, info.shape.n_objects, info.shape.radius = L.GEOM_SCHWARZSCHILD, 0, 1.0
    info.camera.rows, info.camera.cols = rows, cols
    info.max_steps, info.max_radius, info.step_size, info.epsilon, info.horizon_epsilon = max_steps, 100.0, 0.01, 1e-5, 1e-4
    arrays = {"status": np.zeros(n, np.uint8), "stop": np.zeros(n, np.uint8), "steps": np.zeros(n, np.uint32),
              "sky_u": np.zeros(n), "sky_v": np.zeros(n), "sky_redshift": np.ones(n),
              "layer_start": np.zeros(n + 1, np.uint64), "object": np.zeros(0, np.uint8), "u": np.zeros(0),
              "v": np.zeros(0), "redshift": np.zeros(0), "radius": np.zeros(0)}
    grt.GBuffer.write_file(path, info, arrays)


@pytest.mark.parametrize("second,needle", [((3, 5, 1000), "--width / --height"), ((4, 6, 1001), "max_steps")])
def test_files_that_disagree_are_usage_errors(grt, tmp_path, second, needle):
    """Two hand-written frame files that differ in size or in max_steps: exit 2 on the headers,
    before the (missing) scene is loaded or the GPU is touched."""
    _frame_file(grt, tmp_path / "f-0.grtg", 4, 6, 1000)
    _frame_file(grt, tmp_path / "f-1.grtg", *second)
    r = subprocess.run([str(GRT), "--width", "6", "--height", "4", "--config-file", str(tmp_path / "missing.toml"),
                        "reshade-sequence", "--gbuffer-pattern", str(tmp_path / "f-%d.grtg"), "--frames", "2",
                        "--filename-pattern", str(tmp_path / "out-%d.png"), "--adaptive-stacked"], capture_output=True,
                       text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert needle in r.stderr.splitlines()[0] and "f-1.grtg" in r.stderr.splitlines()[0] and "usage:" in r.stderr
    assert not list(tmp_path.glob("*.png")) and not list(tmp_path.glob("*.sub"))


def test_recorded_kernel_hashes():
    """profiles/gbuffer/sequence_adaptive_kernel_hashes.json (tools/kernel_hashes.py on a build
    of the parent commit and on a build of this change): every kernel both builds have kept
    its code in all units; the new kernels are listed apart."""
    doc = json.loads((ROOT / "profiles" / "gbuffer" / "sequence_adaptive_kernel_hashes.json").read_text())
    assert doc["parent"] == doc["this_change"] and len(doc["parent"]) == doc["n_existing"] > 100
    assert doc["existing_kernels_unchanged"] is True
    for kernel in ("gbuffer_shade_sub_kernel", "gbuffer_shade_stack_kernel", "average_kernel", "select_kernel",
                   "offsets_kernel", "gbuffer_split_flags_kernel"):
        hits = [k for k in doc["parent"] if k.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1 and len(doc["parent"][hits[0]]) == 64, kernel
    assert sum(k.startswith("_ZN3grt3seq19gbuffer_fill_kernelILi") for k in doc["parent"]) == 5
    new = doc["new_kernels"]
    assert len(new) == doc["n_new"] == 4 and not set(new) & set(doc["parent"])
    for kernel in ("gbuffer_shade_sub_stack_kernel", "offsets_stack_kernel", "failures_stack_kernel",
                   "gbuffer_split_stack_flags_kernel"):
        assert any(k.startswith(f"_ZN3grt{len(kernel)}{kernel}E") for k in new), kernel
