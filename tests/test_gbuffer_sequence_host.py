"""Host side of the geometry buffers of a camera sequence (grt_gbuffer_trace_sequence,
grt_gbuffer_shade_sequence): the exported entry points, the kernels the library carries for
them, the report's layout, the usage errors of `grt gbuffer-sequence` / `grt reshade-sequence`
and the recorded kernel hashes.  CPU only.
"""
import ctypes as C
import json
import subprocess

import pytest

from conftest import ROOT

GRT = ROOT / "gr_raytracer_amd" / "lib" / "grt"


def test_entry_points_are_exported(grt):
    from gr_raytracer_amd import _lib as L

    for name in ("grt_gbuffer_trace_sequence", "grt_gbuffer_shade_sequence"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)
    assert callable(grt.shade_sequence) and callable(grt.Scene.trace_gbuffer_sequence)


def test_library_carries_the_sequence_fill_and_the_stack_shade(grt):
    """grt::seq::gbuffer_fill_kernel for all five charts, the camera table its last parameter;
    the other units' fill kernels without one; the stack shade and the rebase kernels."""
    from gr_raytracer_amd import _lib as L

    for geometry in range(5):
        seq = L.kernel_symbol(f"grt::seq::gbuffer_fill_kernel<{geometry}>")
        assert seq.endswith("NS_8CamTableE"), seq
        assert len(L.kernel_code_sha256(seq)) == 64
    for name in ("grt::gbuffer_fill_kernel<1>", "grt::kerr_bl::gbuffer_fill_kernel<3>"):
        assert "CamTable" not in L.kernel_symbol(name)
    syms = L.kernel_symbols()
    for kernel in ("gbuffer_shade_stack_kernel", "gbuffer_rebase_kernel"):
        hits = [s for s in syms if s.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1, (kernel, hits)
        assert len(L.kernel_code_sha256(hits[0])) == 64


def test_gbuffer_sequence_report_layout_matches_header(grt, tmp_path):
    from gr_raytracer_amd import _lib as L

    fields = ("n_frames", "n_launches", "frames_per_launch", "n_traces", "wall_ms", "trace_ms", "fill_ms")
    src = tmp_path / "size.c"
    offs = "".join(f'  printf("%zu\\n", offsetof(grt_gbuffer_sequence_report, {f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grt_api.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(grt_gbuffer_sequence_report));\n' + offs + '  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    R = L.GBufferSequenceReport
    assert [int(v) for v in out] == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    assert [f for f, _ in R._fields_] == list(fields)


@pytest.mark.parametrize("args,needle", [
    # a missing path or pattern
    (["gbuffer-sequence", "--filename-pattern", "a-%04d.grtg"], "--camera-path"),
    (["gbuffer-sequence", "--camera-path", "PATH"], "--filename-pattern"),
    (["reshade-sequence", "--frames", "3"], "--gbuffer-pattern"),
    (["reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg"], "--frames"),
    # a pattern without exactly one integer conversion
    (["gbuffer-sequence", "--camera-path", "PATH", "--filename-pattern", "a.grtg"], "--filename-pattern"),
    (["gbuffer-sequence", "--camera-path", "PATH", "--filename-pattern", "a-%d-%d.grtg"], "--filename-pattern"),
    (["gbuffer-sequence", "--camera-path", "PATH", "--filename-pattern", "a-%s.grtg"], "--filename-pattern"),
    (["reshade-sequence", "--gbuffer-pattern", "a.grtg", "--frames", "3"], "--gbuffer-pattern"),
    (["reshade-sequence", "--gbuffer-pattern", "a-%d-%d.grtg", "--frames", "3"], "--gbuffer-pattern"),
    (["reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg", "--frames", "3", "--filename-pattern", "out.png"],
     "--filename-pattern"),
    (["--raw-out", "raw.bin", "reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg", "--frames", "3"], "--raw-out"),
    # no frames
    (["reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg", "--frames", "0"], "--frames"),
    # the stacked calls are 1 spp: --adaptive names the per-frame route
    (["gbuffer-sequence", "--camera-path", "PATH", "--filename-pattern", "a-%04d.grtg", "--adaptive"], "--adaptive"),
    (["reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg", "--frames", "3", "--adaptive"], "--adaptive"),
    # one GPU
    (["--gpus", "2", "gbuffer-sequence", "--camera-path", "PATH", "--filename-pattern", "a-%04d.grtg"], "--gpus"),
    (["--devices", "0,1", "reshade-sequence", "--gbuffer-pattern", "a-%04d.grtg", "--frames", "3"], "--devices"),
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
    if "--adaptive" in args:
        assert "reshade --adaptive" in r.stderr.splitlines()[0]
    assert not list(tmp_path.glob("*.png")) and not list(tmp_path.glob("*.grtg"))


def test_camera_path_errors_name_the_line(tmp_path):
    p = tmp_path / "path.txt"
    p.write_text("-16,0,3.5,0,-3.142,0\n1,2,3\n")
    r = subprocess.run([str(GRT), "--config-file", str(tmp_path / "missing.toml"), "gbuffer-sequence", "--camera-path",
                        str(p), "--filename-pattern", "a-%d.grtg"], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert r.returncode == 2 and f"{p}:2:" in r.stderr and "usage:" in r.stderr, r.stderr


def test_recorded_kernel_hashes():
    """profiles/gbuffer/sequence_kernel_hashes.json (tools/kernel_hashes.py on a build of the
    parent commit and on a build of this change): every kernel both builds have kept its
    code, the two single-buffer shade kernels among them; the new kernels are listed apart."""
    doc = json.loads((ROOT / "profiles" / "gbuffer" / "sequence_kernel_hashes.json").read_text())
    assert doc["parent"] == doc["this_change"] and len(doc["parent"]) == doc["n_existing"] > 50
    assert doc["existing_kernels_unchanged"] is True
    for kernel in ("gbuffer_shade_kernel", "gbuffer_shade_sub_kernel"):
        hits = [k for k in doc["parent"] if k.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1 and doc["parent"][hits[0]] == doc["this_change"][hits[0]], kernel
        assert len(doc["parent"][hits[0]]) == 64
    new = doc["new_kernels"]
    assert len(new) == doc["n_new"] and not set(new) & set(doc["parent"])
    assert sum(k.startswith("_ZN3grt3seq19gbuffer_fill_kernelILi") for k in new) == 5
    assert any(k.startswith("_ZN3grt26gbuffer_shade_stack_kernelE") for k in new)
    assert any(k.startswith("_ZN3grt21gbuffer_rebase_kernelE") for k in new)
    # the other units' fill kernels are existing ones, unchanged
    assert any(k.startswith("_ZN3grt19gbuffer_fill_kernelILi1EE") for k in doc["parent"])
    assert any(k.startswith("_ZN3grt7kerr_bl19gbuffer_fill_kernelILi3EE") for k in doc["parent"])
