"""Host side of camera sequences (grt_render_sequence): the cameras, the camera-path file
and the `grt render-sequence` command line.  CPU only.

A sequence renders K cameras over one loaded scene, so its cameras must be exactly the
ones K separate loads would have built: grt_host_scene_camera against the `camera` of a
fresh grt_host_scene_load with the same --camera-position / --phi / --theta / --psi,
byte for byte, for every chart and every camera_velocity mode, and failing where that
load fails.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import RESOURCES, ROOT, SCENES

GRT = ROOT / "gr_raytracer_amd" / "lib" / "grt"

# three path rows per scene: position and all three angles differ
PATHS = {
    "schwarzschild.toml": [((-16.0, 0.0, 3.5), 0.0, -3.142, 0.0), ((-15.0, 4.0, 3.0), 0.1, -3.0, 0.05),
                           ((-12.0, -9.0, 5.0), -0.2, -3.3, -0.1)],
    "kerr.toml": [((-10.0, 0.0, -0.5), 0.0, 1.52, -1.57), ((-9.0, 3.0, -1.0), 0.05, 1.6, -1.5),
                  ((-7.0, -7.0, 1.5), -0.1, 1.45, -1.65)],
    "kerr-bl.toml": [((-10.0, 0.0, -0.5), 0.0, -3.14159, 0.0), ((-9.5, 2.5, -1.0), 0.08, -3.1, 0.02),
                     ((-8.0, -6.0, 2.0), -0.15, -3.2, -0.07)],
    "euclidean.toml": [((-16.0, 0.0, 3.5), 0.0, -3.142, 0.0), ((-10.0, 5.0, 1.0), 0.3, -2.9, 0.2),
                       ((3.0, -12.0, -2.0), -0.4, -3.4, -0.3)],
    "euclidean-spherical.toml": [((-16.0, 0.0, 3.5), 0.0, -3.142, 0.0), ((-10.0, 5.0, 1.0), 0.3, -2.9, 0.2),
                                 ((3.0, -12.0, -2.0), -0.4, -3.4, -0.3)],
}
# the stock scenes leave camera_velocity at its default (StaticObserver); the other two
# modes of configuration.rs:97-110 through a prefix / suffix of the TOML text
MODES = {
    "StaticObserver": lambda s: s,
    "Zamo": lambda s: 'camera_velocity = "Zamo"\n' + s,
    "Explicit": lambda s: s + "\n[camera_velocity.Explicit]\ncomponents = [1.0, 0.0, 0.0, 0.0]\n",
}


def _opts(grt, row, **kw):
    pos, phi, theta, psi = row
    d = dict(width=24, height=20, camera_position=pos, phi=phi, theta=theta, psi=psi, max_steps=1000)
    d.update(kw)
    return grt.GlobalOpts(**d)


def _scene_file(tmp_path, toml, mode):
    if mode == "StaticObserver":
        return SCENES / toml
    p = tmp_path / toml
    p.write_text(MODES[mode]((SCENES / toml).read_text()))
    return p


def _bytes(cam):
    return C.string_at(C.addressof(cam), C.sizeof(cam))


CASES = [(t, "StaticObserver") for t in PATHS] + [("kerr-bl.toml", "Zamo"), ("kerr.toml", "Zamo"),
                                                  ("schwarzschild.toml", "Zamo"), ("euclidean.toml", "Explicit")]


@pytest.mark.parametrize("toml,mode", CASES)
def test_scene_camera_equals_a_fresh_load(grt, tmp_path, toml, mode):
    path = _scene_file(tmp_path, toml, mode)
    rows = PATHS[toml]
    base = grt.HostScene(str(path), _opts(grt, rows[0]), str(RESOURCES))
    seen = set()
    for row in rows:
        fresh = grt.HostScene(str(path), _opts(grt, row), str(RESOURCES))
        cam = base.camera(*row)
        assert _bytes(cam) == _bytes(fresh.desc.camera), (toml, mode, row)
        assert cam.rows == 20 and cam.cols == 24
        seen.add(_bytes(cam))
    assert len(seen) == len(rows)  # the rows are different cameras


@pytest.mark.parametrize("explicit,position,needle", [
    # a static observer inside the horizon: no future-directed four-velocity
    (False, (0.5, 0.0, 0.0), None),
    # the origin of the spherical chart: no orthonormal tetrad
    (False, (0.0, 0.0, 0.0), None),
    # an Explicit velocity normalised at the first camera's radius is not at another
    (True, (-8.0, 0.0, 1.0), "not normalized"),
])
def test_scene_camera_fails_as_the_load_fails(grt, tmp_path, explicit, position, needle):
    good = ((-16.0, 0.0, 3.5), 0.0, -3.142, 0.0)
    row = (position, 0.0, -3.142, 0.0)
    text = (SCENES / "schwarzschild.toml").read_text()
    if explicit:
        stock = grt.HostScene(str(SCENES / "schwarzschild.toml"), _opts(grt, good), str(RESOURCES))
        r0 = float(np.linalg.norm(good[0]))
        vt = float(1.0 / np.sqrt(1.0 - stock.desc.radius / r0))  # g_tt v_t^2 = -1 at r0
        text += f"\n[camera_velocity.Explicit]\ncomponents = [{vt!r}, 0.0, 0.0, 0.0]\n"
    p = tmp_path / "scene.toml"
    p.write_text(text)
    base = grt.HostScene(str(p), _opts(grt, good), str(RESOURCES))
    with pytest.raises(grt.GrtError) as e_load:
        grt.HostScene(str(p), _opts(grt, row), str(RESOURCES))
    with pytest.raises(grt.GrtError) as e_cam:
        base.camera(*row)
    # "<call> failed (-22): <message>": the same code (-EINVAL) and the same message
    msg_load, msg_cam = str(e_load.value).split(" failed ", 1)[1], str(e_cam.value).split(" failed ", 1)[1]
    assert msg_cam == msg_load and msg_cam.startswith("(-22): ")
    assert needle is None or needle in msg_cam
    assert _bytes(base.camera(*good)) == _bytes(base.desc.camera)  # and the scene still builds cameras


def test_camera_path_parser(grt, tmp_path):
    p = tmp_path / "path.txt"
    p.write_text("# x,y,z,phi,theta,psi\n\n-16,0,3.5,0,-3.142,0\n   \n  # indented comment\n"
                 " -15.5 , 1.0, 3.5, 0.01, -3.1, 0.002 \n-1e1,2,3,4,5,6\n")
    cams = grt.load_camera_path(p)
    assert cams.shape == (3, 6) and cams.dtype == np.float64
    assert np.array_equal(cams[0], [-16.0, 0.0, 3.5, 0.0, -3.142, 0.0])
    assert np.array_equal(cams[1], [-15.5, 1.0, 3.5, 0.01, -3.1, 0.002])
    assert np.array_equal(cams[2], [-10.0, 2.0, 3.0, 4.0, 5.0, 6.0])


@pytest.mark.parametrize("text,line", [
    ("-16,0,3.5,0,-3.142,0\n# c\n1,2,3,4,5\n", 3),        # a short row
    ("\n-16,0,3.5,0,-3.142,zero\n", 2),                   # not a number
    ("1,2,3,4,5,6,7\n", 1),                               # a long row
    ("", 1), ("# only a comment\n\n", 1),                 # no camera at all
])
def test_camera_path_errors_name_the_line(grt, tmp_path, text, line):
    p = tmp_path / "path.txt"
    p.write_text(text)
    with pytest.raises(ValueError) as e:
        grt.load_camera_path(p)
    assert f"{p}:{line}:" in str(e.value), str(e.value)
    # the command line reads the same file the same way: a usage error naming the line
    r = subprocess.run([str(GRT), "--config-file", str(SCENES / "euclidean.toml"), "render-sequence",
                        "--camera-path", str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and f"{p}:{line}:" in r.stderr and "usage:" in r.stderr, r.stderr


@pytest.mark.parametrize("args,needle", [
    (["render-sequence"], "--camera-path"),
    (["--gpus", "2", "render-sequence", "--camera-path", "PATH"], "--gpus"),
    (["--devices", "0,1", "render-sequence", "--camera-path", "PATH"], "--devices"),
    (["render-sequence", "--camera-path", "PATH", "--filename-pattern", "frame.png"], "--filename-pattern"),
    (["--raw-out", "raw.bin", "render-sequence", "--camera-path", "PATH"], "--raw-out"),
])
def test_render_sequence_usage_errors(tmp_path, args, needle):
    """Usage errors exit before the scene is loaded or a GPU touched (the config file
    does not even exist)."""
    p = tmp_path / "path.txt"
    p.write_text("-16,0,3.5,0,-3.142,0\n")
    args = [str(p) if a == "PATH" else a for a in args]
    r = subprocess.run([str(GRT), "--config-file", str(tmp_path / "missing.toml")] + args, capture_output=True,
                       text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert needle in r.stderr.splitlines()[0] and "usage:" in r.stderr
    assert not list(tmp_path.glob("*.png"))


def test_sequence_report_layout_matches_header(grt, tmp_path):
    from gr_raytracer_amd import _lib as L

    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grt_api.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(grt_sequence_report), offsetof(grt_sequence_report, wall_ms),\n'
                   '         offsetof(grt_sequence_report, trace_ms), offsetof(grt_sequence_report, supersample_ms));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    R = L.SequenceReport
    assert [int(v) for v in out] == [C.sizeof(R), R.wall_ms.offset, R.trace_ms.offset, R.supersample_ms.offset]
    for name in ("grt_host_scene_camera", "grt_render_sequence", "grt_set_sequence_group"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)


def test_sequence_unit_is_built_and_left_the_other_units_alone(grt):
    """The library carries the sequence unit's kernels for every chart, beside the other
    units' (readable from the .so without a GPU), and the recorded per-kernel code hashes
    of the parent commit's build and of the build that added the unit agree
    (profiles/sequence/kernel_hashes.json, tools/kernel_hashes.py)."""
    import json

    from gr_raytracer_amd import _lib as L

    for geometry in range(5):
        for vol in ("false", "true"):
            seq = L.kernel_symbol(f"grt::seq::integrate_kernel<{geometry}, {vol}>")
            assert seq.endswith("NS_8CamTableE")  # the camera table is its last parameter
    main = L.kernel_symbol("grt::integrate_kernel<1, false>")
    assert "CamTable" not in main and "CamTable" not in L.kernel_symbol("grt::kerr_bl::integrate_kernel<3, false>")
    for name in ("grt::seq::probe_kernel<2>", "grt::seq::shade_kernel<1, 0>", "grt::seq::tail_kernel<2, false>"):
        assert len(L.kernel_code_sha256(L.kernel_symbol(name))) == 64
    doc = json.loads((ROOT / "profiles" / "sequence" / "kernel_hashes.json").read_text())
    assert doc["parent"] == doc["this_change"] and len(doc["parent"]) == doc["n_existing"] > 50
    assert main in doc["parent"] and not any(k.startswith("_ZN3grt3seq") for k in doc["parent"])
    assert all(k.startswith("_ZN3grt3seq") for k in doc["sequence_unit"]) and len(doc["sequence_unit"]) >= 30
