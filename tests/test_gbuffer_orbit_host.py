"""The host side of the disc's orbital motion (grt_orbit_rate, grt_gbuffer_orbit_uv; CPU only,
no GPU call): the rate against its definition bit for bit, the rotation's properties on
synthetic layer arrays, every -EINVAL, the ctypes mirrors against the header, the stand-alone
caller of tools/, and the usage errors of `grt reshade-orbit`."""
import ctypes as C
import errno
import math
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

GRT = ROOT / "gr_raytracer_amd" / "lib" / "grt"
HEADER = ROOT / "include" / "grt_api.h"


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------------- the rate ----
def _rate(grt, geometry, r_s, a, r):
    L = grt._lib
    out = C.c_double(-1.0)
    rc = L.lib().grt_orbit_rate(geometry, r_s, a, r, C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("geom", ["GEOM_SCHWARZSCHILD", "GEOM_KERR", "GEOM_KERR_BL"])
def test_orbit_rate_is_the_definition(grt, geom):
    """Bits of sm / (pow(r, 1.5) + a sm) with this machine's libm (tests/test_glibc_math.py
    ties the header's pow to it)."""
    g = getattr(grt._lib, geom)
    radii = np.concatenate([np.linspace(0.6, 100.0, 997), [0.6, 1.0, 3.0, 6.0, 100.0]])
    n = 0
    for r_s in (1.0, 2.0):
        for a in (0.0, 0.499, -0.3):
            for r in radii:
                m = 0.5 * r_s
                sm = math.sqrt(m)
                want = sm / (math.pow(float(r), 1.5) + a * sm)
                rc, got = _rate(grt, g, r_s, a, float(r))
                assert rc == 0 and _bits(got)[()] == _bits(want)[()], (geom, r_s, a, r, got, want)
                assert grt.orbit_rate(g, r_s, a, float(r)) == got
                n += 1
    assert n >= 6000


def test_orbit_rate_flat_charts_and_refusals(grt):
    L = grt._lib
    for g in (L.GEOM_EUCLIDEAN, L.GEOM_EUCLIDEAN_SPHERICAL):
        for r in (0.0, 0.6, 7.0, float("inf")):
            rc, got = _rate(grt, g, 1.0, 0.3, r)
            assert rc == 0 and _bits(got)[()] == 0, (g, r, got)  # +0.0, the bit pattern
    rc, _ = _rate(grt, 99, 1.0, 0.0, 6.0)
    assert rc == -errno.EINVAL and "geometry" in L.lib().grt_last_error().decode()
    assert _rate(grt, -1, 1.0, 0.0, 6.0)[0] == -errno.EINVAL
    assert L.lib().grt_orbit_rate(L.GEOM_KERR, 1.0, 0.0, 6.0, None) == -errno.EINVAL
    with pytest.raises(grt.GrtError):
        grt.orbit_rate(99, 1.0, 0.0, 6.0)


# ------------------------------------------------------------------ the rotation ----
def _shape(grt, geometry=None, a=0.499):
    L = grt._lib
    s = L.GBufferShape()
    s.geometry = L.GEOM_KERR_BL if geometry is None else geometry
    s.n_objects, s.radius, s.a = 2, 1.0, a
    s.objects[0].kind, s.objects[0].inner_radius, s.objects[0].outer_radius = L.OBJ_DISC, 3.0, 10.0
    s.objects[1].kind, s.objects[1].radius = L.OBJ_SPHERE, 2.0
    return s


def _layers(n=4000, seed=11):
    """Seeded layer arrays: disc layers (object 0) at distance 0.05 .. 0.5 from (0.5, 0.5) and
    radius 3 .. 10, sphere layers (object 1) anywhere in the unit square, radius +0.0."""
    rng = np.random.default_rng(seed)
    obj = (rng.random(n) < 0.3).astype(np.uint8)
    rho, phi = rng.uniform(0.05, 0.5, n), rng.uniform(-math.pi, math.pi, n)
    disc = obj == 0
    u = np.where(disc, 0.5 + rho * np.cos(phi), rng.random(n))
    v = np.where(disc, 0.5 + rho * np.sin(phi), rng.random(n))
    radius = np.where(disc, rng.uniform(3.0, 10.0, n), 0.0)
    return obj, u, v, radius


TIMES = (1.0, 37.5, -12.25, 700.0)


def test_orbit_uv_rotates_disc_layers_only(grt):
    L = grt._lib
    obj, u, v, radius = _layers()
    disc = obj == 0
    assert disc.sum() > 2000 and (~disc).sum() > 800
    for geometry, a in ((L.GEOM_KERR_BL, 0.499), (L.GEOM_SCHWARZSCHILD, 0.0), (L.GEOM_KERR, -0.3)):
        shape = _shape(grt, geometry, a)
        omega = np.array([grt.orbit_rate(geometry, 1.0, a, float(r)) for r in radius])
        for t in TIMES:
            assert np.abs(omega[disc] * t).max() <= 100.0
            uo, vo = grt.gbuffer_orbit_uv(shape, obj, u, v, radius, t)
            # sphere layers: unchanged bit for bit
            assert np.array_equal(_bits(uo[~disc]), _bits(u[~disc])) and np.array_equal(_bits(vo[~disc]), _bits(v[~disc]))
            # disc layers: the lookup angle decreases by omega t (mod 2 pi) within 1e-12 -- the
            # argument's rounding is <= 100 * 2^-53, sincos and the four products and sums add a
            # few ulp at a distance <= 0.5 -- and the distance from the centre stays within 1e-15
            du, dv, duo, dvo = u[disc] - 0.5, v[disc] - 0.5, uo[disc] - 0.5, vo[disc] - 0.5
            want = np.arctan2(dv, du) - omega[disc] * t
            d = np.mod(np.arctan2(dvo, duo) - want + math.pi, 2.0 * math.pi) - math.pi
            assert np.abs(d).max() <= 1e-12, (geometry, t, np.abs(d).max())
            assert np.abs(np.hypot(duo, dvo) - np.hypot(du, dv)).max() <= 1e-15, (geometry, t)
            assert np.abs(uo[disc] - u[disc]).max() > 0.01  # and they did move (|omega t| >= 0.02 at t = 1)


def test_orbit_uv_identities(grt):
    L = grt._lib
    obj, u, v, radius = _layers()
    shape = _shape(grt)
    for t in (0.0, -0.0):  # th == 0: unchanged
        uo, vo = grt.gbuffer_orbit_uv(shape, obj, u, v, radius, t)
        assert np.array_equal(_bits(uo), _bits(u)) and np.array_equal(_bits(vo), _bits(v))
    for g in (L.GEOM_EUCLIDEAN, L.GEOM_EUCLIDEAN_SPHERICAL):  # omega == 0: unchanged at every time
        uo, vo = grt.gbuffer_orbit_uv(_shape(grt, g), obj, u, v, radius, 37.5)
        assert np.array_equal(_bits(uo), _bits(u)) and np.array_equal(_bits(vo), _bits(v))
    # omega t not finite (a disc layer at radius 0 with a = 0: omega = inf): unchanged
    r0 = radius.copy()
    r0[obj == 0] = 0.0
    uo, vo = grt.gbuffer_orbit_uv(_shape(grt, L.GEOM_SCHWARZSCHILD, 0.0), obj, u, v, r0, 1.0)
    assert np.array_equal(_bits(uo), _bits(u)) and np.array_equal(_bits(vo), _bits(v))
    # n_layers = 0
    e = np.zeros(0)
    uo, vo = grt.gbuffer_orbit_uv(shape, np.zeros(0, np.uint8), e, e, e, 1.0)
    assert uo.shape == vo.shape == (0,)


def _call(grt, shape, obj, u, v, radius, t, uo, vo, n=None):
    L = grt._lib
    p = lambda x: None if x is None else L.dptr(x)  # noqa: E731
    return L.lib().grt_gbuffer_orbit_uv(C.byref(shape) if shape is not None else None, len(obj) if n is None else n,
                                        None if obj is None else L.ptr(obj, C.c_uint8), p(u), p(v), p(radius), t, p(uo),
                                        p(vo))


def test_orbit_uv_aliased_outputs(grt):
    obj, u, v, radius = _layers()
    shape = _shape(grt)
    uo, vo = grt.gbuffer_orbit_uv(shape, obj, u, v, radius, 37.5)
    ua, va = u.copy(), v.copy()
    assert _call(grt, shape, obj, ua, va, radius, 37.5, ua, va) == 0
    assert np.array_equal(_bits(ua), _bits(uo)) and np.array_equal(_bits(va), _bits(vo))
    assert not np.array_equal(_bits(ua), _bits(u))


def test_orbit_uv_refusals(grt):
    L = grt._lib
    obj, u, v, radius = _layers(64)
    shape = _shape(grt)
    uo, vo = np.full(64, 9.0), np.full(64, 9.0)
    good = [shape, obj, u, v, radius, 1.0, uo, vo]
    assert _call(grt, *good) == 0
    uo[:], vo[:] = 9.0, 9.0
    for k in (0, 2, 3, 4, 6, 7):  # every pointer but `object`, then that one
        args = list(good)
        args[k] = None
        assert _call(grt, *args) == -errno.EINVAL, k
    assert _call(grt, shape, None, u, v, radius, 1.0, uo, vo, n=64) == -errno.EINVAL
    for t in (float("nan"), float("inf"), float("-inf")):
        assert _call(grt, shape, obj, u, v, radius, t, uo, vo) == -errno.EINVAL, t
        assert "time" in L.lib().grt_last_error().decode()
    bad = obj.copy()
    bad[63] = 2  # == n_objects
    assert _call(grt, shape, bad, u, v, radius, 1.0, uo, vo) == -errno.EINVAL
    assert "object" in L.lib().grt_last_error().decode()
    unknown = _shape(grt, 99)
    assert _call(grt, unknown, obj, u, v, radius, 1.0, uo, vo) == -errno.EINVAL
    assert np.all(uo == 9.0) and np.all(vo == 9.0)  # a refused call writes nothing
    with pytest.raises(grt.GrtError):
        grt.gbuffer_orbit_uv(shape, obj, u[:10], v, radius, 1.0)
    with pytest.raises(grt.GrtError):
        grt.gbuffer_orbit_uv(shape, bad, u, v, radius, 1.0)


# ----------------------------------------------------------- mirrors and the tools ----
_CTYPE = {"double": C.c_double, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
          "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float), "uint8_t*": C.POINTER(C.c_uint8),
          "uint64_t*": C.POINTER(C.c_uint64), "grt_scene*": C.c_void_p, "grt_gbuffer*": C.c_void_p}


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = re.sub(r"\bconst\b", "", p).strip()
        typ = re.sub(r"\s*\b\w+$", "", p)  # drop the parameter's name
        out.append(re.sub(r"\s+", "", typ))
    return out


def test_ctypes_mirrors_match_the_header(grt):
    L = grt._lib
    structs = {"grt_gbuffer_shape*": C.POINTER(L.GBufferShape), "grt_frame_out*": C.POINTER(L.FrameOut),
               "grt_adaptive_config*": C.POINTER(L.AdaptiveConfig),
               "grt_subsample_failures*": C.POINTER(L.SubsampleFailures),
               "grt_gbuffer_section_report*": C.POINTER(L.GBufferSectionReport)}
    for name in ("grt_orbit_rate", "grt_gbuffer_orbit_uv", "grt_gbuffer_shade_times", "grt_gbuffer_shade_section_at"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)
        fn = getattr(L.lib(), name)
        want = [structs.get(t) or _CTYPE[t] for t in _declaration(name)]
        assert fn.restype is C.c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    # the entry at a time takes grt_gbuffer_shade_section's arguments plus the time
    at, static = _declaration("grt_gbuffer_shade_section_at"), _declaration("grt_gbuffer_shade_section")
    assert at == static + ["double"]
    assert list(L.lib().grt_gbuffer_shade_section_at.argtypes)[:-1] == list(L.lib().grt_gbuffer_shade_section.argtypes)


def test_stand_alone_caller_builds_and_passes(tmp_path):
    """tools/orbit_uv_main.cpp (the program CPU sanitizer builds run) links against the two host
    files alone and passes; built here without a sanitizer."""
    exe = tmp_path / "orbit_uv_main"
    host = ROOT / "gr_raytracer_amd" / "csrc" / "host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tools" / "orbit_uv_main.cpp"), str(host / "orbit.cpp"), str(host / "errors.cpp"), "-o",
                    str(exe)], check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ------------------------------------------------------------------------- the CLI ----
def _run(*args):
    return subprocess.run([str(GRT), *args], capture_output=True, text=True, timeout=60)


def test_cli_usage_errors(grt, tmp_path):
    from test_gbuffer_host import _synthetic

    scene = str(SCENES / "schwarzschild.toml")
    pat = str(tmp_path / "f-%04d.png")

    def usage_error(*args):
        r = _run("--config-file", scene, "reshade-orbit", *args)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and "usage: grt" in r.stderr, r.stderr
        assert "reshade-orbit --gbuffer" in r.stderr  # the usage text names the subcommand
        return r.stderr

    assert "reshade-orbit needs --gbuffer" in usage_error("--times", "0,1,3", "--filename-pattern", pat)
    assert "reshade-orbit needs --times" in usage_error("--gbuffer", "a.grtg", "--filename-pattern", pat)
    for bad in ("0,1", "0,1,2,3", "0,x,3", "0,1,2.5", "0,1,-1", "nan,1,2", "0,inf,2", ""):
        err = usage_error("--gbuffer", "a.grtg", "--times=" + bad, "--filename-pattern", pat)
        assert "--times" in err, (bad, err)
    assert "K must be at least 1" in usage_error("--gbuffer", "a.grtg", "--times", "0,1,0", "--filename-pattern", pat)
    assert "reshade-orbit needs --filename-pattern" in usage_error("--gbuffer", "a.grtg", "--times", "0,1,3")
    assert "--filename-pattern needs one %d" in usage_error("--gbuffer", "a.grtg", "--times", "0,1,3",
                                                            "--filename-pattern", str(tmp_path / "f.png"))
    assert "--raw-out-pattern needs one %d" in usage_error("--gbuffer", "a.grtg", "--times", "0,1,3", "--filename-pattern",
                                                           pat, "--raw-out-pattern", str(tmp_path / "f.raw"))
    assert "do not apply" in _run("--gpus", "2", "--config-file", scene, "reshade-orbit", "--gbuffer", "a.grtg", "--times",
                                  "0,1,3", "--filename-pattern", pat).stderr
    # the frame must be the file's (checked before the GPU is touched)
    info, arrays = _synthetic(grt, [0] * 6)
    info.row0 = info.col0 = 0
    info.camera.rows, info.camera.cols = info.rows, info.cols
    path = tmp_path / "frame.grtg"
    grt.GBuffer.write_file(path, info, arrays)
    r = _run("--width", "64", "--height", "48", "--config-file", scene, "reshade-orbit", "--gbuffer", str(path), "--times",
             "0,1,3", "--filename-pattern", pat)
    assert r.returncode == 2 and "--width / --height must be the g-buffer's frame, 2 x 3" in r.stderr
    # a missing or damaged file is an error message, not a crash
    path.write_bytes(path.read_bytes()[:-3])
    r = _run("--width", "2", "--height", "3", "--config-file", scene, "reshade-orbit", "--gbuffer", str(path), "--times",
             "0,1,3", "--filename-pattern", pat)
    assert r.returncode == 1 and "file length" in r.stderr
    assert not list(tmp_path.glob("f-*.png"))


# --------------------------------------------------------------- recorded hashes ----
KERNELS = ("gbuffer_shade_times_kernel", "gbuffer_orbit_rate_kernel", "gbuffer_shade_at_kernel",
           "gbuffer_shade_sub_at_kernel")


def test_new_kernels_are_in_the_library(grt):
    syms = grt._lib.kernel_symbols()
    for kernel in KERNELS:
        assert sum(s.startswith(f"_ZN3grt{len(kernel)}{kernel}E") for s in syms) == 1, kernel


def test_recorded_kernel_hashes():
    """profiles/gbuffer/orbit_kernel_hashes.json (tools/kernel_hashes.py on a build of the parent
    commit and on a build of this change): every kernel of the parent kept its code in all units,
    the three static deferred-shade kernels among them; the four kernels of the orbital motion
    are new, without scratch or VGPR spills."""
    import json

    doc = json.loads((ROOT / "profiles" / "gbuffer" / "orbit_kernel_hashes.json").read_text())
    assert doc["parent"] == doc["this_change"] and len(doc["parent"]) == doc["n_existing"] > 160
    assert doc["existing_kernels_unchanged"] is True
    for kernel in ("gbuffer_shade_kernel", "gbuffer_shade_sub_kernel", "gbuffer_shade_stack_kernel",
                   "gbuffer_shade_sub_stack_kernel", "average_kernel"):
        hits = [k for k in doc["parent"] if k.startswith(f"_ZN3grt{len(kernel)}{kernel}E")]
        assert len(hits) == 1 and len(doc["parent"][hits[0]]) == 64, kernel
    assert sum("integrate_kernelILi" in k for k in doc["parent"]) >= 10  # every chart, every unit
    new = doc["new_kernels"]
    assert len(new) == doc["n_new"] == 4 and not set(new) & set(doc["parent"])
    for kernel in KERNELS:
        assert any(k.startswith(f"_ZN3grt{len(kernel)}{kernel}E") for k in new), kernel
        res = doc["new_kernel_resources"][kernel]
        assert 0 < res["vgprs"] <= 128 and res["scratch_bytes"] == 0 and res["vgprs_spilled"] == 0, res
