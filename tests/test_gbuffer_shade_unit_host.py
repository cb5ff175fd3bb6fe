"""The deferred shade in its own unit (csrc/device/gbuffer_shade.hip; CPU only, no GPU call):
its eight kernels are in the built library under their names, once each, and the recorded
comparison with a build of the parent commit (profiles/gbuffer/shade_unit_kernel_hashes.json,
from tools/kernel_hashes.py and the compiler's kernel-resource-usage remarks) says what the
move promised -- every other kernel kept its code in all units, and the seven shading kernels
have no scratch, no spilled VGPRs and the parent's occupancy."""
import json

from conftest import ROOT

SHADING = ("gbuffer_shade_kernel", "gbuffer_shade_sub_kernel", "gbuffer_shade_sub_stack_kernel",
           "gbuffer_shade_stack_kernel", "gbuffer_shade_times_kernel", "gbuffer_shade_at_kernel",
           "gbuffer_shade_sub_at_kernel")
KERNELS = SHADING + ("gbuffer_orbit_rate_kernel",)


def _prefix(kernel):
    return f"_ZN3grt{len(kernel)}{kernel}E"


def test_kernels_are_in_the_library_once(grt):
    syms = grt._lib.kernel_symbols()
    for kernel in KERNELS:
        assert sum(s.startswith(_prefix(kernel)) for s in syms) == 1, kernel


def test_recorded_kernel_hashes():
    doc = json.loads((ROOT / "profiles" / "gbuffer" / "shade_unit_kernel_hashes.json").read_text())
    parent, change = doc["parent"], doc["this_change"]
    assert parent == change and len(parent) == doc["n_unchanged"] > 150
    assert all(len(h) == 64 for h in parent.values())
    # the five charts' integrate kernels of every unit: exact (0..4), fused (0, 1, 3, 4: Kerr-Schild
    # always runs exact), KerrBL's own (3), sequence (0..4), plain and volumetric
    for ns, charts in (("", range(5)), ("5fused", (0, 1, 3, 4)), ("7kerr_bl", (3,)), ("3seq", range(5))):
        for g in charts:
            if ns == "" and g == 3:
                continue  # the exact KerrBL trace is grt::kerr_bl's
            for vol in (0, 1):
                name = f"_ZN3grt{ns}16integrate_kernelILi{g}ELb{vol}EE"
                assert sum(k.startswith(name) for k in parent) == 1, name
    assert sum(k.startswith(_prefix("gbuffer_orbit_rate_kernel")) for k in parent) == 1
    changed = doc["changed_kernels"]
    assert set(changed) == set(SHADING) and doc["n_changed"] == 7
    for kernel, e in changed.items():
        assert e["symbol"].startswith(_prefix(kernel)) and e["symbol"] not in parent, kernel
        assert len(e["parent_sha256"]) == len(e["this_change_sha256"]) == 64
        assert e["code_identical"] == (e["parent_sha256"] == e["this_change_sha256"])
        new, old = e["this_change"], e["parent"]
        assert new["scratch_bytes"] == 0 and new["vgprs_spilled"] == 0, (kernel, new)
        assert 0 < new["vgprs"] <= 128 and new["waves_per_simd"] >= old["waves_per_simd"] >= 4, (kernel, new, old)
        assert new["lds_bytes"] == old["lds_bytes"]
    assert doc["library_bytes"]["parent"] > 0 and doc["library_bytes"]["this_change"] > 0
