"""Four layers of geodesic.hip in their own headers (csrc/device/geodesic_*.h), one chart dispatch and
one rectangle-pixel rule (CPU only, no GPU call): the recorded comparison with a build of the
parent commit (profiles/geodesic_split/kernel_hashes.json, from tools/kernel_hashes.py) says
that every kernel of the four units kept its code, under the record's old-to-new symbol map,
and the built library has every kernel of the record under its name, once."""
import json

from conftest import ROOT

RECORD = ROOT / "profiles" / "geodesic_split" / "kernel_hashes.json"


def _doc():
    return json.loads(RECORD.read_text())


def test_recorded_kernel_hashes():
    doc = _doc()
    parent, change, renamed = doc["parent"], doc["this_change"], doc["symbol_map"]
    assert set(renamed) <= set(parent) and len(set(renamed.values())) == len(renamed)
    assert {renamed.get(k, k): h for k, h in parent.items()} == change
    assert all(len(h) == 64 for h in parent.values())
    assert len(change) == len(parent) == doc["n_unchanged"] == 168
    assert doc["n_kernels"] == {"parent": 168, "this_change": 168}
    # the five charts' integrate kernels of every unit: exact (0..4), fused (0, 1, 3, 4: Kerr-Schild
    # always runs exact), KerrBL's own (3), sequence (0..4), plain and volumetric
    for ns, charts in (("", range(5)), ("5fused", (0, 1, 3, 4)), ("7kerr_bl", (3,)), ("3seq", range(5))):
        for g in charts:
            if ns == "" and g == 3:
                continue  # the exact KerrBL trace is grt::kerr_bl's
            for vol in (0, 1):
                name = f"_ZN3grt{ns}16integrate_kernelILi{g}ELb{vol}EE"
                assert sum(k.startswith(name) for k in change) == 1, name
    assert doc["library_bytes"]["parent"] > 0 and doc["library_bytes"]["this_change"] > 0
    for site in doc["not_unified"]:
        assert site["site"] and site["reason"]


def test_recorded_kernels_are_in_the_library_once(grt):
    syms = list(grt._lib.kernel_symbols())
    for symbol in _doc()["this_change"]:
        assert syms.count(symbol) == 1, symbol
