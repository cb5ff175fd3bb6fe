"""grt_set_class_order (the Schwarzschild tile queue grouped by sincos case) without a GPU:
the knob's range, and the CPU model of the order against the committed census."""
import json
import sys

import pytest

from conftest import ROOT


def test_knob_rejects_values_outside_its_range_and_round_trips(grt):
    L = grt._lib
    lib = L.lib()
    try:
        for mode in (0, 1, 2, -1):
            L.check(lib.grt_set_class_order(mode))
            assert lib.grt_get_class_order() == mode
        for bad in (-2, 3, 7):
            with pytest.raises(L.GrtError):
                L.check(lib.grt_set_class_order(bad))
            assert lib.grt_get_class_order() == -1  # a refused value changes nothing
    finally:
        lib.grt_set_class_order(-1)


def test_model_reproduces_the_census_taylor_share():
    """tools/class_order_model.py at C2's camera (a quarter of the frame's resolution: the
    share does not depend on it) against the measured split of the straight-line paths,
    Taylor 16 : table 74 (profiles/div_ok/paths_c2_census.json)."""
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import class_order_model as M
    finally:
        sys.path.pop(0)
    m = M.model((-16.0, 0.0, 3.5), M.math.pi / 4, 375)
    assert abs(m["taylor_share_of_escaping"] - 0.178) <= 0.02, m
    # partitioning the tiles by class leaves the straddling tiles' share, whatever the width
    mixed = m["mixed_fraction"]
    assert mixed["by_class"]["10"] < mixed["row_major"]["4"] < mixed["row_major"]["10"]
    assert abs(mixed["by_class"]["1"] - m["straddling_tiles"] / m["tiles"]) < 1e-12
    json.dumps(m)
