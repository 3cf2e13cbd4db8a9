"""The size / layout queries of the conv launchers are pinned, exactly: tools/host_queries.py calls them over a grid of
shapes, at the default options and with RING_WGS, RING_SC, CONVG_BW8 and CONVG_PERSIST changed one at a time, and
host_queries_expected.json holds every value. The file was written by ``tools/host_queries.py --write`` from the tree
before each kernel family's launch planning was gathered into one geometry function, so a planner that disagrees
with the launchers it replaced shows here as a changed value (no device needed: without one the CU count falls back
to 256, the MI355X's)."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_queries_expected.json")

with open(EXPECTED) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def hq():
    sys.path[:0] = [os.path.join(REPO, "tools")]
    import host_queries
    if not os.path.exists(host_queries.LIB):
        pytest.skip("library not built")
    return host_queries, host_queries.load()


def test_expected_file_covers_the_grid(hq):
    tool, _ = hq
    assert sorted(WANT) == sorted(tool.OPTION_SETS)
    for key in tool.OPTION_SETS:
        assert {q: len(v) for q, v in WANT[key].items()} == {q: len(rows) for q, rows in tool.QUERIES.items()}
    # the grid reaches both sides of what the planners decide: both brick widths, a refused persistent form, and a
    # ring split that changes with the grid target
    d, b0 = WANT["default"], WANT["CONVG_BW8=0"]
    assert d["u3d_convg_brick_gn_nparts"] != b0["u3d_convg_brick_gn_nparts"]
    assert 0 in d["u3d_convg_brick_gn_nparts"] and any(d["u3d_convg_brick_gn_nparts"])
    assert not any(WANT["CONVG_PERSIST=0"]["u3d_convg_brick_gn_nparts"])
    assert d["u3d_conv32_ring_wps"] != WANT["RING_WGS=7"]["u3d_conv32_ring_wps"]
    assert d["u3d_conv32_ring_q_stats_ws_floats"] != WANT["RING_SC=4"]["u3d_conv32_ring_q_stats_ws_floats"]


@pytest.mark.parametrize("key", sorted(WANT))
def test_host_queries(hq, key):
    tool, h = hq
    before = tool.collect(h, None) if key != "default" else None
    got = tool.collect(h, tool.OPTION_SETS[key])
    bad = tool.mismatches(got, WANT[key])
    assert not bad, f"{len(bad)} values differ, first: {bad[:5]}"
    assert before is None or tool.collect(h, None) == before  # the option was restored
