"""Which native calls each route issues, pinned.

The value tests hold the maps to 1e-5 / 1e-2 and the detections bit for bit;
a route that only saves time (the shared fp half, the bf16 acc0 and bias
slabs, the image-major heads order, the bf16 f_TM plane, the per-image memo,
the tile windows of the points route) can vanish without moving a value.
tests/golden/launch_trace.json holds, per flow of tests/launch_trace.py, every
libtmr.so call with its scalar arguments and which pointers were NULL
(tools/make_golden_launch_trace.py); each flow is replayed here and must issue
exactly those calls.
"""
import json
import os

import pytest

import launch_trace
from tmr_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace.json")
_golden = {}


def golden():
    if not _golden:
        with open(GOLDEN) as fh:
            _golden.update(json.load(fh))
    return _golden


def test_fixture_covers_the_flows():
    assert set(golden()) == set(launch_trace.FLOWS)
    assert os.path.getsize(GOLDEN) < 100 * 1024


@pytest.mark.parametrize("name", list(launch_trace.FLOWS))
def test_launch_trace(name):
    got = json.loads(json.dumps(launch_trace.run_flow(name)))
    want = golden()[name]
    assert len(got) == len(want), name
    for i, (g, w) in enumerate(zip(got, want)):
        assert [c[0] for c in g] == [c[0] for c in w], f"{name}[{i}]: another sequence of calls"
        for j, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"{name}[{i}] call {j}: {a} != {b}"


def _syms(trace):
    return [c[0] for c in trace]


def test_fixture_holds_the_routes_it_is_for():
    """The committed traces really contain the speed-only routes (so a
    regenerated fixture cannot quietly pin their absence)."""
    g = golden()
    conv = lambda t: [c for c in t if c[0] == "tmr_split_conv"]  # noqa: E731
    FL = 20  # tmr_split_conv's flags argument (after the symbol)
    # E = 3, bf16: the fp-half launch stores bf16 slabs, the heads launch reads them, image-major by 3
    c = conv(g["units_e3_bf16"][0])
    assert any(x[FL] & _lib.SPLIT_OUT_BF16 and x[FL] & _lib.SPLIT_TILED_OUT and x[FL] & _lib.SPLIT_INIT_BF16 for x in c)
    heads = [x for x in c if x[17] == "p"][-1]  # head_w given: the heads launch
    assert heads[FL] & _lib.SPLIT_INIT_BF16 and (heads[FL] >> _lib.SPLIT_UNITS_PER_IMAGE_SHIFT) & 0xff == 3
    x = [c for c in g["units_e3_bf16"][0] if c[0] == "tmr_xcorr"][0][1]
    assert x["out_bf16"] == 1 and x["algo"] == _lib.XCORR_ALGOS["mfma"]
    assert "tmr_split_xpack16" in _syms(g["units_e3_bf16"][0])
    # the points route: objectness tiles (1, 1), then the points launch; the dense fallback: tiles (0, 1)
    wins = [_lib.split_tile_window_of(x[FL]) for x in conv(g["detect_points"][0])]
    assert (1, 1) in wins and "tmr_split_conv_points" in _syms(g["detect_points"][0])
    wins = [_lib.split_tile_window_of(x[FL]) for x in conv(g["detect_dense"][0])]
    assert (1, 1) in wins and (0, 1) in wins and "tmr_split_conv_points" not in _syms(g["detect_dense"][0])
    assert "tmr_nms_small" in _syms(g["detect_graphs_first_call"][0])
    # the memo hit: the second exemplar call neither projects nor runs the fp half
    first, second = g["module_reuse"]
    assert "tmr_pixel_absmax" in _syms(first) and "tmr_pixel_absmax" not in _syms(second)
    assert len(conv(first)) - len(conv(second)) >= 2 and len(conv(second)) == 1
