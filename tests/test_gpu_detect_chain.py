"""detect() with decoder_b's fp half computed at the candidates only
(TMREngine.box_fp_at_points): every route returns what "never" returns, bit
for bit, and issues the launches it is meant to.

The shape is the pinned flows' (tests/launch_trace.py: cin 16, emb 64, a 64 x 64
map, 2 images x 3 exemplars, decoder_b one 128-channel tile of two): far below
the floor, so "auto" must keep today's calls; "always" ignores the floor.
"""
import numpy as np
import pytest
import torch

import launch_trace
import tmr_amd
from tmr_amd import _lib, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FL = 20  # tmr_split_conv's flags argument (after the symbol)


class _Proxy(launch_trace._Proxy):
    """tests/launch_trace.py's recorder, also recording the chain extension's symbol."""

    def __getattr__(self, name):
        if name not in _lib.POINTS_CHAIN_SIGNATURES:
            return super().__getattr__(name)
        fn, argtypes = getattr(self._lib, name), _lib.POINTS_CHAIN_SIGNATURES[name][1]

        def recorded(*args):
            self._calls.append([name] + [launch_trace._norm(a, t) for a, t in zip(args, argtypes)])
            return fn(*args)

        return recorded


class record(launch_trace.record):
    def __enter__(self):
        calls = super().__enter__()
        _lib._lib = _Proxy(self.lib, calls)
        return calls


_RUNS = {}


def _detect(name, **knobs):
    """One detect() of the pinned detect flows' inputs with the points route
    forced on and the given engine knobs: (outputs, calls, engine), once per name."""
    if name not in _RUNS:
        P = synth.reference_state_dict(51, cin=16, emb=64, obj_bias=0.3)
        eng = tmr_amd.TMREngine({k: v.to(DEV) for k, v in P.items()}, tmr_amd.PathConfig(emb_dim=64))
        eng.xcorr_algo = "mfma"
        eng.use_graphs = False
        eng.box_at_peaks = "always"
        for k, v in knobs.items():
            setattr(eng, k, v)
        feats = torch.from_numpy(synth.sam_features(52, 2, 16, 32, 32)).to(DEV)
        ex, _ = synth.exemplar_set(53, 2, 3, 64, 64, 3, 9)

        def run():
            with record() as calls:
                out = eng.detect(feats, ex, cls_ths=0.5, iou_threshold=0.5)
                torch.cuda.synchronize()
            return out, calls

        eng.detect_again = run
        _RUNS[name] = run() + (eng,)
    return _RUNS[name]


def _never():
    return _detect("never", box_fp_at_points="never")


def _same(got, want):
    for g, w in zip(got, want):  # logits, boxes, refs: per-image lists
        assert len(g) == len(w) == 2
        for a, b in zip(g, w):
            assert a.shape == b.shape and torch.equal(a, b)  # (the shapes carry the kept counts)


def _stores(calls):
    """(first, count) tile windows of the fp-half (tiled out) launches, in order."""
    return [_lib.split_tile_window_of(c[FL]) for c in calls
            if c[0] == "tmr_split_conv" and c[17] == "null" and c[FL] & _lib.SPLIT_TILED_OUT and c[6] == 2]


def _syms(calls):
    return [c[0] for c in calls]


def test_never_is_the_pinned_points_flow():
    out, calls, eng = _never()
    assert eng.last_box_route == "points" and eng.last_points > 0 and sum(len(x) for x in out[0]) > 0
    assert _stores(calls) == [(0, 0)] and "tmr_split_conv_points" in _syms(calls)


def test_always_takes_the_chain_and_equals_never():
    out, calls, eng = _detect("always", box_fp_at_points="always")
    _same(out, _never()[0])
    assert eng.last_box_route == "points_chain" and eng.last_points == _never()[2].last_points
    # the store launch ran decoder_o's tile only, nothing ran decoder_b's fp half densely
    assert _stores(calls) == [(1, 1)]
    assert "tmr_split_conv_points_chain" in _syms(calls) and "tmr_split_conv_points" not in _syms(calls)
    chain = [c for c in calls if c[0] == "tmr_split_conv_points_chain"]
    assert len(chain) == 1 and _lib.split_tile_window_of(chain[0][-2]) == (0, 1)
    n = _never()[2]
    assert 0.0 < eng.last_shared_flops == n.last_shared_flops / 2  # one of two tiles
    assert eng.last_points_flops == n.last_points_flops * (16 + 64) / 64  # C0 + C1 against C1


def test_dense_fallback_stores_late_and_equals_never():
    zero = {k: 0.0 for k in tmr_amd.TMREngine.BOX_POINTS_CROSSOVER}
    out, calls, eng = _detect("dense", box_fp_at_points="always", box_at_peaks="auto", BOX_POINTS_CROSSOVER=zero)
    _same(out, _never()[0])
    assert eng.last_box_route == "dense"
    assert _stores(calls) == [(1, 1), (0, 1)] and eng.last_shared_flops == _never()[2].last_shared_flops
    assert "tmr_split_conv_points_chain" not in _syms(calls) and "tmr_split_conv_points" not in _syms(calls)


def test_cost_rule_can_choose_the_late_store_and_points():
    """"auto" above the floor with a store cheaper than the chain: decoder_b's
    store tiles run after the finder, then today's points launch."""
    out, calls, eng = _detect("late", box_fp_at_points="auto", FP_AT_POINTS_FLOOR_MACS=0.0, FP_STORE_NS_PER_PIXEL=0.0)
    _same(out, _never()[0])
    assert eng.last_box_route == "points" and _stores(calls) == [(1, 1), (0, 1)]
    assert "tmr_split_conv_points" in _syms(calls) and "tmr_split_conv_points_chain" not in _syms(calls)
    assert eng.last_shared_flops == _never()[2].last_shared_flops


def test_auto_below_the_floor_keeps_todays_calls():
    out, calls, eng = _detect("auto", box_fp_at_points="auto")
    _same(out, _never()[0])
    assert calls == _never()[1] and eng.last_box_route == "points"


def test_a_shape_that_lost_the_cost_rule_goes_back_to_todays_order():
    """"auto": the call after one that ended on a late store issues today's
    calls (one store launch over every tile); once a call's count says the
    chain would have won, the next call leaves decoder_b's tiles out again."""
    _, _, eng = _detect("late", box_fp_at_points="auto", FP_AT_POINTS_FLOOR_MACS=0.0, FP_STORE_NS_PER_PIXEL=0.0)
    today = _never()[2].detect_again()[1]  # (a second call: the packed weights and the bias plane are cached)
    out, calls = eng.detect_again()
    _same(out, _never()[0])
    assert calls == today and _stores(calls) == [(0, 0)] and eng.last_box_route == "points"
    eng.FP_STORE_NS_PER_PIXEL = 1.0e9  # this call (today's order) notes that the chain would win
    out, calls = eng.detect_again()
    assert calls == today
    out, calls = eng.detect_again()
    _same(out, _never()[0])
    assert eng.last_box_route == "points_chain" and _stores(calls) == [(1, 1)]
