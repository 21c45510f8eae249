"""CPU-only: the plan field and the floor of TMREngine.box_fp_at_points
(decoder_b's fp half at the candidates only)."""
import numpy as np
import pytest

import tmr_amd
from tmr_amd import _lib as L
from tmr_amd.decoder_plan import decoder_plan, fp_late_bound_macs
from tmr_amd.engine import TMREngine


def _plan(precision="fp32", E=3, B=2, fusion=True, have_feats=True, **kw):
    ui = list(np.repeat(np.arange(B), E))
    return decoder_plan(tmr_amd.PathConfig(precision=precision, fusion=fusion), True, True, False, have_feats, len(ui),
                        B, ui, **kw)


def test_plan_field_defaults_off_and_moves_only_the_store_window():
    off = _plan(box_later=True, nbt=2)
    on = _plan(box_later=True, nbt=2, fp_late=True)
    assert not off.fp_late and on.fp_late
    rest = lambda p: {k: v for k, v in vars(p).items() if k != "fp_late"}  # noqa: E731
    assert rest(on) == rest(off)
    # off: today's word; on: decoder_o's tiles (2, 2) of 4 first, decoder_b's (0, 2) in the late launch
    assert off.fp_store_flags(4) == off.fp_flags == 39 and off.fp_window(4) == (0, 0)
    assert on.fp_store_flags(4) == 39 | 2 << 16 | 2 << 24 and on.fp_store_flags(4, late=True) == 39 | 2 << 24
    assert on.fp_window(4) == (2, 2) and on.fp_window(4, late=True) == (0, 2)
    assert on.heads_flags(*on.window(4)) == off.heads_flags(*off.window(4)) and on.points_flags() == off.points_flags()


@pytest.mark.parametrize("kw", [dict(), dict(nbt=2), dict(box_later=True, nbt=0), dict(box_later=True, nbt=2, E=1),
                                dict(box_later=True, nbt=2, have_feats=False),
                                dict(box_later=True, nbt=2, precision="bf16"),
                                dict(box_later=True, nbt=2, precision="f16"),
                                dict(box_later=True, nbt=2, fusion=False)])
def test_plan_field_needs_the_shared_folded_fp32_points_route(kw):
    """Asked for, it stays off without box_later, without decoder_b tiles,
    unshared (E = 1), unfolded, without fusion, and under the one-term
    engines (their acc0 is a bf16 slab or its rounding is another's)."""
    assert not _plan(fp_late=True, **kw).fp_late


def test_floor_arithmetic():
    """The bound is decoder_b's store tiles in MACs: B H W x 128 nbt x C0 ks^2.
    The pinned flows (cin 16, 64 x 64, 2 images, one tile) are under the floor
    by more than two orders of magnitude, config B (256 features, 128 x 128, 64 images,
    8 tiles) above it."""
    assert fp_late_bound_macs(2, 64, 64, 1, 16, 3) == 2 * 64 * 64 * 128 * 16 * 9 == 150994944
    assert fp_late_bound_macs(64, 128, 128, 8, 256, 3) == 2473901162496
    eng = TMREngine({}, tmr_amd.PathConfig())
    assert eng.box_fp_at_points == "auto"
    assert 100 * 150994944 < eng.FP_AT_POINTS_FLOOR_MACS < 2473901162496
    assert not eng._fp_at_points_wanted(2, 64, 64, 1, 16, 3) and eng._fp_at_points_wanted(64, 128, 128, 8, 256, 3)
    # a shape whose last call lost the cost rule keeps today's order until a call's count wins it
    assert eng._fp_chain_wins(176521, 64, 128, 128) and not eng._fp_chain_wins(252200, 8, 192, 192)  # configs B, E
    eng._fp_late_note(8, 128, 192, 192, False)
    assert not eng._fp_at_points_wanted(8, 192, 192, 8, 256, 3, 128)
    assert eng._fp_at_points_wanted(8, 192, 192, 8, 256, 3, 64)  # (another shape)
    eng._fp_late_note(8, 128, 192, 192, True)
    assert eng._fp_at_points_wanted(8, 192, 192, 8, 256, 3, 128)
    eng._fp_late_note(8, 128, 192, 192, False)
    eng.box_fp_at_points = "always"
    assert eng._fp_at_points_wanted(2, 64, 64, 1, 16, 3) and eng._fp_at_points_wanted(8, 192, 192, 8, 256, 3, 128)
    eng.box_fp_at_points = "never"
    assert not eng._fp_at_points_wanted(64, 128, 128, 8, 256, 3)
    eng.box_fp_at_points = "sometimes"
    with pytest.raises(tmr_amd.TMRError):
        eng._fp_at_points_wanted(2, 64, 64, 1, 16, 3)
    assert eng.FP_CHAIN_NS_PER_POINT > 0 and eng.FP_STORE_NS_PER_PIXEL > 0


def test_chain_symbol_is_an_extension_with_a_header():
    import os
    import re
    assert "tmr_split_conv_points_chain" not in L.SIGNATURES and L.ABI_VERSION == 3
    text = re.sub(r"/\*.*?\*/", "", open(L.POINTS_CHAIN_HEADER).read(), flags=re.S)
    m = re.search(r"int tmr_split_conv_points_chain\((.*?)\);", text, re.S)
    args = [a.strip() for a in m.group(1).split(",")]
    res, sig = L.POINTS_CHAIN_SIGNATURES["tmr_split_conv_points_chain"]
    assert len(args) == len(sig) == 28
    for a, t in zip(args, sig):
        assert ("*" in a) == (t is L._P), a
    assert os.path.basename(L.POINTS_CHAIN_HEADER) == "tmr_points_chain.h"
