"""CPU-only: the evaluation-loss restatement (tests/evalloss_ref.py) against
the reference's own GT_map / SetCriterion_TM fixtures, the host descriptors
and every argument check of tmr_gt_loss (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import evalloss_ref as er
import oracle
import tmr_amd
from tmr_amd import gt_loss  # noqa: F401  (the feature's module: absent without it)
from tmr_amd import _lib, host


@pytest.fixture(scope="module")
def cases(golden):
    return er.load_cases(golden("evalloss"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixture_covers_the_cases(cases):
    assert 30 <= len(cases) <= 48
    assert {(c["pt"], c["nt"]) for c in cases} >= {(p, n) for p in (0.7, 0.5, 1.0) for n in (0.7, 0.5, 1.0)}
    assert any(len(c["levels"]) == 2 for c in cases) and any(c["focal"] for c in cases)
    assert all(any(c[k] for c in cases) for k in "abc")
    assert any(c["B"] == 3 and len({len(b) for b in c["boxes"]}) == 3 for c in cases)
    assert any((c["exemplars"] < 0).any() or (c["exemplars"] > 1).any() for c in cases)
    # a unit without a positive pixel: its dummy pair is among the rows
    assert any((_bits(c["lv"][-1]["pred_reg"]) == _bits(er.DUMMY)).all(1).any() for c in cases)


def test_restatement_matches_reference_fixtures(cases):
    """gt_map, GT rows, sample values and order, labels and the prediction
    rows (xy, and wh through the recorded reference exp) bit for bit; the
    float64 losses within 1e-5 relative of the reference's fp32 values."""
    for c in cases:
        tot_ce = tot_gi = 0.0
        for lv in range(len(c["levels"])):
            L = c["lv"][lv]
            units = er.case_level(c, lv, oracle.expf)
            tag = f"case {c['index']} level {lv}"
            assert np.array_equal(_bits(np.stack([u["gt_map"] for u in units])[:, None]), _bits(L["gt_map"])), tag
            for name, key in (("samples", "pred_obj"), ("labels", "gt_obj"), ("gt", "gt_reg"), ("pred", "pred_reg")):
                got = np.concatenate([u[name] for u in units])
                assert got.shape == L[key].shape, (tag, name)
                if name == "pred":
                    assert np.array_equal(_bits(got[:, :2]), _bits(L[key][:, :2])), (tag, "pred xy")
                assert np.array_equal(_bits(got), _bits(L[key])), (tag, name)
            ce, gi = er.losses(units, c["focal"])
            tot_ce += ce / len(c["levels"])
            tot_gi += gi / len(c["levels"])
        assert abs(tot_ce - c["loss"][0]) <= 1e-5 * abs(c["loss"][0]), (c["index"], tot_ce, c["loss"])
        assert abs(tot_gi - c["loss"][1]) <= 1e-5 * abs(c["loss"][1]), (c["index"], tot_gi, c["loss"])


def test_gt_units_pads_and_scales(cases):
    for c in cases:
        sw, sh = er.case_scales(c)
        for lv, (H, W) in enumerate(c["levels"]):
            u = host.gt_units(c["exemplars"], np.arange(c["B"]), H, W, not c["a"], c["b"], c["c"])
            assert u.dtype.itemsize == 32
            assert np.array_equal(np.stack([u["pad_x"], u["pad_y"]], 1), c["pads"][lv]), c["index"]
            assert np.array_equal(u["mode"], np.full(c["B"], er.case_mode(c)))
            assert np.array_equal(_bits(u["scale_w"]), _bits(sw)) and np.array_equal(_bits(u["scale_h"]), _bits(sh))
            assert np.array_equal(u["image"], np.arange(c["B"]))
    with pytest.raises(ValueError):  # snaps to an empty pixel range
        host.gt_units(np.array([[0.5, 0.5, 0.5, 0.5]], np.float32), [0], 16, 16)
    with pytest.raises(ValueError):
        host.gt_box_table([np.array([[0.1, 0.1, np.inf, 0.2]], np.float32)])
    boxes, off, mn = host.gt_box_table([np.zeros((2, 4)), np.zeros((0, 4)), np.ones((3, 4))])
    assert boxes.shape == (5, 4) and off.tolist() == [0, 2, 2, 5] and mn == 0


def test_symbol_bound_and_struct_layout():
    L = tmr_amd.load()
    assert "tmr_gt_loss" in _lib.SIGNATURES and hasattr(L, "tmr_gt_loss")
    assert ctypes.sizeof(_lib.GtLossArgs) == 17 * 8 + 2 * 8 + 2 * 8 + 10 * 4
    assert _lib.GT_UNIT_DTYPE.itemsize == 32
    for name in ("GT_map", "SetCriterion_TM", "build_criterion", "gIoU_loss", "WeightedFocalLoss"):
        assert hasattr(tmr_amd, name) and name in tmr_amd.__all__
    assert hasattr(tmr_amd.TMREngine, "eval_loss")
    with pytest.raises(_lib.TMRError):  # unknown struct field names are refused, not dropped
        _lib.gt_loss_args(phase=1, gtmap=3)
    assert _lib.gt_loss_args(phase=3, U=2).phase == 3


def _size(*d):
    return int(tmr_amd.load().tmr_size(_lib.SIZE_KINDS["gt_work"], *(list(d) + [0] * (6 - len(d)))))


def test_size_query():
    base = _size(1, 1, 1, 1, 1)
    assert base >= _lib.GT_SLICES * 4 * 8
    # 32-B box records + one word per image pixel + the slice partials per unit
    n = _size(3000, 64, 128, 128, 192)
    need = 3000 * 32 + 64 * 128 * 128 * 4 + 192 * _lib.GT_SLICES * 32
    assert need <= n <= need + 3 * 256
    assert _size(0, 1, 8, 8, 1) == -1 and _size(1, 0, 8, 8, 1) == -1 and _size(1, 1, 8, 8, 0) == -1
    assert _size(1, 1, 1 << 16, 1 << 16, 1) == -1  # H*W past int32


def test_invalid_arguments_without_a_gpu():
    L = tmr_amd.load()
    buf = np.zeros(64, np.float64)
    a = buf.ctypes.data  # never dereferenced: every case is refused before any HIP call
    ok = dict(o=a, reg=a, boxes=a, box_off=a, units=a, work=a, gt_map=a, target=a, counts=a, sums=a,
              samp_off=a, row_off=a, obj_out=a, label_out=a, rows_pred=a, rows_gt=a,
              positive_threshold=0.7, negative_threshold=0.5, U=1, NI=1, H=8, W=8, G_total=2, min_boxes=2)

    def rc(**kw):
        f = dict(ok)
        f.update(kw)
        return L.tmr_gt_loss(ctypes.byref(_lib.gt_loss_args(**f)), None)

    assert L.tmr_gt_loss(None, None) == -1
    for phase in (0, 16, 32, _lib.GT_ROWS | _lib.GT_ASSIGN, _lib.GT_LOSS, _lib.GT_LOSS | _lib.GT_GATHER, -1):
        assert rc(phase=phase) == -1, phase
    A = _lib.GT_ASSIGN
    assert rc(phase=A, G_total=0) == -1 and rc(phase=A, min_boxes=0) == -1  # G = 0
    assert rc(phase=_lib.GT_GATHER, min_boxes=0) == -1
    for name in ("boxes", "box_off", "units", "work", "gt_map", "target", "counts"):
        assert rc(phase=A, **{name: None}) == -1, name
    for name in ("o", "sums"):
        assert rc(phase=A | _lib.GT_LOSS, **{name: None}) == -1, name
    for name in ("o", "samp_off", "row_off", "obj_out", "label_out", "rows_pred", "rows_gt"):
        assert rc(phase=_lib.GT_GATHER, **{name: None}) == -1, name
    assert rc(phase=A, H=1 << 16, W=1 << 16) == -1  # H*W past int32
    assert rc(phase=A, U=0) == -1 and rc(phase=A, NI=0) == -1 and rc(phase=A, H=0) == -1
    assert rc(phase=A, positive_threshold=float("nan")) == -1
    R = _lib.GT_ROWS
    assert rc(phase=R, sums=None) == -1 and rc(phase=R, work=None) == -1
    assert rc(phase=R, n_samples=4, n_rows=0, obj_out=None) == -1
    assert rc(phase=R, n_samples=0, n_rows=2, rows_gt=None) == -1
    assert rc(phase=R, n_samples=-1) == -1
