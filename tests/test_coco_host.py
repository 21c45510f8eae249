"""CPU-only: the COCO matching extension's symbol table matches
include/tmr_coco.h and libtmr.so; tmr_coco_match_plan validates and picks its
variant on the host; CocoEvalGPU.accumulate on CPU tensors equals
CocoEvalMaxDets.accumulate exactly; APMeter's refinery arithmetic equals
eval_log's."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import coco_cases
import tmr_amd
from tmr_amd import _lib, coco_gpu, eval_log

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "evallog_cases.json")


def header_symbols():
    txt = open(_lib.COCO_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tmr_[a-z0-9_]+)\s*\(", txt)))


def test_extension_symbols():
    syms = header_symbols()
    assert syms == ["tmr_coco_match", "tmr_coco_match_plan"]
    assert set(syms) == set(_lib.COCO_SIGNATURES), "ctypes table out of sync with tmr_coco.h"
    assert not set(syms) & set(_lib.SIGNATURES) and not set(syms) & set(_lib.EXT_SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    L = tmr_amd.load()
    assert L.tmr_coco_match.argtypes is not None and L.tmr_version() == 3 and _lib.ABI_VERSION == 3
    assert ctypes.sizeof(_lib.CocoMatchArgs) == 144 and ctypes.sizeof(_lib.CocoMatchPlan) == 24
    txt = open(_lib.COCO_HEADER).read()
    for name, val in (("T_MAX", _lib.COCO_T_MAX), ("D_MAX", _lib.COCO_D_MAX), ("G_MAX", _lib.COCO_G_MAX)):
        assert f"#define TMR_COCO_{name} {val}\n" in txt
    assert callable(tmr_amd.CocoEvalGPU) and callable(tmr_amd.APMeter)


FAKE = 4096  # a non-NULL pointer value: the plan query dereferences nothing


def fields(**kw):
    f = dict(det_off=FAKE, det_box=FAKE, det_area=FAKE, gt_off=FAKE, gt_box=FAKE, gt_area=FAKE, gt_crowd=FAKE,
             area_rng=FAKE, iou_thr=FAKE, dt_match=FAKE, dt_ignore=FAKE, gt_ignore=FAKE, gt_match=FAKE,
             sum_d=8, sum_g=8, I=2, A=4, T=10, max_d=5, max_g=6)
    f.update(kw)
    return f


def test_plan_validation_no_gpu():
    rc = lambda **kw: _lib.coco_match_plan_rc(**fields(**kw))[0]  # noqa: E731
    assert rc() == 0
    # I = 0 is a no-op whatever the pointers
    nul = {k: None for k, v in fields().items() if v == FAKE}
    r, plan = _lib.coco_match_plan_rc(**fields(I=0, sum_d=0, sum_g=0, max_d=0, max_g=0, **nul))
    assert r == 0 and plan["blocks"] == 0 and plan["tile_cap"] > 0
    assert rc(**nul) == -1  # NULL buffers with I > 0
    assert rc(T=17) == -1 and rc(T=16) == 0 and rc(T=0) == -1 and rc(A=0) == -1
    assert rc(max_d=4096, sum_d=4096) == 0 and rc(max_d=4097, sum_d=4097) == -1
    assert rc(max_g=65536, sum_g=65536) == 0 and rc(max_g=65537, sum_g=65537) == -1
    assert rc(I=-1) == -1 and rc(sum_d=-1) == -1 and rc(sum_g=-1) == -1 and rc(max_d=-1) == -1
    assert rc(max_g=-1) == -1
    assert rc(max_d=9) == -1 and rc(sum_g=13) == -1  # maxima that contradict the sums
    L = tmr_amd.load()
    plan = _lib.CocoMatchPlan()
    plan.tile_cap = 7
    assert L.tmr_coco_match_plan(None, ctypes.byref(plan)) == -1 and plan.tile_cap == 0  # zeroed on refusal
    assert L.tmr_coco_match_plan(None, None) == -1
    # tmr_coco_match decides through the same validation, before anything touches the GPU
    args = _lib._fill(_lib.CocoMatchArgs, "tmr_coco_match_args_t", fields(T=17))
    assert L.tmr_coco_match(ctypes.byref(args), None) == -1
    assert L.tmr_coco_match(None, None) == -1
    args = _lib._fill(_lib.CocoMatchArgs, "tmr_coco_match_args_t", fields(I=0, sum_d=0, sum_g=0, max_d=0, max_g=0))
    assert L.tmr_coco_match(ctypes.byref(args), None) == 0
    with pytest.raises(tmr_amd.TMRError):
        _lib.coco_match_plan(**fields(T=17))


def test_plan_variant_switches_at_the_tile_capacity():
    cap = _lib.coco_match_plan(**fields())["tile_cap"]
    at = _lib.coco_match_plan(**fields(max_g=cap, sum_g=cap + 3))
    above = _lib.coco_match_plan(**fields(max_g=cap + 1, sum_g=cap + 3))
    assert at["variant"] == "lds" and above["variant"] == "global"
    assert at["tile_cap"] == above["tile_cap"] == cap == 4096 and at["list_cap"] == 512
    assert at["lds_bytes"] == above["lds_bytes"] == 12304 + 36 * cap <= 160 * 1024
    assert at["blocks"] == 2 * 4
    small = _lib.coco_match_plan(**fields(max_g=1024, sum_g=1024))
    big = _lib.coco_match_plan(**fields(max_g=1025, sum_g=1025))
    assert (small["threads"], big["threads"]) == (256, 1024)
    assert small["lds_bytes"] == 12304 + 36 * 1024 and small["variant"] == big["variant"] == "lds"
    empty = _lib.coco_match_plan(**fields(max_g=0, sum_g=0))
    assert empty["lds_bytes"] == 12304 and empty["variant"] == "lds"


def test_cpu_tensor_is_refused():
    gt, dets = coco_cases.make(1, n_img=2, max_d=4, max_g=4)
    ev = coco_gpu.CocoEvalGPU(gt, dets, device="cpu")
    with pytest.raises(tmr_amd.TMRError):
        ev.evaluate()


def _accumulate_both(gt, dets, max_dets):
    ev = coco_cases.numpy_eval(gt, dets, max_dets)
    cpu = coco_gpu.CocoEvalGPU(gt, dets, device="cpu")
    cpu.params.maxDets = list(ev.params.maxDets)
    cpu.load_matches(ev)
    cpu.accumulate()
    cpu.summarize()
    coco_cases.assert_tables_equal(ev, cpu)
    return ev


@pytest.mark.parametrize("max_dets", [[2, 3, 5], [900, 1000, 1100]])
def test_accumulate_on_cpu_equals_numpy(max_dets):
    minus = 0
    for seed in range(12):
        gt, dets = coco_cases.make(seed, n_img=5, max_d=12, max_g=16)
        ev = _accumulate_both(gt, dets, max_dets)
        minus += int((ev.eval["recall"] == -1).any())
    assert minus == 0  # the generator's sizes fill every area range; the -1 cells are below


def test_accumulate_edge_cells():
    # only small ground truths: medium / large keep their -1; image 2 has neither
    # ground truths nor detections; image 3 has detections only
    gt, dets = coco_cases.explicit(
        [[(0, 0, 12, 12), (24, 0, 12, 12), (0, 0, 12, 12)], [], []],
        [[((0, 0, 12, 12), .9), ((4, 0, 12, 12), .9), ((24, 0, 12, 12), .5), ((60, 60, 12, 12), .5),
          ((0, 0, 12, 12), .3), ((0, 0, 12, 12), .1)], [], [((0, 0, 12, 12), .9), ((0, 0, 60, 60), .5)]])
    for md in ([2, 3, 5], [900, 1000, 1100]):
        ev = _accumulate_both(gt, dets, md)
        assert (ev.eval["precision"][:, :, :, 2:, :] == -1).all() and (ev.eval["recall"][:, :, 0, :] > -1).all()
    # ground truths without any detection: recall 0, precision 0
    gt, dets = coco_cases.explicit([[(0, 0, 12, 12)], []], [[], []])
    ev = _accumulate_both(gt, dets, [2, 3, 5])
    assert (ev.eval["recall"][:, :, 0, :] == 0).all()
    # nothing at all
    gt, dets = coco_cases.explicit([[], []], [[], []])
    ev = _accumulate_both(gt, dets, [2, 3, 5])
    assert (ev.eval["precision"] == -1).all()


def _golden_inputs():
    g = json.load(open(GOLDEN))
    b = dict(g["batch"])
    b["img_size"] = torch.tensor(b["img_size"])
    b["orig_boxes"] = [np.array(x, np.float32) for x in b["orig_boxes"]]
    b["orig_exemplars"] = [np.array(x, np.float32) for x in b["orig_exemplars"]]
    t = lambda xs: [torch.tensor(x, dtype=torch.float32) for x in xs]  # noqa: E731
    return b, t(g["logits"]), t(g["boxes"]), t(g["refs"])


def test_accumulate_on_the_golden_eval_log_case(tmp_path, monkeypatch):
    real = os.listdir
    monkeypatch.setattr(eval_log.os, "listdir", lambda p: sorted(real(p)))
    batch, L, B, R = _golden_inputs()
    eval_log.image_info_collector(str(tmp_path), "test", batch, L, B, R)
    eval_log.coco_style_annotation_generator(str(tmp_path), "test")
    ev = eval_log.coco_evaluate(str(tmp_path), "test")
    for md in ([900, 1000, 1100], [2, 3, 5]):
        _accumulate_both(ev.gt, ev.dt, md)


def test_refinery_arithmetic_on_cpu_tensors():
    # test_refinery_edges' own values: the score-0 dummy row is kept, negatives dropped, .5 rounds to even
    lg = torch.tensor([[0.0, 0.0], [-1e-9, 0.0], [0.5, 0.0]])
    bx = torch.tensor([[0.0, 0.0, 1e-14, 1e-14], [0.1, 0.1, 0.2, 0.2], [0.25, 0.5, 0.75, 1.0]])
    rf = torch.tensor([[0.0, 0.0], [0.15, 0.15], [0.5, 0.75]])
    keep, b, p = coco_gpu.pred_refine(lg, bx, rf, [100, 10])
    assert b[keep].tolist() == [[0, 0, 0, 0], [25, 5, 50, 5]] and p[keep].tolist() == [[0, 0], [50, 8]]
    rng = np.random.default_rng(3)
    for size in ([100, 10], [512, 384], [1333, 801]):
        n = 200
        lg = torch.from_numpy(rng.standard_normal((n, 2)).astype(np.float32))
        k = torch.from_numpy(rng.integers(0, 2 * size[0], (n, 4)).astype(np.float32))
        bx = (k + 0.5) / torch.tensor([size[0], size[1], size[0], size[1]], dtype=torch.float32)  # near .5 pixels
        rf = bx[:, :2].clone()
        l0, b0, p0 = eval_log.pred_refinery(lg, bx, rf, size)
        keep, b, p = coco_gpu.pred_refine(lg, bx, rf, size)
        assert lg[keep].tolist() == l0 and b[keep].tolist() == b0 and p[keep].tolist() == p0
        ob = rng.integers(0, 4 * size[0], (n, 4)).astype(np.float32) / 4  # quarter pixels: .5 cases
        assert coco_gpu.gt_refine(ob).tolist() == eval_log.gt_refinery(ob, ob)[0]
        assert coco_gpu.gt_refine(torch.from_numpy(ob)).tolist() == eval_log.gt_refinery(ob, ob)[0]
    batch, L, B, R = _golden_inputs()
    for i in range(len(L)):
        size = batch["img_size"][i].tolist()
        l0, b0, p0 = eval_log.pred_refinery(L[i], B[i], R[i], size)
        keep, b, p = coco_gpu.pred_refine(L[i], B[i], R[i], size)
        assert L[i][keep].tolist() == l0 and b[keep].tolist() == b0 and p[keep].tolist() == p0
        assert coco_gpu.gt_refine(batch["orig_boxes"][i]).tolist() == \
            eval_log.gt_refinery(batch["orig_boxes"][i], batch["orig_exemplars"][i])[0]
