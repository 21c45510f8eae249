"""tmr_coco_match, CocoEvalGPU and APMeter on the GPU against
eval_log.CocoEvalMaxDets / eval_log.bbox_iou (tests/coco_cases.py).  Every
comparison is exact equality: the matching is integer bookkeeping over single
IEEE fp64 operations, the tables are integer counts and one division each.

The shapes are small and chosen for where the kernel can go wrong: the lane,
wave and block boundaries of the ground-truth loop (63 / 64 / 65, 257), the
switch from 256 to 1024 threads (1025), the tile capacity (cap + 1: the global
variant), the candidate list's capacity (more than 512 candidates for one
detection: the serial rescan, in both variants), and empty images.
"""
import json
import os

import numpy as np
import pytest
import torch

import coco_cases
import guarded_alloc as ga
import oracle
import tmr_amd
from tmr_amd import coco_gpu, eval_log, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "evallog_cases.json")
CAP = 4096  # the LDS tile capacity tmr_coco_match_plan reports (asserted below)


def gpu_eval(gt, dets, max_dets=None, tables=True):
    ev = coco_gpu.CocoEvalGPU(gt, dets, device=DEV)
    if max_dets is not None:
        ev.params.maxDets = list(max_dets)
    ev.evaluate()
    if tables:
        ev.accumulate()
        ev.summarize()
    return ev


def check_matching(gt, dets, variant, threads):
    """One kernel call for all A x T; the plan names the variant that serves it."""
    ref = coco_cases.numpy_eval(gt, dets, summarize=False)
    got = gpu_eval(gt, dets, tables=False)
    plan = coco_gpu.match_plan(got._packs[0], len(ref.params.areaRng), len(ref.params.iouThrs))
    assert plan["tile_cap"] == CAP and plan["list_cap"] == 512
    assert (plan["variant"], plan["threads"]) == (variant, threads)
    coco_cases.assert_matching_equal(ref, got)
    return ref, got


# ------------------------------------------------------------------ matching
SHAPES = [(1, 1), (5, 0), (0, 5), (3, 63), (3, 64), (3, 65), (7, 257), (40, 1025)]


@pytest.mark.parametrize("D,G", SHAPES)
def test_matching_shapes(D, G):
    gt, dets = coco_cases.make(100 + D + G, exact_counts=[(D, G)])
    check_matching(gt, dets, "lds", 256 if G <= 1024 else 1024)


def test_matching_many_images_one_call():
    gt, dets = coco_cases.make(7, exact_counts=SHAPES[:4] + [(0, 0)] + SHAPES[4:])
    check_matching(gt, dets, "lds", 1024)


def test_matching_global_variant_above_the_tile():
    gt, dets = coco_cases.make(8, exact_counts=[(8, CAP + 1)])
    ref, _ = check_matching(gt, dets, "global", 1024)
    assert (ref.evalImgs[0]["dtMatches"] != 0).any()
    # mixed with images the LDS variant serves in the same launch
    gt, dets = coco_cases.make(9, exact_counts=[(5, 40), (8, CAP + 1), (0, 0), (6, 3)])
    check_matching(gt, dets, "global", 1024)


def test_matching_all_equal_boxes():
    """Every IoU is 1 and every choice a tie: the largest index decides."""
    box = (12, 12, 24, 40)
    gt, dets = coco_cases.explicit([[box] * 6], [[(box, s) for s in (.9, .9, .7, .5, .5, .3, .1, .1)]])
    ref, got = check_matching(gt, dets, "lds", 256)
    assert got.eval_imgs(0)[0]["dtMatches"][0].tolist() == [6, 5, 4, 3, 2, 1, 0, 0]


@pytest.mark.parametrize("G,variant,threads", [(600, "lds", 256), (CAP + 1, "global", 1024)])
def test_matching_more_candidates_than_the_list_holds(G, variant, threads):
    """More than list_cap ground truths reach the lowest threshold for one
    detection: the scan falls back to every ground truth, serially."""
    box, other = (0, 0, 60, 60), (20, 0, 60, 60)  # IoU 1/2 with each other
    gts = [box if j % 3 else other for j in range(G)]
    gt, dets = coco_cases.explicit([gts], [[(box, .9), (other, .9), (box, .5), ((0, 0, 12, 12), .3)]],
                                   crowd={(0, 5), (0, G - 1)})
    assert G > 512
    check_matching(gt, dets, variant, threads)


def test_matching_only_ignored_candidates():
    """The only candidate >= thr is an ignored ground truth (out of the area
    range): the detection matches it and is ignored itself."""
    gt, dets = coco_cases.explicit([[(0, 0, 120, 100)]], [[((0, 0, 120, 100), .9)]])
    ref, got = check_matching(gt, dets, "lds", 256)
    small = ref.evalImgs[1 * 1 + 0]  # area range 'small'
    assert small["gtIgnore"].tolist() == [1] and (small["dtMatches"] != 0).all() and small["dtIgnore"].all()
    q = got.eval_imgs(1)[0]
    assert (q["dtMatches"] == 1).all() and q["dtIgnore"].all()


def test_matching_non_ignored_beats_a_better_ignored_one():
    """An ignored (crowd) ground truth with IoU 1 and a non-ignored one with
    IoU 1/2: the non-ignored one is taken where it reaches the threshold."""
    gt, dets = coco_cases.explicit([[(0, 0, 60, 60), (20, 0, 60, 60)]], [[((0, 0, 60, 60), .9)]], crowd={(0, 0)})
    ref, got = check_matching(gt, dets, "lds", 256)
    dtm = got.eval_imgs(0)[0]["dtMatches"][:, 0]
    assert dtm[0] == 2 and (dtm[1:] == 1).all()  # t = .5: index 1 (non-ignored); above: the crowd
    assert ref.evalImgs[0]["dtMatches"][0, 0] == 2


def test_matching_crowd_takes_several_detections():
    gt, dets = coco_cases.explicit([[(0, 0, 120, 100), (0, 0, 12, 12)]],
                                   [[((0, 0, 12, 12), .9), ((12, 12, 24, 40), .7), ((36, 0, 12, 12), .5),
                                     ((60, 60, 24, 40), .3)]], crowd={(0, 0)})
    ref, got = check_matching(gt, dets, "lds", 256)
    q = got.eval_imgs(0)[0]
    assert (q["dtMatches"][0] == 1).sum() == 3 and q["dtIgnore"][0].sum() == 3


def test_matching_area_above_2_to_32():
    big = (0, 0, 70000, 70000)  # area 4.9e9: above 2^32, inside the 1e10 bound
    gt, dets = coco_cases.explicit([[big, (0, 0, 70000, 35000)]], [[(big, .9), ((0, 0, 70000, 35000), .5)]])
    assert 2 ** 32 < gt["annotations"][0]["area"] < 1e10
    ref, got = check_matching(gt, dets, "lds", 256)
    q = got.eval_imgs(3)[0]  # 'large'
    assert q["dtMatches"][0].tolist() == [1, 2] and not q["dtIgnore"].any() and not q["gtIgnore"].any()


# --------------------------------------------------------------------- sweep
SWEEP_SEEDS = range(40)


@pytest.fixture(scope="module")
def sweep():
    """The seeded sweep (I <= 6, D <= 48, G <= 96) and the reference's results,
    computed once."""
    out = []
    for seed in SWEEP_SEEDS:
        gt, dets = coco_cases.make(seed, n_img=seed % 6 + 1, max_d=48, max_g=96)
        out.append((gt, dets, coco_cases.numpy_eval(gt, dets)))
    return out


def test_sweep_reference_has_the_hard_cases(sweep):
    props = np.array([coco_cases.reference_properties(ev) for _, _, ev in sweep])
    ties, ign, on_thr = (props > 0).sum(0)
    assert ties >= 1 and ign >= 1 and on_thr >= 1, (ties, ign, on_thr)


def test_sweep_matching(sweep):
    for gt, dets, ref in sweep:
        got = gpu_eval(gt, dets, tables=False)
        coco_cases.assert_matching_equal(ref, got)


@pytest.mark.parametrize("max_dets", [[2, 3, 5], [900, 1000, 1100]])
def test_sweep_end_to_end(sweep, max_dets):
    for gt, dets, ref in sweep:
        if max_dets != ref.params.maxDets:
            ref = coco_cases.numpy_eval(gt, dets, max_dets)
        got = gpu_eval(gt, dets, max_dets)
        coco_cases.assert_matching_equal(ref, got)
        coco_cases.assert_tables_equal(ref, got)


# ---------------------------------------------------------------- end to end
def test_end_to_end_cut_at_the_largest_max_dets():
    gt, dets = coco_cases.make(11, exact_counts=[(6, 9), (6, 2), (3, 4)])
    ref = coco_cases.numpy_eval(gt, dets, [2, 3, 5])
    got = gpu_eval(gt, dets, [2, 3, 5])
    assert got._packs[0].max_d == 5
    coco_cases.assert_matching_equal(ref, got)
    coco_cases.assert_tables_equal(ref, got)


def test_end_to_end_scores_tied_across_images():
    a, b, c = (0, 0, 24, 40), (36, 0, 24, 40), (0, 48, 24, 40)
    gt, dets = coco_cases.explicit([[a, b], [a, c], [b]],
                                   [[(a, .5), (c, .5), (b, .5)], [(c, .5), (b, .5), (a, .5)], [(a, .5), (b, .5)]])
    ref = coco_cases.numpy_eval(gt, dets)
    got = gpu_eval(gt, dets)
    coco_cases.assert_tables_equal(ref, got)
    assert 0 < ref.stats[0] < 1  # the order among the ties decides the curve


def test_end_to_end_real_slicing():
    """1101, 950 and 10 detections against maxDets [900, 1000, 1100]."""
    gt, dets = coco_cases.make(12, exact_counts=[(1101, 120), (950, 120), (10, 120)])
    ref = coco_cases.numpy_eval(gt, dets)
    got = gpu_eval(gt, dets)
    assert got._packs[0].max_d == 1100
    coco_cases.assert_matching_equal(ref, got)
    coco_cases.assert_tables_equal(ref, got)


def _golden_inputs():
    g = json.load(open(GOLDEN))
    b = dict(g["batch"])
    b["img_size"] = torch.tensor(b["img_size"])
    b["orig_boxes"] = [np.array(x, np.float32) for x in b["orig_boxes"]]
    b["orig_exemplars"] = [np.array(x, np.float32) for x in b["orig_exemplars"]]
    t = lambda xs: [torch.tensor(x, dtype=torch.float32) for x in xs]  # noqa: E731
    return b, t(g["logits"]), t(g["boxes"]), t(g["refs"])


def test_get_ap_scores_device_route(tmp_path, monkeypatch):
    real = os.listdir
    monkeypatch.setattr(eval_log.os, "listdir", lambda p: sorted(real(p)))
    batch, L, B, R = _golden_inputs()
    eval_log.image_info_collector(str(tmp_path), "test", batch, L, B, R)
    eval_log.coco_style_annotation_generator(str(tmp_path), "test")
    assert eval_log.Get_AP_scores(str(tmp_path), "test", device=DEV) == eval_log.Get_AP_scores(str(tmp_path), "test")
    ref, got = eval_log.coco_evaluate(str(tmp_path), "test"), eval_log.coco_evaluate(str(tmp_path), "test", DEV)
    assert isinstance(got, coco_gpu.CocoEvalGPU)
    coco_cases.assert_tables_equal(ref, got)
    # the in-memory meter over the same batch
    meter = tmr_amd.APMeter(DEV)
    meter.update(batch, [x.to(DEV) for x in L], [x.to(DEV) for x in B], [x.to(DEV) for x in R])
    out = meter.compute()
    assert out[:3] == eval_log.Get_AP_scores(str(tmp_path), "test")
    mae, rmse = eval_log.Get_MAE_RMSE(str(tmp_path), "test")
    assert out[3] == mae and out[4] == rmse and np.array_equal(meter.stats, ref.stats)


# ------------------------------------------------------------------- APMeter
@pytest.fixture(scope="module")
def detections():
    """Kept detections of a small detect() run: 3 images, one exemplar each, at
    a threshold between the two weakest images' best peaks, so that one image
    has no candidate and carries the dummy row."""
    P = oracle.reference_weights(0, cin=32, emb=32)
    P["objectness_head.head.0.bias"] = torch.tensor([0.4])
    feats = torch.from_numpy(synth.sam_features(21, 3, 32, 12, 12)).to(DEV)
    ex, _ = synth.exemplar_set(22, 3, 1, 24, 24, 3, 7)
    eng = tmr_amd.TMREngine({k: v.to(DEV) for k, v in P.items()}, tmr_amd.PathConfig(emb_dim=32))
    r = eng.forward_units(feats, np.arange(3), ex.reshape(-1, 4))
    top = np.sort(torch.sigmoid(r["o"].double()).amax(dim=(1, 2, 3)).cpu().numpy())
    thr = float(top[0] + top[1]) / 2
    assert top[0] < thr < top[1]
    L, Bx, R = eng.detect(feats, ex, cls_ths=thr, iou_threshold=0.5)
    size = [512, 384]
    s4 = np.array(size * 2, np.float32)
    # ground truths: the image's first detections, some moved by a few pixels; one image has none
    gts = []
    for b in range(3):
        bx = Bx[b].cpu().numpy()[:4] * s4
        bx[1::2] += 3.0
        gts.append(bx.astype(np.float32) if b != 1 else np.zeros((0, 4), np.float32))
    batch = {"img_name": [f"i{b}.jpg" for b in range(3)], "img_url": [""] * 3, "img_id": [30, 10, 20],
             "img_size": torch.tensor([size] * 3), "orig_boxes": gts,
             "orig_exemplars": [np.array([[0, 0, 10, 10]], np.float32)] * 3}
    return batch, L, Bx, R


def _file_path_numbers(tmp_path, batch, L, Bx, R):
    d = str(tmp_path)
    eval_log.image_info_collector(d, "t", batch, L, Bx, R)
    eval_log.coco_style_annotation_generator(d, "t")
    mae, rmse = eval_log.Get_MAE_RMSE(d, "t")
    return eval_log.Get_AP_scores(d, "t") + (mae, rmse), eval_log.coco_evaluate(d, "t").stats


def test_ap_meter_equals_the_file_path(detections, tmp_path):
    batch, L, Bx, R = detections
    # the dummy row of an image without candidates: score 0, box (0, 0, 1e-14, 1e-14)
    dummy = [b for b in range(3) if L[b].shape[0] == 1 and float(L[b][0, 0]) == 0.0 and float(Bx[b].max()) < 1e-10]
    assert dummy and sum(int(x.shape[0]) for x in L) > 3
    want, stats = _file_path_numbers(tmp_path, batch, L, Bx, R)
    meter = tmr_amd.APMeter(DEV)
    for b in range(3):  # one image per update, as a loader with batch size 1
        one = {k: v[b:b + 1] for k, v in batch.items()}
        meter.update(one, L[b:b + 1], Bx[b:b + 1], R[b:b + 1])
    got = meter.compute()
    assert got == want
    assert np.array_equal(meter.stats, stats) and want[0] > 0


# --------------------------------------------------------- guarded allocator
POISONS = [pytest.param(ga.POISON_ZERO, id="zero"), pytest.param(ga.POISON_FF, id="ff")]


@pytest.mark.parametrize("poison", POISONS)
def test_guarded_matching(poison):
    """The four outputs come from torch.empty: poisoned and guard-banded here.
    Every element is written (no poison value survives) and nothing outside."""
    gt, dets = coco_cases.make(13, exact_counts=[(9, 70), (0, 0), (5, 0), (0, 6), (12, 300)])
    ref = coco_cases.numpy_eval(gt, dets, summarize=False)
    with ga.GuardedAlloc(poison, DEV) as a:
        got = gpu_eval(gt, dets, tables=False)
        m = got._matches[0]
        assert len(a.records) >= 4
        a.check()
        if poison == ga.POISON_FF:
            assert int((m["dt_match"] < 0).sum()) == 0 and int((m["gt_match"] < 0).sum()) == 0
            assert int((m["dt_ignore"] > 1).sum()) == 0 and int((m["gt_ignore"] > 1).sum()) == 0
        coco_cases.assert_matching_equal(ref, got)


@pytest.mark.parametrize("poison", POISONS)
def test_guarded_ap_meter(poison, detections, tmp_path):
    batch, L, Bx, R = detections
    want, stats = _file_path_numbers(tmp_path, batch, L, Bx, R)
    with ga.GuardedAlloc(poison, DEV) as a:
        meter = tmr_amd.APMeter(DEV)
        meter.update(batch, L, Bx, R)
        got = meter.compute()
        m = meter.evaluator._matches[0]
        assert len(a.records) >= 4
        a.check()
        assert int((m["dt_match"] < 0).sum()) == 0 and int((m["dt_ignore"] > 1).sum()) == 0
        assert int((m["gt_match"] < 0).sum()) == 0 and int((m["gt_ignore"] > 1).sum()) == 0
    assert got == want and np.array_equal(meter.stats, stats)
    assert not np.isnan(meter.stats).any()
