"""Shared COCO AP cases for tests/test_coco_host.py and tests/test_gpu_coco.py
(no test functions here).

Boxes are integer pixels from a small grid, with sizes chosen so that
duplicates, equal IoUs and IoUs exactly on a threshold are common:
same-size boxes shifted by w/3, w/4, w/7 overlap by exactly 1/2, 3/5, 3/4, and
a box of 9/10 the height by 9/10.  Scores come from a handful of values (ties
within and across images); sizes straddle 32^2 and 96^2, so every area range
has ignored and non-ignored ground truths.

The reference is eval_log.CocoEvalMaxDets with eval_log.bbox_iou; every
comparison is exact equality.
"""
import numpy as np

from tmr_amd import eval_log

SIZES = [(12, 12), (24, 40), (32, 32), (84, 20), (60, 60), (96, 96), (84, 120), (120, 100)]
SCORES = [0.1, 0.3, 0.5, 0.5, 0.7, 0.9]
GRID = 12


def explicit(gts_per_img, dets_per_img, crowd=None):
    """(gt dict, detection annotations) from per-image lists of (x, y, w, h)
    and ((x, y, w, h), score); crowd: set of (image, index)."""
    images = [{"id": i + 1, "height": 100, "width": 100, "file_name": f"{i}.jpg"} for i in range(len(gts_per_img))]
    anns, aid = [], 1
    for i, bs in enumerate(gts_per_img):
        for j, (x, y, w, h) in enumerate(bs):
            anns.append({"id": aid, "image_id": i + 1, "area": int(w * h),
                         "iscrowd": int(bool(crowd and (i, j) in crowd)), "bbox": [x, y, w, h], "category_id": 1})
            aid += 1
    gt = {"categories": [{"name": "fg", "id": 1}], "images": images, "annotations": anns}
    res = [{"image_id": i + 1, "category_id": 1, "bbox": list(b), "score": s}
           for i, ds in enumerate(dets_per_img) for b, s in ds]
    return gt, (eval_log.load_res(gt, res) if res else [])


def random_boxes(rng, n):
    out = []
    for _ in range(n):
        w, h = SIZES[int(rng.integers(0, len(SIZES)))]
        out.append((int(rng.integers(0, 6)) * GRID, int(rng.integers(0, 6)) * GRID, w, h))
    return out


def derived_det(rng, gts):
    """A detection derived from a ground truth: identical, or shifted / shrunk
    to an exact IoU, or elsewhere on the grid."""
    if not gts or rng.random() < 0.2:
        return random_boxes(rng, 1)[0]
    x, y, w, h = gts[int(rng.integers(0, len(gts)))]
    kind = int(rng.integers(0, 6))
    if kind == 1:
        return (x + w // 3, y, w, h)
    if kind == 2:
        return (x + w // 4, y, w, h)
    if kind == 3:
        return (x + w // 7, y, w, h)
    if kind == 4:
        return (x, y, w, h * 9 // 10)
    return (x, y, w, h)


def make(seed, n_img=4, max_d=48, max_g=96, crowd=True, exact_counts=None):
    """A seeded case.  exact_counts: [(D, G), ...] fixes each image's counts."""
    rng = np.random.default_rng(seed)
    gts, dts, crowds = [], [], set()
    n_img = len(exact_counts) if exact_counts else n_img
    for i in range(n_img):
        if exact_counts:
            nd, ng = exact_counts[i]
        elif rng.random() < 0.15:
            nd, ng = 0, 0  # an image with neither
        else:
            ng = int(rng.integers(0, max_g + 1)) if rng.random() < 0.85 else 0
            nd = int(rng.integers(0, max_d + 1)) if rng.random() < 0.85 else 0
        g = random_boxes(rng, ng)
        gts.append(g)
        if crowd:
            crowds |= {(i, j) for j in range(ng) if rng.random() < 0.12}
        dts.append([(derived_det(rng, g), SCORES[int(rng.integers(0, len(SCORES)))]) for _ in range(nd)])
    return explicit(gts, dts, crowds)


def numpy_eval(gt, dets, max_dets=None, summarize=True):
    ev = eval_log.CocoEvalMaxDets(gt, dets)
    if max_dets is not None:
        ev.params.maxDets = list(max_dets)
    ev.evaluate()
    if summarize:
        ev.accumulate()
        ev.summarize()
    return ev


def reference_properties(ev):
    """Counts on the reference's own output: (ties resolved by index, matches
    to an ignored ground truth, IoUs exactly on a threshold)."""
    p = ev.params
    ties = ign = on_thr = 0
    I0 = len(p.imgIds)
    for img in p.imgIds:
        ious = ev.ious[(img, 1)]
        if len(ious):
            on_thr += int(sum((ious == min(t, 1 - 1e-10)).sum() for t in p.iouThrs))
    for a in range(len(p.areaRng)):
        for i, img in enumerate(p.imgIds):
            e = ev.evalImgs[a * I0 + i]
            if e is None:
                continue
            ign += int(((e["dtMatches"] != 0) & (e["dtIgnore"] != 0)).sum())
            ious = ev.ious[(img, 1)]
            if not len(ious):
                continue
            g = ev._gts[(img, 1)]
            gid = {x["id"]: j for j, x in enumerate(g)}
            arng = p.areaRng[a]
            g_ign = [int(x["ignore"] or x["area"] < arng[0] or x["area"] > arng[1]) for x in g]
            gtind = np.argsort(g_ign, kind="mergesort")
            dts = ev._dts[(img, 1)]
            order = np.argsort([-d["score"] for d in dts], kind="mergesort")[:p.maxDets[-1]]
            dpos = {dts[j]["id"]: k for k, j in enumerate(order)}
            for t in range(len(p.iouThrs)):
                gtm = {int(gtind[c]): e["gtMatches"][t, c] for c in range(len(g))}
                for d in range(e["dtMatches"].shape[1]):
                    if e["dtMatches"][t, d] == 0:
                        continue
                    m = gid[int(e["dtMatches"][t, d])]
                    for j in range(len(g)):
                        free = gtm[j] == 0 or dpos[int(gtm[j])] > d
                        if j != m and g_ign[j] == g_ign[m] and ious[d, j] == ious[d, m] and free \
                                and not g[j]["iscrowd"]:
                            ties += 1
                            break
    return ties, ign, on_thr


def assert_matching_equal(ev, gpu):
    """ev: a numpy evaluator after evaluate(); gpu: a CocoEvalGPU after
    evaluate().  Per area range and image: the nonzero patterns of dtMatches and
    gtMatches, the matched ground truth itself, dtIgnore, gtIgnore, dtScores."""
    p = ev.params
    I0 = len(p.imgIds)
    for a in range(len(p.areaRng)):
        got = gpu.eval_imgs(a)
        assert len(got) == I0
        for i, img in enumerate(p.imgIds):
            e, q = ev.evalImgs[a * I0 + i], got[i]
            assert (e is None) == (q is None), (a, img)
            if e is None:
                continue
            where = f"area {a} image {img}"
            assert np.array_equal(e["dtMatches"] != 0, q["dtMatches"] != 0), where
            assert np.array_equal(e["gtMatches"] != 0, q["gtMatches"] != 0), where
            assert np.array_equal(np.asarray(e["dtIgnore"], bool), q["dtIgnore"]), where
            assert np.array_equal(np.asarray(e["gtIgnore"]), q["gtIgnore"]), where
            assert np.array_equal(np.asarray(e["dtScores"], np.float64), q["dtScores"]), where
            # the same ground truth, not only some ground truth (the largest-index rule)
            ids = np.array([0] + [x["id"] for x in ev._gts.get((img, 1), [])])
            assert np.array_equal(e["dtMatches"], ids[q["dtMatches"]]), where


def assert_tables_equal(ev, gpu):
    for k in ("precision", "recall", "scores"):
        a, b = ev.eval[k], gpu.eval[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    assert ev.eval["counts"] == gpu.eval["counts"]
    if ev.stats is not None:
        assert np.array_equal(ev.stats, gpu.stats)
