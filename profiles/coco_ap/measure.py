"""COCO AP at the scale of the reference's test split, on the MI355X.

A seeded synthetic evaluation set: --images images (default 1200), ground
truths per image drawn uniformly up to --max-gt (3700), detections up to 1100
(jittered copies of ground truths plus false positives, integer pixels).

Timed, after one warm-up each:
  gpu_end_to_end   CocoEvalGPU.evaluate + accumulate on COCO dicts (host clock
                   around a device synchronise), with its three phases:
                   pack (array passes over the dicts: group, sort, CSR arrays, upload), the
                   tmr_coco_match call, accumulate (torch, tables to the host)
  kernel           tmr_coco_match alone, device events, --reps calls
  numpy            eval_log.CocoEvalMaxDets.evaluate + accumulate (the numpy
                   path of this tree, unchanged from the parent commit) on a
                   seeded random subset of --numpy-images images, extrapolated
                   to all images by the images' sum of D x G (the matching
                   loop's work); the subset's wall time is reported as measured
Checked: on the subset the GPU's per-image match arrays and tables equal numpy's.

    python profiles/coco_ap/measure.py --out profiles/coco_ap/result.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from tmr_import import load_package  # noqa: E402

load_package()
from tmr_amd import _lib, coco_gpu, eval_log  # noqa: E402


def synth_set(seed, n_img, max_gt, max_dt, size=1536):
    rng = np.random.default_rng(seed)
    images, anns, dets = [], [], []
    aid = 1
    for i in range(n_img):
        images.append({"id": i + 1, "height": size, "width": size, "file_name": f"{i}.jpg"})
        ng = int(rng.integers(1, max_gt + 1))
        side = rng.choice([6, 10, 16, 24, 40, 70, 110], size=ng, p=[.2, .25, .25, .15, .08, .05, .02])
        w = np.maximum(2, side + rng.integers(-2, 3, ng))
        h = np.maximum(2, side + rng.integers(-2, 3, ng))
        x = rng.integers(0, size - w)
        y = rng.integers(0, size - h)
        for j in range(ng):
            anns.append({"id": aid, "image_id": i + 1, "area": int(w[j] * h[j]), "iscrowd": 0,
                         "bbox": [int(x[j]), int(y[j]), int(w[j]), int(h[j])], "category_id": 1})
            aid += 1
        nd = int(min(max_dt + 50, max(1, ng * rng.uniform(0.3, 1.2))))
        src = rng.integers(0, ng, nd)
        fp = rng.random(nd) < 0.15
        dx, dy = rng.integers(-3, 4, nd), rng.integers(-3, 4, nd)
        sc = np.round(rng.random(nd), 3)
        for k in range(nd):
            j = src[k]
            if fp[k]:
                bb = [int(rng.integers(0, size - 20)), int(rng.integers(0, size - 20)), 16, 16]
            else:
                bb = [int(x[j] + dx[k]), int(y[j] + dy[k]), int(w[j]), int(h[j])]
            dets.append({"image_id": i + 1, "category_id": 1, "bbox": bb, "score": float(sc[k])})
    gt = {"categories": [{"name": "fg", "id": 1}], "images": images, "annotations": anns}
    return gt, eval_log.load_res(gt, dets)


def subset(gt, dets, ids):
    ids = set(ids)
    g = {"categories": gt["categories"], "images": [im for im in gt["images"] if im["id"] in ids],
         "annotations": [a for a in gt["annotations"] if a["image_id"] in ids]}
    return g, [d for d in dets if d["image_id"] in ids]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1200)
    ap.add_argument("--max-gt", type=int, default=3700)
    ap.add_argument("--max-dt", type=int, default=1100)
    ap.add_argument("--numpy-images", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    t0 = time.time()
    gt, dets = synth_set(a.seed, a.images, a.max_gt, a.max_dt)
    res = {"images": a.images, "ground_truths": len(gt["annotations"]), "detections": len(dets),
           "device": torch.cuda.get_device_name(0), "synth_s": round(time.time() - t0, 2)}
    print(json.dumps(res), flush=True)

    def sync():
        torch.cuda.synchronize(dev)

    # ---- GPU end to end, phases on a host clock that ends in a synchronise
    runs = []
    for rep in range(3):
        ev = coco_gpu.CocoEvalGPU(gt, dets, device=dev)
        sync()
        t0 = time.perf_counter()
        p = ev._normalise_params()
        ev._packs = ev._pack_all()
        sync()
        t1 = time.perf_counter()
        ev._matches = [coco_gpu.coco_match(pk, p.areaRng, p.iouThrs, dev) for pk in ev._packs]
        sync()
        t2 = time.perf_counter()
        ev.accumulate()
        sync()
        t3 = time.perf_counter()
        runs.append({"pack_s": t1 - t0, "match_s": t2 - t1, "accumulate_s": t3 - t2, "total_s": t3 - t0})
        print("gpu run", rep, json.dumps(runs[-1]), flush=True)
    ev.summarize()
    res["gpu_end_to_end_runs"] = runs[1:]  # the first run warms up (code objects, allocator)
    res["gpu_end_to_end_s"] = float(np.median([r["total_s"] for r in runs[1:]]))
    res["gpu_stats"] = [float(x) for x in ev.stats]
    pk = ev._packs[0]
    res["max_d"], res["max_g"], res["sum_d_after_cut"] = pk.max_d, pk.max_g, pk.sum_d
    res["plan"] = coco_gpu.match_plan(pk, len(p.areaRng), len(p.iouThrs))

    # ---- the kernel alone, device events
    times = []
    for rep in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ar = torch.as_tensor(np.asarray(p.areaRng, np.float64)).to(dev)
        th = torch.as_tensor(np.asarray(p.iouThrs, np.float64)).to(dev)
        out = ev._matches[0]
        do, go = torch.from_numpy(pk.det_off).to(dev), torch.from_numpy(pk.gt_off).to(dev)
        sync()
        e0.record()
        _lib.coco_match(_lib.stream(dev), det_off=_lib.ptr(do), det_box=_lib.ptr(pk.det_box),
                        det_area=_lib.ptr(pk.det_area), gt_off=_lib.ptr(go), gt_box=_lib.ptr(pk.gt_box),
                        gt_area=_lib.ptr(pk.gt_area), gt_crowd=_lib.ptr(pk.gt_crowd), area_rng=_lib.ptr(ar),
                        iou_thr=_lib.ptr(th), dt_match=_lib.ptr(out["dt_match"]),
                        dt_ignore=_lib.ptr(out["dt_ignore"]), gt_ignore=_lib.ptr(out["gt_ignore"]),
                        gt_match=_lib.ptr(out["gt_match"]), sum_d=pk.sum_d, sum_g=pk.sum_g, I=pk.n_img,
                        A=len(p.areaRng), T=len(p.iouThrs), max_d=pk.max_d, max_g=pk.max_g)
        e1.record()
        sync()
        times.append(e0.elapsed_time(e1))
    res["kernel_ms"] = times[1:]
    res["kernel_ms_median"] = float(np.median(times[1:]))
    nd, ng = np.diff(pk.det_off), np.diff(pk.gt_off)
    pairs = float((nd * ng).sum()) * len(p.areaRng)
    res["iou_pairs_per_call"] = pairs
    res["iou_pairs_per_s"] = pairs / (res["kernel_ms_median"] * 1e-3)
    print("kernel", json.dumps({"ms": times}), flush=True)

    # ---- numpy on a seeded subset, and the equality check there
    rng = np.random.default_rng(a.seed + 1)
    ids = sorted(int(i) + 1 for i in rng.choice(a.images, size=min(a.numpy_images, a.images), replace=False))
    g2, d2 = subset(gt, dets, ids)
    ref = eval_log.CocoEvalMaxDets(g2, d2)
    t0 = time.perf_counter()
    ref.evaluate()
    t1 = time.perf_counter()
    ref.accumulate()
    t2 = time.perf_counter()
    ref.summarize()
    work = {i + 1: float(nd[i] * ng[i]) for i in range(a.images)}
    share = sum(work[i] for i in ids) / sum(work.values())
    res["numpy"] = {"image_ids": ids, "evaluate_s": t1 - t0, "accumulate_s": t2 - t1,
                    "subset_share_of_DxG": share, "extrapolated_evaluate_s": (t1 - t0) / share,
                    "threads": os.environ.get("OMP_NUM_THREADS")}
    print("numpy", json.dumps(res["numpy"]), flush=True)
    sub = coco_gpu.CocoEvalGPU(g2, d2, device=dev)
    sub.evaluate()
    sub.accumulate()
    sub.summarize()
    I0 = len(ids)
    same = True
    for ai in range(len(p.areaRng)):
        got = sub.eval_imgs(ai)
        for i in range(I0):
            e, q = ref.evalImgs[ai * I0 + i], got[i]
            same &= np.array_equal(e["dtMatches"] != 0, q["dtMatches"] != 0)
            same &= np.array_equal(e["gtMatches"] != 0, q["gtMatches"] != 0)
            same &= np.array_equal(np.asarray(e["dtIgnore"], bool), q["dtIgnore"])
            same &= np.array_equal(np.asarray(e["gtIgnore"]), q["gtIgnore"])
    for k in ("precision", "recall", "scores"):
        same &= np.array_equal(ref.eval[k], sub.eval[k])
    same &= np.array_equal(ref.stats, sub.stats)
    res["subset_equal_to_numpy"] = bool(same)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not same:
        raise SystemExit("the GPU results differ from numpy on the subset")


if __name__ == "__main__":
    main()
