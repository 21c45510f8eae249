"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/evalloss.npz from the
reference's own GT_map.Get_pred_gts (utils/TM_utils.py) and SetCriterion_TM
(criterion/criterions_TM.py), run on seeded small inputs.  Nothing of the
reference is copied into the repository; only data is written.

It runs only where the reference checkout exists (see oracle/make_golden.py,
whose import_reference it uses).  torchvision is absent there, so
``torchvision.ops.generalized_box_iou_loss`` is the stub below, transcribed
from torchvision's ops/giou_loss.py and ops/_utils.py: the GIoU fixtures
therefore cross-check the kernel and tests/evalloss_ref.py but stay UNPINNED
against real torchvision (like py_nms in oracle/make_golden.py).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_evalloss.py
"""
from __future__ import annotations

import json
import math
import os
import sys
from types import SimpleNamespace

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import make_golden  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "evalloss.npz")


def generalized_box_iou_loss(boxes1, boxes2, reduction="none", eps=1e-7):
    """Transcription of torchvision.ops.generalized_box_iou_loss (xyxy rows)."""
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    xkis1, ykis1 = torch.max(x1, x1g), torch.max(y1, y1g)
    xkis2, ykis2 = torch.min(x2, x2g), torch.min(y2, y2g)
    intsctk = torch.zeros_like(x1)
    mask = (ykis2 > ykis1) & (xkis2 > xkis1)
    intsctk[mask] = (xkis2[mask] - xkis1[mask]) * (ykis2[mask] - ykis1[mask])
    unionk = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - intsctk
    iouk = intsctk / (unionk + eps)
    xc1, yc1 = torch.min(x1, x1g), torch.min(y1, y1g)
    xc2, yc2 = torch.max(x2, x2g), torch.max(y2, y2g)
    area_c = (xc2 - xc1) * (yc2 - yc1)
    miouk = iouk - ((area_c - unionk) / (area_c + eps))
    loss = 1 - miouk
    if reduction == "mean":
        loss = loss.mean() if loss.numel() > 0 else 0.0 * loss.sum()
    elif reduction == "sum":
        loss = loss.sum()
    return loss


def import_reference():
    R = make_golden.import_reference()
    sys.modules["torchvision.ops"].generalized_box_iou_loss = generalized_box_iou_loss
    make_golden._pkg("criterion", make_golden.REF + "/criterion")
    R.crit = make_golden._load("criterion.criterions_TM", make_golden.REF + "/criterion/criterions_TM.py")
    return R


def rand_boxes(rng, n, lo=0.08, hi=0.45):
    c = rng.uniform(0.1, 0.9, (n, 2))
    s = rng.uniform(lo, hi, (n, 2))
    return np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)


def special_boxes(kind, rng, H, W):
    b = rand_boxes(rng, 4)
    if kind == "zero_width":
        b[1, 2] = b[1, 0]
        b[3, 3] = b[3, 1]
    elif kind == "duplicated":
        b[2] = b[0]
        b = np.concatenate([b, b[1:2]])
    elif kind == "grid_aligned":
        g = np.array([[2, 2, 6, 7], [1, 3, 5, 5], [4, 0, 8, 4], [3, 3, 4, 4]], np.float32)
        b = (g / np.array([W, H, W, H], np.float32)).astype(np.float32)
    return b


def cases():
    out = []
    ths = (0.7, 0.5, 1.0)
    seed = 0

    def add(**kw):
        nonlocal seed
        seed += 1
        d = dict(seed=seed, levels=[(16, 16)], G=[3], pt=0.7, nt=0.7, a=False, b=False, c=False, focal=False,
                 boxes=None, exemplars=None)
        d.update(kw)
        out.append(d)

    for pt in ths:
        for nt in ths:
            add(pt=pt, nt=nt, G=[4])
    for pt in ths:
        for nt in ths:
            add(pt=pt, nt=nt, levels=[(12, 20), (8, 8)], G=[2, 5], focal=(pt == nt))
    for abl in ("a", "b", "c", "ab", "bc"):
        for focal in (False, True):
            add(a="a" in abl, b="b" in abl, c="c" in abl, focal=focal, G=[3, 6], pt=0.7, nt=0.5)
    for focal in (False, True):
        add(levels=[(32, 32)], G=[1, 5, 11], focal=focal, pt=0.7, nt=0.5)
    for focal in (False, True):  # image 1's exemplar leaves a 2-px-wide rectangle no box reaches
        add(G=[3, 2], focal=focal, exemplars=[[0.3, 0.3, 0.5, 0.6], [0.0, 0.0, 1.0, 1.0]],
            boxes=[None, [[0.05, 0.05, 0.2, 0.2], [0.7, 0.75, 0.95, 0.9]]])
    for kind in ("zero_width", "duplicated", "grid_aligned"):
        for pt in (0.7, 1.0):
            add(boxes=[kind], pt=pt, nt=0.5, G=[4])
    add(exemplars=[[-0.1, 0.2, 0.3, 1.2]], G=[4], pt=0.5, nt=0.5)
    add(exemplars=[[0.6, -0.3, 1.4, 0.4], [0.45, 0.45, 0.55, 0.5]], G=[3, 3], focal=True, levels=[(12, 20)])
    return out


def main():
    R = import_reference()
    data, meta = {}, []
    for ci, c in enumerate(cases()):
        rng = np.random.default_rng(1000 + c["seed"])
        B = len(c["G"])
        H0, W0 = c["levels"][-1]
        gtb = []
        for bi in range(B):
            spec = c["boxes"][bi] if c["boxes"] else None
            if spec is None:
                gtb.append(rand_boxes(rng, c["G"][bi]))
            elif isinstance(spec, str):
                gtb.append(special_boxes(spec, rng, H0, W0))
            else:
                gtb.append(np.asarray(spec, np.float32))
        if c["exemplars"]:
            ex = np.asarray(c["exemplars"], np.float32)
        else:
            ex = rand_boxes(rng, B, 0.1, 0.3)
        args = SimpleNamespace(positive_threshold=c["pt"], negative_threshold=c["nt"],
                               ablation_no_box_regression=c["a"])
        batch = {"regression_ablation_a": c["a"], "regression_ablation_b": c["b"],
                 "regression_ablation_c": c["c"]}
        po, pr = [], []
        for (H, W) in c["levels"]:
            po.append(torch.from_numpy((rng.standard_normal((B, 1, H, W)) * 2.0).astype(np.float32)))
            pr.append(torch.from_numpy((rng.standard_normal((B, 4, H, W)) * 0.5).astype(np.float32)))
        gen = R.tu.GT_map(args)
        tb = [torch.from_numpy(b) for b in gtb]
        tex = [torch.from_numpy(ex[bi:bi + 1]) for bi in range(B)]
        with torch.no_grad():
            preds, gts, maps = gen.Get_pred_gts(po, pr, tb, tex, batch)
            loss = R.crit.SetCriterion_TM(c["focal"])(preds, gts)
        k = f"c{ci}_"
        for bi in range(B):
            data[k + f"boxes{bi}"] = gtb[bi]
        data[k + "exemplars"] = ex
        pads = np.zeros((len(c["levels"]), B, 2), np.int32)
        for lv, (H, W) in enumerate(c["levels"]):
            data[k + f"l{lv}_o"] = po[lv].numpy()
            data[k + f"l{lv}_reg"] = pr[lv].numpy()
            data[k + f"l{lv}_gt_map"] = maps[lv].numpy()
            data[k + f"l{lv}_pred_obj"] = preds["objectness"][lv].numpy()
            data[k + f"l{lv}_pred_reg"] = preds["regressions"][lv].numpy()
            data[k + f"l{lv}_gt_obj"] = gts["objectness"][lv].numpy()
            data[k + f"l{lv}_gt_reg"] = gts["regressions"][lv].numpy()
            for bi in range(B):  # the boundary pads, recorded from the reference's own mask
                nib = gen.Get_not_in_boundary(H, W, tex[bi][0], "cpu").reshape(H, W).numpy()
                ys, xs = np.flatnonzero(nib.any(1)), np.flatnonzero(nib.any(0))
                assert ys.size and xs.size, "an empty boundary rectangle is not a fixture case"
                assert ys[0] == H - 1 - ys[-1] and xs[0] == W - 1 - xs[-1]
                pads[lv, bi] = (xs[0], ys[0])
        data[k + "pads"] = pads
        data[k + "loss"] = np.array([float(loss["loss_ce"]), float(loss["loss_giou"])], np.float32)
        assert all(math.isfinite(float(v)) for v in data[k + "loss"])
        meta.append(dict(levels=c["levels"], B=B, pt=c["pt"], nt=c["nt"], a=c["a"], b=c["b"], c=c["c"],
                         focal=c["focal"]))
    data["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {len(meta)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
