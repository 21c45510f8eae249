"""COCO AP on the GPU (reference: utils/log_utils.py:137-205 through
pycocotools' COCOeval, as eval_log.CocoEvalMaxDets restates it).

* ``CocoEvalGPU``: CocoEvalMaxDets with the per-image matching in one
  tmr_coco_match call (include/tmr_coco.h) and the accumulation in torch on the
  same device.  Same constructor, ``params``, evaluate / accumulate /
  summarize, ``eval`` and ``stats``; every array equals the numpy class's bit
  for bit (integer counts and single IEEE fp64 operations, no tolerance).
* ``APMeter``: the in-memory form of image_info_collector ->
  coco_style_annotation_generator -> Get_MAE_RMSE + Get_AP_scores: kept
  detections stay device tensors, no JSON file is written, and the host reads
  results only in ``compute()``.

Like the numpy restatement it matches, this is parity-unpinned against
pycocotools itself (not importable here).
"""
from __future__ import annotations

from itertools import chain
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream
from .eval_log import CocoEvalMaxDets

_F64 = torch.float64


class _Pack:
    """One category's images in CSR form: host offsets, device arrays.  The
    detections of an image are in descending score order (stable) and cut to
    the largest maxDets."""

    def __init__(self, det_off, gt_off, det_box, det_area, det_score, gt_box, gt_area, gt_crowd):
        self.det_off = np.ascontiguousarray(det_off, np.int64)
        self.gt_off = np.ascontiguousarray(gt_off, np.int64)
        self.det_box, self.det_area, self.det_score = det_box, det_area, det_score
        self.gt_box, self.gt_area, self.gt_crowd = gt_box, gt_area, gt_crowd
        self.sum_d, self.sum_g = int(self.det_off[-1]), int(self.gt_off[-1])
        nd, ng = np.diff(self.det_off), np.diff(self.gt_off)
        self.max_d = int(nd.max()) if nd.size else 0
        self.max_g = int(ng.max()) if ng.size else 0
        # position of each detection inside its image
        self.pos = np.arange(self.sum_d, dtype=np.int64) - np.repeat(self.det_off[:-1], nd)

    @property
    def n_img(self):
        return len(self.det_off) - 1


def match_plan(pack: _Pack, A: int, T: int):
    """tmr_coco_match_plan for a pack: host only (no pointer is dereferenced)."""
    return _lib.coco_match_plan(I=0, A=A, T=T) if pack.n_img == 0 else _lib.coco_match_plan(
        det_off=1, det_box=1, det_area=1, gt_off=1, gt_box=1, gt_area=1, gt_crowd=1, area_rng=1, iou_thr=1,
        dt_match=1, dt_ignore=1, gt_ignore=1, gt_match=1, sum_d=pack.sum_d, sum_g=pack.sum_g, I=pack.n_img,
        A=A, T=T, max_d=pack.max_d, max_g=pack.max_g)


def coco_match(pack: _Pack, area_rng, iou_thrs, device) -> Dict[str, torch.Tensor]:
    """One tmr_coco_match call on the current stream: dt_match [A,T,sum_d] int32
    (ground truth index in its image + 1, or 0), dt_ignore [A,T,sum_d] uint8,
    gt_ignore [A,sum_g] uint8, gt_match [A,T,sum_g] int32.  Nothing is read back."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.TMRError("tmr_coco_match runs on a HIP device (MI355X); no CPU path exists")
    ar = torch.as_tensor(np.asarray(area_rng, np.float64).reshape(-1, 2)).to(device)
    th = torch.as_tensor(np.asarray(iou_thrs, np.float64).reshape(-1)).to(device)  # as the host made them
    A, T = int(ar.shape[0]), int(th.shape[0])
    out = {"dt_match": torch.empty((A, T, pack.sum_d), dtype=torch.int32, device=device),
           "dt_ignore": torch.empty((A, T, pack.sum_d), dtype=torch.uint8, device=device),
           "gt_ignore": torch.empty((A, pack.sum_g), dtype=torch.uint8, device=device),
           "gt_match": torch.empty((A, T, pack.sum_g), dtype=torch.int32, device=device)}
    det_off = torch.from_numpy(pack.det_off).to(device)
    gt_off = torch.from_numpy(pack.gt_off).to(device)
    _lib.coco_match(stream(device), det_off=ptr(det_off), det_box=ptr(pack.det_box), det_area=ptr(pack.det_area),
                    gt_off=ptr(gt_off), gt_box=ptr(pack.gt_box), gt_area=ptr(pack.gt_area),
                    gt_crowd=ptr(pack.gt_crowd), area_rng=ptr(ar), iou_thr=ptr(th),
                    dt_match=ptr(out["dt_match"]), dt_ignore=ptr(out["dt_ignore"]),
                    gt_ignore=ptr(out["gt_ignore"]), gt_match=ptr(out["gt_match"]),
                    sum_d=pack.sum_d, sum_g=pack.sum_g, I=pack.n_img, A=A, T=T, max_d=pack.max_d, max_g=pack.max_g)
    return out


class CocoEvalGPU(CocoEvalMaxDets):
    """CocoEvalMaxDets with the matching on the GPU.  ``params.maxDets``,
    ``iouThrs`` and ``areaRng`` are honoured as set before ``evaluate()``
    (T <= 16, maxDets[-1] <= 4096, ground truths per image <= 65536; beyond
    that the kernel refuses: TMRError)."""

    def __init__(self, gt: dict, dt_anns: List[dict], device="cuda:0"):
        super().__init__(gt, dt_anns)
        self.device = torch.device(device)
        self._packs: Optional[List[_Pack]] = None
        self._preset = False
        self._matches: List[Dict[str, torch.Tensor]] = []

    # ------------------------------------------------------------- evaluate
    def _pack_all(self) -> List[_Pack]:
        """_prepare's grouping and filtering and _compute_iou's ordering, as array
        passes over the annotation lists instead of per-image Python loops: one
        pack per category, images in params.imgIds order, each image's ground
        truths in file order and its detections in descending score order
        (stable), cut at maxDets[-1]."""
        p = self.params
        dev = self.device
        img_pos = {im: i for i, im in enumerate(p.imgIds)}
        cat_pos = {c: k for k, c in enumerate(p.catIds)}
        n_img = len(p.imgIds)

        def columns(anns, extra):
            n = len(anns)
            img = np.fromiter((img_pos.get(x["image_id"], -1) for x in anns), np.int64, n)
            cat = np.fromiter((cat_pos.get(x["category_id"], -1) for x in anns), np.int64, n)
            box = np.fromiter(chain.from_iterable(x["bbox"] for x in anns), np.float64, 4 * n).reshape(n, 4)
            area = np.fromiter((x["area"] for x in anns), np.float64, n)
            return img, cat, box, area, extra(anns, n)

        g_img, g_cat, g_box, g_area, g_crowd = columns(
            self.gt.get("annotations", []), lambda A, n: np.fromiter((int(x["iscrowd"]) for x in A), np.uint8, n))
        d_img, d_cat, d_box, d_area, d_score = columns(
            self.dt, lambda A, n: np.fromiter((x["score"] for x in A), np.float64, n))

        def up(x):
            return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

        packs = []
        for k in range(len(p.catIds)):
            gi = np.flatnonzero((g_img >= 0) & (g_cat == k))
            gi = gi[np.argsort(g_img[gi], kind="stable")]
            di = np.flatnonzero((d_img >= 0) & (d_cat == k))
            di = di[np.lexsort((-d_score[di], d_img[di]))]  # by image, then descending score; stable
            nd = np.bincount(d_img[di], minlength=n_img)
            first = np.concatenate([[0], np.cumsum(nd)])[:-1]
            di = di[np.arange(di.size) - np.repeat(first, nd) < p.maxDets[-1]]
            nd = np.minimum(nd, p.maxDets[-1])
            ng = np.bincount(g_img[gi], minlength=n_img)
            packs.append(_Pack(np.concatenate([[0], np.cumsum(nd)]), np.concatenate([[0], np.cumsum(ng)]),
                               up(d_box[di]), up(d_area[di]), up(d_score[di]), up(g_box[gi]), up(g_area[gi]),
                               up(g_crowd[gi])))
        return packs

    def set_packs(self, packs: List[_Pack]):
        """Device-resident inputs (APMeter): one pack per category, images in
        np.unique(imgIds) order; evaluate() then packs nothing."""
        self._packs, self._preset = packs, True

    def _normalise_params(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        return p

    def evaluate(self):
        p = self._normalise_params()
        if not self._preset:
            self._packs = self._pack_all()
        self._matches = [coco_match(pk, p.areaRng, p.iouThrs, self.device) for pk in self._packs]

    def load_matches(self, ev: CocoEvalMaxDets):
        """Take a numpy evaluator's per-image results (after its evaluate())
        instead of running the kernel: accumulate() then runs on any device,
        CPU included.  gt_ignore is in that evaluator's (ignore-sorted) order
        and gt_match is not carried."""
        p = self._normalise_params()
        dev = self.device
        A, I0, T = len(p.areaRng), len(p.imgIds), len(p.iouThrs)
        self._packs, self._matches, self._preset = [], [], True
        for k in range(len(p.catIds)):
            E = [[ev.evalImgs[k * A * I0 + a * I0 + i] for i in range(I0)] for a in range(A)]
            nd = [0 if e is None else len(e["dtScores"]) for e in E[0]]
            ng = [0 if e is None else len(e["gtIgnore"]) for e in E[0]]
            score = np.concatenate([np.asarray(e["dtScores"], np.float64) for e in E[0] if e is not None]
                                   + [np.zeros(0)])
            z4, z1 = torch.zeros((0, 4), dtype=_F64, device=dev), torch.zeros((0,), dtype=_F64, device=dev)
            self._packs.append(_Pack(np.concatenate([[0], np.cumsum(nd)]), np.concatenate([[0], np.cumsum(ng)]),
                                     z4, z1, torch.from_numpy(score).to(dev), z4, z1,
                                     torch.zeros((0,), dtype=torch.uint8, device=dev)))

            def cat(key, width, dtype):
                n_of = "gtIgnore" if key == "gtIgnore" else "dtScores"
                rows = [np.concatenate([np.asarray(e[key]).reshape(width, len(e[n_of])) for e in Ea if e is not None]
                                       + [np.zeros((width, 0))], axis=1) for Ea in E]
                return torch.from_numpy(np.ascontiguousarray(np.stack(rows) != 0).astype(dtype)).to(dev)

            self._matches.append({"dt_match": cat("dtMatches", T, np.int32),
                                  "dt_ignore": cat("dtIgnore", T, np.uint8),
                                  "gt_ignore": cat("gtIgnore", 1, np.uint8)[:, 0]})

    # ----------------------------------------------------------- accumulate
    def accumulate(self):
        """COCOeval.accumulate in torch on ``self.device`` (device-agnostic):
        integer cumulative sums, one fp64 division per recall / precision
        value, the reverse running maximum and a left searchsorted with
        pycocotools' stop at the first index past the end.  One transfer to the
        host, of the finished tables."""
        p = self.params
        dev = self.device
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        precision = torch.full((T, R, K, A, M), -1.0, dtype=_F64, device=dev)
        recall = torch.full((T, K, A, M), -1.0, dtype=_F64, device=dev)
        scores = torch.full((T, R, K, A, M), -1.0, dtype=_F64, device=dev)
        rth = torch.from_numpy(np.asarray(p.recThrs, np.float64)).to(dev).expand(T, R).contiguous()
        eps = float(np.spacing(1))
        zero = torch.zeros((), dtype=_F64, device=dev)
        for k, (pk, mt) in enumerate(zip(self._packs, self._matches)):
            if pk.sum_d == 0 and pk.sum_g == 0:  # no image has a ground truth or a detection
                continue
            npig_all = (mt["gt_ignore"] == 0).sum(dim=1)  # [A], stays on the device
            for m, max_det in enumerate(p.maxDets):
                sel_np = np.flatnonzero(pk.pos < max_det)  # each image's first max_det, in image order
                nd = int(sel_np.size)
                if nd:
                    sel = torch.from_numpy(sel_np).to(dev)
                    s = pk.det_score[sel]
                    order = torch.sort(-s, stable=True).indices
                    s_sorted, idx = s[order], sel[order]
                for a in range(A):
                    npig = npig_all[a]
                    has = npig > 0  # a cell without a non-ignored ground truth keeps its -1
                    if nd == 0:
                        zero_or_keep = torch.where(has, zero, -1.0)
                        recall[:, k, a, m] = zero_or_keep
                        precision[:, :, k, a, m] = zero_or_keep
                        scores[:, :, k, a, m] = zero_or_keep
                        continue
                    dtm = mt["dt_match"][a][:, idx] != 0
                    dig = mt["dt_ignore"][a][:, idx] != 0
                    tp = torch.cumsum(dtm & ~dig, dim=1, dtype=torch.int64).to(_F64)
                    fp = torch.cumsum(~dtm & ~dig, dim=1, dtype=torch.int64).to(_F64)
                    rc = tp / npig.to(_F64)
                    pr = tp / (fp + tp + eps)
                    pr = torch.cummax(pr.flip(1), dim=1).values.flip(1)
                    ri = torch.searchsorted(rc.contiguous(), rth, side="left")
                    ok = torch.cumprod((ri < nd).to(torch.int64), dim=1).bool()
                    rj = ri.clamp(max=nd - 1)
                    q = torch.where(ok, pr.gather(1, rj), 0.0)
                    ss = torch.where(ok, s_sorted[rj], 0.0)
                    recall[:, k, a, m] = torch.where(has, rc[:, -1], -1.0)
                    precision[:, :, k, a, m] = torch.where(has, q, -1.0)
                    scores[:, :, k, a, m] = torch.where(has, ss, -1.0)
        self.eval = {"params": p, "counts": [T, R, K, A, M], "precision": precision.cpu().numpy(),
                     "recall": recall.cpu().numpy(), "scores": scores.cpu().numpy()}

    # ------------------------------------------------------------ per image
    def eval_imgs(self, a: int, k: int = 0) -> List[Optional[dict]]:
        """Area range a's per-image results in CocoEvalMaxDets.evalImgs' form
        (None for an image with neither ground truths nor detections):
        dtMatches [T,D] (ground truth index in the image + 1, or 0) and
        gtMatches [T,G] (detection index + 1, or 0) -- compare their nonzero
        patterns --, dtIgnore [T,D] bool, dtScores [D], and gtIgnore [G] /
        gtMatches in pycocotools' order (ground truths sorted by ignore flag,
        stably).  Reads the match arrays back."""
        pk, mt = self._packs[k], self._matches[k]
        dtm, dig = mt["dt_match"][a].cpu().numpy(), mt["dt_ignore"][a].cpu().numpy()
        gig, gtm = mt["gt_ignore"][a].cpu().numpy(), mt["gt_match"][a].cpu().numpy()
        sc = pk.det_score.cpu().numpy()
        out = []
        for i in range(pk.n_img):
            d0, d1, g0, g1 = pk.det_off[i], pk.det_off[i + 1], pk.gt_off[i], pk.gt_off[i + 1]
            if d0 == d1 and g0 == g1:
                out.append(None)
                continue
            gtind = np.argsort(gig[g0:g1], kind="mergesort")
            out.append({"dtMatches": dtm[:, d0:d1], "dtIgnore": dig[:, d0:d1] != 0, "dtScores": sc[d0:d1],
                        "gtIgnore": gig[g0:g1][gtind].astype(np.int64), "gtMatches": gtm[:, g0:g1][:, gtind]})
        return out


# ---------------------------------------------------------------- APMeter
def gt_refine(orig_boxes, device=None) -> torch.Tensor:
    """eval_log.gt_refinery's arithmetic on tensors: xyxy -> xywh in the input's
    dtype, round half to even, int64 [G,4]."""
    b = torch.as_tensor(np.asarray(orig_boxes) if not isinstance(orig_boxes, torch.Tensor) else orig_boxes)
    b = b.reshape(-1, 4)
    if device is not None:
        b = b.to(device)
    if not b.is_floating_point():
        b = b.to(_F64)
    return torch.round(torch.cat((b[:, :2], b[:, 2:] - b[:, :2]), dim=1)).to(torch.int64)


def pred_refine(logits, bboxes, ref_points, img_size):
    """eval_log.pred_refinery's arithmetic on tensors, without the filtering
    (no synchronisation): (keep [N] bool = logits[:,0] >= 0, boxes int64 [N,4]
    pixel xywh, points int64 [N,2] or None).  fp32 multiply by the image size,
    round half to even, int, then xyxy -> xywh on the integers."""
    img_w, img_h = int(img_size[0]), int(img_size[1])
    lg = logits.reshape(-1, logits.shape[-1])
    keep = lg[:, 0] >= 0.0
    bx = bboxes.reshape(-1, 4).to(torch.float32)
    s4 = torch.tensor([img_w, img_h, img_w, img_h], dtype=torch.float32, device=bx.device)
    bx = torch.round(bx * s4).to(torch.int64)
    bx = torch.cat((bx[:, :2], bx[:, 2:] - bx[:, :2]), dim=1)
    pts = None
    if ref_points is not None:
        pts = torch.round(ref_points.reshape(-1, 2).to(torch.float32) * s4[:2]).to(torch.int64)
    return keep, bx, pts


class APMeter:
    """AP / AP50 / AP75 / MAE / RMSE of an evaluation epoch, in memory.

    ``update(batch, pred_logits, pred_boxes, ref_points)`` takes
    image_info_collector's arguments and keeps compact per-image device
    tensors (the refineries' arithmetic runs on the device, nothing is read
    back); ``compute()`` runs the matching and the accumulation on the device
    and reads the results back once the tables are finished (before that only
    the per-image kept counts, which size the kernel's launch).

    Images are ordered by sorted ``img_id``.  An image without a kept row
    contributes no detection.  The file path's "dummy prediction" for that
    case (eval_log.coco_style_annotation_generator, the branch at
    ``len(preds["annotations"]) == 0``) depends on the directory's listing
    order; it cannot occur for Get_pred_boxes / NMS outputs, which always carry
    a row (the dummy row of an image without candidates has score 0 and is
    kept, so it counts as a detection here as it does in Get_MAE_RMSE)."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self._imgs: List[tuple] = []
        self.stats = None
        self.evaluator: Optional[CocoEvalGPU] = None

    def reset(self):
        self._imgs, self.stats, self.evaluator = [], None, None

    def update(self, batch, pred_logits, pred_boxes, ref_points=None):
        dev = self.device
        for b in range(len(batch["img_name"])):
            size = batch["img_size"][b]
            size = size.tolist() if hasattr(size, "tolist") else list(size)
            gt = gt_refine(batch["orig_boxes"][b], dev)
            lg = torch.as_tensor(pred_logits[b]).to(dev)
            keep, bx, _ = pred_refine(lg, torch.as_tensor(pred_boxes[b]).to(dev), None, size)
            img_id = batch["img_id"][b]
            img_id = img_id.item() if hasattr(img_id, "item") else img_id
            self._imgs.append((img_id, gt, lg.reshape(-1, lg.shape[-1])[:, 0].to(_F64), keep, bx))

    def compute(self):
        """(AP, AP50, AP75, MAE, RMSE), AP in percent with negatives -> 0 as
        Get_AP_scores; ``stats`` holds the 12 COCO numbers."""
        if not self._imgs:
            raise _lib.TMRError("APMeter.compute: no image was added")
        dev = self.device
        imgs = sorted(self._imgs, key=lambda r: r[0])
        n_img = len(imgs)
        ids = [r[0] for r in imgs]
        n_gt = [int(r[1].shape[0]) for r in imgs]
        rows = [int(r[3].shape[0]) for r in imgs]
        img_of = torch.from_numpy(np.repeat(np.arange(n_img), rows)).to(dev)
        keep = torch.cat([r[3] for r in imgs])
        kept = torch.nonzero(keep).flatten()
        n_pred = torch.bincount(img_of[kept], minlength=n_img).cpu().numpy().astype(np.int64)
        score = torch.cat([r[2] for r in imgs])[kept]
        box = torch.cat([r[4] for r in imgs])[kept]
        img_of = img_of[kept]
        # per image: descending score, stable; then the cut at the largest maxDets
        ev = CocoEvalGPU({"images": [{"id": i} for i in ids], "categories": [{"id": 1}]}, [], device=dev)
        max_det = sorted(ev.params.maxDets)[-1]
        o1 = torch.sort(-score, stable=True).indices
        perm = o1[torch.sort(img_of[o1], stable=True).indices]
        off_full = np.concatenate([[0], np.cumsum(n_pred)])
        pos = np.arange(int(off_full[-1]), dtype=np.int64) - np.repeat(off_full[:-1], n_pred)
        perm = perm[torch.from_numpy(np.flatnonzero(pos < max_det)).to(dev)]
        n_cut = np.minimum(n_pred, max_det)
        box = box[perm]
        gt = torch.cat([r[1] for r in imgs])
        pack = _Pack(np.concatenate([[0], np.cumsum(n_cut)]), np.concatenate([[0], np.cumsum(n_gt)]),
                     box.to(_F64).contiguous(), (box[:, 2] * box[:, 3]).to(_F64).contiguous(),
                     score[perm].contiguous(), gt.to(_F64).contiguous(),
                     (gt[:, 2] * gt[:, 3]).to(_F64).contiguous(),
                     torch.zeros((gt.shape[0],), dtype=torch.uint8, device=dev))
        ev.set_packs([pack])
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
        self.evaluator, self.stats = ev, ev.stats
        ap, ap50, ap75 = (float(ev.stats[i] * 100 if ev.stats[i] >= 0 else 0) for i in range(3))
        # Get_MAE_RMSE: per image |#gt - #pred| over every image
        error = sum(abs(g - int(q)) for g, q in zip(n_gt, n_pred))
        squared = sum((g - int(q)) ** 2 for g, q in zip(n_gt, n_pred))
        return ap, ap50, ap75, error / n_img, np.sqrt(squared / n_img)
