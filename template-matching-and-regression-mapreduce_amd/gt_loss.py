"""Evaluation losses on the GPU (tmr_gt_loss, include/tmr.h): the GT target
maps of GT_map.Get_pred_gts (utils/TM_utils.py:94-222) and the BCE / focal and
GIoU sums of SetCriterion_TM (criterion/criterions_TM.py) for one level.

These are the launch wrappers the public surface shares (TMREngine.eval_loss,
tm_utils.GT_map, criterion.SetCriterion_TM).  Outputs carry no autograd graph:
training and backward are out of scope.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import exp_table, host
from ._lib import (GT_ASSIGN, GT_GATHER, GT_LOSS, GT_ROWS, TMRError, gt_loss, ptr, require_gpu, size,
                   stream)
from .graphs import _h2d


def _table(dev):
    from .engine import TMREngine
    return exp_table.device_table(dev) if TMREngine.exp_mode == "reference" else None


def host_boxes(gt_boxes) -> list:
    """Per-image GT boxes as host fp32 arrays (a device tensor is read back)."""
    return [b.detach().float().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float32)
            for b in gt_boxes]


class Assigned:
    """The device state of one TMR_GT_ASSIGN call (one level)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def assign(o: torch.Tensor, reg: Optional[torch.Tensor], units: np.ndarray, gt_boxes: Sequence,
           positive_threshold: float, negative_threshold: float, last_level: bool,
           focal: bool = False, with_loss: bool = False) -> Assigned:
    """TMR_GT_ASSIGN (| TMR_GT_LOSS) over o [U,1,H,W] / reg [U,4,H,W]:
    gt_map [U,1,H,W] fp32, target [U,H,W] int32, counts [U,2] int32 and, with
    the loss, sums [U,2] fp64 = {sum ce, sum giou}.  No sync."""
    require_gpu(o, "objectness")
    dev = o.device
    o = o.detach().float().contiguous()
    U, H, W = o.shape[0], o.shape[-2], o.shape[-1]
    if units.shape[0] != U:
        raise TMRError(f"{units.shape[0]} unit descriptors for {U} objectness maps")
    boxes, box_off, min_boxes = host.gt_box_table(host_boxes(gt_boxes))
    NI = len(box_off) - 1
    if U and (units["image"].min() < 0 or units["image"].max() >= NI):
        raise TMRError("a unit names an image outside gt_boxes")
    if min_boxes == 0:
        raise TMRError("an image without GT boxes (the reference's torch.min raises for it)")
    if reg is not None:
        reg = reg.detach().float().contiguous()
        if tuple(reg.shape) != (U, 4, H, W):
            raise TMRError(f"regressions {tuple(reg.shape)} do not match objectness {tuple(o.shape)}")
    elif (units["mode"] != 2).any():
        raise TMRError("regression maps are required unless box regression is ablated")
    st = Assigned(o=o, reg=reg, U=U, H=H, W=W, NI=NI, G_total=int(boxes.shape[0]), min_boxes=min_boxes,
                  focal=bool(focal), last_level=bool(last_level),
                  pt=float(positive_threshold), nt=float(negative_threshold), table=_table(dev))
    st.boxes = _h2d(boxes, dev)
    st.box_off = _h2d(box_off, dev)
    st.units = _h2d(units.view(np.uint8), dev)
    st.work = torch.empty(size("gt_work", st.G_total, NI, H, W, U), device=dev, dtype=torch.uint8)
    st.gt_map = torch.empty((U, 1, H, W), device=dev, dtype=torch.float32)
    st.target = torch.empty((U, H, W), device=dev, dtype=torch.int32)
    st.counts = torch.empty((U, 2), device=dev, dtype=torch.int32)
    st.sums = torch.empty((U, 2), device=dev, dtype=torch.float64) if with_loss else None
    _launch(st, GT_ASSIGN | (GT_LOSS if with_loss else 0))
    return st


def _launch(st: Assigned, phase: int, **extra) -> None:
    gt_loss(stream(st.o.device), o=ptr(st.o), reg=ptr(st.reg), boxes=ptr(st.boxes), box_off=ptr(st.box_off),
            units=ptr(st.units), exp_table=ptr(st.table), work=ptr(st.work), gt_map=ptr(st.gt_map),
            target=ptr(st.target), counts=ptr(st.counts), sums=ptr(st.sums),
            positive_threshold=st.pt, negative_threshold=st.nt, U=st.U, NI=st.NI, H=st.H, W=st.W,
            G_total=st.G_total, min_boxes=st.min_boxes, last_level=int(st.last_level), focal=int(st.focal),
            phase=phase, **extra)


def gather(st: Assigned):
    """TMR_GT_GATHER after assign(): reads the counts back (the one sync of
    the drop-in form) and returns (samples, labels, rows_pred, rows_gt,
    counts_host): every unit's positives then negatives in row-major order and
    its prediction / GT rows (or the dummy pair), unit after unit."""
    dev = st.o.device
    counts = st.counts.cpu().numpy().astype(np.int64)
    n_s = counts.sum(1)
    n_r = np.maximum(counts[:, 0], 1)
    samp_off = np.concatenate([[0], np.cumsum(n_s)[:-1]]).astype(np.int64)
    row_off = np.concatenate([[0], np.cumsum(n_r)[:-1]]).astype(np.int64)
    ts, tr = int(n_s.sum()), int(n_r.sum())
    obj = torch.empty(ts, device=dev, dtype=torch.float32)
    lab = torch.empty(ts, device=dev, dtype=torch.float32)
    rp = torch.empty((tr, 4), device=dev, dtype=torch.float32)
    rg = torch.empty((tr, 4), device=dev, dtype=torch.float32)
    so, ro = _h2d(samp_off, dev), _h2d(row_off, dev)
    # an empty sample list still needs non-NULL pointers (nothing is written)
    keep = [t if t.numel() else torch.empty(4, device=dev, dtype=torch.float32) for t in (obj, lab)]
    _launch(st, GT_GATHER, samp_off=ptr(so), row_off=ptr(ro), obj_out=ptr(keep[0]), label_out=ptr(keep[1]),
            rows_pred=ptr(rp), rows_gt=ptr(rg))
    return obj, lab, rp, rg, counts


def rows_loss(samples: torch.Tensor, labels: torch.Tensor, rows_pred: torch.Tensor, rows_gt: torch.Tensor,
              focal: bool) -> torch.Tensor:
    """TMR_GT_ROWS: fp64 [2] = {sum ce, sum giou} over gathered lists."""
    require_gpu(samples, "samples")
    dev = samples.device
    s = samples.detach().float().contiguous().reshape(-1)
    t = labels.detach().float().contiguous().reshape(-1)
    p = rows_pred.detach().float().contiguous().reshape(-1, 4)
    g = rows_gt.detach().float().contiguous().reshape(-1, 4)
    if s.shape != t.shape or p.shape != g.shape:
        raise TMRError("samples / labels or prediction / GT rows differ in length")
    work = torch.empty(size("gt_work", 1, 1, 1, 1, 1), device=dev, dtype=torch.uint8)
    sums = torch.empty(2, device=dev, dtype=torch.float64)
    gt_loss(stream(dev), phase=GT_ROWS, work=ptr(work), sums=ptr(sums), focal=int(bool(focal)),
            obj_out=ptr(s) if s.numel() else None, label_out=ptr(t) if t.numel() else None,
            rows_pred=ptr(p) if p.numel() else None, rows_gt=ptr(g) if g.numel() else None,
            n_samples=s.numel(), n_rows=p.shape[0])
    return sums


def group_losses(sums: torch.Tensor, counts: torch.Tensor, groups: Optional[Sequence[int]]):
    """(loss_ce, loss_giou) fp32 per group from the per-unit sums / counts of
    one level: sum over the group's units / its number of rows (a unit
    without a positive pixel counts its dummy row).  On the device, no sync,
    fixed order."""
    U = sums.shape[0]
    rows = counts[:, 0].clamp(min=1).to(torch.float64)
    vals = torch.cat([sums, rows[:, None]], 1)  # [U,3]
    if groups is None:
        tot = vals.sum(0, keepdim=True)
    else:
        g = np.asarray(groups, np.int64).reshape(-1)
        if g.shape[0] != U or (U and g.min() < 0):
            raise TMRError("groups: one non-negative group index per unit")
        ng = int(g.max()) + 1 if U else 0
        onehot = np.zeros((ng, U), np.float64)
        onehot[g, np.arange(U)] = 1.0
        tot = (_h2d(onehot, sums.device)[:, :, None] * vals[None]).sum(1)
    ce, gi = (tot[:, 0] / tot[:, 2]).float(), (tot[:, 1] / tot[:, 2]).float()
    return (ce[0], gi[0]) if groups is None else (ce, gi)
