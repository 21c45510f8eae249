"""Drop-in evaluation criterion (reference: criterion/criterions_TM.py,
criterion/__init__.py).

``SetCriterion_TM`` keeps the reference's call form -- ``criterion(preds,
gts)`` on the dicts ``GT_map.Get_pred_gts`` returns -- and its result: a dict
of 0-d fp32 tensors ``loss_ce`` and ``loss_giou``.  The element losses and
their fp64 fixed-order sums run in libtmr.so (tmr_gt_loss, TMR_GT_ROWS), so a
repeat call gives the same bits.  Outputs carry no autograd graph: training
and backward are out of scope (the reference's evaluation steps,
trainer.py:75-153, only log these values).
"""
from __future__ import annotations

import torch
from torch import nn

from . import gt_loss as gl
from ._lib import TMRError


def _empty_like_rows(t: torch.Tensor) -> torch.Tensor:
    return torch.empty((0, 4), device=t.device, dtype=torch.float32)


def gIoU_loss(pred, target, reduction="sum"):
    """criterions_TM.py:7-13: generalized_box_iou_loss(eps=1e-13) of
    [cx, cy, w, h] rows, summed ("sum") or averaged ("mean") in fp64 on the
    GPU; a 0-d fp32 tensor.  The per-row form (reduction="none") is not
    provided: the kernel reduces as it goes."""
    if reduction not in ("sum", "mean"):
        raise TMRError("gIoU_loss: reduction must be 'sum' or 'mean' (the kernel reduces as it goes)")
    empty = torch.empty(0, device=pred.device, dtype=torch.float32)
    s = gl.rows_loss(empty, empty, pred, target, False)[1]
    if reduction == "mean":
        s = s / max(1, pred.shape[0])
    return s.float()


class WeightedFocalLoss(nn.Module):
    """criterions_TM.py:15-30 with the reference's alpha = .25, gamma = 2
    (the only form its criterion builds).  ``forward`` returns the SUM of the
    element losses (0-d fp32), which is all SetCriterion_TM uses."""

    def __init__(self, alpha=.25, gamma=2):
        super().__init__()
        if float(alpha) != 0.25 or float(gamma) != 2.0:
            raise TMRError("WeightedFocalLoss: the kernel implements alpha=.25, gamma=2")
        self.alpha, self.gamma = alpha, gamma

    def forward(self, inputs, targets):
        return gl.rows_loss(inputs, targets, _empty_like_rows(inputs), _empty_like_rows(inputs), True)[0].float()


class SetCriterion_TM(nn.Module):
    """criterions_TM.py:32-58: per level, sum(ce) / num_positive and
    sum(giou) / num_positive with num_positive = the level's number of
    regression rows (dummy rows included), then the mean over levels."""

    def __init__(self, use_focal_loss=False):
        super().__init__()
        self.use_focal_loss = bool(use_focal_loss)

    def forward(self, outputs, targets):
        ce_losses, bboxes_losses = [], []
        for level in range(len(outputs["objectness"])):
            num_positive = len(targets["regressions"][level])
            sums = gl.rows_loss(outputs["objectness"][level], targets["objectness"][level],
                                outputs["regressions"][level], targets["regressions"][level],
                                self.use_focal_loss)
            per = (sums / num_positive).float()
            ce_losses.append(per[0])
            bboxes_losses.append(per[1])
        return {"loss_ce": torch.stack(ce_losses).mean(), "loss_giou": torch.stack(bboxes_losses).mean()}


def build_criterion(args):
    """criterion/__init__.py:3-6."""
    return SetCriterion_TM(args.focal_loss)
