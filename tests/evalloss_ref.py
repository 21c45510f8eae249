"""TEST HELPER: a numpy restatement of the evaluation losses (include/tmr.h,
tmr_gt_loss), written from the per-pixel statement of the semantics and not
from the reference's text.

Class and target arithmetic is fp32 with every operation separately rounded;
the losses are evaluated in float64 from the fp32 samples and rows.  The
random GPU sweeps compare against this file; tests/test_evalloss_host.py pins
it to tests/golden/evalloss.npz (the reference's own GT_map and
SetCriterion_TM) on the CPU.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
DUMMY = np.array([[0.0, 0.0, 1e-14, 1e-14]], np.float32)


def box_records(boxes, pt: float, nt: float):
    """Per GT box: cx, cy, ws, hs, ratio, bias_p, bias_n, area (fp32)."""
    b = np.asarray(boxes, f32).reshape(-1, 4)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cx, cy = (x2 + x1) / f32(2), (y2 + y1) / f32(2)
        ws, hs = x2 - x1, y2 - y1
        ratio = -hs / ws
        bias_p = f32((1.0 - pt) / (1.0 + pt)) * hs
        bias_n = f32((1.0 - nt) / (1.0 + nt)) * hs
        area = (x2 - x1) * (y2 - y1)
    return dict(cx=cx, cy=cy, ws=ws, hs=hs, ratio=ratio, bias_p=bias_p, bias_n=bias_n, area=area)


def pixel_centers(H: int, W: int):
    """(cxs, cys) per pixel i = y*W + x: fl32(x)/fl32(W), fl32(y)/fl32(H)."""
    xs = np.arange(W, dtype=f32) / f32(W)
    ys = np.arange(H, dtype=f32) / f32(H)
    return np.tile(xs, H), np.repeat(ys, W)


def classify_image(boxes, H: int, W: int, pt: float, nt: float, last_level: bool):
    """The per-image part: any_pos, all_pos, any_notneg (bool [H*W]) and
    target (int [H*W]), one box at a time (no [H*W, G] matrix)."""
    r = box_records(boxes, pt, nt)
    cxs, cys = pixel_centers(H, W)
    HW, G = H * W, len(r["cx"])
    if G == 0:
        raise ValueError("an image without GT boxes")
    any_pos = np.zeros(HW, bool)
    all_pos = np.ones(HW, bool)
    any_notneg = np.zeros(HW, bool)
    best_a = np.zeros(HW, f32)
    target = np.zeros(HW, np.int64)
    idx = np.arange(HW)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(G):
            rx = np.abs(cxs - r["cx"][g])
            ry = np.abs(cys - r["cy"][g])
            t = (r["ratio"][g] * rx).astype(f32)
            inpos = (t + r["bias_p"][g]).astype(f32) >= ry
            inneg = (t + r["bias_n"][g]).astype(f32) < ry
            isc = idx == int(np.argmin((rx + ry).astype(f32)))  # the lowest index on ties
            if pt == 1.0:
                inpos = isc
            if nt == 1.0:
                inneg = ~isc
            pos = (inpos | isc) if last_level else inpos
            any_pos |= pos
            all_pos &= pos
            any_notneg |= ~inneg
            a = np.where(pos, r["area"][g], f32(100000000.0)).astype(f32)
            take = a < best_a if g else np.ones(HW, bool)
            best_a = np.where(take, a, best_a)
            target = np.where(take, g, target)
    return any_pos, all_pos, any_notneg, target


def unit_classes(cls, H: int, W: int, pad_x: int, pad_y: int):
    """A unit's rectangle over its image's classes -> dict of positive,
    negative (bool [H*W]), gt_map (fp32 [H,W]), target (int32 [H,W])."""
    any_pos, all_pos, any_notneg, target = cls
    y, x = np.repeat(np.arange(H), W), np.tile(np.arange(W), H)
    nib = (y >= pad_y) & (y < H - pad_y) & (x >= pad_x) & (x < W - pad_x)
    positive = nib & any_pos
    ignore = nib & ~all_pos & any_notneg
    negative = ~(positive | ignore)
    gt_map = np.where(positive, f32(1.0), np.where(negative, f32(0.0), f32(0.5))).astype(f32)
    return dict(positive=positive, negative=negative, gt_map=gt_map.reshape(H, W),
                target=np.where(positive, target, 0).astype(np.int32).reshape(H, W))


def pred_rows(reg, positive, H: int, W: int, scale_w, scale_h, mode: int, expf):
    """(cx, cy, w, h) rows of the positive pixels, fp32; `expf` is the decode's
    exp (oracle.expf)."""
    idx = np.flatnonzero(positive)
    cxs, cys = pixel_centers(H, W)
    if mode == 2 or reg is None:
        r = np.zeros((idx.size, 4), f32)
    else:
        r = np.ascontiguousarray(np.asarray(reg, f32).reshape(4, H * W)[:, idx].T)
    sw, sh = f32(scale_w), f32(scale_h)
    sxy = np.array([1.0, 1.0], f32) if mode == 1 else np.array([sw, sh], f32)
    xy = (np.stack([cxs[idx], cys[idx]], 1) + (r[:, :2] * sxy).astype(f32)).astype(f32)
    wh = (expf(r[:, 2:]) * np.array([sw, sh], f32)).astype(f32)
    return np.concatenate([xy, wh], 1).astype(f32)


def gt_rows(boxes, target, positive):
    r = box_records(boxes, 0.5, 0.5)
    t = np.asarray(target).reshape(-1)[np.flatnonzero(positive)]
    return np.stack([r["cx"][t], r["cy"][t], r["ws"][t], r["hs"][t]], 1).astype(f32)


def unit(o, reg, boxes, cls, H, W, pad_x, pad_y, scale_w, scale_h, mode, expf):
    """Everything of one unit: its classes, samples (positives then negatives,
    row-major), labels and pred / gt rows (the dummy pair when no pixel is
    positive)."""
    u = unit_classes(cls, H, W, pad_x, pad_y)
    of = np.asarray(o, f32).reshape(-1)
    u["samples"] = np.concatenate([of[u["positive"]], of[u["negative"]]])
    u["labels"] = np.concatenate([np.ones(int(u["positive"].sum()), f32),
                                  np.zeros(int(u["negative"].sum()), f32)])
    if u["positive"].any():
        u["pred"] = pred_rows(reg, u["positive"], H, W, scale_w, scale_h, mode, expf)
        u["gt"] = gt_rows(boxes, u["target"], u["positive"])
    else:
        u["pred"], u["gt"] = DUMMY.copy(), DUMMY.copy()
    return u


def ce_terms(x, t, focal: bool):
    """BCE with logits per element (float64), optionally the weighted focal form."""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    ce = np.maximum(x, 0.0) - x * t + np.log1p(np.exp(-np.abs(x)))
    if focal:
        at = np.where(t == 1.0, 0.25, 0.75)
        ce = at * (1.0 - np.exp(-ce)) ** 2 * ce
    return ce


def giou_terms(pred, gt, eps: float = 1e-13):
    """generalized_box_iou_loss per cxcywh row pair (float64)."""
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    x1, y1, x2, y2 = p[:, 0] - p[:, 2] / 2, p[:, 1] - p[:, 3] / 2, p[:, 0] + p[:, 2] / 2, p[:, 1] + p[:, 3] / 2
    a1, b1, a2, b2 = g[:, 0] - g[:, 2] / 2, g[:, 1] - g[:, 3] / 2, g[:, 0] + g[:, 2] / 2, g[:, 1] + g[:, 3] / 2
    xk1, yk1, xk2, yk2 = np.maximum(x1, a1), np.maximum(y1, b1), np.minimum(x2, a2), np.minimum(y2, b2)
    ok = (yk2 > yk1) & (xk2 > xk1)
    inter = np.where(ok, (xk2 - xk1) * (yk2 - yk1), 0.0)
    union = (x2 - x1) * (y2 - y1) + (a2 - a1) * (b2 - b1) - inter
    iou = inter / (union + eps)
    ac = (np.maximum(x2, a2) - np.minimum(x1, a1)) * (np.maximum(y2, b2) - np.minimum(y1, b1))
    return 1.0 - iou + (ac - union) / (ac + eps)


def losses(units, focal: bool):
    """(loss_ce, loss_giou) of one criterion call over `units` (one level):
    the sums over every unit's samples / rows divided by the number of rows."""
    n = sum(len(u["pred"]) for u in units)
    ce = sum(float(ce_terms(u["samples"], u["labels"], focal).sum()) for u in units)
    gi = sum(float(giou_terms(u["pred"], u["gt"]).sum()) for u in units)
    return ce / n, gi / n


# ---------------------------------------------------------------- fixtures
def load_cases(z):
    """The cases of tests/golden/evalloss.npz (a dict of its arrays) as dicts:
    meta fields, boxes (list per image), exemplars [B,4], pads [L,B,2], loss
    [2] and per level o, reg, gt_map, pred_obj, pred_reg, gt_obj, gt_reg."""
    import json

    meta = json.loads(bytes(z["meta"]).decode())
    out = []
    for ci, m in enumerate(meta):
        k = f"c{ci}_"
        c = dict(m, index=ci, exemplars=z[k + "exemplars"], pads=z[k + "pads"], loss=z[k + "loss"],
                 boxes=[z[k + f"boxes{b}"] for b in range(m["B"])], lv=[])
        for lv in range(len(m["levels"])):
            c["lv"].append({n: z[k + f"l{lv}_{n}"] for n in
                            ("o", "reg", "gt_map", "pred_obj", "pred_reg", "gt_obj", "gt_reg")})
        out.append(c)
    return out


def case_mode(c) -> int:
    return 2 if c["a"] else (1 if c["c"] else 0)


def case_scales(c):
    """Clamped exemplar (w, h) per image, or (1, 1) under ablation b (fp32)."""
    e = np.asarray(c["exemplars"], f32)
    cl = np.where(e > f32(0), e, f32(0)).astype(f32)
    cl = np.where(cl < f32(1), cl, f32(1)).astype(f32)
    sw, sh = (cl[:, 2] - cl[:, 0]).astype(f32), (cl[:, 3] - cl[:, 1]).astype(f32)
    if c["b"]:
        sw, sh = np.ones_like(sw), np.ones_like(sh)
    return sw, sh


def case_level(c, lv: int, expf, pads=None):
    """The restatement of level lv of a fixture case: the list of its units
    (image b with exemplar b), with the recorded pads unless `pads` [B,2]."""
    H, W = c["levels"][lv]
    last = lv == len(c["levels"]) - 1
    sw, sh = case_scales(c)
    pads = c["pads"][lv] if pads is None else pads
    L = c["lv"][lv]
    units = []
    for b in range(c["B"]):
        cls = classify_image(c["boxes"][b], H, W, c["pt"], c["nt"], last)
        units.append(unit(L["o"][b, 0], L["reg"][b], c["boxes"][b], cls, H, W, int(pads[b][0]), int(pads[b][1]),
                          sw[b], sh[b], case_mode(c), expf))
    return units
