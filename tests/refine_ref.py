"""TEST HELPER: a numpy restatement of tmr_mask_boxes, written from the
statement in include/tmr_refine.h (the interpolation rule and both
epilogues), not from the kernel and not from the reference's text.

Every operation is fp32 and separately rounded (numpy float32 arrays, one
operation per expression node).  The GPU tests compare the kernel against
this file exactly; tests/test_refine_host.py pins it to
tests/golden/refine.npz (the reference's own refiner) on the CPU.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def _axis(n_in: int, n_out: int):
    """Source index pair and weights of one axis: (i0, i1, lo, hi)."""
    s = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0.0)
    r = s * np.arange(n_out, dtype=f32)
    i0 = r.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    lo = r - i0.astype(f32)
    hi = f32(1.0) - lo
    return i0, i1, lo, hi


def upsample(mask, size):
    """The [H,W] fp32 values v of one [h,w] mask under the header's rule."""
    m = np.asarray(mask, f32)
    h, w = m.shape
    H, W = size
    y0, y1, ly, hy = _axis(h, H)
    x0, x1, lx, hx = _axis(w, W)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = m[y0][:, x0], m[y0][:, x1]
        c, d = m[y1][:, x0], m[y1][:, x1]
        top = hx[None, :] * a + lx[None, :] * b
        bot = hx[None, :] * c + lx[None, :] * d
        return hy[:, None] * top + ly[:, None] * bot


def upsample_contracted(mask, size):
    """upsample with each `p * a + q * b` of the rule evaluated as ONE fused
    multiply-add, fl32(p * a + fl32(q * b)) with the first product exact
    (float64 holds the product of two fp32 values exactly, and its sum with an
    fp32 value is rounded to fp32 once for all but double-rounding ties): what
    a build that lost -ffp-contract=off would compute.  NOT the rule: the
    host test counts the ramp masks whose box tells the two apart."""
    m = np.asarray(mask, f32)
    h, w = m.shape
    H, W = size
    y0, y1, ly, hy = _axis(h, H)
    x0, x1, lx, hx = _axis(w, W)
    f64 = np.float64

    def fma(p, a, q, b):
        return (p.astype(f64) * a.astype(f64) + (q * b).astype(f32).astype(f64)).astype(f32)

    with np.errstate(invalid="ignore", over="ignore"):
        a, b = m[y0][:, x0], m[y0][:, x1]
        c, d = m[y1][:, x0], m[y1][:, x1]
        top = fma(hx[None, :], a, lx[None, :], b)
        bot = fma(hx[None, :], c, lx[None, :], d)
        return fma(hy[:, None], top, ly[:, None], bot)


def int_boxes(masks, size, value_fn=None):
    """[N,4] int64 (min X, min Y, max X, max Y) of v > 0; zeros when empty.
    value_fn(mask, size) gives v (default: upsample, the rule)."""
    value_fn = value_fn or upsample
    masks = np.asarray(masks, f32)
    if masks.ndim == 4:
        masks = masks[:, 0]
    out = np.zeros((masks.shape[0], 4), np.int64)
    for n, m in enumerate(masks):
        ys, xs = np.nonzero(value_fn(m, size) > 0)
        if ys.size:
            out[n] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def mask_boxes(masks, size, logits, iou, scaler=None):
    """-> (logits_out [N,2], boxes [N,4], refs [N,2]) fp32."""
    H, W = size
    ib = int_boxes(masks, size)
    logits = np.asarray(logits, f32).reshape(-1, 2)
    iou = np.asarray(iou, f32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        box = ib.astype(f32) / np.array([W, H, W, H], f32)
        if scaler is not None:
            s = np.asarray(scaler, f32).reshape(4)
            cx, cy = (box[:, 0] + box[:, 2]) / f32(2), (box[:, 1] + box[:, 3]) / f32(2)
            l, t = (cx - box[:, 0]) * s[0], (cy - box[:, 1]) * s[1]
            r, b = (box[:, 2] - cx) * s[2], (box[:, 3] - cy) * s[3]
            box = np.stack([cx - l, cy - t, cx + r, cy + b], axis=-1)
        refs = np.stack([(box[:, 0] + box[:, 2]) / f32(2), (box[:, 1] + box[:, 3]) / f32(2)], axis=-1)
        lout = np.stack([iou * logits[:, 0], f32(0.0) * logits[:, 1]], axis=-1)
    return lout.astype(f32), box.astype(f32), refs.astype(f32)


def exemplar_scaler(mask, size, exemplar):
    """forward_refine's scaler [4] from the exemplar's own mask [h,w] and its
    box (x1, y1, x2, y2); None when the mask has no positive pixel."""
    H, W = size
    m = np.asarray(mask, f32).reshape(1, *np.asarray(mask).shape[-2:])
    if not (upsample(m[0], size) > 0).any():
        return None
    box = int_boxes(m, size).astype(f32) / np.array([W, H, W, H], f32)
    x1, y1, x2, y2 = (f32(v) for v in np.asarray(exemplar, f32).reshape(4))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cx, cy = (box[:, 0] + box[:, 2]) / f32(2), (box[:, 1] + box[:, 3]) / f32(2)
        l, t, r, b = cx - box[:, 0], cy - box[:, 1], box[:, 2] - cx, box[:, 3] - cy
        return np.concatenate([(cx - x1) / l, (cy - y1) / t, (x2 - cx) / r, (y2 - cy) / b]).astype(f32)


def blob_masks(rng, N: int, h: int, w: int):
    """N seeded mask-logit planes [N,h,w]: one or two Gaussian blobs above a
    negative floor plus a little noise (the shape of a SAM mask: a positive
    region with a smooth zero crossing)."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((N, h, w), f32)
    for n in range(N):
        m = np.full((h, w), -rng.uniform(1.0, 4.0))
        for _ in range(int(rng.integers(1, 3))):
            cy, cx = rng.uniform(0, max(h - 1, 1e-3)), rng.uniform(0, max(w - 1, 1e-3))
            sy, sx = rng.uniform(0.08, 0.3) * max(h, 2), rng.uniform(0.08, 0.3) * max(w, 2)
            m += rng.uniform(5.0, 12.0) * np.exp(-((ys - cy) ** 2 / (2 * sy * sy) + (xs - cx) ** 2 / (2 * sx * sx)))
        out[n] = (m + 0.05 * rng.standard_normal((h, w))).astype(f32)
    return out


def ramp_masks(h: int, w: int, H: int, W: int, x_stride: int = 1):
    """Masks whose box rests on the last bits of v: for an output column X
    (1 .. W-2, every x_stride-th) the plane m[y][x] = fl32(x) - c with
    c = sx * fl32(X), sx = fl32(w-1) / fl32(W-1) as the rule computes it, and
    its negation; likewise m[y][x] = fl32(y) - sy * fl32(Y) for every output
    row Y in 1 .. H-2.  In exact arithmetic the interpolated value at column X
    (row Y) is zero, so its sign -- whether that column belongs to the box --
    is the rounding of the rule's own operation order: a fused multiply-add, a
    reordered sum or a weight computed another way moves the box.  [N,h,w]."""
    sx = f32(w - 1) / f32(W - 1) if W > 1 else f32(0.0)
    sy = f32(h - 1) / f32(H - 1) if H > 1 else f32(0.0)
    xs = np.broadcast_to(np.arange(w, dtype=f32)[None, :], (h, w))
    ys = np.broadcast_to(np.arange(h, dtype=f32)[:, None], (h, w))
    out = []
    for X in range(1, W - 1, x_stride):
        m = xs - sx * f32(X)
        out += [m, -m]
    for Y in range(1, H - 1):
        m = ys - sy * f32(Y)
        out += [m, -m]
    return np.stack(out).astype(f32)


# the ramp shapes of the refiner tests: (h, w, H, W), x_stride.  The last three
# stage reduced bands (tmr_mask_boxes_plan): 11 rows with the staged rows at
# their cap, 12 rows, and 1 row at the widest mask the kernel takes.
RAMP_SHAPES = [((16, 16, 64, 64), 1), ((7, 11, 23, 37), 1), ((30, 700, 37, 900), 8), ((200, 100, 30, 45), 1),
               ((3, 4096, 7, 50), 1)]


def margin_ok(masks, size, value_fn=None) -> bool:
    """The fixtures' condition: for every mask the box of {v > +eps} equals
    the box of {v > -eps}, eps = 1e-5 * max|mask| -- no box rests on the last
    bits of v.  value_fn(mask, size) gives v (default: upsample)."""
    value_fn = value_fn or upsample
    masks = np.asarray(masks, f32)
    if masks.ndim == 4:
        masks = masks[:, 0]
    for m in masks:
        v = np.asarray(value_fn(m, size), np.float64)
        eps = 1e-5 * float(np.abs(m).max())
        boxes = []
        for thr in (eps, -eps):
            ys, xs = np.nonzero(v > thr)
            boxes.append((xs.min(), ys.min(), xs.max(), ys.max()) if ys.size else None)
        if boxes[0] != boxes[1]:
            return False
    return True
