"""TEST HELPER: greedy NMS from its definition, in float64.

torchvision is not installed; oracle/tmr_oracle.c: orc_nms and the NMS kernels
are this project's reading of its CPU kernel.  The definition is short: visit
the boxes by descending score and keep a box iff no kept box overlaps it with
IoU > thr.  Here the IoU is float64 and the decision carries a margin: fp32
IoU of fp32 boxes is accurate to about 5e-7 relative (the min / max are exact
and each difference, product, sum and quotient rounds once), so a pair within
1e-5 of the threshold (20x that error) is one on which an fp32 implementation
may legitimately differ; such a set is flagged and the callers skip it.

Tie order and the order of non-finite scores are torchvision implementation
details, not definition: the reference-generated nms / nms_nonfinite fixtures
own them.  The sets made here are tie-free, finite and of positive area.
"""
import numpy as np


def greedy_f64(boxes, scores, thr, margin=1e-5):
    """(keep int64[] in descending-score order, ambiguous)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4).astype(np.float64)
    s = np.asarray(scores, np.float32).reshape(-1)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    order = np.argsort(-s.astype(np.float64), kind="stable")
    keep, ambiguous = [], False
    for i in order:
        if keep:
            k = b[keep]
            w = np.minimum(k[:, 2], b[i, 2]) - np.maximum(k[:, 0], b[i, 0])
            h = np.minimum(k[:, 3], b[i, 3]) - np.maximum(k[:, 1], b[i, 1])
            inter = np.clip(w, 0, None) * np.clip(h, 0, None)
            iou = inter / (area[keep] + area[i] - inter)
            if (np.abs(iou - thr) <= margin).any():
                ambiguous = True
            if (iou > thr).any():
                continue
        keep.append(int(i))
    return np.asarray(keep, np.int64), ambiguous


def random_set(seed, n):
    """(boxes fp32[n,4], scores fp32[n]): centres uniform in the unit square,
    sides 0.02 .. 0.3, scores a permutation of 1..n divided by n (tie-free)."""
    r = np.random.default_rng(seed)
    c = r.uniform(0.0, 1.0, (n, 2))
    half = r.uniform(0.02, 0.3, (n, 2)) / 2
    boxes = np.concatenate([c - half, c + half], 1).astype(np.float32)
    scores = ((r.permutation(n) + 1) / n).astype(np.float32)
    assert np.unique(scores).size == n
    assert ((boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])).all()
    return boxes, scores
