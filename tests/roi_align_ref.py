"""TEST HELPER: RoIAlign from its definition, in float64, on ATen's sampler.

torchvision is not installed, so oracle/tmr_oracle.c: orc_roi_align and
csrc/templates.hip: roi_align_kernel are this project's own reading of its CPU
kernel.  What is written here is not a third reading of that code: it is the
operation's definition,

    roi_align(f, roi, (PH, PW), spatial_scale=1, sampling_ratio=-1, aligned=True)

a (PH, PW) grid of bins of size (y2-y1)/PH x (x2-x1)/PW, each the mean of a
gh x gw grid of bilinear samples at

    start - 0.5 + p * bin + (i + 0.5) * bin / g,   g = ceil(roi_size / P),

evaluated in float64 with torch.nn.functional.grid_sample (bilinear, border
padding, align_corners=True) as the sampler.  ATen's sampler is the
independent part: border padding equals torchvision's clamp for samples in
[-1, H] x [-1, W], and the samples outside that range count as zero.

The second, sampler-free check is ramp_expected(): on f = a*x + b*y + d
bilinear sampling is exact and a bin's symmetric samples average to its centre.
It sees a wrong offset or bin size, and by construction not a wrong grid count.

tests/test_third_party_pins_host.py (oracle) and
tests/test_gpu_third_party_pins.py (kernel) share the case list below.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

AMBIGUOUS_REL = 1e-6  # a grid quotient this close to an integer may ceil differently in fp32


def _roi64(roi):
    return np.asarray(roi, np.float32).reshape(4).astype(np.float64)


def grid_counts(roi, PH, PW):
    """(gh, gw, ambiguous): the adaptive sampling grid of one bin, from the
    fp32 roi in float64.  ambiguous: a quotient lies within AMBIGUOUS_REL
    (relative) of an integer, so an fp32 evaluation may take the other ceil."""
    x1, y1, x2, y2 = _roi64(roi)
    qh, qw = (y2 - y1) / PH, (x2 - x1) / PW
    amb = any(abs(q - round(q)) <= AMBIGUOUS_REL * max(abs(q), 1.0) for q in (qh, qw))
    return int(math.ceil(qh)), int(math.ceil(qw)), amb


def roi_align_f64(f, roi, PH, PW, return_zeroed=False):
    """float64 [C,PH,PW] of f[C,H,W] (fp32) over roi[4] (fp32 feature px).
    return_zeroed: also the number of sample points outside [-1,H] x [-1,W]."""
    f = torch.from_numpy(np.asarray(f, np.float32).astype(np.float64))  # a copy: the map may be read-only
    C, H, W = f.shape
    assert H >= 2 and W >= 2, "align_corners coordinates need a 2x2 map"
    x1, y1, x2, y2 = _roi64(roi)
    gh, gw, _ = grid_counts(roi, PH, PW)
    if gh <= 0 or gw <= 0:  # an empty grid: the mean over max(0, 1) of nothing
        out = np.zeros((C, PH, PW), np.float64)
        return (out, 0) if return_zeroed else out
    bh, bw = (y2 - y1) / PH, (x2 - x1) / PW
    ys = (y1 - 0.5 + np.arange(PH)[:, None] * bh + (np.arange(gh)[None, :] + 0.5) * bh / gh).reshape(-1)
    xs = (x1 - 0.5 + np.arange(PW)[:, None] * bw + (np.arange(gw)[None, :] + 0.5) * bw / gw).reshape(-1)
    inside = ((ys >= -1.0) & (ys <= H))[:, None] & ((xs >= -1.0) & (xs <= W))[None, :]
    gx = np.broadcast_to((2.0 * xs / (W - 1) - 1.0)[None, :], inside.shape)
    gy = np.broadcast_to((2.0 * ys / (H - 1) - 1.0)[:, None], inside.shape)
    grid = torch.from_numpy(np.stack([gx, gy], -1)[None].copy())
    s = F.grid_sample(f[None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
    s = s * torch.from_numpy(inside.astype(np.float64))
    out = (s.reshape(C, PH, gh, PW, gw).sum(dim=(2, 4)) / max(gh * gw, 1)).numpy()
    return (out, int((~inside).sum())) if return_zeroed else out


def ramp(coef, H, W):
    """f[c,y,x] = a_c*x + b_c*y + d_c as fp32 (exact for multiples of 1/64)."""
    coef = np.asarray(coef, np.float64).reshape(-1, 3)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = coef[:, 0, None, None] * x + coef[:, 1, None, None] * y + coef[:, 2, None, None]
    f32 = f.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), f), "ramp not exact in fp32"
    return f32


def ramp_coefficients(seed, C):
    """[C,3] multiples of 1/64 in [-2, 2]."""
    r = np.random.default_rng(seed)
    return r.integers(-128, 129, size=(C, 3)).astype(np.float64) / 64.0


def is_interior(roi, H, W):
    """No sample of the roi clamps: 1 <= x1, x2 <= W-1, 1 <= y1, y2 <= H-1."""
    x1, y1, x2, y2 = _roi64(roi)
    return 1.0 <= x1 and x2 <= W - 1 and 1.0 <= y1 and y2 <= H - 1


def ramp_expected(coef, roi, PH, PW):
    """float64 [C,PH,PW]: the ramp at each bin's centre, whatever the grid.
    Holds only for is_interior() rois."""
    coef = np.asarray(coef, np.float64).reshape(-1, 3)
    x1, y1, x2, y2 = _roi64(roi)
    bh, bw = (y2 - y1) / PH, (x2 - x1) / PW
    cy = (y1 - 0.5 + (np.arange(PH) + 0.5) * bh)[None, :, None]
    cx = (x1 - 0.5 + (np.arange(PW) + 0.5) * bw)[None, None, :]
    return coef[:, 0, None, None] * cx + coef[:, 1, None, None] * cy + coef[:, 2, None, None]


def smooth_features(seed, C, H, W):
    """fp32 [C,H,W]: three sinusoids of at most 1.5 periods across the map, an
    x*y term and a constant per channel.  Smooth on purpose: the fp32 sample
    coordinates of the code under test carry ~1e-7 relative error, which a
    steep gradient (white noise) multiplies to within reach of the 1e-5 bound."""
    r = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = u / (W - 1), v / (H - 1)
    f = np.zeros((C, H, W), np.float64)
    for c in range(C):
        for _ in range(3):
            amp, ku, kv, ph = r.uniform(0.3, 1.0), r.uniform(-1.5, 1.5), r.uniform(-1.5, 1.5), r.uniform(0, 2 * np.pi)
            f[c] += amp * np.sin(2 * np.pi * (ku * u + kv * v) + ph)
        f[c] += r.uniform(-1.0, 1.0) * u * v + r.uniform(-1.0, 1.0)
    return f.astype(np.float32)


# ---------------------------------------------------------------- case list
MAPS = [(2, 2), (3, 4), (4, 4), (6, 9), (20, 13), (5, 7), (7, 6), (8, 8), (9, 16), (12, 16), (16, 16),
        (17, 31), (24, 40), (32, 32), (33, 64), (48, 48), (64, 64), (100, 75), (129, 129)]
BOXES_PER_MAP = 31
CHANNELS = 8


def template_size(box, H, W):
    """models/template_matching.py:56-73 (the reference's own Python, pinned by
    the `template` golden): clamp to [0,1], scale in fp32, odd ceil-floor size.
    -> (roi fp32[4], PH, PW), or None when the size is not positive."""
    c = np.minimum(np.maximum(np.asarray(box, np.float32), np.float32(0)), np.float32(1))
    x1, x2 = c[0] * np.float32(W), c[2] * np.float32(W)
    y1, y2 = c[1] * np.float32(H), c[3] * np.float32(H)
    pw = int(math.ceil(x2)) - int(math.floor(x1))
    ph = int(math.ceil(y2)) - int(math.floor(y1))
    pw -= pw % 2 == 0
    ph -= ph % 2 == 0
    if ph <= 0 or pw <= 0:
        return None
    return np.array([x1, y1, x2, y2], np.float32), ph, pw


def _aligned_even(r, n):
    """A pixel-aligned span of even length on an n-pixel axis, normalised.
    (A 2-pixel span gives a 1-bin side with quotient exactly 2, which is always
    ambiguous: spans start at 4 pixels where the axis has them.)"""
    length = 2 * int(r.integers(2 if n >= 4 else 1, max(n // 2, 1) + 1))
    start = int(r.integers(0, n - length + 1))
    return start / n, (start + length) / n


def _cases():
    out = []
    k = 0
    for m, (H, W) in enumerate(MAPS):
        r = np.random.default_rng(1000 + m)
        got = 0
        while got < BOXES_PER_MAP:
            x1, y1 = r.uniform(-0.1, 0.8, 2)
            x2 = min(x1 + r.uniform(0.02, 0.6), 1.1)
            y2 = min(y1 + r.uniform(0.02, 0.6), 1.1)
            if k % 5 == 0:
                x1 = 0.0
            if k % 7 == 0:
                x2 = 1.0
            if k % 3 == 0:  # even pixel-aligned sides: the size drops to odd and the grid to 2
                which = (k // 3) % 3  # both axes, x only, y only
                if which in (0, 1):
                    x1, x2 = _aligned_even(r, W)
                if which in (0, 2):
                    y1, y2 = _aligned_even(r, H)
            box = np.array([x1, y1, x2, y2], np.float32)
            if template_size(box, H, W) is None:
                continue  # degenerate after the clamp: the reference rejects it too
            out.append((m, H, W, box))
            got += 1
            k += 1
    return out


CASES = _cases()  # (map index, H, W, box fp32[4] normalised), fixed


def case_features(m, H, W):
    """The smooth map of CASES' map m (every box of a map shares it)."""
    return smooth_features(50 + m, CHANNELS, H, W)


# Rois partly outside the map, handed over as rois (no box clamp before them):
# (H, W, roi, PH, PW).  The first hangs off the top-left, the second off the
# bottom-right, the third has whole rows and columns of bins outside.
OUTSIDE = [
    (12, 16, (-6.0, -3.0, 10.0, 9.0), 7, 9),
    (12, 16, (9.5, 6.25, 22.0, 17.5), 5, 7),
    (9, 11, (-8.0, -7.0, 20.0, 18.5), 5, 5),
]


def normwise(a, b, scale=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.abs(b).max() if scale is None else scale
    return float(np.abs(a - b).max() / max(s, 1e-30))
