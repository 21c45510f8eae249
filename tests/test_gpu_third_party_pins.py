"""GPU: the RoIAlign / prototype kernels (tmr_templates) and the NMS kernels
against definitions the project did not write (tests/roi_align_ref.py,
tests/nms_ref.py), next to the bit-exact comparison with the CPU oracle.

Bounds: RoIAlign bit-equal to oracle.roi_align and <= 1e-5 normwise (the fp32
contract) from the float64 definition and from the closed form on ramps;
prototype <= 1e-6 normwise from the float64 mean (the kernel accumulates in
double and rounds once: 6e-8 relative, and cancellation in a mean of smooth
features of mixed sign stays far below 16x); NMS keep lists equal.

Every shape is the smallest that reaches its path: both sides of the LDS
sample cache limit, a launch of several units of both template types with one
and with two channel groups, rois that hang off the map, and the NMS sizes on
either side of the one-workgroup limit.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import nms_ref
import oracle
import roi_align_ref as rr
import tmr_amd
from tmr_amd._lib import UNIT_DTYPE, call, ptr, stream
from tmr_amd.graphs import _units_to_device

pytestmark = pytest.mark.gpu

TOL = 1e-5
PROTO_TOL = 1e-6
DEV = torch.device("cuda:0")
MAX_SAMPLES = 1536  # csrc/templates.hip
SENTINEL = np.float32(-12345.678)


def cuda(x):
    return torch.as_tensor(x).to(DEV)


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _features(m, H, W):
    f = rr.case_features(m, H, W)
    f.setflags(write=False)
    return f


def _check_roi_align(got, f, roi, ph, pw, what):
    """bit-equal to the oracle; within TOL of the definition unless ambiguous.
    Returns the normwise error against the definition (None when skipped)."""
    assert got.shape == (f.shape[0], ph, pw), what
    assert bits_equal(got, oracle.roi_align(f, roi, ph, pw)), what
    if rr.grid_counts(roi, ph, pw)[2]:
        return None
    err = rr.normwise(got, rr.roi_align_f64(f, roi, ph, pw))
    assert err <= TOL, (what, err)
    return err


# ------------------------------------------------------- extract_template
def test_extract_template_vs_definition():
    """TemplateMatching("roi_align").extract_template over the shared case
    list, maps <= 64x64, C = 8."""
    m = tmr_amd.TemplateMatching("roi_align").to(DEV)
    cases = [c for c in rr.CASES if c[1] <= 64 and c[2] <= 64]
    dev = {}
    worst, skipped, grids = 0.0, 0, set()
    for mi, H, W, box in cases:
        f = _features(mi, H, W)
        if mi not in dev:
            dev[mi] = cuda(f[None].copy())  # the cached map stays read-only
        roi, ph, pw = rr.template_size(box, H, W)
        got = m.extract_template(dev[mi], torch.from_numpy(box)).cpu().numpy()[0]
        err = _check_roi_align(got, f, roi, ph, pw, (mi, H, W, box.tolist()))
        if err is None:
            skipped += 1
        else:
            worst = max(worst, err)
            grids.add(rr.grid_counts(roi, ph, pw)[:2])
    print(f"extract_template vs float64 definition: worst normwise {worst:.3g} over "
          f"{len(cases) - skipped} cases, {skipped} of {len(cases)} ambiguous skipped, grids {sorted(grids)}")
    assert {(1, 1), (1, 2), (2, 1), (2, 2)} <= grids
    assert skipped <= 0.10 * len(cases)


def test_extract_template_vs_ramp():
    """The closed form on linear ramps, interior rois of the same list."""
    m = tmr_amd.TemplateMatching("roi_align").to(DEV)
    ramps = {}
    worst, n = 0.0, 0
    for mi, H, W, box in rr.CASES:
        roi, ph, pw = rr.template_size(box, H, W)
        if H > 64 or W > 64 or not rr.is_interior(roi, H, W):
            continue
        if mi not in ramps:
            coef = rr.ramp_coefficients(mi, rr.CHANNELS)
            f = rr.ramp(coef, H, W)
            ramps[mi] = (coef, f, cuda(f[None]))
        coef, f, fd = ramps[mi]
        got = m.extract_template(fd, torch.from_numpy(box)).cpu().numpy()[0]
        err = rr.normwise(got, rr.ramp_expected(coef, roi, ph, pw), np.abs(f).max())
        assert err <= TOL, (mi, H, W, box.tolist(), err)
        worst = max(worst, err)
        n += 1
    print(f"extract_template vs closed form on ramps: worst normwise {worst:.3g} over {n} interior cases")
    assert n >= 50, n


# (box in pixels of the 64x64 map (x1,y1,x2,y2), (PH,PW), (gh,gw), cached)
STAGING = [
    ((3.25, 5.25, 41.75, 43.75), (39, 39), (1, 1), True),    # 1521 samples
    ((3.25, 5.25, 41.75, 45.75), (41, 39), (1, 1), False),   # 1599
    ((8.0, 6.0, 28.0, 26.0), (19, 19), (2, 2), True),        # 4 * 361 = 1444
    ((8.0, 6.0, 28.0, 28.0), (21, 19), (2, 2), False),       # 4 * 399 = 1596
]


@pytest.mark.parametrize("px,size,grid,cached", STAGING)
def test_roi_align_staging_limit(px, size, grid, cached):
    """One template on each side of the kernel's LDS sample cache limit
    (gh*gw*PH*PW <= MAX_SAMPLES), with one and with four samples per bin."""
    src = os.path.join(os.path.dirname(tmr_amd.__file__), "csrc", "templates.hip")
    with open(src) as fh:
        limit = int(re.search(r"constexpr int MAX_SAMPLES = (\d+);", fh.read()).group(1))
    assert limit == MAX_SAMPLES, "the staging limit moved: STAGING no longer straddles it"
    H = W = 64
    box = (np.array(px, np.float64) / 64).astype(np.float32)  # exact: x / 64 * 64 == x
    roi, ph, pw = rr.template_size(box, H, W)
    gh, gw, amb = rr.grid_counts(roi, ph, pw)
    assert (ph, pw) == size and (gh, gw) == grid and not amb
    assert (gh * gw * ph * pw <= limit) == cached
    f = _features(rr.MAPS.index((H, W)), H, W)
    assert f.shape == (rr.CHANNELS, H, W)
    m = tmr_amd.TemplateMatching("roi_align").to(DEV)
    got = m.extract_template(cuda(f[None].copy()), torch.from_numpy(box)).cpu().numpy()[0]
    err = _check_roi_align(got, f, roi, ph, pw, (px, size))
    print(f"staging {size} grid {grid} cached={cached}: normwise {err:.3g}")


# ------------------------------------------------------- direct launches
def _launch(f, units, total, B):
    """tmr_templates over hand-built units into a sentinel-filled buffer."""
    _, C, H, W = f.shape
    t = torch.full((total,), float(SENTINEL), device=DEV, dtype=torch.float32)
    fd, ud = cuda(f), _units_to_device(units, DEV)
    call("tmr_templates", ptr(fd), B, C, H, W, ptr(ud), len(units), int(units["ht"].max()),
         int(units["wt"].max()), ptr(t), stream())
    torch.cuda.synchronize()
    return t.cpu().numpy()


# (image, type, box): sorted by image, the two template types interleaved;
# a clamped box, an even pixel-aligned one (grid 2x2) and plain ones
MULTI = [
    (0, "roi_align", (0.12, 0.20, 0.47, 0.61)),
    (0, "prototype", (0.30, 0.10, 0.80, 0.55)),
    (0, "roi_align", (8 / 32, 2 / 16, 16 / 32, 8 / 16)),
    (1, "prototype", (-0.05, 0.40, 0.33, 1.20)),
    (1, "roi_align", (0.55, -0.10, 1.05, 0.37)),
]


@pytest.mark.parametrize("C", [20, 5])
def test_templates_mixed_units_one_launch(C):
    """B = 2 images, U = 5 units of both types and of different sizes in one
    tmr_templates launch.  C = 20: two channel groups per unit, split at 10;
    C = 5: C / 8 == 0, the kernel must fall back to one group.  Nothing
    outside the units' ranges may be written."""
    B, H, W = 2, 16, 32
    f = np.stack([rr.smooth_features(300 + b, C, H, W) for b in range(B)])
    units = np.zeros(len(MULTI), UNIT_DTYPE)
    off, spans = 7, []  # gaps before, between and after the units hold the sentinel
    for u, (img, ttype, box) in enumerate(MULTI):
        box = np.array(box, np.float32)
        if ttype == "roi_align":
            roi, ht, wt = rr.template_size(box, H, W)
            units[u] = (img, 0, ht, wt, tuple(roi.tolist()), (0, 0, 0, 0), off, 0, 0)
        else:
            pbox = oracle.prototype_box(box, H, W)
            ht = wt = 1
            units[u] = (img, 1, 1, 1, (0.0, 0.0, 0.0, 0.0), tuple(pbox.tolist()), off, 0, 0)
        spans.append((off, off + C * ht * wt))
        off += C * ht * wt + 3
    total = off + 8
    assert len({s[1] - s[0] for s in spans}) >= 4, "templates of different sizes"
    out = _launch(f, units, total, B)

    touched = np.zeros(total, bool)
    for u, (img, ttype, box) in enumerate(MULTI):
        a, b = spans[u]
        touched[a:b] = True
        if ttype == "roi_align":
            ht, wt = int(units["ht"][u]), int(units["wt"][u])
            err = _check_roi_align(out[a:b].reshape(C, ht, wt), f[img], units["roi"][u], ht, wt, (C, u))
            assert err is not None, (u, "ambiguous grid: pick another box")
        else:
            x1, y1, x2, y2 = units["pbox"][u].tolist()
            want = f[img][:, y1:y2, x1:x2].astype(np.float64).mean(axis=(1, 2))
            err = rr.normwise(out[a:b], want)
            assert err <= PROTO_TOL, (C, u, err)
        print(f"C={C} unit {u} ({ttype}, image {img}): normwise {err:.3g}")
    assert rr.grid_counts(units["roi"][2], int(units["ht"][2]), int(units["wt"][2]))[:2] == (2, 2)
    rest = out[~touched]
    assert np.array_equal(rest.view(np.uint32), np.full(rest.shape, SENTINEL).view(np.uint32)), \
        "a float outside the units' template ranges changed"


@pytest.mark.parametrize("i", range(len(rr.OUTSIDE)))
def test_roi_align_outside_the_map(i):
    """Rois hanging off the map through the ABI, with a hand-built tmr_unit_t
    (no box clamp before them): the samples outside [-1,H] x [-1,W] are zero."""
    H, W, roi, ph, pw = rr.OUTSIDE[i]
    roi = np.asarray(roi, np.float32)
    f = rr.smooth_features(900 + i, rr.CHANNELS, H, W) + np.float32(3.0)
    _, zeroed = rr.roi_align_f64(f, roi, ph, pw, return_zeroed=True)
    assert zeroed > 0
    units = np.zeros(1, UNIT_DTYPE)
    units[0] = (0, 0, ph, pw, tuple(roi.tolist()), (0, 0, 0, 0), 5, 0, 0)
    n = rr.CHANNELS * ph * pw
    out = _launch(f[None], units, n + 10, 1)
    err = _check_roi_align(out[5:5 + n].reshape(rr.CHANNELS, ph, pw), f, roi, ph, pw, i)
    assert err is not None
    assert (out[:5] == SENTINEL).all() and (out[5 + n:] == SENTINEL).all()
    print(f"outside roi {i}: {zeroed} samples zeroed, normwise {err:.3g}")


# ------------------------------------------------------------------- nms
@pytest.mark.parametrize("n", [200, 257, 1500])
def test_nms_vs_greedy_f64(n):
    """n = 200: the one-workgroup kernel; 257: the first size on the sorted /
    binned path; 1500.  Tie-free scores; keep lists equal the float64 greedy
    rule's.  A set with an IoU within 1e-5 of the threshold is replaced by the
    next seed, at most once per size."""
    replaced = 0
    for thr in (0.15, 0.5):
        seed = 7002 + n
        boxes, scores = nms_ref.random_set(seed, n)
        want, amb = nms_ref.greedy_f64(boxes, scores, thr)
        if amb:
            replaced += 1
            boxes, scores = nms_ref.random_set(seed + 1, n)
            want, amb = nms_ref.greedy_f64(boxes, scores, thr)
        assert not amb and replaced <= 1, (n, thr, replaced)
        assert 0 < want.size < n
        logits = np.stack([scores, np.zeros_like(scores)], 1)
        keep = tmr_amd.NMS_process(cuda(boxes), cuda(logits), thr).cpu().numpy()
        assert np.array_equal(keep, want), (n, thr)
        print(f"nms n={n} thr={thr}: {want.size} kept, equal; {replaced} replaced")
