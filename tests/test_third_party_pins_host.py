"""The CPU oracle's RoIAlign and NMS against definitions the project did not
write (tests/roi_align_ref.py, tests/nms_ref.py).  No GPU.

torchvision is absent, so oracle.roi_align / oracle.nms are transcriptions by
the same hand as the kernels they check.  These tests pin them to the
operations' definitions instead: RoIAlign in float64 on ATen's grid_sample and
in closed form on linear ramps, NMS as the float64 greedy rule.

Bounds: 1e-5 normwise, the project's fp32 contract (measured: 6.2e-7 against
the definition on smooth features, 1.6e-7 on ramps); NMS keep lists equal.
Cases on which fp32 and float64 may legitimately take another branch (a grid
quotient within 1e-6 of an integer, an IoU within 1e-5 of the threshold) are
skipped and counted against a cap.

Each check takes the function under test as an argument, so a mutated build of
the oracle can be run through the same code.
"""
import numpy as np

import nms_ref
import oracle
import roi_align_ref as rr

TOL = 1e-5
ROI_SKIP_CAP = 0.10
NMS_SKIP_CAP = 0.05
NMS_SETS = 240
NMS_THRS = (0.15, 0.3, 0.5, 0.7)


def check_roi_align_definition(roi_align, cases=rr.CASES, verbose=True):
    """roi_align(f, roi, PH, PW) vs roi_align_f64 over the shared case list."""
    feats = {}
    worst, skipped, grids = 0.0, 0, set()
    for m, H, W, box in cases:
        roi, ph, pw = rr.template_size(box, H, W)
        o_roi, o_ph, o_pw = oracle.template_size(box, H, W)
        assert (ph, pw) == (o_ph, o_pw) and np.array_equal(roi, o_roi)
        gh, gw, amb = rr.grid_counts(roi, ph, pw)
        if amb:
            skipped += 1
            continue
        if m not in feats:
            feats[m] = rr.case_features(m, H, W)
        err = rr.normwise(roi_align(feats[m], roi, ph, pw), rr.roi_align_f64(feats[m], roi, ph, pw))
        assert err <= TOL, (m, H, W, box.tolist(), (gh, gw), err)
        worst = max(worst, err)
        grids.add((gh, gw))
    if verbose:
        print(f"roi_align vs float64 definition: worst normwise {worst:.3g} over "
              f"{len(cases) - skipped} cases, {skipped} of {len(cases)} ambiguous skipped, "
              f"grids {sorted(grids)}")
    assert {(1, 1), (1, 2), (2, 1), (2, 2)} <= grids, sorted(grids)
    assert skipped <= ROI_SKIP_CAP * len(cases), (skipped, len(cases))
    return worst


def check_roi_align_ramp(roi_align, cases=rr.CASES, verbose=True):
    """roi_align vs the closed form on linear ramps, interior rois only."""
    worst, n = 0.0, 0
    ramps = {}
    for m, H, W, box in cases:
        roi, ph, pw = rr.template_size(box, H, W)
        if not rr.is_interior(roi, H, W):
            continue
        if m not in ramps:
            coef = rr.ramp_coefficients(m, rr.CHANNELS)
            ramps[m] = (coef, rr.ramp(coef, H, W))
        coef, f = ramps[m]
        err = rr.normwise(roi_align(f, roi, ph, pw), rr.ramp_expected(coef, roi, ph, pw), np.abs(f).max())
        assert err <= TOL, (m, H, W, box.tolist(), err)
        worst = max(worst, err)
        n += 1
    if verbose:
        print(f"roi_align vs closed form on ramps: worst normwise {worst:.3g} over {n} interior cases")
    assert n >= 50, n  # the interior subset must not dwindle away
    return worst


def check_roi_align_outside(roi_align, verbose=True):
    """Rois hanging off the map: samples outside [-1,H] x [-1,W] count as zero."""
    worst = 0.0
    for i, (H, W, roi, ph, pw) in enumerate(rr.OUTSIDE):
        roi = np.asarray(roi, np.float32)
        assert not rr.grid_counts(roi, ph, pw)[2]
        f = rr.smooth_features(900 + i, rr.CHANNELS, H, W) + np.float32(3.0)  # away from 0
        ref, zeroed = rr.roi_align_f64(f, roi, ph, pw, return_zeroed=True)
        assert zeroed > 0, (i, "no sample outside the map: the case is stale")
        err = rr.normwise(roi_align(f, roi, ph, pw), ref)
        assert err <= TOL, (i, roi.tolist(), err)
        worst = max(worst, err)
        if verbose:
            print(f"outside roi {i}: {zeroed} samples zeroed, normwise {err:.3g}")
    return worst


def nms_sets():
    """(seed, n, thr) of the seeded sets: n covers 1 .. 400."""
    r = np.random.default_rng(7)
    ns = [1, 2, 3, 400] + [int(v) for v in r.integers(1, 401, NMS_SETS - 4)]
    return [(5000 + i, n, NMS_THRS[i % 4]) for i, n in enumerate(ns)]


def check_nms(nms, verbose=True):
    sets = nms_sets()
    assert len(sets) >= 200
    skipped = suppressed = 0
    for seed, n, thr in sets:
        boxes, scores = nms_ref.random_set(seed, n)
        want, amb = nms_ref.greedy_f64(boxes, scores, thr)
        if amb:
            skipped += 1
            continue
        got = np.asarray(nms(boxes, scores, thr))
        assert np.array_equal(got, want), (seed, n, thr)
        suppressed += n - want.size
    if verbose:
        print(f"nms vs float64 greedy: 0 mismatches over {len(sets) - skipped} sets, "
              f"{skipped} of {len(sets)} ambiguous skipped, {suppressed} boxes suppressed")
    assert suppressed > 0
    assert skipped <= NMS_SKIP_CAP * len(sets), (skipped, len(sets))


def test_oracle_roi_align_vs_definition():
    check_roi_align_definition(oracle.roi_align)


def test_oracle_roi_align_vs_ramp():
    check_roi_align_ramp(oracle.roi_align)


def test_oracle_roi_align_outside_the_map():
    check_roi_align_outside(oracle.roi_align)


def test_oracle_nms_vs_greedy_f64():
    check_nms(oracle.nms)
