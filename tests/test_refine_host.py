"""CPU-only: the numpy restatement of tmr_mask_boxes (tests/refine_ref.py)
reproduces the reference's own refiner (tests/golden/refine.npz, made by
tools/make_golden_refine.py) exactly; the extension's symbol table matches
include/tmr_refine.h and libtmr.so."""
import ctypes
import os
import re

import numpy as np

import refine_ref
import tmr_amd
from tmr_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    """Exact equality, a NaN equal to a NaN (its sign and payload differ between processors)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def chunks(g, tag):
    """(image, lo, hi, call) of every candidate chunk and {image: call} of the
    exemplar calls, in the order the refiner makes them."""
    step, out, ex, k = int(g["step"]), [], {}, 0
    for i, n in enumerate(g["counts"]):
        if n == 0:
            continue
        if tag == "rfn":
            ex[i] = k
            k += 1
        for lo in range(0, n, step):
            out.append((i, lo, min(lo + step, n), k))
            k += 1
    assert k == int(g[f"{tag}_ncalls"])
    return out, ex


def test_fixture_shape(golden):
    g = golden("refine")
    assert list(g["counts"]) == [7, 1, 4, 0] and int(g["step"]) == 3
    size = tuple(g["image_size"])
    masks = np.concatenate([g[f"fwd_call{k}_masks"] for k in range(int(g["fwd_ncalls"]))])
    v = [refine_ref.upsample(m[0], size) for m in masks]
    assert any((x <= 0).all() for x in v) and any((x > 0).all() for x in v)
    ib = refine_ref.int_boxes(masks, size)
    assert any(tuple(b[:2]) == (0, size[0] - 1) or tuple(b[:2]) == (0, 0) for b in ib)  # a corner blob
    # the condition the generator asserts, under the header's rule as well
    for tag in ("fwd", "rfn"):
        for k in range(int(g[f"{tag}_ncalls"])):
            assert refine_ref.margin_ok(g[f"{tag}_call{k}_masks"], size), (tag, k)
    k = chunks(g, "rfn")[1][1]  # image 1's exemplar mask is one column wide
    assert np.isinf(refine_ref.exemplar_scaler(g[f"rfn_call{k}_masks"][0, 0], size, g["exemplars"][1, 0])).any()


def test_ref_reproduces_reference_forward(golden):
    g = golden("refine")
    size = tuple(g["image_size"])
    res = np.array([size[1], size[0], size[1], size[0]], np.float32)
    ch, _ = chunks(g, "fwd")
    for i, lo, hi, k in ch:
        assert same(g[f"in_boxes{i}"][lo:hi] * res, g[f"fwd_call{k}_boxes"])
        lg, bx, rf = refine_ref.mask_boxes(g[f"fwd_call{k}_masks"], size, g[f"in_logits{i}"][lo:hi],
                                           g[f"fwd_call{k}_iou"])
        assert same(lg, g[f"fwd_logits{i}"][lo:hi]), (i, lo)
        assert same(bx, g[f"fwd_boxes{i}"][lo:hi]), (i, lo)
        assert same(rf, g[f"fwd_refs{i}"][lo:hi]), (i, lo)
    for what in ("logits", "boxes", "refs"):  # the image without candidates passes through
        assert same(g[f"fwd_{what}3"], g[f"in_{what}3"]) and g[f"fwd_{what}3"].shape[0] == 0


def test_ref_reproduces_reference_forward_refine(golden):
    g = golden("refine")
    size = tuple(g["image_size"])
    res = np.array([size[1], size[0], size[1], size[0]], np.float32)
    ch, ex = chunks(g, "rfn")
    scalers = {}
    for i, k in ex.items():
        assert same(g["exemplars"][i] * res, g[f"rfn_call{k}_boxes"])
        scalers[i] = refine_ref.exemplar_scaler(g[f"rfn_call{k}_masks"][0, 0], size, g["exemplars"][i, 0])
    for i, lo, hi, k in ch:
        assert same(g[f"in_boxes{i}"][lo:hi] * res, g[f"rfn_call{k}_boxes"])
        lg, bx, rf = refine_ref.mask_boxes(g[f"rfn_call{k}_masks"], size, g[f"in_logits{i}"][lo:hi],
                                           g[f"rfn_call{k}_iou"], scalers[i])
        assert same(lg, g[f"rfn_logits{i}"][lo:hi]), (i, lo)
        assert same(bx, g[f"rfn_boxes{i}"][lo:hi]), (i, lo)
        assert same(rf, g[f"rfn_refs{i}"][lo:hi]), (i, lo)
    assert np.isnan(g["rfn_refs1"]).any()  # the infinite scaler reaches the results


def test_empty_exemplar_mask_has_no_scaler():
    assert refine_ref.exemplar_scaler(-np.ones((4, 5), np.float32), (9, 11), [0.1, 0.1, 0.5, 0.5]) is None


def test_ramp_masks_tell_a_contracted_build_apart():
    """The condition that makes the GPU comparison on the ramp masks
    meaningful: at each ramp shape at least 10 masks change their integer box
    between the rule (every operation rounded on its own) and the same
    expressions with one fused multiply-add each.  Measured: 123 of 248, 53 of
    112, 111 of 296, 24 of 142, 12 of 106."""
    counts = {(16, 16, 64, 64): 248, (7, 11, 23, 37): 112, (30, 700, 37, 900): 296, (200, 100, 30, 45): 142,
              (3, 4096, 7, 50): 106}
    for shape, stride in refine_ref.RAMP_SHAPES:
        h, w, H, W = shape
        masks = refine_ref.ramp_masks(h, w, H, W, stride)
        assert masks.shape == (counts[shape], h, w) and masks.dtype == np.float32
        assert same(masks[1], -masks[0])
        rule = refine_ref.int_boxes(masks, (H, W))
        fused = refine_ref.int_boxes(masks, (H, W), refine_ref.upsample_contracted)
        changed = int((rule != fused).any(1).sum())
        print(f"ramp masks {shape}: {changed} of {len(masks)} boxes change under contraction")
        assert changed >= 10, (shape, changed)
        assert not refine_ref.margin_ok(masks, (H, W))  # these are the masks the margin filter removes


def test_mask_boxes_plan_no_gpu():
    """tmr_mask_boxes_plan: the band rule on the host (band rows, staged-row cap, bands per mask)."""
    plan = _lib.mask_boxes_plan
    assert plan(h=16, w=16, H=64, W=64) == (16, 512, 4)
    assert plan(h=40, w=300, H=40, W=300) == (16, 27, 3)  # the largest full-height band of the suite: 18 rows staged
    assert plan(h=30, w=700, H=37, W=900) == (11, 11, 4)  # staged rows at their cap
    assert plan(h=200, w=100, H=30, W=45) == (12, 81, 3)
    assert plan(h=3, w=4096, H=7, W=50) == (1, 2, 7)  # the widest mask
    assert plan(h=5, w=2100, H=5, W=2100) == (1, 3, 5)
    assert plan(h=20, w=600, H=20, W=600) == (11, 13, 2)
    L = tmr_amd.load()
    out = [ctypes.c_int32(7) for _ in range(3)]

    def rc(**kw):
        f = dict(N=1, h=4, w=4, H=8, W=8, mode=0)
        f.update(kw)
        return L.tmr_mask_boxes_plan(ctypes.byref(_lib._fill(_lib.MaskBoxesArgs, "tmr_mask_boxes_args_t", f)),
                                     *(ctypes.byref(o) for o in out))

    assert rc(w=4097) == -1 and [o.value for o in out] == [0, 0, 0]
    assert rc() == -1  # null buffers with N > 0, as tmr_mask_boxes
    assert rc(N=0) == 0 and [o.value for o in out] == [16, 2048, 1]
    assert L.tmr_mask_boxes_plan(None, None, None, None) == -1
    try:
        plan(h=0, w=4, H=8, W=8)
    except tmr_amd.TMRError:
        pass
    else:
        raise AssertionError("an invalid shape must raise TMRError")


def header_symbols():
    txt = open(os.path.join(REPO, "include", "tmr_refine.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tmr_[a-z0-9_]+)\s*\(", txt)))


def test_extension_symbols():
    syms = header_symbols()
    assert syms == ["tmr_mask_boxes", "tmr_mask_boxes_plan"]
    assert set(syms) == set(_lib.EXT_SIGNATURES), "ctypes table out of sync with tmr_refine.h"
    assert not set(syms) & set(_lib.SIGNATURES), "the extension stays outside the core ABI table"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    L = tmr_amd.load()
    assert L.tmr_mask_boxes.argtypes is not None and L.tmr_version() == 3
    assert ctypes.sizeof(_lib.MaskBoxesArgs) == 96
    txt = open(os.path.join(REPO, "include", "tmr_refine.h")).read()
    assert "((int64_t)%d * (int64_t)(N))" % _lib.MASK_BOXES_WORK_PER_MASK in txt


def test_invalid_shapes_no_gpu():
    """Shape limits are checked before anything touches the GPU."""
    L = tmr_amd.load()

    def rc(**kw):
        f = dict(N=1, h=4, w=4, H=8, W=8, mode=0)
        f.update(kw)
        return L.tmr_mask_boxes(ctypes.byref(_lib._fill(_lib.MaskBoxesArgs, "tmr_mask_boxes_args_t", f)), None)

    assert rc(N=0) == 0  # a no-op, whatever the pointers
    assert rc(h=0) == -1 and rc(W=0) == -1 and rc(w=4097) == -1 and rc(H=65537) == -1
    assert rc(N=-1) == -1 and rc(mode=2) == -1
    assert rc() == -1  # null buffers with N > 0
    assert tmr_amd.TMRError is _lib.TMRError and callable(tmr_amd.mask_boxes)
    try:
        import torch

        tmr_amd.mask_boxes(torch.zeros(1, 4, 4), (8, 8), torch.zeros(1, 2), torch.zeros(1))
    except tmr_amd.TMRError:
        pass
    else:
        raise AssertionError("a CPU tensor must raise TMRError")
