"""TEST INFRASTRUCTURE ONLY -- the golden file of the SAM box refiner
(tests/golden/refine.npz).

Runs the reference's own utils/box_refine.py (SAM_box_refiner.forward and
forward_refine) on the CPU with seeded stand-ins for the two SAM modules and
records the inputs, every stand-in call's outputs, the boxes each call
received and the reference's results.  Needs the reference checkout (path
below or $TMR_REFERENCE); runs where the fixtures are made, never in a test.

The reference's constructor builds the SAM mask decoder and fetches its
checkpoint.  Neither is reached here: torch.hub.load_state_dict_from_url is
replaced by a function that raises BEFORE the module is imported, the object
is made with __new__ + nn.Module.__init__, its attributes are set by hand and
prompt_encoder_init is overridden.  The vendored segment_anything package the
module imports from is stubbed (its classes are never instantiated).

Stand-ins: the prompt encoder returns small constant embeddings and records
the boxes it receives; the mask decoder returns the next seeded low-res masks
[n,1,16,24] and iou [n,1].  Three images of 7, 1 (the Get_pred_boxes dummy
row) and 4 candidates plus an image without candidates (the pass-through), at
step = 3: full chunks and ragged last chunks.  Among the masks: one all
negative, one all positive, one with a single positive low-res pixel in a
corner, and (forward_refine, image 1) an exemplar mask one column wide, which
makes two scaler entries infinite, followed by an empty candidate mask (zero
extents times the infinite scaler: NaN).

Condition asserted (re-seeded until it holds): for every recorded mask, under
the reference's own F.interpolate, the box of {v > +eps} equals the box of
{v > -eps}, eps = 1e-5 * max|mask| -- no recorded box rests on rounding.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_refine.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.path.join(os.environ.get("TMR_REFERENCE", "/root/reference"), "utils", "box_refine.py")
sys.path.insert(0, os.path.join(REPO, "tests"))
import refine_ref  # noqa: E402

h, w, IMG_H, IMG_W = 16, 24, 61, 93
EMB = (4, 6)
COUNTS = [7, 1, 4, 0]
STEP = 3


def _no_fetch(*a, **k):
    raise RuntimeError("the golden generator must never fetch a checkpoint")


def load_ref():
    torch.hub.load_state_dict_from_url = _no_fetch
    pkg = types.ModuleType("refutils")
    pkg.__path__ = []
    sys.modules["refutils"] = pkg
    sa = types.ModuleType("refutils.segment_anything")
    sa.__path__ = []
    sys.modules["refutils.segment_anything"] = sa
    mod = types.ModuleType("refutils.segment_anything.modeling")
    mod.MaskDecoder = mod.TwoWayTransformer = mod.PromptEncoder = object
    sys.modules["refutils.segment_anything.modeling"] = mod
    spec = importlib.util.spec_from_file_location("refutils.box_refine", REF)
    m = importlib.util.module_from_spec(spec)
    sys.modules["refutils.box_refine"] = m
    spec.loader.exec_module(m)
    return m


class PromptStub(nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, points, boxes, masks):
        assert points is None and masks is None
        self.log.append(boxes.detach().clone().numpy())
        n = boxes.shape[0]
        return torch.zeros(n, 2, 4), torch.zeros(n, 4, *EMB)

    def get_dense_pe(self):
        return torch.zeros(1, 4, *EMB)


class DecoderStub(nn.Module):
    def __init__(self, calls):
        super().__init__()
        self.calls, self.k = calls, 0

    def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings,
                multimask_output):
        assert multimask_output is False and image_embeddings.shape[0] == 1
        m, iou = self.calls[self.k]
        assert sparse_prompt_embeddings.shape[0] == m.shape[0]
        self.k += 1
        return torch.from_numpy(m), torch.from_numpy(iou)


def chunk_sizes(with_exemplar):
    out = []
    for n in COUNTS:
        if n == 0:
            continue
        if with_exemplar:
            out.append(1)
        out += [min(STEP, n - a) for a in range(0, n, STEP)]
    return out


def draw(seed):
    rng = np.random.default_rng(seed)
    d = {}
    for i, n in enumerate(COUNTS):
        if i == 1:  # the Get_pred_boxes dummy row
            lg, bx, rf = np.zeros((1, 2), np.float32), np.array([[0, 0, 1e-14, 1e-14]], np.float32), \
                np.zeros((1, 2), np.float32)
        else:
            c = rng.uniform(0.1, 0.9, (n, 2))
            s = rng.uniform(0.02, 0.2, (n, 2))
            bx = np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)
            rf = c.astype(np.float32)
            lg = np.stack([rng.uniform(0.1, 1.0, n), 1 - rng.uniform(0.1, 1.0, n)], 1).astype(np.float32)
        d[f"in_logits{i}"], d[f"in_boxes{i}"], d[f"in_refs{i}"] = lg, bx, rf
    ex = np.zeros((len(COUNTS), 1, 4), np.float32)
    for i in range(len(COUNTS)):
        c, s = rng.uniform(0.3, 0.7, 2), rng.uniform(0.05, 0.2, 2)
        ex[i, 0] = np.concatenate([c - s / 2, c + s / 2])
    d["exemplars"] = ex
    calls = {}
    for tag, with_ex in (("fwd", False), ("rfn", True)):
        sizes = chunk_sizes(with_ex)
        masks = refine_ref.blob_masks(rng, sum(sizes), h, w)
        if tag == "fwd":  # image 0's masks 1, 2 and 4: chunk 0 and chunk 1
            masks[1] = -np.abs(masks[1]) - 0.5
            masks[2] = np.abs(masks[2]) + 0.5
            masks[4] = -0.7
            masks[4, h - 1, 0] = 1.0
        else:  # image 1's exemplar mask (after image 0's 1 + 7): one output column wide
            k = 8
            masks[k] = -10.0
            masks[k, 3:9, 5] = 1.0
            masks[k + 1] = -np.abs(masks[k + 1]) - 0.5  # its candidate's mask is empty: 0 * inf = NaN
        iou = rng.uniform(0.3, 1.0, (sum(sizes), 1)).astype(np.float32)
        o, cl = 0, []
        for n in sizes:
            cl.append((masks[o:o + n, None].copy(), iou[o:o + n].copy()))
            o += n
        calls[tag] = cl
    return d, calls


def margins_hold(calls):
    def ref_value(m, size):
        return F.interpolate(torch.from_numpy(m)[None, None], size, mode="bilinear", align_corners=True)[0, 0].numpy()

    return all(refine_ref.margin_ok(m[:, 0], (IMG_H, IMG_W), ref_value) for cl in calls.values() for m, _ in cl)


def main():
    ref = load_ref()
    seed = 0
    while True:
        d, calls = draw(seed)
        if margins_hold(calls):
            break
        seed += 1
    d["seed"] = np.int64(seed)
    d["mask_size"], d["image_size"], d["emb_size"] = np.array([h, w]), np.array([IMG_H, IMG_W]), np.array(EMB)
    d["step"], d["counts"] = np.int64(STEP), np.array(COUNTS)
    B = len(COUNTS)
    image = torch.zeros(B, 3, IMG_H, IMG_W)
    feats = torch.zeros(B, 2, *EMB)
    for tag in ("fwd", "rfn"):
        log = []
        r = ref.SAM_box_refiner.__new__(ref.SAM_box_refiner)
        nn.Module.__init__(r)
        r.step, r.prompt_embed_dim = STEP, 256
        r.mask_decoder = DecoderStub(calls[tag])
        enc = PromptStub(log)
        r.prompt_encoder_init = lambda image_size, emb_size: enc
        L = [torch.from_numpy(d[f"in_logits{i}"]) for i in range(B)]
        Bx = [torch.from_numpy(d[f"in_boxes{i}"]) for i in range(B)]
        R = [torch.from_numpy(d[f"in_refs{i}"]) for i in range(B)]
        with torch.no_grad():
            if tag == "fwd":
                oL, oB, oR = r.forward(L, Bx, R, image, feats)
            else:
                oL, oB, oR = r.forward_refine(L, Bx, R, image, torch.from_numpy(d["exemplars"]), feats)
        assert r.mask_decoder.k == len(calls[tag]) == len(log)
        d[f"{tag}_ncalls"] = np.int64(len(log))
        for k, ((m, iou), bx) in enumerate(zip(calls[tag], log)):
            d[f"{tag}_call{k}_masks"], d[f"{tag}_call{k}_iou"], d[f"{tag}_call{k}_boxes"] = m, iou, bx
        for i in range(B):
            d[f"{tag}_logits{i}"], d[f"{tag}_boxes{i}"], d[f"{tag}_refs{i}"] = \
                oL[i].numpy(), oB[i].numpy(), oR[i].numpy()
    assert not np.isfinite(d["rfn_boxes1"]).all(), "the one-column exemplar mask gives an infinite scaler"
    out = os.path.join(REPO, "tests", "golden", "refine.npz")
    np.savez_compressed(out, **d)
    print(f"wrote {out}: seed {seed}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
