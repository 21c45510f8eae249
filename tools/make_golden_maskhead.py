"""TEST INFRASTRUCTURE ONLY -- the golden file of the fused SAM mask head
(tests/golden/maskhead.npz).

Runs the reference's own utils/segment_anything/modeling/mask_decoder.py
(MaskDecoder.forward, this fork's argmax selection) on the CPU and records the
inputs, the stand-in transformer's outputs, the state dict and the reference's
results.  Needs the reference checkout (path below or $TMR_REFERENCE); runs
where the fixtures are made, never in a test.

The reference's segment_anything/__init__.py needs torchvision; it is never
executed: the packages are stubs that carry a __path__ only, and
modeling/mask_decoder.py (with modeling/common.py) is imported through them.

The decoder: transformer_dim 256, iou_head_hidden_dim 32, a seeded STAND-IN
transformer that returns the recorded (hs [N,7,256], src [N,h*w,256]) whatever
it is given.  Every 1-D parameter is re-drawn (biases and LayerNorm2d away
from 0 / 1).  The token-side weights (embeddings, the four hypernetwork MLPs,
the IoU head) are drawn on a coarse grid of fp16-representable values and
stored as float16, which keeps the file small; output_upscaling stays full
fp32, so the lo terms of the kernel's split are exercised.

Record 1: N = 5 prompts, embedding 6x8, image 61x93; src = 3 * noise inside a
random window of 2-3 cells per side per prompt, zero outside.  Conditions
asserted, re-seeding until they hold: at least 3 of the 5 masks have a share
of positive pixels strictly between 0.02 and 0.9; for every mask, under the
reference's own F.interpolate(..., align_corners=True), the box of {v > +d}
equals the box of {v > -d}, d = 1e-4 * max|mask|; the argmax picks at least
two different mask tokens.
Record 2 ("nf_"): one prompt whose src carries a NaN in one row and an
infinity in another, with the reference's output.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_maskhead.py
"""
from __future__ import annotations

import importlib
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
REF = os.path.join(os.environ.get("TMR_REFERENCE", "/root/reference"), "utils", "segment_anything")
sys.path.insert(0, os.path.join(REPO, "tests"))
import maskhead_ref  # noqa: E402

N, EMB, IMG, DIM = 5, (6, 8), (61, 93), 256


def load_ref():
    for name, path in (("refsam", REF), ("refsam.modeling", os.path.join(REF, "modeling"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    return importlib.import_module("refsam.modeling.mask_decoder")


class Replay(nn.Module):
    """The stand-in transformer: returns the recorded (hs, src)."""

    def __init__(self, hs, src):
        super().__init__()
        self.hs, self.src = hs, src

    def forward(self, src, pos_src, tokens):
        assert src.shape[0] == self.src.shape[0] == tokens.shape[0] and pos_src.shape == src.shape
        assert src.shape[2] * src.shape[3] == self.src.shape[1]
        return self.hs, self.src


def grid16(rng, shape, step, levels):
    """Values k * step, |k| <= levels: exact in fp16, few distinct values."""
    return (rng.integers(-levels, levels + 1, shape) * step).astype(np.float32)


def build(ref, rng):
    dec = ref.MaskDecoder(transformer_dim=DIM, transformer=nn.Identity(), iou_head_hidden_dim=32)
    wt = maskhead_ref.weights(int(rng.integers(1 << 30)))
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if name.startswith("output_upscaling"):
                continue
            if p.dim() == 1:
                p.copy_(torch.from_numpy(grid16(rng, tuple(p.shape), 1 / 32, 8)))
            elif "tokens" in name or "iou_token" in name:
                p.copy_(torch.from_numpy(grid16(rng, tuple(p.shape), 1 / 4, 4)))
            else:
                p.copy_(torch.from_numpy(grid16(rng, tuple(p.shape), 1 / 64, 4)))
        up = dec.output_upscaling
        for p, key in ((up[0].weight, "W1"), (up[0].bias, "b1"), (up[1].weight, "g"), (up[1].bias, "beta"),
                       (up[3].weight, "W2"), (up[3].bias, "b2")):
            p.copy_(torch.from_numpy(wt[key]))
    return dec.eval()


def run(dec, hs, src, emb):
    """The reference's forward with the replayed transformer outputs."""
    n = hs.shape[0]
    dec.transformer = Replay(torch.from_numpy(hs), torch.from_numpy(src))
    inputs = {
        "image_embeddings": np.zeros((1, DIM, *emb), np.float32),
        "image_pe": np.zeros((1, DIM, *emb), np.float32),
        "sparse_prompt_embeddings": np.zeros((n, 2, DIM), np.float32),
        "dense_prompt_embeddings": np.zeros((n, DIM, *emb), np.float32),
    }
    with torch.no_grad():
        masks, iou = dec(**{k: torch.from_numpy(v) for k, v in inputs.items()}, multimask_output=False)
        iou_pred = dec.iou_prediction_head(torch.from_numpy(hs)[:, 0])
        ids = torch.argmax(iou_pred, 1)
        hyper = torch.stack([dec.output_hypernetworks_mlps[int(i)](torch.from_numpy(hs)[k, 1 + int(i)])
                             for k, i in enumerate(ids)])
    return inputs, masks.numpy(), iou.numpy(), ids.numpy(), hyper.numpy()


def box_of(v, thr):
    ys, xs = np.nonzero(v > thr)
    return (0, 0, 0, 0) if len(ys) == 0 else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def boxes_of(masks):
    """(int boxes, margins hold, positive shares) under the reference's own upsampling."""
    up = F.interpolate(torch.from_numpy(masks), IMG, mode="bilinear", align_corners=True).numpy()[:, 0]
    ib, ok, share = [], True, []
    for m, v in zip(masks[:, 0], up):
        d = 1e-4 * float(np.abs(m).max())
        ib.append(box_of(v, 0.0))
        ok = ok and box_of(v, d) == box_of(v, -d) == ib[-1]
        share.append(float((v > 0).mean()))
    return np.array(ib, np.int32), ok, share


def main():
    ref = load_ref()
    seed = 0
    while True:
        rng = np.random.default_rng(seed)
        dec = build(ref, rng)
        hs = rng.standard_normal((N, 7, DIM)).astype(np.float32)
        src = maskhead_ref.windowed_src(rng, N, *EMB)
        inputs, masks, iou, ids, hyper = run(dec, hs, src, EMB)
        ib, ok, share = boxes_of(masks)
        if ok and sum(0.02 < s < 0.9 for s in share) >= 3 and len(set(ids.tolist())) >= 2:
            break
        seed += 1
    d = {"seed": np.int64(seed), "emb_size": np.array(EMB), "image_size": np.array(IMG), "hs": hs, "src": src,
         "masks": masks, "iou": iou, "ids": ids.astype(np.int64), "hyper": hyper, "iboxes": ib,
         "boxes": ib.astype(np.float32) / np.array([IMG[1], IMG[0], IMG[1], IMG[0]], np.float32),
         "shares": np.array(share)}
    for k, v in inputs.items():
        d["in_" + k] = v
    for k, v in dec.state_dict().items():
        if k.startswith("transformer"):
            continue
        a = v.numpy()
        if not k.startswith("output_upscaling"):
            assert np.array_equal(a.astype(np.float16).astype(np.float32), a), k
            a = a.astype(np.float16)
        d["sd_" + k] = a
    d["eps"] = np.float64(dec.output_upscaling[1].eps)

    # record 2: a NaN in one src row, an infinity in another
    hs2 = rng.standard_normal((1, 7, DIM)).astype(np.float32)
    src2 = (3.0 * rng.standard_normal((1, EMB[0] * EMB[1], DIM))).astype(np.float32)
    p_nan, p_inf = 1 * EMB[1] + 2, 4 * EMB[1] + 7
    src2[0, p_nan, 17] = np.nan
    src2[0, p_inf, 200] = np.inf
    _, masks2, iou2, ids2, hyper2 = run(dec, hs2, src2, EMB)
    want = np.zeros(masks2.shape[2:], bool)
    for p in (p_nan, p_inf):
        y, x = divmod(p, EMB[1])
        want[4 * y:4 * y + 4, 4 * x:4 * x + 4] = True
    assert np.array_equal(np.isnan(masks2[0, 0]), want) and np.isfinite(masks2[0, 0][~want]).all()
    d.update(nf_hs=hs2, nf_src=src2, nf_masks=masks2, nf_iou=iou2, nf_ids=ids2.astype(np.int64), nf_hyper=hyper2,
             nf_pixels=np.array([p_nan, p_inf]))

    out = os.path.join(REPO, "tests", "golden", "maskhead.npz")
    np.savez_compressed(out, **d)
    print(f"wrote {out}: seed {seed}, ids {ids.tolist()}, shares {[round(s, 3) for s in share]}, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
