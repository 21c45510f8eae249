"""Times the fused SAM mask head at the refiner's workload shape: one chunk of
50 prompts on a 64 x 64 embedding (masks 256 x 256).

  fused   tmr_amd.mask_head (tmr_mask_head: one launch) on the selected
          hypernetwork row, plus the token-side ops FusedMaskDecoder runs (the
          IoU head, the argmax, the four MLPs on all rows, the gather)
  stock   the stock torch head on the same GPU: output_upscaling
          (ConvTranspose2d, LayerNorm2d, GELU, ConvTranspose2d, GELU), the four
          MLPs, the [N,4,32] x [N,32,65536] matmul, the argmax selection

Both exclude the transformer, run in one process on the same seeded (hs, src)
and weights, alternating, after a warm-up of each; every sample is a pair of
device events around work that ends in a device synchronise.  "kernel" is the
tmr_mask_head launch alone (events).

A second part times one whole chunk -- prompt encoder stand-in, mask decoder,
tmr_mask_boxes to 1024 x 1024 -- with the stock decoder and with
FusedMaskDecoder around it, with a two-way transformer of SAM's published
structure (depth 2, 8 heads, MLP 2048, attention downsample 2; written out
below, seeded weights): what share of the chunk the head was.

Reported: median, quartiles and extremes of the samples, the ratios of the
medians, and the kernel's time against its two bounds (bytes it must move,
algorithmic FLOP).  Needs a GPU.

Usage:  python tools/kbench_mask_head.py [--reps 40] [--warmup 5] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from tmr_import import load_package  # noqa: E402

tmr = load_package()
import maskhead_ref as R  # noqa: E402

N, EMB, SIZE, DIM = 50, 64, 1024, 256


class Attention(nn.Module):
    def __init__(self, dim, heads, down=1):
        super().__init__()
        self.heads, inner = heads, dim // down
        self.q, self.k, self.v, self.o = (nn.Linear(dim, inner), nn.Linear(dim, inner), nn.Linear(dim, inner),
                                          nn.Linear(inner, dim))

    def forward(self, q, k, v):
        def split(x):
            b, n, c = x.shape
            return x.reshape(b, n, self.heads, c // self.heads).transpose(1, 2)

        q, k, v = split(self.q(q)), split(self.k(k)), split(self.v(v))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1]), dim=-1) @ v
        return self.o(a.transpose(1, 2).flatten(2))


class Block(nn.Module):
    def __init__(self, dim, heads, mlp, skip_pe):
        super().__init__()
        self.self_attn, self.t2i, self.i2t = Attention(dim, heads), Attention(dim, heads, 2), Attention(dim, heads, 2)
        self.n1, self.n2, self.n3, self.n4 = (nn.LayerNorm(dim) for _ in range(4))
        self.mlp = nn.Sequential(nn.Linear(dim, mlp), nn.ReLU(), nn.Linear(mlp, dim))
        self.skip_pe = skip_pe

    def forward(self, q, k, qpe, kpe):
        if self.skip_pe:
            q = self.self_attn(q, q, q)
        else:
            q = q + self.self_attn(q + qpe, q + qpe, q)
        q = self.n1(q)
        q = self.n2(q + self.t2i(q + qpe, k + kpe, k))
        q = self.n3(q + self.mlp(q))
        k = self.n4(k + self.i2t(k + kpe, q + qpe, q))
        return q, k


class TwoWay(nn.Module):
    """SAM's two-way transformer, structure only (seeded weights)."""

    def __init__(self, depth=2, dim=DIM, heads=8, mlp=2048):
        super().__init__()
        self.layers = nn.ModuleList(Block(dim, heads, mlp, i == 0) for i in range(depth))
        self.final, self.norm = Attention(dim, heads, 2), nn.LayerNorm(dim)

    def forward(self, image_embedding, image_pe, point_embedding):
        k = image_embedding.flatten(2).permute(0, 2, 1)
        kpe = image_pe.flatten(2).permute(0, 2, 1)
        q = point_embedding
        for layer in self.layers:
            q, k = layer(q, k, point_embedding, kpe)
        q = self.norm(q + self.final(q + point_embedding, k + kpe, k))
        return q, k


class BoxPrompt(nn.Module):
    """A prompt encoder stand-in of SAM's cost: random-Fourier corner
    embeddings [n,2,256], a broadcast no-mask dense embedding, a dense PE."""

    def __init__(self, size, emb):
        super().__init__()
        self.size, self.emb = size, emb
        self.register_buffer("gauss", torch.randn(2, DIM // 2))
        self.corner = nn.Embedding(2, DIM)
        self.no_mask = nn.Embedding(1, DIM)

    def pe(self, xy):
        p = (2 * xy - 1) @ self.gauss * (2 * math.pi)
        return torch.cat([p.sin(), p.cos()], -1)

    def forward(self, points, boxes, masks):
        xy = (boxes.reshape(-1, 2, 2) + 0.5) / boxes.new_tensor([self.size[1], self.size[0]])
        sparse = self.pe(xy) + self.corner.weight
        dense = self.no_mask.weight.reshape(1, -1, 1, 1).expand(boxes.shape[0], -1, *self.emb)
        return sparse, dense

    def get_dense_pe(self):
        ys, xs = torch.meshgrid((torch.arange(self.emb[0], device=self.gauss.device) + 0.5) / self.emb[0],
                                (torch.arange(self.emb[1], device=self.gauss.device) + 0.5) / self.emb[1], indexing="ij")
        return self.pe(torch.stack([xs, ys], -1)).permute(2, 0, 1)[None]


def spread(x):
    x = np.sort(np.asarray(x, np.float64))
    q = np.percentile(x, [25, 50, 75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2]), "min_ms": float(x[0]),
            "max_ms": float(x[-1]), "n": int(x.size)}


def alternate(fns, reps, warmup):
    """{name: [event ms]} of the functions run in turn, reps times, after warmup rounds of each."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_mask_head: no GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    dec = R.Decoder(iou_hidden=256)
    R.set_upscaling(dec.output_upscaling, R.weights(0))
    dec = dec.to(dev).eval()
    hs = torch.randn(N, 7, DIM, device=dev)
    src = 2 * torch.randn(N, EMB * EMB, DIM, device=dev)
    fused_dec = tmr.FusedMaskDecoder(dec)
    T = dec.num_mask_tokens

    def token_side():
        iou_pred = dec.iou_prediction_head(hs[:, 0])
        ids = torch.argmax(iou_pred, 1)
        hyper_all = torch.stack([dec.output_hypernetworks_mlps[i](hs[:, 1 + i]) for i in range(T)], 1)
        return torch.gather(hyper_all, 1, ids.view(-1, 1, 1).expand(-1, 1, 32))[:, 0], torch.gather(iou_pred, 1,
                                                                                                   ids.view(-1, 1))

    with torch.no_grad():
        hyper = token_side()[0].contiguous()
        fns = {
            "fused_head": lambda: tmr.mask_head(src, token_side()[0], fused_dec.weights, (EMB, EMB)),
            "stock_head": lambda: dec.stock_head(hs, src, (EMB, EMB)),
            "kernel": lambda: tmr.mask_head(src, hyper, fused_dec.weights, (EMB, EMB)),
        }
        t = alternate(fns, a.reps, a.warmup)
        got, want = fns["fused_head"](), fns["stock_head"]()[0]
        err = float((got - want).abs().max() / want.abs().max())

        # one whole chunk: prompt encoder + decoder + tmr_mask_boxes
        dec.transformer = TwoWay().to(dev).eval()
        enc = BoxPrompt((SIZE, SIZE), (EMB, EMB)).to(dev)
        feat = torch.randn(DIM, EMB, EMB, device=dev)
        c = torch.rand(N, 2, device=dev) * 0.6 + 0.2
        boxes = torch.cat([c - 0.1, c + 0.1], 1)
        logits = torch.rand(N, 2, device=dev)
        image = torch.zeros(1, 3, SIZE, SIZE, device=dev)

        def chunk(decoder):
            r = tmr.SAM_box_refiner(decoder, lambda image_size, emb_size: enc)
            return lambda: r([logits], [boxes], [c], image, feat[None])

        tc = alternate({"chunk_stock": chunk(dec), "chunk_fused": chunk(fused_dec)}, a.reps, a.warmup)
        bs, bf = chunk(dec)()[1][0], chunk(fused_dec)()[1][0]

    res = {"what": f"{N} prompts, {EMB}x{EMB} embedding -> masks {4 * EMB}x{4 * EMB}; chunk: boxes at {SIZE}x{SIZE}",
           "device": torch.cuda.get_device_name(0), "method": "device events, alternating in one process",
           "normwise_fused_vs_stock": err,
           "chunk_boxes_equal": int((bs == bf).all(1).sum().item()), "chunk_boxes": N}
    for k, v in {**t, **tc}.items():
        res[k] = spread(v)
    res["ratio_head_medians"] = res["stock_head"]["median_ms"] / res["fused_head"]["median_ms"]
    res["ratio_chunk_medians"] = res["chunk_stock"]["median_ms"] / res["chunk_fused"]["median_ms"]
    res["head_share_of_stock_chunk"] = res["stock_head"]["median_ms"] / res["chunk_stock"]["median_ms"]
    k_s = res["kernel"]["median_ms"] * 1e-3
    res["kernel_bytes"] = N * EMB * EMB * DIM * 4 + N * 16 * EMB * EMB * 4
    res["kernel_flop_algorithmic"] = 2 * N * EMB * EMB * (256 * 256 + 4 * 64 * 128)
    res["kernel_GBps"] = res["kernel_bytes"] / k_s / 1e9
    res["kernel_TFLOPs_algorithmic"] = res["kernel_flop_algorithmic"] / k_s / 1e12
    res["kernel_TFLOPs_executed_f16"] = 3 * res["kernel_TFLOPs_algorithmic"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
