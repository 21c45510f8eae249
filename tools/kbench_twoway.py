"""Times the fused two-way transformer at the refiner's workload shape: one
chunk of 50 prompts on a 64 x 64 embedding, a seeded transformer of SAM's
published structure (depth 2, 8 heads, MLP 2048, attention downsample 2).

  (a) stock      the stock-structured torch transformer alone, on materialised
                 [50,256,64,64] inputs (what the parent's decoder hands it)
  (b) shared     FusedTwoWayTransformer.forward_shared on the [1,256,64,64]
                 inputs; its five kernel calls timed one by one on the operands
                 a forward really passes (recorded from one), and the
                 token-side remainder as the difference of the medians
  (c) chunk      one refiner chunk -- prompt encoder stand-in, mask decoder,
                 tmr_mask_boxes to 1024 x 1024 -- with FusedMaskDecoder(dec)
                 (the parent's best) and with fuse_transformer=True; the 50
                 boxes of the two are compared
  (d) floors     each kernel call against the bytes it must move and its
                 algorithmic FLOP (present rows only), at the measured HBM read
                 rate of profiles/peaks_measured.json and the fp32-input MFMA
                 rate (64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz = 157 TFLOP/s)

All routes run in one process on the same seeded weights and inputs,
alternating, after a warm-up of each; every sample is a pair of device events
around work that ends in a device synchronise.  Reported: median, quartiles and
extremes.  "faster" follows the project's rule: the new median is below the
parent's by more than the sum of the two interquartile ranges.  Needs a GPU.

Usage:  python tools/kbench_twoway.py [--reps 40] [--warmup 5] [--out FILE.json]
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
import maskhead_ref  # noqa: E402
import twoway_ref as R  # noqa: E402
from tmr_amd import twoway as tw  # noqa: E402

N, EMB, SIZE, DIM, T = 50, 64, 1024, 256, 7
P = EMB * EMB
MFMA_F32_TFLOPS = 64 * 1024 * 2.4e9 / 1e12


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


def record_kernel_calls(fused, emb, pe, tokens):
    """The (name, args) of the five kernel calls of one forward_shared."""
    calls = []
    real_pool, real_update = tw.twoway_pool, tw.twoway_update

    def pool(*a):
        calls.append(("pool", tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in a)))
        return real_pool(*a)

    def update(*a, out=None):
        calls.append(("update", tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in a)))
        return real_update(*a, out=out)

    tw.twoway_pool, tw.twoway_update = pool, update
    try:
        fused.forward_shared(emb, pe, tokens)
    finally:
        tw.twoway_pool, tw.twoway_update = real_pool, real_update
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "twoway", "kbench.json"))
    ap.add_argument("--forward-only", action="store_true",
                    help="run forward_shared a few times and exit (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_twoway: no GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tr = R.module(R.weights(0, mlp_dim=2048)).to(dev)
    dec = maskhead_ref.Decoder(iou_hidden=256, transformer=tr)
    maskhead_ref.set_upscaling(dec.output_upscaling, maskhead_ref.weights(0))
    dec = dec.to(dev).eval()
    fused_tr = tmr.FusedTwoWayTransformer(tr)
    emb1, pe1 = torch.randn(1, DIM, EMB, EMB, device=dev), torch.randn(1, DIM, EMB, EMB, device=dev)
    tokens = torch.randn(N, T, DIM, device=dev)
    peaks = json.load(open(os.path.join(REPO, "profiles", "peaks_measured.json")))

    with torch.no_grad():
        if a.forward_only:
            for _ in range(a.warmup):
                fused_tr.forward_shared(emb1, pe1, tokens)
            torch.cuda.synchronize()
            return
        emb_n, pe_n = emb1.repeat(N, 1, 1, 1), pe1.repeat(N, 1, 1, 1)
        calls = record_kernel_calls(fused_tr, emb1, pe1, tokens)
        assert [c[0] for c in calls] == ["pool", "update", "pool", "update", "pool"]
        names = ["pool_layer0_shared", "update_layer0_shared", "pool_layer1", "update_layer1", "pool_final"]
        out_buf = torch.empty(N, P, DIM, device=dev)
        fns = {"stock_transformer": lambda: tr(emb_n, pe_n, tokens),
               "fused_shared": lambda: fused_tr.forward_shared(emb1, pe1, tokens)}
        for name, (kind, args) in zip(names, calls):
            if kind == "pool":
                fns[name] = lambda args=args: tw.twoway_pool(*args)
            else:
                fns[name] = lambda args=args: tw.twoway_update(*args, out=out_buf)
        t = alternate(fns, a.reps, a.warmup)
        want, got = fns["stock_transformer"](), fns["fused_shared"]()
        err = [float((g - w).abs().max() / w.abs().max()) for g, w in zip(got, want)]

        # one whole chunk: prompt encoder + decoder + tmr_mask_boxes
        enc = BoxPrompt((SIZE, SIZE), (EMB, EMB)).to(dev)
        feat = torch.randn(DIM, EMB, EMB, device=dev)
        c = torch.rand(N, 2, device=dev) * 0.6 + 0.2
        boxes = torch.cat([c - 0.1, c + 0.1], 1)
        logits = torch.rand(N, 2, device=dev)
        image = torch.zeros(1, 3, SIZE, SIZE, device=dev)
        parent_dec, new_dec = tmr.FusedMaskDecoder(dec), tmr.FusedMaskDecoder(dec, fuse_transformer=True)

        def chunk(decoder):
            r = tmr.SAM_box_refiner(decoder, lambda image_size, emb_size: enc)
            return lambda: r([logits], [boxes], [c], image, feat[None])

        tc = alternate({"chunk_parent": chunk(parent_dec), "chunk_new": chunk(new_dec)}, a.reps, a.warmup)
        bp, bn = chunk(parent_dec)()[1][0], chunk(new_dec)()[1][0]
        routes = dict(new_dec.transformer_calls)

    res = {"what": f"{N} prompts, {EMB}x{EMB} embedding, {T} tokens; transformer depth 2, 8 heads, MLP 2048, "
                   f"downsample 2; chunk: boxes at {SIZE}x{SIZE}",
           "device": torch.cuda.get_device_name(0), "method": "device events, alternating in one process",
           "normwise_fused_vs_stock_hs_keys": err, "chunk_routes_taken": routes,
           "chunk_boxes_equal": int((bp == bn).all(1).sum().item()), "chunk_boxes": N}
    for k, v in {**t, **tc}.items():
        res[k] = spread(v)
    kern = sum(res[k]["median_ms"] for k in names)
    res["fused_shared_kernels_ms_sum_of_medians"] = kern
    res["fused_shared_token_side_ms_by_difference"] = res["fused_shared"]["median_ms"] - kern
    res["ratio_transformer_medians"] = res["stock_transformer"]["median_ms"] / res["fused_shared"]["median_ms"]
    res["ratio_chunk_medians"] = res["chunk_parent"]["median_ms"] / res["chunk_new"]["median_ms"]
    iqr = lambda s: s["q75_ms"] - s["q25_ms"]  # noqa: E731
    res["chunk_faster"] = bool(res["chunk_parent"]["median_ms"] - res["chunk_new"]["median_ms"]
                               > iqr(res["chunk_parent"]) + iqr(res["chunk_new"]))
    hbm = peaks["hbm_read_gbs"] * 1e9
    floors = {}
    for name in names:
        nk = 1 if name.endswith("shared") else N
        if name.startswith("pool"):
            nbytes = (nk * P + P) * DIM * 4 + 2 * N * DIM * 64 * 4
            flop = 2 * 2 * 8 * T * DIM * P * N
        else:
            nbytes = (nk * P + P + N * P) * DIM * 4 + 2 * N * DIM * 64 * 4
            flop = 2 * 2 * 8 * T * DIM * P * N
        s = res[name]["median_ms"] * 1e-3
        floors[name] = {"bytes": nbytes, "flop_algorithmic": flop, "byte_floor_ms": nbytes / hbm * 1e3,
                        "flop_floor_ms": flop / (MFMA_F32_TFLOPS * 1e12) * 1e3, "GBps": nbytes / s / 1e9,
                        "TFLOPs_algorithmic": flop / s / 1e12, "TFLOPs_executed": flop / s / 1e12 * 8 / T}
    res["kernels"] = floors
    res["peaks_used"] = {"hbm_read_gbs": peaks["hbm_read_gbs"], "mfma_f32_tflops_by_arithmetic": MFMA_F32_TFLOPS}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
