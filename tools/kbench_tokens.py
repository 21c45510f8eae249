"""Times the token side in HIP (fuse_tokens=True) against the torch token side
at the refiner's workload shape -- the workload and the method of
tools/kbench_twoway.py: one chunk of 50 prompts on a 64 x 64 embedding, 7
tokens, a seeded transformer of SAM's published structure (depth 2, 8 heads,
MLP 2048, attention downsample 2), the decoder's real head sizes.

  (a) transformer  FusedTwoWayTransformer.forward_shared with fuse_tokens off
                   (the parent's route, the baseline) and on
  (b) chunk        one refiner chunk -- prompt encoder stand-in, mask decoder,
                   tmr_mask_boxes to 1024 x 1024 -- with
                   FusedMaskDecoder(dec, fuse_transformer=True) (the parent's
                   best) and with fuse_tokens=True as well; the 50 boxes of the
                   two are compared
  (c) kernels      each token kernel call alone, on the operands a forward
                   really passes (recorded from one): front and back of layers 0
                   and 1, of the final attention, and the tail

All routes run in one process on the same seeded weights and inputs,
alternating, after a warm-up of each; every sample is a pair of device events
around work that ends in a device synchronise.  Reported: median, quartiles and
extremes.  "faster" follows the project's rule: the new median is below the
parent's by more than the sum of the two interquartile ranges.  Needs a GPU.

Usage:  python tools/kbench_tokens.py [--reps 40] [--warmup 5] [--out FILE.json]
        python tools/kbench_tokens.py --forward-only {off,on}   (for a kernel trace)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from tmr_import import load_package  # noqa: E402

tmr = load_package()
import maskhead_ref  # noqa: E402
import twoway_ref as R  # noqa: E402
from kbench_twoway import DIM, EMB, N, SIZE, T, BoxPrompt, alternate, spread  # noqa: E402
from tmr_amd import tokens as tk  # noqa: E402


def record_token_calls(decoder, args):
    """The (kernel, args, kwargs) of the token kernel calls of one decoder forward."""
    calls = []
    real = {n: getattr(tk, n) for n in ("tokens_front", "tokens_back", "tokens_tail")}

    def wrap(name):
        def fn(*a, **kw):
            calls.append((name, tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in a), kw))
            return real[name](*a, **kw)
        return fn

    for n in real:
        setattr(tk, n, wrap(n))
    try:
        decoder(*args, False)
    finally:
        for n, f in real.items():
            setattr(tk, n, f)
    return calls, real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tokens", "kbench.json"))
    ap.add_argument("--forward-only", choices=("off", "on"),
                    help="run a few decoder forwards with fuse_tokens off or on and exit (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_tokens: no GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tr = R.module(R.weights(0, mlp_dim=2048)).to(dev)
    dec = maskhead_ref.Decoder(iou_hidden=256, transformer=tr)
    maskhead_ref.set_upscaling(dec.output_upscaling, maskhead_ref.weights(0))
    dec = dec.to(dev).eval()
    off_tr, on_tr = tmr.FusedTwoWayTransformer(tr), tmr.FusedTwoWayTransformer(tr, fuse_tokens=True)
    off_dec = tmr.FusedMaskDecoder(dec, fuse_transformer=True)
    on_dec = tmr.FusedMaskDecoder(dec, fuse_transformer=True, fuse_tokens=True)
    emb1, pe1 = torch.randn(1, DIM, EMB, EMB, device=dev), torch.randn(1, DIM, EMB, EMB, device=dev)
    tokens = torch.randn(N, T, DIM, device=dev)
    sparse = torch.randn(N, 2, DIM, device=dev)
    dense = torch.randn(1, DIM, EMB, EMB, device=dev).expand(N, -1, -1, -1)
    dec_args = (emb1, pe1, sparse, dense)

    with torch.no_grad():
        if a.forward_only:
            d = on_dec if a.forward_only == "on" else off_dec
            for _ in range(a.warmup):
                d(*dec_args, False)
            torch.cuda.synchronize()
            return
        calls, real = record_token_calls(on_dec, dec_args)
        kinds = [c[0] for c in calls]
        assert kinds == ["tokens_front", "tokens_back"] * 3 + ["tokens_tail"], kinds
        names = ["front_layer0", "back_layer0", "front_layer1", "back_layer1", "front_final", "back_final", "tail"]
        fns = {"transformer_off": lambda: off_tr.forward_shared(emb1, pe1, tokens),
               "transformer_on": lambda: on_tr.forward_shared(emb1, pe1, tokens)}
        for name, (kind, args, kw) in zip(names, calls):
            fns[name] = lambda kind=kind, args=args, kw=kw: real[kind](*args, **kw)
        t = alternate(fns, a.reps, a.warmup)
        want, got = fns["transformer_off"](), fns["transformer_on"]()
        err = [float((g - w).abs().max() / w.abs().max()) for g, w in zip(got, want)]

        # one whole chunk: prompt encoder + decoder + tmr_mask_boxes
        enc = BoxPrompt((SIZE, SIZE), (EMB, EMB)).to(dev)
        feat = torch.randn(DIM, EMB, EMB, device=dev)
        c = torch.rand(N, 2, device=dev) * 0.6 + 0.2
        boxes = torch.cat([c - 0.1, c + 0.1], 1)
        logits = torch.rand(N, 2, device=dev)
        image = torch.zeros(1, 3, SIZE, SIZE, device=dev)

        def chunk(decoder):
            r = tmr.SAM_box_refiner(decoder, lambda image_size, emb_size: enc)
            return lambda: r([logits], [boxes], [c], image, feat[None])

        tc = alternate({"chunk_off": chunk(off_dec), "chunk_on": chunk(on_dec)}, a.reps, a.warmup)
        bp, bn = chunk(off_dec)()[1][0], chunk(on_dec)()[1][0]
        routes = dict(on_dec.transformer_calls)

    res = {"what": f"{N} prompts, {EMB}x{EMB} embedding, {T} tokens; transformer depth 2, 8 heads, MLP 2048, "
                   f"downsample 2; IoU head hidden 256, 4 hypernetwork MLPs; chunk: boxes at {SIZE}x{SIZE}; "
                   "off = the torch token side (the parent's route), on = fuse_tokens=True",
           "device": torch.cuda.get_device_name(0), "method": "device events, alternating in one process",
           "normwise_on_vs_off_hs_keys": err, "chunk_routes_taken": routes,
           "chunk_boxes_equal": int((bp == bn).all(1).sum().item()), "chunk_boxes": N,
           "max_abs_box_difference": float((bp - bn).abs().max().item())}
    for k, v in {**t, **tc}.items():
        res[k] = spread(v)
    res["token_kernels_ms_sum_of_medians"] = sum(res[k]["median_ms"] for k in names)
    res["ratio_transformer_medians"] = res["transformer_off"]["median_ms"] / res["transformer_on"]["median_ms"]
    res["ratio_chunk_medians"] = res["chunk_off"]["median_ms"] / res["chunk_on"]["median_ms"]
    iqr = lambda s: s["q75_ms"] - s["q25_ms"]  # noqa: E731
    for what in ("transformer", "chunk"):
        off, on = res[what + "_off"], res[what + "_on"]
        res[what + "_faster"] = bool(off["median_ms"] - on["median_ms"] > iqr(off) + iqr(on))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
