"""Times the mask -> box step of the SAM box refiner at the workload's own
size: one chunk of 50 masks, 256 x 256 -> 1024 x 1024.

  fused         tmr_amd.mask_boxes (tmr_mask_boxes: three launches, no sync)
  materialised  the plain-torch form of the reference (box_refine.py:232-246)
                on the same GPU: F.interpolate(align_corners=True), threshold,
                the Python loop over the masks with torch.where + min / max
                (one device sync per mask), the elementwise epilogue

Both run in the same process on the same seeded blob masks, alternating,
after a warm-up of each; every sample is a host clock around work that ends
in a device synchronise, and (fused only, which never syncs inside) a pair of
device events.  Reported: the median, the quartiles and the extremes of the
samples, the ratio of the medians, and the fused form's input bytes over its
median event time.  Needs a GPU: there is no CPU path to time.

Usage:  python tools/kbench_mask_boxes.py [--reps 30] [--warmup 5] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch.nn import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from tmr_import import load_package  # noqa: E402

tmr = load_package()
import refine_ref  # noqa: E402

N, LOW, SIZE = 50, 256, 1024


def materialised(masks, logits, iou, img_res):
    """Upsampled plane written, thresholded plane written, one torch.where
    (a sync) and four reductions per mask, then the elementwise tail."""
    pos = F.interpolate(masks, (SIZE, SIZE), mode="bilinear", align_corners=True)[:, 0] > 0
    ibox = torch.zeros((pos.shape[0], 4), dtype=torch.float32, device=masks.device)
    for n in range(pos.shape[0]):
        ys, xs = torch.where(pos[n])
        if ys.numel():
            ibox[n, 0], ibox[n, 1], ibox[n, 2], ibox[n, 3] = xs.min(), ys.min(), xs.max(), ys.max()
    boxes = ibox / img_res
    refs = torch.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], dim=-1)
    return torch.cat([iou, torch.zeros_like(iou)], dim=-1) * logits, boxes, refs


def spread(x):
    x = np.sort(np.asarray(x, np.float64))
    q = np.percentile(x, [25, 50, 75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2]), "min_ms": float(x[0]),
            "max_ms": float(x[-1]), "n": int(x.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_mask_boxes: no GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    masks = torch.from_numpy(refine_ref.blob_masks(rng, N, LOW, LOW)).to(dev)[:, None]
    logits = torch.from_numpy(rng.uniform(0.1, 1, (N, 2)).astype(np.float32)).to(dev)
    iou = torch.from_numpy(rng.uniform(0.1, 1, (N, 1)).astype(np.float32)).to(dev)
    img_res = torch.tensor([SIZE, SIZE, SIZE, SIZE], dtype=torch.float32, device=dev)

    def fused():
        return tmr.mask_boxes(masks, (SIZE, SIZE), logits, iou)

    for _ in range(a.warmup):
        f_out = fused()
        m_out = materialised(masks, logits, iou, img_res)
    torch.cuda.synchronize()
    same_boxes = bool(torch.equal(f_out[1], m_out[1]))

    wall = {"fused": [], "materialised": []}
    ev = []
    for _ in range(a.reps):
        for name, fn in (("fused", fused), ("materialised", lambda: materialised(masks, logits, iou, img_res))):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            if name == "fused":
                ev.append(e0.elapsed_time(e1))
    res = {"what": f"{N} masks {LOW}x{LOW} -> {SIZE}x{SIZE}", "device": torch.cuda.get_device_name(0),
           "boxes_equal": same_boxes,
           "fused_wall": spread(wall["fused"]), "fused_events": spread(ev),
           "materialised_wall": spread(wall["materialised"])}
    res["ratio_wall_medians"] = res["materialised_wall"]["median_ms"] / res["fused_wall"]["median_ms"]
    in_bytes = N * LOW * LOW * 4
    res["fused_input_bytes"] = in_bytes
    res["fused_pixels_per_s"] = N * SIZE * SIZE / (res["fused_events"]["median_ms"] * 1e-3)
    res["materialised_plane_bytes_not_moved"] = N * SIZE * SIZE * 10
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
