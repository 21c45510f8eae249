"""TMREngine.BOX_POINTS_CROSSOVER, measured: at each bench config the points
launch over every candidate (box_at_points) and decoder_b's dense tiles
(box_dense) on the same heads context, HIP events around each call, best of
three; the crossover is (ns per pixel of the dense tiles) / (ns per point of
the points launch), the candidate fraction above which the dense tiles win.

    python profiles/points_crossover.py OUT.json [configs, default B C D E]
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402  (loads the package)
from tmr_amd import synth  # noqa: E402

tmr = bench.tmr


def events(fn, reps=3):
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def measure(config):
    cfg = bench.CONFIGS[config]
    dev = torch.device("cuda", 0)
    H = W = 2 * cfg["hf"]
    prec = cfg.get("precision", "fp32")
    eng = tmr.TMREngine(synth.reference_state_dict(0, device=dev), tmr.PathConfig(precision=prec))
    eng.use_graphs = False
    eng.box_at_peaks = "always"
    B, E = cfg["batch"], cfg["E"]
    feats = torch.from_numpy(synth.sam_features(1000, B, bench.CIN, H // 2, W // 2)).to(dev)
    ex, _ = synth.exemplar_set(2000, B, E, H, W, cfg["kmin"], cfg["kmax"])
    eng.detect(feats, ex, cls_ths=cfg["cls"], iou_threshold=cfg["iou"])  # warm-up
    rec = {}
    points, dense = eng.box_at_points, eng.box_dense

    def both(box, tiles):
        rec["points_ms_all"] = events(lambda: points(box, tiles))
        rec["dense_ms_all"] = events(dense)
        rec["tiles"] = len(tiles)
        points(box, tiles)  # (the dense tiles wrote the same bits at the candidates)

    eng.box_at_points = both
    eng.detect(feats, ex, cls_ths=cfg["cls"], iou_threshold=cfg["iou"])
    torch.cuda.synchronize()
    assert eng.last_box_route == "points" and "tiles" in rec
    n, pixels = eng.last_points, B * E * H * W
    pm, dm = min(rec["points_ms_all"]), min(rec["dense_ms_all"])
    direct = eng.last_points_flops / (pm * 1e-3) / 1e12
    out = dict(points=n, pixels=pixels, fraction=n / pixels, tiles=rec["tiles"], points_ms=pm, dense_ms=dm,
               ns_per_point=pm * 1e6 / n, ns_per_pixel=dm * 1e6 / pixels,
               crossover=(dm / pixels) / (pm / n), points_direct_tflops=direct,
               points_executed_tflops=direct * bench.SPLIT_TERMS[prec],
               points_ms_all=rec["points_ms_all"], dense_ms_all=rec["dense_ms_all"])
    return out


def main():
    out_path = sys.argv[1]
    res = {}
    for c in sys.argv[2:] or ["B", "C", "D", "E"]:
        res[c] = measure(c)
        print(c, json.dumps({k: res[c][k] for k in ("points", "points_ms", "dense_ms", "crossover")}), flush=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    assert all(np.isfinite(r["crossover"]) for r in res.values())


if __name__ == "__main__":
    main()
