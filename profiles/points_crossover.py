"""TMREngine.BOX_POINTS_CROSSOVER, measured: at each bench config the points
launch over every candidate (box_at_points) and decoder_b's dense tiles
(box_dense) on the same heads context, HIP events around each call, best of
three; the crossover is (ns per pixel of the dense tiles) / (ns per point of
the points launch), the candidate fraction above which the dense tiles win.

    python profiles/points_crossover.py OUT.json [configs, default B C D E]

--chain: TMREngine.FP_CHAIN_NS_PER_POINT, FP_STORE_NS_PER_PIXEL and
FP_AT_POINTS_FLOOR_MACS (box_fp_at_points).  At config B, a D-like config with
two exemplars per image ("D2") and config E, on one heads context: the chained
points launch, decoder_b's late store tiles and then the plain points launch,
HIP events, best of three; c_chain = (chain - points) / candidates, c_store =
store / image pixels.  Then config B's shapes at batch sizes 1..64: detect() as
a whole with box_fp_at_points "never" and "always" (graphs off), five timed
calls each; the floor is the smallest bound (decoder_plan.fp_late_bound_macs)
from which on the chain route's median beats the parent route's by more than
three times the larger spread (max - min) of the two.

    python profiles/points_crossover.py --chain OUT.json
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


CHAIN_CONFIGS = {"B": bench.CONFIGS["B"], "D2": dict(bench.CONFIGS["D"], E=2), "E": bench.CONFIGS["E"]}
FLOOR_BATCHES = (1, 2, 4, 8, 16, 32, 64)


def _chain_engine(cfg, B, mode):
    dev = torch.device("cuda", 0)
    H = W = 2 * cfg["hf"]
    eng = tmr.TMREngine(synth.reference_state_dict(0, device=dev), tmr.PathConfig())
    eng.use_graphs = False
    eng.box_at_peaks = "always"
    eng.box_fp_at_points = mode
    feats = torch.from_numpy(synth.sam_features(1000, B, bench.CIN, H // 2, W // 2)).to(dev)
    ex, _ = synth.exemplar_set(2000, B, cfg["E"], H, W, cfg["kmin"], cfg["kmax"])
    return eng, (lambda: eng.detect(feats, ex, cls_ths=cfg["cls"], iou_threshold=cfg["iou"])), H, W


def measure_chain(name):
    from tmr_amd.decoder_plan import fp_late_bound_macs
    cfg = CHAIN_CONFIGS[name]
    B = cfg["batch"]
    eng, detect, H, W = _chain_engine(cfg, B, "always")
    detect()  # warm-up
    rec = {}
    chain, points, store = eng.box_chain_at_points, eng.box_at_points, eng.box_late_store

    def all_three(box, tiles):
        rec["chain_ms_all"] = events(lambda: chain(box, tiles))
        rec["store_ms_all"] = events(store)
        rec["points_ms_all"] = events(lambda: points(box, tiles))  # (acc0 now holds decoder_b's tiles)
        rec["tiles"] = len(tiles)
        rec["nbt"] = eng._box_ctx.plan.skip_tiles

    eng.box_chain_at_points = all_three
    detect()
    torch.cuda.synchronize()
    assert eng.last_box_route == "points_chain" and "tiles" in rec
    n, pixels = eng.last_points, B * H * W
    cm, sm, pm = (min(rec[k]) for k in ("chain_ms_all", "store_ms_all", "points_ms_all"))
    c_chain, c_store = (cm - pm) * 1e6 / n, sm * 1e6 / pixels
    return dict(points=n, image_pixels=pixels, fraction_of_unit_pixels=n / (pixels * cfg["E"]), tiles=rec["tiles"],
                chain_ms=cm, store_ms=sm, points_ms=pm, c_chain_ns_per_point=c_chain, c_store_ns_per_pixel=c_store,
                rule_takes_chain=bool(n * c_chain < pixels * c_store), saving_ms=sm - (cm - pm),
                bound_macs=fp_late_bound_macs(B, H, W, rec["nbt"], bench.CIN, 3),
                **{k: rec[k] for k in rec if k.endswith("_all")})


def measure_floor():
    from tmr_amd.decoder_plan import fp_late_bound_macs
    cfg, rows = bench.CONFIGS["B"], []
    for B in FLOOR_BATCHES:
        row = dict(batch=B)
        for mode in ("never", "always"):
            eng, detect, H, W = _chain_engine(cfg, B, mode)
            detect()
            detect()
            torch.cuda.synchronize()
            row[mode + "_ms_all"] = t = events(detect, reps=5)
            row[mode + "_route"] = eng.last_box_route
            row[mode + "_ms"] = float(np.median(t))
        row["bound_macs"] = fp_late_bound_macs(B, H, W, 8, bench.CIN, 3)
        row["gain_ms"] = row["never_ms"] - row["always_ms"]
        row["spread_ms"] = max(max(row[m + "_ms_all"]) - min(row[m + "_ms_all"]) for m in ("never", "always"))
        row["wins"] = bool(row["gain_ms"] > 3 * row["spread_ms"])
        rows.append(row)
        print("floor", json.dumps({k: row[k] for k in ("batch", "never_ms", "always_ms", "spread_ms", "wins")}),
              flush=True)
    floor = None
    for i in range(len(rows) - 1, -1, -1):  # the smallest bound from which on every larger one wins too
        if not rows[i]["wins"]:
            break
        floor = rows[i]["bound_macs"]
    return dict(rows=rows, floor_macs=floor)


def main_chain(out_path):
    res = {"configs": {}}
    for c in CHAIN_CONFIGS:
        res["configs"][c] = r = measure_chain(c)
        print(c, json.dumps({k: r[k] for k in ("points", "chain_ms", "store_ms", "points_ms", "c_chain_ns_per_point",
                                               "c_store_ns_per_pixel", "rule_takes_chain")}), flush=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    res["floor"] = measure_floor()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    if sys.argv[1] == "--chain":
        return main_chain(sys.argv[2])
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
