"""The evaluation losses on the GPU (tmr_gt_loss): GT target maps, BCE / focal
and GIoU, through the ABI wrappers (tmr_amd.gt_loss), the drop-in
GT_map / SetCriterion_TM and the fused TMREngine.eval_loss.

Class maps, targets, counts, sample lists and rows are compared bit for bit.
Losses: 1e-5 relative (the project's fp32 contract; every term is
non-negative, so element rounding bounds the sum) against the reference's
fp32 fixtures and against the float64 restatement (tests/evalloss_ref.py).
Per-unit fp64 sums against the restatement: 1e-9 relative -- both sides sum
at most 128*128 non-negative fp64 terms (n * 2^-53 = 2e-12) whose elements
differ only by libm's exp / log1p rounding.
The kernel stages box records in chunks of 256 (GT_CHUNK), so the sweep's box
counts are the issue's {1, 2, 63, 64, 65, 300} plus 255, 256, 257.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import evalloss_ref as er
import oracle
import tmr_amd
from tmr_amd import gt_loss as gl
from tmr_amd import host, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REL = 1e-5
ULP32 = 2.0 ** -23


def cuda(x):
    return torch.as_tensor(x).to(DEV)


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def close(a, b, rel):
    return abs(float(a) - float(b)) <= rel * abs(float(b))


@pytest.fixture(scope="module")
def cases(golden):
    return er.load_cases(golden("evalloss"))


def _batch(c):
    return {"regression_ablation_a": c["a"], "regression_ablation_b": c["b"], "regression_ablation_c": c["c"]}


def _ref_losses(c):
    ce = gi = 0.0
    for lv in range(len(c["levels"])):
        a, b = er.losses(er.case_level(c, lv, oracle.expf), c["focal"])
        ce += a / len(c["levels"])
        gi += b / len(c["levels"])
    return ce, gi


def test_golden_cases_dropin_and_fused(cases):
    """Every fixture case through GT_map.Get_pred_gts + SetCriterion_TM (ABI
    phases ASSIGN, GATHER, ROWS) and through eval_loss (ASSIGN | LOSS)."""
    for c in cases:
        run_golden_case(c)


def run_golden_case(c, put=cuda):
    """One fixture case with every assertion of test_golden_cases_dropin_and_fused;
    returns the outputs as host arrays (put: how an input reaches the device)."""
    tag = f"case {c['index']}"
    args = SimpleNamespace(positive_threshold=c["pt"], negative_threshold=c["nt"],
                           ablation_no_box_regression=c["a"], focal_loss=c["focal"])
    po = [put(L["o"]) for L in c["lv"]]
    pr = [put(L["reg"]) for L in c["lv"]]
    gtb = [put(b) for b in c["boxes"]]
    ex = [put(c["exemplars"][b:b + 1]) for b in range(c["B"])]
    preds, gts, maps = tmr_amd.GT_map(args).Get_pred_gts(po, pr, gtb, ex, _batch(c))
    assert set(preds) == {"objectness", "regressions"}
    assert set(gts) == {"objectness", "regressions", "weight_objectness", "weight_regressions"}
    for lv, L in enumerate(c["lv"]):
        assert maps[lv].dtype == torch.float32 and bits_equal(maps[lv].cpu().numpy(), L["gt_map"]), tag
        assert bits_equal(preds["objectness"][lv].cpu().numpy(), L["pred_obj"]), tag
        assert bits_equal(preds["regressions"][lv].cpu().numpy(), L["pred_reg"]), tag
        assert bits_equal(gts["objectness"][lv].cpu().numpy(), L["gt_obj"]), tag
        assert bits_equal(gts["regressions"][lv].cpu().numpy(), L["gt_reg"]), tag
        assert gts["weight_objectness"][lv] is None and gts["weight_regressions"][lv] is None
    loss = tmr_amd.build_criterion(args)(preds, gts)
    assert set(loss) == {"loss_ce", "loss_giou"}
    fused = tmr_amd.TMREngine.eval_loss(
        po, pr, np.arange(c["B"]), c["exemplars"], c["boxes"], positive_threshold=c["pt"],
        negative_threshold=c["nt"], focal=c["focal"], ablation_no_box_regression=c["a"],
        regression_scaling_imgsize=c["b"], regression_scaling_WH_only=c["c"])
    rce, rgi = _ref_losses(c)
    for name, d in (("drop-in", loss), ("fused", fused)):
        for k, gold, ref in (("loss_ce", c["loss"][0], rce), ("loss_giou", c["loss"][1], rgi)):
            v = d[k]
            assert v.dtype == torch.float32 and v.dim() == 0 and not v.requires_grad
            print(f"{tag} {name} {k}: got {float(v):.9g} golden {float(gold):.9g} float64 {ref:.12g}")
            assert close(v, gold, REL), (tag, name, k, float(v), float(gold))
            assert close(v, ref, REL), (tag, name, k, float(v), ref)
    for lv, L in enumerate(c["lv"]):
        assert bits_equal(fused["gt_map"][lv].cpu().numpy(), L["gt_map"]), tag
    host_ = lambda xs: [x.cpu().numpy() for x in xs]  # noqa: E731
    return dict(maps=host_(maps), pred_obj=host_(preds["objectness"]), pred_reg=host_(preds["regressions"]),
                gt_obj=host_(gts["objectness"]), gt_reg=host_(gts["regressions"]),
                loss=[loss[k].cpu().numpy() for k in ("loss_ce", "loss_giou")],
                fused=[fused[k].cpu().numpy() for k in ("loss_ce", "loss_giou", "sums", "counts", "target")],
                fused_maps=host_(fused["gt_map"]))


# ---------------------------------------------------------------- seeded sweep
def _boxes(rng, G, H, W):
    c = rng.uniform(0.05, 0.95, (G, 2))
    s = rng.uniform(0.03, 0.4, (G, 2))
    b = np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)
    if G >= 3:  # the fixtures' special boxes: zero-width, duplicated, grid-aligned
        b[0, 2] = b[0, 0]
        b[G // 2] = b[1]
        g = np.array([1, 2, 5, 6], np.float32) / np.array([W, H, W, H], np.float32)
        b[G - 1] = g.astype(np.float32)
    return b


def _sweep_case(seed, H, W, G, NI, E):
    rng = np.random.default_rng(seed)
    cfg = dict(H=H, W=W, NI=NI, E=E,
               pt=(0.7, 0.5, 1.0, 0.7)[seed % 4], nt=(0.5, 0.5, 0.7, 1.0)[seed % 4],
               last=bool((seed // 2) % 2 == 0), focal=bool(seed % 2),
               a=seed % 5 == 3, b=seed % 7 == 2, c=seed % 3 == 1)
    # images with G, G-ish box counts; every image at least one box
    cfg["boxes"] = [_boxes(rng, max(1, G - 3 * i), H, W) for i in range(NI)]
    ex = []
    for _ in range(NI * E):  # exemplars of different sizes (different pads), some outside [0,1]
        c0 = rng.uniform(0.2, 0.8, 2)
        s = rng.uniform(0.08, 0.7, 2)
        ex.append(np.concatenate([c0 - s / 2, c0 + s / 2]))
    cfg["ex"] = np.asarray(ex, np.float32)
    cfg["ui"] = np.repeat(np.arange(NI), E)
    U = NI * E
    cfg["o"] = (rng.standard_normal((U, 1, H, W)) * 2).astype(np.float32)
    cfg["reg"] = (rng.standard_normal((U, 4, H, W)) * 0.5).astype(np.float32)
    return cfg


def _mode(cfg):
    return 2 if cfg["a"] else (1 if cfg["c"] else 0)


def _ref_units(cfg):
    H, W = cfg["H"], cfg["W"]
    units = host.gt_units(cfg["ex"], cfg["ui"], H, W, not cfg["a"], cfg["b"], cfg["c"])
    cls = [er.classify_image(b, H, W, cfg["pt"], cfg["nt"], cfg["last"]) for b in cfg["boxes"]]
    out = []
    for u in range(len(cfg["ui"])):
        m = int(cfg["ui"][u])
        out.append(er.unit(cfg["o"][u, 0], cfg["reg"][u], cfg["boxes"][m], cls[m], H, W, int(units["pad_x"][u]),
                           int(units["pad_y"][u]), units["scale_w"][u], units["scale_h"][u], _mode(cfg),
                           oracle.expf))
    return units, out


def _assign(cfg, units, sel=None, with_loss=True, put=cuda):
    """TMR_GT_ASSIGN | TMR_GT_LOSS over `units`, the descriptors of the maps
    `sel` (default all)."""
    sel = np.arange(len(cfg["ui"])) if sel is None else np.asarray(sel)
    return gl.assign(put(cfg["o"][sel]), None if cfg["a"] else put(cfg["reg"][sel]), units, cfg["boxes"],
                     cfg["pt"], cfg["nt"], cfg["last"], cfg["focal"], with_loss=with_loss)


SWEEP = [(H, W, G) for (H, W) in ((8, 8), (12, 20), (32, 32)) for G in (1, 2, 63, 64, 65, 255, 256, 257, 300)]
SWEEP.append((128, 128, 300))


@pytest.mark.parametrize("k", range(len(SWEEP)))
def test_sweep_against_restatement(k):
    run_sweep(k)


def run_sweep(k, put=cuda, fused=False):
    """SWEEP[k] with every assertion of test_sweep_against_restatement, and the
    same case through the fused eval_loss (the batch as one group, against the
    restatement at REL); returns the outputs as host arrays."""
    H, W, G = SWEEP[k]
    NI, E = (2, 2) if H == 128 else (1 + k % 3, 1 + (k // 3) % 3)
    cfg = _sweep_case(100 + k, H, W, G, NI, E)
    units, ref = _ref_units(cfg)
    st = _assign(cfg, units, put=put)
    obj, lab, rp, rg, counts = gl.gather(st)
    gm, tg, sums = st.gt_map.cpu().numpy(), st.target.cpu().numpy(), st.sums.cpu().numpy()
    so = ro = 0
    for u, r in enumerate(ref):
        tag = f"{SWEEP[k]} unit {u}"
        assert bits_equal(gm[u, 0], r["gt_map"]), tag
        assert np.array_equal(tg[u], r["target"]), tag
        npos, nneg = int(r["positive"].sum()), int(r["negative"].sum())
        assert counts[u].tolist() == [npos, nneg], tag
        ns, nr = npos + nneg, max(npos, 1)
        assert bits_equal(obj[so:so + ns].cpu().numpy(), r["samples"]), tag
        assert bits_equal(lab[so:so + ns].cpu().numpy(), r["labels"]), tag
        assert bits_equal(rp[ro:ro + nr].cpu().numpy(), r["pred"]), tag
        assert bits_equal(rg[ro:ro + nr].cpu().numpy(), r["gt"]), tag
        so, ro = so + ns, ro + nr
        ce = float(er.ce_terms(r["samples"], r["labels"], cfg["focal"]).sum())
        gi = float(er.giou_terms(r["pred"], r["gt"]).sum())
        assert close(sums[u, 0], ce, 1e-9) or (ce == 0.0 and sums[u, 0] == 0.0), (tag, sums[u, 0], ce)
        assert close(sums[u, 1], gi, 1e-9), (tag, sums[u, 1], gi)
    assert so == obj.shape[0] and ro == rp.shape[0]
    # the list form over the gathered lists, and the whole batch as one group
    rce, rgi = er.losses(ref, cfg["focal"])
    rows = gl.rows_loss(obj, lab, rp, rg, cfg["focal"]).cpu().numpy() / rp.shape[0]
    ce, gi = gl.group_losses(st.sums, st.counts, None)
    for got in ((rows[0], rows[1]), (ce, gi)):
        assert close(got[0], rce, REL) and close(got[1], rgi, REL), (SWEEP[k], got, rce, rgi)
    out = dict(gt_map=gm, target=tg, sums=sums, counts=counts, obj=obj.cpu().numpy(), lab=lab.cpu().numpy(),
               rp=rp.cpu().numpy(), rg=rg.cpu().numpy(), rows=rows, ce=ce.cpu().numpy(), gi=gi.cpu().numpy())
    if fused:  # the same case through the fused entry point (one level: it is the last)
        f = tmr_amd.TMREngine.eval_loss(
            put(cfg["o"]), None if cfg["a"] else put(cfg["reg"]), cfg["ui"], cfg["ex"], cfg["boxes"],
            positive_threshold=cfg["pt"], negative_threshold=cfg["nt"], focal=cfg["focal"],
            ablation_no_box_regression=cfg["a"], regression_scaling_imgsize=cfg["b"],
            regression_scaling_WH_only=cfg["c"])
        assert cfg["last"], "eval_loss treats its one level as the last"
        assert close(f["loss_ce"], rce, REL) and close(f["loss_giou"], rgi, REL), \
            (SWEEP[k], float(f["loss_ce"]), rce, float(f["loss_giou"]), rgi)
        out["fused"] = [f[n].cpu().numpy() for n in ("loss_ce", "loss_giou", "gt_map", "sums", "counts", "target")]
    return out


def test_batch_independence_and_repeat():
    """A unit's gt_map, target, counts and sums are bit-identical alone (its
    image alone) and inside a batch; two runs are bit-identical."""
    cfg = _sweep_case(7, 20, 28, 70, 3, 2)
    units, _ = _ref_units(cfg)
    a, b = _assign(cfg, units), _assign(cfg, units)
    full = [x.cpu().numpy() for x in (a.gt_map, a.target, a.counts, a.sums)]
    again = [x.cpu().numpy() for x in (b.gt_map, b.target, b.counts, b.sums)]
    for x, y in zip(full, again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for u in range(len(cfg["ui"])):
        m = int(cfg["ui"][u])
        one = dict(cfg, boxes=[cfg["boxes"][m]])
        un = units[[u]].copy()
        un["image"] = 0
        s = _assign(one, un, sel=[u])
        for x, y in zip(full, (s.gt_map, s.target, s.counts, s.sums)):
            y = y.cpu().numpy()
            assert np.array_equal(np.ascontiguousarray(x[u:u + 1]).view(np.uint8), y.view(np.uint8)), u


def _per_call(cfg, sel, images):
    """One trainer model() call's drop-in result: Get_pred_gts + criterion over
    the units `sel` (one per image of `images`)."""
    args = SimpleNamespace(positive_threshold=cfg["pt"], negative_threshold=cfg["nt"],
                           ablation_no_box_regression=cfg["a"], focal_loss=cfg["focal"])
    batch = {"regression_ablation_a": cfg["a"], "regression_ablation_b": cfg["b"],
             "regression_ablation_c": cfg["c"]}
    preds, gts, _ = tmr_amd.GT_map(args).Get_pred_gts(
        [cuda(cfg["o"][sel])], [cuda(cfg["reg"][sel])], [cfg["boxes"][m] for m in images],
        [cuda(cfg["ex"][u:u + 1]) for u in sel], batch)
    return tmr_amd.build_criterion(args)(preds, gts)


def test_grouping_matches_the_per_call_form():
    """One group per exemplar = each_step_multi_exemplars' per-call losses; one
    group for the batch = each_step's batched call.  The two forms sum the
    same fp64 terms in different orders and round once to fp32: one fp32 ulp."""
    cfg = _sweep_case(12, 16, 24, 9, 1, 3)  # one image, three exemplars
    kw = dict(positive_threshold=cfg["pt"], negative_threshold=cfg["nt"], focal=cfg["focal"],
              ablation_no_box_regression=cfg["a"], regression_scaling_imgsize=cfg["b"],
              regression_scaling_WH_only=cfg["c"])
    o, reg = cuda(cfg["o"]), cuda(cfg["reg"])
    r = tmr_amd.TMREngine.eval_loss(o, reg, cfg["ui"], cfg["ex"], cfg["boxes"], groups=[0, 1, 2], **kw)
    assert r["loss_ce"].shape == (3,) and r["loss_giou"].shape == (3,)
    for e in range(3):
        want = _per_call(cfg, [e], [0])
        for k in ("loss_ce", "loss_giou"):
            assert close(r[k][e], want[k], ULP32), (e, k, float(r[k][e]), float(want[k]))
    cfg = _sweep_case(13, 16, 24, 9, 3, 1)  # three images, one exemplar each
    kw.update(positive_threshold=cfg["pt"], negative_threshold=cfg["nt"], focal=cfg["focal"],
              ablation_no_box_regression=cfg["a"], regression_scaling_imgsize=cfg["b"],
              regression_scaling_WH_only=cfg["c"])
    r = tmr_amd.TMREngine.eval_loss(cuda(cfg["o"]), cuda(cfg["reg"]), cfg["ui"], cfg["ex"], cfg["boxes"], **kw)
    want = _per_call(cfg, [0, 1, 2], [0, 1, 2])
    for k in ("loss_ce", "loss_giou"):
        assert r[k].dim() == 0 and close(r[k], want[k], ULP32), (k, float(r[k]), float(want[k]))


def test_python_layer_refuses_bad_boxes():
    cfg = _sweep_case(5, 8, 8, 2, 2, 1)
    kw = dict(positive_threshold=0.7, negative_threshold=0.5)
    o, reg = cuda(cfg["o"]), cuda(cfg["reg"])
    with pytest.raises(tmr_amd.TMRError):  # G = 0
        tmr_amd.TMREngine.eval_loss(o, reg, cfg["ui"], cfg["ex"], [cfg["boxes"][0], np.zeros((0, 4))], **kw)
    bad = cfg["boxes"][1].copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        tmr_amd.TMREngine.eval_loss(o, reg, cfg["ui"], cfg["ex"], [cfg["boxes"][0], bad], **kw)


def test_end_to_end_at_smoke_shape():
    """Module forward -> Get_pred_gts -> criterion at smoke()'s shape (2 images
    of 32 x 16 x 16 features, 3 exemplars each), against the same steps on the
    oracle's forward maps.  The class maps do not depend on the maps' values
    and are identical; BCE is 1-Lipschitz in the logit, so |d loss_ce| <=
    sum |o_gpu - o_oracle| / num_positive (plus the two fp32 roundings of the
    returned 0-d values).  The GIoU difference is reported, not bounded."""
    cin = emb = 32
    margs = SimpleNamespace(emb_dim=emb, fusion=True, ablation_no_box_regression=False, encoder="original",
                            feature_upsample=True, no_matcher=False, template_type="roi_align", squeeze=False,
                            decoder_num_layer=1, decoder_kernel_size=3, modeltype="matching_net",
                            backbone="features", num_channels=cin, positive_threshold=0.7,
                            negative_threshold=0.5, focal_loss=False)
    model = tmr_amd.build_model(margs)
    P = oracle.reference_weights(0, cin=cin, emb=emb)
    P["objectness_head.head.0.bias"] = torch.tensor([0.5])
    model.load_state_dict(P, strict=True)
    model = model.to(DEV).eval()
    feats = synth.sam_features(1, 2, cin, 16, 16)
    ex, _ = synth.exemplar_set(2, 2, 3, 32, 32, 3, 7)
    rng = np.random.default_rng(3)
    gtb = [_boxes(rng, 6, 32, 32), _boxes(rng, 4, 32, 32)]
    batch = {"regression_ablation_a": False, "regression_ablation_b": False, "regression_ablation_c": False}
    gen, crit = tmr_amd.GT_map(margs), tmr_amd.build_criterion(margs)
    report = []
    for img in range(2):
        for e in range(3):  # trainer.py:97-104, one model() call per exemplar
            exemplars = [cuda(ex[img, e:e + 1])]
            with torch.no_grad():
                po, pr, _, _ = model(cuda(feats[img:img + 1]), exemplars)
            ro, rb, _, _ = oracle.forward_torch(torch.from_numpy(feats[img:img + 1]),
                                                [torch.from_numpy(ex[img, e:e + 1])], P)
            got = gen.Get_pred_gts(po, pr, [gtb[img]], exemplars, batch)
            want = gen.Get_pred_gts([cuda(ro[0])], [cuda(rb[0])], [gtb[img]], exemplars, batch)
            assert bits_equal(got[2][0].cpu().numpy(), want[2][0].cpu().numpy())
            assert bits_equal(got[1]["regressions"][0].cpu().numpy(), want[1]["regressions"][0].cpu().numpy())
            lg, lw = crit(got[0], got[1]), crit(want[0], want[1])
            npos = got[1]["regressions"][0].shape[0]
            d_o = float((got[0]["objectness"][0].double() - want[0]["objectness"][0].double()).abs().sum())
            d_ce = abs(float(lg["loss_ce"]) - float(lw["loss_ce"]))
            round32 = 2.0 ** -24 * (abs(float(lg["loss_ce"])) + abs(float(lw["loss_ce"])))
            report.append(f"image {img} exemplar {e}: num_positive {npos}, |d loss_ce| {d_ce:.3e} <= "
                          f"{d_o / npos:.3e}, |d loss_giou| "
                          f"{abs(float(lg['loss_giou']) - float(lw['loss_giou'])):.3e}")
            assert d_ce <= d_o / npos + round32, report[-1]
            assert np.isfinite(float(lg["loss_giou"])) and np.isfinite(float(lw["loss_giou"])), report[-1]
    print("\n".join(report))
