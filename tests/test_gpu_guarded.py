"""Every eager route under the poisoning, guard-banded allocator
(tests/guarded_alloc.py).

The value comparisons against the oracle are the existing tests' own (their
bodies are shared: run_config / _module_variant in test_gpu_random.py,
run_sweep / run_golden_case in test_gpu_evalloss.py, run_maxpool in
test_gpu_parity.py, check_feature_stats in test_stream.py).  New here, per flow:

(a) the flow meets those comparisons unpatched, with every package allocation
    poisoned with zero bytes, and with 0xFF bytes (NaN / -1);
(b) the SPECIFIED parts of its outputs are bit-identical across the three runs:
    a result that depends on memory nobody wrote (an element a kernel should
    have written, a buffer the caller should have zeroed) differs;
(c) no guard byte around any buffer allocated during the flow was written
    (tmr_size and the kernels' bounds agree).

Each flow is parametrised over the poison, zero first: the 0xFF run can turn a
latent read of an unwritten index into a wild address, so it follows a passed
zero run.  The unpatched and zero outputs are kept per flow for the 0xFF case
to compare against (recomputed when it runs alone).

Everything runs eagerly, because a poison fill inside a graph capture would
become part of the graph: engines get use_graphs = False before their first
call; a module's engine likewise (matching_net.engine() is built and switched
inside the context, and the module is called once); the tm_utils, gt_loss,
mapreduce and conv entry points never capture.  Engines and modules are built
inside the context, so their memo caches hold guarded tensors, and are dropped
(the flow returns host arrays only) before it exits.
"""
import numpy as np
import pytest
import torch

import guarded_alloc as ga
import oracle
import test_gpu_evalloss as T_eval
import test_gpu_parity as T_par
import test_gpu_random as T_rand
import test_stream as T_stream
import tmr_amd
from tmr_amd import mapreduce as mr
from tmr_amd import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
POISONS = [pytest.param(ga.POISON_ZERO, id="zero"), pytest.param(ga.POISON_FF, id="ff")]
_KEPT = {}  # flow key -> {"plain": outputs, "zero": outputs}


def _same_bits(a, b, path):
    """Bitwise equality of two nested outputs (dicts / lists of host arrays)."""
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same_bits(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_bits(x, y, f"{path}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, path
    else:
        x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype, (path, x.shape, y.shape, x.dtype, y.dtype)
        diff = x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8)
        assert not diff.any(), (f"{path}: {int(diff.sum())} bytes differ between two runs of the same flow, first at "
                                f"element {int(np.flatnonzero(diff)[0]) // max(x.itemsize, 1)} of {x.shape} {x.dtype}")


def _guarded_runs(key, poison, flow, verify=None):
    """flow(alloc) -> the specified outputs as host arrays.  Runs it unpatched
    (once per key) and under `poison`, asserts (c) inside the context and (b)
    against every other run kept for the key.  Assertion (a) is made by the
    flow itself where it shares an existing test's body, else by verify(out)
    on each run's outputs, after (b) and (c)."""
    kept = _KEPT.setdefault(key, {})
    fresh = []
    if "plain" not in kept:
        with ga.context(None, DEV) as a:
            kept["plain"] = flow(a)
        fresh.append(kept["plain"])
    if poison == ga.POISON_FF and "zero" not in kept:
        # alone, or after a failed zero case: the zero run comes first, and a
        # failure there ends this case before anything runs on 0xFF indices
        _guarded_runs(key, ga.POISON_ZERO, flow, verify)
    with ga.GuardedAlloc(poison, DEV) as a:
        out = flow(a)
        n = len(a.records)
        a.check()  # (c)
    assert n > 0, "the flow allocated nothing through the patched functions"
    name = "zero" if poison == ga.POISON_ZERO else "ff"
    for other, ref in kept.items():
        _same_bits(ref, out, f"{key}: {name} vs {other}")  # (b)
    if verify is not None:
        for o in fresh + [out]:
            verify(o)  # (a)
    kept[name] = out
    return out


# ------------------------------------------------------ detect + forward_units
def _eager(eng):
    eng.use_graphs = False  # nothing is captured: detect() takes its unspeculated eager route


def _mfma(eng):
    _eager(eng)
    eng.xcorr_algo = "mfma"


def _mfma_points(eng):
    _mfma(eng)
    eng.box_at_peaks = "always"


def _points(eng):
    _eager(eng)
    eng.box_at_peaks = "always"


def _dense_fallback(eng):
    """"auto" with the crossover at zero candidates: decoder_b's dense tiles
    (box_dense) whenever there is a candidate at all."""
    _eager(eng)
    eng.BOX_POINTS_CROSSOVER = {k: 0.0 for k in eng.BOX_POINTS_CROSSOVER}


# flow -> (draw() seed of the existing sweep, engine setup, expected record of the route, candidates expected)
DETECT = {
    # map 18 x 18 (W % 4 != 0: the generic VALU correlation), B 4, E 2, kmin 1
    "23": (23, _eager, dict(xcorr="valu"), False),
    # W = 64, E = 1, fp32: unshared fp half; "auto" picks the MFMA correlation; no pixel reaches cls 0.5, so
    # the points route launches nothing and every unit returns its dummy row
    "159": (159, _eager, dict(xcorr="mfma", box_route="points", points=0), False),
    # W = 64, E = 5, k <= 31, fp32: MFMA fragments, exponents, band staging
    "10": (10, _mfma, dict(xcorr="mfma"), False),
    "47": (47, _eager, dict(), False),  # W = 64, E = 4, f16
    # W = 64, bf16: one-term MFMA writing the bf16 f_TM plane, points launch
    "130": (130, _mfma_points, dict(xcorr="mfma", out16=True, box_route="points"), True),
    "141": (141, _points, dict(box_route="points"), True),  # 20 units, fp32: points launch
    "141-dense": (141, _dense_fallback, dict(box_route="dense"), True),  # the same: decoder_b's dense-tile fallback
    "78": (78, _eager, dict(), False),  # 20 units, f16
}


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", list(DETECT))
def test_detect_and_forward_units(name, poison):
    seed, setup, want, candidates = DETECT[name]
    c = T_rand.draw(seed)
    assert 2 * c["hf"] <= 48 and 2 * c["wf"] <= 64 and c["B"] * c["E"] <= 20

    def flow(a):
        r = T_rand.run_config(seed, alloc=a, setup=setup)  # (a): maps vs the oracle, detections bit-exact
        route = r["route"]
        assert route["graph"] == "eager", route
        for k, v in want.items():
            assert route[k] == v, (name, k, route)
        assert not candidates or route["points"] > 0, route  # the launch really had candidates
        return {k: r[k] for k in ("o", "b", "L", "Bx", "R")}

    _guarded_runs(f"detect{name}", poison, flow)


def test_detect_flows_cover_the_routes():
    cfg = {s: T_rand.draw(s) for s, _, _, _ in DETECT.values()}
    assert cfg[23]["wf"] * 2 % 4 != 0 and cfg[23]["precision"] == "fp32"
    assert all(cfg[s]["wf"] * 2 == 64 for s in (159, 10, 47, 130))
    assert cfg[159]["E"] == 1 and cfg[10]["E"] == 5 and cfg[10]["kmax"] == 31
    assert [cfg[s]["precision"] for s in (23, 159, 10, 47, 130, 141, 78)] == \
        ["fp32", "fp32", "fp32", "f16", "bf16", "fp32", "f16"]
    assert all(cfg[s]["B"] * cfg[s]["E"] == 20 for s in (141, 78))
    assert all(cfg[s]["emb"] == 64 for s in (159, 130, 141))  # decoder_b in whole 128-channel tiles


# --------------------------------------------------------------- module forward
# draw_variant() seeds: 35 squeeze, no upsample, 2 layers, k 5; 37 squeeze + prototype, 2 layers; 9 prototype,
# no box regression, no upsample, k 5; 14 no fusion, no box regression, k 5; 115 no_matcher, no fusion, no
# upsample, 2 layers; 51 squeeze + prototype, k 1; 146 no fusion, no upsample, 2 layers, k 1
VARIANTS = (35, 37, 9, 14, 115, 51, 146)


def _eager_module(model):
    model.engine().use_graphs = False


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("seed", VARIANTS)
def test_module_forward(seed, poison):
    def flow(a):
        r = T_rand._module_variant(seed, 1e-5, alloc=a, setup=_eager_module)  # (a)
        assert r["graph"] in (None, "eager"), r["graph"]
        return {k: r[k] for k in ("o", "b", "f_tm", "f0")}

    _guarded_runs(f"module{seed}", poison, flow)


def test_module_flows_cover_the_switches():
    v = {s: T_rand.draw_variant(s) for s in VARIANTS}
    assert v[35]["squeeze"] and not v[35]["upsample"] and v[35]["layers"] == 2 and v[35]["k"] == 5
    assert v[37]["squeeze"] and v[37]["template_type"] == "prototype" and v[37]["layers"] == 2
    assert v[9]["template_type"] == "prototype" and not v[9]["box_reg"] and not v[9]["upsample"] and v[9]["k"] == 5
    assert not v[14]["fusion"] and not v[14]["box_reg"] and v[14]["k"] == 5
    assert v[115]["no_matcher"] and not v[115]["fusion"] and not v[115]["upsample"] and v[115]["layers"] == 2
    assert v[51]["squeeze"] and v[51]["template_type"] == "prototype" and v[51]["k"] == 1
    assert not v[146]["fusion"] and not v[146]["upsample"] and v[146]["layers"] == 2 and v[146]["k"] == 1


# ------------------------------------------------- Get_pred_boxes, NMS (tm_utils)
@pytest.mark.parametrize("poison", POISONS)
def test_get_pred_boxes_with_an_empty_unit(poison):
    """3 units on a 17 x 33 map, drawn as test_get_pred_boxes_empty_units_dummy_row
    draws them: unit 1 has no peak (its row 0 holds the dummy row), units 0 and
    2 have.  Counts (the list lengths), the candidate rows below counts[u] and
    the dummy row are specified; rows past counts[u] are never read here
    (include/tmr.h, tmr_peaks_decode: "rows past counts[u] are not written")."""
    H, W = 17, 33
    prob = np.full((3, H, W), 0.05, np.float32)
    prob[0, 10, 12] = 0.9
    prob[2, 0, 0], prob[2, 16, 32], prob[2, 8, 31], prob[2, 3, 7] = 0.8, 0.95, 0.7, 0.6  # corners and the last column
    reg = synth.normal(91, (3, 4, H, W)) * 0.5
    ex = np.array([[0.1, 0.1, 0.3, 0.3], [0.2, 0.2, 0.5, 0.6], [0.4, 0.1, 0.6, 0.2]], np.float32)
    batch = {"regression_ablation_b": False, "regression_ablation_c": False}
    oL, oB, oR = oracle.get_pred_boxes_prob(list(prob), list(reg), [e[None] for e in ex], 0.5, True, False, False)
    assert [len(x) for x in oL] == [1, 1, 4]

    def flow(a):
        L, Bx, R = tmr_amd.Get_pred_boxes([a.place(prob[:, None])], [a.place(reg)], [a.place(e[None]) for e in ex],
                                          batch, 0.5, True, input_is_prob=True)
        assert all(x.dtype == torch.float32 for x in L + Bx + R)
        return dict(L=[x.cpu().numpy() for x in L], Bx=[x.cpu().numpy() for x in Bx], R=[x.cpu().numpy() for x in R])

    def verify(out):  # (a): exact
        for b in range(3):
            assert out["L"][b].shape == np.asarray(oL[b]).shape
            assert T_par.bits_equal(out["L"][b], oL[b]) and T_par.bits_equal(out["Bx"][b], oB[b]), b
            assert T_par.bits_equal(out["R"][b], oR[b]), b
        assert np.array_equal(out["Bx"][1], np.array([[0, 0, 1e-14, 1e-14]], np.float32))

    _guarded_runs("pred_boxes", poison, flow, verify)


def _nms_rows(n):
    """Rows as test_nms_random_vs_oracle draws them (ties in the scores)."""
    u = synth.uniform(n, 5 * n).reshape(n, 5).astype(np.float32)
    xy = u[:, :2] * 0.9
    bx = np.concatenate([xy, xy + 0.01 + u[:, 2:4] * 0.1], 1).astype(np.float32)
    sc = (np.round(u[:, 4] * 64) / 64).astype(np.float32)
    return bx, np.stack([sc, np.zeros_like(sc)], 1), np.ascontiguousarray(bx[:, :2])


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("sizes", [(65,), (700,), (200, 700, 65)], ids=["65", "700", "200+700+65"])
def test_nms(sizes, poison):
    """65 rows: the one-workgroup path; 700: gather + radix sort + binned
    pairs; 3 images of which one exceeds 256 rows: the binned path for all.
    Keep indices (NMS_process, want_keep) and kept rows (NMS) against
    oracle.nms, exact."""
    thr = 0.5
    rows = [_nms_rows(n) for n in sizes]
    keeps = [oracle.nms(bx, lg[:, 0], thr) for bx, lg, _ in rows]

    def flow(a):
        out = dict(keep=[], L=None, Bx=None, R=None)
        for (bx, lg, _), k in zip(rows, keeps):
            got = tmr_amd.NMS_process(a.place(bx), a.place(lg), thr)
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), k)
            out["keep"].append(got.cpu().numpy())
        L, Bx, R = tmr_amd.NMS([a.place(lg) for _, lg, _ in rows], [a.place(bx) for bx, _, _ in rows],
                               [a.place(rf) for _, _, rf in rows], thr)
        for i, ((bx, lg, rf), k) in enumerate(zip(rows, keeps)):
            assert T_par.bits_equal(L[i].cpu().numpy(), lg[k]) and T_par.bits_equal(Bx[i].cpu().numpy(), bx[k]), i
            assert T_par.bits_equal(R[i].cpu().numpy(), rf[k]), i
        out.update(L=[x.cpu().numpy() for x in L], Bx=[x.cpu().numpy() for x in Bx], R=[x.cpu().numpy() for x in R])
        return out

    _guarded_runs(f"nms{sizes}", poison, flow)


# ------------------------------------------- eval_loss, GT_map + criterion
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("shape", [(12, 20, 257), (8, 8, 1)], ids=["12x20-G257", "8x8-G1"])
def test_eval_loss_sweep_case(shape, poison):
    """gt_map, target, counts, sums, the gathered lists and the losses: all
    specified (include/tmr.h, tmr_gt_loss)."""
    k = T_eval.SWEEP.index(shape)
    _guarded_runs(f"evalloss{shape}", poison, lambda a: T_eval.run_sweep(k, put=a.place, fused=True))


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("index", range(4))
def test_eval_loss_fixture_case(index, poison, golden):
    c = T_eval.er.load_cases(golden("evalloss"))[index]
    _guarded_runs(f"evalfix{index}", poison, lambda a: T_eval.run_golden_case(c, put=a.place))


# --------------------------------------------------------- small entry points
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("shape", [(3, 7, 5, 3), (2, 8, 8, 8)])
def test_feature_stats(shape, poison):
    f = synth.sam_features(11, *shape)
    f[:, :, 0, 0] = 0.0

    def flow(a):
        got = mr.feature_stats(a.place(f))
        T_stream.check_feature_stats(f, got)
        return got

    _guarded_runs(f"stats{shape}", poison, flow)


@pytest.mark.parametrize("poison", POISONS)
def test_custom_shape_maxpool(poison):
    _guarded_runs("maxpool", poison, lambda a: T_par.run_maxpool((2, 3, 7, 9), put=a.place))


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("ttype", ["roi_align", "prototype"])
def test_standalone_template_matching(ttype, poison):
    """TemplateMatching.forward on a 29 x 37 map (W % 4 != 0) against the
    oracle's restatement of the reference module, within the fp32 contract."""
    C, H, W = 12, 29, 37
    f = synth.normal(41, (2, C, H, W))
    boxes = np.stack([synth.exemplar_box(7, H, W, 3, 11, 5), synth.exemplar_box(3, H, W, 20, 30)])
    ref = oracle.template_matching_torch(torch.from_numpy(f), [torch.from_numpy(b[None]) for b in boxes],
                                         torch.tensor([0.75]), template_type=ttype).numpy()

    def flow(a):
        m = tmr_amd.TemplateMatching(ttype).to(DEV)
        with torch.no_grad():
            m.scale.fill_(0.75)
            got = m(a.place(f), [a.place(b[None]) for b in boxes]).cpu().numpy()
        assert got.shape == ref.shape
        for b in range(2):
            assert T_par.normwise(got[b], ref[b]) <= T_par.TOL, (b, T_par.normwise(got[b], ref[b]))
        return got

    _guarded_runs(f"tm_{ttype}", poison, flow)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv2d_split(prec, poison):
    """conv2d_split at (C 40, N 72, 17 x 33, ks 3) against ATen's fp32 CPU
    conv + LeakyReLU, at test_split_conv_vs_torch's tolerances."""
    from tmr_amd.operands import conv2d_split
    C, N, H, W, ks = 40, 72, 17, 33, 3
    torch.manual_seed(C * 7 + N + ks)
    x = torch.randn(2, C, H, W)
    w = torch.randn(N, C, ks, ks) * (1.0 / (ks * C ** 0.5))
    b = torch.randn(N)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x, w, b, padding=ks // 2), 0.01).numpy()

    def flow(a):
        got = conv2d_split(a.place(x), a.place(w), a.place(b), True, prec).cpu().numpy()
        assert T_par.normwise(got, ref) <= T_par.SPLIT_TOL[prec], T_par.normwise(got, ref)
        return got

    _guarded_runs(f"conv_{prec}", poison, flow)
