"""GPU: the three kernels of include/tmr_tokens.h against their rules in float64
(the restatement in tests/twoway_ref.py plus three-layer MLPs in numpy),
FusedTwoWayTransformer(fuse_tokens=True) against the reference's own
TwoWayTransformer (tests/golden/twoway.npz) and against the torch token side on
the same device, tokens_tail and FusedMaskDecoder(fuse_tokens=True) against the
reference's decoder fixture (tests/golden/maskhead.npz).

The contract is the project's fp32 one: normwise (max |got - ref| / max |ref|
per output tensor) <= 1e-5, NaN patterns equal to the rule's, and a prompt's
bits independent of the batch around it."""
import functools

import numpy as np
import pytest
import torch

import guarded_alloc as ga
import maskhead_ref
import twoway_ref as R
import tmr_amd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
f32 = np.float32
TOL = 1e-5
L0, L1 = "layers.0", "layers.1"
T2I, I2T = ".cross_attn_token_to_image", ".cross_attn_image_to_token"


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def normwise(got, ref):
    """R.normwise; 0 when the rule leaves nothing finite and non-zero to compare."""
    ok = np.isfinite(ref)
    return R.normwise(got, ref) if ok.any() and np.abs(ref[ok]).max() > 0 else 0.0


@functools.lru_cache(maxsize=None)
def weights(inner, mlp_dim):
    """(state dict, its torch module on the device) for one cross-attention
    internal dimension and MLP width.  Shared and never modified."""
    sd = R.weights(1000 + inner + mlp_dim, mlp_dim=mlp_dim, downsample=256 // inner)
    return sd, R.module(sd).to(DEV)


def draws(seed, N, T):
    """x, p [N,T,256] and ctx [N,64,256] whose absent rows (t >= T) hold NaN: they are never read."""
    rng = np.random.default_rng(seed)
    x, p = rng.standard_normal((N, T, 256)).astype(f32), rng.standard_normal((N, T, 256)).astype(f32)
    ctx = rng.standard_normal((N, 64, 256)).astype(f32)
    ctx[:, (np.arange(64) % 8) >= T] = np.nan
    return x, p, ctx


# ---------------------------------------------------------------- the rules, float64
def front_ref(sd, L, mode, cross, x, p):
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    x1 = x if mode == "none" else R._tokens_front(sd, L, 0 if mode == "skip" else 1, x, p)
    return x1, R.fold_t2i(sd, cross, x1 + p)


def back_ref(sd, L, t2i, norm, mlp, x1, p, ctx):
    x1, p = np.asarray(x1, np.float64), np.asarray(p, np.float64)
    T = x1.shape[1]
    c = np.asarray(ctx, np.float64).copy()
    c[:, (np.arange(64) % 8) >= T] = 0.0  # (unfold_ctx slices them away; keep the einsum free of NaN warnings)
    x2 = R._norm(sd, norm, x1 + R.unfold_ctx(sd, t2i, c, T))
    if not mlp:
        return (x2,)
    x3 = R._mlp(sd, L, x2)
    return (x3,) + R.fold_i2t(sd, L + I2T, x3 + p, x3)


def mlp3_ref(mlp, x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, layer in enumerate(mlp.layers):
            x = x @ layer.weight.detach().cpu().numpy().astype(np.float64).T \
                + layer.bias.detach().cpu().numpy().astype(np.float64)
            if i < 2:
                x = np.maximum(x, 0)  # propagates NaN, as torch.relu
    return x


def tail_ref(iou_head, mlps, hs):
    return mlp3_ref(iou_head, hs[:, 0]), np.stack([mlp3_ref(m, hs[:, 1 + i]) for i, m in enumerate(mlps)], 1)


# ---------------------------------------------------------------- the kernels
def run_front(tr, L, mode, x, p, place=cuda):
    blk = tr.layers[int(L[-1])]
    xs, ps = place(x), place(p)
    before = (xs.clone(), ps.clone())
    if mode == "none":
        out = tmr_amd.tokens_front(xs, ps, tr.final_attn_token_to_image)
    else:
        out = tmr_amd.tokens_front(xs, ps, blk.cross_attn_token_to_image, self_attn=blk.self_attn, norm1=blk.norm1,
                                   skip_pe=mode == "skip")
    assert xs.cpu().numpy().tobytes() == before[0].cpu().numpy().tobytes()  # inputs are not modified
    assert ps.cpu().numpy().tobytes() == before[1].cpu().numpy().tobytes()
    assert tuple(out[0].shape) == x.shape and tuple(out[1].shape) == (x.shape[0], 64, 256)
    return tuple(o.cpu().numpy() for o in out)


def run_back(tr, L, mlp, x1, p, ctx, place=cuda):
    blk = tr.layers[int(L[-1])]
    xs, ps, cs = place(x1), place(p), place(ctx)
    before = [t.clone() for t in (xs, ps, cs)]
    if mlp:
        out = tmr_amd.tokens_back(xs, ps, cs, blk.cross_attn_token_to_image, blk.norm2, mlp=blk.mlp, norm3=blk.norm3,
                                  next_attn=blk.cross_attn_image_to_token)
        assert [tuple(o.shape) for o in out] == [x1.shape, (x1.shape[0], 64, 256), (x1.shape[0], 64),
                                                 (x1.shape[0], 64, 256)]
    else:
        out = (tmr_amd.tokens_back(xs, ps, cs, tr.final_attn_token_to_image, tr.norm_final_attn),)
        assert tuple(out[0].shape) == x1.shape
    for t, b in zip((xs, ps, cs), before):
        assert t.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    return tuple(o.cpu().numpy() for o in out)


def compare(names, got, ref, T, what):
    absent = (np.arange(64) % 8) >= T
    for name, g, r in zip(names, got, ref):
        assert g.shape == r.shape, (what, name)
        if g.shape[1:2] == (64,):
            assert not g[:, absent].any() and not r[:, absent].any(), (what, name)  # written as exactly 0
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, name)
        err = normwise(g, r)
        print(f"{what} {name}: {err:.3e} normwise")
        assert err <= TOL, (what, name, err)


FRONT_NAMES, BACK_NAMES = ("x1", "qf"), ("x_out", "A", "c", "B")

# N in {1, 2, 3, 5}: a lone prompt, one full 16-row tile, a half-filled second tile, several tiles;
# T in {1, 5, 7, 8}; every mode; both internal dimensions
FRONT_CASES = [(1, 7, "skip", 128), (2, 5, "pe", 256), (3, 8, "none", 128), (5, 1, "pe", 128), (3, 7, "skip", 256),
               (5, 8, "none", 256), (2, 1, "skip", 128), (5, 7, "pe", 128)]


@pytest.mark.parametrize("N,T,mode,inner", FRONT_CASES)
def test_front_equals_rule(N, T, mode, inner):
    sd, tr = weights(inner, 64)
    x, p, _ = draws(10 * N + T, N, T)
    L = L0 if mode == "skip" else L1
    cross = "final_attn_token_to_image" if mode == "none" else L + T2I
    compare(FRONT_NAMES, run_front(tr, L, mode, x, p), front_ref(sd, L, mode, cross, x, p), T,
            f"front N={N} T={T} {mode} I={inner}")


# mlp: 0 = absent (the final attention), else mlp_dim; 2048 (four chunks of hidden activations) at N = 3 only
BACK_CASES = [(1, 7, 64, 128), (2, 5, 0, 256), (3, 7, 2048, 128), (5, 8, 64, 256), (5, 1, 0, 128), (3, 8, 2048, 256),
              (2, 1, 64, 128), (5, 7, 0, 128)]


@pytest.mark.parametrize("N,T,mlp,inner", BACK_CASES)
def test_back_equals_rule(N, T, mlp, inner):
    sd, tr = weights(inner, mlp or 64)
    x1, p, ctx = draws(20 * N + T, N, T)
    t2i, norm = (L1 + T2I, L1 + ".norm2") if mlp else ("final_attn_token_to_image", "norm_final_attn")
    compare(BACK_NAMES, run_back(tr, L1, mlp, x1, p, ctx), back_ref(sd, L1, t2i, norm, mlp, x1, p, ctx), T,
            f"back N={N} T={T} mlp={mlp} I={inner}")


@functools.lru_cache(maxsize=None)
def tail_modules(hid, M=4):
    torch.manual_seed(300 + hid)
    iou = maskhead_ref.MLP(256, hid, M, 3).to(DEV).eval()
    mlps = torch.nn.ModuleList(maskhead_ref.MLP(256, hid, 32, 3) for _ in range(M)).to(DEV).eval()
    return iou, mlps


def run_tail(hid, hs, place=cuda):
    iou, mlps = tail_modules(hid)
    h = place(hs)
    before = h.clone()
    iou_pred, hyper_all = tmr_amd.tokens_tail(h, iou, mlps)
    assert h.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    assert tuple(iou_pred.shape) == (hs.shape[0], 4) and tuple(hyper_all.shape) == (hs.shape[0], 4, 32)
    return iou_pred.cpu().numpy(), hyper_all.cpu().numpy()


# N = 19: a second block of 16 prompts, partly filled; T = 5 is the smallest hs with M = 4
@pytest.mark.parametrize("N,T,hid", [(1, 7, 32), (2, 5, 256), (3, 7, 256), (5, 8, 32), (19, 7, 32), (19, 5, 256)])
def test_tail_equals_rule(N, T, hid):
    hs = np.random.default_rng(30 * N + T).standard_normal((N, T, 256)).astype(f32)
    got, ref = run_tail(hid, hs), tail_ref(*tail_modules(hid), hs)
    for name, g, r in zip(("iou_pred", "hyper_all"), got, ref):
        err = normwise(g, r)
        print(f"tail N={N} T={T} hidden={hid} {name}: {err:.3e} normwise")
        assert g.shape == r.shape and err <= TOL, (name, err)


# ---------------------------------------------------------------- bits
def all_outputs(x, p, ctx, hs, place=cuda):
    """Every output of the three kernels, every mode, as one dict of arrays."""
    _, tr = weights(128, 64)
    out = {}
    for mode, L in (("skip", L0), ("pe", L1), ("none", L1)):
        for k, v in zip(FRONT_NAMES, run_front(tr, L, mode, x, p, place)):
            out[f"front_{mode}_{k}"] = v
    for mlp in (64, 0):
        for k, v in zip(BACK_NAMES, run_back(tr, L1, mlp, x, p, ctx, place)):
            out[f"back_{mlp}_{k}"] = v
    for hid in (32, 256):
        for k, v in zip(("iou_pred", "hyper_all"), run_tail(hid, hs, place)):
            out[f"tail_{hid}_{k}"] = v
    return out


def test_alone_equals_batch():
    """Prompt 1 of a batch of 5 (the second half of a 16-row tile) against the
    same prompt alone (the first half, the second empty): the same bits."""
    x, p, ctx = draws(41, 5, 7)
    hs = np.random.default_rng(42).standard_normal((5, 7, 256)).astype(f32)
    batch = all_outputs(x, p, ctx, hs)
    for n in (1, 4):
        one = all_outputs(x[n:n + 1], p[n:n + 1], ctx[n:n + 1], hs[n:n + 1])
        assert set(one) == set(batch)
        for k in batch:
            assert one[k][0].tobytes() == batch[k][n].tobytes(), (k, n)
    again = all_outputs(x, p, ctx, hs)
    for k in batch:
        assert again[k].tobytes() == batch[k].tobytes(), k


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_stays_with_its_prompt(bad):
    """One NaN, then one +inf, in token 2 of prompt 1 of 3 (x, ctx and hs each):
    prompts 0 and 2 keep the clean run's bits, prompt 1's NaN pattern is the
    float64 rule's.  In the tail the value goes through both ReLUs: a ReLU that
    dropped a NaN (fmaxf) would return finite numbers where the rule has NaN."""
    N, T = 3, 7
    sd, tr = weights(128, 64)
    x, p, ctx = draws(51, N, T)
    hs = np.random.default_rng(52).standard_normal((N, T, 256)).astype(f32)
    clean = all_outputs(x, p, ctx, hs)
    xb, cb, hb = x.copy(), ctx.copy(), hs.copy()
    xb[1, 2, 5] = bad
    cb[1, 8 * 3 + 2, 7] = bad
    hb[1, 2, 100] = bad  # token 2 = hypernetwork 1's input
    hb[1, 0, 3] = bad  # and the IoU head's
    dirty = all_outputs(xb, p, cb, hb)
    for k in clean:
        for n in (0, 2):
            assert dirty[k][n].tobytes() == clean[k][n].tobytes(), (k, n)
    ref = {}
    for mode, L in (("skip", L0), ("pe", L1), ("none", L1)):
        cross = "final_attn_token_to_image" if mode == "none" else L + T2I
        ref.update(zip((f"front_{mode}_{k}" for k in FRONT_NAMES), front_ref(sd, L, mode, cross, xb, p)))
    ref.update(zip((f"back_64_{k}" for k in BACK_NAMES), back_ref(sd, L1, L1 + T2I, L1 + ".norm2", 64, xb, p, cb)))
    ref["back_0_x_out"] = back_ref(sd, L1, "final_attn_token_to_image", "norm_final_attn", 0, xb, p, cb)[0]
    for hid in (32, 256):
        ref.update(zip((f"tail_{hid}_{k}" for k in ("iou_pred", "hyper_all")), tail_ref(*tail_modules(hid), hb)))
    assert set(ref) == set(dirty)
    for k in sorted(ref):
        assert np.array_equal(np.isnan(dirty[k]), np.isnan(ref[k])), k
        assert normwise(dirty[k], ref[k]) <= TOL, k
    # what the pattern is: self-attention spreads a token's value over its prompt; without it the token
    # keeps it (an infinity may stay one where every term of a sum has its sign, so "not finite" here)
    nf = lambda k: ~np.isfinite(dirty[k][1])  # noqa: E731
    assert np.isnan(dirty["front_skip_x1"][1]).all() and nf("front_pe_qf")[(np.arange(64) % 8) < T].all()
    assert np.array_equal(nf("front_none_qf").all(1), (np.arange(64) % 8) == 2)
    assert np.array_equal(nf("front_none_qf").any(1), (np.arange(64) % 8) == 2)
    assert np.array_equal(np.isnan(dirty["back_64_x_out"][1]).all(1), np.arange(T) == 2)
    assert np.array_equal(np.isnan(dirty["back_64_x_out"][1]).any(1), np.arange(T) == 2)
    assert np.array_equal(np.isnan(dirty["back_64_c"][1]), (np.arange(64) % 8) == 2)
    for hid in (32, 256):
        assert nf(f"tail_{hid}_iou_pred").all()
        assert np.array_equal(nf(f"tail_{hid}_hyper_all").all(1), np.arange(4) == 1)
        assert np.array_equal(nf(f"tail_{hid}_hyper_all").any(1), np.arange(4) == 1)


def module_inputs(seed, N, h=5, w=7, T=7):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(1, 256, h, w, generator=gen).to(DEV), torch.randn(1, 256, h, w, generator=gen).to(DEV),
            torch.randn(N, T, 256, generator=gen).to(DEV))


def test_under_guarded_allocator():
    """The three kernels (every mode, a half-filled tile) and one fuse_tokens
    forward: the same bits unpatched, zero- and 0xFF-poisoned, and no guard
    byte written (outputs and the tests' own inputs are all guarded)."""
    x, p, ctx = draws(61, 3, 7)
    hs = np.random.default_rng(62).standard_normal((3, 7, 256)).astype(f32)
    x5, p5, ctx5 = draws(63, 2, 5)
    fused = tmr_amd.FusedTwoWayTransformer(weights(128, 64)[1], fuse_tokens=True)
    emb, pe, pts = (t.cpu().numpy() for t in module_inputs(64, 3))

    def flow(a):
        place = lambda v: a.place(np.ascontiguousarray(v))  # noqa: E731
        out = all_outputs(x, p, ctx, hs, place)
        out.update({"t5_" + k: v for k, v in all_outputs(x5, p5, ctx5, hs[:2, :5], place).items()})
        with torch.no_grad():
            hs_f, keys_f = fused.forward_shared(place(emb), place(pe), place(pts))
        out["module_hs"], out["module_keys"] = hs_f.cpu().numpy(), keys_f.cpu().numpy()
        return out

    with ga.context(None, DEV) as a:
        plain = flow(a)
    for poison in (ga.POISON_ZERO, ga.POISON_FF):
        with ga.GuardedAlloc(poison, DEV) as a:
            out = flow(a)
            assert len(a.records) > 0
            a.check()
        assert set(out) == set(plain)
        for k in plain:
            assert out[k].tobytes() == plain[k].tobytes(), (k, hex(poison))


# ---------------------------------------------------------------- the modules
def test_module_on_fixture(golden):
    """fuse_tokens=True against the reference's own transformer, both routes,
    and against the same wrapper with the torch token side on the same device."""
    g = golden("twoway")
    tr = R.module(R.weights(int(g["seed"]))).to(DEV)
    fused, plain = tmr_amd.FusedTwoWayTransformer(tr, fuse_tokens=True), tmr_amd.FusedTwoWayTransformer(tr)
    N = g["hs"].shape[0]
    emb, pe, pts = cuda(g["image_embedding"]), cuda(g["image_pe"]), cuda(g["point_embedding"])
    with torch.no_grad():
        results = {}
        for name, m in (("tokens", fused), ("torch", plain)):
            results[name] = (m.forward_shared(emb, pe, pts), m(emb.repeat(N, 1, 1, 1), pe.repeat(N, 1, 1, 1), pts))
    assert fused.calls == plain.calls == {"shared": 1, "batched": 1, "stock": 0} and tr.calls == 0
    assert fused.token_calls == 2 and plain.token_calls == 0
    for i, route in enumerate(("forward_shared", "forward")):
        hs, keys = (t.cpu().numpy() for t in results["tokens"][i])
        hs_t, keys_t = (t.cpu().numpy() for t in results["torch"][i])
        assert hs.shape == g["hs"].shape and keys.shape == g["keys"].shape
        e1, e2 = R.normwise(hs, g["hs"]), R.normwise(keys, g["keys"])
        e3, e4 = R.normwise(hs, hs_t), R.normwise(keys, keys_t)
        print(f"{route}: vs the reference hs {e1:.3e}, keys {e2:.3e}; vs the torch token side hs {e3:.3e}, keys {e4:.3e}")
        assert max(e1, e2, e3, e4) <= TOL, route


def test_module_stock_fallbacks_unchanged():
    """Nine tokens fall through to the caller's module with fuse_tokens as without."""
    tr = weights(128, 64)[1]
    fused = tmr_amd.FusedTwoWayTransformer(tr, fuse_tokens=True)
    emb, pe, pts = module_inputs(71, 2, 4, 4, 9)
    calls = tr.calls
    with torch.no_grad():
        want = tr(emb.repeat(2, 1, 1, 1), pe.repeat(2, 1, 1, 1), pts)
        got = fused(emb.repeat(2, 1, 1, 1), pe.repeat(2, 1, 1, 1), pts)
    assert fused.calls == {"shared": 0, "batched": 0, "stock": 1} and fused.token_calls == 0 and tr.calls == calls + 2
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_tail_on_decoder_fixture(golden):
    g = golden("maskhead")
    hs = g["hs"]
    dec = maskhead_ref.decoder_from_fixture(g, cuda(hs), cuda(g["src"])).to(DEV)
    ref_iou, ref_hyper = tail_ref(dec.iou_prediction_head, dec.output_hypernetworks_mlps, hs)
    # the selection is decided by the float64 rule alone before any result is compared
    top2 = np.sort(ref_iou, 1)[:, -2:]
    gap, bound = (top2[:, 1] - top2[:, 0]).min(), 100 * TOL * np.abs(ref_iou).max()
    print(f"smallest top-two IoU gap {gap:.3e}, bound {bound:.3e}")
    assert gap > bound
    iou_pred, hyper_all = tmr_amd.tokens_tail(cuda(hs), dec.iou_prediction_head, dec.output_hypernetworks_mlps)
    e1, e2 = R.normwise(iou_pred.cpu().numpy(), ref_iou), R.normwise(hyper_all.cpu().numpy(), ref_hyper)
    print(f"tokens_tail on the fixture: iou_pred {e1:.3e}, hyper_all {e2:.3e}")
    assert e1 <= TOL and e2 <= TOL
    ids = torch.argmax(iou_pred, 1)
    assert np.array_equal(ids.cpu().numpy(), g["ids"]) and np.array_equal(np.argmax(ref_iou, 1), g["ids"])
    ar = torch.arange(hs.shape[0], device=DEV)
    assert R.normwise(hyper_all[ar, ids].cpu().numpy(), g["hyper"]) <= TOL
    assert R.normwise(iou_pred[ar, ids][:, None].cpu().numpy(), g["iou"]) <= TOL


def test_decoder_with_fused_tokens(golden):
    """The fixture's decoder around a seeded transformer: fuse_tokens=True
    against fuse_transformer=True alone, masks, iou and the boxes of the masks."""
    g = golden("maskhead")
    dec = maskhead_ref.decoder_from_fixture(g, None, None)
    dec.transformer = R.module(R.weights(81))
    dec = dec.to(DEV).eval()
    plain = tmr_amd.FusedMaskDecoder(dec, fuse_transformer=True)
    fused = tmr_amd.FusedMaskDecoder(dec, fuse_transformer=True, fuse_tokens=True)
    args = [cuda(g["in_" + k]) for k in ("image_embeddings", "image_pe", "sparse_prompt_embeddings",
                                         "dense_prompt_embeddings")]
    N = args[2].shape[0]
    shared = args[:3] + [args[3][:1].expand(N, -1, -1, -1)]  # a batch-broadcast dense embedding: the shared route
    with torch.no_grad():
        for what, a in (("batched", args), ("shared", shared)):
            want_m, want_iou = plain(*a, False)
            m, iou = fused(*a, False)
            e_m, e_i = R.normwise(m.cpu().numpy(), want_m.cpu().numpy()), R.normwise(iou.cpu().numpy(),
                                                                                     want_iou.cpu().numpy())
            print(f"{what}: masks {e_m:.3e}, iou {e_i:.3e} normwise")
            assert tuple(m.shape) == tuple(want_m.shape) and tuple(iou.shape) == (N, 1)
            assert e_m <= TOL and e_i <= TOL, what
            img = tuple(int(v) for v in g["image_size"])
            lg = cuda(np.tile(np.array([[2.0, -1.0]], f32), (N, 1)))
            boxes, want_boxes = tmr_amd.mask_boxes(m, img, lg, iou)[1], tmr_amd.mask_boxes(want_m, img, lg, want_iou)[1]
            assert torch.equal(boxes, want_boxes), what
    assert fused.transformer_calls == plain.transformer_calls == {"shared": 1, "batched": 1, "stock": 0}
    assert fused.fused_transformer.token_calls == 2 and dec.transformer.calls == 0
