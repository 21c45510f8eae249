"""GPU: the two kernels of include/tmr_twoway.h against their rules in float64
(tests/twoway_ref.py), FusedTwoWayTransformer against the reference's own
TwoWayTransformer (tests/golden/twoway.npz) and against the tests' torch module
on the same device, and FusedMaskDecoder(fuse_transformer=True) against
FusedMaskDecoder().

The contract is the project's fp32 one: normwise (max |got - ref| / max |ref|
over a call) <= 1e-5, and NaN patterns equal to the rule's.  Shapes come from
the plans: one pixel, a part of a tile, a tile and one pixel, two chunks and a
ragged third."""
import numpy as np
import pytest
import torch

import guarded_alloc as ga
import maskhead_ref
import twoway_ref as R
import tmr_amd
from tmr_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
f32 = np.float32
TOL = 1e-5


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pool_sizes():
    p = _lib.twoway_pool_plan(P=48, T=7)
    return [1, 48, p["tile_pixels"] + 1, 2 * p["chunk_pixels"] + 3]


def update_sizes():
    p = _lib.twoway_update_plan(P=48, T=7)
    return [1, 48, p["tile_pixels"] + 1, 2 * p["chunk_pixels"] + 3]


def test_plan_sizes():
    """The sizes below are the plans': a change of tiling moves the tests with it."""
    assert pool_sizes() == [1, 48, 33, 1027] and update_sizes() == [1, 48, 129, 515]
    assert _lib.twoway_pool_plan(P=1027, T=7)["chunks"] == 3 and _lib.twoway_update_plan(P=515, T=7)["chunks"] == 3


def run_pool(d, T, place=cuda):
    got = tmr_amd.twoway_pool(place(d["keys"]), place(d["pe"]), place(d["qf"]), T)
    assert got.dtype == torch.float32 and tuple(got.shape) == d["qf"].shape
    return got.cpu().numpy()


def run_update(d, T, in_place=False, place=cuda):
    keys = place(d["keys"])
    args = [place(d[k]) for k in ("pe", "A", "c", "B", "bo", "g", "beta")]
    if in_place:
        keys = keys.clone()
        got = tmr_amd.twoway_update(keys, *args, 1e-5, T, out=keys)
        assert got is keys
    else:
        before = keys.clone()
        got = tmr_amd.twoway_update(keys, *args, 1e-5, T)
        assert torch.equal(keys, before) or bool(torch.isnan(before).any())
    assert tuple(got.shape) == (d["A"].shape[0], d["keys"].shape[1], 256)
    return got.cpu().numpy()


def normwise(got, ref):
    """R.normwise; 0 when the rule leaves nothing finite and non-zero to compare (the NaN pattern is
    compared separately)."""
    ok = np.isfinite(ref)
    return R.normwise(got, ref) if ok.any() and np.abs(ref[ok]).max() > 0 else 0.0


def pool_ref(d, T):
    return R.pool_rule(d["keys"], d["pe"], d["qf"], T)


def check_pool(d, T, what=""):
    got, ref = run_pool(d, T), pool_ref(d, T)
    absent = (np.arange(64) % 8) >= T
    assert not got[:, absent].any() and not ref[:, absent].any()  # written as 0, whatever the absent rows hold
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    err = normwise(got, ref)
    print(f"pool {what}: {err:.3e} normwise")
    assert err <= TOL, (what, err)
    return got, ref


def update_ref(d, T):
    return R.update_rule(d["keys"], d["pe"], d["A"], d["c"], d["B"], d["bo"], d["g"], d["beta"], 1e-5, T)


def check_update(d, T, in_place, what=""):
    got, ref = run_update(d, T, in_place), update_ref(d, T)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    err = normwise(got, ref)
    print(f"update {what} in_place={in_place}: {err:.3e} normwise")
    assert err <= TOL, (what, err)
    return got, ref


# every P, N and T of the issue's lists, both key layouts
CASES = [(1, 0, 7), (3, 1, 5), (5, 2, 8), (3, 3, 7), (1, 3, 8), (5, 1, 5)]  # (N, index into the sizes, T)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("N,pi,T", CASES)
def test_pool_equals_rule(N, pi, T, shared):
    P = pool_sizes()[pi]
    d = R.operands(100 * N + pi, N, P, T, 1 if shared else N)
    check_pool(d, T, f"N={N} P={P} T={T} Nk={'1' if shared else 'N'}")


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("N,pi,T", CASES)
def test_update_equals_rule(N, pi, T, shared):
    P = update_sizes()[pi]
    d = R.operands(200 * N + pi, N, P, T, 1 if shared else N)
    what = f"N={N} P={P} T={T} Nk={'1' if shared else 'N'}"
    a, _ = check_update(d, T, False, what)
    if not shared or N == 1:  # in place needs every prompt's own keys
        b, _ = check_update(d, T, True, what)
        assert a.tobytes() == b.tobytes()


def test_update_in_place_needs_own_keys():
    d = R.operands(3, 3, 48, 7, 1)
    out = torch.empty(3, 48, 256, device=DEV)
    with pytest.raises(tmr_amd.TMRError):
        tmr_amd.twoway_update(cuda(d["keys"]), cuda(d["pe"]), cuda(d["A"]), cuda(d["c"]), cuda(d["B"]), cuda(d["bo"]),
                              cuda(d["g"]), cuda(d["beta"]), 1e-5, 7, out=out[:, :, :128])
    k = cuda(d["keys"])
    with pytest.raises(tmr_amd.TMRError):  # out = keys with Nk = 1 < N: wrong shape, refused before the launch
        tmr_amd.twoway_update(k, cuda(d["pe"]), cuda(d["A"]), cuda(d["c"]), cuda(d["B"]), cuda(d["bo"]),
                              cuda(d["g"]), cuda(d["beta"]), 1e-5, 7, out=k)


def test_pool_scores_span_300():
    """Scores from about -300 to +300 in every present row: exp overflows
    fp32 at 88.7, so a kernel that does not subtract the running max returns
    inf / NaN here.  The bound is the same 1e-5, so the draw must leave the
    RULE well conditioned in fp32: a score of magnitude 300 is only known to
    ~1e-4 after an fp32 dot product of 256 terms, and near-tied top scores
    would turn that into a 1e-4 relative error of their weights in ANY fp32
    evaluation (the stock module's included).  Each row j therefore gets one
    designated winner p_j (score +a_j, a_j in [200, 300]) and one designated
    loser (score -a_j); every other pixel's score is a_j * N(0, 0.09) (|.| < 110
    at 4 sd), so the winner leads by > 50 (asserted below on the float64
    scores) and the result is keys[p_j] to e^-50.  The winners are spread over
    all three chunks, so the running max rises inside chunks and the partials
    of losing chunks are scaled to 0 in the combination."""
    N, T = 3, 7
    P = pool_sizes()[3]
    d = R.operands(77, N, P, T, N)
    rng = np.random.default_rng(78)
    present = np.nonzero((np.arange(64) % 8) < T)[0]
    x = d["keys"].astype(np.float64) + d["pe"].astype(np.float64)
    chunk = _lib.twoway_pool_plan(P=P, T=T)["chunk_pixels"]
    for n in range(N):
        for i, j in enumerate(present):
            lo = (i % 3) * chunk  # the winners go round the three chunks (the last has 3 pixels)
            win = int(rng.integers(lo, min(lo + chunk, P)))
            lose = int(rng.choice(np.delete(np.arange(P), win)))
            a = rng.uniform(200.0, 300.0)
            d["qf"][n, j] = (a * (x[n, win] / (x[n, win] ** 2).sum() - x[n, lose] / (x[n, lose] ** 2).sum())).astype(f32)
    s = np.einsum("njc,npc->njp", d["qf"][:, present].astype(np.float64), x)
    top2 = np.sort(s, axis=2)[:, :, -2:]
    print(f"scores: min {s.min():.0f}, max {s.max():.0f}, smallest lead {np.min(top2[:, :, 1] - top2[:, :, 0]):.0f}")
    assert (s.max(2) > 150).all() and (s.min(2) < -150).all() and s.max() > 270 and s.min() < -270
    assert (top2[:, :, 1] - top2[:, :, 0] > 50).all()
    assert set((np.argmax(s, 2) // chunk).ravel().tolist()) == {0, 1, 2}
    got, _ = check_pool(d, T, "scores +-300")
    assert np.isfinite(got).all()


# ------------------------------------------------------------------ non-finite values
@pytest.mark.parametrize("where", ["first", "last"])
def test_pool_nan_in_keys(where):
    """A NaN in one pixel of prompt 1's keys, in the first chunk or in the
    last (ragged) tile of the last one: every present row of ctx[1] is NaN, the
    other prompts keep the contract."""
    N, T = 3, 7
    P = pool_sizes()[3]
    d = R.operands(31, N, P, T, N)
    d["keys"][1, 5 if where == "first" else P - 1, 100] = np.nan
    got, _ = check_pool(d, T, f"NaN in the {where} chunk")
    present = (np.arange(64) % 8) < T
    assert np.isnan(got[1][present]).all() and np.isfinite(got[[0, 2]]).all()


def test_pool_nan_elsewhere():
    N, T, P = 3, 5, 48
    present = (np.arange(64) % 8) < T
    d = R.operands(32, N, P, T, 1)
    d["pe"][7, 3] = np.nan  # pe reaches everyone
    got, _ = check_pool(d, T, "NaN in pe")
    assert np.isnan(got[:, present]).all()
    d = R.operands(33, N, P, T, 1)
    d["keys"][0, 40, 255] = np.nan  # so do shared keys
    got, _ = check_pool(d, T, "NaN in shared keys")
    assert np.isnan(got[:, present]).all()
    d = R.operands(34, N, P, T, N)
    d["qf"][2, 9] = np.nan  # a NaN in qf[n][j] is row j's alone, as the rule has it
    d["qf"][2, 9, 0] = 1.0
    got, _ = check_pool(d, T, "NaN in qf")
    assert np.isnan(got[2, 9]).all() and np.isfinite(np.delete(got[2], 9, 0)).all() and np.isfinite(got[:2]).all()
    d = R.operands(35, N, P, T, N)
    d["keys"][1, 11, 17] = np.inf  # an infinity: NaN wherever the rule makes NaN
    got, ref = check_pool(d, T, "inf in keys")
    assert np.isnan(ref[1]).any() and np.isfinite(got[[0, 2]]).all()


def test_update_non_finite():
    N, T = 3, 7
    P = update_sizes()[3]
    d = R.operands(41, N, P, T, N)
    d["keys"][1, 70, 9] = np.nan
    d["keys"][1, P - 1, 200] = np.inf
    d["keys"][2, 0, 0] = -np.inf
    for in_place in (False, True):
        got, _ = check_update(d, T, in_place, "non-finite x rows")
        bad = np.zeros((N, P), bool)
        bad[1, 70] = bad[1, P - 1] = bad[2, 0] = True
        assert np.array_equal(np.isnan(got).all(2), bad) and np.array_equal(np.isnan(got).any(2), bad)
    d = R.operands(42, N, 48, T, 1)
    d["pe"][13, 77] = np.nan  # a pe row: that pixel of every prompt
    got, _ = check_update(d, T, False, "NaN in pe")
    assert np.array_equal(np.isnan(got).all(2), np.isnan(got).any(2)) and np.isnan(got[:, 13]).all()
    assert np.isnan(got).all(2).sum() == N
    for key, idx in (("A", (1, 9, 4)), ("c", (1, 20)), ("B", (1, 33, 250))):
        d = R.operands(43, N, update_sizes()[2], T, 1)
        d[key][idx] = np.nan
        got, _ = check_update(d, T, False, f"NaN in {key}")
        assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all(), key


# ------------------------------------------------------------------ bits
def test_alone_equals_batch_and_reruns():
    """Prompt n alone against the batch of 5, and a call against itself: the
    same bits (the chunking depends on P alone, nothing is accumulated
    atomically)."""
    N, T = 5, 7
    for P, seed in ((pool_sizes()[3], 51), (48, 52)):
        d = R.operands(seed, N, P, T, N)
        a, b = run_pool(d, T), run_pool(d, T)
        assert a.tobytes() == b.tobytes()
        ua, ub = run_update(d, T), run_update(d, T)
        assert ua.tobytes() == ub.tobytes()
        shared = dict(d, keys=d["keys"][:1])
        sa, sua = run_pool(shared, T), run_update(shared, T)
        assert sa[0].tobytes() == a[0].tobytes() and sua[0].tobytes() == ua[0].tobytes()
        for n in (0, 3, 4):
            one = {k: (v[n:n + 1] if k in ("keys", "qf", "A", "c", "B") else v) for k, v in d.items()}
            assert run_pool(one, T)[0].tobytes() == a[n].tobytes(), (P, n)
            assert run_update(one, T)[0].tobytes() == ua[n].tobytes(), (P, n)
            one["keys"] = shared["keys"]
            assert run_pool(one, T)[0].tobytes() == sa[n].tobytes(), (P, n)


def test_kernels_under_guarded_allocator():
    """Ragged last tiles and chunks (33, 129, 1027 pixels), both key layouts: the
    same bits unpatched, zero- and 0xFF-poisoned, and no guard byte written
    (outputs, the work buffer and the tests' own inputs are all guarded)."""

    def flow(a):
        place = lambda x: a.place(np.ascontiguousarray(x))  # noqa: E731
        out = {}
        for key, (N, P, T, Nk) in (("p33", (2, 33, 7, 2)), ("p129", (3, 129, 5, 1)), ("p1027", (2, 1027, 8, 2))):
            d = R.operands(60 + P, N, P, T, Nk)
            out["pool_" + key] = run_pool(d, T, place)
            out["update_" + key] = run_update(d, T, False, place)
            if Nk == N:
                out["update_in_place_" + key] = run_update(d, T, True, place)
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


# ------------------------------------------------------------------ the module
def fixture_module(g):
    return tmr_amd.FusedTwoWayTransformer(R.module(R.weights(int(g["seed"]))).to(DEV))


def test_module_on_fixture(golden):
    g = golden("twoway")
    fused = fixture_module(g)
    N = g["hs"].shape[0]
    emb, pe, pts = cuda(g["image_embedding"]), cuda(g["image_pe"]), cuda(g["point_embedding"])
    with torch.no_grad():
        hs_s, keys_s = fused.forward_shared(emb, pe, pts)
        hs_b, keys_b = fused(emb.repeat(N, 1, 1, 1), pe.repeat(N, 1, 1, 1), pts)
        hs_e, keys_e = fused(emb.expand(N, -1, -1, -1), pe.expand(N, -1, -1, -1), pts)
    assert fused.calls == {"shared": 1, "batched": 2, "stock": 0} and fused.transformer.calls == 0
    for what, hs, keys in (("forward_shared", hs_s, keys_s), ("forward", hs_b, keys_b), ("forward, expanded", hs_e, keys_e)):
        assert tuple(hs.shape) == g["hs"].shape and tuple(keys.shape) == g["keys"].shape
        e1, e2 = R.normwise(hs.cpu().numpy(), g["hs"]), R.normwise(keys.cpu().numpy(), g["keys"])
        print(f"{what} vs the reference: hs {e1:.3e}, keys {e2:.3e}")
        assert e1 <= TOL and e2 <= TOL, what


def test_module_on_fixture_nan_record(golden):
    g = golden("twoway")
    fused = fixture_module(g)
    N = g["hs"].shape[0]
    n, c, y, x = (int(v) for v in g["nf_at"])
    emb = np.repeat(g["image_embedding"], N, 0)
    emb[n, c, y, x] = np.nan
    with torch.no_grad():
        hs, keys = fused(cuda(emb), cuda(np.repeat(g["image_pe"], N, 0)), cuda(g["point_embedding"]))
    hs, keys = hs.cpu().numpy(), keys.cpu().numpy()
    others = [i for i in range(N) if i != n]
    assert np.isnan(hs[n]).all() and np.isnan(keys[n]).all()
    assert np.isfinite(hs[others]).all() and np.isfinite(keys[others]).all()
    assert R.normwise(hs[others], g["hs"][others]) <= TOL and R.normwise(keys[others], g["keys"][others]) <= TOL


def test_module_equals_torch_module_on_device():
    """Embedding 5x7, N = 3, against the stock-structured torch module on the
    same device, both routes."""
    tr = R.module(R.weights(11)).to(DEV)
    fused = tmr_amd.FusedTwoWayTransformer(tr)
    gen = torch.Generator(device="cpu").manual_seed(12)
    emb, pe = torch.randn(1, 256, 5, 7, generator=gen).to(DEV), torch.randn(1, 256, 5, 7, generator=gen).to(DEV)
    pts = torch.randn(3, 7, 256, generator=gen).to(DEV)
    with torch.no_grad():
        want_hs, want_keys = tr(emb.repeat(3, 1, 1, 1), pe.repeat(3, 1, 1, 1), pts)
        for route in ("shared", "batched"):
            if route == "shared":
                hs, keys = fused.forward_shared(emb, pe, pts)
            else:
                hs, keys = fused(emb.repeat(3, 1, 1, 1), pe.repeat(3, 1, 1, 1), pts)
            e1 = R.normwise(hs.cpu().numpy(), want_hs.cpu().numpy())
            e2 = R.normwise(keys.cpu().numpy(), want_keys.cpu().numpy())
            print(f"{route} vs the torch module: hs {e1:.3e}, keys {e2:.3e}")
            assert e1 <= TOL and e2 <= TOL, route
    assert tr.calls == 1


@pytest.mark.parametrize("layout", ["channels_last", "1x1", "plain"])
def test_forward_leaves_its_inputs_unchanged(layout):
    """forward updates the keys in place in a copy of its own.  A channels_last
    embedding and a 1x1 embedding already have the [N, h*w, 256] layout in
    memory, so a .contiguous() of the permuted view would be the caller's own
    tensor: the inputs are the same bits afterwards, and the results the torch
    module's."""
    tr = R.module(R.weights(15)).to(DEV)
    fused = tmr_amd.FusedTwoWayTransformer(tr)
    gen = torch.Generator(device="cpu").manual_seed(16)
    h, w = (1, 1) if layout == "1x1" else (3, 5)
    emb, pe = torch.randn(3, 256, h, w, generator=gen).to(DEV), torch.randn(1, 256, h, w, generator=gen).to(DEV)
    pts = torch.randn(3, 7, 256, generator=gen).to(DEV)
    if layout == "channels_last":
        emb = emb.contiguous(memory_format=torch.channels_last)
        assert emb.permute(0, 2, 3, 1).is_contiguous()
    pe_n = pe.expand(3, -1, -1, -1)
    before = [t.clone() for t in (emb, pe, pts)]
    with torch.no_grad():
        hs, keys = fused(emb, pe_n, pts)
        assert fused.calls["batched"] == 1
        for t, b in zip((emb, pe, pts), before):
            assert torch.equal(t, b)
        assert keys.data_ptr() != emb.data_ptr()
        want_hs, want_keys = tr(emb, pe_n, pts)
    assert R.normwise(hs.cpu().numpy(), want_hs.cpu().numpy()) <= TOL
    assert R.normwise(keys.cpu().numpy(), want_keys.cpu().numpy()) <= TOL
    with torch.no_grad():  # forward_shared never writes its input either (layer 0 is out of place)
        e1 = emb[:1].clone()
        fused.forward_shared(emb[:1], pe, pts)
        assert torch.equal(emb[:1], e1)


def test_nine_tokens_fall_through():
    tr = R.module(R.weights(13)).to(DEV)
    fused = tmr_amd.FusedTwoWayTransformer(tr)
    gen = torch.Generator(device="cpu").manual_seed(14)
    emb, pe = torch.randn(1, 256, 4, 4, generator=gen).to(DEV), torch.randn(1, 256, 4, 4, generator=gen).to(DEV)
    pts = torch.randn(2, 9, 256, generator=gen).to(DEV)
    with torch.no_grad():
        want = tr(emb.repeat(2, 1, 1, 1), pe.repeat(2, 1, 1, 1), pts)
        a = fused(emb.repeat(2, 1, 1, 1), pe.repeat(2, 1, 1, 1), pts)
        b = fused.forward_shared(emb, pe, pts)
    assert fused.calls == {"shared": 0, "batched": 0, "stock": 2} and tr.calls == 3
    assert torch.equal(a[0], want[0]) and torch.equal(a[1], want[1])  # the same call of the same module
    for got, ref in zip(b, want):  # the module on expanded instead of repeated inputs
        assert R.normwise(got.cpu().numpy(), ref.cpu().numpy()) <= 1e-6


def test_fused_decoder_with_fused_transformer():
    """FusedMaskDecoder(dec, fuse_transformer=True) against FusedMaskDecoder(dec)
    on one seeded decoder: the shared route for a batch-broadcast dense
    embedding, the batched one for a materialised one."""
    torch.manual_seed(21)
    dec = maskhead_ref.Decoder(transformer=R.module(R.weights(22)))
    maskhead_ref.set_upscaling(dec.output_upscaling, maskhead_ref.weights(23))
    dec = dec.to(DEV).eval()
    plain, fused = tmr_amd.FusedMaskDecoder(dec), tmr_amd.FusedMaskDecoder(dec, fuse_transformer=True)
    N, h, w = 5, 5, 7
    gen = torch.Generator(device="cpu").manual_seed(24)
    emb, pe = torch.randn(1, 256, h, w, generator=gen).to(DEV), torch.randn(1, 256, h, w, generator=gen).to(DEV)
    sparse = torch.randn(N, 2, 256, generator=gen).to(DEV)
    dense1 = torch.randn(1, 256, h, w, generator=gen).to(DEV)
    with torch.no_grad():
        want_m, want_iou = plain(emb, pe, sparse, dense1.expand(N, -1, -1, -1), False)
        assert fused.transformer_calls == {"shared": 0, "batched": 0, "stock": 0}
        m1, iou1 = fused(emb, pe, sparse, dense1.expand(N, -1, -1, -1), False)
        assert fused.transformer_calls == {"shared": 1, "batched": 0, "stock": 0}
        m2, iou2 = fused(emb, pe, sparse, dense1.expand(N, -1, -1, -1).contiguous(), False)
        assert fused.transformer_calls == {"shared": 1, "batched": 1, "stock": 0}
        m3, _ = fused(emb, pe, sparse[:1], dense1, False)  # shape[0] == 1 is a broadcast too
        assert fused.transformer_calls == {"shared": 2, "batched": 1, "stock": 0}
    assert dec.transformer.calls == 1  # the plain decoder's call only
    assert tuple(m1.shape) == (N, 1, 4 * h, 4 * w) and tuple(iou1.shape) == (N, 1)
    for what, m, iou in (("shared", m1, iou1), ("batched", m2, iou2)):
        e_m = R.normwise(m.cpu().numpy(), want_m.cpu().numpy())
        e_i = R.normwise(iou.cpu().numpy(), want_iou.cpu().numpy())
        print(f"{what}: masks {e_m:.3e}, iou {e_i:.3e} normwise")
        assert e_m <= TOL and e_i <= TOL, what
    assert R.normwise(m3.cpu().numpy(), want_m[:1].cpu().numpy()) <= TOL
