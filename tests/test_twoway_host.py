"""CPU-only: the float64 restatement of the two-way transformer
(tests/twoway_ref.py) reproduces the reference's own TwoWayTransformer
(tests/golden/twoway.npz, made by tools/make_golden_twoway.py); the folded
form (both rules of include/tmr_twoway.h) equals the unfolded one; the
extension's symbol table matches the header and libtmr.so; the plans are
validated on the host; the module refuses what the kernels are not built for;
the built kernels use no private memory."""
import ctypes
import re

import numpy as np
import pytest
import torch
from torch import nn

import twoway_ref as R
import tmr_amd
from tmr_amd import _lib
from test_maskhead_host import kernel_metadata


def fixture_inputs(g, nf=False):
    N = g["point_embedding"].shape[0]
    emb = np.repeat(g["image_embedding"], N, 0)
    if nf:
        n, c, y, x = (int(v) for v in g["nf_at"])
        emb[n, c, y, x] = np.nan
    return emb, np.repeat(g["image_pe"], N, 0), g["point_embedding"]


def test_fixture_conditions(golden):
    g = golden("twoway")
    assert g["hs"].shape == (5, 7, 256) and g["keys"].shape == g["keys_layer0"].shape == (5, 48, 256)
    assert tuple(g["emb_size"]) == (6, 8) and g["image_embedding"].shape == g["image_pe"].shape == (1, 256, 6, 8)
    assert all(g[k].dtype == np.float32 for k in ("hs", "keys", "keys_layer0", "image_embedding", "point_embedding"))
    assert (g["ref_fp32_err"] <= 2e-6).all()  # the reference's own fp32 forward against its float64 one
    assert not any(k.startswith("sd_") or "weight" in k for k in g)  # the seed stands for the weights


def test_restatement_reproduces_reference(golden):
    """<= 2e-6 normwise: the bound the fixture's tool holds the reference's own
    fp32 forward to against its float64 forward."""
    g = golden("twoway")
    hs, keys, keys0 = R.transformer(R.weights(int(g["seed"])), *fixture_inputs(g))
    for name, got in (("hs", hs), ("keys", keys), ("keys_layer0", keys0)):
        err = R.normwise(g[name], got)
        print(f"float64 restatement vs the reference's fp32 {name}: {err:.3e} normwise")
        assert err <= 2e-6, name


def test_restatement_reproduces_nan_pattern(golden):
    g = golden("twoway")
    hs, keys, _ = R.transformer(R.weights(int(g["seed"])), *fixture_inputs(g, nf=True))
    n = int(g["nf_at"][0])
    others = [i for i in range(hs.shape[0]) if i != n]
    assert np.isnan(hs[n]).all() and np.isnan(keys[n]).all()
    assert np.isfinite(hs[others]).all() and np.isfinite(keys[others]).all()
    assert R.normwise(g["hs"][others], hs[others]) <= 2e-6 and R.normwise(g["keys"][others], keys[others]) <= 2e-6


@pytest.mark.parametrize("shared", [True, False])
def test_folded_equals_unfolded(golden, shared):
    """Float64 on both sides: the folding is algebra, so the two differ by
    rounding alone (<= 1e-12 normwise)."""
    g = golden("twoway")
    sd = R.weights(int(g["seed"]))
    emb, pe, pts = fixture_inputs(g)
    want = R.transformer(sd, emb, pe, pts)
    got = R.transformer_folded(sd, g["image_embedding"] if shared else emb, g["image_pe"], pts)
    for name, a, b in zip(("hs", "keys", "keys_layer0"), got, want):
        err = R.normwise(a, b)
        print(f"folded vs unfolded {name}: {err:.3e}")
        assert err <= 1e-12, name
    got = R.transformer_folded(sd, *fixture_inputs(g, nf=True)[:1], g["image_pe"], pts)
    want = R.transformer(sd, *fixture_inputs(g, nf=True))
    for a, b in zip(got[:2], want[:2]):
        assert np.array_equal(np.isnan(a), np.isnan(b))


def test_k_proj_bias_cancels(golden):
    """The k_proj bias adds one constant per row to every pixel's score: the
    softmax of the pooling rule does not see it."""
    g = golden("twoway")
    sd = R.weights(int(g["seed"]))
    rng = np.random.default_rng(5)
    q = rng.standard_normal((3, 7, 256))
    keys, pe = rng.standard_normal((3, 48, 256)), rng.standard_normal((48, 256))
    name = "layers.1.cross_attn_token_to_image"
    qf, const = R.fold_t2i(sd, name, q, drop_k_bias=False)
    assert np.abs(const).max() > 0.05  # a bias that would matter
    got = R.unfold_ctx(sd, name, R.pool_rule(keys, pe, qf, 7), 7)
    want = R.attention(sd, name, q, keys + pe, keys)
    assert R.normwise(got, want) <= 1e-12
    s = np.einsum("njc,npc->njp", qf, keys + pe)
    assert R.normwise(R.softmax(s + const[:, :, None], 2), R.softmax(s, 2)) <= 1e-12


def test_torch_module_reproduces_reference(golden):
    """The tests' own torch module (what FusedTwoWayTransformer wraps on the
    GPU) gives the reference's results on the CPU."""
    g = golden("twoway")
    tr = R.module(R.weights(int(g["seed"])))
    with torch.no_grad():
        hs, keys = tr(*(torch.from_numpy(a) for a in fixture_inputs(g)))
    assert R.normwise(hs.numpy(), g["hs"]) <= 2e-6 and R.normwise(keys.numpy(), g["keys"]) <= 2e-6


def header_symbols():
    txt = open(_lib.TWOWAY_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tmr_[a-z0-9_]+)\s*\(", txt)))


def test_extension_symbols():
    syms = header_symbols()
    assert syms == ["tmr_twoway_pool", "tmr_twoway_pool_plan", "tmr_twoway_update", "tmr_twoway_update_plan"]
    assert set(syms) == set(_lib.TWOWAY_SIGNATURES), "ctypes table out of sync with tmr_twoway.h"
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.COCO_SIGNATURES, _lib.MASKHEAD_SIGNATURES):
        assert not set(syms) & set(other), "the extension has its own table"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    L = tmr_amd.load()
    assert L.tmr_twoway_pool.argtypes is not None and L.tmr_version() == 3
    assert ctypes.sizeof(_lib.TwoWayPoolArgs) == 80 and ctypes.sizeof(_lib.TwoWayUpdateArgs) == 112
    assert ctypes.sizeof(_lib.TwoWayPlan) == 32
    txt = open(_lib.TWOWAY_HEADER).read()
    assert "#define TMR_TWOWAY_POOL_CHUNK %d\n" % _lib.TWOWAY_POOL_CHUNK in txt.replace("   /*", "\n/*")
    assert "#define TMR_TWOWAY_ROWS %d " % _lib.TWOWAY_ROWS in txt
    for code, name in _lib.TWOWAY_VARIANTS.items():
        assert re.search(r"#define TMR_TWOWAY_VARIANT_%s %d\b" % (name.upper(), code), txt)
    # TMR_TWOWAY_POOL_WORK_BYTES: per (prompt, chunk) 64 rows of 256 + 2 floats
    assert _lib.twoway_pool_work_bytes(50, 4096) == 50 * 8 * 64 * 258 * 4
    assert _lib.twoway_pool_work_bytes(1, 1) == 64 * 258 * 4 and _lib.twoway_pool_work_bytes(3, 513) == 3 * 2 * 64 * 258 * 4


FAKE = 4096  # a non-null, 16-B aligned address: a plan dereferences nothing
POOL_BUFS = {k: FAKE for k in ("keys", "pe", "qf", "ctx", "work")}
UPD_BUFS = dict({k: FAKE for k in ("keys_in", "pe", "A", "c", "B", "bo", "g", "beta")}, keys_out=2 * FAKE)


def test_pool_plan_no_gpu():
    plan, rc = _lib.twoway_pool_plan, _lib.twoway_pool_plan_rc
    base = {"variant": "f32mfma", "tile_pixels": 32, "chunk_pixels": 512, "threads": 256, "lds_bytes": 66560}
    assert plan(P=4096, T=7) == dict(base, chunks=8, blocks=0)
    assert plan(P=1, T=1) == dict(base, chunks=1, blocks=0)
    assert plan(P=512, T=8) == dict(base, chunks=1, blocks=0) and plan(P=513, T=8)["chunks"] == 2
    assert plan(P=4096, T=7, N=50, **POOL_BUFS) == dict(base, chunks=8, blocks=400)
    assert plan(P=4096, T=7, N=50, Nk=1, **POOL_BUFS) == dict(base, chunks=8, blocks=400)
    # the chunking is a function of P alone
    for P in (1, 48, 513, 1027, 4096):
        got = {(plan(P=P, T=T, N=N, **POOL_BUFS)["chunks"], plan(P=P, T=T, N=N, **POOL_BUFS)["chunk_pixels"])
               for N in (1, 3, 50) for T in (1, 7, 8)}
        assert got == {((P + 511) // 512, 512)}
    assert rc(P=48, T=7, C=128) == (-3, None) and rc(P=48, T=7, H=4) == (-3, None) and rc(P=48, T=9) == (-3, None)
    assert rc(P=48, T=0) == (-1, None) and rc(P=0, T=7) == (-1, None) and rc(P=48, T=7, N=-1) == (-1, None)
    assert rc(P=(1 << 24) + 1, T=7) == (-1, None) and rc(P=1 << 24, T=7, N=128, **POOL_BUFS) == (-1, None)
    assert rc(P=1, T=7, N=(1 << 25) - 1, **POOL_BUFS)[0] == 0 and rc(P=1, T=7, N=1 << 25, **POOL_BUFS) == (-1, None)  # 64 N
    assert rc(P=48, T=7, N=5, Nk=2, **POOL_BUFS) == (-1, None) and rc(P=48, T=7, N=5, Nk=0, **POOL_BUFS) == (-1, None)
    assert rc(P=48, T=7, N=1) == (-1, None)  # null buffers with N > 0
    for k in POOL_BUFS:
        assert rc(P=48, T=7, N=1, **dict(POOL_BUFS, **{k: None})) == (-1, None), k
        assert rc(P=48, T=7, N=1, **dict(POOL_BUFS, **{k: FAKE + 4})) == (-1, None), k
    with pytest.raises(tmr_amd.TMRError):
        plan(P=0, T=7)
    with pytest.raises(tmr_amd.TMRError, match="no field"):
        plan(P=48, T=7, h=8)
    L = tmr_amd.load()
    assert L.tmr_twoway_pool_plan(None, None) == -1
    p = _lib.TwoWayPlan(7, 7, 7, 7, 7, 7, 7, 7)
    a = _lib._fill(_lib.TwoWayPoolArgs, "tmr_twoway_pool_args_t", dict(P=0, T=7, C=256, H=8, Nk=1))
    assert L.tmr_twoway_pool_plan(ctypes.byref(a), ctypes.byref(p)) == -1
    assert [getattr(p, n) for n, _ in p._fields_] == [0] * 8


def test_update_plan_no_gpu():
    plan, rc = _lib.twoway_update_plan, _lib.twoway_update_plan_rc
    base = {"variant": "f32mfma", "tile_pixels": 128, "chunk_pixels": 256, "threads": 512,
            "lds_bytes": (2 * 64 * 260 + 3 * 256) * 4}
    assert base["lds_bytes"] <= 160 * 1024
    assert plan(P=4096, T=7, eps=1e-5) == dict(base, chunks=16, blocks=0)
    assert plan(P=1, T=1) == dict(base, chunks=1, blocks=0) and plan(P=257, T=8)["chunks"] == 2
    assert plan(P=4096, T=7, N=50, **UPD_BUFS) == dict(base, chunks=16, blocks=800)
    assert plan(P=4096, T=7, N=50, Nk=1, **UPD_BUFS)["blocks"] == 800
    assert rc(P=48, T=7, C=512) == (-3, None) and rc(P=48, T=7, H=16) == (-3, None) and rc(P=48, T=9) == (-3, None)
    assert rc(P=48, T=0) == (-1, None) and rc(P=0, T=7) == (-1, None) and rc(P=48, T=7, N=-1) == (-1, None)
    assert rc(P=48, T=7, eps=-1.0) == (-1, None) and rc(P=48, T=7, eps=float("nan")) == (-1, None)
    assert rc(P=48, T=7, N=5, Nk=4, **UPD_BUFS) == (-1, None)
    assert rc(P=48, T=7, N=1) == (-1, None)
    for k in UPD_BUFS:
        assert rc(P=48, T=7, N=1, **dict(UPD_BUFS, **{k: None})) == (-1, None), k
        if k != "c":
            assert rc(P=48, T=7, N=1, **dict(UPD_BUFS, **{k: FAKE + 4})) == (-1, None), k
    # in place: only when every prompt has its own keys
    assert rc(P=48, T=7, N=5, **dict(UPD_BUFS, keys_out=FAKE))[0] == 0
    assert rc(P=48, T=7, N=1, Nk=1, **dict(UPD_BUFS, keys_out=FAKE))[0] == 0
    assert rc(P=48, T=7, N=5, Nk=1, **dict(UPD_BUFS, keys_out=FAKE)) == (-1, None)
    assert tmr_amd.load().tmr_twoway_update_plan(None, None) == -1


def test_launches_validate_no_gpu():
    """N = 0 is a no-op and bad arguments are refused before anything touches the GPU."""
    L = tmr_amd.load()

    def rc(fn, struct, **kw):
        f = dict(N=1, Nk=1, P=48, C=256, H=8, T=7)
        f.update(kw)
        return fn(ctypes.byref(_lib._fill(struct, "args", f)), None)

    for fn, struct in ((L.tmr_twoway_pool, _lib.TwoWayPoolArgs), (L.tmr_twoway_update, _lib.TwoWayUpdateArgs)):
        assert rc(fn, struct, N=0) == 0 and rc(fn, struct, N=0, Nk=0) == 0  # whatever the pointers
        assert rc(fn, struct, C=128) == -3 and rc(fn, struct, N=0, T=9) == -3 and rc(fn, struct, H=4) == -3
        assert rc(fn, struct) == -1 and rc(fn, struct, P=0) == -1 and rc(fn, struct, N=-1) == -1
        assert fn(None, None) == -1
    with pytest.raises(tmr_amd.TMRError, match="no field"):
        _lib.twoway_pool(None, bogus=1)


def test_cpu_tensors_raise():
    z = torch.zeros
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        tmr_amd.twoway_pool(z(1, 4, 256), z(4, 256), z(1, 64, 256), 7)
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        tmr_amd.twoway_update(z(1, 4, 256), z(4, 256), z(1, 64, 256), z(1, 64), z(1, 64, 256), z(256), z(256), z(256),
                              1e-5, 7)
    fused = tmr_amd.FusedTwoWayTransformer(R.TwoWayTransformer())
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        fused(z(1, 256, 2, 2), z(1, 256, 2, 2), z(1, 7, 256))
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        fused.forward_shared(z(1, 256, 2, 2), z(1, 256, 2, 2), z(1, 7, 256))


def test_refuses_other_structures():
    T = R.TwoWayTransformer
    assert isinstance(tmr_amd.FusedTwoWayTransformer(T()), nn.Module)
    assert isinstance(tmr_amd.FusedTwoWayTransformer(T(depth=3, mlp_dim=2048)), nn.Module)
    with pytest.raises(tmr_amd.TMRError, match="has embedding 128"):
        tmr_amd.FusedTwoWayTransformer(T(dim=128))
    with pytest.raises(tmr_amd.TMRError, match="has 4 heads"):
        tmr_amd.FusedTwoWayTransformer(T(heads=4))
    with pytest.raises(tmr_amd.TMRError, match="no layers"):
        tmr_amd.FusedTwoWayTransformer(nn.Identity())
    for name in ("self_attn", "norm1", "cross_attn_token_to_image", "norm2", "mlp", "norm3", "norm4",
                 "cross_attn_image_to_token", "skip_first_layer_pe"):
        tr = T()
        delattr(tr.layers[1], name)
        with pytest.raises(tmr_amd.TMRError, match=rf"layers\.1 has no {name}"):
            tmr_amd.FusedTwoWayTransformer(tr)
    for name in ("final_attn_token_to_image", "norm_final_attn"):
        tr = T()
        delattr(tr, name)
        with pytest.raises(tmr_amd.TMRError, match=f"no {name}"):
            tmr_amd.FusedTwoWayTransformer(tr)
    tr = T()
    tr.layers[0].norm4 = nn.BatchNorm1d(256)
    with pytest.raises(tmr_amd.TMRError, match=r"layers\.0\.norm4 must be an affine nn\.LayerNorm\(256\)"):
        tmr_amd.FusedTwoWayTransformer(tr)
    tr = T()
    tr.layers[0].cross_attn_image_to_token.out_proj = nn.Linear(128, 256, bias=False)
    with pytest.raises(tmr_amd.TMRError, match=r"layers\.0\.cross_attn_image_to_token\.out_proj"):
        tmr_amd.FusedTwoWayTransformer(tr)
    import maskhead_ref

    with pytest.raises(tmr_amd.TMRError, match="no layers"):  # maskhead_ref's default transformer is an Identity
        tmr_amd.FusedMaskDecoder(maskhead_ref.Decoder(), fuse_transformer=True)
    dec = tmr_amd.FusedMaskDecoder(maskhead_ref.Decoder(transformer=T()), fuse_transformer=True)
    assert dec.transformer_calls == {"shared": 0, "batched": 0, "stock": 0}
    assert tmr_amd.FusedMaskDecoder(maskhead_ref.Decoder()).transformer_calls is None


def test_kernels_use_no_private_memory():
    """No spill and no scratch in the built kernels; both main kernels within
    the 256 registers of two waves per SIMD (two pooling blocks per CU, one
    update block of 8 waves)."""
    for name, cap in (("twoway_pool_kernelENS", 256), ("twoway_update_kernelENS", 256),
                      ("twoway_pool_combine_kernel", 512)):
        md = kernel_metadata(name)
        print(name, md)
        assert md[".private_segment_fixed_size"] == 0 and md[".vgpr_spill_count"] == 0
        assert md[".sgpr_spill_count"] == 0 and md[".vgpr_count"] <= cap
