"""CPU-only: the token-side extension (include/tmr_tokens.h): its symbol table
matches the header and libtmr.so, the plans are validated on the host, the
Python wrappers refuse what the kernels are not built for, the built kernels
use no private memory."""
import ctypes
import re

import pytest
import torch
from torch import nn

import maskhead_ref
import twoway_ref as R
import tmr_amd
from tmr_amd import _lib
from test_maskhead_host import kernel_metadata

FAKE = 4096  # a non-null, 16-B aligned address: a plan dereferences nothing


def header_symbols():
    txt = open(_lib.TOKENS_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tmr_[a-z0-9_]+)\s*\(", txt)))


def test_extension_symbols():
    syms = header_symbols()
    assert syms == ["tmr_tokens_back", "tmr_tokens_back_plan", "tmr_tokens_front", "tmr_tokens_front_plan",
                    "tmr_tokens_tail", "tmr_tokens_tail_plan"]
    assert set(syms) == set(_lib.TOKENS_SIGNATURES), "ctypes table out of sync with tmr_tokens.h"
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.COCO_SIGNATURES, _lib.MASKHEAD_SIGNATURES,
                  _lib.TWOWAY_SIGNATURES, _lib.POINTS_CHAIN_SIGNATURES):
        assert not set(syms) & set(other), "the extension has its own table"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    L = tmr_amd.load()
    assert L.tmr_tokens_front.argtypes is not None and L.tmr_version() == 3
    assert ctypes.sizeof(_lib.TokLinear) == 24 and ctypes.sizeof(_lib.TokAttn) == 96
    assert ctypes.sizeof(_lib.TokNorm) == 24 and ctypes.sizeof(_lib.TokMlp3) == 72
    assert ctypes.sizeof(_lib.TokensFrontArgs) == 32 + 96 + 24 + 96 + 8 + 24 == 280
    assert ctypes.sizeof(_lib.TokensBackArgs) == 56 + 96 + 24 + 48 + 24 + 96 + 8 + 16 == 368
    assert ctypes.sizeof(_lib.TokensTailArgs) == 24 + 72 + 8 * 72 + 8 + 16 == 696
    assert ctypes.sizeof(_lib.TokensPlan) == 24
    txt = open(_lib.TOKENS_HEADER).read()
    for name, val in (("MAX_MASKS", _lib.TOKENS_MAX_MASKS), ("HYPER_OUT", _lib.TOKENS_HYPER_OUT),
                      ("MLP_CHUNK", _lib.TOKENS_MLP_CHUNK)):
        assert re.search(r"#define TMR_TOKENS_%s %d\b" % (name, val), txt)
    for code, name in _lib.TOKENS_VARIANTS.items():
        assert re.search(r"#define TMR_TOKENS_VARIANT_%s %d\b" % (name.upper(), code), txt)
    # tmr.h and the twoway header are untouched by this extension
    assert "tokens" not in open(_lib.HEADER).read() and "tmr_tokens_" not in open(_lib.TWOWAY_HEADER).read()


# ---------------------------------------------------------------- descriptors of fake addresses
def lin(cin, cout, w=FAKE, b=FAKE):
    return _lib.tok_linear(w, b, cin, cout)


def attn(inner=128, dim=256, **kw):
    return _lib.tok_attn(lin(dim, inner, **kw), lin(dim, inner, **kw), lin(dim, inner, **kw), lin(inner, dim, **kw))


def norm(eps=1e-5, g=FAKE, b=FAKE):
    return _lib.tok_norm(g, b, eps)


def mlp3(hid, out, cin=256, **kw):
    return _lib.tok_mlp3(lin(cin, hid, **kw), lin(hid, hid, **kw), lin(hid, out, **kw))


def front_fields(T=7, N=0, inner=128, self_inner=256, sa=True, **kw):
    f = dict(T=T, N=N, cross=attn(inner), has_self_attn=int(sa), skip_pe=0)
    if sa:
        f.update(self_attn=attn(self_inner), norm1=norm())
    if N:
        f.update(x=FAKE, p=FAKE, x1=FAKE, qf=FAKE)
    f.update(kw)
    return f


def back_fields(T=7, N=0, inner=128, mlp_dim=2048, mlp=True, **kw):
    f = dict(T=T, N=N, t2i=attn(inner), norm=norm(), has_mlp=int(mlp))
    if mlp:
        f.update(lin1=lin(256, mlp_dim), lin2=lin(mlp_dim, 256), norm3=norm(), i2t=attn(inner))
    if N:
        f.update(x1=FAKE, p=FAKE, ctx=FAKE, x_out=FAKE)
        if mlp:
            f.update(A=FAKE, c=FAKE, B=FAKE)
    f.update(kw)
    return f


def tail_fields(T=7, N=0, M=4, iou_hid=256, hid=256, **kw):
    f = dict(T=T, N=N, M=M, iou=mlp3(iou_hid, M), hyper=[mlp3(hid, 32) for _ in range(M)])
    if N:
        f.update(hs=FAKE, iou_pred=FAKE, hyper_all=FAKE)
    f.update(kw)
    return f


def test_front_plan_no_gpu():
    plan, rc = _lib.tokens_plan, _lib.tokens_plan_rc
    base = {"variant": "f32mfma", "threads": 1024, "lds_bytes": 7 * 16 * 260 * 4, "prompts_per_block": 2}
    assert base["lds_bytes"] <= 160 * 1024
    assert plan("front", **front_fields()) == dict(base, blocks=0)
    for inner in (128, 256):
        for self_inner in (128, 256):
            assert plan("front", **front_fields(N=50, inner=inner, self_inner=self_inner)) == dict(base, blocks=25)
    assert plan("front", **front_fields(N=5, T=1, sa=False))["blocks"] == 3
    assert plan("front", **front_fields(N=1, T=8, skip_pe=1))["blocks"] == 1
    assert rc("front", **front_fields(T=9)) == (-3, None) and rc("front", **front_fields(C=128)) == (-3, None)
    assert rc("front", **front_fields(H=4)) == (-3, None) and rc("front", **front_fields(inner=64)) == (-3, None)
    assert rc("front", **front_fields(self_inner=64)) == (-3, None)
    assert rc("front", **front_fields(self_inner=64, has_self_attn=0))[0] == 0  # not read, not judged
    assert rc("front", **front_fields(cross=attn(128, dim=128))) == (-3, None)
    assert rc("front", **front_fields(T=0)) == (-1, None) and rc("front", **front_fields(N=-1)) == (-1, None)
    assert rc("front", **front_fields(norm1=norm(eps=-1.0))) == (-1, None)
    assert rc("front", T=7, N=1, cross=attn(), has_self_attn=0) == (-1, None)  # null buffers with N > 0
    for k in ("x", "p", "x1", "qf"):
        assert rc("front", **front_fields(N=1, **{k: None})) == (-1, None), k
        assert rc("front", **front_fields(N=1, **{k: FAKE + 4})) == (-1, None), k
    for bad in (dict(w=None), dict(w=FAKE + 4), dict(b=None), dict(b=FAKE + 8)):
        assert rc("front", **front_fields(N=1, self_attn=attn(256, **bad))) == (-1, None), bad
        assert rc("front", **front_fields(N=0, self_attn=attn(256, **bad)))[0] == 0, bad  # N = 0: whatever the pointers
    assert rc("front", **front_fields(N=1, norm1=norm(g=FAKE + 4))) == (-1, None)
    assert rc("front", **front_fields(N=1, norm1=norm(b=None))) == (-1, None)
    with pytest.raises(tmr_amd.TMRError):
        plan("front", **front_fields(T=9))
    with pytest.raises(tmr_amd.TMRError, match="no field"):
        plan("front", **front_fields(bogus=1))
    L = tmr_amd.load()
    assert L.tmr_tokens_front_plan(None, None) == -1
    p = _lib.TokensPlan(7, 7, 7, 7, 7, 7)
    a = _lib.tokens_args("front", **front_fields(T=0))
    assert L.tmr_tokens_front_plan(ctypes.byref(a), ctypes.byref(p)) == -1
    assert [getattr(p, n) for n, _ in p._fields_] == [0] * 6


def test_back_plan_no_gpu():
    plan, rc = _lib.tokens_plan, _lib.tokens_plan_rc
    base = {"variant": "f32mfma", "threads": 1024, "lds_bytes": (5 * 16 * 260 + 16 * 516) * 4, "prompts_per_block": 2}
    assert base["lds_bytes"] <= 160 * 1024
    for inner in (128, 256):
        for mlp_dim in (64, 2048, 8192):
            assert plan("back", **back_fields(N=50, inner=inner, mlp_dim=mlp_dim)) == dict(base, blocks=25)
    assert plan("back", **back_fields(N=3, mlp=False)) == dict(base, blocks=2)
    assert plan("back", **back_fields()) == dict(base, blocks=0)
    assert rc("back", **back_fields(T=9)) == (-3, None) and rc("back", **back_fields(C=128)) == (-3, None)
    assert rc("back", **back_fields(mlp_dim=100)) == (-3, None) and rc("back", **back_fields(inner=64)) == (-3, None)
    assert rc("back", **back_fields(mlp_dim=8256)) == (-3, None) and rc("back", **back_fields(mlp_dim=0)) == (-3, None)
    assert rc("back", **back_fields(mlp_dim=100, has_mlp=0))[0] == 0  # not read, not judged
    assert rc("back", **back_fields(lin2=lin(2048, 128))) == (-3, None)
    assert rc("back", **back_fields(T=0)) == (-1, None) and rc("back", **back_fields(N=-1)) == (-1, None)
    assert rc("back", **back_fields(norm=norm(eps=float("nan")))) == (-1, None)
    for k in ("x1", "p", "ctx", "x_out", "A", "c", "B"):
        assert rc("back", **back_fields(N=1, **{k: None})) == (-1, None), k
        assert rc("back", **back_fields(N=1, **{k: FAKE + 4})) == (-1, None), k
    assert rc("back", **back_fields(N=1, mlp=False))[0] == 0  # A, c, B are not written without the MLP
    assert rc("back", **back_fields(N=1, lin1=lin(256, 2048, w=None))) == (-1, None)
    assert rc("back", **back_fields(N=1, lin2=lin(2048, 256, b=FAKE + 4))) == (-1, None)
    assert rc("back", **back_fields(N=1, i2t=attn(128, w=FAKE + 4))) == (-1, None)
    assert tmr_amd.load().tmr_tokens_back_plan(None, None) == -1


def test_tail_plan_no_gpu():
    plan, rc = _lib.tokens_plan, _lib.tokens_plan_rc
    base = {"variant": "f32mfma", "threads": 1024, "lds_bytes": 3 * 16 * 260 * 4, "prompts_per_block": 16}
    for hid in (32, 256):
        assert plan("tail", **tail_fields(N=50, hid=hid, iou_hid=hid)) == dict(base, blocks=4 * 5)
    assert plan("tail", **tail_fields()) == dict(base, blocks=0)
    assert plan("tail", **tail_fields(N=16, M=8, T=9))["blocks"] == 9
    assert rc("tail", **tail_fields(hid=48)) == (-3, None) and rc("tail", **tail_fields(iou_hid=288)) == (-3, None)
    assert rc("tail", **tail_fields(C=128)) == (-3, None)
    assert rc("tail", **tail_fields(iou=mlp3(256, 3))) == (-3, None)  # the IoU head has M outputs
    assert rc("tail", **tail_fields(hyper=[mlp3(256, 16)] * 4)) == (-3, None)
    assert rc("tail", T=10, N=0, M=9, iou=mlp3(256, 9)) == (-3, None)
    assert rc("tail", **tail_fields(T=4)) == (-1, None) and rc("tail", **tail_fields(M=0)) == (-1, None)
    assert rc("tail", **tail_fields(N=-1)) == (-1, None)
    for k in ("hs", "iou_pred", "hyper_all"):
        assert rc("tail", **tail_fields(N=1, **{k: None})) == (-1, None), k
        assert rc("tail", **tail_fields(N=1, **{k: FAKE + 4})) == (-1, None), k
    assert rc("tail", **tail_fields(N=1, iou=mlp3(256, 4, b=None))) == (-1, None)
    assert rc("tail", **tail_fields(N=1, hyper=[mlp3(256, 32)] * 3 + [mlp3(256, 32, w=FAKE + 4)])) == (-1, None)
    assert tmr_amd.load().tmr_tokens_tail_plan(None, None) == -1


def test_launches_validate_no_gpu():
    """N = 0 is a no-op and bad arguments are refused before anything touches the GPU."""
    L = tmr_amd.load()
    for which, fields, fn in (("front", front_fields, L.tmr_tokens_front), ("back", back_fields, L.tmr_tokens_back),
                              ("tail", tail_fields, L.tmr_tokens_tail)):
        call = lambda **kw: fn(ctypes.byref(_lib.tokens_args(which, **fields(**kw))), None)  # noqa: E731
        assert call(N=0) == 0
        assert call(N=0, C=128) == -3 and call(N=-1) == -1
        assert call(N=1, **{"hs" if which == "tail" else "p": None}) == -1
        assert fn(None, None) == -1
    assert L.tmr_tokens_front(ctypes.byref(_lib.tokens_args("front", **front_fields(T=9))), None) == -3
    _lib.tokens_launch("back", None, **back_fields())  # N = 0 through the wrapper


# ---------------------------------------------------------------- Python refusals
def test_cpu_and_fp16_raise():
    tr = R.TwoWayTransformer()
    blk = tr.layers[0]
    z = torch.zeros
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        tmr_amd.tokens_front(z(1, 7, 256), z(1, 7, 256), blk.cross_attn_token_to_image, blk.self_attn, blk.norm1, True)
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        tmr_amd.tokens_back(z(1, 7, 256), z(1, 7, 256), z(1, 64, 256), blk.cross_attn_token_to_image, blk.norm2)
    dec = maskhead_ref.Decoder()
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        tmr_amd.tokens_tail(z(1, 7, 256), dec.iou_prediction_head, dec.output_hypernetworks_mlps)
    # parameters are judged like tensors, and named
    from tmr_amd import tokens as T

    with pytest.raises(tmr_amd.TMRError, match=r"self_attn\.q_proj\.weight must be a tensor on a HIP device"):
        T._attn(blk.self_attn, "self_attn")
    with pytest.raises(tmr_amd.TMRError, match=r"norm1\.weight"):
        T._norm(blk.norm1, "norm1")

    class OnGpu(torch.Tensor):  # the other checks come after the device check: pose as a device tensor
        is_cuda = True

    with pytest.raises(tmr_amd.TMRError, match=r"lin\.weight must be fp32, got torch\.float16"):
        T._param(torch.zeros(256, 256, dtype=torch.float16).as_subclass(OnGpu), "lin.weight")
    with pytest.raises(tmr_amd.TMRError, match=r"lin\.weight must be 16-byte aligned"):
        T._param(torch.zeros(256 * 256 + 1)[1:].view(256, 256).as_subclass(OnGpu), "lin.weight")
    with pytest.raises(tmr_amd.TMRError, match=r"lin\.weight must be contiguous"):
        T._param(torch.zeros(256, 512)[:, ::2].as_subclass(OnGpu), "lin.weight")
    with pytest.raises(tmr_amd.TMRError, match=r"queries must be fp32"):
        tmr_amd.tokens_front(torch.zeros(1, 7, 256, dtype=torch.float16).as_subclass(OnGpu), z(1, 7, 256),
                             blk.cross_attn_token_to_image)


def test_refuses_other_structures():
    T = R.TwoWayTransformer
    fused = tmr_amd.FusedTwoWayTransformer(T(), fuse_tokens=True)
    assert fused.fuse_tokens and fused.token_calls == 0 and fused.calls == {"shared": 0, "batched": 0, "stock": 0}
    plain = tmr_amd.FusedTwoWayTransformer(T())
    assert not plain.fuse_tokens and plain.token_calls == 0
    assert isinstance(tmr_amd.FusedTwoWayTransformer(T(depth=3, mlp_dim=2048), fuse_tokens=True), nn.Module)
    tr = T()
    tr.layers[1].mlp.act = nn.GELU()
    assert isinstance(tmr_amd.FusedTwoWayTransformer(tr), nn.Module)  # the torch token side runs any MLP
    with pytest.raises(tmr_amd.TMRError, match=r"layers\.1\.mlp\.act must be nn\.ReLU"):
        tmr_amd.FusedTwoWayTransformer(tr, fuse_tokens=True)
    tr = T()
    tr.layers[0].self_attn = R.Attention(256, 4)
    assert isinstance(tmr_amd.FusedTwoWayTransformer(tr), nn.Module)
    with pytest.raises(tmr_amd.TMRError, match=r"layers\.0\.self_attn has 4 heads"):
        tmr_amd.FusedTwoWayTransformer(tr, fuse_tokens=True)
    tr = T()
    tr.layers[0].mlp.lin2 = nn.Linear(64, 256, bias=False)
    with pytest.raises(tmr_amd.TMRError, match=r"layers\.0\.mlp\.lin2"):
        tmr_amd.FusedTwoWayTransformer(tr, fuse_tokens=True)

    D = maskhead_ref.Decoder
    with pytest.raises(tmr_amd.TMRError, match="fuse_tokens=True requires fuse_transformer=True"):
        tmr_amd.FusedMaskDecoder(D(transformer=T()), fuse_tokens=True)
    dec = tmr_amd.FusedMaskDecoder(D(transformer=T()), fuse_transformer=True, fuse_tokens=True)
    assert dec.fuse_tokens and dec.fused_transformer.fuse_tokens
    assert not tmr_amd.FusedMaskDecoder(D(transformer=T()), fuse_transformer=True).fused_transformer.fuse_tokens
    d = D(transformer=T())
    d.iou_prediction_head.sigmoid_output = True
    assert isinstance(tmr_amd.FusedMaskDecoder(d, fuse_transformer=True), nn.Module)
    with pytest.raises(tmr_amd.TMRError, match="iou_prediction_head has a sigmoid output"):
        tmr_amd.FusedMaskDecoder(d, fuse_transformer=True, fuse_tokens=True)
    d = D(transformer=T())
    d.output_hypernetworks_mlps[2] = maskhead_ref.MLP(256, 256, 32, 2)
    with pytest.raises(tmr_amd.TMRError, match=r"output_hypernetworks_mlps\.2 must be an MLP of three"):
        tmr_amd.FusedMaskDecoder(d, fuse_transformer=True, fuse_tokens=True)
    with pytest.raises(tmr_amd.TMRError, match=r"output_hypernetworks_mlps\.2 must be an MLP of three"):
        tmr_amd.tokens.check_mlp3(d.output_hypernetworks_mlps[2], "output_hypernetworks_mlps.2")


def test_kernels_use_no_private_memory():
    """No spill and no scratch in the three kernels; each within the 128
    registers of four waves per SIMD (one block of 16 waves per CU)."""
    for name in ("tokens_front_kernel", "tokens_back_kernel", "tokens_tail_kernel"):
        md = kernel_metadata(name)
        print(name, md)
        assert md[".private_segment_fixed_size"] == 0 and md[".vgpr_spill_count"] == 0
        assert md[".sgpr_spill_count"] == 0 and md[".vgpr_count"] <= 128
