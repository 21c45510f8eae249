"""CPU-only: the float64 restatement of the mask-head rule (tests/maskhead_ref.py)
reproduces the reference's own MaskDecoder.forward (tests/golden/maskhead.npz,
made by tools/make_golden_maskhead.py); the extension's symbol table matches
include/tmr_maskhead.h and libtmr.so; shapes are validated on the host; the
module refuses what the kernel is not built for; the built kernel uses no
private memory."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import maskhead_ref
import tmr_amd
from tmr_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_conditions(golden):
    g = golden("maskhead")
    assert g["masks"].shape == (5, 1, 24, 32) and tuple(g["emb_size"]) == (6, 8) and tuple(g["image_size"]) == (61, 93)
    assert sum(0.02 < s < 0.9 for s in g["shares"]) >= 3 and len(set(g["ids"].tolist())) >= 2
    assert g["sd_output_upscaling.0.weight"].dtype == np.float32
    w1 = g["sd_output_upscaling.0.weight"]
    assert not np.array_equal(w1.astype(np.float16).astype(np.float32), w1)  # the split's lo terms carry weight
    assert g["sd_output_hypernetworks_mlps.0.layers.0.weight"].dtype == np.float16


def test_ref_reproduces_reference(golden):
    """<= 2e-6 normwise: 5x the difference between the reference's fp32 forward
    and the float64 rule measured when the rule was written (4.3e-7)."""
    g = golden("maskhead")
    ref = maskhead_ref.ref_of(maskhead_ref.fixture_weights(g), g["src"], g["hyper"], tuple(g["emb_size"]))
    err = maskhead_ref.normwise(ref, g["masks"][:, 0])
    print(f"float64 rule vs the reference's forward: {err:.3e} normwise")
    assert err <= 2e-6


def test_ref_reproduces_nonfinite_pattern(golden):
    g = golden("maskhead")
    ref = maskhead_ref.ref_of(maskhead_ref.fixture_weights(g), g["nf_src"], g["nf_hyper"], tuple(g["emb_size"]))
    want = np.isnan(g["nf_masks"][:, 0])
    assert want.sum() == 32 and np.array_equal(np.isnan(ref), want) and np.isfinite(ref[~want]).all()
    w = int(g["emb_size"][1])
    for p in g["nf_pixels"]:
        y, x = divmod(int(p), w)
        assert want[0, 4 * y:4 * y + 4, 4 * x:4 * x + 4].all()
    assert maskhead_ref.normwise(ref, g["nf_masks"][:, 0]) <= 2e-6


def test_torch_decoder_reproduces_reference(golden):
    """The tests' own stock decoder (the module FusedMaskDecoder is compared
    with on the GPU) gives the reference's results on the CPU."""
    g = golden("maskhead")
    dec = maskhead_ref.decoder_from_fixture(g, torch.from_numpy(g["hs"]), torch.from_numpy(g["src"]))
    with torch.no_grad():
        m, iou, ids = dec.stock_head(torch.from_numpy(g["hs"]), torch.from_numpy(g["src"]), tuple(g["emb_size"]))
    assert np.array_equal(ids.numpy(), g["ids"])
    assert maskhead_ref.normwise(m.numpy(), g["masks"]) <= 1e-6 and np.abs(iou.numpy() - g["iou"]).max() <= 1e-6


def header_symbols():
    txt = open(_lib.MASKHEAD_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tmr_[a-z0-9_]+)\s*\(", txt)))


def test_extension_symbols():
    syms = header_symbols()
    assert syms == ["tmr_mask_head", "tmr_mask_head_plan", "tmr_mask_head_prep"]
    assert set(syms) == set(_lib.MASKHEAD_SIGNATURES), "ctypes table out of sync with tmr_maskhead.h"
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.COCO_SIGNATURES):
        assert not set(syms) & set(other), "the extension has its own table"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    L = tmr_amd.load()
    assert L.tmr_mask_head.argtypes is not None and L.tmr_version() == 3
    assert ctypes.sizeof(_lib.MaskHeadArgs) == 104 and ctypes.sizeof(_lib.MaskHeadPlan) == 24
    txt = open(_lib.MASKHEAD_HEADER).read()
    assert "#define TMR_MASK_HEAD_WPACK_BYTES (9 * 32768 + 64)" in txt and _lib.MASK_HEAD_WPACK_BYTES == 9 * 32768 + 64
    for code, name in _lib.MASK_HEAD_VARIANTS.items():
        assert re.search(r"#define TMR_MASK_HEAD_VARIANT_%s %d\b" % (name.upper(), code), txt)


def test_plan_no_gpu():
    plan = _lib.mask_head_plan
    base = {"variant": "mfma128", "tile_pixels": 128, "threads": 256, "lds_bytes": 65536}
    assert plan(h=64, w=64) == dict(base, tiles=32, blocks=0)
    assert plan(h=1, w=1) == dict(base, tiles=1, blocks=0)
    assert plan(h=8, w=16) == dict(base, tiles=1, blocks=0)
    assert plan(h=3, w=43) == dict(base, tiles=2, blocks=0)
    assert plan(h=16384, w=1024, N=0)["tiles"] == 131072
    fake = 4096  # a non-null, 16-B aligned address: the plan dereferences nothing
    bufs = {k: fake for k in ("src", "hyper", "wpack", "b1", "g", "beta", "b2", "masks")}
    assert plan(h=64, w=64, N=50, **bufs) == dict(base, tiles=32, blocks=1600)
    assert plan(h=5, w=7, N=51, **bufs) == dict(base, tiles=1, blocks=51)
    rc = _lib.mask_head_plan_rc
    assert rc(h=4, w=4, C=128) == (-3, None) and rc(h=4, w=4, C=512) == (-3, None)  # TMR_E_UNSUPPORTED
    assert rc(h=0, w=4) == (-1, None) and rc(h=4, w=0) == (-1, None) and rc(h=4, w=4, N=-1) == (-1, None)
    assert rc(h=16385, w=4) == (-1, None) and rc(h=4, w=1025) == (-1, None)
    assert rc(h=16384, w=1024, N=128) == (-1, None)  # N h w = 2^31
    assert rc(h=4, w=4, N=1) == (-1, None)  # null buffers with N > 0
    assert rc(h=4, w=4, N=1, **dict(bufs, masks=None)) == (-1, None)
    assert rc(h=4, w=4, N=1, **dict(bufs, src=fake + 4)) == (-1, None)  # alignment
    with pytest.raises(tmr_amd.TMRError):
        plan(h=0, w=4)
    with pytest.raises(tmr_amd.TMRError, match="no field"):
        plan(h=4, w=4, H=8)
    L = tmr_amd.load()
    assert L.tmr_mask_head_plan(None, None) == -1
    p = _lib.MaskHeadPlan(7, 7, 7, 7, 7, 7)
    a = _lib._fill(_lib.MaskHeadArgs, "tmr_mask_head_args_t", dict(h=0, w=4, C=256))
    assert L.tmr_mask_head_plan(ctypes.byref(a), ctypes.byref(p)) == -1
    assert [getattr(p, n) for n, _ in p._fields_] == [0] * 6


def test_invalid_shapes_no_gpu():
    """Shape limits are checked before anything touches the GPU."""
    L = tmr_amd.load()

    def rc(fn=L.tmr_mask_head, **kw):
        f = dict(N=1, h=4, w=4, C=256, eps=1e-6)
        f.update(kw)
        return fn(ctypes.byref(_lib._fill(_lib.MaskHeadArgs, "tmr_mask_head_args_t", f)), None)

    assert rc(N=0) == 0  # a no-op, whatever the pointers
    assert rc(C=128) == -3 and rc(N=0, C=128) == -3
    assert rc(h=0) == -1 and rc(w=0) == -1 and rc(N=-1) == -1 and rc(h=16385) == -1
    assert rc() == -1  # null buffers with N > 0
    assert L.tmr_mask_head(None, None) == -1
    assert rc(L.tmr_mask_head_prep) == -1 and rc(L.tmr_mask_head_prep, C=128) == -3
    assert L.tmr_mask_head_prep(None, None) == -1
    with pytest.raises(tmr_amd.TMRError, match="no field"):
        _lib.mask_head(None, bogus=1)


def test_cpu_tensors_raise():
    dec = maskhead_ref.Decoder()
    w = tmr_amd.mask_head_weights(dec.output_upscaling)  # the structure check needs no GPU
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        tmr_amd.mask_head(torch.zeros(1, 4, 256), torch.zeros(1, 32), w, (2, 2))
    fused = tmr_amd.FusedMaskDecoder(dec)
    with pytest.raises(tmr_amd.TMRError, match="HIP device"):
        fused(torch.zeros(1, 256, 2, 2), torch.zeros(1, 256, 2, 2), torch.zeros(1, 2, 256), torch.zeros(1, 256, 2, 2),
              False)
    with pytest.raises(tmr_amd.TMRError, match="mask_head_weights"):
        tmr_amd.mask_head(torch.zeros(1, 4, 256), torch.zeros(1, 32), dec.output_upscaling, (2, 2))


def test_fused_decoder_refuses_other_structures():
    assert isinstance(tmr_amd.FusedMaskDecoder(maskhead_ref.Decoder()), nn.Module)
    with pytest.raises(tmr_amd.TMRError, match="transformer_dim is 128"):
        tmr_amd.FusedMaskDecoder(maskhead_ref.Decoder(dim=128))
    with pytest.raises(tmr_amd.TMRError, match=r"output_upscaling\.2 must be nn\.GELU\(approximate='none'\)"):
        tmr_amd.FusedMaskDecoder(maskhead_ref.Decoder(gelu=lambda: nn.GELU(approximate="tanh")))
    dec = maskhead_ref.Decoder()
    del dec.output_upscaling
    with pytest.raises(tmr_amd.TMRError, match="no output_upscaling"):
        tmr_amd.FusedMaskDecoder(dec)
    dec = maskhead_ref.Decoder()
    dec.output_upscaling[0] = nn.ConvTranspose2d(256, 64, 2, 2, bias=False)
    with pytest.raises(tmr_amd.TMRError, match=r"output_upscaling\.0"):
        tmr_amd.FusedMaskDecoder(dec)
    dec = maskhead_ref.Decoder()
    dec.output_upscaling[1] = nn.BatchNorm2d(64)
    with pytest.raises(tmr_amd.TMRError, match=r"output_upscaling\.1"):
        tmr_amd.FusedMaskDecoder(dec)
    dec = maskhead_ref.Decoder()
    dec.output_hypernetworks_mlps[2] = maskhead_ref.MLP(256, 256, 16, 3)
    with pytest.raises(tmr_amd.TMRError, match=r"output_hypernetworks_mlps\.2 must end in 32"):
        tmr_amd.FusedMaskDecoder(dec)


def kernel_metadata(name):
    """The code object's metadata record of the kernel whose symbol holds
    `name`, read from libtmr.so: {key: int} of the integer fields that follow
    its .name (the record's keys are sorted)."""
    blob = open(_lib.LIB_PATH, "rb").read()
    hits = [m for m in re.finditer(rb"\xa5\.name[\xa0-\xbf\xd9][\x00-\xff]?(_Z[A-Za-z0-9_]+)", blob)
            if name.encode() in m.group(1)]
    assert len(hits) == 1, (name, [m.group(1) for m in hits])
    i, out = hits[0].end(), {}
    while blob[i] & 0xe0 == 0xa0 or blob[i] == 0xd9:  # the next key: a msgpack str
        n, i = (blob[i] & 0x1f, i + 1) if blob[i] != 0xd9 else (blob[i + 1], i + 2)
        key, i = blob[i:i + n].decode(), i + n
        t = blob[i]
        if t <= 0x7f:
            val, i = t, i + 1
        elif t in (0xc2, 0xc3):  # a bool (.uses_dynamic_stack)
            val, i = t == 0xc3, i + 1
        elif t in (0xcc, 0xcd, 0xce):
            size = {0xcc: 1, 0xcd: 2, 0xce: 4}[t]
            val, i = int.from_bytes(blob[i + 1:i + 1 + size], "big"), i + 1 + size
        elif t & 0xe0 == 0xa0 or t == 0xd9:  # a string value (.symbol)
            n, i = (t & 0x1f, i + 1) if t != 0xd9 else (blob[i + 1], i + 2)
            val, i = blob[i:i + n].decode(), i + n
        else:
            break
        out[key] = val
    return out


def test_kernel_uses_no_private_memory():
    """No spill and no scratch in the built mask_head_kernel; its registers fit
    the one-wave-per-SIMD budget (512 with the accumulation registers)."""
    md = kernel_metadata("mask_head_kernelENS")
    print(md)
    assert md[".private_segment_fixed_size"] == 0 and md[".vgpr_spill_count"] == 0 and md[".sgpr_spill_count"] == 0
    assert md[".vgpr_count"] <= 512
    for helper in ("mask_head_pack_kernel", "mask_head_wmax_kernel"):
        assert kernel_metadata(helper)[".private_segment_fixed_size"] == 0
