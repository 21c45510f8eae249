"""The token side of the SAM mask decoder in HIP (include/tmr_tokens.h;
reference utils/segment_anything/modeling/transformer.py:62-240 and
mask_decoder.py:145-159).

Everything the two-way transformer does to its 7 rows of 256 floats per prompt
between the two image-side kernels of tmr_amd/twoway.py, and the decoder's IoU
and hypernetwork MLPs, as three launches:

  ``tokens_front``: self-attention + norm1 (optional), then the folded queries
  qf of a tokens -> image attention;
  ``tokens_back``: the attention's value / output projections on the pooled
  context, the residual and its norm, the MLP + norm3 and the folded operands
  A, c, B of the image -> tokens attention (or, for the final attention, the
  norm alone);
  ``tokens_tail``: the IoU head and the M hypernetwork MLPs.

The kernels read the caller's live ``nn.Linear`` / ``nn.LayerNorm`` parameters
in place: nothing is packed, cached or version-tracked.  fp32 on a HIP device
only; there is no CPU path.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import TWOWAY_DIM, TWOWAY_HEADS, TWOWAY_ROWS, TMRError, ptr, require_gpu, stream


def _param(t, name):
    """The address of a parameter the kernels read in place."""
    if not isinstance(t, torch.Tensor):
        raise TMRError(f"tokens: {name} is missing")
    require_gpu(t, name)
    if t.dtype != torch.float32:
        raise TMRError(f"tokens: {name} must be fp32, got {t.dtype}")
    if not t.is_contiguous():
        raise TMRError(f"tokens: {name} must be contiguous (the kernels read the live parameter)")
    if t.data_ptr() % 16:
        raise TMRError(f"tokens: {name} must be 16-byte aligned")
    return t.data_ptr()


def _tensor(t, name, shape=None):
    require_gpu(t, name)
    if t.dtype != torch.float32:
        raise TMRError(f"tokens: {name} must be fp32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise TMRError(f"tokens: expected {name} {list(shape)}, got {list(t.shape)}")
    t = t.detach().contiguous()
    if t.data_ptr() % 16:
        raise TMRError(f"tokens: {name} must be 16-byte aligned")
    return t


def _linear(lin, name):
    if not isinstance(lin, nn.Linear) or lin.bias is None:
        raise TMRError(f"tokens: {name} must be an nn.Linear with a bias")
    return _lib.tok_linear(_param(lin.weight, name + ".weight"), _param(lin.bias, name + ".bias"), lin.in_features,
                           lin.out_features)


def _attn(att, name):
    if getattr(att, "num_heads", None) != TWOWAY_HEADS:
        raise TMRError(f"tokens: {name} has {getattr(att, 'num_heads', None)} heads; the kernels are built for "
                       f"{TWOWAY_HEADS}")
    return _lib.tok_attn(*(_linear(getattr(att, p, None), f"{name}.{p}") for p in ("q_proj", "k_proj", "v_proj",
                                                                                  "out_proj")))


def _norm(m, name):
    if not isinstance(m, nn.LayerNorm) or m.weight is None or m.bias is None:
        raise TMRError(f"tokens: {name} must be an affine nn.LayerNorm")
    return _lib.tok_norm(_param(m.weight, name + ".weight"), _param(m.bias, name + ".bias"), m.eps)


def check_mlp_block(mlp, name):
    """Raise TMRError unless ``mlp`` is the transformer's MLPBlock: lin1 -> ReLU -> lin2."""
    for p in ("lin1", "lin2"):
        if not isinstance(getattr(mlp, p, None), nn.Linear) or getattr(mlp, p).bias is None:
            raise TMRError(f"tokens: {name}.{p} must be an nn.Linear with a bias")
    if not isinstance(getattr(mlp, "act", None), nn.ReLU):
        raise TMRError(f"tokens: {name}.act must be nn.ReLU (the kernel computes lin2(relu(lin1(x)))), got "
                       f"{getattr(mlp, 'act', None)}")


def check_mlp3(mlp, name):
    """Raise TMRError unless ``mlp`` is the decoder's MLP with three Linear
    layers (ReLU between them) and no sigmoid on its output; returns the layers."""
    layers = getattr(mlp, "layers", None)
    if layers is None or len(layers) != 3 or not all(isinstance(m, nn.Linear) and m.bias is not None for m in layers):
        raise TMRError(f"tokens: {name} must be an MLP of three nn.Linear layers (`layers`), got {mlp}")
    if getattr(mlp, "sigmoid_output", False):
        raise TMRError(f"tokens: {name} has a sigmoid output; the kernel ends in the third Linear")
    return list(layers)


def _mlp3(mlp, name):
    return _lib.tok_mlp3(*(_linear(m, f"{name}.layers.{i}") for i, m in enumerate(check_mlp3(mlp, name))))


def _tokens(x, p):
    require_gpu(x, "queries")
    if x.dim() != 3 or x.shape[2] != TWOWAY_DIM:
        raise TMRError(f"tokens: expected queries [N, T, {TWOWAY_DIM}], got {list(x.shape)}")
    x = _tensor(x, "queries")
    return x, _tensor(p, "point_embedding", x.shape), int(x.shape[0]), int(x.shape[1])


def tokens_front(queries, point_embedding, cross_attn, self_attn=None, norm1=None, skip_pe=False):
    """tmr_tokens_front, one launch: ``(x1, qf)``.

    queries, point_embedding [N, T, 256]; with ``self_attn`` (and ``norm1``)
    x1 = norm1(Att(x, x, x)) when ``skip_pe`` else norm1(x + Att(x + p, x + p, x));
    without, x1 = x.  qf [N, 64, 256] are the folded queries of ``cross_attn``
    (tokens -> image) for x1 + p, rows t >= T zero."""
    x, p, N, T = _tokens(queries, point_embedding)
    f = dict(cross=_attn(cross_attn, "cross_attn"), has_self_attn=0, skip_pe=int(bool(skip_pe)))
    if self_attn is not None:
        f.update(self_attn=_attn(self_attn, "self_attn"), norm1=_norm(norm1, "norm1"), has_self_attn=1)
    x1 = torch.empty_like(x)
    qf = torch.empty((N, TWOWAY_ROWS, TWOWAY_DIM), device=x.device, dtype=torch.float32)
    _lib.tokens_launch("front", stream(x.device), x=ptr(x), p=ptr(p), x1=ptr(x1), qf=ptr(qf), N=N, T=T, **f)
    return x1, qf


def tokens_back(x1, point_embedding, ctx, attn, norm, mlp=None, norm3=None, next_attn=None):
    """tmr_tokens_back, one launch.

    x1 [N, T, 256] and ctx [N, 64, 256] (``twoway_pool``'s result for
    ``attn``): x2 = norm(x1 + attn.out_proj(attn.v_proj per head of ctx)).
    With ``mlp``, ``norm3`` and ``next_attn`` (image -> tokens) returns
    ``(x3, A, c, B)``: x3 = norm3(x2 + mlp(x2)) and ``twoway_update``'s folded
    operands; without them returns x2."""
    x, p, N, T = _tokens(x1, point_embedding)
    ctx = _tensor(ctx, "ctx", (N, TWOWAY_ROWS, TWOWAY_DIM))
    f = dict(t2i=_attn(attn, "attn"), norm=_norm(norm, "norm"), has_mlp=0)
    out = torch.empty_like(x)
    if mlp is None:
        _lib.tokens_launch("back", stream(x.device), x1=ptr(x), p=ptr(p), ctx=ptr(ctx), x_out=ptr(out), N=N, T=T, **f)
        return out
    check_mlp_block(mlp, "mlp")
    f.update(lin1=_linear(mlp.lin1, "mlp.lin1"), lin2=_linear(mlp.lin2, "mlp.lin2"), norm3=_norm(norm3, "norm3"),
             i2t=_attn(next_attn, "next_attn"), has_mlp=1)
    A = torch.empty((N, TWOWAY_ROWS, TWOWAY_DIM), device=x.device, dtype=torch.float32)
    B = torch.empty_like(A)
    c = torch.empty((N, TWOWAY_ROWS), device=x.device, dtype=torch.float32)
    _lib.tokens_launch("back", stream(x.device), x1=ptr(x), p=ptr(p), ctx=ptr(ctx), x_out=ptr(out), A=ptr(A), c=ptr(c),
                       B=ptr(B), N=N, T=T, **f)
    return out, A, c, B


def tokens_tail(hs, iou_head, hyper_mlps):
    """tmr_tokens_tail, one launch: ``(iou_pred [N, M], hyper_all [N, M, 32])``
    = (iou_head(hs[:, 0]), stack of hyper_mlps[i](hs[:, 1 + i])) for the
    decoder's three-layer MLPs.  Selecting a mask stays the caller's."""
    require_gpu(hs, "hs")
    if hs.dim() != 3 or hs.shape[2] != TWOWAY_DIM:
        raise TMRError(f"tokens: expected hs [N, T, {TWOWAY_DIM}], got {list(hs.shape)}")
    hs = _tensor(hs, "hs")
    N, T, M = int(hs.shape[0]), int(hs.shape[1]), len(hyper_mlps)
    if not 1 <= M <= _lib.TOKENS_MAX_MASKS or T < 1 + M:
        raise TMRError(f"tokens: {M} hypernetwork MLPs for {T} tokens (1 <= M <= {_lib.TOKENS_MAX_MASKS}, T >= 1 + M)")
    iou = _mlp3(iou_head, "iou_prediction_head")
    hyper = [_mlp3(m, f"output_hypernetworks_mlps.{i}") for i, m in enumerate(hyper_mlps)]
    iou_pred = torch.empty((N, M), device=hs.device, dtype=torch.float32)
    hyper_all = torch.empty((N, M, _lib.TOKENS_HYPER_OUT), device=hs.device, dtype=torch.float32)
    _lib.tokens_launch("tail", stream(hs.device), hs=ptr(hs), iou_pred=ptr(iou_pred), hyper_all=ptr(hyper_all), iou=iou,
                       hyper=hyper, N=N, T=T, M=M)
    return iou_pred, hyper_all
