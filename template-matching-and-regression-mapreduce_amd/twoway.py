"""The image side of the SAM mask decoder's two-way transformer, fused
(reference: utils/segment_anything/modeling/transformer.py:62-240).

The stock module projects all h*w pixels of every prompt four times per layer
and makes about fifteen passes over [N, h*w, 256] tensors.  Both of its
cross-attentions fold so that the image side needs no projection weights
(include/tmr_twoway.h):

  tokens -> image is attention pooling of the RAW keys (``twoway_pool``: one
  read of keys, no K or V tensor);
  image -> tokens, its residual and norm4 are one pass (``twoway_update``:
  keys read once, written once).

Self-attention, the MLP, the token-side norms, the folding and the value /
output projections after pooling are torch ops on token-sized tensors; the
kernels see no weights, so nothing is packed or version-tracked.  With
``fuse_tokens=True`` that token side runs in HIP as well (tmr_amd/tokens.py:
``tokens_front`` and ``tokens_back`` on the live parameters), about 15 launches
per forward instead of about 120.

``FusedTwoWayTransformer`` is the drop-in for the caller's ``TwoWayTransformer``:

    decoder = FusedMaskDecoder(mask_decoder, fuse_transformer=True)

fp32 on a HIP device only; there is no CPU path.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _lib
from ._lib import TWOWAY_DIM, TWOWAY_HEADS, TWOWAY_ROWS, TMRError, ptr, require_gpu, stream

TOKENS_MAX = TWOWAY_ROWS // TWOWAY_HEADS  # 8 token slots per head


def _f32_gpu(t, name, shape=None):
    require_gpu(t, name)
    if t.dtype != torch.float32:
        raise TMRError(f"two-way transformer: {name} must be fp32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise TMRError(f"two-way transformer: expected {name} {list(shape)}, got {list(t.shape)}")
    return t.detach().contiguous()


def _keys_shape(keys, pe, N):
    if keys.dim() != 3 or keys.shape[2] != TWOWAY_DIM or keys.shape[0] not in (1, N):
        raise TMRError(f"two-way transformer: expected keys [1 or {N}, P, {TWOWAY_DIM}], got {list(keys.shape)}")
    P = int(keys.shape[1])
    if tuple(pe.shape) != (P, TWOWAY_DIM):
        raise TMRError(f"two-way transformer: expected pe [{P}, {TWOWAY_DIM}], got {list(pe.shape)}")
    return int(keys.shape[0]), P


def twoway_pool(keys, pe, qf, tokens_per_head):
    """Attention pooling of the raw keys (tmr_twoway_pool, two launches).

    keys [Nk, P, 256] with Nk = 1 (shared by every prompt) or N; pe [P, 256];
    qf [N, 64, 256], row 8 h + t, rows with t >= tokens_per_head absent (never
    read).  Returns ctx [N, 64, 256] (absent rows 0)."""
    require_gpu(qf, "qf")
    if qf.dim() != 3 or tuple(qf.shape[1:]) != (TWOWAY_ROWS, TWOWAY_DIM):
        raise TMRError(f"twoway_pool: expected qf [N, {TWOWAY_ROWS}, {TWOWAY_DIM}], got {list(qf.shape)}")
    N = int(qf.shape[0])
    require_gpu(keys, "keys")
    require_gpu(pe, "pe")
    Nk, P = _keys_shape(keys, pe, N)
    keys, pe, qf = _f32_gpu(keys, "keys"), _f32_gpu(pe, "pe"), _f32_gpu(qf, "qf")
    ctx = torch.empty_like(qf)
    work = torch.empty(max(_lib.twoway_pool_work_bytes(N, P), 16), device=qf.device, dtype=torch.uint8)
    _lib.twoway_pool(stream(qf.device), keys=ptr(keys), pe=ptr(pe), qf=ptr(qf), ctx=ptr(ctx), work=ptr(work),
                     N=N, Nk=Nk, P=P, T=int(tokens_per_head))
    return ctx


def twoway_update(keys, pe, A, c, B, bo, g, beta, eps, tokens_per_head, out=None):
    """Cross attention image -> tokens + residual + LayerNorm (tmr_twoway_update,
    one launch).

    keys [Nk, P, 256], pe [P, 256]; A, B [N, 64, 256] and c [N, 64] the folded
    token operands (row 8 h + t); bo, g, beta [256]: out_proj's bias and the
    LayerNorm's weight and bias.  ``out`` [N, P, 256] may be ``keys`` itself
    when Nk = N.  Returns out."""
    require_gpu(A, "A")
    if A.dim() != 3 or tuple(A.shape[1:]) != (TWOWAY_ROWS, TWOWAY_DIM):
        raise TMRError(f"twoway_update: expected A [N, {TWOWAY_ROWS}, {TWOWAY_DIM}], got {list(A.shape)}")
    N = int(A.shape[0])
    require_gpu(keys, "keys")
    require_gpu(pe, "pe")
    Nk, P = _keys_shape(keys, pe, N)
    if out is keys and not keys.is_contiguous():
        raise TMRError("twoway_update: an in-place update needs contiguous keys")
    keys_c, pe = _f32_gpu(keys, "keys"), _f32_gpu(pe, "pe")
    A, B = _f32_gpu(A, "A"), _f32_gpu(B, "B", (N, TWOWAY_ROWS, TWOWAY_DIM))
    c = _f32_gpu(c, "c", (N, TWOWAY_ROWS))
    bo, g, beta = (_f32_gpu(t, nm, (TWOWAY_DIM,)) for t, nm in ((bo, "bo"), (g, "g"), (beta, "beta")))
    if out is None:
        out = torch.empty((N, P, TWOWAY_DIM), device=A.device, dtype=torch.float32)
    else:
        require_gpu(out, "out")
        if tuple(out.shape) != (N, P, TWOWAY_DIM) or out.dtype != torch.float32 or not out.is_contiguous():
            raise TMRError(f"twoway_update: out must be a contiguous fp32 [{N}, {P}, {TWOWAY_DIM}]")
    _lib.twoway_update(stream(A.device), keys_in=ptr(keys_c), pe=ptr(pe), A=ptr(A), c=ptr(c), B=ptr(B), bo=ptr(bo),
                       g=ptr(g), beta=ptr(beta), keys_out=ptr(out), N=N, Nk=Nk, P=P, T=int(tokens_per_head),
                       eps=float(eps))
    return out


def _check_attention(att, name, dim):
    for p in ("q_proj", "k_proj", "v_proj", "out_proj"):
        lin = getattr(att, p, None)
        if not isinstance(lin, nn.Linear) or lin.bias is None:
            raise TMRError(f"FusedTwoWayTransformer: {name}.{p} must be an nn.Linear with a bias")
    if att.q_proj.in_features != dim or att.out_proj.out_features != dim:
        raise TMRError(f"FusedTwoWayTransformer: {name} has embedding {att.q_proj.in_features}; the kernels are "
                       f"built for {dim}")
    heads = getattr(att, "num_heads", None)
    if heads != TWOWAY_HEADS:
        raise TMRError(f"FusedTwoWayTransformer: {name} has {heads} heads; the kernels are built for {TWOWAY_HEADS}")
    inner = att.q_proj.out_features
    if inner % heads or att.k_proj.out_features != inner or att.v_proj.out_features != inner \
            or att.out_proj.in_features != inner:
        raise TMRError(f"FusedTwoWayTransformer: {name}'s internal dimension {inner} does not split into "
                       f"{heads} heads")


def _check_norm(m, name, dim):
    if not isinstance(m, nn.LayerNorm) or tuple(m.normalized_shape) != (dim,) or m.weight is None or m.bias is None:
        raise TMRError(f"FusedTwoWayTransformer: {name} must be an affine nn.LayerNorm({dim}), got {m}")


def check_transformer(tr, dim=TWOWAY_DIM):
    """Raise TMRError naming the mismatch unless ``tr`` has the structure of
    SAM's TwoWayTransformer with embedding 256 and 8 heads."""
    layers = getattr(tr, "layers", None)
    if not isinstance(layers, (nn.ModuleList, list, tuple)) or len(layers) == 0:
        raise TMRError("FusedTwoWayTransformer: the transformer has no layers")
    for i, blk in enumerate(layers):
        for name in ("self_attn", "norm1", "cross_attn_token_to_image", "norm2", "mlp", "norm3", "norm4",
                     "cross_attn_image_to_token", "skip_first_layer_pe"):
            if not hasattr(blk, name):
                raise TMRError(f"FusedTwoWayTransformer: layers.{i} has no {name}")
        for name in ("cross_attn_token_to_image", "cross_attn_image_to_token"):
            _check_attention(getattr(blk, name), f"layers.{i}.{name}", dim)
        for name in ("norm1", "norm2", "norm3", "norm4"):
            _check_norm(getattr(blk, name), f"layers.{i}.{name}", dim)
    for name in ("final_attn_token_to_image", "norm_final_attn"):
        if not hasattr(tr, name):
            raise TMRError(f"FusedTwoWayTransformer: the transformer has no {name}")
    _check_attention(tr.final_attn_token_to_image, "final_attn_token_to_image", dim)
    _check_norm(tr.norm_final_attn, "norm_final_attn", dim)


def _rows(x):
    """[N, T, H, ...] -> [N, 64, ...]: row 8 h + t, rows t >= T zero."""
    N, T, H = x.shape[:3]
    out = torch.zeros((N, H, TOKENS_MAX) + tuple(x.shape[3:]), device=x.device, dtype=x.dtype)
    out[:, :, :T] = x.transpose(1, 2)
    return out.reshape((N, H * TOKENS_MAX) + tuple(x.shape[3:]))


def fold_tokens_to_image(att, q):
    """qf [N, 64, 256] of tokens -> image attention ``att`` for the (PE-added)
    token queries q [N, T, 256]."""
    N, T, _ = q.shape
    H = att.num_heads
    d = att.q_proj.out_features // H
    qh = att.q_proj(q).view(N, T, H, d) * (1.0 / math.sqrt(d))
    return _rows(torch.einsum("nthd,hdc->nthc", qh, att.k_proj.weight.view(H, d, -1)))


def unfold_context(att, ctx, T):
    """out_proj(concat_h(ctx_h . Wv_h^T + bv_h)): the attention's output
    [N, T, 256] from the pooled raw keys ctx [N, 64, 256]."""
    N = ctx.shape[0]
    H = att.num_heads
    d = att.v_proj.out_features // H
    c = ctx.view(N, H, TOKENS_MAX, -1)[:, :, :T]
    v = torch.einsum("nhtc,hdc->nthd", c, att.v_proj.weight.view(H, d, -1)) + att.v_proj.bias.view(H, d)
    return att.out_proj(v.reshape(N, T, H * d))


def fold_image_to_tokens(att, k_tok, v_tok):
    """(A [N,64,256], c [N,64], B [N,64,256]) of image -> tokens attention
    ``att`` whose keys come from k_tok and values from v_tok [N, T, 256]."""
    N, T, _ = k_tok.shape
    H = att.num_heads
    d = att.q_proj.out_features // H
    kt = att.k_proj(k_tok).view(N, T, H, d) * (1.0 / math.sqrt(d))
    vt = att.v_proj(v_tok).view(N, T, H, d)
    A = torch.einsum("nthd,hdc->nthc", kt, att.q_proj.weight.view(H, d, -1))
    c = torch.einsum("nthd,hd->nth", kt, att.q_proj.bias.view(H, d))
    B = torch.einsum("nthd,chd->nthc", vt, att.out_proj.weight.view(-1, H, d))
    return _rows(A), _rows(c), _rows(B)


class FusedTwoWayTransformer(nn.Module):
    """The reference's ``TwoWayTransformer`` with its image side fused: same
    ``forward`` signature and results (queries [N,T,256], keys [N,h*w,256]).
    Wraps the caller's module and owns no weights.  ``forward_shared`` is the
    route for one image embedding shared by every prompt (what the refiner
    has): layer 0 reads the one [h*w,256] tensor instead of N copies.
    ``calls`` counts the routes taken ("shared", "batched", "stock").

    ``fuse_tokens=True`` runs the token side of the fused routes through
    ``tokens_front`` / ``tokens_back`` (tmr_amd/tokens.py) instead of torch ops;
    ``token_calls`` counts the forwards that did."""

    def __init__(self, transformer, fuse_tokens=False):
        super().__init__()
        check_transformer(transformer)
        if fuse_tokens:
            from .tokens import check_mlp_block

            for i, blk in enumerate(transformer.layers):
                _check_attention(blk.self_attn, f"layers.{i}.self_attn", TWOWAY_DIM)
                check_mlp_block(blk.mlp, f"layers.{i}.mlp")
        self.transformer = transformer
        self.fuse_tokens = bool(fuse_tokens)
        self.calls = {"shared": 0, "batched": 0, "stock": 0}
        self.token_calls = 0

    def forward(self, image_embedding, image_pe, point_embedding):
        require_gpu(image_embedding, "image_embedding")
        N, T = int(point_embedding.shape[0]), int(point_embedding.shape[1])
        pe = self._shared_pe(image_pe)
        if T > TOKENS_MAX or pe is None or image_embedding.shape[0] != N:
            self.calls["stock"] += 1
            return self.transformer(image_embedding, image_pe, point_embedding)
        self.calls["batched"] += 1
        # always a copy, since it is updated in place below: .contiguous() would hand back the caller's
        # own memory for a channels_last or a 1x1 embedding
        keys = image_embedding.detach().flatten(2).permute(0, 2, 1).clone(memory_format=torch.contiguous_format)
        return self._run(keys, pe, point_embedding, own=True)

    def forward_shared(self, image_embedding, image_pe, point_embedding):
        require_gpu(image_embedding, "image_embedding")
        if image_embedding.shape[0] != 1 or image_pe.shape[0] != 1:
            raise TMRError("FusedTwoWayTransformer.forward_shared: image_embedding and image_pe are [1, 256, h, w]")
        N, T = int(point_embedding.shape[0]), int(point_embedding.shape[1])
        if T > TOKENS_MAX:
            self.calls["stock"] += 1
            return self.transformer(image_embedding.expand(N, -1, -1, -1), image_pe.expand(N, -1, -1, -1),
                                    point_embedding)
        self.calls["shared"] += 1
        keys = image_embedding.detach().flatten(2).permute(0, 2, 1).contiguous()
        return self._run(keys, self._shared_pe(image_pe), point_embedding, own=False)

    @staticmethod
    def _shared_pe(image_pe):
        """[h*w, 256] when every prompt has the same positional encoding (what
        the kernels take), else None.  A batch of 1 or a broadcast (stride 0) is
        taken as it is; a materialised per-prompt batch is compared on the
        device, which costs one host sync."""
        if image_pe.shape[0] != 1 and image_pe.stride(0) != 0 and not bool((image_pe == image_pe[:1]).all()):
            return None
        return image_pe[0].detach().flatten(1).t().contiguous()

    def _run(self, keys, pe, point_embedding, own):
        tr = self.transformer
        if keys.shape[2] != TWOWAY_DIM or point_embedding.shape[2] != TWOWAY_DIM:
            raise TMRError(f"FusedTwoWayTransformer: embedding {keys.shape[2]}; the kernels are built for {TWOWAY_DIM}")
        if keys.dtype != torch.float32 or point_embedding.dtype != torch.float32:
            raise TMRError("FusedTwoWayTransformer: fp32 only")
        N, T = int(point_embedding.shape[0]), int(point_embedding.shape[1])
        if self.fuse_tokens:
            return self._run_tokens(keys, pe, point_embedding, own)
        queries = point_embedding
        for blk in tr.layers:
            if blk.skip_first_layer_pe:
                queries = blk.self_attn(q=queries, k=queries, v=queries)
            else:
                q = queries + point_embedding
                queries = queries + blk.self_attn(q=q, k=q, v=queries)
            queries = blk.norm1(queries)
            att = blk.cross_attn_token_to_image
            ctx = twoway_pool(keys, pe, fold_tokens_to_image(att, queries + point_embedding), T)
            queries = blk.norm2(queries + unfold_context(att, ctx, T))
            queries = blk.norm3(queries + blk.mlp(queries))
            att = blk.cross_attn_image_to_token
            A, c, B = fold_image_to_tokens(att, queries + point_embedding, queries)
            in_place = own and keys.shape[0] == N
            keys = twoway_update(keys, pe, A, c, B, att.out_proj.bias, blk.norm4.weight, blk.norm4.bias, blk.norm4.eps,
                                 T, out=keys if in_place else None)
            own = True
        att = tr.final_attn_token_to_image
        ctx = twoway_pool(keys, pe, fold_tokens_to_image(att, queries + point_embedding), T)
        queries = tr.norm_final_attn(queries + unfold_context(att, ctx, T))
        return queries, keys

    def _run_tokens(self, keys, pe, point_embedding, own):
        """_run with the token side in HIP: per layer front, pool, back, update."""
        from .tokens import tokens_back, tokens_front

        tr = self.transformer
        N, T = int(point_embedding.shape[0]), int(point_embedding.shape[1])
        self.token_calls += 1
        pts = queries = point_embedding.detach().contiguous()
        for blk in tr.layers:
            att = blk.cross_attn_token_to_image
            queries, qf = tokens_front(queries, pts, att, self_attn=blk.self_attn, norm1=blk.norm1,
                                       skip_pe=blk.skip_first_layer_pe)
            ctx = twoway_pool(keys, pe, qf, T)
            att2 = blk.cross_attn_image_to_token
            queries, A, c, B = tokens_back(queries, pts, ctx, att, blk.norm2, mlp=blk.mlp, norm3=blk.norm3,
                                           next_attn=att2)
            in_place = own and keys.shape[0] == N
            keys = twoway_update(keys, pe, A, c, B, att2.out_proj.bias, blk.norm4.weight, blk.norm4.bias, blk.norm4.eps,
                                 T, out=keys if in_place else None)
            own = True
        att = tr.final_attn_token_to_image
        queries, qf = tokens_front(queries, pts, att)
        ctx = twoway_pool(keys, pe, qf, T)
        return tokens_back(queries, pts, ctx, att, tr.norm_final_attn), keys
