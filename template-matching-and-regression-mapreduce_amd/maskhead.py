"""The fused mask head of the SAM mask decoder (reference:
utils/segment_anything/modeling/mask_decoder.py:71-161).

The stock decoder upscales the transformer's [N, h*w, 256] output to
[N,64,2h,2w] and [N,32,4h,4w], multiplies by FOUR hypernetwork rows per prompt
and keeps one mask (this fork's argmax selection, :101-103).  Here the part
after the transformer is one launch (tmr_mask_head, include/tmr_maskhead.h)
that reads ``src`` once and writes the one selected [N,1,4h,4w] mask per
prompt; neither intermediate tensor exists.

``mask_head`` is that step as a function, ``mask_head_weights`` its packed
weights, ``FusedMaskDecoder`` the drop-in for the caller's ``MaskDecoder``:

    refiner = SAM_box_refiner(FusedMaskDecoder(mask_decoder), prompt_encoder_factory)

The transformer, the token-side MLPs and the prompt encoder stay the caller's
modules.  fp32 on a HIP device only; there is no CPU path.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import MASK_HEAD_DIM, MASK_HEAD_WPACK_BYTES, TMRError, ptr, require_gpu, stream


def _is_convT(m, cin, cout):
    return (isinstance(m, nn.ConvTranspose2d) and m.in_channels == cin and m.out_channels == cout
            and tuple(m.kernel_size) == (2, 2) and tuple(m.stride) == (2, 2) and tuple(m.padding) == (0, 0)
            and tuple(m.output_padding) == (0, 0) and tuple(m.dilation) == (1, 1) and m.groups == 1
            and m.bias is not None)


def _is_gelu(m):
    return isinstance(m, nn.GELU) and getattr(m, "approximate", "none") == "none"


def check_upscaling(up, dim=MASK_HEAD_DIM):
    """Raise TMRError naming the mismatch unless ``up`` is the decoder's
    output_upscaling: ConvTranspose2d(dim, dim/4, 2, 2), a LayerNorm2d-like
    module (weight / bias / eps), exact GELU, ConvTranspose2d(dim/4, dim/8, 2,
    2), exact GELU."""
    if dim != MASK_HEAD_DIM:
        raise TMRError(f"fused mask head: transformer_dim is {dim}; the kernel is built for {MASK_HEAD_DIM}")
    if not isinstance(up, (nn.Sequential, list, tuple)) or len(up) != 5:
        raise TMRError("fused mask head: output_upscaling must be a Sequential of 5 modules "
                       "(ConvTranspose2d, LayerNorm2d, GELU, ConvTranspose2d, GELU)")
    if not _is_convT(up[0], dim, dim // 4):
        raise TMRError(f"fused mask head: output_upscaling.0 must be ConvTranspose2d({dim}, {dim // 4}, "
                       f"kernel_size=2, stride=2) with a bias, got {up[0]}")
    ln = up[1]
    if not (isinstance(getattr(ln, "weight", None), torch.Tensor) and isinstance(getattr(ln, "bias", None), torch.Tensor)
            and isinstance(getattr(ln, "eps", None), float) and tuple(ln.weight.shape) == (dim // 4,)
            and tuple(ln.bias.shape) == (dim // 4,)) or isinstance(ln, (nn.BatchNorm2d, nn.GroupNorm)):
        raise TMRError(f"fused mask head: output_upscaling.1 must be a LayerNorm2d over {dim // 4} channels "
                       f"(weight, bias, eps), got {ln}")
    for i in (2, 4):
        if not _is_gelu(up[i]):
            raise TMRError(f"fused mask head: output_upscaling.{i} must be nn.GELU(approximate='none'), got {up[i]}")
    if not _is_convT(up[3], dim // 4, dim // 8):
        raise TMRError(f"fused mask head: output_upscaling.3 must be ConvTranspose2d({dim // 4}, {dim // 8}, "
                       f"kernel_size=2, stride=2) with a bias, got {up[3]}")


class MaskHeadWeights:
    """The packed operands of tmr_mask_head for one output_upscaling.  Packs on
    first use and again when one of the six tensors (both ConvTranspose2d
    weights and biases, the LayerNorm2d weight and bias) was replaced, moved
    or edited in place (identity, address and version are remembered, as the
    engine's caches do); ``packs`` counts the prep launches."""

    def __init__(self, output_upscaling):
        check_upscaling(output_upscaling)
        self.up = output_upscaling
        self.packs = 0
        self._key = None
        self._held = None

    def _tensors(self):
        up = self.up
        return (up[0].weight, up[0].bias, up[1].weight, up[1].bias, up[3].weight, up[3].bias)

    def get(self, device):
        """(wpack, b1, g, beta, b2, eps) on ``device``, current."""
        ts = self._tensors()
        key = tuple((id(t), t.data_ptr(), t._version, str(t.device), t.dtype) for t in ts) + (str(device),)
        if key != self._key:
            for t in ts:
                require_gpu(t, "output_upscaling weights")
                if t.device != device:
                    raise TMRError(f"fused mask head: output_upscaling is on {t.device}, the inputs on {device}")
            w1, b1, g, beta, w2, b2 = (t.detach().float().contiguous() for t in ts)
            wpack = torch.empty(MASK_HEAD_WPACK_BYTES, device=device, dtype=torch.uint8)
            _lib.mask_head_prep(stream(device), w1=ptr(w1), w2=ptr(w2), wpack=ptr(wpack), C=MASK_HEAD_DIM)
            self.packs += 1
            self._held = (wpack, b1, g, beta, b2)
            self._key = key
        return self._held + (float(self.up[1].eps),)


def mask_head_weights(output_upscaling) -> MaskHeadWeights:
    """The packed weights of ``mask_head`` for a decoder's output_upscaling
    (structure checked here; packed on first use, repacked after an edit)."""
    return MaskHeadWeights(output_upscaling)


def mask_head(src, hyper, weights, size=None):
    """The mask head for N prompts, one launch.

    src [N, h*w, 256]: the two-way transformer's second output, token-major, as
    it returns it; hyper [N, 32]: each prompt's selected hypernetwork row;
    weights: ``mask_head_weights(output_upscaling)``; size = (h, w) of the
    embedding (default: square).  fp32 on a HIP device.  Returns masks
    [N,1,4h,4w] (include/tmr_maskhead.h has the rule)."""
    if not isinstance(weights, MaskHeadWeights):
        raise TMRError("mask_head: weights come from tmr_amd.mask_head_weights(output_upscaling)")
    require_gpu(src, "src")
    require_gpu(hyper, "hyper")
    if src.dim() != 3 or src.shape[2] != MASK_HEAD_DIM:
        raise TMRError(f"mask_head: expected src [N, h*w, {MASK_HEAD_DIM}], got {tuple(src.shape)}")
    N, hw = int(src.shape[0]), int(src.shape[1])
    if size is None:
        h = int(round(hw ** 0.5))
        size = (h, h)
    h, w = int(size[0]), int(size[1])
    if h * w != hw:
        raise TMRError(f"mask_head: src holds {hw} pixels per prompt, size {(h, w)} has {h * w}")
    if tuple(hyper.shape) != (N, MASK_HEAD_DIM // 8):
        raise TMRError(f"mask_head: expected hyper [{N}, {MASK_HEAD_DIM // 8}], got {tuple(hyper.shape)}")
    if src.dtype != torch.float32 or hyper.dtype != torch.float32:
        raise TMRError("mask_head: src and hyper must be fp32")
    s = src.detach().contiguous()
    hy = hyper.detach().contiguous()
    wpack, b1, g, beta, b2, eps = weights.get(s.device)
    masks = torch.empty((N, 1, 4 * h, 4 * w), device=s.device, dtype=torch.float32)
    _lib.mask_head(stream(s.device), src=ptr(s), hyper=ptr(hy), wpack=ptr(wpack), b1=ptr(b1), g=ptr(g),
                   beta=ptr(beta), b2=ptr(b2), masks=ptr(masks), N=N, h=h, w=w, C=MASK_HEAD_DIM, eps=eps)
    return masks


class FusedMaskDecoder(nn.Module):
    """The reference's ``MaskDecoder`` (mask_decoder.py:16-161) with its mask
    head fused: same ``forward`` signature, same results (masks [N,1,4h,4w],
    iou [N,1]).  Wraps the caller's decoder and owns no weights of its own.

    ``fuse_transformer=True`` also runs the decoder's two-way transformer
    through ``FusedTwoWayTransformer`` (tmr_amd/twoway.py): its shared route
    when one image embedding, one positional encoding and a batch-broadcast
    dense prompt embedding serve every prompt (what ``SAM_box_refiner``
    passes), its batched route otherwise.  ``transformer_calls`` then counts
    the routes taken.

    ``fuse_tokens=True`` (with ``fuse_transformer=True``) also runs the token
    side in HIP (tmr_amd/tokens.py): the transformer's through
    ``FusedTwoWayTransformer(..., fuse_tokens=True)``, the IoU head and the
    hypernetwork MLPs through ``tokens_tail``; the argmax and the two gathers
    stay torch ops."""

    def __init__(self, mask_decoder, fuse_transformer=False, fuse_tokens=False):
        super().__init__()
        if fuse_tokens and not fuse_transformer:
            raise TMRError("FusedMaskDecoder: fuse_tokens=True requires fuse_transformer=True")
        dim = getattr(mask_decoder, "transformer_dim", None)
        if dim != MASK_HEAD_DIM:
            raise TMRError(f"FusedMaskDecoder: transformer_dim is {dim}; the fused head is built for "
                           f"{MASK_HEAD_DIM}")
        for name in ("transformer", "iou_token", "mask_tokens", "output_upscaling", "output_hypernetworks_mlps",
                     "iou_prediction_head", "num_mask_tokens"):
            if not hasattr(mask_decoder, name):
                raise TMRError(f"FusedMaskDecoder: the decoder has no {name}")
        check_upscaling(mask_decoder.output_upscaling, dim)
        T = int(mask_decoder.num_mask_tokens)
        mlps = mask_decoder.output_hypernetworks_mlps
        if len(mlps) != T:
            raise TMRError(f"FusedMaskDecoder: {len(mlps)} output_hypernetworks_mlps for num_mask_tokens = {T}")
        for i, mlp in enumerate(mlps):
            last = [m for m in mlp.modules() if isinstance(m, nn.Linear)]
            if not last or last[-1].out_features != dim // 8:
                raise TMRError(f"FusedMaskDecoder: output_hypernetworks_mlps.{i} must end in {dim // 8} outputs")
        self.mask_decoder = mask_decoder
        self.weights = mask_head_weights(mask_decoder.output_upscaling)
        self.fused_transformer = None
        self.fuse_tokens = bool(fuse_tokens)
        if fuse_tokens:
            from .tokens import check_mlp3

            check_mlp3(mask_decoder.iou_prediction_head, "iou_prediction_head")
            for i, mlp in enumerate(mlps):
                check_mlp3(mlp, f"output_hypernetworks_mlps.{i}")
        if fuse_transformer:
            from .twoway import FusedTwoWayTransformer

            self.fused_transformer = FusedTwoWayTransformer(mask_decoder.transformer, fuse_tokens=fuse_tokens)

    @property
    def transformer_calls(self):
        return None if self.fused_transformer is None else self.fused_transformer.calls

    def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings,
                multimask_output=False):
        d = self.mask_decoder
        require_gpu(image_embeddings, "image_embeddings")
        # predict_masks up to the transformer call (mask_decoder.py:125-144)
        output_tokens = torch.cat([d.iou_token.weight, d.mask_tokens.weight], dim=0)
        output_tokens = output_tokens.unsqueeze(0).expand(sparse_prompt_embeddings.size(0), -1, -1)
        tokens = torch.cat((output_tokens, sparse_prompt_embeddings), dim=1)
        ft = self.fused_transformer
        if (ft is not None and image_embeddings.shape[0] == 1 and image_pe.shape[0] == 1
                and (dense_prompt_embeddings.shape[0] == 1 or dense_prompt_embeddings.stride(0) == 0)):
            # one embedding for every prompt: the add is done once, nothing is repeated
            dense = dense_prompt_embeddings[:1]
            if dense.shape[1:] != image_embeddings.shape[1:]:
                dense = nn.UpsamplingBilinear2d(scale_factor=1.5)(dense)
            src1 = image_embeddings + dense
            if image_pe.shape[1:] != image_embeddings.shape[1:]:
                image_pe = nn.UpsamplingBilinear2d(scale_factor=1.5)(image_pe)
            h, w = src1.shape[2:]
            hs, src = ft.forward_shared(src1, image_pe, tokens)
            return self._head(hs, src, h, w)
        src = torch.repeat_interleave(image_embeddings, tokens.shape[0], dim=0)
        if dense_prompt_embeddings.shape[1:] != image_embeddings.shape[1:]:
            dense_prompt_embeddings = nn.UpsamplingBilinear2d(scale_factor=1.5)(dense_prompt_embeddings)
        src = src + dense_prompt_embeddings
        if image_pe.shape[1:] != image_embeddings.shape[1:]:
            image_pe = nn.UpsamplingBilinear2d(scale_factor=1.5)(image_pe)
        if ft is not None and image_pe.shape[0] == 1:
            pos_src = image_pe.expand(tokens.shape[0], -1, -1, -1)  # a broadcast: the wrapper sees it is shared
        else:
            pos_src = torch.repeat_interleave(image_pe, tokens.shape[0], dim=0)
        b, c, h, w = src.shape
        hs, src = (d.transformer if ft is None else ft)(src, pos_src, tokens)
        return self._head(hs, src, h, w)

    def _head(self, hs, src, h, w):
        d = self.mask_decoder
        # token-sized: the IoU head, the selection, every MLP on all rows and the gather
        T = d.num_mask_tokens
        if self.fuse_tokens:
            from .tokens import tokens_tail

            iou_pred, hyper_all = tokens_tail(hs, d.iou_prediction_head, d.output_hypernetworks_mlps)
            ids = torch.argmax(iou_pred, dim=1)
        else:
            iou_pred = d.iou_prediction_head(hs[:, 0, :])
            ids = torch.argmax(iou_pred, dim=1)
            hyper_all = torch.stack([d.output_hypernetworks_mlps[i](hs[:, 1 + i, :]) for i in range(T)], dim=1)
        hyper = torch.gather(hyper_all, 1, ids.view(-1, 1, 1).expand(-1, 1, hyper_all.shape[2]))[:, 0]
        iou = torch.gather(iou_pred, 1, ids.view(-1, 1))
        if src.dtype != torch.float32:
            raise TMRError(f"FusedMaskDecoder: the transformer returned {src.dtype}; the fused head is fp32")
        masks = mask_head(src, hyper.float(), self.weights, (h, w))
        return masks, iou
