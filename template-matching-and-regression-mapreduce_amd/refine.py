"""The SAM box refiner (reference: utils/box_refine.py:22-258).

``SAM_box_refiner`` keeps the reference's ``forward`` / ``forward_refine``
signatures and per-image list results.  The two SAM modules are the caller's:
the constructor takes the mask decoder and a factory for the prompt encoder
instead of building them from a checkpoint (this package fetches nothing).
What follows the decoder -- the upsampling of the mask logits to the image
size, the threshold, the per-mask min / max loop and the box arithmetic --
is one fused launch per chunk (tmr_mask_boxes, include/tmr_refine.h) that
writes straight into the image's preallocated outputs: the upsampled masks
never exist and the mask path reads nothing back.

``mask_boxes`` is that step as a function.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import (MASK_BOXES_WORK_PER_MASK, REFINE_FORWARD, REFINE_SCALED, TMRError, ptr, require_gpu,
                   stream)


def _rows(masks: torch.Tensor) -> torch.Tensor:
    """[N,1,h,w] or [N,h,w] mask logits -> contiguous fp32 [N,h,w]."""
    require_gpu(masks, "masks")
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    if masks.dim() != 3:
        raise TMRError(f"mask_boxes: expected [N,1,h,w] or [N,h,w] masks, got {tuple(masks.shape)}")
    return masks.detach().float().contiguous()


def _launch(masks, size, logits, iou, scaler, out_logits, out_boxes, out_refs):
    """One tmr_mask_boxes launch on the current stream; the outputs are
    contiguous fp32 row blocks ([N,2], [N,4], [N,2]).  Returns the work buffer
    (int32 [N,4] accumulators: column 2 stays negative for an empty mask)."""
    m = _rows(masks)
    N, h, w = m.shape
    H, W = int(size[0]), int(size[1])
    require_gpu(logits, "logits")
    require_gpu(iou, "iou")
    lg = logits.detach().float().contiguous()
    io = iou.detach().float().contiguous()
    if tuple(lg.shape) != (N, 2) or io.numel() != N:
        raise TMRError(f"mask_boxes: {N} masks need logits [{N},2] and iou [{N}], got {tuple(logits.shape)} "
                       f"and {tuple(iou.shape)}")
    sc = None
    if scaler is not None:
        require_gpu(scaler, "scaler")
        sc = scaler.detach().float().contiguous()
        if sc.numel() != 4:
            raise TMRError(f"mask_boxes: scaler holds 4 values, got {tuple(scaler.shape)}")
    for t, cols in ((out_logits, 2), (out_boxes, 4), (out_refs, 2)):
        if t.dtype != torch.float32 or tuple(t.shape) != (N, cols):
            raise TMRError("mask_boxes: outputs are fp32 [N,2], [N,4], [N,2]")
    work = torch.empty((max(N, 1), MASK_BOXES_WORK_PER_MASK // 4), device=m.device, dtype=torch.int32)
    _lib.mask_boxes(stream(m.device), masks=ptr(m), logits=ptr(lg), iou=ptr(io), scaler=ptr(sc),
                    boxes=ptr(out_boxes), refs=ptr(out_refs), logits_out=ptr(out_logits), work=ptr(work),
                    N=N, h=h, w=w, H=H, W=W, mode=REFINE_FORWARD if sc is None else REFINE_SCALED)
    return work


def mask_boxes(masks, size, logits, iou, scaler=None):
    """The reference's mask -> box step (box_refine.py:232-246; with
    ``scaler`` [4], forward_refine's :158-176) for N masks.

    masks: [N,1,h,w] or [N,h,w] fp32 mask logits on a HIP device; size =
    (H, W), the image size the reference upsamples to (bilinear,
    align_corners=True); logits [N,2] the candidates' score rows; iou [N] or
    [N,1] the decoder's IoU predictions.  Returns (logits [N,2], boxes [N,4],
    refs [N,2]): normalised xyxy boxes of the positive pixels (zeros for an
    empty mask), their centres, and (iou * logits[:,0], 0 * logits[:,1])."""
    m = _rows(masks)
    N = m.shape[0]
    out_l = torch.empty((N, 2), device=m.device, dtype=torch.float32)
    out_b = torch.empty((N, 4), device=m.device, dtype=torch.float32)
    out_r = torch.empty((N, 2), device=m.device, dtype=torch.float32)
    _launch(m, size, logits, iou, scaler, out_l, out_b, out_r)
    return out_l, out_b, out_r


class SAM_box_refiner(nn.Module):
    """box_refine.py:22-258 without the checkpoint download.

    mask_decoder: the caller's SAM mask decoder (the reference's vendored
    ``MaskDecoder`` with the weights the caller already holds);
    prompt_encoder_factory(image_size, emb_size) returns the prompt encoder
    for one image size / embedding size pair; it is built once per pair."""

    def __init__(self, mask_decoder, prompt_encoder_factory):
        super().__init__()
        self.step = 50
        self.prompt_embed_dim = 256
        self.mask_decoder = mask_decoder
        self.prompt_encoder_factory = prompt_encoder_factory
        self._encoders = {}

    def prompt_encoder_init(self, image_size, emb_size):
        return self.prompt_encoder_factory(image_size, emb_size)

    def _encoder(self, image_size, emb_size, device):
        key = (tuple(int(v) for v in image_size), tuple(int(v) for v in emb_size), str(device))
        enc = self._encoders.get(key)
        if enc is None:
            enc = self.prompt_encoder_init(image_size, emb_size)
            if hasattr(enc, "to"):
                enc = enc.to(device)
            self._encoders[key] = enc
        return enc

    def _decode(self, enc, box, feature):
        """One prompt-encoder + mask-decoder call, as box_refine.py:216-229."""
        sparse, dense = enc(points=None, boxes=box, masks=None)
        return self.mask_decoder(image_embeddings=feature.unsqueeze(0), image_pe=enc.get_dense_pe(),
                                 sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense,
                                 multimask_output=False)

    def _exemplar_scaler(self, enc, exemplar, img_res, img_shape, feature):
        """box_refine.py:84-114: the exemplar's own mask box against the
        exemplar box -> the four ltrb ratios [4] (device, fp32).  One
        read-back (is the mask empty?), where the reference syncs too."""
        ex = torch.as_tensor(exemplar, dtype=img_res.dtype, device=img_res.device).reshape(1, 4)
        masks_, iou_ = self._decode(enc, ex * img_res, feature)
        one = torch.ones((1, 2), device=img_res.device, dtype=torch.float32)
        out_l = torch.empty((1, 2), device=img_res.device, dtype=torch.float32)
        mbox = torch.empty((1, 4), device=img_res.device, dtype=torch.float32)
        out_r = torch.empty((1, 2), device=img_res.device, dtype=torch.float32)
        work = _launch(masks_[:1], img_shape, one, iou_.reshape(-1)[:1], None, out_l, mbox, out_r)
        if int(work[0, 2].item()) < 0:  # torch.min of an empty tensor in the reference
            raise ValueError("SAM_box_refiner.forward_refine: the exemplar's mask has no positive pixel")
        mbox = mbox.to(img_res.dtype)
        # fp32 on the device, in the reference's order: the mask box's centre, its four extents,
        # the exemplar box's extents about the same centre, the ratios
        cx, cy = (mbox[:, 0] + mbox[:, 2]) / 2, (mbox[:, 1] + mbox[:, 3]) / 2
        mask_ext = (cx - mbox[:, 0], cy - mbox[:, 1], mbox[:, 2] - cx, mbox[:, 3] - cy)
        ex_ext = (cx - ex[0, 0], cy - ex[0, 1], ex[0, 2] - cx, ex[0, 3] - cy)
        return torch.cat([e / m for e, m in zip(ex_ext, mask_ext)], dim=-1)

    def _run(self, pred_logits, pred_boxes, ref_points, image, exemplars, features):
        """Both entry points: per image, the exemplar's scaler (forward_refine
        only), then one decoder call and one tmr_mask_boxes launch per chunk
        of ``step`` candidates, into the image's preallocated rows."""
        outs = ([], [], [])
        for i in range(len(pred_logits)):
            cand_l, cand_b = pred_logits[i], pred_boxes[i]
            n = len(cand_b)
            if n == 0:  # nothing to refine: the image's own (empty) tensors go through
                for dst, src in zip(outs, (cand_l, cand_b, ref_points[i])):
                    dst.append(src)
                continue
            require_gpu(cand_b, "pred_boxes")
            size = tuple(image[i].shape[-2:])
            res = torch.tensor([size[1], size[0], size[1], size[0]], dtype=image.dtype, device=image.device)
            enc = self._encoder(size, features[i].shape[-2:], image.device)
            scaler = None
            if exemplars is not None:
                scaler = self._exemplar_scaler(enc, exemplars[i][0], res, size, features[i])
            out_l = torch.empty((n, 2), device=cand_b.device, dtype=torch.float32)
            out_b = torch.empty((n, 4), device=cand_b.device, dtype=torch.float32)
            out_r = torch.empty((n, 2), device=cand_b.device, dtype=torch.float32)
            for lo in range(0, n, self.step):
                hi = min(lo + self.step, n)
                masks, iou = self._decode(enc, cand_b[lo:hi] * res, features[i])
                _launch(masks, size, cand_l[lo:hi], iou, scaler, out_l[lo:hi], out_b[lo:hi], out_r[lo:hi])
            # result dtypes as the reference's promotions give them (fp32 for fp32 inputs)
            ldt = torch.promote_types(iou.dtype, cand_l.dtype)
            bdt = torch.promote_types(cand_b.dtype, res.dtype)
            outs[0].append(out_l if ldt == torch.float32 else out_l.to(ldt))
            outs[1].append(out_b if bdt == torch.float32 else out_b.to(bdt))
            outs[2].append(out_r if bdt == torch.float32 else out_r.to(bdt))
        return outs

    def forward_refine(self, pred_logits, pred_boxes, ref_points, image, exemplars, features):
        """box_refine.py:64-188: as forward, with every mask box's extents
        about its centre scaled by the exemplar's box / mask-box ratios."""
        return self._run(pred_logits, pred_boxes, ref_points, image, exemplars, features)

    def forward(self, pred_logits, pred_boxes, ref_points, image, features):
        """box_refine.py:190-258: per image, the candidates in chunks of
        ``step`` through the prompt encoder and the mask decoder; each
        candidate's box becomes its mask's box, its score the decoder's IoU
        prediction times the original score."""
        return self._run(pred_logits, pred_boxes, ref_points, image, None, features)
