"""ctypes binding of libtmr.so (include/tmr.h).

The library is the ONLY compute path: there is no CPU / PyTorch fallback.  A
missing or unloadable library, or a CPU tensor handed to a compute entry
point, raises immediately.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtmr.so")
if os.environ.get("TMR_LIB_VARIANT"):  # profiling only: an experiment build next to libtmr.so
    LIB_PATH = os.path.join(_HERE, "libtmr_%s.so" % os.environ["TMR_LIB_VARIANT"])
HEADER = os.path.join(os.path.dirname(_HERE), "include", "tmr.h")

_lock = threading.Lock()
_lib = None

# ABI structs (must match include/tmr.h)
UNIT_DTYPE = np.dtype({
    "names": ["image", "type", "ht", "wt", "roi", "pbox", "tmpl_offset", "row_offset", "pad_"],
    "formats": [np.int32, np.int32, np.int32, np.int32, (np.float32, 4), (np.int32, 4), np.int64,
                np.int32, np.int32],
    "offsets": [0, 4, 8, 12, 16, 32, 48, 56, 60],
    "itemsize": 64,
})
PEAK_DTYPE = np.dtype({
    "names": ["thr", "scale_w", "scale_h", "mask", "mode", "pad_"],
    "formats": [np.float32, np.float32, np.float32, np.int32, np.int32, np.int32],
    "offsets": [0, 4, 8, 12, 16, 20],
    "itemsize": 24,
})

GT_UNIT_DTYPE = np.dtype({  # tmr_gt_unit_t
    "names": ["image", "pad_x", "pad_y", "mode", "scale_w", "scale_h", "pad_"],
    "formats": [np.int32, np.int32, np.int32, np.int32, np.float32, np.float32, (np.int32, 2)],
    "offsets": [0, 4, 8, 12, 16, 20, 24],
    "itemsize": 32,
})

TEMPLATE_ROI_ALIGN = 0
TEMPLATE_PROTOTYPE = 1

# decoder-conv precision modes of the split 16-bit-MFMA kernel (include/tmr.h)
PREC_CODES = {"fp32": 0, "bf16": 1, "f16": 2}
SPLIT_TILED_OUT, SPLIT_TILED_INIT, SPLIT_INIT_BCAST = 1, 2, 4
SPLIT_OUT_BF16, SPLIT_INIT_BF16 = 8, 16  # one-term precisions: bf16 acc0 slabs
SPLIT_XMAX_PER_UNIT = 32  # xmax is float[U]: one activation scale per unit / output slab
SPLIT_XMAX_PER_PIXEL = 64  # 1x1 stores: xmax is float[U][H][W], one scale per output pixel
PEAKS_PROB_SCRATCH = 2  # tmr_peaks_decode: prob is scratch (low logits hold -1)
SPLIT_UNITS_PER_IMAGE_SHIFT = 8  # flags bits 8..15: E units per image -> image-major heads order
# flags bits 16..23 / 24..30: the launch's window (first, count) of 128-channel tiles; 0/0 = all
SPLIT_TILE_FIRST_SHIFT, SPLIT_TILE_COUNT_SHIFT = 16, 24
PEAKS_FIND_ONLY, PEAKS_DECODE_ONLY = 8, 16  # tmr_peaks_decode: the finder alone / the decode alone
POINTS_TILE = 64  # TMR_POINTS_TILE: candidates per tile of tmr_split_conv_points
# correlation kernel choice (tmr_xcorr_args_t.algo)
XCORR_ALGOS = {"auto": 0, "valu": 1, "mfma": 2}
XPACK_UPSAMPLE, XPACK_ONES = 1, 2  # tmr_split_xpack `up` bits
# tmr_size kinds
SIZE_KINDS = {"template_split": 1, "heads_partials": 2, "xpack": 3, "wpack": 4, "acc": 5, "nms_work": 6,
              "stats_work": 7, "gt_work": 8}
# tmr_gt_loss_args_t.phase bits; TMR_GT_SLICES
GT_ASSIGN, GT_LOSS, GT_GATHER, GT_ROWS = 1, 2, 4, 8
GT_SLICES = 16
ABI_VERSION = 3

_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64
_D = ctypes.c_double


class XcorrArgs(ctypes.Structure):
    """tmr_xcorr_args_t (include/tmr.h)."""
    _fields_ = [("f", _P), ("templates", _P), ("units", _P), ("img_units", _P), ("scale", _P), ("out", _P),
                ("relu_out", _P), ("work", _P), ("out_absmax", _P), ("tmpl_split", _P), ("total_rows", _L),
                ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("U", ctypes.c_int32), ("max_ht", ctypes.c_int32), ("max_wt", ctypes.c_int32),
                ("squeeze", ctypes.c_int32), ("algo", ctypes.c_int32), ("min_k", ctypes.c_int32),
                ("prec", ctypes.c_int32), ("out_bf16", ctypes.c_int32)]


class XcorrPlan(ctypes.Structure):
    """tmr_xcorr_plan_t (include/tmr.h)."""
    _fields_ = [("kernel", ctypes.c_int32), ("band_rows", ctypes.c_int32), ("col_groups", ctypes.c_int32),
                ("out16", ctypes.c_int32)]


XCORR_KERNELS = {0: "valu", 1: "rows15", 2: "rows31", 3: "mfma"}  # TMR_XCORR_KERNEL_*


class GtLossArgs(ctypes.Structure):
    """tmr_gt_loss_args_t (include/tmr.h)."""
    _fields_ = [("o", _P), ("reg", _P), ("boxes", _P), ("box_off", _P), ("units", _P), ("exp_table", _P),
                ("work", _P), ("gt_map", _P), ("target", _P), ("counts", _P), ("sums", _P), ("samp_off", _P),
                ("row_off", _P), ("obj_out", _P), ("label_out", _P), ("rows_pred", _P), ("rows_gt", _P),
                ("positive_threshold", _D), ("negative_threshold", _D), ("n_samples", _L), ("n_rows", _L),
                ("U", ctypes.c_int32), ("NI", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("G_total", ctypes.c_int32), ("min_boxes", ctypes.c_int32), ("last_level", ctypes.c_int32),
                ("focal", ctypes.c_int32), ("phase", ctypes.c_int32), ("pad_", ctypes.c_int32)]


# name -> (restype, argtypes)
SIGNATURES = {
    "tmr_version": (_I, []),
    "tmr_strerror": (ctypes.c_char_p, [_I]),
    "tmr_upsample2x": (_I, [_P, _I, _I, _I, _P, _P]),
    "tmr_templates": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P]),
    "tmr_size": (_L, [_I, _L, _L, _L, _L, _L, _L]),
    "tmr_xcorr": (_I, [ctypes.POINTER(XcorrArgs), _P]),
    "tmr_xcorr_plan": (_I, [ctypes.POINTER(XcorrArgs), ctypes.POINTER(XcorrPlan)]),
    "tmr_template_split": (_I, [_P, _P, _I, _I, _L, _I, _P, _P]),  # (..., total_rows, prec, out, stream)
    "tmr_heads_reduce": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "tmr_absmax_rows": (_I, [_P, _I, _L, _I, _P, _P]),
    "tmr_scale_merge": (_I, [_P, _P, _P, _I, _I, _P, _P, _P]),
    "tmr_pixel_absmax": (_I, [_P, _I, _I, _L, _P, _P]),
    "tmr_split_xpack": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P]),
    "tmr_split_xpack16": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "tmr_split_fold_proj": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _P, _P]),
    "tmr_split_wpack": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "tmr_split_conv": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I,
                            _P]),
    "tmr_split_conv_points": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P,
                                   _P, _P, _I, _P, _I, _P]),
    "tmr_peaks_decode": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tmr_maxpool3x3": (_I, [_P, _L, _I, _I, _I, _P, _P]),
    "tmr_nms": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _L, _L, _L, _D, _P, _P, _P, _P, _P, _P, _P]),
    "tmr_nms_small": (_I, [_P, _P, _P, _P, _P, _P, _I, _D, _P, _P, _P, _P, _P, _P]),
    "tmr_feature_stats": (_I, [_P, _I, _L, _P, _P, _P]),
    "tmr_gt_loss": (_I, [ctypes.POINTER(GtLossArgs), _P]),
    "tmr_exp_table_encode": (_L, [_P, _L, _P, _L]),
    "tmr_exp_table_decode": (_L, [_P, _L, _P, _L]),
}


class MaskBoxesArgs(ctypes.Structure):
    """tmr_mask_boxes_args_t (include/tmr_refine.h)."""
    _fields_ = [("masks", _P), ("logits", _P), ("iou", _P), ("scaler", _P), ("boxes", _P), ("refs", _P),
                ("logits_out", _P), ("work", _P), ("N", _L), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("mode", ctypes.c_int32), ("pad_", ctypes.c_int32)]


# the optional evaluation extension (include/tmr_refine.h): exported by the same libtmr.so, outside
# the core ABI above
EXT_HEADER = os.path.join(os.path.dirname(_HERE), "include", "tmr_refine.h")
EXT_SIGNATURES = {
    "tmr_mask_boxes": (_I, [ctypes.POINTER(MaskBoxesArgs), _P]),
    "tmr_mask_boxes_plan": (_I, [ctypes.POINTER(MaskBoxesArgs), ctypes.POINTER(ctypes.c_int32),
                                 ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
}
REFINE_FORWARD, REFINE_SCALED = 0, 1  # tmr_mask_boxes_args_t.mode
MASK_BOXES_WORK_PER_MASK = 16  # TMR_MASK_BOXES_WORK_BYTES(N) = 16 * N


class CocoMatchArgs(ctypes.Structure):
    """tmr_coco_match_args_t (include/tmr_coco.h)."""
    _fields_ = [("det_off", _P), ("det_box", _P), ("det_area", _P), ("gt_off", _P), ("gt_box", _P),
                ("gt_area", _P), ("gt_crowd", _P), ("area_rng", _P), ("iou_thr", _P), ("dt_match", _P),
                ("dt_ignore", _P), ("gt_ignore", _P), ("gt_match", _P), ("sum_d", _L), ("sum_g", _L),
                ("I", ctypes.c_int32), ("A", ctypes.c_int32), ("T", ctypes.c_int32), ("max_d", ctypes.c_int32),
                ("max_g", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class CocoMatchPlan(ctypes.Structure):
    """tmr_coco_match_plan_t (include/tmr_coco.h)."""
    _fields_ = [("variant", ctypes.c_int32), ("tile_cap", ctypes.c_int32), ("list_cap", ctypes.c_int32),
                ("threads", ctypes.c_int32), ("lds_bytes", ctypes.c_int32), ("blocks", ctypes.c_int32)]


# the COCO AP matching extension (include/tmr_coco.h): same libtmr.so, outside the core ABI as well
COCO_HEADER = os.path.join(os.path.dirname(_HERE), "include", "tmr_coco.h")
COCO_SIGNATURES = {
    "tmr_coco_match": (_I, [ctypes.POINTER(CocoMatchArgs), _P]),
    "tmr_coco_match_plan": (_I, [ctypes.POINTER(CocoMatchArgs), ctypes.POINTER(CocoMatchPlan)]),
}
COCO_VARIANTS = {0: "lds", 1: "global"}  # TMR_COCO_VARIANT_*
COCO_T_MAX, COCO_D_MAX, COCO_G_MAX = 16, 4096, 65536


class MaskHeadArgs(ctypes.Structure):
    """tmr_mask_head_args_t (include/tmr_maskhead.h)."""
    _fields_ = [("src", _P), ("hyper", _P), ("w1", _P), ("w2", _P), ("wpack", _P), ("b1", _P), ("g", _P),
                ("beta", _P), ("b2", _P), ("masks", _P), ("N", _L), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("C", ctypes.c_int32), ("eps", ctypes.c_float)]


class MaskHeadPlan(ctypes.Structure):
    """tmr_mask_head_plan_t (include/tmr_maskhead.h)."""
    _fields_ = [("variant", ctypes.c_int32), ("tile_pixels", ctypes.c_int32), ("threads", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("tiles", ctypes.c_int32), ("blocks", ctypes.c_int32)]


# the fused SAM mask head (include/tmr_maskhead.h): same libtmr.so, outside the core ABI as well
MASKHEAD_HEADER = os.path.join(os.path.dirname(_HERE), "include", "tmr_maskhead.h")
MASKHEAD_SIGNATURES = {
    "tmr_mask_head_prep": (_I, [ctypes.POINTER(MaskHeadArgs), _P]),
    "tmr_mask_head": (_I, [ctypes.POINTER(MaskHeadArgs), _P]),
    "tmr_mask_head_plan": (_I, [ctypes.POINTER(MaskHeadArgs), ctypes.POINTER(MaskHeadPlan)]),
}
MASK_HEAD_VARIANTS = {0: "mfma128"}  # TMR_MASK_HEAD_VARIANT_*
MASK_HEAD_WPACK_BYTES = 9 * 32768 + 64  # TMR_MASK_HEAD_WPACK_BYTES
MASK_HEAD_DIM = 256  # the one transformer_dim the kernel is built for


class TwoWayPoolArgs(ctypes.Structure):
    """tmr_twoway_pool_args_t (include/tmr_twoway.h)."""
    _fields_ = [("keys", _P), ("pe", _P), ("qf", _P), ("ctx", _P), ("work", _P), ("N", _L), ("Nk", _L), ("P", _L),
                ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("T", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class TwoWayUpdateArgs(ctypes.Structure):
    """tmr_twoway_update_args_t (include/tmr_twoway.h)."""
    _fields_ = [("keys_in", _P), ("pe", _P), ("A", _P), ("c", _P), ("B", _P), ("bo", _P), ("g", _P), ("beta", _P),
                ("keys_out", _P), ("N", _L), ("Nk", _L), ("P", _L), ("C", ctypes.c_int32), ("H", ctypes.c_int32),
                ("T", ctypes.c_int32), ("eps", ctypes.c_float)]


class TwoWayPlan(ctypes.Structure):
    """tmr_twoway_plan_t (include/tmr_twoway.h)."""
    _fields_ = [("variant", ctypes.c_int32), ("tile_pixels", ctypes.c_int32), ("chunk_pixels", ctypes.c_int32),
                ("chunks", ctypes.c_int32), ("threads", ctypes.c_int32), ("lds_bytes", ctypes.c_int32),
                ("blocks", ctypes.c_int32), ("pad_", ctypes.c_int32)]


# the two-way transformer's image side (include/tmr_twoway.h): same libtmr.so, outside the core ABI as well
TWOWAY_HEADER = os.path.join(os.path.dirname(_HERE), "include", "tmr_twoway.h")
TWOWAY_SIGNATURES = {
    "tmr_twoway_pool": (_I, [ctypes.POINTER(TwoWayPoolArgs), _P]),
    "tmr_twoway_update": (_I, [ctypes.POINTER(TwoWayUpdateArgs), _P]),
    "tmr_twoway_pool_plan": (_I, [ctypes.POINTER(TwoWayPoolArgs), ctypes.POINTER(TwoWayPlan)]),
    "tmr_twoway_update_plan": (_I, [ctypes.POINTER(TwoWayUpdateArgs), ctypes.POINTER(TwoWayPlan)]),
}
TWOWAY_VARIANTS = {0: "f32mfma"}  # TMR_TWOWAY_VARIANT_*
TWOWAY_DIM, TWOWAY_HEADS, TWOWAY_ROWS = 256, 8, 64  # the one shape the kernels are built for; TMR_TWOWAY_ROWS
TWOWAY_POOL_CHUNK = 512  # TMR_TWOWAY_POOL_CHUNK


def twoway_pool_work_bytes(N: int, P: int) -> int:
    """TMR_TWOWAY_POOL_WORK_BYTES(N, P)."""
    return N * ((P + TWOWAY_POOL_CHUNK - 1) // TWOWAY_POOL_CHUNK) * TWOWAY_ROWS * (TWOWAY_DIM + 2) * 4


class TokLinear(ctypes.Structure):
    """tmr_tok_linear_t (include/tmr_tokens.h)."""
    _fields_ = [("w", _P), ("b", _P), ("in_", ctypes.c_int32), ("out", ctypes.c_int32)]


class TokAttn(ctypes.Structure):
    """tmr_tok_attn_t (include/tmr_tokens.h)."""
    _fields_ = [("q", TokLinear), ("k", TokLinear), ("v", TokLinear), ("o", TokLinear)]


class TokNorm(ctypes.Structure):
    """tmr_tok_norm_t (include/tmr_tokens.h)."""
    _fields_ = [("g", _P), ("b", _P), ("eps", ctypes.c_float), ("pad_", ctypes.c_int32)]


class TokMlp3(ctypes.Structure):
    """tmr_tok_mlp3_t (include/tmr_tokens.h)."""
    _fields_ = [("l", TokLinear * 3)]


TOKENS_MAX_MASKS, TOKENS_HYPER_OUT, TOKENS_MLP_CHUNK = 8, 32, 512  # TMR_TOKENS_MAX_MASKS, _HYPER_OUT, _MLP_CHUNK


class TokensFrontArgs(ctypes.Structure):
    """tmr_tokens_front_args_t (include/tmr_tokens.h)."""
    _fields_ = [("x", _P), ("p", _P), ("x1", _P), ("qf", _P), ("self_attn", TokAttn), ("norm1", TokNorm),
                ("cross", TokAttn), ("N", _L), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("T", ctypes.c_int32),
                ("has_self_attn", ctypes.c_int32), ("skip_pe", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class TokensBackArgs(ctypes.Structure):
    """tmr_tokens_back_args_t (include/tmr_tokens.h)."""
    _fields_ = [("x1", _P), ("p", _P), ("ctx", _P), ("x_out", _P), ("A", _P), ("c", _P), ("B", _P), ("t2i", TokAttn),
                ("norm", TokNorm), ("lin1", TokLinear), ("lin2", TokLinear), ("norm3", TokNorm), ("i2t", TokAttn),
                ("N", _L), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("T", ctypes.c_int32),
                ("has_mlp", ctypes.c_int32)]


class TokensTailArgs(ctypes.Structure):
    """tmr_tokens_tail_args_t (include/tmr_tokens.h)."""
    _fields_ = [("hs", _P), ("iou_pred", _P), ("hyper_all", _P), ("iou", TokMlp3), ("hyper", TokMlp3 * TOKENS_MAX_MASKS),
                ("N", _L), ("C", ctypes.c_int32), ("T", ctypes.c_int32), ("M", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class TokensPlan(ctypes.Structure):
    """tmr_tokens_plan_t (include/tmr_tokens.h)."""
    _fields_ = [("variant", ctypes.c_int32), ("threads", ctypes.c_int32), ("lds_bytes", ctypes.c_int32),
                ("blocks", ctypes.c_int32), ("prompts_per_block", ctypes.c_int32), ("pad_", ctypes.c_int32)]


# the mask decoder's token side (include/tmr_tokens.h): same libtmr.so, outside the core ABI as well
TOKENS_HEADER = os.path.join(os.path.dirname(_HERE), "include", "tmr_tokens.h")
TOKENS_SIGNATURES = {
    "tmr_tokens_front": (_I, [ctypes.POINTER(TokensFrontArgs), _P]),
    "tmr_tokens_back": (_I, [ctypes.POINTER(TokensBackArgs), _P]),
    "tmr_tokens_tail": (_I, [ctypes.POINTER(TokensTailArgs), _P]),
    "tmr_tokens_front_plan": (_I, [ctypes.POINTER(TokensFrontArgs), ctypes.POINTER(TokensPlan)]),
    "tmr_tokens_back_plan": (_I, [ctypes.POINTER(TokensBackArgs), ctypes.POINTER(TokensPlan)]),
    "tmr_tokens_tail_plan": (_I, [ctypes.POINTER(TokensTailArgs), ctypes.POINTER(TokensPlan)]),
}
TOKENS_VARIANTS = {0: "f32mfma"}  # TMR_TOKENS_VARIANT_*


# decoder_b's chain at the candidates (include/tmr_points_chain.h): same libtmr.so, outside the core ABI as well
POINTS_CHAIN_HEADER = os.path.join(os.path.dirname(_HERE), "include", "tmr_points_chain.h")
POINTS_CHAIN_SIGNATURES = {
    "tmr_split_conv_points_chain": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I,
                                         _I, _P, _P, _P, _P, _I, _P, _I, _P]),
}


class TMRError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libtmr.so (once).  Raises TMRError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise TMRError(
                f"libtmr.so not found at {LIB_PATH}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(EXT_SIGNATURES.items())
                                  + list(COCO_SIGNATURES.items()) + list(MASKHEAD_SIGNATURES.items())
                                  + list(TWOWAY_SIGNATURES.items()) + list(POINTS_CHAIN_SIGNATURES.items())
                                  + list(TOKENS_SIGNATURES.items())):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.tmr_version() != ABI_VERSION:
            raise TMRError("libtmr.so ABI version mismatch")
        _lib = lib
        return lib


def split_tile_window(first: int, count: int) -> int:
    """TMR_SPLIT_TILE_WINDOW: the flags bits of a channel-tile window (0, 0 = every tile)."""
    if not (0 <= first < 256 and 0 <= count < 128):
        raise TMRError("tile window out of range")
    return (first << SPLIT_TILE_FIRST_SHIFT) | (count << SPLIT_TILE_COUNT_SHIFT)


def split_tile_window_of(flags: int):
    """(first, count) of a flags word's tile window."""
    return (flags >> SPLIT_TILE_FIRST_SHIFT) & 0xff, (flags >> SPLIT_TILE_COUNT_SHIFT) & 0x7f


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().tmr_strerror(rc).decode()
        raise TMRError(f"{what}: {msg} (rc={rc})" if what else msg)


def ptr(t) -> int | None:
    """Device pointer of a tensor (None -> NULL).  CPU tensors are rejected."""
    if t is None:
        return None
    if not t.is_cuda:
        raise TMRError("tmr_amd kernels run on the GPU only; got a CPU tensor")
    if not t.is_contiguous():
        raise TMRError("tmr_amd kernels need contiguous tensors")
    return t.data_ptr()


def stream(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def call(name: str, *args) -> None:
    check(getattr(load(), name)(*args), name)


def size(kind: str, *dims) -> int:
    """tmr_size: bytes (or floats) of a caller-provided buffer; raises on
    invalid dimensions."""
    d = [int(x) for x in dims] + [0] * (6 - len(dims))
    n = int(load().tmr_size(SIZE_KINDS[kind], *d))
    if n < 0:
        raise TMRError(f"tmr_size({kind}, {dims}): invalid dimensions")
    return n


def _fill(struct, what: str, fields: dict):
    """A ctypes.Structure from keyword fields (pointer fields take ptr(...) or None; omitted and
    None fields are 0 / NULL).  A name the struct lacks is an error, never a Python attribute."""
    unknown = set(fields) - {n for n, _ in struct._fields_ if n != "pad_"}
    if unknown:
        raise TMRError(f"{what} has no field(s) {sorted(unknown)}")
    a = struct()
    for k, v in fields.items():
        if v is not None:
            setattr(a, k, v)
    return a


def xcorr(stream=None, **fields) -> None:
    """tmr_xcorr(&args, stream) with a tmr_xcorr_args_t from keyword fields."""
    check(load().tmr_xcorr(ctypes.byref(_fill(XcorrArgs, "tmr_xcorr_args_t", fields)), stream), "tmr_xcorr")


def xcorr_plan_rc(**fields):
    """tmr_xcorr_plan(&args, &plan) -> (return code, (kernel name, band_rows, col_groups, out16) or None):
    the kernel tmr_xcorr would launch for these fields; host only, nothing is launched."""
    plan = XcorrPlan()
    fields.pop("stream", None)
    rc = load().tmr_xcorr_plan(ctypes.byref(_fill(XcorrArgs, "tmr_xcorr_args_t", fields)), ctypes.byref(plan))
    if rc != 0:
        return rc, None
    return rc, (XCORR_KERNELS[plan.kernel], plan.band_rows, plan.col_groups, plan.out16)


def xcorr_plan(**fields):
    """xcorr_plan_rc's plan; raises TMRError where tmr_xcorr would refuse the launch."""
    rc, plan = xcorr_plan_rc(**fields)
    check(rc, "tmr_xcorr_plan")
    return plan


def gt_loss_args(**fields) -> GtLossArgs:
    return _fill(GtLossArgs, "tmr_gt_loss_args_t", fields)


def gt_loss(stream_=None, **fields) -> None:
    """tmr_gt_loss(&args, stream)."""
    check(load().tmr_gt_loss(ctypes.byref(gt_loss_args(**fields)), stream_), "tmr_gt_loss")


def mask_boxes(stream_=None, **fields) -> None:
    """tmr_mask_boxes(&args, stream) (include/tmr_refine.h)."""
    check(load().tmr_mask_boxes(ctypes.byref(_fill(MaskBoxesArgs, "tmr_mask_boxes_args_t", fields)), stream_),
          "tmr_mask_boxes")


def mask_boxes_plan(**fields):
    """tmr_mask_boxes_plan(&args, ...) -> (band_rows, cap_rows, nbands); host only.  With N = 0 (the
    default) the geometry of (h, w, H, W) alone, whatever the pointers."""
    out = [ctypes.c_int32() for _ in range(3)]
    check(load().tmr_mask_boxes_plan(ctypes.byref(_fill(MaskBoxesArgs, "tmr_mask_boxes_args_t", fields)),
                                     *(ctypes.byref(o) for o in out)), "tmr_mask_boxes_plan")
    return tuple(o.value for o in out)


def coco_match(stream_=None, **fields) -> None:
    """tmr_coco_match(&args, stream) (include/tmr_coco.h)."""
    check(load().tmr_coco_match(ctypes.byref(_fill(CocoMatchArgs, "tmr_coco_match_args_t", fields)), stream_),
          "tmr_coco_match")


def coco_match_plan_rc(**fields):
    """tmr_coco_match_plan(&args, &plan) -> (return code, plan dict or None); host only."""
    plan = CocoMatchPlan()
    rc = load().tmr_coco_match_plan(ctypes.byref(_fill(CocoMatchArgs, "tmr_coco_match_args_t", fields)),
                                    ctypes.byref(plan))
    if rc != 0:
        return rc, None
    out = {n: getattr(plan, n) for n, _ in CocoMatchPlan._fields_}
    out["variant"] = COCO_VARIANTS[plan.variant]
    return rc, out


def coco_match_plan(**fields):
    """coco_match_plan_rc's plan; raises TMRError where tmr_coco_match would refuse the call."""
    rc, plan = coco_match_plan_rc(**fields)
    check(rc, "tmr_coco_match_plan")
    return plan


def mask_head_prep(stream_=None, **fields) -> None:
    """tmr_mask_head_prep(&args, stream) (include/tmr_maskhead.h)."""
    check(load().tmr_mask_head_prep(ctypes.byref(_fill(MaskHeadArgs, "tmr_mask_head_args_t", fields)), stream_),
          "tmr_mask_head_prep")


def mask_head(stream_=None, **fields) -> None:
    """tmr_mask_head(&args, stream) (include/tmr_maskhead.h)."""
    check(load().tmr_mask_head(ctypes.byref(_fill(MaskHeadArgs, "tmr_mask_head_args_t", fields)), stream_),
          "tmr_mask_head")


def mask_head_plan_rc(**fields):
    """tmr_mask_head_plan(&args, &plan) -> (return code, plan dict or None); host only."""
    plan = MaskHeadPlan()
    fields.setdefault("C", MASK_HEAD_DIM)
    rc = load().tmr_mask_head_plan(ctypes.byref(_fill(MaskHeadArgs, "tmr_mask_head_args_t", fields)),
                                   ctypes.byref(plan))
    if rc != 0:
        return rc, None
    out = {n: getattr(plan, n) for n, _ in MaskHeadPlan._fields_}
    out["variant"] = MASK_HEAD_VARIANTS[plan.variant]
    return rc, out


def mask_head_plan(**fields):
    """mask_head_plan_rc's plan; raises TMRError where tmr_mask_head would refuse the call.  With
    N = 0 (the default) the geometry of (h, w) alone, whatever the pointers."""
    rc, plan = mask_head_plan_rc(**fields)
    check(rc, "tmr_mask_head_plan")
    return plan


def _twoway_defaults(fields):
    fields.setdefault("C", TWOWAY_DIM)
    fields.setdefault("H", TWOWAY_HEADS)
    if "Nk" not in fields:
        fields["Nk"] = fields.get("N", 0) or 1
    return fields


def twoway_pool(stream_=None, **fields) -> None:
    """tmr_twoway_pool(&args, stream) (include/tmr_twoway.h)."""
    a = _fill(TwoWayPoolArgs, "tmr_twoway_pool_args_t", _twoway_defaults(fields))
    check(load().tmr_twoway_pool(ctypes.byref(a), stream_), "tmr_twoway_pool")


def twoway_update(stream_=None, **fields) -> None:
    """tmr_twoway_update(&args, stream) (include/tmr_twoway.h)."""
    a = _fill(TwoWayUpdateArgs, "tmr_twoway_update_args_t", _twoway_defaults(fields))
    check(load().tmr_twoway_update(ctypes.byref(a), stream_), "tmr_twoway_update")


def _twoway_plan_rc(fn, struct, what, fields):
    plan = TwoWayPlan()
    rc = getattr(load(), fn)(ctypes.byref(_fill(struct, what, _twoway_defaults(fields))), ctypes.byref(plan))
    if rc != 0:
        return rc, None
    out = {n: getattr(plan, n) for n, _ in TwoWayPlan._fields_ if n != "pad_"}
    out["variant"] = TWOWAY_VARIANTS[plan.variant]
    return rc, out


def twoway_pool_plan_rc(**fields):
    """tmr_twoway_pool_plan(&args, &plan) -> (return code, plan dict or None); host only.  Nk defaults
    to N (1 when N = 0), C and H to 256 and 8."""
    return _twoway_plan_rc("tmr_twoway_pool_plan", TwoWayPoolArgs, "tmr_twoway_pool_args_t", fields)


def twoway_update_plan_rc(**fields):
    """tmr_twoway_update_plan(&args, &plan) -> (return code, plan dict or None); host only."""
    return _twoway_plan_rc("tmr_twoway_update_plan", TwoWayUpdateArgs, "tmr_twoway_update_args_t", fields)


def twoway_pool_plan(**fields):
    """twoway_pool_plan_rc's plan; raises TMRError where tmr_twoway_pool would refuse the call.  With
    N = 0 (the default) the geometry of (P, T) alone, whatever the pointers."""
    rc, plan = twoway_pool_plan_rc(**fields)
    check(rc, "tmr_twoway_pool_plan")
    return plan


def twoway_update_plan(**fields):
    """twoway_update_plan_rc's plan; raises TMRError where tmr_twoway_update would refuse the call."""
    rc, plan = twoway_update_plan_rc(**fields)
    check(rc, "tmr_twoway_update_plan")
    return plan


def tok_linear(w, b, in_, out) -> TokLinear:
    """tmr_tok_linear_t from two addresses (or None) and the layer's sizes."""
    return TokLinear(w, b, int(in_), int(out))


def tok_attn(q, k, v, o) -> TokAttn:
    return TokAttn(q, k, v, o)


def tok_norm(g, b, eps) -> TokNorm:
    return TokNorm(g, b, float(eps), 0)


def tok_mlp3(l0, l1, l2) -> TokMlp3:
    return TokMlp3((TokLinear * 3)(l0, l1, l2))


def _tokens_args(struct, what, fields):
    """A tokens args struct from keyword fields: plain ones through _fill (C and H default to 256
    and 8), descriptor structs (and the list `hyper`) assigned as they are."""
    nested = {k: fields.pop(k) for k in list(fields) if isinstance(fields[k], (ctypes.Structure, list, tuple))}
    names = {n for n, _ in struct._fields_}
    if "C" in names:
        fields.setdefault("C", TWOWAY_DIM)
    if "H" in names:
        fields.setdefault("H", TWOWAY_HEADS)
    a = _fill(struct, what, fields)
    for k, v in nested.items():
        if k not in names:
            raise TMRError(f"{what} has no field(s) {[k]}")
        if k == "hyper":
            if len(v) > TOKENS_MAX_MASKS:
                raise TMRError(f"{what}: at most {TOKENS_MAX_MASKS} hypernetwork MLPs")
            for i, m in enumerate(v):
                a.hyper[i] = m
        else:
            setattr(a, k, v)
    return a


_TOKENS = {"front": (TokensFrontArgs, "tmr_tokens_front"), "back": (TokensBackArgs, "tmr_tokens_back"),
           "tail": (TokensTailArgs, "tmr_tokens_tail")}


def tokens_args(which: str, **fields):
    """The args struct of tmr_tokens_<which> ("front", "back", "tail") from keyword fields."""
    struct, fn = _TOKENS[which]
    return _tokens_args(struct, fn + "_args_t", fields)


def tokens_launch(which: str, stream_=None, **fields) -> None:
    """tmr_tokens_<which>(&args, stream) (include/tmr_tokens.h)."""
    struct, fn = _TOKENS[which]
    check(getattr(load(), fn)(ctypes.byref(_tokens_args(struct, fn + "_args_t", fields)), stream_), fn)


def tokens_plan_rc(which: str, **fields):
    """tmr_tokens_<which>_plan(&args, &plan) -> (return code, plan dict or None); host only."""
    struct, fn = _TOKENS[which]
    plan = TokensPlan()
    rc = getattr(load(), fn + "_plan")(ctypes.byref(_tokens_args(struct, fn + "_args_t", fields)), ctypes.byref(plan))
    if rc != 0:
        return rc, None
    out = {n: getattr(plan, n) for n, _ in TokensPlan._fields_ if n != "pad_"}
    out["variant"] = TOKENS_VARIANTS[plan.variant]
    return rc, out


def tokens_plan(which: str, **fields):
    """tokens_plan_rc's plan; raises TMRError where the launch would refuse the call."""
    rc, plan = tokens_plan_rc(which, **fields)
    check(rc, f"tmr_tokens_{which}_plan")
    return plan


def require_gpu(t: torch.Tensor, name: str = "input") -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TMRError(f"{name} must be a tensor on a HIP device (MI355X); no CPU path exists")
