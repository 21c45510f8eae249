"""Recorder of libtmr.so calls and the flows whose call traces are pinned
(tests/test_gpu_launch_trace.py, tools/make_golden_launch_trace.py).

Most routes of the engine change only speed: the shared fp half, the bf16
accumulator slabs, the image-major heads order, the bf16 f_TM plane, the
per-image memo.  Value comparisons cannot see one of them go missing; the
sequence of native calls and their scalar arguments can.

The recorder swaps tmr_amd._lib._lib (what _lib.load() returns, and every
entry point is reached through load() at call time) for a proxy around the
loaded library.  Flows use the public engine and module API only.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

import oracle
import tmr_amd
from tmr_amd import _lib, synth

DEV = torch.device("cuda:0")
UNRECORDED = ("tmr_size", "tmr_version", "tmr_strerror")


def _norm(v, ctype):
    if ctype is ctypes.c_void_p:
        return "null" if not v else "p"
    if isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer):
        s = v._obj  # ctypes.byref(struct)
        return {n: _norm(getattr(s, n), t) for n, t in s._fields_}
    if ctype is ctypes.c_double:
        return float(v)
    return int(v)


class _Proxy:
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _lib.SIGNATURES or name in UNRECORDED:
            return fn
        argtypes = _lib.SIGNATURES[name][1]

        def recorded(*args):
            self._calls.append([name] + [_norm(a, t) for a, t in zip(args, argtypes)])
            return fn(*args)

        return recorded


class record:
    """with record() as calls: ... -> calls = [[symbol, arg, ...], ...]."""

    def __enter__(self):
        self.lib = _lib.load()
        self.calls = []
        _lib._lib = _Proxy(self.lib, self.calls)
        return self.calls

    def __exit__(self, *exc):
        _lib._lib = self.lib
        return False


# ------------------------------------------------------------------ flows
def _units_flow(E, precision, algo):
    """forward_units over 2 images x E exemplars on a 64 x 64 map."""
    def run():
        P = synth.reference_state_dict(31, cin=8, emb=16)
        eng = tmr_amd.TMREngine({k: v.to(DEV) for k, v in P.items()},
                                tmr_amd.PathConfig(emb_dim=16, precision=precision))
        eng.xcorr_algo = algo
        feats = torch.from_numpy(synth.sam_features(32, 2, 8, 32, 32)).to(DEV)
        ex, _ = synth.exemplar_set(33, 2, E, 64, 64, 3, 9)
        with record() as calls:
            eng.forward_units(feats, np.repeat(np.arange(2), E), ex.reshape(-1, 4))
            torch.cuda.synchronize()
        return [calls]
    return run


def _variant_flow(**switch):
    """forward_units of one architecture switch: 2 images x 2 exemplars, 32 x 32 map."""
    def run():
        kw = dict(num_layers=switch.get("decoder_num_layer", 1), k=switch.get("decoder_kernel_size", 3),
                  squeeze=switch.get("squeeze", False), fusion=switch.get("fusion", True))
        P = oracle.reference_weights(41, cin=8, emb=16, **kw)
        eng = tmr_amd.TMREngine({k: v.to(DEV) for k, v in P.items()}, tmr_amd.PathConfig(emb_dim=16, **switch))
        eng.xcorr_algo = "valu"
        feats = torch.from_numpy(synth.sam_features(42, 2, 8, 16, 16)).to(DEV)
        ex, _ = synth.exemplar_set(43, 2, 2, 32, 32, 3, 7)
        with record() as calls:
            eng.forward_units(feats, np.repeat(np.arange(2), 2), ex.reshape(-1, 4))
            torch.cuda.synchronize()
        return [calls]
    return run


def _detect_flow(setup, ncalls=1):
    """detect() over 2 images x 3 exemplars on a 64 x 64 map, decoder_b one
    128-channel tile, dense near-tied candidates."""
    def run():
        P = synth.reference_state_dict(51, cin=16, emb=64, obj_bias=0.3)
        eng = tmr_amd.TMREngine({k: v.to(DEV) for k, v in P.items()}, tmr_amd.PathConfig(emb_dim=64))
        eng.xcorr_algo = "mfma"
        setup(eng)
        feats = torch.from_numpy(synth.sam_features(52, 2, 16, 32, 32)).to(DEV)
        ex, _ = synth.exemplar_set(53, 2, 3, 64, 64, 3, 9)
        traces = []
        for _ in range(ncalls):
            with record() as calls:
                eng.detect(feats, ex, cls_ths=0.5, iou_threshold=0.5)
                torch.cuda.synchronize()
            traces.append(calls)
        return traces, eng
    return run


def _points(eng):
    eng.use_graphs = False
    eng.box_at_peaks = "always"


def _dense(eng):  # as test_gpu_guarded._dense_fallback
    eng.use_graphs = False
    eng.BOX_POINTS_CROSSOVER = {k: 0.0 for k in eng.BOX_POINTS_CROSSOVER}


def _detect_points():
    traces, eng = _detect_flow(_points)()
    assert eng.last_box_route == "points" and eng.last_points > 0
    return traces


def _detect_dense():
    traces, eng = _detect_flow(_dense)()
    assert eng.last_box_route == "dense" and eng.last_points > 0
    return traces


def _detect_graphs_first_call():
    traces, eng = _detect_flow(lambda eng: None)()
    assert eng.last_graph == "eager"
    return traces


class _Passthrough(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.num_channels = c

    def forward(self, x):
        return x


def _module_reuse():
    """The module API (reuse_image_work), graphs off: two exemplar calls on
    one feature tensor."""
    args = SimpleNamespace(emb_dim=16, fusion=True, ablation_no_box_regression=False, encoder="original",
                           feature_upsample=True, no_matcher=False, template_type="roi_align", squeeze=False,
                           decoder_num_layer=1, decoder_kernel_size=3, modeltype="matching_net")
    model = tmr_amd.matching_net(_Passthrough(8), args)
    model.load_state_dict(oracle.reference_weights(61, cin=8, emb=16), strict=True)
    model = model.to(DEV).eval()
    eng = model.engine()
    eng.use_graphs = False
    eng.xcorr_algo = "valu"
    feats = torch.from_numpy(synth.sam_features(62, 1, 8, 16, 16)).to(DEV)
    ex, _ = synth.exemplar_set(63, 1, 2, 32, 32, 3, 7)
    traces = []
    with torch.no_grad():
        for e in range(2):
            with record() as calls:
                model(feats, [torch.from_numpy(ex[0, e:e + 1]).to(DEV)])
                torch.cuda.synchronize()
            traces.append(calls)
    return traces


FLOWS = {
    "units_e1_fp32": _units_flow(1, "fp32", "valu"),
    "units_e1_bf16": _units_flow(1, "bf16", "mfma"),
    "units_e1_f16": _units_flow(1, "f16", "mfma"),
    "units_e3_fp32": _units_flow(3, "fp32", "valu"),
    "units_e3_bf16": _units_flow(3, "bf16", "mfma"),
    "units_e3_f16": _units_flow(3, "f16", "mfma"),
    "no_fusion": _variant_flow(fusion=False),
    "no_matcher": _variant_flow(no_matcher=True),
    "squeeze": _variant_flow(squeeze=True),
    "two_layers": _variant_flow(decoder_num_layer=2),
    "kernel5": _variant_flow(decoder_kernel_size=5),
    "detect_points": _detect_points,
    "detect_dense": _detect_dense,
    "detect_graphs_first_call": _detect_graphs_first_call,
    "module_reuse": _module_reuse,
}


def run_flow(name):
    """The traces (one list of calls per recorded API call) of a flow, as
    plain JSON values."""
    return FLOWS[name]()
