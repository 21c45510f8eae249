"""HIP-graph capture and replay of an engine forward: the pinned blob of its
tagged host inputs, the staging copy that becomes a view of it inside a
capture (_h2d), the capture itself, and which launch signatures are captured."""
from __future__ import annotations

import gc
import threading
import weakref
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from ._lib import TMRError

# while a forward is being captured, every tagged host input staged by _h2d
# is a view of the capture's _HostBlob
_capture = threading.local()


def capturing() -> bool:
    return getattr(_capture, "blob", None) is not None


class _HostBlob:
    """The tagged host inputs of a captured forward in ONE pinned buffer and
    ONE device buffer: the capture's first node copies the pinned bytes up,
    every tagged _h2d inside the capture is a view of the device buffer, and a
    replay only rewrites the pinned bytes -- one copy node per forward instead
    of one per input (each is a ~5 us blit on the GPU's timeline)."""

    def __init__(self, host_in: Dict[str, np.ndarray], device):
        self.offs: Dict[str, tuple] = {}
        o = 0
        for t, a in host_in.items():
            if a.nbytes:
                self.offs[t] = (o, a.nbytes)
                o += (a.nbytes + 15) // 16 * 16  # 16-B aligned sections
        self.pinned = torch.empty(max(o, 16), dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(max(o, 16), dtype=torch.uint8, device=device)
        self.fill(host_in)

    def fill(self, host: Dict[str, np.ndarray]):
        pn = self.pinned.numpy()
        for t, a in host.items():
            if t in self.offs:
                o, n = self.offs[t]
                pn[o:o + n] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)

    def upload(self):  # inside the capture, before anything reads the inputs
        self.dev.copy_(self.pinned, non_blocking=True)

    def view(self, tag: Optional[str], t: torch.Tensor) -> torch.Tensor:
        o, n = self.offs.get(tag, (0, -1)) if tag is not None else (0, -1)
        if n != t.numel() * t.element_size():
            raise TMRError(f"host input {tag!r} inside a graph capture has no pre-allocated slot")
        pn = self.pinned.numpy()
        pn[o:o + n] = t.numpy().reshape(-1).view(np.uint8)  # (the capture's own values)
        return self.dev[o:o + n].view(t.dtype).reshape(t.shape)


def _h2d(arr: np.ndarray, device, dtype=None, tag: Optional[str] = None) -> torch.Tensor:
    """A small host array on the device WITHOUT a stream sync: staged through
    torch's caching pinned-memory allocator and copied non_blocking (the
    allocator keeps the pinned block until the copy's stream event has
    completed).  A pageable `.to(device)` synchronises the stream, leaving the
    GPU idle while the host prepares the next launches.  Inside a graph
    capture a tagged input is a view of the capture's _HostBlob (the replay
    rewrites its pinned bytes)."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if dtype is not None:
        t = t.to(dtype)
    device = torch.device(device)
    if device.type != "cuda":
        return t.to(device)
    blob = getattr(_capture, "blob", None)
    if blob is None:
        return t.pin_memory().to(device, non_blocking=True)
    return blob.view(tag, t)


def _units_to_device(units: np.ndarray, device, tag: Optional[str] = None) -> torch.Tensor:
    return _h2d(units.view(np.uint8), device, tag=tag)


def _clone_outputs(out: Dict[str, object], keep=("fp",)) -> Dict[str, object]:
    """Fresh copies of a replayed graph's static outputs (a caller may keep
    one call's maps while the next replay runs): tensors that are contiguous
    views of one storage (o and b) are copied out by ONE copy of the range
    they cover; names in `keep` are returned as they are."""
    res, groups = {}, {}
    for k, v in out.items():
        if isinstance(v, torch.Tensor) and k not in keep:
            groups.setdefault(v.untyped_storage().data_ptr(), []).append(k)
        else:
            res[k] = v
    for ks in groups.values():
        ts = [out[k] for k in ks]
        if len(ks) == 1 or not all(t.is_contiguous() for t in ts):
            res.update({k: out[k].clone() for k in ks})
            continue
        lo = min(t.storage_offset() for t in ts)
        hi = max(t.storage_offset() + t.numel() for t in ts)
        base = ts[0].as_strided((hi - lo,), (1,), lo).clone()
        for k, t in zip(ks, ts):
            res[k] = base.as_strided(t.shape, t.stride(), t.storage_offset() - lo)
    return res


class _GraphBook:
    """Which launch signatures have a captured graph, how often the others
    were seen, and which failed to capture.  A signature is captured on its
    second sighting; the seen-counts are an LRU bounded by `seen_cap` (mapper
    workloads with varied exemplar sizes make a new signature almost every
    batch), graphs an LRU of `cap`, and a signature whose capture failed
    stays eager (bounded too) instead of retrying the sync + clone + capture
    on every call.  Host-only: tested on CPU."""

    def __init__(self, cap: int, seen_cap: int = 256):
        self.cap, self.seen_cap = cap, seen_cap
        self.graphs: "OrderedDict[tuple, object]" = OrderedDict()
        self.seen: "OrderedDict[tuple, int]" = OrderedDict()
        self.failed: "OrderedDict[tuple, None]" = OrderedDict()

    def get(self, sig):
        g = self.graphs.get(sig)
        if g is not None:
            self.graphs.move_to_end(sig)
        return g

    def want_capture(self, sig) -> bool:
        """Count a sighting of sig (no graph yet); True when it should be
        captured now (second sighting, never failed)."""
        if sig in self.failed:
            return False
        n = self.seen.pop(sig, 0) + 1
        self.seen[sig] = n
        while len(self.seen) > self.seen_cap:
            self.seen.popitem(last=False)
        return n >= 2

    def put(self, sig, g):
        self.seen.pop(sig, None)
        if g is None:
            self.failed[sig] = None
            while len(self.failed) > self.seen_cap:
                self.failed.popitem(last=False)
            return
        self.graphs[sig] = g
        while len(self.graphs) > self.cap:
            self.graphs.popitem(last=False)

    def clear(self):
        self.graphs.clear(); self.seen.clear(); self.failed.clear()


class _no_gc:
    """Python's cyclic GC off for the length of a graph capture: a collection
    inside the capture can destroy an unreachable object that owns a HIP
    event or graph (an evicted replay's), and a destroy call during a global
    capture aborts the process (seen once in
    test_module_graph_replays_back_to_back).  torch.cuda.graph collects on
    entry; this keeps it off until the capture has ended."""

    def __enter__(self):
        self.was = gc.isenabled()
        gc.collect()
        gc.disable()

    def __exit__(self, *exc):
        if self.was:
            gc.enable()
        return False


class _ForwardGraph:
    """One captured forward (projection ... peaks) for a fixed launch
    signature: the inputs are a static feature buffer and the pinned host
    blob of its tagged host inputs; the outputs the forward's static
    buffers.  A replay refills both and launches the whole forward at once."""

    def __init__(self, graph, feats, blob, outputs, last):
        self.graph, self.feats, self.blob, self.outputs, self.last = graph, feats, blob, outputs, last
        self.done = None  # event after the last replay: its copy node reads the pinned blob
        self.src = None  # (tensor ref, version, data_ptr) of the features last copied into feats
        self.memo = None  # module API, an image's first call: the capture's per-image memo

    def replay(self, engine, feats: torch.Tensor, host: Dict[str, np.ndarray], reuse_feats: bool = False):
        """Refill the inputs, launch, and give `engine` the last_* record of
        the captured forward.  reuse_feats (the module API's later exemplar
        calls on one image): skip the feature copy when the same tensor object
        at the same version was copied last.  detect() always copies: a write
        through a raw pointer or a caller's own graph replay changes a tensor
        without bumping its version."""
        # the blob is rewritten by the host at once: a previous replay still
        # queued (two calls with no sync between them) must have read it first
        if self.done is not None:
            self.done.synchronize()
        self.blob.fill(host)
        src = self.src
        if not reuse_feats or src is None or src[0]() is not feats or \
                src[1] != (feats._version, feats.data_ptr()):
            self.feats.copy_(feats)
            self.src = (weakref.ref(feats), (feats._version, feats.data_ptr()))
        self.graph.replay()
        if self.done is None:
            self.done = torch.cuda.Event()
        self.done.record()
        for k, v in self.last.items():
            setattr(engine, k, v)
        return self.outputs


def capture(engine, feats: torch.Tensor, host_in: Dict[str, np.ndarray], run) -> Optional[_ForwardGraph]:
    """Capture run(static) on a static copy of feats (caches built by the
    eager call that preceded), with host_in as the capture's host blob.  None
    when a launch in it cannot be captured (engine.last_graph_error says why)."""
    static = feats.detach().float().contiguous().clone()
    blob = _HostBlob(host_in, feats.device)
    torch.cuda.synchronize(feats.device)
    graph = torch.cuda.CUDAGraph()
    _capture.blob = blob
    try:
        with _no_gc(), torch.cuda.graph(graph):
            blob.upload()
            out = run(static)
    except Exception as err:  # noqa: BLE001 -- stay eager
        engine.last_graph_error = f"{type(err).__name__}: {err}"
        return None
    finally:
        _capture.blob = None
    last = {k: v for k, v in vars(engine).items() if k.startswith("last_") and not k.startswith("last_graph")}
    return _ForwardGraph(graph, static, blob, out, last)
