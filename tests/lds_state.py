"""Known LDS contents in front of a kernel under test (tests/lds_state/).

Every MFMA kernel of the package pads its tiles with zero operands, which is
safe only where the other operand was staged: 0 x (stale LDS bits) can be NaN.
Whether a run catches such a read depends on what the previous kernel on that
CU left in its LDS.  This module decides it: `lds_fill` launches blocks that
each own the whole 160 KiB of a CU's LDS and write one 32-bit pattern to every
word, so the next dispatch on the stream starts on LDS that holds the pattern.

    with filled(PATTERN_FF):            # every stream-taking libtmr.so call is
        out = run_the_flow()            # preceded by a fill on its own stream

    out = fill_then(PATTERN_FF, fn)     # fill on the current stream, then fn()

A result that read an LDS word its kernel did not write differs between the
patterns: PATTERN_ZERO is the benign state and always runs first; PATTERN_FF is
NaN as fp32, fp16 and bf16 and -1 as an index; PATTERN_7B is a large finite
value in all three formats (fmaxf-style reductions ignore NaN, so a stale word
in a maximum only shows with a finite poison).

What it cannot do.  Registers cannot be filled, neither can LDS addresses
outside a kernel's allocation.  Only the first block a CU runs after the fill
sees the poison (a later block sees the leavings of an earlier one), so cases
keep their grids at or below one block per CU.  Of an entry point that launches
several kernels only the first starts on filled LDS.  Another tenant's kernel
between the fill and the launch weakens a case: that can produce a miss, never
a false alarm.  Graph replay is out of scope.  Not a conftest, not a plugin:
tests import it.
"""
import contextlib
import ctypes
import os

PATTERN_ZERO = 0x00000000
PATTERN_FF = 0xFFFFFFFF
PATTERN_7B = 0x7B7B7B7B
PATTERNS = (PATTERN_ZERO, PATTERN_FF, PATTERN_7B)

# blocks of one fill or probe = FILL_MULTIPLE x the device's CU count (measured: DESIGN.md,
# "LDS state"; test_fill_reaches_every_cu holds it to that)
FILL_MULTIPLE = 8

HELPER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lds_state", "liblds_state.so")
# entry points of libtmr.so that launch nothing, whatever their last parameter is
PASS_THROUGH = ("tmr_size", "tmr_version", "tmr_strerror", "tmr_exp_table_encode", "tmr_exp_table_decode")

_helper = None


class LdsStateError(RuntimeError):
    pass


def helper():
    """liblds_state.so (once)."""
    global _helper
    if _helper is None:
        if not os.path.exists(HELPER_PATH):
            raise LdsStateError(f"{HELPER_PATH} not found; build it with "
                                "`python -c 'import __graft_entry__ as g; g.build()'`")
        lib = ctypes.CDLL(HELPER_PATH)
        p, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        for name, args in (("lds_fill", [u, i, p]), ("lds_probe", [u, i, p, p, p]), ("lds_planted_read", [p, p]),
                           ("lds_planted_blocks", [])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = i, args
        _helper = lib
    return _helper


def signature_tables():
    """name -> (restype, argtypes) of every symbol tmr_amd._lib.load() binds."""
    from tmr_amd import _lib as L
    out = {}
    for name in dir(L):
        if name == "SIGNATURES" or name.endswith("_SIGNATURES"):
            out.update(getattr(L, name))
    return out


def stream_entry_points(tables=None):
    """The bound entry points that launch on a caller's stream: the last parameter is a void *
    (the stream), and the name is neither a *_plan nor one of PASS_THROUGH."""
    tables = signature_tables() if tables is None else tables
    return sorted(n for n, (_, args) in tables.items()
                  if args and args[-1] is ctypes.c_void_p and not n.endswith("_plan") and n not in PASS_THROUGH)


def fill_blocks():
    import torch
    return FILL_MULTIPLE * torch.cuda.get_device_properties(0).multi_processor_count


def fill(pattern, stream, blocks=None, lib=None):
    """lds_fill(pattern) on `stream` (a raw handle or None)."""
    rc = (lib or helper()).lds_fill(pattern, fill_blocks() if blocks is None else blocks, stream)
    if rc != 0:
        raise LdsStateError(f"lds_fill failed (rc={rc})")


def probe(pattern, blocks=None):
    """lds_probe on the current stream -> (keys, bad): the CU key and the count of words that
    differ from `pattern`, per block, as host arrays."""
    import torch
    blocks = fill_blocks() if blocks is None else blocks
    keys = torch.zeros(blocks, dtype=torch.int32, device="cuda:0")
    bad = torch.zeros(blocks, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = helper().lds_probe(pattern, blocks, keys.data_ptr(), bad.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise LdsStateError(f"lds_probe failed (rc={rc})")
    torch.cuda.synchronize()
    return keys.cpu().numpy(), bad.cpu().numpy()


def planted_read():
    """lds_planted_read on the current stream -> float32[blocks] on the host (2016.0 each when exact)."""
    import torch
    out = torch.full((helper().lds_planted_blocks(),), -1.0, dtype=torch.float32, device="cuda:0")
    rc = helper().lds_planted_read(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise LdsStateError(f"lds_planted_read failed (rc={rc})")
    return out.cpu().numpy()


class FillingProxy:
    """Stands in for the ctypes handle of libtmr.so: every wrapped entry point first launches
    fill(pattern, <its stream argument>), then makes the real call and returns its code."""

    def __init__(self, real, pattern, wrapped, fill_fn):
        self._real, self._pattern, self._wrapped, self._fill = real, pattern, frozenset(wrapped), fill_fn
        self.calls = []  # names of the wrapped calls made, in order

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._wrapped:
            return fn

        def call(*args):
            self._fill(self._pattern, args[-1])
            self.calls.append(name)
            return fn(*args)

        call.__name__ = name
        return call


@contextlib.contextmanager
def filled(pattern, only=None, lib_module=None, fill_fn=None):
    """Swap tmr_amd._lib._lib (the handle load() returns) for a FillingProxy; pattern None leaves
    the handle alone (the unfilled run).  only: wrap these entry points alone.  Yields the proxy."""
    if lib_module is None:
        from tmr_amd import _lib as lib_module
    if pattern is None:
        yield None
        return
    real = lib_module.load()
    wrapped = stream_entry_points() if only is None else only
    proxy = FillingProxy(real, pattern, wrapped, fill_fn or fill)
    lib_module._lib = proxy
    try:
        yield proxy
    finally:
        lib_module._lib = real


def fill_then(pattern, fn):
    """Fill on the current stream, then fn(), with nothing launched in between: allocate and
    pre-fill every buffer before.  pattern None: fn() alone."""
    if pattern is not None:
        import torch
        fill(pattern, torch.cuda.current_stream().cuda_stream)
    return fn()
