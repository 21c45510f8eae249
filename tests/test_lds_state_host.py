"""tests/lds_state.py without a GPU: the filling proxy against a fake library,
and the coverage table of tests/test_gpu_lds_state.py against the signature
tables of tmr_amd/_lib.py and the kernel sources."""
import ctypes
import os
import re
import types

import pytest

import lds_state as ls
import test_gpu_lds_state as T_lds
from tmr_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")


# ------------------------------------------------------------------ the proxy
class FakeLib:
    """Records (name, args) of every call; each entry point returns its own code."""

    def __init__(self, log):
        self.log = log
        for name, rc in (("tmr_xcorr", 0), ("tmr_nms", -3), ("tmr_xcorr_plan", 7), ("tmr_size", 4096),
                         ("tmr_version", 3), ("tmr_strerror", b"ok"), ("tmr_exp_table_decode", 11),
                         ("tmr_exp_table_encode", 12), ("tmr_mask_head_plan", 5)):
            setattr(self, name, self._fn(name, rc))

    def _fn(self, name, rc):
        def fn(*args):
            self.log.append((name, args))
            return rc
        return fn

    def tmr_boom(self, *args):
        raise RuntimeError("boom")


def _fake_module(log):
    m = types.SimpleNamespace()
    m._lib = FakeLib(log)
    m.load = lambda: m._lib
    return m


def _filled(m, log, pattern=ls.PATTERN_FF, only=None):
    names = ("tmr_xcorr", "tmr_nms", "tmr_boom") if only is None else only
    return ls.filled(pattern, only=names, lib_module=m,
                     fill_fn=lambda pat, stream: log.append(("lds_fill", (pat, stream))))


def test_wrapped_calls_fill_on_their_stream_and_return_the_real_code():
    log = []
    m = _fake_module(log)
    real = m._lib
    with _filled(m, log) as proxy:
        assert m.load() is proxy and proxy is not real
        assert m.load().tmr_xcorr("args", 0xBEEF) == 0
        assert m.load().tmr_nms(1, 2, None) == -3  # the real return code, the NULL stream as it is
        assert getattr(m.load(), "tmr_nms")(5, 0x10) == -3
    assert log == [("lds_fill", (ls.PATTERN_FF, 0xBEEF)), ("tmr_xcorr", ("args", 0xBEEF)),
                   ("lds_fill", (ls.PATTERN_FF, None)), ("tmr_nms", (1, 2, None)),
                   ("lds_fill", (ls.PATTERN_FF, 0x10)), ("tmr_nms", (5, 0x10))]
    assert proxy.calls == ["tmr_xcorr", "tmr_nms", "tmr_nms"]
    assert m._lib is real


def test_unwrapped_names_pass_through_untouched():
    log = []
    m = _fake_module(log)
    with _filled(m, log):
        lib = m.load()
        assert lib.tmr_size(1, 2) == 4096 and lib.tmr_version() == 3 and lib.tmr_strerror(0) == b"ok"
        assert lib.tmr_xcorr_plan("a", "p") == 7 and lib.tmr_mask_head_plan("a", "p") == 5
        assert lib.tmr_exp_table_decode(1, 2, 3, 4) == 11 and lib.tmr_exp_table_encode(1, 2, 3, 4) == 12
        assert lib.tmr_size == m._lib._real.tmr_size  # the real bound function itself
        with pytest.raises(AttributeError):
            lib.tmr_no_such_symbol
    assert not [e for e in log if e[0] == "lds_fill"]


def test_only_restricts_the_fill():
    log = []
    m = _fake_module(log)
    with _filled(m, log, only=("tmr_nms",)):
        m.load().tmr_xcorr("a", 1)
        m.load().tmr_nms("b", 2)
    assert [e[0] for e in log] == ["tmr_xcorr", "lds_fill", "tmr_nms"]


def test_handle_is_restored_after_an_exception():
    log = []
    m = _fake_module(log)
    real = m._lib
    with pytest.raises(RuntimeError, match="boom"):
        with _filled(m, log):
            m.load().tmr_boom(1, 2)
    assert m._lib is real and log == [("lds_fill", (ls.PATTERN_FF, 2))]
    with pytest.raises(ls.LdsStateError):  # a failing fill raises before the real call
        with ls.filled(0, only=("tmr_xcorr",), lib_module=m,
                       fill_fn=lambda pat, s: (_ for _ in ()).throw(ls.LdsStateError("fill"))):
            m.load().tmr_xcorr("a", 1)
    assert m._lib is real and log[-1][0] == "lds_fill"


def test_pattern_none_leaves_the_handle_alone():
    m = _fake_module([])
    real = m._lib
    with ls.filled(None, lib_module=m) as proxy:
        assert proxy is None and m.load() is real


def test_missing_helper_names_build(monkeypatch):
    monkeypatch.setattr(ls, "_helper", None)
    monkeypatch.setattr(ls, "HELPER_PATH", os.path.join(os.path.dirname(ls.HELPER_PATH), "no_such_lib.so"))
    with pytest.raises(ls.LdsStateError, match=r"build\(\)"):
        ls.helper()


def test_patterns():
    import numpy as np
    assert ls.PATTERNS == (0x00000000, 0xFFFFFFFF, 0x7B7B7B7B)  # zero first
    ff = np.array([ls.PATTERN_FF], np.uint32)
    assert np.isnan(ff.view(np.float32)).all() and np.isnan(ff.view(np.float16)).all() and ff.view(np.int32)[0] == -1
    assert (ff.view(np.uint16) & 0x7F80 == 0x7F80).all() and (ff.view(np.uint16) & 0x7F != 0).all()  # bf16 NaN
    b7 = np.array([ls.PATTERN_7B], np.uint32)
    assert np.isfinite(b7.view(np.float32)).all() and b7.view(np.float32)[0] > 1e36
    assert np.isfinite(b7.view(np.float16)).all() and (b7.view(np.float16) > 6e4).all()
    assert (b7.view(np.uint16) & 0x7F80 != 0x7F80).all() and (b7.view(np.uint16) >> 7 & 0xFF > 200).all()  # bf16, large


# ------------------------------------------------------------------ the coverage table
def test_stream_entry_points_are_read_from_the_signature_tables():
    tables = ls.signature_tables()
    bound = set()
    for name in dir(_lib):  # every table load() binds
        if name == "SIGNATURES" or name.endswith("_SIGNATURES"):
            bound |= set(getattr(_lib, name))
    assert set(tables) == bound and len(bound) > 40
    names = ls.stream_entry_points()
    assert "tmr_xcorr" in names and "tmr_tokens_tail" in names and "tmr_split_conv_points_chain" in names
    assert not [n for n in names if n.endswith("_plan") or n in ls.PASS_THROUGH]
    for n in set(tables) - set(names):  # what is left launches nothing
        assert n.endswith("_plan") or n in ls.PASS_THROUGH, n
    for n in names:
        assert tables[n][1][-1] is ctypes.c_void_p


def _coverage_problems(cases, no_lds, names):
    """What keeps (cases, no_lds) from covering `names` exactly once, as strings."""
    out = []
    for n in names:
        if (n in cases) + (n in no_lds) != 1:
            out.append(f"{n}: in {(n in cases) + (n in no_lds)} of CASES and NO_LDS (tests/test_gpu_lds_state.py)")
    out += [f"{n}: no stream-taking entry point of tmr_amd/_lib.py" for n in list(cases) + list(no_lds)
            if n not in names]
    out += [f"{n}: no cases" for n, c in cases.items() if not c]
    return out


def _source_of(name):
    """The csrc file that defines the extern "C" entry point."""
    hits = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cpp"))
            and re.search(r'extern "C" \w[\w \*]*\b%s\(' % name, open(os.path.join(CSRC, f)).read())]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def test_every_stream_entry_point_is_covered_exactly_once():
    names = ls.stream_entry_points()
    problems = _coverage_problems(T_lds.CASES, T_lds.NO_LDS, names)
    assert not problems, problems
    # the check itself: an entry point in neither list, and one in both, are reported
    some = names[0]
    less = {k: v for k, v in T_lds.CASES.items() if k != some}
    assert _coverage_problems(less, T_lds.NO_LDS, names) == \
        [f"{some}: in 0 of CASES and NO_LDS (tests/test_gpu_lds_state.py)"]
    assert _coverage_problems(T_lds.CASES, dict(T_lds.NO_LDS, **{some: "x.hip"}), names)


def test_no_lds_entries_name_a_source_without_shared_storage():
    for name, src in T_lds.NO_LDS.items():
        assert _source_of(name) == src, (name, src)
        assert "__shared__" not in open(os.path.join(CSRC, src)).read(), \
            f"{src} declares __shared__ storage: {name} needs cases in tests/test_gpu_lds_state.py"
    # every entry point with cases is defined where the table's reader would look for it
    for name in T_lds.CASES:
        assert _source_of(name).endswith(".hip"), name


def test_case_ids_are_unique_and_runs_start_with_zero():
    ids = [f"{e}-{c}" for e, c in T_lds.ENTRY_CASES]
    assert len(ids) == len(set(ids))
    assert [p for _, p in T_lds.RUNS] == [None, ls.PATTERN_ZERO, ls.PATTERN_FF, ls.PATTERN_7B]
