"""Host side of the regression-at-the-peaks route (no GPU): the tile-list
builder, the flags' tile-window packing and the ctypes table of the new entry
point against the header."""
import re

import numpy as np

import tmr_amd
from tmr_amd import _lib, host


def test_point_tiles_counts_and_skipped_units():
    T = _lib.POINTS_TILE
    counts = np.array([0, 1, T, T + 1])
    tiles = host.point_tiles(counts, T)
    assert tiles.dtype == np.int32 and tiles.shape == (4, 3)
    assert tiles.tolist() == [[1, 0, 1], [2, 0, T], [3, 0, T], [3, T, 1]]
    # a unit without regression (mode 2) is zeroed by the caller and gets no tile
    params = np.zeros(4, _lib.PEAK_DTYPE)
    params["mode"] = [0, 2, 0, 1]
    need = np.where(params["mode"] != 2, np.array([5, 70, 0, 2 * T]), 0)
    tiles = host.point_tiles(need, T)
    assert tiles.tolist() == [[0, 0, 5], [3, 0, T], [3, T, T]]
    assert host.point_tiles(np.zeros(3, np.int64), T).shape == (0, 3)
    # every candidate exactly once, no tile across units, none above T
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 5 * T, 50)
    tiles = host.point_tiles(counts, T)
    assert (tiles[:, 2] >= 1).all() and (tiles[:, 2] <= T).all()
    for u, c in enumerate(counts):
        mine = tiles[tiles[:, 0] == u]
        assert mine[:, 2].sum() == c
        assert np.array_equal(mine[:, 1], np.arange(len(mine)) * T)


def test_tile_window_flag_bits_round_trip():
    for first, count in ((0, 0), (0, 8), (8, 8), (255, 127), (3, 1)):
        fl = _lib.split_tile_window(first, count)
        assert _lib.split_tile_window_of(fl) == (first, count)
        assert fl & 0xffff == 0 and fl < 2 ** 31  # the flag byte and the units-per-image byte stay free
        E = 16
        word = fl | (E << _lib.SPLIT_UNITS_PER_IMAGE_SHIFT) | _lib.SPLIT_TILED_INIT | _lib.SPLIT_XMAX_PER_UNIT
        assert (word >> _lib.SPLIT_UNITS_PER_IMAGE_SHIFT) & 0xff == E
        assert word & 0xff == _lib.SPLIT_TILED_INIT | _lib.SPLIT_XMAX_PER_UNIT
        assert _lib.split_tile_window_of(word) == (first, count)
    for bad in ((-1, 0), (256, 1), (0, 128)):
        try:
            _lib.split_tile_window(*bad)
        except tmr_amd.TMRError:
            continue
        raise AssertionError(bad)


def _header_defines():
    text = open(_lib.HEADER).read()
    return text, {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(TMR_\w+)\s+(\d+)\s", text)}


def test_ctypes_table_matches_header():
    text, defs = _header_defines()
    assert defs["TMR_SPLIT_TILE_FIRST_SHIFT"] == _lib.SPLIT_TILE_FIRST_SHIFT
    assert defs["TMR_SPLIT_TILE_COUNT_SHIFT"] == _lib.SPLIT_TILE_COUNT_SHIFT
    assert defs["TMR_SPLIT_UNITS_PER_IMAGE_SHIFT"] + 8 <= defs["TMR_SPLIT_TILE_FIRST_SHIFT"]
    assert defs["TMR_PEAKS_FIND_ONLY"] == _lib.PEAKS_FIND_ONLY
    assert defs["TMR_PEAKS_DECODE_ONLY"] == _lib.PEAKS_DECODE_ONLY
    assert defs["TMR_POINTS_TILE"] == _lib.POINTS_TILE
    m = re.search(r"int tmr_split_conv_points\((.*?)\);", text, re.S)
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES["tmr_split_conv_points"]
    assert res is _lib._I and len(args) == len(params)
    for p, a in zip(params, args):
        assert a is (_lib._P if "*" in p else _lib._I), p
    # the dense launch's operand list is the points launch's, in the same order
    dense = re.search(r"int tmr_split_conv\((.*?)\);", text, re.S).group(1).replace("\n", " ").split(",")
    names = lambda ps: [p.strip().split()[-1].lstrip("*") for p in ps]  # noqa: E731
    assert names(params)[:17] == names(dense)[:17]
    assert tmr_amd._lib.ABI_VERSION == 3
