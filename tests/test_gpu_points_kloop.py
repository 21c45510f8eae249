"""tmr_split_conv_points over a K loop that runs on across chunks: C1 = 160
(five 32-channel chunks, an odd count; the other points tests stop at two).

Shapes: tests/test_gpu_points_pairs.py's (a 17 x 33 map, three images, four
units, unit 3's f_TM scaled by 2^10) with C0 = 64 and C1 = 160.  In the tiled
forms src0's half lives in the acc_init slab and the points loop walks the
five chunks of src1; in the broadcast-plane E = 1 form it walks seven, which
cross from src0 to src1.  Windows nb = 1 (one pass) and nb = 5 (two passes,
the second partial); fp32, bf16 and f16; the bf16 slab of the one-term engines
at nb = 5.  Candidate lists per case: one full tile, one tile of one
candidate, and an odd number of tiles (every pixel of unit 0: 8 tiles + 49).

The expected values are the dense window of tmr_split_conv + tmr_heads_reduce
at the listed pixels, bit for bit, the sentinel in every other element of b;
every case under the guarded allocator's three runs, as in the pairs file.

The helpers are those of tests/test_gpu_points_pairs.py, whose shapes are
module constants: a second instance of that module is loaded here and its C1
set, so that it keeps reference and input caches of its own.
"""
import importlib.util

import numpy as np
import pytest

import test_gpu_points_pairs as _pairs
from test_gpu_points import SENTINEL
from tmr_amd import host
from tmr_amd._lib import POINTS_TILE

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_points_pairs_c160", _pairs.__file__)
K = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K)
K.C1 = 160
assert K.C0 == 64 and (K.H, K.W, K.B, K.U) == (17, 33, 3, 4) and not K._INPUTS and not K._WANT


def _lists():
    T = POINTS_TILE
    every = host.point_tiles(np.array([K.HW, 0, 0, 0]), T)
    assert len(every) % 2 == 1 and every[-1, 2] == K.HW % T
    return {"full": np.array([[0, T, T]], np.int32), "single": np.array([[1, 0, 1]], np.int32), "odd": every}


CASES = [(nb, prec, form) for nb in (1, 5) for prec in ("fp32", "bf16", "f16") for form in ("tiled", "bcast")]
CASES += [(5, "bf16", "tiled16")]


@pytest.mark.parametrize("nb,prec,form", CASES)
def test_five_chunk_loop_equals_dense_bits(nb, prec, form):
    assert K._inputs(nb)["x1"].shape[1] == 160 and K._inputs(nb)["w"].shape[1] == 64 + 160
    lists = _lists()
    out = K._run(f"kloop{nb}-{prec}-{form}", nb, prec, form, lists)
    # (K._run compared every list with the dense bits and the sentinel; the counts once more)
    assert int((out["full"] != SENTINEL).sum()) == 4 * POINTS_TILE
    assert int((out["single"] != SENTINEL).sum()) == 4
    assert int((out["odd"][0] != SENTINEL).sum()) == 4 * K.HW and (out["odd"][1:] == SENTINEL).all()
