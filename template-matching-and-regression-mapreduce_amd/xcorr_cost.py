"""Which correlation kernel a launch runs (tmr_xcorr_args_t.algo "auto").

The cost table is the committed rocprofv3 sweep xcorr_cost.json
(profiles/gpu_xcorr_sweep.sh -> profiles/xcorr_sweep_assemble.py; DESIGN.md
4.3): kernel-trace durations of both kernels per template size k, re-swept
whenever xcorr.hip changes (the file records the source digest and
tests/test_abi_host.py fails on a stale one).  Costs are ms per unit at the
512 x 128^2 map size in two regimes: E = 3 (64 images x 3 exemplars at 128^2)
and E = 16 (8 x 16 at 192^2, times / 2.25 for the area).  "auto" interpolates
the regimes in log E, sums the per-unit costs of a launch (linear in k in
between) and runs the cheaper kernel: fp32 MFMA from k = 7 in both regimes;
one bf16 term from k = 5 at E = 3 and at every k at E = 16.
"""
from __future__ import annotations

import json
import os

import numpy as np

from ._lib import TMRError

XCORR_COST_K = (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31)
_COST_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xcorr_cost.json")


def _load_xcorr_cost(path: str = _COST_JSON):
    """(table, source) of the swept per-k cost table.  A file that is missing
    or does not parse raises: a silently moved crossover would change which
    kernel runs."""
    try:
        with open(path) as fh:
            d = json.load(fh)
    except (OSError, ValueError) as err:
        raise TMRError(f"{path}: missing or malformed correlation cost table ({err})") from err
    reg = d.get("regimes", {})

    def per_unit(name, algo, area):
        r = reg[name]
        ks, ms = zip(*sorted((int(k), float(v)) for k, v in r["ms"][algo] if v is not None))
        return np.interp(XCORR_COST_K, ks, np.asarray(ms) / (r["images"] * r["E"]) / area)

    try:
        table = {
            "valu": (per_unit("r128_e3_fp32", "valu", 1.0), per_unit("r192_e16_fp32", "valu", 2.25)),
            "mfma": (per_unit("r128_e3_fp32", "mfma", 1.0), per_unit("r192_e16_fp32", "mfma", 2.25)),
            "mfma1": (per_unit("r128_e3_bf16", "mfma", 1.0), per_unit("r192_e16_bf16", "mfma", 2.25)),
        }
    except (KeyError, ValueError, TypeError) as err:
        raise TMRError(f"{path}: correlation cost table lacks a regime or algorithm ({err!r})") from err
    return table, d.get("source", path)


XCORR_COST, XCORR_COST_SOURCE = _load_xcorr_cost()
# A mixed-size MFMA launch stages every band with the LARGEST template's halo
# rows (and that template's band height), and its band staging is shared by
# fewer units when an image has few of them: 1.04x the per-k sum at the
# config-B 3..15 mix (3.764 ms mix vs 3.619 ms per-k mean, one run on one
# box).  Empirical: 1 + MIX / units-per-image.
XCORR_MFMA_MIX = 0.12


def mfma_fits(W: int, max_ht: int, max_wt: int) -> bool:
    """xcorr.hip mfma_fits: a 32-row band, its halo and WIN_OVER = 3 rows
    staged in registers."""
    return W % 64 == 0 and W <= 256 and max_ht <= 31 and max_wt <= 31 and (35 + max_ht // 2 * 2) * W <= 16384


def xcorr_choice(ht: np.ndarray, wt: np.ndarray, units_per_image: float, mfma_ok: bool,
                 one_term: bool = False) -> str:
    """The cheaper correlation kernel ("valu" or "mfma") for a launch over
    units of these template sizes (XCORR_COST model); one_term: the MFMA
    kernel runs one 16-bit term (bf16 contract) instead of the 3-term split."""
    if not mfma_ok:
        return "valu"
    k = np.maximum(np.asarray(ht), np.asarray(wt)).astype(np.float64)
    lam = float(np.clip(np.log(max(units_per_image, 1.0) / 3.0) / np.log(16.0 / 3.0), 0.0, 1.0))
    cost = {}
    for alg, table in (("valu", "valu"), ("mfma", "mfma1" if one_term else "mfma")):
        c3, c16 = XCORR_COST[table]
        per_k = (1.0 - lam) * c3 + lam * c16
        cost[alg] = float(np.interp(k, XCORR_COST_K, per_k).sum())
    if k.size and k.min() != k.max():
        cost["mfma"] *= 1.0 + XCORR_MFMA_MIX / max(units_per_image, 1.0)
    return min(cost, key=cost.get)
