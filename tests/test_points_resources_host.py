"""The committed register figures of split_points_kernel
(profiles/points_kloop/resources.json, written by profiles/kernel_resources.py
from the compiler's resource-usage remarks) belong to this tree's sources and
show no spill: every instantiation keeps its K loop, prologue and epilogues in
registers (two waves per SIMD, 256 registers).  No compile here: a kernel edit
without re-running the tool turns the digest check red."""
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("F16X3", "BF16", "F16")


@pytest.fixture(scope="module")
def rec():
    return json.load(open(os.path.join(REPO, "profiles", "points_kloop", "resources.json")))


def test_resources_belong_to_this_tree(rec):
    from tmr_amd import buildinfo
    assert rec["source_digest"] == buildinfo.source_digest("heads"), "re-run profiles/kernel_resources.py"
    assert sorted(rec["kernels"]) == sorted(PRECS) == sorted(rec["parent"])


@pytest.mark.parametrize("prec", PRECS)
def test_no_spill_no_scratch(rec, prec):
    k, parent = rec["kernels"][prec], rec["parent"][prec]
    assert k["vgpr_spills"] == 0 and k["scratch_bytes_per_lane"] == 0, k
    assert k["vgprs"] + k.get("agprs", 0) <= 256 and k["occupancy"] == 2, k
    assert parent["vgpr_spills"] > 0 and parent["scratch_bytes_per_lane"] > 0
