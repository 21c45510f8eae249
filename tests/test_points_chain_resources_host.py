"""The committed register figures of split_points_chain_kernel
(profiles/points_kloop/resources_chain.json, written by
`profiles/kernel_resources.py --kernel split_points_chain_kernel` from the
compiler's resource-usage remarks) belong to this tree's sources and show no
spill: both K loops, the phase switch between them, the prologue and the
epilogues stay in registers at two waves per SIMD.  No compile here: a kernel
edit without re-running the tool turns the digest check red."""
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rec():
    return json.load(open(os.path.join(REPO, "profiles", "points_kloop", "resources_chain.json")))


def test_resources_belong_to_this_tree(rec):
    from tmr_amd import buildinfo
    assert rec["source_digest"] == buildinfo.source_digest("heads"), \
        "re-run profiles/kernel_resources.py --kernel split_points_chain_kernel"
    assert rec["kernel"] == "split_points_chain_kernel<3>" and list(rec["kernels"]) == ["F16X3"]


def test_no_spill_no_scratch_two_waves(rec):
    k = rec["kernels"]["F16X3"]
    assert k["vgpr_spills"] == 0 and k["scratch_bytes_per_lane"] == 0, k
    assert k["vgprs"] + k.get("agprs", 0) <= 256 and k["occupancy"] == 2, k
