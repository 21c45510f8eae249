"""Register figures of split_points_kernel from the compiler's own remarks.

Compiles csrc/conv_split.hip for the device only, with the flags csrc/Makefile
builds it with plus -Rpass-analysis=kernel-resource-usage (about a minute, no
GPU), and writes profiles/points_kloop/resources.json: per instantiation the
VGPRs, VGPR spills, scratch bytes per lane and occupancy, beside the values of
the tree before the K loop was fitted into its registers, and the `heads`
source digest of what was compiled (tests/test_points_resources_host.py holds
the committed file to this tree's digest).  It reads the remarks only.

    python profiles/kernel_resources.py [OUT.json]
    python profiles/kernel_resources.py --kernel split_points_chain_kernel [OUT.json]

--kernel split_points_chain_kernel: the same figures of
split_points_chain_kernel<3> (tmr_split_conv_points_chain, F16X3 only) into
profiles/points_kloop/resources_chain.json.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tmr_import import load_package  # noqa: E402

CSRC = os.path.join(REPO, "template-matching-and-regression-mapreduce_amd", "csrc")
OUT = os.path.join(REPO, "profiles", "points_kloop", "resources.json")
PRECS = {0: "F16X3", 1: "BF16", 2: "F16"}  # TMR_PREC_* of split_points_kernel<3, PREC>
# the same compile of the parent tree (commit 85ce6ab)
PARENT = {
    "F16X3": {"vgprs": 256, "vgpr_spills": 146, "scratch_bytes_per_lane": 252, "occupancy": 2},
    "BF16": {"vgprs": 256, "vgpr_spills": 10, "scratch_bytes_per_lane": 44, "occupancy": 2},
    "F16": {"vgprs": 256, "vgpr_spills": 110, "scratch_bytes_per_lane": 204, "occupancy": 2},
}
FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "VGPRs Spill": "vgpr_spills", "SGPRs Spill": "sgpr_spills",
          "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy"}


def makefile_flags():
    """HIPCC and FLAGS of csrc/Makefile, its variables expanded (EXTRA empty)."""
    var = {"EXTRA": ""}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"^(\w+)\s*\??=\s*(.*)$", line.rstrip("\n"))
        if m and m.group(1) not in var:
            var[m.group(1)] = m.group(2)
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: expand(var.get(m.group(1), "")), s)  # noqa: E731
    return os.environ.get("HIPCC", expand(var["HIPCC"])), expand(var["FLAGS"]).split()


def remarks(hipcc, flags):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(CSRC, "conv_split.hip"), "-o", os.path.join(tmp, "conv_split.o")]
        return subprocess.run(cmd, check=True, capture_output=True, text=True).stderr


CHAIN = "split_points_chain_kernel"
OUT_CHAIN = os.path.join(REPO, "profiles", "points_kloop", "resources_chain.json")


def parse(text, kernel="split_points_kernel"):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: +([^:]+): (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            if kernel == CHAIN:
                cur = out.setdefault("F16X3", {}) if re.search(CHAIN + r"ILi3EE", val) else None
            else:
                k = re.search(r"split_points_kernelILi3ELi(\d)EE", val)
                cur = out.setdefault(PRECS[int(k.group(1))], {}) if k else None
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    return out


def main():
    argv = sys.argv[1:]
    chain = argv[:2] == ["--kernel", CHAIN]
    if chain:
        argv = argv[2:]
    out_path = argv[0] if argv else OUT_CHAIN if chain else OUT
    hipcc, flags = makefile_flags()
    kernels = parse(remarks(hipcc, flags), CHAIN if chain else "split_points_kernel")
    assert sorted(kernels) == (["F16X3"] if chain else sorted(PRECS.values())), kernels
    load_package()
    from tmr_amd import buildinfo
    rec = {"kernel": "split_points_chain_kernel<3>" if chain else "split_points_kernel<3, PREC>", "flags": flags,
           "source_digest": buildinfo.source_digest("heads"), "kernels": kernels}
    if not chain:
        rec["parent"] = PARENT
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for p, k in kernels.items():
        print(p, json.dumps(k))


if __name__ == "__main__":
    main()
