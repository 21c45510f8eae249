"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/launch_trace.json: the
libtmr.so calls (symbol + normalised arguments) of the flows in
tests/launch_trace.py, recorded on an MI355X.

The flows use only the public engine and module API, so this script runs
unchanged on any commit: the fixture is made from the commit BEFORE a change
that must not move a launch, and tests/test_gpu_launch_trace.py replays the
flows after it.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_launch_trace.py [OUT]
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), REPO):
    sys.path.insert(0, p)
from tmr_import import load_package  # noqa: E402

load_package()
import launch_trace  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "launch_trace.json")


def dumps(traces: dict) -> str:
    """One call per line (a diff of the fixture names the launch that moved)."""
    flows = []
    for name, runs in traces.items():
        body = ",\n".join("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in run) + "\n]" for run in runs)
        flows.append(f"{json.dumps(name)}: [{body}]")
    return "{\n" + ",\n".join(flows) + "\n}\n"


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    traces = {name: launch_trace.run_flow(name) for name in launch_trace.FLOWS}
    text = dumps(traces)
    assert json.loads(text) == json.loads(json.dumps(traces))
    with open(out, "w") as fh:
        fh.write(text)
    print(f"{out}: {len(traces)} flows, {sum(len(r) for t in traces.values() for r in t)} calls, {len(text)} bytes")


if __name__ == "__main__":
    main()
