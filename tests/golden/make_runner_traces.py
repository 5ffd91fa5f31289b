#!/usr/bin/env python3
"""Record tests/golden/runner_traces.json: what vnect_amd/runner.py's device tracking loops call on a scripted handle, yield and raise in
every scenario of tests/runner_trace.golden_scenarios().

Run it on the commit whose loops are the standard (the file in the repository was recorded at the parent of the commit that built the
loops from one in-flight window), never to make a failing tests/test_runner_trace_cpu.py pass.  Needs neither the library nor a GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from tests import runner_trace  # noqa: E402
from vnect_amd import runner  # noqa: E402


def main():
    traces = {name: f(runner) for name, f in runner_trace.golden_scenarios().items()}
    path = os.path.join(HERE, "runner_traces.json")
    with open(path, "w") as fh:
        json.dump(traces, fh, indent=0, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
    print("%s: %d scenarios, %d calls, %d bytes" % (path, len(traces), sum(len(t["calls"]) for t in traces.values()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
