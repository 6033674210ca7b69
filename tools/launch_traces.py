#!/usr/bin/env python
"""Write the launch traces of the smoothing paths (tests/launch_trace.py: every ops call of a cycle, its flags and the
buffers it reads and writes, on CPU tensors) as JSON.  tests/golden/launch_traces.json is the output of this script on the
commit before smoothing.py and torch_ops.py were split off; tests/test_launch_traces_cpu.py compares against it.

    python tools/launch_traces.py [out.json]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if __name__ == "__main__":
    import launch_trace
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "launch_traces.json")
    with open(out, "w") as f:
        launch_trace.dump(launch_trace.all_traces(), f)
