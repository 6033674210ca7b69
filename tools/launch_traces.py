#!/usr/bin/env python
"""Write the launch traces of the smoothing paths (tests/launch_trace.py: every ops call of a cycle, its flags and the
buffers it reads and writes, on CPU tensors) as JSON: the tool regenerates tests/golden/launch_traces.json from the current
tree.  tests/test_launch_traces_cpu.py compares the traces of the tree against that file, so a change that is meant to alter
a launch sequence (or the name of a stand-in's parameter, which the lines print) commits the regenerated file with it, and
the diff of the file shows what changed.

    python tools/launch_traces.py [out.json]         # default: tests/golden/launch_traces.json
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
