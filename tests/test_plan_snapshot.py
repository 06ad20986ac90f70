"""The general graph planner's plans, pinned on the CPU: `plan_dump` (csrc/plan_dump.cc, built by `make`) prints every
field of the GraphPlan of each golden .onnx model, and the text must equal tests/golden/graph_plans.txt: every launch,
view, buffer, weight offset, elementwise program and a hash of every constant record, or the refusal's whole message.
No device needed.

A pull request that changes plans on purpose regenerates the snapshot, from the repository root, and reviews its diff:

    (cd tests/golden && ../../nshogi-engine_amd/csrc/plan_dump $(python ../test_plan_snapshot.py)) > tests/golden/graph_plans.txt
"""
import difflib
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PLAN_DUMP = os.path.join(ROOT, "nshogi-engine_amd", "csrc", "plan_dump")
PLANES = {"net_graph_gpool93.onnx": 93}  # every other model: 86


def arguments():
    """plan_dump's arguments, relative to tests/golden: every .onnx model by name, each behind its plane count."""
    args = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.onnx"))):
        name = os.path.basename(path)
        args += ["--planes", str(PLANES.get(name, 86)), name]
    return args


def test_the_planner_gives_the_plans_of_the_snapshot():
    if not os.path.exists(PLAN_DUMP):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    args = arguments()
    assert len(args) == 3 * 13, args
    got = subprocess.run([PLAN_DUMP] + args, cwd=GOLDEN, check=True, capture_output=True, text=True).stdout
    with open(os.path.join(GOLDEN, "graph_plans.txt")) as f:
        want = f.read()
    assert got.count("\n== ") + 1 == 13 and "\n#" in got
    if got != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.splitlines(), "tests/golden/graph_plans.txt", "plan_dump", lineterm="", n=1))
        shown = "\n".join(line if len(line) < 600 else line[:600] + " ..." for line in diff[:60])
        raise AssertionError(f"the plans differ from the snapshot ({len(diff)} diff lines; the first 60, long lines cut):\n{shown}")


if __name__ == "__main__":
    print(" ".join(arguments()))
