"""The specialised path's launch forms, pinned on the CPU: `form_dump` (csrc/form_dump.cc, built by `make`) prints what
chooseLaunchForm (csrc/launch_form.cc) decides for every batch size from 1 to 4 CUs + 64 of each configuration of a fixed
grid, runs of equal forms on one line, and the text must equal tests/golden/launch_forms.txt.  That file is the table of
which batch takes which form: team trunk, cooperative trunk, whole-trunk launch, two-part batch, half-batch chains or
one per-layer chain, with the tile plan, the members, the parts and the trunk's arithmetic.  No device needed.

The grid: 256, 64 and 32 CUs x every precision x (F, cpad) in (128,128) (192,128) (192,192) (256,128) (256,256) (384,128)
x teamAvailable x coopAvailable x outsideM8Window, and every knob of LaunchConfig and ConvTuning one at a time at the
values its tests and the evaluator's environment check admit.  To keep the file small enough to read and review, 128 CUs
and the knob variants at 32 CUs are left out, a section prints its first table in full and of every other variant only
the batch sizes whose form differs from it, and text that an earlier section printed is named instead of repeated;
form_dump.cc's header explains a line.

A pull request that changes a decision on purpose regenerates the table, from the repository root, and reviews its diff:

    nshogi-engine_amd/csrc/form_dump > tests/golden/launch_forms.txt
"""
import difflib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_forms.txt")
FORM_DUMP = os.path.join(ROOT, "nshogi-engine_amd", "csrc", "form_dump")


def test_every_batch_takes_the_launch_form_of_the_table():
    if not os.path.exists(FORM_DUMP):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    got = subprocess.run([FORM_DUMP], check=True, capture_output=True, text=True).stdout
    with open(GOLDEN) as f:
        want = f.read()
    assert got.count("\n== ") + 1 == 3 * 6 * 6 and os.path.getsize(GOLDEN) < (1 << 20) and "\n-- " in got
    if got != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.splitlines(), "tests/golden/launch_forms.txt", "form_dump", lineterm="", n=1))
        shown = "\n".join(diff[:60])
        raise AssertionError(f"the launch forms differ from the table ({len(diff)} diff lines; the first 60):\n{shown}")
