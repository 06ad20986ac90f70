"""The host-only weight preparation, pinned on the CPU: `weights_dump` (csrc/weights_dump.cc, built by `make`) runs
prepareNet (csrc/net_prepare.cc) -- the NSGW parser, BN folding in double, the power-of-two weight scale, the re-layout
into MFMA fragment order, the activation-bound estimate -- on nets it generates from an integer LCG, in every precision,
and prints the dims, the bound, and per layer the image size, accScale and a 64-bit FNV-1a digest of the packed image
and of the bias; then the buffer sequence of the 3x3 layers for 0 to 3 blocks, and the code and message of every blob
the loader refuses.  The text must equal tests/golden/net_prepare.txt: a change to a record order, a slab layout, a
converter or the fold shows up here as a diff of the layers it touches.  No device needed.

The nets: 45 input planes (padded at every granule), F = 64 and 128 (the kF16m6 slab groups fragments by four, so 128
has a second group), 0 to 2 blocks, pc = 27, vc = 3, vh = 64, and one net whose BN gains put the bound past the kF16m8
window.  weights_dump.cc's header explains a line.

A pull request that changes the packed bytes on purpose regenerates the table, from the repository root, and reviews
its diff:

    nshogi-engine_amd/csrc/weights_dump > tests/golden/net_prepare.txt
"""
import difflib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "net_prepare.txt")
WEIGHTS_DUMP = os.path.join(ROOT, "nshogi-engine_amd", "csrc", "weights_dump")


def test_prepared_nets_equal_the_table():
    if not os.path.exists(WEIGHTS_DUMP):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    got = subprocess.run([WEIGHTS_DUMP], check=True, capture_output=True, text=True).stdout
    with open(GOLDEN) as f:
        want = f.read()
    # 7 nets x 6 precisions, both sides of the kF16m8 window, the sequences, the refusals
    assert got.count("== net ") == 42 and got.count("== sequence ") == 4 and got.count("\n", got.index("== refusals")) == 10
    assert "outsideM8Window=1" in got and "prec=f16m8\n" in got and "error" not in got
    if got != want:
        diff = list(difflib.unified_diff(want.splitlines(), got.splitlines(), "tests/golden/net_prepare.txt", "weights_dump", lineterm="", n=1))
        shown = "\n".join(diff[:60])
        raise AssertionError(f"the prepared nets differ from the table ({len(diff)} diff lines; the first 60):\n{shown}")
