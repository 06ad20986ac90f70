#!/usr/bin/env python3
"""Instruction counts, by class, of the staged epilogue of a conv kernel inside a hipcc object file:
scripts/epilogue_isa.py <file.o> <substring of the mangled kernel name> [--dump]

The epilogue of a tileBody is the MFMA-free run of instructions that reads the accumulators back
(v_accvgpr_read) and ends at the last global store behind them; a persistent trunk kernel holds two (the residual
and the non-residual body; the residual one is the one that decodes fp6 blocks / has more loads than stores).
Counts are printed for the whole run and per fragment (fragments = 16-row MFMA result tiles)."""
import os, re, subprocess, sys, tempfile
from collections import Counter, OrderedDict

LLVM = "/opt/rocm/lib/llvm/bin/"

CLASSES = OrderedDict([
    ("v_accvgpr_read", r"v_accvgpr_read"),
    ("v_accvgpr_write", r"v_accvgpr_write"),
    ("v_mov / copies", r"v_mov_|v_accvgpr_mov|v_swap|v_pk_mov"),
    ("s_nop", r"s_nop"),
    ("conversions (v_cvt_*)", r"v_cvt_"),
    ("v_fma_mix", r"v_fma_mix"),
    ("fma / pk_fma (bias, scale)", r"v_fma_f32|v_fmac_f32|v_pk_fma_f32|v_pk_mul_f32|v_mul_f32"),
    ("adds (v_pk_add_f32 / v_add_f32)", r"v_pk_add_f32|v_add_f32"),
    ("med3 / max3 / max", r"v_med3|v_max3|v_max_f|v_pk_max"),
    ("permlane", r"v_permlane"),
    ("selects (v_cndmask)", r"v_cndmask"),
    ("ds_*", r"ds_"),
    ("VMEM (flat_ / global_ / buffer_)", r"global_|buffer_|flat_|scratch_"),
    ("s_waitcnt", r"s_waitcnt"),
    ("address / mask VALU", r"v_"),  # every other vector instruction: integer adds, shifts, compares, ...
    ("scalar / branches", r"s_"),
])


def disassemble(obj, pat):
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fb.bin"), os.path.join(d, "k.co")
        subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj])
        subprocess.check_call([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb, "--output=" + co,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        syms = subprocess.run([LLVM + "llvm-readelf", "-sW", co], capture_output=True, text=True, check=True).stdout
        names = sorted({m.group(1) for m in re.finditer(r"FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", syms, re.M) if pat in m.group(1)})
        if len(names) != 1:
            sys.exit("kernel name must match exactly one symbol, got: %s" % names)
        txt = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--disassemble-symbols=" + names[0], co],
                             capture_output=True, text=True, check=True).stdout
    ins = []
    for line in txt.splitlines():
        m = re.match(r"^\s+([a-z_0-9]+)(\s.*)?$", line)
        if m and not line.lstrip().startswith("//"):
            ins.append((m.group(1), line.strip()))
    return names[0], ins


def classify(op):
    for name, rx in CLASSES.items():
        if re.match(rx, op):
            return name
    return "other"


def epilogues(ins):
    """(first, last) instruction index of every MFMA-free run that reads at least 16 accumulators back."""
    out, start = [], 0
    bounds = [i for i, (op, _) in enumerate(ins) if op.startswith("v_mfma")] + [len(ins)]
    for b in bounds:
        seg = range(start, b)
        reads = [i for i in seg if ins[i][0].startswith("v_accvgpr_read")]
        stores = [i for i in seg if re.match(r"(global|buffer|flat)_store", ins[i][0])]
        if len(reads) >= 16 and stores:
            out.append((start, max(stores)))
        start = b + 1
    return out


def main():
    obj, pat = sys.argv[1], sys.argv[2]
    name, ins = disassemble(obj, pat)
    print("kernel %s: %d instructions" % (name[:110], len(ins)))
    for k, (a, b) in enumerate(epilogues(ins)):
        seg = ins[a:b + 1]
        cnt = Counter(classify(op) for op, _ in seg)
        # (an MX encoder runs one 32-wide conversion per fragment; the read count also holds reads that are not the epilogue's)
        frags = float(sum(1 for op, _ in seg if op.startswith("v_cvt_scalef32_pk32_fp6_f16")) or cnt["v_accvgpr_read"] / 16.0)
        loads = sum(1 for op, _ in seg if re.match(r"(global|buffer|flat)_load", op))
        residual = any(op.startswith("v_cvt_scalef32_pk32_f16_fp6") for op, _ in seg) or loads >= frags * 4
        print("\nepilogue %d (%s residual): %d instructions, %g fragments, %.1f per fragment"
              % (k, "with" if residual else "without", len(seg), frags, len(seg) / frags))
        print("  %-34s %8s %12s" % ("class", "total", "per fragment"))
        for c in list(CLASSES) + ["other"]:
            if cnt[c]:
                print("  %-34s %8d %12.1f" % (c, cnt[c], cnt[c] / frags))
        valu = sum(n for c, n in cnt.items() if c not in ("ds_*", "VMEM (flat_ / global_ / buffer_)", "s_waitcnt", "s_nop", "scalar / branches", "other"))
        print("  %-34s %8d %12.1f" % ("(all vector ALU, reads included)", valu, valu / frags))
        if "--dump" in sys.argv:
            for _, line in seg:
                print("    " + line)


if __name__ == "__main__":
    main()
