#!/usr/bin/env python
"""Static instruction budget of one kernel instantiation, from the assembly hipcc writes for gfx950 (no GPU involved).

    python tools/isa_budget.py [SOURCE] --kernel "256, 192, 160" [--asm FILE] [--blocks] [--path FILE] [--loop LABEL]

SOURCE (default torchani_amd/csrc/mlp_fused.hip) is compiled to assembly, device side only, with the flags the library is
built with (torchani_amd/_lib.py: HIPCC_FLAGS); --asm reads an assembly file made earlier instead.  The kernel is picked by
a substring of its demangled name (the last match of --kernel; every kernel of the file is listed with its register and
spill figures).  The instantiation is split into basic blocks (a label, or the instruction behind a branch, starts one) and
the instructions of every block are counted by class:

    mfma    v_mfma* / v_smfmac*            lds     ds_*                    bar    s_barrier
    lane_r  v_readlane of a spill register  vmem    global_* buffer_* flat_* scratch_*
    lane_w  v_writelane                     salu    every other s_* but s_nop / s_waitcnt (nop, wait: own columns)
    add64   v_lshl_add_u64, v_add_co*, v_addc_co*, v_add_co_ci*            mov    v_mov_b32 / v_mov_b64 / v_accvgpr_*
    cnd     v_cndmask_b32                   valu    every other v_* (the arithmetic, the address arithmetic, ...)

A v_readlane counts as lane_r when its source register is one the kernel also writes with v_writelane (the home of spilled
scalars); the lane reads of a wave reduction count as valu.  `vector` = everything that issues on the vector ALU and is no
MFMA: valu + mov + cnd + add64 + lane_r + lane_w.

--path FILE weighs the blocks: lines `LABEL COUNT` (anything behind a # is a comment; a block without a label is named by
the label ahead of it and a running number, as --blocks prints it); the weighted sums are the instructions one wave executes
on that path.  --loop LABEL reports the lane traffic of the blocks from LABEL to the end of the kernel (the item loop of
k_mlp_fused starts at the block that holds its first `;;#ASMSTART` of the opaque copy of threadIdx.x).

It classifies by mnemonic; it checks nothing.
"""
from __future__ import annotations

import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["mfma", "valu", "mov", "cnd", "add64", "lane_r", "lane_w", "lds", "vmem", "salu", "nop", "wait", "bar"]
VECTOR = ["valu", "mov", "cnd", "add64", "lane_r", "lane_w"]
ADD64 = ("v_lshl_add_u64", "v_add_co_u32", "v_addc_co_u32", "v_add_co_ci_u32", "v_sub_co_u32", "v_subb_co_u32")
BRANCH = ("s_branch", "s_cbranch", "s_endpgm", "s_setpc", "s_swappc")


def compile_asm(source: str) -> str:
    sys.path.insert(0, ROOT)
    from torchani_amd._lib import HIPCC_FLAGS

    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = os.path.join(tempfile.mkdtemp(prefix="isa_budget_"), os.path.basename(source) + ".s")
    subprocess.check_call(["hipcc"] + flags + ["--cuda-device-only", "-S", "-o", out, source])
    return out


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def metadata(text: str):
    """name -> {field: value} from the .amdhsa metadata and the compiler's comments behind each kernel"""
    meta = collections.OrderedDict()
    cur = None   # the entry of amdhsa.kernels being read: its items start with `  - .` and its fields are indented by four
    for line in text.splitlines():
        if line.startswith("  - ."):
            cur = {}
            line = "    " + line[4:]
        elif not line.startswith("    "):
            cur = None
        if cur is None:
            continue
        m = re.match(r"    \.name:\s+(\S+)", line)
        if m:
            cur = meta.setdefault(m.group(1), cur)
        m = re.match(r"    \.(sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count|private_segment_fixed_size|agpr_count):\s+(\d+)", line)
        if m:
            cur[m.group(1)] = int(m.group(2))
    name = None
    for line in text.splitlines():
        m = re.match(r"(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            name = m.group(1)
        m = re.match(r"; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", line)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return meta


def classify(mn: str, ops: str, spill_regs) -> str:
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if mn.startswith("v_writelane"):
        return "lane_w"
    if mn.startswith("v_readlane"):
        src = ops.split(",")[1].strip() if "," in ops else ""
        return "lane_r" if src in spill_regs else "valu"
    if mn.startswith(ADD64):
        return "add64"
    if mn.startswith(("v_mov_b", "v_accvgpr")):
        return "mov"
    if mn.startswith("v_cndmask"):
        return "cnd"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn == "s_barrier":
        return "bar"
    if mn == "s_nop":
        return "nop"
    if mn.startswith("s_waitcnt"):
        return "wait"
    if mn.startswith("s_"):
        return "salu"
    return ""


def blocks_of(text: str, kernel: str):
    """[(block name, Counter, [mnemonics])] of the kernel's body"""
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start + 1:end]
    spill_regs = set()
    for l in body:
        m = re.match(r"\s+v_writelane_b32\s+(v\d+)", l)
        if m:
            spill_regs.add(m.group(1))
    out = []
    label, sub, cur, mns = "entry", 0, collections.Counter(), []

    def close():
        nonlocal cur, mns, sub
        if mns or cur:
            out.append((label if sub == 0 else f"{label}+{sub}", cur, mns))
            sub += 1
        cur, mns = collections.Counter(), []

    for l in body:
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            close()
            label, sub = m.group(1), 0
            continue
        m = re.match(r"\s+([a-z_0-9]+)\s*([^;]*)", l)
        if not m or l.lstrip().startswith((";", ".")):
            if "ASMSTART" in l:
                cur["asm"] += 1
            continue
        mn, ops = m.group(1), m.group(2)
        c = classify(mn, ops, spill_regs)
        if not c:
            continue
        cur[c] += 1
        mns.append(mn)
        if mn.startswith(BRANCH):
            close()
    close()
    return out, spill_regs


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source", nargs="?", default=os.path.join(ROOT, "torchani_amd", "csrc", "mlp_fused.hip"))
    ap.add_argument("--kernel", default=None, help="substring of the demangled name of the instantiation to split into blocks")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling SOURCE")
    ap.add_argument("--blocks", action="store_true", help="print the table of all basic blocks")
    ap.add_argument("--path", default=None, help="file of `LABEL COUNT` lines: the blocks one wave executes and how often")
    ap.add_argument("--loop", default=None, help="label of the first block of the item loop")
    a = ap.parse_args()

    text = open(a.asm or compile_asm(a.source)).read()
    meta = metadata(text)
    names = demangle(list(meta))
    print("kernel | NumVgprs | NumAgprs | TotalNumSgprs | sgpr_spill | vgpr_spill | ScratchSize | Occupancy")
    for k, v in meta.items():
        if "NumVgprs" not in v:
            continue
        short = re.sub(r"\(.*\)$", "", names[k]).replace("void anihip::", "")
        print(f"{short} | {v.get('NumVgprs')} | {v.get('NumAgprs')} | {v.get('TotalNumSgprs')} | {v.get('sgpr_spill_count')} | "
              f"{v.get('vgpr_spill_count')} | {v.get('ScratchSize')} | {v.get('Occupancy')}")
    if not a.kernel:
        return 0
    match = [k for k in meta if a.kernel in names[k] or a.kernel in k]
    if not match:
        print(f"no kernel matches {a.kernel!r}", file=sys.stderr)
        return 1
    kernel = match[-1]
    blocks, spill_regs = blocks_of(text, kernel)
    print(f"\n{names[kernel]}\n{len(blocks)} basic blocks; scalar spill registers: {sorted(spill_regs) or 'none'}")
    hdr = f"{'block':>16} " + " ".join(f"{c:>6}" for c in CLASSES) + f" {'vector':>7}"

    def row(name, c, w=None):
        vec = sum(c[x] for x in VECTOR)
        pre = f"{name:>16} " if w is None else f"{name:>16} x{w:<3}"
        return pre + " ".join(f"{c[x]:>6}" for x in CLASSES) + f" {vec:>7}"

    total = collections.Counter()
    for _, c, _ in blocks:
        total.update(c)
    if a.blocks:
        print(hdr)
        for name, c, _ in blocks:
            print(row(name, c))
    print(hdr)
    print(row("static total", total))
    if a.loop:
        idx = next(i for i, (n, _, _) in enumerate(blocks) if n == a.loop)
        inside = collections.Counter()
        for _, c, _ in blocks[idx:]:
            inside.update(c)
        print(row(f"from {a.loop}", inside))
        print(f"item loop (static): {inside['lane_r']} spill lane reads, {inside['lane_w']} lane writes, {inside['nop']} s_nop, "
              f"{inside['add64']} 64-bit add idioms")
    if a.path:
        by_name = {n: c for n, c, _ in blocks}
        dyn = collections.Counter()
        print(f"\npath {a.path}")
        print(f"{'block':>16}     " + " ".join(f"{c:>6}" for c in CLASSES) + f" {'vector':>7}")
        for line in open(a.path):
            line = line.split("#")[0].split()
            if not line:
                continue
            name, w = line[0], int(line[1])
            if name not in by_name:
                print(f"path names an unknown block {name}", file=sys.stderr)
                return 1
            print(row(name, by_name[name], w))
            for k2, v in by_name[name].items():
                dyn[k2] += w * v
        print(row("path total", dyn) + "   (per wave)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
