#!/usr/bin/env python3
"""isa_counts.py -- instruction counts per basic block of the overlap-save kernels, from a device-only cross-compile (no GPU).

    python tools/isa_counts.py [--tree DIR] [--kernel REGEX] [--min N] [--all]
    python tools/isa_counts.py --file fir_bank --same-as DIR

compiles DIR/llzlab_amd/csrc/kernels/fir_ols.hip (DIR: this tree by default; a checkout of another commit for a comparison) with
the Makefile's flags to assembly, and prints for every kernel whose name matches REGEX (default: the 1024-point kernels)
  * VGPRs, scratch bytes, static LDS bytes and code bytes from the kernel's metadata and its .size, and
  * its basic blocks of at least N instructions (default 40), counted by class only: vector ALU, LDS, global load, global
    store, waits, scalar/other, and -- of the vector ALU -- the v_mov copies.
A block is named for what it holds: `transform` has a kernel's most vector ALU instructions (and every block within 5 % of it:
the full and the short job), `request` 48 or 32 global loads, `store` 48 or 32 global stores; `back-edge` is the block that
ends a loop on a conditional branch backwards and holds none of the above.  --all prints every block.  The dynamic LDS size is
the launcher's (OLS_RUNGS), not the compiler's, and is not shown.
--same-as DIR compiles the same file of another tree too and says, for every kernel whose name does NOT match REGEX, whether its
instructions are the same in both (labels renumbered, comments dropped)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-fPIC", "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wno-unused-function"]     # csrc/Makefile HIPFLAGS


def classify(op):
    if op.startswith("s_waitcnt") or op.startswith("s_wait_"):
        return "wait"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_load", "flat_load", "buffer_load", "scratch_load")):
        return "gload"
    if op.startswith(("global_store", "flat_store", "buffer_store", "scratch_store")):
        return "gstore"
    if op.startswith("v_"):
        return "valu"
    return "other"


def kernels_of(asm):
    """{name: (lines of the body, metadata dict)}"""
    out = {}
    lines = asm.splitlines()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", asm, flags=re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                      for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    i = 0
    while i < len(lines):
        m = re.match(r"^(\w+):\s*(;.*)?$", lines[i])
        if m and m.group(1) in meta:
            name, body = m.group(1), []
            i += 1
            while i < len(lines) and not lines[i].startswith("\t.section") and not lines[i].startswith(".Lfunc_end"):
                body.append(lines[i])
                i += 1
            out[name] = (body, meta[name])
        i += 1
    return out


def blocks_of(body):
    """[(label, [opcodes])] in layout order; a block ends at a label or behind a branch.  A skip over code that no lane is live
    for (s_cbranch_execz / execnz, fall-through in the steady state) ends no block: the compiler sinks the transform's last pass
    behind such a skip"""
    blocks, label, ops, index = [], "entry", [], {}
    for ln in body:
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            if ops:
                blocks.append((label, ops))
            label, ops = m.group(1), []
            continue
        s = ln.strip()
        if not s or s.startswith((";", ".", "//")):
            continue
        ops.append(s.split(";")[0].strip())
        if s.startswith(("s_cbranch", "s_branch", "s_endpgm")) and not s.startswith("s_cbranch_exec"):
            blocks.append((label, ops))
            label, ops = label + "+", []
    if ops:
        blocks.append((label, ops))
    for k, (lab, _) in enumerate(blocks):
        index.setdefault(lab, k)
    return blocks, index


def count(ops):
    c = {"valu": 0, "lds": 0, "gload": 0, "gstore": 0, "wait": 0, "other": 0, "v_mov": 0, "n": len(ops)}
    for o in ops:
        op = o.split()[0]
        c[classify(op)] += 1
        if op.startswith("v_mov_b") or op.startswith("v_accvgpr"):
            c["v_mov"] += 1
    return c


def code_bytes(asm, name):
    # the assembler's own size needs an object file; the listing gives the instruction count, and the metadata comment the bytes
    m = re.search(r"; -- End function\n\t\.set " + re.escape(name) + r"\.num_vgpr.*?; codeLenInByte = (\d+)", asm, flags=re.S)
    if m:
        return int(m.group(1))
    m = re.search(re.escape(name) + r":.*?; codeLenInByte = (\d+)", asm, flags=re.S)
    return int(m.group(1)) if m else -1


def report(asm, pattern, minimum, everything, out):
    ks = kernels_of(asm)
    for name in sorted(ks):
        if not re.search(pattern, name):
            continue
        body, meta = ks[name]
        blocks, index = blocks_of(body)
        counts = [count(ops) for _, ops in blocks]
        top = max(c["valu"] for c in counts)
        out.write(f"{name}\n  vgprs {meta['vgpr_count']}  scratch {meta['private_segment_fixed_size']} B  "
                  f"static lds {meta['group_segment_fixed_size']} B  code {code_bytes(asm, name)} B  blocks {len(blocks)}\n")
        for k, ((label, ops), c) in enumerate(zip(blocks, counts)):
            kind = ""
            if c["valu"] >= 0.95 * top and top > 500:
                kind = "transform"
            elif c["gload"] in (32, 48):
                kind = "request"
            elif c["gstore"] in (32, 48):
                kind = "store"
            else:
                last = ops[-1].split()
                if last[0].startswith("s_cbranch") and index.get(last[-1], len(blocks)) <= k:
                    kind = "back-edge"
            if not everything and not kind and c["n"] < minimum:
                continue
            out.write(f"  {label:<14} {kind:<10} n {c['n']:>5}  valu {c['valu']:>5} (v_mov {c['v_mov']:>3})  lds {c['lds']:>4}  "
                      f"gload {c['gload']:>3}  gstore {c['gstore']:>3}  wait {c['wait']:>3}  other {c['other']:>4}\n")


def normal(body):
    """the instructions of a kernel with the function's number taken out of its labels"""
    ops = []
    for ln in body:
        t = ln.split(";")[0].strip()
        if t and not t.startswith((".p2align", ".loc", ".file", ".cfi")):
            ops.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return ops


def same_as(asm, other, pattern, out):
    a, b = kernels_of(asm), kernels_of(other)
    for name in sorted(a):
        if re.search(pattern, name):
            continue
        if name not in b:
            out.write(f"  {name}: not in the other tree\n")
            continue
        na, nb = normal(a[name][0]), normal(b[name][0])
        out.write(f"  {name}: {'identical' if na == nb else 'DIFFERENT'} ({len(na)} lines, vgprs {a[name][1]['vgpr_count']}, "
                  f"scratch {a[name][1]['private_segment_fixed_size']} B)\n")


def compile_asm(hipcc, tree, file, flags, keep=""):
    src = os.path.join(tree, "llzlab_amd", "csrc", "kernels", file + ".hip")
    with tempfile.TemporaryDirectory() as tmp:
        s = keep or os.path.join(tmp, "k.s")
        subprocess.check_call([hipcc] + FLAGS + flags.split() + ["--cuda-device-only", "-S", src, "-o", s],
                              stderr=subprocess.DEVNULL)
        return open(s).read()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--file", default="fir_ols", help="kernel file under csrc/kernels, without .hip")
    ap.add_argument("--kernel", default=r"k_fir_ols_(chain|seg)_f32")
    ap.add_argument("--min", type=int, default=40)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--flags", default="", help="extra hipcc flags, e.g. -DLLZ_OLS_SB_INT_INDEX")
    ap.add_argument("--keep", default="", help="write the assembly here as well")
    ap.add_argument("--same-as", default="", help="another tree: compare the kernels that do not match --kernel")
    a = ap.parse_args()
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    asm = compile_asm(hipcc, a.tree, a.file, a.flags, a.keep)
    if a.same_as:
        same_as(asm, compile_asm(hipcc, a.same_as, a.file, ""), a.kernel, sys.stdout)
    else:
        report(asm, a.kernel, a.min, a.all, sys.stdout)


if __name__ == "__main__":
    main()
