#!/usr/bin/env python3
"""Compare the kernels of two builds of lkg_gemm_tall.hip instruction by instruction (no GPU needed).

Both inputs are device assembly, made with the library's flags (literalkg_amd/build.py):
    hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 --cuda-device-only -S -I literalkg_amd/csrc -I include \
        lkg_gemm_tall.hip -o tall.s
    python tools/tall_isa_compare.py parent.s new.s > profiles/tall_cleanup_isa.txt
Kernels are matched by base name and (BN, EPI, ONE): the mangled names differ when template parameters come or go (a
parent instantiation with WN != 64 or TM_ != 128 has no counterpart and is listed as such).  Comments and the numbers of
local labels do not count; .vgpr_count, .sgpr_count, LDS and scratch sizes of the metadata must be equal too."""
import difflib
import re
import sys

EPI = {0: "PLAIN", 1: "GATE", 2: "ACTLN"}
DIFF_LINES = 60          # of a differing kernel's unified diff that are printed


def key_of(sym):
    m = re.search(r"\d+(gemm_tall_kernel|b_planes_kernel|b_exponent_kernel|row_absmax_kernel|gemm_tall_ws_kernel)"
                  r"(?:I((?:L[ib]\d+E)+)E)?E", sym)
    if not m:
        return sym
    base, targs = m.group(1), re.findall(r"L([ib])(\d+)E", m.group(2) or "")
    vals = [int(v) for _, v in targs]
    if base == "gemm_tall_kernel":
        bn, epi, one = vals[:3]
        rest = vals[3:]
        if rest and rest != [64, 128]:
            return f"gemm_tall_kernel<{bn}, {EPI[epi]}, {'one' if one else 'two'}, WN={rest[0]}, TM={rest[1]}>"
        return f"gemm_tall_kernel<{bn}, {EPI[epi]}, {'one' if one else 'two'}>"
    if base == "gemm_tall_ws_kernel":
        return f"gemm_tall_ws_kernel<{EPI[vals[0]]}>"
    return base + (f"<{vals[0]}>" if vals else "")


def parse(path):
    text = open(path).read()
    kernels = {}
    # function bodies: from "SYM:" after ".type SYM,@function" to ".Lfunc_end"
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        sym, body = m.group(1), m.group(2)
        labels, stream = {}, []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line == sym + ":" or (line.startswith(".") and not line.startswith(".LBB")):
                continue
            line = re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), line)
            stream.append(re.sub(r"\s+", " ", line.replace(sym, "SELF")))
        kernels[key_of(sym)] = {"sym": sym, "stream": stream}
    # metadata: one YAML entry per kernel, closed by its .wavefront_size
    for m in re.finditer(r"^\s*- \.agpr_count:.*?\.wavefront_size:", text, re.S | re.M):
        entry = m.group(0)
        sym = re.search(r"\.symbol:\s+(\S+)\.kd", entry).group(1)
        meta = {f: int(re.search(rf"\.{f}:\s+(\d+)", entry).group(1))
                for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}
        kernels[key_of(sym)]["meta"] = meta
    return kernels


def main():
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    print(f"{'kernel':46s} {'instructions':>12s}  {'vgpr':>4s} {'sgpr':>4s} {'lds':>6s} {'scratch':>7s}  verdict")
    bad = 0
    for k in sorted(new):
        n = new[k]
        insn = sum(1 for l in n["stream"] if not l.endswith(":"))
        mt = n["meta"]
        cols = f"{k:46s} {insn:12d}  {mt['vgpr_count']:4d} {mt['sgpr_count']:4d} {mt['group_segment_fixed_size']:6d} {mt['private_segment_fixed_size']:7d}"
        if k not in old:
            print(cols + "  NEW (no parent counterpart)")
            bad += 1
            continue
        o = old[k]
        same = o["stream"] == n["stream"] and o["meta"] == mt
        print(cols + ("  SAME" if same else "  DIFF"))
        if not same:
            bad += 1
            if o["meta"] != mt:
                print(f"    parent metadata: {o['meta']}")
            ops_old, ops_new = [l.split(" ")[0] for l in o["stream"]], [l.split(" ")[0] for l in n["stream"]]
            differing = sum(1 for a, b in zip(o["stream"], n["stream"]) if a != b) + abs(len(o["stream"]) - len(n["stream"]))
            print(f"    parent {len(o['stream'])} lines, new {len(n['stream'])} lines, {differing} differ; opcode sequence "
                  f"{'identical (operands differ: register numbers, kernel-argument offsets)' if ops_old == ops_new else 'differs'}")
            diff = list(difflib.unified_diff(o["stream"], n["stream"], "parent", "new", n=1, lineterm=""))
            for line in diff[:DIFF_LINES]:
                print("    " + line)
            if len(diff) > DIFF_LINES:
                print(f"    ... ({len(diff) - DIFF_LINES} more diff lines)")
    gone = sorted(k for k in old if k not in new)
    print(f"\nparent kernels without a counterpart (removed): {len(gone)}")
    for k in gone:
        print(f"    {k}")
    print(f"\n{len(new)} kernels in the new file, {len(new) - bad} SAME, {bad} not")
    return 0


if __name__ == "__main__":
    sys.exit(main())
