#!/usr/bin/env python3
"""Static instruction census of the literal SRBD kernels (CPU only).

Compiles quadrupedal_loco_amd/csrc/qloco_srbd_lit.hip for gfx950, device
only, to assembly with the flags of quadrupedal_loco_amd/build.py plus line
tables, and counts, per kernel and per phase of srbd_lit_one, the VALU
instructions (fp64 ones and MFMA apart), LDS instructions and s_nop padding.  Every
instruction is attributed to the source line of its line-table entry; lines
of inlined helpers outside srbd_lit_one (DPP macros, math library code) count
for the phase of the last srbd_lit_one line seen before them, so the split
between neighbouring phases is approximate where the scheduler interleaves
them; the kernel totals and the resource lines are exact.

For the ADMM inner loop alone (the innermost loop that holds the DPP matvec
and ends in a scalar back-edge: one iteration, executed as counted) it also
prints the VALU instructions, the LDS reads by width, the LDS writes, the
s_waitcnt that wait on lgkmcnt and the s_nop.

  python tools/lit_valu_census.py [--src FILE] [--asm FILE] [--tag TEXT]

--asm reads an existing assembly file (made with -gline-tables-only)."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quadrupedal_loco_amd import build as qbuild  # noqa: E402

SRC = os.path.join(qbuild.CSRC, "qloco_srbd_lit.hip")
# (phase, marker that opens it): in source order inside srbd_lit_one
MARKERS = [
    ("inputs, model, gradient, rows", "// ---------------- 1. inputs"),
    ("Ruiz", "// ---------------- 5. modified Ruiz"),
    ("scaled problem to LDS", "// block-uniform scalars live in SGPRs"),
    ("residuals (P x, checks' norms)", "auto p_times_x = "),
    ("warm start", "// warm start (x, z, y) before the first factorisation"),
    ("G^-1 tables", "// G^-1 in six N x N blocks"),
    ("factorisation", "// ---------------- 6a. factorisation"),
    ("ADMM iteration body", "bool refactor = false;"),
    ("termination and rho checks", "iter = ui(iter);"),
    ("outputs, records", "// ---------------- 7. outputs"),
]
INVERT = ("// In-place Gauss-Jordan inverse of the 60 x 60", "// Lane-derived indices re-derived")


def compile_asm(src, out):
    cmd = ([qbuild.HIPCC, "--offload-arch=" + qbuild.ARCH, "-x", "hip"] + qbuild.COMMON +
           qbuild.EXTRA["qloco_srbd_lit.hip"] + ["-gline-tables-only", "--cuda-device-only", "-S", src, "-o", out])
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def phase_map(src):
    lines = open(src).read().split("\n")

    def find(text, start=0):
        for i in range(start, len(lines)):
            if text in lines[i]:
                return i + 1
        raise SystemExit("marker not found in %s: %s" % (src, text))

    one = find("void srbd_lit_one(")
    bounds = [(name, find(text, one)) for name, text in MARKERS]
    end = find("template <bool WS>", one)
    inv = (find(INVERT[0]), find(INVERT[1]))

    def phase(line):
        if inv[0] <= line < inv[1]:
            return "factorisation"
        if line < bounds[0][1] or line >= end:
            return None
        cur = bounds[0][0]
        for name, first in bounds:
            if line >= first:
                cur = name
        return cur
    return phase, [n for n, _ in MARKERS]


def census(asm, src):
    phase, names = phase_map(src)
    files, kernels, meta = {}, {}, {}
    cur, ph, src_base = None, None, os.path.basename(src)
    text = open(asm).read()
    notes = text[text.find("amdhsa.kernels:"):]
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:  # one entry per kernel
        m = re.search(r"\n\s+\.name:\s+(\S+)", blk)
        found = {k: re.search(r"\n\s+\.%s:\s+(\d+)" % k, blk) for k in (
            "vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
            "vgpr_spill_count", "kernarg_segment_size")}
        if m:
            meta[m.group(1)] = {k: int(v.group(1)) if v else None for k, v in found.items()}
    for ln in text.split("\n"):
        s = ln.strip()
        m = re.match(r"\.file\s+(\d+)\s+(?:\"([^\"]*)\"\s+)?\"([^\"]*)\"", s)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3))
            continue
        m = re.match(r"(_ZN5qloco\w+):", ln)
        if m and "kernel" in m.group(1):
            cur = kernels.setdefault(m.group(1), {})
            ph = names[0]
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            if files.get(int(m.group(1))) == src_base:
                p = phase(int(m.group(2)))
                if p:
                    ph = p
            continue
        m = re.match(r"([sv]_\w+|ds_\w+|global_\w+|buffer_\w+|flat_\w+|scratch_\w+)\b", s)
        if not m:
            continue
        op = m.group(1)
        row = cur.setdefault(ph, {"valu": 0, "f64": 0, "mfma": 0, "lds": 0, "nop": 0, "vmem": 0})
        if op.startswith("v_"):
            row["valu"] += 1
            if op.startswith("v_mfma"):
                row["mfma"] += 1
            elif re.search(r"_f64|_i64|_u64|_b64", op):
                row["f64"] += 1
        elif op.startswith("ds_"):
            row["lds"] += 1
        elif op == "s_nop":
            row["nop"] += 1
        elif not op.startswith("s_"):
            row["vmem"] += 1
    return names, kernels, meta


def inner_loop(asm):
    """{kernel: counts of the ADMM iteration's loop body}: the block from the
    last label before the 60-column matvec's first row_newbcast:14 operand that
    follows an `s_cbranch_scc1` back to that label."""
    lines = open(asm).read().split("\n")
    res, cur = {}, None
    for i, ln in enumerate(lines):
        m = re.match(r"(_ZN5qloco\w+):", ln)
        if m and "kernel" in m.group(1):
            cur = m.group(1)
            continue
        m = re.match(r"\s+s_cbranch_scc1\s+(\.LBB\d+_\d+)", ln)
        if not (m and cur) or cur in res:
            continue
        top = next((j for j in range(i, -1, -1) if lines[j].startswith(m.group(1) + ":")), None)
        body = [x.strip() for x in lines[top:i + 1]] if top is not None else []
        if sum("row_newbcast:14" in x for x in body) < 4 or any(re.match(r"\.LBB\d+_\d+:", x) for x in body[1:]):
            continue
        c = collections.OrderedDict((k, 0) for k in (
            "VALU", "LDS read b128", "LDS read other", "LDS write", "s_waitcnt lgkmcnt", "s_nop", "scratch"))
        for x in body:
            op = x.split()[0] if x.split() else ""
            if op.startswith("v_"):
                c["VALU"] += 1
            elif op.startswith("ds_read"):
                c["LDS read b128" if op == "ds_read_b128" else "LDS read other"] += 1
            elif op.startswith("ds_write"):
                c["LDS write"] += 1
            elif op == "s_waitcnt" and "lgkmcnt" in x:
                c["s_waitcnt lgkmcnt"] += 1
            elif op == "s_nop":
                c["s_nop"] += 1
            elif op.startswith("scratch_"):
                c["scratch"] += 1
        res[cur] = c
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=SRC)
    ap.add_argument("--asm")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    asm = a.asm
    tmp = None
    if not asm:
        tmp = tempfile.mkdtemp()
        asm = os.path.join(tmp, "lit.s")
        compile_asm(a.src, asm)
    names, kernels, meta = census(asm, a.src)
    loops = inner_loop(asm)
    print("# literal SRBD kernels: static instruction census %s" % a.tag)
    print("# (static counts per phase of srbd_lit_one; 64-bit VALU and MFMA counted apart and included in VALU)")
    for k in sorted(kernels):
        r = meta.get(k, {})
        print("\n%s" % k)
        print("  vgpr %s  sgpr %s  lds %s B  private %s B  spills %s  kernarg %s B" % (
            r.get("vgpr_count"), r.get("sgpr_count"), r.get("group_segment_fixed_size"),
            r.get("private_segment_fixed_size"), r.get("vgpr_spill_count"), r.get("kernarg_segment_size")))
        print("  %-34s %7s %7s %6s %6s %6s %6s" % ("phase", "VALU", "64-bit", "MFMA", "LDS", "s_nop", "VMEM"))
        tot = {"valu": 0, "f64": 0, "mfma": 0, "lds": 0, "nop": 0, "vmem": 0}
        for n in names:
            row = kernels[k].get(n)
            if not row:
                continue
            print("  %-34s %7d %7d %6d %6d %6d %6d" % (n, row["valu"], row["f64"], row["mfma"], row["lds"], row["nop"], row["vmem"]))
            for key in tot:
                tot[key] += row[key]
        print("  %-34s %7d %7d %6d %6d %6d %6d" % ("total", tot["valu"], tot["f64"], tot["mfma"], tot["lds"], tot["nop"], tot["vmem"]))
        if k in loops:
            print("  ADMM inner loop, one iteration: " + ", ".join("%s %d" % kv for kv in loops[k].items()))
    if tmp:
        os.remove(asm)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
