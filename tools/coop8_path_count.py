#!/usr/bin/env python3
"""Executed instruction slots of one wave of cbfqp_coop8_du_kernel<float, true, true, false>, by class.

CPU only.  Builds the gfx950 assembly of safe_control_amd/csrc/cbf_qp_f32c64.hip with the flags the Makefile gives that file
(or reads a finished listing, --asm), and walks the kernel from its entry to s_endpgm.  An s_branch is followed; at every
conditional branch the walk does what the table says: one letter per conditional branch in the order the walk meets them, T =
taken, N = falls through.  A lone wave per SIMD issues one instruction every four cycles whatever it is, so the length of this
walk is what the headline launch pays for.

The default table is the wave the benchmark batch is made of: every lane holds a circle (flag 0), soft mode, |theta| < 1e5, some
row violated at u_box (the wave enters the solve), and neither exit to the generic sequence is taken (no row with nn == 0, no flat
direction, no parallel partner).  On that path every conditional branch falls through -- the table holds no T -- and the walk
reaches s_endpgm without jumping over any cold code.  The count of taken branches printed at the end includes the unconditional
ones the walk follows: it is 1, the s_branch of the kernel-argument preload prologue in front of the entry's code.  The table belongs to ONE
listing: when the block layout changes, run with --trace, read the condition in front of each branch, and write the new table.
--trace prints every conditional branch met with its line, the instruction that set its condition and what the table did.  A table
that is too short, too long, or names a branch that the walk does not meet is an error, not a shorter count.

Instructions are classified by mnemonic prefix only:
  vector   v_* without a DPP control          dpp      v_*_dpp
  salu     s_* not named below                nop      s_nop
  control  s_branch, s_cbranch_*, s_*_saveexec_*, s_endpgm
  memory   global_*, flat_*, ds_*, s_load_*, s_waitcnt

usage: coop8_path_count.py [--asm file.s] [--kernel substring] [--table TNTN...] [--trace]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safe_control_amd", "csrc")
KERNEL = "cbfqp_coop8_du_kernelIfLb1ELb1ELb0E"     # <float, FULL = true, HAS_H = true, HARD = false>

# One letter per conditional branch on the path of the default wave, in the order the walk meets them (see the docstring).
#    1  N  the early exit (some flag not 0, or not |theta| < 1e5): no lane
#    2  N  the compiler's own test that the early exit was not taken (it keeps the two arms of that branch as a flag)
#    3  N  the solve: some row of the wave is violated at u_box
#    4  N  the late exit (a row without nn > 0, a flat direction, a parallel partner): no lane
#    5  N  the store of u and status: lane 0 of every group
# The listing of the commit before (ten branches, six of them taken around cold blocks) is walked by TNTNTNTTTN.
DEFAULT_TABLE = "NNNNN"

CLASSES = ("vector", "dpp", "salu", "nop", "control", "memory")


def classify(mn):
    if mn == "s_nop":
        return "nop"
    if mn in ("s_branch", "s_endpgm") or mn.startswith("s_cbranch") or "saveexec" in mn:
        return "control"
    if mn.startswith(("global_", "flat_", "ds_", "s_load", "s_waitcnt", "buffer_", "scratch_")):
        return "memory"
    if mn.startswith("v_"):
        return "dpp" if mn.endswith("_dpp") else "vector"
    if mn.startswith("s_"):
        return "salu"
    raise SystemExit(f"unclassified mnemonic {mn!r}")


def makefile_flags(unit):
    """CXXFLAGS and FLAGS_<unit> of csrc/Makefile, through make itself so that the two cannot drift apart."""
    mk = "include Makefile\nprint-flags:\n\t@echo $(CXXFLAGS) $(FLAGS_%s)\n" % unit
    out = subprocess.run(["make", "-s", "-C", CSRC, "-f", "-", "print-flags"], input=mk, capture_output=True, text=True, check=True)
    return out.stdout.split()


def build_asm(unit="cbf_qp_f32c64"):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.run([hipcc, *makefile_flags(unit), "--cuda-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", out],
                       check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def kernel_body(text, kernel):
    """[(line number, label or None, mnemonic or None, text)] of the first symbol whose name holds `kernel`."""
    lines = text.splitlines()
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and kernel in l), None)
    if start is None:
        raise SystemExit(f"no kernel symbol holds {kernel!r}")
    body = []
    for i in range(start + 1, len(lines)):
        l = lines[i].split(";")[0].rstrip()
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            body.append((i + 1, m.group(1), None, l))
            continue
        s = l.strip()
        if not s or s.startswith("."):
            continue
        body.append((i + 1, None, s.split()[0], s))
    return body


def sets_condition(mn, txt):
    """For --trace only: does this instruction write what a conditional branch tests?  Compares and scalar mask algebra by
    mnemonic, anything else by a first operand that is vcc, scc or exec."""
    if mn.startswith(("s_cmp", "v_cmp", "s_and", "s_or", "s_xor")):
        return True
    operands = txt.split(None, 1)[1] if " " in txt else ""
    return re.search(r"\b(vcc|scc|exec)\b", operands.split(",")[0]) is not None


def walk(body, table, trace=False):
    labels = {lab: n for n, (_, lab, _, _) in enumerate(body) if lab}
    counts = dict.fromkeys(CLASSES, 0)
    taken = 0                                   # taken branches on the path, conditional or not: each is an instruction-fetch redirect
    pc, used, last_cond, steps = 0, 0, "", 0
    while True:
        steps += 1
        if steps > 100000:
            raise SystemExit("the walk does not end: the table sends it round a loop")
        line, lab, mn, txt = body[pc]
        pc += 1
        if lab:
            continue
        mn = re.sub(r"_e(32|64)$", "", mn)
        counts[classify(mn)] += 1
        if mn == "s_endpgm":
            break
        if sets_condition(mn, txt):
            last_cond = f"{line}: {txt}"
        if mn == "s_branch":
            pc = labels[txt.split()[1]]
            taken += 1
        elif mn.startswith("s_cbranch"):
            if used >= len(table):
                raise SystemExit(f"the table ends before the walk does: branch {used + 1} at line {line}: {txt}   (after {last_cond})")
            take = table[used] == "T"
            used += 1
            if trace:
                print(f"  branch {used:2d}  line {line:5d}  {txt:34s} {'taken' if take else 'falls through':14s} after {last_cond}")
            if take:
                pc = labels[txt.split()[1]]
                taken += 1
    if used != len(table):
        raise SystemExit(f"the walk met {used} conditional branches, the table has {len(table)}")
    return counts, taken


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="a finished --cuda-device-only -S listing instead of building one")
    ap.add_argument("--kernel", default=KERNEL)
    ap.add_argument("--table", default=DEFAULT_TABLE)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if not re.fullmatch(r"[TN]*", a.table):
        raise SystemExit("the table is a string of T and N")
    text = open(a.asm).read() if a.asm else build_asm()
    body = kernel_body(text, a.kernel)
    counts, taken = walk(body, a.table, a.trace)
    static = sum(1 for _, lab, _, _ in body if not lab)
    print(f"kernel *{a.kernel}*: {static} instructions in the listing, table {a.table}")
    for c in CLASSES:
        print(f"  {c:8s} {counts[c]:4d}")
    print(f"  {'total':8s} {sum(counts.values()):4d}")
    print(f"  taken branches on the path: {taken} (the s_branch of the kernel-argument preload prologue included)")


if __name__ == "__main__":
    sys.exit(main())
