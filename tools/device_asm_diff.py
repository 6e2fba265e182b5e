#!/usr/bin/env python3
"""Compare the device code of two source trees, unit by unit and kernel by kernel (no GPU needed).

    tools/device_asm_diff.py OLD_TREE NEW_TREE [--units tracking tracking_od ...] [--jobs N] [--out DIR]

Every csrc/*.hip unit of both trees is compiled to device assembly with the unit's own flags (CXXFLAGS + FLAGS_<unit>,
--offload-device-only -S), read from NEW_TREE's csrc/Makefile for both trees (a change of flags is not what this tool compares); the guarded units are compiled a second time with the guard build's flags.
Lines that name the per-file symbol __hip_cuid_ are dropped.  A unit is EQUAL when both trees give the same set of
.amdhsa_kernel symbols and every kernel's text, from its label to the end of its .amdhsa_kernel block, is the same; the order in
which the kernels were instantiated does not count, and is reported.  Exit status 1 when any unit differs."""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def unit_flags(tree):
    """FLAGS_<unit>, SAFE_RA, CXXFLAGS and GUARDED as the Makefile of `tree` sets them (simple := assignments only)."""
    v = {}
    for line in open(os.path.join(tree, "safe_control_amd", "csrc", "Makefile")):
        m = re.match(r"^(\w+)\s*[:?]?=\s*(.*)$", line.rstrip("\n"))
        if m:
            v[m.group(1)] = m.group(2)
    def expand(s):
        for _ in range(8):
            s = re.sub(r"\$\((\w+)\)", lambda m: v.get(m.group(1), ""), s)
        return s.split()
    return v, expand


def kernels(asm_path):
    lines = [l for l in open(asm_path) if "__hip_cuid_" not in l]
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    text = {}
    for n in names:
        a = next(i for i, l in enumerate(lines) if l.startswith(n + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        text[n] = "".join(lines[a:b + 1])
    return names, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--units", nargs="*"); ap.add_argument("--jobs", type=int, default=4); ap.add_argument("--out", default="build/asm_diff")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    v, expand = unit_flags(a.new)
    csrc = lambda t: os.path.join(t, "safe_control_amd", "csrc")
    units = a.units or sorted(f[:-4] for f in os.listdir(csrc(a.new)) if f.endswith(".hip"))
    jobs = [(u, "", expand(v.get("FLAGS_" + u, ""))) for u in units]
    jobs += [(u, "+guard", expand("$(SAFE_RA)")) for u in units if u in v.get("GUARDED", "").split()]

    def run(job):
        u, tag, flags = job
        outs = []
        for side, tree in (("old", a.old), ("new", a.new)):
            o = os.path.join(a.out, f"{u}{tag}.{side}.s")
            cmd = [v.get("HIPCC", "/opt/rocm/bin/hipcc")] + [f for f in expand("$(CXXFLAGS)") if f != "-Wall"] + flags + \
                  ["--offload-device-only", "-S", os.path.join(csrc(tree), u + ".hip"), "-o", o]
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.exit(f"{' '.join(cmd)}\nfailed:\n{r.stderr[-4000:]}")
            outs.append(o)
        (n0, t0), (n1, t1) = kernels(outs[0]), kernels(outs[1])
        equal = set(n0) == set(n1) and all(t0[k] == t1[k] for k in n0)
        differ = [k for k in n0 if k in t1 and t0[k] != t1[k]]
        return u + tag, len(n0), len(n1), equal, n0 != n1, differ

    bad = 0
    with ThreadPoolExecutor(a.jobs) as ex:
        for name, k0, k1, equal, reordered, differ in ex.map(run, jobs):
            print(f"{name:28s} kernels {k0:3d} -> {k1:3d}  {'EQUAL' if equal else 'DIFFERENT'}  order {'changed' if reordered else 'same'}",
                  flush=True)
            for k in differ[:5]:
                print("    differs:", k)
            bad += 0 if equal else 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
