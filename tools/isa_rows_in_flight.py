#!/usr/bin/env python3
"""How many vector loads does each kernel of a HIP source keep in flight?  (no GPU needed)

Compiles the given csrc/*.hip for gfx950 to assembly and prints, per kernel, in text order of the code object:
  loads     global_load* instructions
  batches   the loads issued between two FULL waits (s_waitcnt vmcnt(0)), runs of equal counts folded: "1x9" is nine
            waits with one load each, the signature of a row loop with one row in flight per thread
  max       the largest such batch
  br        conditional branches (s_cbranch_*): a streaming loop whose per-element code tests run-time switches has
            one or two per element
  vgpr      the code object's VGPR count (occupancy: <= 64: 8 waves per SIMD, <= 128: 4)
  scr       bytes of scratch per lane (must stay 0 in a streaming kernel)

Only global_load*, s_waitcnt, s_cbranch* lines and the kernels' metadata are read.  A partial wait (vmcnt(n), n > 0)
does not end a batch: memory returns in order, the loads behind it stay in flight.

    python tools/isa_rows_in_flight.py unidefense_amd/csrc/fused.hip [--filter bn_] [more.hip ...]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-"]

_WAIT_VM = re.compile(r"vmcnt\((\d+)\)")


def assembly(path):
    r = subprocess.run([HIPCC, *FLAGS, path], check=True, capture_output=True, text=True)
    return r.stdout


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:          # no demangler at hand: the mangled names say enough
        return {n: n for n in names}
    out = subprocess.run([tool, *names], check=True, capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def short(name):
    """`void (anonymous namespace)::k<float, 1>(args...)` -> `k<float, 1>`"""
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):          # cut at the argument list: the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i]
    return name


def fold(batches):
    out, i = [], 0
    while i < len(batches):
        j = i
        while j < len(batches) and batches[j] == batches[i]:
            j += 1
        out.append(f"{batches[i]}x{j - i}" if j - i > 1 else str(batches[i]))
        i = j
    return " ".join(out)


def survey(asm):
    """[(mangled name, loads, batches, branches, vgpr, scratch)] for every kernel of an assembly text"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    rows, cur, order = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in kernels:
            cur = rows[m.group(1)] = dict(loads=0, batches=[], run=0, br=0, vgpr=None, scr=None)
            order.append(m.group(1))
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith("global_load"):
            cur["loads"] += 1
            cur["run"] += 1
        elif t.startswith("s_waitcnt"):
            m = _WAIT_VM.search(t)
            if m and int(m.group(1)) == 0 and cur["run"]:
                cur["batches"].append(cur["run"])
                cur["run"] = 0
        elif t.startswith("s_cbranch"):
            cur["br"] += 1
        elif t.startswith("; NumVgprs:"):
            cur["vgpr"] = int(t.split(":")[1])
        elif t.startswith("; ScratchSize:"):
            cur["scr"] = int(t.split(":")[1])
            if cur["run"]:
                cur["batches"].append(cur["run"])
                cur["run"] = 0
            cur = None
    return [(n, rows[n]) for n in order]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--filter", default=None, help="only kernels whose demangled name matches this regular expression")
    ap.add_argument("--width", type=int, default=72, help="columns of the batches field")
    args = ap.parse_args()
    for src in args.sources:
        rows = survey(assembly(src))
        names = demangle([n for n, _ in rows])
        print(f"== {os.path.basename(src)}")
        print(f"{'kernel':58s} {'loads':>5s} {'max':>4s} {'br':>4s} {'vgpr':>4s} {'scr':>4s}  batches between full waits")
        for n, r in rows:
            name = short(names[n])
            if args.filter and not re.search(args.filter, name):
                continue
            b = fold(r["batches"])
            if len(b) > args.width:
                b = b[: args.width - 3] + "..."
            print(f"{name[:58]:58s} {r['loads']:5d} {max(r['batches'], default=0):4d} {r['br']:4d} "
                  f"{r['vgpr'] if r['vgpr'] is not None else -1:4d} {r['scr'] if r['scr'] is not None else -1:4d}  {b}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
