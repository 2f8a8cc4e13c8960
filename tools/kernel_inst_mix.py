#!/usr/bin/env python3
"""Static instruction mix of one gfx950 kernel: cross-compiles a .hip unit to assembly (no GPU needed) and prints, for every kernel
whose demangled name contains KERNEL, the instructions by class, the VGPR -> VGPR v_mov count, the v_cndmask and v_swap counts and
every run of at least --min-run consecutive v_mov instructions inside one basic block, with the loop depth the compiler's own
`Loop:` comments give that block.  A static count: what a wave executes depends on the path it takes.

usage: tools/kernel_inst_mix.py oak_amd/csrc/oakgpu.hip 'k_rollout_queue<64, 4>' [--min-run 8] [--json] [--asm FILE] [--flags "..."]
  --asm FILE   read this assembly instead of compiling (the unit is then only a label in the output)
  --flags      extra compiler flags, e.g. "-DOAK_LONG_STEPS=300"
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S"]  # as build(): -O3 -std=c++17


def compile_to_asm(src, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "unit.s")
        subprocess.check_call([hipcc] + BASE_FLAGS + extra + [src, "-o", out])
        return open(out).read()


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines())) if r.returncode == 0 else {n: n for n in names}


def kernels(asm):
    """{mangled name: its lines}: from the function's label to its .Lfunc_end."""
    lines = asm.splitlines()
    labels = {}
    for k, l in enumerate(lines):
        m = re.match(r"([A-Za-z_][\w$.]*):", l)
        if m:
            labels.setdefault(m.group(1), k)
    funcs = [m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m]
    out = {}
    for name in funcs:
        if name not in labels:
            continue
        start = labels[name]
        end = next((k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end")), len(lines))
        out[name] = lines[start + 1:end]
    return out


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier", "s_setprio", "s_endpgm")):
        return "wait/misc"
    if op.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "other"


def mix(body, min_run):
    classes = collections.Counter()
    c = collections.Counter()
    runs = []
    depth, block = 0, "entry"
    run = None  # [block, depth, moves, of them VGPR -> VGPR]

    def close():
        nonlocal run
        if run and run[2] >= min_run:
            runs.append(dict(block=run[0], loop_depth=run[1], moves=run[2], vgpr_to_vgpr=run[3]))
        run = None
    for line in body:
        s = line.strip()
        m = re.match(r"(\.LBB\d+_\d+):", s) or re.match(r";\s*%bb\.(\d+):", s)
        if m:                                  # a new basic block: depth 0 unless its comments say otherwise
            close()
            block, depth = m.group(1), 0
        d = re.search(r"(?:Loop Header: |in Loop: .*)Depth=(\d+)", s)
        if d:
            depth = int(d.group(1))
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        if not re.match(r"[a-z]+_", op):
            continue
        classes[classify(op)] += 1
        c["instructions"] += 1
        is_mov = op in ("v_mov_b32_e32", "v_mov_b32", "v_mov_b64_e32", "v_mov_b64")
        v2v = False
        if is_mov:
            ops = s.split(";")[0].split(None, 1)[1].split(",")
            v2v = len(ops) == 2 and re.match(r"\s*v(\d+|\[\d+:\d+\])\s*$", ops[1]) is not None
            c["v_mov_b64" if "b64" in op else "v_mov_b32"] += 1
            c["v_mov_vgpr_to_vgpr"] += v2v
            if run is None:
                run = [block, depth, 0, 0]
            run[2] += 1
            run[3] += v2v
        else:
            close()
            if op.startswith("v_cndmask"):
                c["v_cndmask"] += 1
            elif op.startswith("v_swap"):
                c["v_swap"] += 1
    close()
    by_depth = collections.Counter()
    for r in runs:
        by_depth[r["loop_depth"]] += r["moves"]
    return dict(classes=dict(sorted(classes.items())), counts={k: int(c[k]) for k in ("instructions", "v_mov_b32", "v_mov_b64", "v_mov_vgpr_to_vgpr", "v_cndmask", "v_swap")},
                min_run=min_run, move_runs=runs, moves_in_runs_by_loop_depth={str(k): v for k, v in sorted(by_depth.items())})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("unit")
    ap.add_argument("kernel")
    ap.add_argument("--min-run", type=int, default=8)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--asm")
    ap.add_argument("--flags", default="")
    a = ap.parse_args()
    asm = open(a.asm).read() if a.asm else compile_to_asm(a.unit if os.path.isabs(a.unit) else os.path.join(os.getcwd(), a.unit), a.flags.split())
    ks = kernels(asm)
    names = demangle(list(ks))
    hits = {n: ks[n] for n in ks if a.kernel in names.get(n, n)}
    if not hits:
        sys.exit("no kernel matches %r; the unit has:\n  %s" % (a.kernel, "\n  ".join(sorted(names.values()))))
    res = {names[n]: mix(body, a.min_run) for n, body in hits.items()}
    if a.json:
        print(json.dumps(dict(unit=os.path.relpath(a.unit, ROOT) if os.path.isabs(a.unit) else a.unit, kernels=res), indent=1))
        return
    for name, r in res.items():
        print(name[:150])
        print("  " + "  ".join("%s %d" % kv for kv in r["classes"].items()))
        print("  " + "  ".join("%s %d" % kv for kv in r["counts"].items()))
        print("  moves in runs of >= %d, by loop depth: %s" % (a.min_run, r["moves_in_runs_by_loop_depth"] or "none"))
        for run in r["move_runs"]:
            print("    %-12s depth %d  %3d moves (%d VGPR -> VGPR)" % (run["block"], run["loop_depth"], run["moves"], run["vgpr_to_vgpr"]))


if __name__ == "__main__":
    main()
