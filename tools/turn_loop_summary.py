#!/usr/bin/env python3
"""The output of tools/turn_loop_ab.sh ($OUT, default prof_out/turn_loop/) -> one JSON record on stdout: every run of the alternating
A/B of both commands with min / median / max, the slowest-above-fastest verdicts against the parent, the --dump-outputs comparison, and
the counters of the profiled launch per turn-step.  profiles/r18_turn_loop.json is this record beside those of the earlier steps.
usage: tools/turn_loop_summary.py [OUT]"""
import collections
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OUT") or os.path.join(ROOT, "prof_out", "turn_loop")


def last_json(path):
    return json.loads([l for l in open(path).read().splitlines() if l.startswith("{")][-1])


runs, err63 = {}, 0
for f in sorted(glob.glob(os.path.join(src, "run_*_*_*.json"))):
    m = re.match(r"run_(default|steps20)_(\w+)_(\d+)\.json", os.path.basename(f))
    r = last_json(f)
    err63 += sum(r.get("queue_counters", {}).get("error_word_63", []))
    runs.setdefault(m.group(1), {}).setdefault(m.group(2), []).append(round(r["value"] / 1e9, 3))
summary, verdict = {}, {}
for cmd, d in runs.items():
    summary[cmd] = {v: dict(min=min(x), median=round(statistics.median(x), 3), max=max(x), n=len(x)) for v, x in d.items()}
    p = summary[cmd].get("parent")
    for v, s in summary[cmd].items():
        if p and v != "parent":
            verdict.setdefault(cmd, {})[v] = ("gain" if s["min"] > p["max"] else "loss" if s["max"] < p["min"] else "inside the spread") + \
                " (median %+.1f %%)" % (100.0 * (s["median"] / p["median"] - 1.0))
counters = {}
for f in sorted(glob.glob(os.path.join(src, "pmc_*.csv"))):
    v = os.path.basename(f)[4:-4]
    tot = collections.defaultdict(float)
    for r in csv.DictReader(open(f)):
        if "k_rollout_queue" in r["Kernel_Name"]:
            tot[r["Counter_Name"]] += float(r["Counter_Value"])
    steps = int(re.search(r"steps (\d+)", open(f[:-4] + ".log").read()).group(1))
    counters[v] = dict(tot, turn_steps=steps, valu_per_turn_step=round(tot["SQ_INSTS_VALU"] / steps, 3), salu_per_turn_step=round(tot["SQ_INSTS_SALU"] / steps, 3),
                       wave_cycles_per_turn_step=round(tot["SQ_WAVE_CYCLES"] / steps, 3), thread_cycles_per_valu_inst=round(tot["SQ_THREAD_CYCLES_VALU"] / tot["SQ_INSTS_VALU"], 3))
dumps = open(os.path.join(src, "dump_compare.txt")).read().split("\n")[:-1] if os.path.exists(os.path.join(src, "dump_compare.txt")) else None
print(json.dumps(dict(order="alternating, both orders, a fresh process per run", rule="a gain only if the branch's slowest run lies above the parent's fastest",
                      runs_G_turn_steps_per_s=runs, summary=summary, verdict_against_parent=verdict, error_word_63_sum_over_all_runs=err63,
                      dump_outputs_against_parent=dumps, counters_one_launch_of_1310720_playouts=counters), indent=1))
