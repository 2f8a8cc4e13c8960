#!/usr/bin/env python3
"""The output of tools/move_carry_ab.sh ($OUT, default prof_out/move_carry/) -> profiles/r16_move_carry.json: every run of the alternating A/B of both commands,
the --dump-outputs verdicts, the counters and the region profile (exec_move per pass) per threshold, and the verdict by the
project's rule (a setting is a gain on a command only if its slowest run lies above the parent's fastest).
usage: tools/move_carry_summary.py [chosen default]"""
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.environ.get("OUT") or os.path.join(ROOT, "prof_out", "move_carry")
last = lambda f: json.loads(open(f).read().strip().splitlines()[-1])
variants = sorted({re.match(r"run_default_(\w+?)_\d+\.json$", os.path.basename(f)).group(1) for f in glob.glob(os.path.join(src, "run_default_*.json"))},
                  key=lambda v: -1 if v == "parent" else int(v[1:]))
runs, summary, errors = {}, {}, 0
for cmd in ("default", "steps20"):
    for v in variants:
        files = sorted(glob.glob(os.path.join(src, "run_%s_%s_*.json" % (cmd, v))), key=lambda f: int(re.search(r"_(\d+)\.json$", f).group(1)))
        vals = []
        for f in files:
            d = last(f)
            vals.append(round(d["value"] / 1e9, 3))
            errors += sum(d["config"]["queue_counters"]["error_word_63"])
        runs["%s_%s" % (cmd, v)] = vals
        summary["%s_%s" % (cmd, v)] = {"n": len(vals), "min": min(vals), "median": statistics.median(vals), "max": max(vals)}
verdict = {}
for cmd in ("default", "steps20"):
    p = summary["%s_parent" % cmd]
    for v in variants[1:]:
        b = summary["%s_%s" % (cmd, v)]
        verdict["%s_%s" % (cmd, v)] = {"gain": b["min"] > p["max"], "loss_beyond_spread": b["max"] < p["min"], "median_ratio": round(b["median"] / p["median"], 4)}
sites, pmc = {}, {}
for v in variants:
    f = os.path.join(src, "site_%s.json" % v)
    if os.path.exists(f):
        d = last(f)
        keep = {r["region"]: {k: round(r[k], 3) if isinstance(r[k], float) else r[k] for k in ("passes", "lanes_per_pass", "cycles_per_pass", "share_of_step_cycles")}
                for r in d["rows"] if r["region"] in ("refill", "step", "legal_draw", "order", "exec_move", "exec_move_k0", "exec_move_k1", "switch_in", "faint_residual", "publish")}
        step = keep["step"]
        sites[v] = {"turn_steps": d["turn_steps"], "launch_ms_profile_build": round(d["launch_ms"], 2), "regions": keep,
                    "wave_iterations": step["passes"], "step_cycles_total_G": round(step["passes"] * step["cycles_per_pass"] / 1e9, 2),
                    "exec_move_passes_per_wave_iteration": round(keep["exec_move"]["passes"] / step["passes"], 3),
                    "exec_move_passes_per_1000_turn_steps": round(1000.0 * keep["exec_move"]["passes"] / d["turn_steps"], 2)}
    f = os.path.join(src, "pmc_%s.json" % v)
    if os.path.exists(f):
        pmc[v] = {k: (round(x, 3) if isinstance(x, float) and x < 1e6 else x) for k, x in last(f).items()}
out = {
    "what": "round 16: move carry of k_rollout_queue (oakgpu_set_move_carry).  `parent` = the parent commit's library under its own Python package; "
            "`bN` = this commit's library with OAKGPU_MOVE_CARRY=N.  Commands: `python bench.py --gpus 1 --workload rollout --no-cpu-baseline` (default, "
            "160 steps, two streams) and the same with --steps 20 --warmup 5 (steps20, one launch).  G turn-steps/s.",
    "order": "alternating, a fresh process per run: even repetitions parent b0 b8 b16 b32 b64, odd ones reversed; within a variant the default run, then the steps20 run",
    "rule": "a setting is a gain on a command only if its slowest run lies above the parent's fastest",
    "runs": runs, "summary": summary, "verdict": verdict,
    "error_word_63_sum_over_all_runs": errors,
    "dump_outputs_against_parent": open(os.path.join(src, "dump_compare.txt")).read().split("\n")[:-1],
    "counters_one_launch_of_1310720_playouts": pmc,
    "site_profile_one_launch_of_1310720_playouts": sites,
    "site_profile_note": "-DOAKGPU_SITE_PROFILE builds (tools/site_profile.sh); `parent` is the parent commit built with this commit's per-pass sites: its k0 / k1 are "
                         "update_frame's two passes; in this commit k0 is the iteration's first trip through the move pipeline and k1 the second.  A region's "
                         "cycles are wave cycles of the profile build, which runs ~1.6x slower than the product: shares and ratios, not times.",
    "chosen_default": int(sys.argv[1]) if len(sys.argv) > 1 else None,
}
json.dump(out, open(os.path.join(ROOT, "profiles", "r16_move_carry.json"), "w"), indent=1)
for k in summary:
    print("%-18s %s %s" % (k, summary[k], verdict.get(k, "")))
for v in sites:
    r = sites[v]["regions"]
    print(v, "iterations", sites[v]["wave_iterations"], "step cyc", r["step"]["cycles_per_pass"], "total G", sites[v]["step_cycles_total_G"], "k0", r["exec_move_k0"], "k1", r["exec_move_k1"])
