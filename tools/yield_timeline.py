#!/usr/bin/env python3
"""Timeline of the default command's group launches under the yielding schedule, from a kernel trace of
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --workload rollout --no-cpu-baseline`.

  python tools/yield_timeline.py DIR [LAUNCHES] [DRY_MS]      (prints one JSON object)

A launch is a first dispatch of k_rollout_queue (more than half of the device's resident waves) and, under the schedule, one follow-up
dispatch behind it on the same hardware queue.  For the last LAUNCHES (default 8) launches: the launch period, the first dispatch's
length, the follow-up's start, length and waves, and the start of the launch against the other context's first dispatch -- its end,
and its dry moment estimated as its start + DRY_MS (default 8.2: the wave timeline of a lone launch, profiles/r33_yield_schedule.json;
a kernel trace does not show it).  With the schedule off the follow-up fields are null.  Counter collection CSVs in DIR (a run with
--pmc and no tracing) are summed per counter over the k_rollout_queue dispatches instead."""
import csv
import glob
import json
import os
import sys


def read(d, pattern):
    out = []
    for f in sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True)):
        with open(f, newline="") as fh:
            out += list(csv.DictReader(fh))
    return out


def counters(rows):
    tot, disp = {}, set()
    for r in rows:
        if "k_rollout_queue" in r["Kernel_Name"]:
            tot[r["Counter_Name"]] = tot.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            disp.add(r.get("Dispatch_Id"))
    print(json.dumps({"k_rollout_queue_dispatches": len(disp), "sums": tot}, indent=1))


def main():
    d = sys.argv[1]
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dry_ms = float(sys.argv[3]) if len(sys.argv) > 3 else 8.2
    pmc = read(d, "*counter_collection.csv")
    if pmc:
        return counters(pmc)
    roll = []
    for r in read(d, "*kernel_trace.csv"):
        if "k_rollout_queue" in r["Kernel_Name"]:
            wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 64)
            roll.append({"q": (r.get("Agent_Id"), r.get("Queue_Id")), "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"]),
                         "waves": int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) // max(wg, 1)})
    if not roll:
        raise SystemExit("no k_rollout_queue dispatch under %s" % d)
    roll.sort(key=lambda r: r["t0"])
    big = max(r["waves"] for r in roll)
    first = [r for r in roll if 2 * r["waves"] > big]
    sel = first[-last:]
    origin = sel[0]["t0"]
    ms = lambda t: round((t - origin) / 1e6, 3)
    launches = []
    for r in sel:
        nxt = [p for p in first if p["q"] == r["q"] and p["t0"] > r["t0"]]
        follow = [p for p in roll if p["q"] == r["q"] and 2 * p["waves"] <= big and p["t0"] >= r["t0"] and (not nxt or p["t0"] < nxt[0]["t0"])]
        other = [p for p in first if p["q"] != r["q"] and p["t0"] < r["t0"]]
        e = {"queue": "%s/%s" % r["q"], "waves": r["waves"], "start": ms(r["t0"]), "end": ms(r["t1"]), "first_dispatch_ms": round((r["t1"] - r["t0"]) / 1e6, 3),
             "follow_up_waves": follow[0]["waves"] if follow else None, "follow_up_start": ms(follow[0]["t0"]) if follow else None,
             "follow_up_ms": round((follow[0]["t1"] - follow[0]["t0"]) / 1e6, 3) if follow else None,
             "launch_ms": round(((follow[0]["t1"] if follow else r["t1"]) - r["t0"]) / 1e6, 3)}
        if other:
            o = other[-1]
            e["start_minus_other_first_dispatch_end_ms"] = round((r["t0"] - o["t1"]) / 1e6, 3)
            e["start_minus_other_dry_est_ms"] = round((r["t0"] - o["t0"]) / 1e6 - dry_ms, 3)
        launches.append(e)
    starts = [e["start"] for e in launches]
    med = lambda xs: sorted(xs)[len(xs) // 2] if xs else None
    print(json.dumps({"launches": launches, "period_ms": round((starts[-1] - starts[0]) / max(len(starts) - 1, 1), 3),
                      "median_first_dispatch_ms": med([e["first_dispatch_ms"] for e in launches]),
                      "median_follow_up_ms": med([e["follow_up_ms"] for e in launches if e["follow_up_ms"] is not None]),
                      "median_launch_ms": med([e["launch_ms"] for e in launches]),
                      "median_start_minus_other_dry_est_ms": med([e["start_minus_other_dry_est_ms"] for e in launches if "start_minus_other_dry_est_ms" in e]),
                      "dry_ms_assumed": dry_ms}, indent=1))


if __name__ == "__main__":
    main()
