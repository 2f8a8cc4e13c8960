#!/usr/bin/env python3
"""Timeline of back-to-back group launches on two streams, from a kernel trace of
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --workload rollout --no-cpu-baseline`.

  python tools/launch_overlap.py DIR [LAUNCHES]     (prints one JSON object)

For each of the last LAUNCHES (default 8: the timed region of the default command) dispatches of k_rollout_queue: on the
launch's own hardware queue, the end of the previous rollout -> the start of the caller's reduce -> the start of the first
fill kernel and of k_queue_order -> the start of this rollout; and the rollout that runs on the OTHER queue meanwhile, with
the moment its playout queue runs dry (not in a kernel trace: start + DRY_MS, the wave timeline of profiles/r13_drain.json).
Times are milliseconds from the start of the first listed rollout."""
import csv
import glob
import json
import os
import sys

DRY_MS = 10.1   # profiles/r13_drain.json, final_timeline: the queue is dry 10.09-10.15 ms into a 20-batch launch


def rows(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % d)
    out = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                # (the hardware queue tells the two contexts' streams apart; the trace's Stream_Id is the same for both)
                out.append({"name": r["Kernel_Name"], "q": (r.get("Agent_Id"), r.get("Queue_Id")), "stream": r.get("Stream_Id"),
                            "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"]),
                            "wg": int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 0), "grid": int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)})
    out.sort(key=lambda r: r["t0"])
    return out


def kind(name):
    if "k_rollout_queue" in name:
        return "rollout"
    if "k_queue_order" in name or "k_clear_launch_words" in name:
        return "queue_order"
    if "fillBuffer" in name or "FillBuffer" in name:
        return "fill"
    if "reduce" in name.lower():
        return "reduce"
    if "at::native" in name:
        return "torch_elementwise"   # the caller's cast in front of its reduction and the add behind it
    if "copyBuffer" in name or "CopyBuffer" in name:
        return "copy"
    return "other"


def main():
    d = sys.argv[1]
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    ks = rows(d)
    roll = [r for r in ks if kind(r["name"]) == "rollout"]
    sel = roll[-last:]
    origin = sel[0]["t0"]
    ms = lambda t: round((t - origin) / 1e6, 3)
    launches = []
    for r in sel:
        prev = [p for p in roll if p["q"] == r["q"] and p["t1"] <= r["t0"]]
        prev = prev[-1] if prev else None
        between = [k for k in ks if k["q"] == r["q"] and prev is not None and prev["t1"] <= k["t0"] < r["t0"] and k is not prev]
        first = lambda what: next((ms(k["t0"]) for k in between if kind(k["name"]) == what), None)
        other = [p for p in roll if p["q"] != r["q"] and p["t0"] < r["t0"] and p["t1"] > (prev["t1"] if prev else r["t0"])]
        other = other[-1] if other else None
        e = {"queue": "%s/%s" % r["q"], "stream": r["stream"], "waves": r["grid"] // max(r["wg"], 1) if r["wg"] else None,
             "prev_rollout_end": ms(prev["t1"]) if prev else None, "reduce_start": first("reduce"), "first_fill_start": first("fill"),
             "queue_order_start": first("queue_order"), "rollout_start": ms(r["t0"]), "rollout_end": ms(r["t1"]),
             "rollout_ms": round((r["t1"] - r["t0"]) / 1e6, 3),
             "idle_before_rollout_ms": round((r["t0"] - prev["t1"]) / 1e6, 3) if prev else None,
             "small_kernels_between": ["%s/%d @%.3f %.1fus" % (kind(k["name"]), k["wg"], ms(k["t0"]), (k["t1"] - k["t0"]) / 1e3) for k in between]}   # kind/block @start duration
        if other:
            e["other_rollout_start"] = ms(other["t0"])
            e["other_queue_dry_est"] = round(ms(other["t0"]) + DRY_MS, 3)
            e["other_rollout_end"] = ms(other["t1"])
            e["rollout_start_minus_other_dry_ms"] = round(e["rollout_start"] - e["other_queue_dry_est"], 3)
        launches.append(e)
    starts = [e["rollout_start"] for e in launches]
    period = round((launches[-1]["rollout_end"] - launches[0]["rollout_start"]) / len(launches), 3)
    print(json.dumps({"launches": launches, "rollout_starts": starts, "span_per_launch_ms": period, "dry_ms_assumed": DRY_MS,
                      "dry_note": "other_queue_dry_est is NOT measured: a kernel trace does not show it; it is the other rollout's start + dry_ms_assumed"}, indent=1))


if __name__ == "__main__":
    main()
