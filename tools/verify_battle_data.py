"""Check `.battle.data` files against this engine: every game is replayed on the GPU from its stored battle through its stored
choices (the reference's frames.h:52-67 self-check, for a whole corpus; the rules are in include/oakgpu.h).

  python tools/verify_battle_data.py PATH... [--chunk-mb N] [--json OUT] [--show K] [--extract DIR] [--oracle K] [--index-only]

PATH: files, or directories whose `*.battle.data` files (recursively, sorted) are read.  Prints one JSON summary.  Exit status 0 when
every record is OK, 1 on any failure (a MALFORMED record or a stopped file included), 2 on unreadable input.
  --extract DIR   every failing record, unchanged, into DIR/failures.battle.data, with one JSON line per record in DIR/failures.jsonl
  --oracle K      replay every failing record and a seeded sample of K passing ones on the CPU oracle (tests/replay_oracle.py, honours
                  ORACLE_SO) and report whether it agrees with the GPU on status, frame and the state at the verdict
  --index-only    no GPU: records, frame counts, MALFORMED records and stop offsets"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _paths(args):
    out = []
    for p in args:
        if os.path.isdir(p):
            found = []
            for d, _, files in os.walk(p):
                found += [os.path.join(d, f) for f in files if f.endswith(".battle.data")]
            out += sorted(found)
        elif os.path.isfile(p):
            out.append(p)
        else:
            raise FileNotFoundError(p)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--chunk-mb", type=float, default=256)
    ap.add_argument("--json")
    ap.add_argument("--show", type=int, default=20)
    ap.add_argument("--extract")
    ap.add_argument("--oracle", type=int, default=-1)
    ap.add_argument("--index-only", action="store_true")
    a = ap.parse_args(argv)
    import numpy as np
    from oak_amd import _lib
    from oak_amd.frames import REPLAY_STATUS, engine_switches, replay_check_files, replay_index
    try:
        paths = _paths(a.paths)
        for p in paths:
            with open(p, "rb"):
                pass
    except OSError as e:
        print(json.dumps({"error": "unreadable input: %s" % e}))
        return 2
    t0 = time.perf_counter()
    summary = {"library": _lib.LIB_PATH, "engine_switches": engine_switches(), "files": len(paths)}
    if a.index_only:
        records = frames = 0
        malformed, stopped = [], []
        for p in paths:
            data = open(p, "rb").read()
            idx = replay_index(data)
            records += len(idx["offsets"])
            frames += int(idx["frames"].astype(np.int64).sum())
            malformed += [{"file": p, "offset": int(o)} for o in idx["offsets"][idx["malformed"]]]
            if idx["stopped_at"] != len(data):
                stopped.append({"file": p, "offset": idx["stopped_at"]})
        summary.update(records=records, frames=frames, malformed=malformed, stopped=stopped, wall_s=time.perf_counter() - t0)
        fail = bool(malformed or stopped)
    else:
        from oak_amd.engine import Context
        ctx = Context(0)
        want = a.oracle >= 0
        res = replay_check_files(ctx, paths, chunk_bytes=int(a.chunk_mb * (1 << 20)), want_states=want)
        wall = time.perf_counter() - t0
        rep = res["reports"]
        frames_played = int(rep["frame"].astype(np.int64).sum())
        counts = {s: int((rep["status"] == i).sum()) for i, s in enumerate(REPLAY_STATUS)}
        bad = np.nonzero(rep["status"] != 0)[0]
        row = lambda i: {"file": paths[rep["file"][i]], "offset": int(rep["offset"][i]), "frame": int(rep["frame"][i]),
                         "status": REPLAY_STATUS[rep["status"][i]], "player": int(rep["player"][i]), "expected": int(rep["expected"][i]),
                         "got": int(rep["got"][i])}
        stopped = [{"file": f["path"], "offset": f["stopped_at"]} for f in res["files"] if f["stopped_at"] is not None]
        summary.update(records=int(len(rep)), frames=frames_played, counts=counts,
                       malformed=[{"file": paths[rep["file"][i]], "offset": int(rep["offset"][i])} for i in bad if rep["status"][i] == 5],
                       stopped=stopped, failures=[row(i) for i in bad[:a.show]], wall_s=wall,
                       frames_per_s=frames_played / wall if wall > 0 else None)
        fail = bool(len(bad) or stopped)

        def record_bytes(i):
            with open(paths[rep["file"][i]], "rb") as f:
                f.seek(int(rep["offset"][i]))
                head = f.read(4)
                return head + f.read(int.from_bytes(head, "little") - 4)
        if a.extract:
            os.makedirs(a.extract, exist_ok=True)
            with open(os.path.join(a.extract, "failures.battle.data"), "wb") as out, open(os.path.join(a.extract, "failures.jsonl"), "w") as js:
                for i in bad:
                    out.write(record_bytes(i))
                    js.write(json.dumps(row(i)) + "\n")
            summary["extracted"] = {"dir": a.extract, "records": int(len(bad))}
        if want:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import replay_oracle as RO
            good = np.nonzero(rep["status"] == 0)[0]
            sample = np.random.default_rng(0).choice(good, size=min(a.oracle, len(good)), replace=False) if len(good) else good
            checked, disagree = 0, []
            for i in sorted(set(bad.tolist()) | set(sample.tolist())):
                st, pl, fr, ex, got, b, d = RO.replay(record_bytes(i))
                same = (st, pl, fr, ex, got) == (rep["status"][i], rep["player"][i], rep["frame"][i], rep["expected"][i], rep["got"][i])
                same = same and (b == res["battles"][i]).all() and (d == res["durations"][i]).all()
                checked += 1
                if not same:
                    disagree.append(row(i))
            summary["oracle"] = {"checked": checked, "agree": checked - len(disagree), "disagree": disagree[:a.show]}
            fail = fail or bool(disagree)
    text = json.dumps(summary, indent=1)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")
    print(text)
    return 1 if fail else 0


if __name__ == "__main__":
    sys.exit(main())
