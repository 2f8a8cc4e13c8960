"""`.battle.data` training frames (host side): reader / writer over the C ABI and the GPU self-play game loop.

Mirrors Train::Battle::CompressedFrames (cpp/include/train/battle/compressed-frame.h:37-243) and the per-game loop of
the reference's data generator (cpp/src/generate.cc:238-322); the (de)serialisation and the loop themselves are C++
(oak_amd/csrc/selfplay.hip) -- this module only marshals arrays."""
import ctypes as C

import numpy as np

from . import _lib


def read_frames(data):
    """Parse a `.battle.data` byte string (a concatenation of game records).  Returns a list of games:
    {"battle": uint8[384], "result": int, "updates": [{"m", "n", "c1", "c2", "iterations", "empirical_value",
    "nash_value", "p1_empirical", "p1_nash", "p2_empirical", "p2_nash"}, ...]}."""
    lib = _lib.load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    games, pos = [], 0
    while pos < buf.size:
        battle = np.zeros(384, dtype=np.uint8)
        result, count, used = C.c_uint8(0), C.c_uint32(0), C.c_size_t(0)
        p = buf[pos:].ctypes.data_as(C.c_void_p)
        _lib.check(lib.oakgpu_frames_read(p, buf.size - pos, None, None, None, 0, C.byref(count), C.byref(used)))   # count first
        ups = (_lib.FrameUpdate * max(count.value, 1))()
        _lib.check(lib.oakgpu_frames_read(p, buf.size - pos, battle.ctypes.data_as(C.c_void_p), C.byref(result), ups, count.value,
                                          C.byref(count), C.byref(used)))
        games.append({"battle": battle, "result": int(result.value), "updates": [
            {"m": u.m, "n": u.n, "c1": u.c1, "c2": u.c2, "iterations": u.iterations, "empirical_value": u.empirical_value,
             "nash_value": u.nash_value, "p1_empirical": np.array(u.p1_empirical[:u.m]), "p1_nash": np.array(u.p1_nash[:u.m]),
             "p2_empirical": np.array(u.p2_empirical[:u.n]), "p2_nash": np.array(u.p2_nash[:u.n])} for u in ups[:count.value]]})
        pos += used.value
    return games


def write_frames(battle, result, updates):
    """One game record (bytes) from the first battle (after the opening update), the final result byte and a list of
    update dicts shaped like read_frames' (probability arrays of length m / n)."""
    lib = _lib.load()
    ups = (_lib.FrameUpdate * max(len(updates), 1))()
    for k, u in enumerate(updates):
        ups[k].m, ups[k].n, ups[k].c1, ups[k].c2 = int(u["m"]), int(u["n"]), int(u["c1"]), int(u["c2"])
        ups[k].iterations = int(u["iterations"])
        ups[k].empirical_value, ups[k].nash_value = float(u["empirical_value"]), float(u["nash_value"])
        for name in ("p1_empirical", "p1_nash", "p2_empirical", "p2_nash"):
            arr = getattr(ups[k], name)
            for i, x in enumerate(u[name]):
                arr[i] = float(x)
    size = lib.oakgpu_frames_size(ups, len(updates))
    out = np.zeros(size, dtype=np.uint8)
    written = C.c_size_t(0)
    b = np.ascontiguousarray(battle, dtype=np.uint8).reshape(384)
    _lib.check(lib.oakgpu_frames_write(b.ctypes.data_as(C.c_void_p), int(result), ups, len(updates), out.ctypes.data_as(C.c_void_p), size,
                                       C.byref(written)))
    return out[:written.value].tobytes()


def selfplay_game(ctx, teams, battle_seed, iterations=1 << 12, batch=1024, bandit="ucb", c=2.0, evaluator="mc", policy_mode="e",
                  policy_temp=1.0, policy_min=0.0, max_battle_length=0, seed=1, alpha=0.05, root_rolls=3, other_rolls=1, keep_node=False,
                  stats=None):
    """One self-play game on the GPU path (oakgpu_selfplay_game).  teams: uint8[2, 6, 5] (species + 4 moves per set).
    keep_node: generate's --keep-node (one heap for the game, Heap::update after every turn); stats: optional dict that
    receives "nodes_kept".  Returns (record bytes, number of frames, final result byte)."""
    use_net = not isinstance(evaluator, str)
    prm = _lib.SelfplayParams()
    prm.search = _lib.SearchParams(iterations=int(iterations), batch=int(batch), ucb_c=float(c),
                                   bandit={"ucb": 0, "pucb": 1, "ucb1": 2, "exp3": 3, "pexp3": 4}[bandit],
                                   eval=1 if use_net else {"mc": 0, "poke-engine": 2}[evaluator], max_depth=0, root_rolls=int(root_rolls),
                                   other_rolls=int(other_rolls), seed=0, matrix_ucb=0, mucb_delay=0, mucb_minimum=0, mucb_c=0.0,
                                   exp3_alpha=float(alpha))
    prm.policy_mode = policy_mode.encode()
    prm.policy_temp, prm.policy_min = float(policy_temp), float(policy_min)
    prm.max_battle_length, prm.seed = int(max_battle_length), int(seed)
    prm.keep_node = 1 if keep_node else 0
    t = np.ascontiguousarray(teams, dtype=np.uint8).reshape(60)
    cap = 4 + 2 + 384 + 1 + 83 * (int(max_battle_length) or 2048)
    out = np.zeros(cap, dtype=np.uint8)
    written, frames, result = C.c_size_t(0), C.c_uint32(0), C.c_uint8(0)
    _lib.check(ctx.lib.oakgpu_selfplay_game(ctx.handle, evaluator.handle if use_net else None, t.ctypes.data_as(C.c_void_p), int(battle_seed),
                                            C.byref(prm), out.ctypes.data_as(C.c_void_p), cap, C.byref(written), C.byref(frames), C.byref(result)))
    if stats is not None:
        stats["nodes_kept"] = int(prm.nodes_kept)
    return out[:written.value].tobytes(), int(frames.value), int(result.value)


def selfplay_games(ctxs, teams, battle_seeds, seeds, iterations=1 << 12, batch=1024, bandit="ucb", c=2.0, evaluator="mc", policy_mode="e",
                   policy_temp=1.0, policy_min=0.0, max_battle_length=0, alpha=0.05, root_rolls=3, other_rolls=1, keep_node=False,
                   threads_per_game=0):
    """n self-play games at once on one GPU (oakgpu_selfplay_games): game g on ctxs[g] with teams[g] (uint8[n, 2, 6, 5]), battle_seeds[g]
    and policy seed seeds[g].  Returns a list of (record bytes, number of frames, final result byte) -- each what selfplay_game(ctxs[g],
    teams[g], battle_seeds[g], seed=seeds[g], ...) returns alone."""
    n = len(ctxs)
    use_net = not isinstance(evaluator, str)
    prms = (_lib.SelfplayParams * n)()
    for g in range(n):
        prms[g].search = _lib.SearchParams(iterations=int(iterations), batch=int(batch), ucb_c=float(c),
                                           bandit={"ucb": 0, "pucb": 1, "ucb1": 2, "exp3": 3, "pexp3": 4}[bandit],
                                           eval=1 if use_net else {"mc": 0, "poke-engine": 2}[evaluator], max_depth=0, root_rolls=int(root_rolls),
                                           other_rolls=int(other_rolls), seed=0, matrix_ucb=0, mucb_delay=0, mucb_minimum=0, mucb_c=0.0,
                                           exp3_alpha=float(alpha))
        prms[g].policy_mode = policy_mode.encode()
        prms[g].policy_temp, prms[g].policy_min = float(policy_temp), float(policy_min)
        prms[g].max_battle_length, prms[g].seed = int(max_battle_length), int(seeds[g])
        prms[g].keep_node = 1 if keep_node else 0
    t = np.ascontiguousarray(teams, dtype=np.uint8).reshape(n, 60)
    bs = (C.c_uint64 * n)(*[int(x) for x in battle_seeds])
    cap = 4 + 2 + 384 + 1 + 83 * (int(max_battle_length) or 2048)
    out = np.zeros((n, cap), dtype=np.uint8)
    written, frames, result = (C.c_size_t * n)(), (C.c_uint32 * n)(), (C.c_uint8 * n)()
    cp = (C.c_void_p * n)(*[c_.handle for c_ in ctxs])
    _lib.check(ctxs[0].lib.oakgpu_selfplay_games(cp, evaluator.handle if use_net else None, t.ctypes.data_as(C.c_void_p), bs, prms, n, int(threads_per_game),
                                                 out.ctypes.data_as(C.c_void_p), cap, written, frames, result))
    return [(out[g, :written[g]].tobytes(), int(frames[g]), int(result[g])) for g in range(n)]


# ---- replay check of `.battle.data` records on the GPU (oakgpu_replay_records; the rules are in include/oakgpu.h) ----------------
REPLAY_STATUS = ("OK", "COUNT", "ILLEGAL", "EARLY_END", "RESULT", "MALFORMED")
REPORT_DTYPE = np.dtype([("status", np.uint8), ("player", np.uint8), ("frame", np.uint32), ("expected", np.uint8), ("got", np.uint8),
                         ("offset", np.uint64)])
_RAW_REPORT = np.dtype([("frame", "<u4"), ("status", "u1"), ("player", "u1"), ("expected", "u1"), ("got", "u1")])   # oakgpu_replay_report


def replay_index(data):
    """Record boundaries of a `.battle.data` byte string and oakgpu_frames_read's validation of each record.  Returns
    {"offsets": uint64[n], "frames": uint16[n], "malformed": bool[n], "stopped_at": int}; indexing stops at the first record whose
    length field cannot be trusted (stopped_at = len(data) when it does not)."""
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    n, stop = C.c_uint32(0), C.c_size_t(0)
    p = buf.ctypes.data_as(C.c_void_p)
    _lib.check(lib.oakgpu_replay_index(p, len(data), None, None, None, 0, C.byref(n), C.byref(stop)))
    offs, fr, mal = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint16), np.zeros(max(n.value, 1), np.uint8)
    if n.value:
        _lib.check(lib.oakgpu_replay_index(p, len(data), offs.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p),
                                           mal.ctypes.data_as(C.c_void_p), n.value, C.byref(n), None))
    k = n.value
    return {"offsets": offs[:k], "frames": fr[:k], "malformed": mal[:k].astype(bool), "stopped_at": int(stop.value)}


def replay_check(ctx, data, want_states=False):
    """Replay every record of a `.battle.data` byte string on the GPU through its stored choices.  Returns {"reports": structured
    array (status, player, frame, expected, got, offset) per record, "stopped_at": int, "battles": uint8[n, 384] and "durations":
    uint8[n, 8] at each verdict (want_states) or None}."""
    lib = ctx.lib
    idx = replay_index(data)
    n = len(idx["offsets"])
    reports = np.zeros(n, dtype=REPORT_DTYPE)
    battles = np.zeros((n, 384), np.uint8) if want_states else None
    durations = np.zeros((n, 8), np.uint8) if want_states else None
    if n:
        buf = np.frombuffer(data, dtype=np.uint8)
        raw = np.zeros(n, dtype=_RAW_REPORT)
        got, stop = C.c_uint32(0), C.c_size_t(0)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(lib.oakgpu_replay_records(ctx.handle, vp(buf), len(data), vp(raw), n, C.byref(got), C.byref(stop), vp(battles), vp(durations)))
        assert got.value == n and stop.value == idx["stopped_at"]
        for f in ("status", "player", "frame", "expected", "got"):
            reports[f] = raw[f]
        reports["offset"] = idx["offsets"]
    return {"reports": reports, "stopped_at": idx["stopped_at"], "battles": battles, "durations": durations}


def engine_switches():
    """The compile-time engine switches of the loaded library (DESIGN 0 order): MULTIHIT_ROLL_FIRST, PSYWAVE_SHOWDOWN, COUNTER_SHOWDOWN,
    ACCURACY_LAST."""
    lib = _lib.load()
    out = (C.c_int * 4)()
    _lib.check(lib.oakgpu_engine_switches(C.byref(out)))
    return {"MULTIHIT_ROLL_FIRST": out[0], "PSYWAVE_SHOWDOWN": out[1], "COUNTER_SHOWDOWN": out[2], "ACCURACY_LAST": out[3]}


def _whole_records(f, chunk_bytes):
    """Yield (file offset, bytes) pieces of an open `.battle.data` file, each ending on a record boundary, of about chunk_bytes
    (more when one record is longer), then (stop offset or None, b"")."""
    import struct
    f.seek(0, 2)
    size = f.tell()
    f.seek(0)
    base, carry = 0, b""
    while True:
        fresh = f.read(max(chunk_bytes - len(carry), 1 << 16))
        buf = carry + fresh
        at_eof = f.tell() >= size
        if not buf:
            yield None, b""
            return
        idx = replay_index(buf)
        s = idx["stopped_at"]
        if s == len(buf):
            yield base, buf
            base, carry = base + s, b""
            if at_eof:
                yield None, b""
                return
            continue
        # indexing stopped inside this piece: a chunk boundary (read on) or a record whose length cannot be trusted (stop)
        rest, left = len(buf) - s, size - f.tell()
        true_stop = at_eof
        if not at_eof and rest >= 6:
            total = struct.unpack_from("<I", buf, s)[0]
            true_stop = total < 391 or total > rest + left
        if s:
            yield base, buf[:s]
        if true_stop:
            yield base + s, b""
            return
        base, carry = base + s, buf[s:]


def replay_check_files(ctx, paths, chunk_bytes=64 << 20, want_states=False):
    """Replay every record of many `.battle.data` files: small files are packed into one launch up to chunk_bytes, large ones read
    in pieces that end on record boundaries (a record is never split between launches).  Returns {"reports": structured array with
    a "file" field (index into paths) beside replay_check's fields, "offset" = byte offset in that file; "files": [{"path", "size",
    "records", "stopped_at" (None when the whole file was indexed)}]; "battles" / "durations" as replay_check}."""
    import os
    dtype = np.dtype(REPORT_DTYPE.descr + [("file", np.uint32)])
    out, states, files = [], [], []
    pend, pend_map = [], []   # pieces waiting for a launch, (file, file offset, offset in the launch buffer)

    def flush():
        if not pend:
            return
        blob = b"".join(pend)
        res = replay_check(ctx, blob, want_states)
        rep = res["reports"]
        starts = np.array([m[2] for m in pend_map], dtype=np.uint64)
        seg = np.searchsorted(starts, rep["offset"], side="right") - 1
        r = np.zeros(len(rep), dtype=dtype)
        for name in REPORT_DTYPE.names:
            r[name] = rep[name]
        r["file"] = np.array([pend_map[s][0] for s in seg], dtype=np.uint32)
        r["offset"] = rep["offset"] - starts[seg] + np.array([pend_map[s][1] for s in seg], dtype=np.uint64)
        out.append(r)
        if want_states:
            states.append((res["battles"], res["durations"]))
        pend.clear()
        pend_map.clear()

    for fi, path in enumerate(paths):
        info = {"path": str(path), "size": os.path.getsize(path), "records": 0, "stopped_at": None}
        with open(path, "rb") as f:
            for off, piece in _whole_records(f, chunk_bytes):
                if not piece:
                    info["stopped_at"] = off
                    continue
                if pend and sum(len(p) for p in pend) + len(piece) > chunk_bytes:
                    flush()
                pend_map.append((fi, off, sum(len(p) for p in pend)))
                pend.append(piece)
                info["records"] += len(replay_index(piece)["offsets"])
        files.append(info)
    flush()
    reports = np.concatenate(out) if out else np.zeros(0, dtype=dtype)
    res = {"reports": reports, "files": files, "battles": None, "durations": None}
    if want_states:
        res["battles"] = np.concatenate([s[0] for s in states]) if states else np.zeros((0, 384), np.uint8)
        res["durations"] = np.concatenate([s[1] for s in states]) if states else np.zeros((0, 8), np.uint8)
    return res
