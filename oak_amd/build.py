"""Team building on the GPU: the build network's rollout, the provider of `generate`, and `.build.data` records.

Mirrors TeamBuilding::Provider::get_trajectory / rollout_build_network (cpp/include/util/team-building.h:36-84, 190-241) and
Encode::Build::CompressedTrajectory (encode/build/compressed-trajectory.h); the rollout, the provider's prelude and the record packer are
HIP (oak_amd/csrc/buildnet.hip, contract in include/oakgpu.h) -- this module only marshals arrays.  numpy arrays in give numpy arrays
out; torch GPU tensors in give tensors on that device out and copy nothing to the host (seeds as int64 bit patterns, the u16 outputs
as int16: every value is below 3,749)."""
import ctypes as C

import numpy as np

from . import _lib

N_DIM, MAX_ACTIONS, MAX_STEPS, RECORD_BYTES = 3749, 339, 31, 128
_STEP_ARRAYS = (("action", np.uint16), ("index", np.uint16), ("n_legal", np.uint16), ("prob", np.float32))
_TRACE_ARRAYS = (("trace_legal", np.int16), ("trace_logits", np.float32), ("trace_policy", np.float32))


def tables():
    """(legal_species uint8[149], species_move_list uint8[3749, 2], species_move_table int32[152, 166], -1 where there is no cell)."""
    legal, cells, table = np.zeros(149, np.uint8), np.zeros((N_DIM, 2), np.uint8), np.zeros((152, 166), np.int32)
    _lib.check(_lib.load().oakgpu_build_tables(legal.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p), table.ctypes.data_as(C.c_void_p)))
    return legal, cells, table


def check_net(data):
    """The refusals of a `.build.net`, by name, without a GPU."""
    buf = np.frombuffer(bytes(data), np.uint8)
    _lib.check(_lib.load().oakgpu_build_net_check(buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size))


def check_teams(teams, sizes=None, input_update=0):
    """The refusals of rollout's teams, by name, without a GPU."""
    t = np.ascontiguousarray(teams, np.uint8).reshape(-1, 30)
    s = None if sizes is None else np.ascontiguousarray(sizes, np.uint8).reshape(-1)
    _lib.check(_lib.load().oakgpu_build_teams_check(t.ctypes.data_as(C.c_void_p) if t.size else None, None if s is None else s.ctypes.data_as(C.c_void_p),
                                                    t.shape[0], int(input_update)))


def check_provide(pool, n, max_pokemon=6, pokemon_delete_prob=0., move_delete_prob=0., team_modify_prob=0.):
    """The refusals of provide, by name, without a GPU."""
    p = np.ascontiguousarray(pool, np.uint8).reshape(-1, 30)
    _lib.check(_lib.load().oakgpu_build_provide_check(p.ctypes.data_as(C.c_void_p) if p.size else None, p.shape[0], int(n), int(max_pokemon),
                                                      float(pokemon_delete_prob), float(move_delete_prob), float(team_modify_prob)))


class BuildNetwork:
    """A `.build.net` resident on the context's device; close() (or the context manager) frees it before the context goes."""

    def __init__(self, ctx, bytes_or_path):
        data = bytes_or_path if isinstance(bytes_or_path, (bytes, bytearray, memoryview)) else open(bytes_or_path, "rb").read()
        buf = np.frombuffer(bytes(data), np.uint8)
        self.ctx, self.handle = ctx, C.c_void_p()
        _lib.check(ctx.lib.oakgpu_build_net_load(ctx.handle, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, C.byref(self.handle)))
        p, v = C.c_uint32(0), C.c_uint32(0)
        _lib.check(ctx.lib.oakgpu_build_net_shape(self.handle, C.byref(p), C.byref(v)))
        self.policy_hidden, self.value_hidden = int(p.value), int(v.value)

    def close(self):
        if self.handle:
            self.ctx.lib.oakgpu_build_net_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _alloc(n, trace, provide, device):
    """The output arrays of one call, cleared (the legal trace to -1): numpy, or torch tensors on `device`."""
    shapes = [("teams_out", (n, 30), np.uint8), ("n_updates", (n,), np.uint8)] + [(k, (n, MAX_STEPS), t) for k, t in _STEP_ARRAYS]
    if trace:
        shapes += [(k, (n, MAX_STEPS, MAX_ACTIONS), t) for k, t in _TRACE_ARRAYS]
    if provide:
        shapes += [("teams_init", (n, 30), np.uint8), ("sizes", (n,), np.uint8), ("team_index", (n,), np.int32)]
    out = {}
    for name, shape, dtype in shapes:
        fill = -1 if name == "trace_legal" else 0
        if device is None:
            out[name] = np.full(shape, fill, dtype)
        else:
            import torch
            tdt = {np.uint8: torch.uint8, np.uint16: torch.int16, np.int16: torch.int16, np.float32: torch.float32, np.int32: torch.int32}[dtype]
            out[name] = torch.full(shape, fill, dtype=tdt, device=device)
    return out


def _pointers(out, ptr):
    o = _lib.BuildOutputs()
    fields = set(f[0] for f in _lib.BuildOutputs._fields_)
    for name in out:
        field = "sizes_out" if name == "sizes" else name
        if field in fields and name != "teams_in":
            setattr(o, field, ptr(out[name]))
    return o


def _run(ctx, on_device, device, inputs, call_dev, call_host, out):
    if on_device:
        import torch
        mine, theirs = torch.cuda.ExternalStream(ctx.stream_ptr(), device=device), torch.cuda.current_stream(device)
        mine.wait_stream(theirs)
        _lib.check(call_dev(*[None if x is None else x.data_ptr() for x in inputs], _pointers(out, lambda a: a.data_ptr())))
        theirs.wait_stream(mine)
    else:
        _lib.check(call_host(*[None if x is None else x.ctypes.data_as(C.c_void_p) for x in inputs], _pointers(out, lambda a: a.ctypes.data_as(C.c_void_p))))
    return out


def rollout(ctx, net, teams, seeds, sizes=None, input_update=0, trace=False, out=None):
    """Complete every team with the build network: one launch (oakgpu_build_rollout).  teams uint8[n, 30] (6 x {species, 4 moves}), seeds
    uint64[n], sizes uint8[n] or None (6).  Returns a dict: teams_out [n, 30], n_updates [n], and per step [n, 31] action (the cell), index
    (the position in the legal list), n_legal, prob; with trace=True also trace_legal (-1 padded), trace_logits, trace_policy [n, 31, 339].
    Entries at or past a row's n_updates / a step's n_legal are left as they were (zeros here).  out: the same dict preallocated by the
    caller (a test's prefilled arrays)."""
    on_device = hasattr(teams, "data_ptr")
    if on_device:
        n, device = int(teams.shape[0]), teams.device
        t, sd, sz = teams.contiguous().view(n, 30), seeds.contiguous(), None if sizes is None else sizes.contiguous()
    else:
        t = np.ascontiguousarray(teams, np.uint8).reshape(-1, 30)
        n, device = t.shape[0], None
        sd = np.ascontiguousarray(np.asarray(seeds).astype(np.uint64)).reshape(n)
        sz = None if sizes is None else np.ascontiguousarray(sizes, np.uint8).reshape(n)
    out = _alloc(n, trace, False, device) if out is None else out
    lib, iu = ctx.lib, int(input_update)
    out.pop("sizes", None)
    _run(ctx, on_device, device, (t, sz, sd),
         lambda a, b, c, o: lib.oakgpu_build_rollout_dev(ctx.handle, net.handle, a, b, c, n, iu, C.byref(o)),
         lambda a, b, c, o: lib.oakgpu_build_rollout(ctx.handle, net.handle, a, b, c, n, iu, C.byref(o)), out)
    out["teams_in"] = t      # what records() starts from
    if sz is not None:
        out["sizes"] = sz
    return out


def provide(ctx, net, pool, seeds, max_pokemon=6, pokemon_delete_prob=0., move_delete_prob=0., team_modify_prob=0., input_update=0, trace=False):
    """Provider::get_trajectory for len(seeds) rows over a pool of teams (uint8[T, 30]): rollout's dict plus teams_init [n, 30] and sizes [n]
    (the team before the rollout, what a record starts from) and team_index int32[n] (-1 for built rows)."""
    on_device = hasattr(pool, "data_ptr")
    if on_device:
        device = pool.device
        p, sd = pool.contiguous().view(-1, 30), seeds.contiguous()
        n = int(sd.shape[0])
    else:
        p, device = np.ascontiguousarray(pool, np.uint8).reshape(-1, 30), None
        sd = np.ascontiguousarray(np.asarray(seeds).astype(np.uint64)).reshape(-1)
        n = sd.shape[0]
    prm = _lib.BuildProvider(int(max_pokemon), int(input_update), float(pokemon_delete_prob), float(move_delete_prob), float(team_modify_prob))
    out = _alloc(n, trace, True, device)
    lib, pool_n = ctx.lib, int(p.shape[0])
    return _run(ctx, on_device, device, (p, sd),
                lambda a, c, o: lib.oakgpu_build_provide_dev(ctx.handle, net.handle, a, pool_n, c, n, C.byref(prm), C.byref(o)),
                lambda a, c, o: lib.oakgpu_build_provide(ctx.handle, net.handle, a, pool_n, c, n, C.byref(prm), C.byref(o)), out)


def _next_seed(seed):
    """One splitmix64 step: a redrawn row's fresh seed."""
    m = (1 << 64) - 1
    z = (int(seed) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def provide_pairs(ctx, net, pool, seeds, max_tries=16, **kw):
    """Both seats' teams of len(seeds) games: seeds uint64[n, 2], one provide call per seat on the device; a pair that fails the endless
    battle check (on the host, as generate.cc:224-227 draws again) gets fresh seeds -- one splitmix64 step of the old ones -- and is
    provided again, before any game starts.  Returns (teams uint8[n, 60], (p1, p2)): provide's dict per seat, numpy; each also holds the
    "seeds" the kept rows were made from."""
    lib = ctx.lib
    seeds = np.array(seeds, np.uint64).reshape(-1, 2)
    n = seeds.shape[0]
    seats = [None, None]
    rows = np.arange(n)
    for _ in range(max_tries):
        for s in (0, 1):
            got = provide(ctx, net, pool, seeds[rows, s], **kw)
            if seats[s] is None:
                seats[s] = got
            else:
                for name in got:
                    seats[s][name][rows] = got[name]
        teams = np.ascontiguousarray(np.concatenate([seats[0]["teams_out"], seats[1]["teams_out"]], axis=1))
        rows = np.array([g for g in rows if lib.oakgpu_endless_battle_check(teams[g].ctypes.data_as(C.c_void_p))], np.int64)
        if not rows.size:
            seats[0]["seeds"], seats[1]["seeds"] = seeds[:, 0].copy(), seeds[:, 1].copy()
            return teams, tuple(seats)
        for g in rows:
            seeds[g] = [_next_seed(seeds[g, 0]), _next_seed(seeds[g, 1])]
    raise _lib.OakGpuError("provide_pairs: %d pairs still fail the endless battle check after %d draws" % (rows.size, max_tries))


def records(ctx, trajectories, value, score):
    """The `.build.data` records of the built rows (n_updates > 0) of a rollout / provide dict, in row order.  value, score: one float per row or
    a scalar; a score that is None, NaN or negative means none.  numpy in: bytes; tensors in: a uint8 tensor."""
    tr = trajectories
    on_device = hasattr(tr["n_updates"], "data_ptr")
    teams = tr["teams_init"] if "teams_init" in tr else tr["teams_in"]
    sizes = tr.get("sizes")
    n = int(tr["n_updates"].shape[0])
    lib = ctx.lib
    if on_device:
        import torch
        device = tr["n_updates"].device

        def per_row(x):
            if x is None:
                x = -1.0
            return x.to(torch.float32).contiguous() if hasattr(x, "data_ptr") else torch.full((n,), float(x), dtype=torch.float32, device=device)
        v, s = per_row(value), per_row(score)
        out, count = torch.zeros((n, RECORD_BYTES), dtype=torch.uint8, device=device), torch.zeros(1, dtype=torch.int32, device=device)
        mine, theirs = torch.cuda.ExternalStream(ctx.stream_ptr(), device=device), torch.cuda.current_stream(device)
        mine.wait_stream(theirs)
        _lib.check(lib.oakgpu_build_records_dev(ctx.handle, teams.data_ptr(), None if sizes is None else sizes.data_ptr(), tr["n_updates"].data_ptr(),
                                                tr["action"].data_ptr(), tr["prob"].data_ptr(), v.data_ptr(), s.data_ptr(), n, out.data_ptr(), count.data_ptr()))
        theirs.wait_stream(mine)
        return out[:int(count.item())].reshape(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    per_row = lambda x: np.ascontiguousarray(np.broadcast_to(np.asarray(-1.0 if x is None else x, np.float32), (n,)))
    v, s = per_row(value), np.nan_to_num(per_row(score), nan=-1.0)
    out, count = np.zeros((n, RECORD_BYTES), np.uint8), C.c_uint32(0)
    t = np.ascontiguousarray(teams, np.uint8).reshape(n, 30)
    _lib.check(lib.oakgpu_build_records(ctx.handle, vp(t), None if sizes is None else vp(np.ascontiguousarray(sizes, np.uint8)), vp(tr["n_updates"]),
                                        vp(np.ascontiguousarray(tr["action"])), vp(np.ascontiguousarray(tr["prob"])), vp(v), vp(s), n, vp(out), C.byref(count)))
    return out[:count.value].tobytes()


def game_targets(status, result, matchup, seat):
    """oakgpu_build_game_targets_host (no GPU): the (value, score) of a seat's record of one self-play game -- seat 0 = p1: value =
    float32(matchup), seat 1: float32(1 - matchup); score from the result byte, None for a skipped game -- or None when a game of this
    status (frames.FSP_STATUS) gives no record."""
    v, s = C.c_float(0), C.c_float(0)
    rc = _lib.load().oakgpu_build_game_targets_host(int(status), int(result), float(matchup), int(seat), C.byref(v), C.byref(s))
    if rc < 0:
        _lib.check(rc)
    return None if rc == 0 else (v.value, None if s.value < 0 else s.value)


def game_records(ctx, seats, status, results, matchup, out=None):
    """Both seats' `.build.data` records of a batch of self-play games, on the device in one launch (oakgpu_build_game_records_dev):
    seats = (p1, p2), provide's dict per seat; status, results, matchup: forest_selfplay's per-game outputs (stats["matchup"]).  A game
    with status OK or SKIPPED gives one record per built seat, game-major, p1 before p2, with game_targets' value and score.  Tensors in:
    returns (records uint8 [2 n, 128], count int32 [1]) -- both stay on the device, count is what BuildWindow.append takes; out: the caller's
    records tensor.  numpy in: staged through torch (which must have initialised the GPU before the library did), returns the records' bytes."""
    import torch
    on_device = hasattr(status, "data_ptr")
    device = status.device if on_device else torch.device("cuda", ctx.device)
    steps = {"action": torch.int16, "prob": torch.float32}

    def dev(x, dtype):
        if hasattr(x, "data_ptr"):
            return x.contiguous()
        a = np.ascontiguousarray(x)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        return torch.from_numpy(a).to(device=device, dtype=dtype)
    n = int(status.shape[0])
    held, arrays = [], []
    for seat in seats:
        t = {"teams_init": dev(seat["teams_init"], torch.uint8), "sizes": dev(seat["sizes"], torch.uint8), "n_updates": dev(seat["n_updates"], torch.uint8),
             "action": dev(seat["action"], steps["action"]), "prob": dev(seat["prob"], steps["prob"])}
        if any(int(t[k].shape[0]) != n for k in t):
            raise ValueError("game_records: every seat array has one row per game")
        held.append(t)
        arrays.append(_lib.BuildSeatArrays(*[t[k].data_ptr() for k in ("teams_init", "sizes", "n_updates", "action", "prob")]))
    st, rs, mu = dev(status, torch.uint8), dev(results, torch.uint8), dev(matchup, torch.float64)
    if int(rs.shape[0]) != n or int(mu.shape[0]) != n or mu.dtype != torch.float64:
        raise ValueError("game_records: status, results uint8[n] and matchup float64[n]")
    records = torch.zeros((2 * n, RECORD_BYTES), dtype=torch.uint8, device=device) if out is None else out
    if records.numel() < 2 * n * RECORD_BYTES or records.dtype != torch.uint8 or not records.is_contiguous():
        raise ValueError("game_records: out holds 2 n x 128 bytes")
    count = torch.zeros(1, dtype=torch.int32, device=device)
    mine, theirs = torch.cuda.ExternalStream(ctx.stream_ptr(), device=device), torch.cuda.current_stream(device)
    mine.wait_stream(theirs)
    _lib.check(ctx.lib.oakgpu_build_game_records_dev(ctx.handle, C.byref(arrays[0]), C.byref(arrays[1]), st.data_ptr(), rs.data_ptr(), mu.data_ptr(), n,
                                                     records.data_ptr(), count.data_ptr()))
    theirs.wait_stream(mine)
    if on_device:
        return records, count
    return records.reshape(-1)[:int(count.item()) * RECORD_BYTES].cpu().numpy().tobytes()


def decode_records(data):
    """`.build.data` bytes (NoTeam records) -> a list of {"score" (None: no score), "value", "action" uint16[31], "probability" uint16[31]}."""
    buf = np.frombuffer(bytes(data), np.uint8)
    if buf.size % RECORD_BYTES:
        raise ValueError("decode_records: %d bytes is not a multiple of %d" % (buf.size, RECORD_BYTES))
    out = []
    for r in buf.reshape(-1, RECORD_BYTES):
        if r[0] != 0:
            raise ValueError("decode_records: a record of format %d (only NoTeam records are read)" % r[0])
        ups = r[4:].view("<u2").reshape(MAX_STEPS, 2)
        out.append({"score": None if r[1] == 255 else r[1] / 2.0, "value": int(r[2:4].view("<u2")[0]) / 65535.0, "action": ups[:, 0].copy(),
                    "probability": ups[:, 1].copy()})
    return out


# ---- reading `.build.data` back: trajectories and the network-free half of process_targets (oak_amd/csrc/buildtraj.hip) -----------------
TRAJ_STATUS = ("OK", "BAD_ACTION", "NO_SPECIES", "TEAM_FULL", "NOT_LEGAL", "LIST_OVERFLOW")
_MASK_DTYPES = {"int64": (0, np.int64), "int16": (1, np.int16)}
_TRAJ_ARRAYS = (("action", (MAX_STEPS,), np.int64), ("mask", (MAX_STEPS, MAX_ACTIONS), None), ("n_legal", (MAX_STEPS,), np.uint16),
                ("policy", (MAX_STEPS,), np.float32), ("value", (), np.float32), ("score", (), np.float32), ("start", (), np.int64),
                ("end", (), np.int64), ("status", (), np.uint8))
_TARGET_ARRAYS = (("valid", (MAX_STEPS,), np.uint8, False), ("rows", (2,), np.uint32, True), ("state_cells", (MAX_STEPS,), np.uint16, True),
                  ("state_n", (), np.uint8, True), ("old_logp", (), np.float32, True), ("rewards", (MAX_STEPS,), np.float32, False))


def _torch_dtype(dtype):
    import torch
    return {np.uint8: torch.uint8, np.uint16: torch.int16, np.int16: torch.int16, np.uint32: torch.int32, np.int64: torch.int64, np.float32: torch.float32}[dtype]


def _empty(shape, dtype, device):
    if device is None:
        return np.empty(shape, dtype)
    import torch
    return torch.empty(shape, dtype=_torch_dtype(dtype), device=device)


def _ptr(a):
    return None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def _on_stream(ctx, device, call):
    """One _dev call on the context's stream, ordered after and before the caller's torch stream."""
    import torch
    mine, theirs = torch.cuda.ExternalStream(ctx.stream_ptr(), device=device), torch.cuda.current_stream(device)
    mine.wait_stream(theirs)
    _lib.check(call())
    theirs.wait_stream(mine)


def check_records(data):
    """The status of every record of `.build.data` bytes (uint8[n], an index into TRAJ_STATUS), without a GPU; refuses by name a length that
    is not a multiple of 128 and a record whose format byte is not 0."""
    buf = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    status = np.zeros(buf.size // RECORD_BYTES, np.uint8)
    _lib.check(_lib.load().oakgpu_build_traj_check(buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, status.ctypes.data_as(C.c_void_p)))
    return status


class TrajectoryCorpus:
    """The records of one or more `.build.data` files resident on the context's device: `paths_or_bytes` is a path, bytes, or a list of
    either (one entry per file).  close() (or the context manager) frees it before the context goes."""

    def __init__(self, ctx, paths_or_bytes):
        is_bytes = lambda x: isinstance(x, (bytes, bytearray, memoryview))
        files = [paths_or_bytes] if (is_bytes(paths_or_bytes) or isinstance(paths_or_bytes, str)) else list(paths_or_bytes)
        blobs = [bytes(f) if is_bytes(f) else open(f, "rb").read() for f in files]
        buf = np.frombuffer(b"".join(blobs), np.uint8)
        sizes = (C.c_size_t * max(len(blobs), 1))(*[len(b) for b in blobs])
        self.ctx, self.handle = ctx, C.c_void_p()
        _lib.check(ctx.lib.oakgpu_build_corpus_create(ctx.handle, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, sizes, len(blobs),
                                                      C.byref(self.handle)))
        self.file_records = [len(b) // RECORD_BYTES for b in blobs]
        self.records = sum(self.file_records)

    def close(self):
        if self.handle:
            self.ctx.lib.oakgpu_build_corpus_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """{"records", "files", "status": count per TRAJ_STATUS name}: one scan of all records on the device the first time."""
        st = _lib.BuildCorpusStats()
        _lib.check(self.ctx.lib.oakgpu_build_corpus_info(self.handle, C.byref(st)))
        return {"records": int(st.records), "files": int(st.files), "status": {name: int(st.status_count[k]) for k, name in enumerate(TRAJ_STATUS)}}

    def _call(self, n, device, mask_dtype, no_score, mask, out, trim, run_dev, run_host):
        code, mdt = _MASK_DTYPES[mask_dtype]
        if out is None:
            out = {name: _empty((n,) + shape, mdt if dtype is None else dtype, device) for name, shape, dtype in _TRAJ_ARRAYS if mask or name != "mask"}
            out["t_max"] = _empty((1,), np.uint32, device)
        o, prm = _lib.BuildTrajectories(), _lib.BuildTrajParams(code, int(bool(no_score)))
        for name in out:
            setattr(o, name, _ptr(out[name]))
        if device is None:
            _lib.check(run_host(prm, o))
        else:
            _on_stream(self.ctx, device, lambda: run_dev(prm, o))
        if trim and "t_max" in out:
            t = int(out["t_max"][0])
            for name in ("action", "mask", "n_legal", "policy"):
                if name in out:
                    out[name] = out[name][:, :t]
        return out

    def decode(self, picks, mask_dtype="int64", no_score=False, mask=True, out=None, trim=False):
        """The trajectories of explicit picks (global record indices: the files' records in file order).  numpy picks give numpy arrays, a
        torch GPU tensor (int32) gives tensors on its device and copies nothing to the host.  A dict: action int64 [n, 31], mask [n, 31, 339]
        in mask_dtype (left out with mask=False, which makes the call cheap), n_legal [n, 31], policy f32 [n, 31], value / score f32 [n],
        start / end int64 [n], status uint8 [n], t_max [1] = max(end).  trim=True slices the per-step arrays to [:, :t_max] (the T of
        oak.torch.BuildTrajectories; it reads t_max, so it waits for the call).  out: the same dict preallocated by the caller."""
        lib, ctx, h = self.ctx.lib, self.ctx.handle, self.handle
        if hasattr(picks, "data_ptr"):
            p, device = picks.contiguous(), picks.device
        else:
            p, device = np.ascontiguousarray(picks, np.uint32).reshape(-1), None
        n = int(p.shape[0])
        return self._call(n, device, mask_dtype, no_score, mask, out, trim,
                          lambda prm, o: lib.oakgpu_build_traj_dev(ctx, h, _ptr(p), n, C.byref(prm), C.byref(o)),
                          lambda prm, o: lib.oakgpu_build_traj(ctx, h, _ptr(p), n, C.byref(prm), C.byref(o)))

    def sample(self, n, seed, mask_dtype="int64", no_score=False, mask=True, device=None, out=None, trim=False):
        """n draws of the reference's two-stage rule (draw i: fast_prng seeded with seed + i, a file, then a record of it) decoded as decode
        does, plus "picks" uint32 [n].  device None: numpy arrays; a torch device: tensors on it."""
        lib, ctx, h = self.ctx.lib, self.ctx.handle, self.handle
        picks = _empty((int(n),), np.uint32, device)
        out = self._call(int(n), device, mask_dtype, no_score, mask, out, trim,
                         lambda prm, o: lib.oakgpu_build_traj_sample_dev(ctx, h, int(n), int(seed), C.byref(prm), _ptr(picks), C.byref(o)),
                         lambda prm, o: lib.oakgpu_build_traj_sample(ctx, h, int(n), int(seed), C.byref(prm), _ptr(picks), C.byref(o)))
        out["picks"] = picks
        return out


class BuildWindow(TrajectoryCorpus):
    """The newest max_records `.build.data` records resident on the context's device (oakgpu_build_window_*): self-play appends, the oldest
    leave first, and info / decode / sample are TrajectoryCorpus's on the surviving records as ONE file, oldest first, bit for bit."""

    def __init__(self, ctx, max_records):
        self.ctx, self.window, self.handle, self.max_records = ctx, C.c_void_p(), C.c_void_p(), int(max_records)
        _lib.check(ctx.lib.oakgpu_build_window_create(ctx.handle, int(max_records), C.byref(self.window)))
        self.handle = C.c_void_p(ctx.lib.oakgpu_build_window_corpus(self.window))      # borrowed: freed with the window

    def close(self):
        if self.window:
            self.ctx.lib.oakgpu_build_window_destroy(self.window)
            self.window, self.handle = C.c_void_p(), C.c_void_p()

    def append(self, records, count=None):
        """records: `.build.data` bytes (or a uint8 array), or a uint8 GPU tensor of whole records with count, an int32 / uint32 GPU tensor of
        one word (game_records' pair) -- count None: every record of the tensor.  A record whose format byte is not 0 is rejected."""
        lib = self.ctx.lib
        if hasattr(records, "data_ptr"):
            import torch
            r = records.contiguous().view(-1)
            n = int(r.numel()) // RECORD_BYTES
            if r.dtype != torch.uint8 or r.numel() % RECORD_BYTES:
                raise ValueError("BuildWindow.append: a uint8 tensor of whole records")
            if count is None:
                count = torch.full((1,), n, dtype=torch.int32, device=r.device)
            _on_stream(self.ctx, r.device, lambda: lib.oakgpu_build_window_append_dev(self.ctx.handle, self.window, r.data_ptr(), count.data_ptr(), n))
        else:
            buf = np.frombuffer(bytes(records), np.uint8) if isinstance(records, (bytes, bytearray, memoryview)) else np.ascontiguousarray(records, np.uint8).reshape(-1)
            _lib.check(lib.oakgpu_build_window_append(self.ctx.handle, self.window, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size))

    def records(self):
        """the held records' bytes, oldest first"""
        size = C.c_size_t(0)
        _lib.check(self.ctx.lib.oakgpu_build_window_records(self.window, None, 0, C.byref(size)))
        out = np.zeros(max(size.value, 1), np.uint8)
        _lib.check(self.ctx.lib.oakgpu_build_window_records(self.window, out.ctypes.data_as(C.c_void_p), size.value, C.byref(size)))
        return out[:size.value].tobytes()

    def stats(self):
        st = (C.c_uint64 * 4)()
        _lib.check(self.ctx.lib.oakgpu_build_window_stats(self.window, C.byref(st)))
        return {"records": int(st[0]), "appended": int(st[1]), "evicted": int(st[2]), "rejected": int(st[3])}


def targets(ctx, traj, value_weight):
    """The network-free half of build.py's process_targets from a decoded dict (untrimmed): valid bool [n, 31]; n_valid; rows [V, 2] = (b, t)
    in the order of torch's x[valid]; state_cells [V, 31] / state_n [V], the actions in front of each valid step in step order (padded with
    65,535; -1 as int16 on the device); old_logp f32 [V] = the logarithm of policy taken in double, rounded once; rewards f32 [n, 31]."""
    on_device = hasattr(traj["action"], "data_ptr")
    device = traj["action"].device if on_device else None
    n = int(traj["action"].shape[0])
    t = _lib.BuildTrajectories()
    keep = {}
    for name in ("action", "policy", "value", "score", "start", "end"):
        keep[name] = traj[name].contiguous() if on_device else np.ascontiguousarray(traj[name])
        setattr(t, name, _ptr(keep[name]))
    out = {name: _empty((n * MAX_STEPS,) + shape if compact else (n,) + shape, dtype, device) for name, shape, dtype, compact in _TARGET_ARRAYS}
    count = _empty((1,), np.uint32, device)
    o = _lib.BuildTargetOutputs()
    for name in out:
        setattr(o, name, _ptr(out[name]))
    o.n_valid = _ptr(count)
    if on_device:
        _on_stream(ctx, device, lambda: ctx.lib.oakgpu_build_targets_dev(ctx.handle, C.byref(t), n, float(value_weight), C.byref(o)))
    else:
        _lib.check(ctx.lib.oakgpu_build_targets(ctx.handle, C.byref(t), n, float(value_weight), C.byref(o)))
    v = int(count[0])
    for name, _, _, compact in _TARGET_ARRAYS:
        if compact:
            out[name] = out[name][:v]
    out["valid"] = out["valid"].bool() if on_device else out["valid"].astype(bool)
    out["n_valid"] = v
    return out


def dense_state(ctx, targets, lo, hi):
    """f32 [hi - lo, 3749]: the dense 0/1 state of the valid rows lo .. hi-1, get_state(action)[valid][lo:hi] bit for bit."""
    cells, counts = targets["state_cells"], targets["state_n"]
    lo, hi = int(lo), int(hi)
    if hasattr(cells, "data_ptr"):
        import torch
        out = torch.empty((hi - lo, N_DIM), dtype=torch.float32, device=cells.device)
        _on_stream(ctx, cells.device, lambda: ctx.lib.oakgpu_build_state_dense_dev(ctx.handle, cells.data_ptr(), counts.data_ptr(), lo, hi, out.data_ptr()))
        return out
    out = np.empty((hi - lo, N_DIM), np.float32)
    _lib.check(ctx.lib.oakgpu_build_state_dense(ctx.handle, _ptr(np.ascontiguousarray(cells)), _ptr(np.ascontiguousarray(counts)), lo, hi, _ptr(out)))
    return out


# ---- training the build network: build.py's optimiser step on the device (oak_amd/csrc/buildtrain.hip) ------------------------------------
TRAINER_SEGMENT = 256      # OAKGPU_BUILD_TRAINER_SEGMENT: entries of one piece of a cell's segment in the transposed sparse products
TRAINER_PARTS = ("parameters", "gradients", "m", "v", "average")
TRAINER_TENSORS = tuple("%s.fc%d.%s" % (net, k, part) for net in ("policy", "value") for k in (1, 2, 3) for part in ("bias", "weight"))


def check_trainer(data, max_traj=1):
    """The refusals of Trainer, by name, without a GPU."""
    buf = np.frombuffer(bytes(data), np.uint8)
    _lib.check(_lib.load().oakgpu_build_trainer_check(buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, int(max_traj)))


class NoValidStep(Exception):
    """accumulate_batch: the first chunks of a run held no valid step"""


def accumulate_batch(ctx, corpus, trainer, batch_size, trajectories_per_step, keep_prob, value_weight, seed0, chunks, rows, device, hyper, generator=None):
    """One optimiser step's gradient (build.py:295-332: backward() per chunk until the batch is full), for tools/train_build_net.py and
    rl.run alike: zero_gradients, then chunks of trajectories_per_step draws from `corpus` (a TrajectoryCorpus or a BuildWindow) -- chunk
    number c draws with seed0 + c * trajectories_per_step, so no stream is used twice -- targets, the keep mask (torch.rand below
    keep_prob, from `generator` when given) and trainer.accumulate until batch_size kept rows are in.  chunks, rows: the run's counts so
    far; returns them advanced.  The caller follows with trainer.adam.  Raises NoValidStep when the run's first 16 chunks hold no valid step."""
    import torch
    trainer.zero_gradients()
    b = 0
    while b < batch_size:
        seed = (seed0 + chunks * trajectories_per_step) & (2 ** 64 - 1)
        chunks += 1
        traj = corpus.sample(trajectories_per_step, seed, mask_dtype="int16", device=device)
        tg = targets(ctx, traj, value_weight)
        keep = None if keep_prob >= 1.0 else torch.rand(tg["n_valid"], device=device, generator=generator) < keep_prob
        k = tg["n_valid"] if keep is None else int(keep.sum())
        if k == 0:
            if tg["n_valid"] == 0 and chunks > 16 and rows == 0:
                raise NoValidStep("no valid step in the first chunks")
            continue                                                 # "empty targets after sampling, probably a small buffer"
        trainer.accumulate(traj, tg, keep=keep, total=batch_size, remaining=batch_size - b, **hyper)
        b += k
        rows += min(k, batch_size - (b - k))
    return chunks, rows


class Trainer:
    """The optimiser step of the reference's build.py on the device, for the three-layer nets this project's rollout reads (a `.build.net`;
    NOT build.py's two-layer EmbeddingNets, which the reference's own reader cannot load): forward on the valid rows of a chunk of decoded
    trajectories, the loss with GAE, its exact gradient accumulated over chunks, torch.optim.Adam and the rolling average.  The rule is in
    include/oakgpu.h, "Training the build network".  A chunk is (traj, targets) as TrajectoryCorpus.decode / sample (untrimmed, with the
    mask) and build.targets return them on the device.  Every call but report / read / net_bytes is asynchronous on the context's stream."""

    def __init__(self, ctx, bytes_or_path, max_traj):
        data = bytes_or_path if isinstance(bytes_or_path, (bytes, bytearray, memoryview)) else open(bytes_or_path, "rb").read()
        buf = np.frombuffer(bytes(data), np.uint8)
        self.ctx, self.handle = ctx, C.c_void_p()
        _lib.check(ctx.lib.oakgpu_build_trainer_create(ctx.handle, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, int(max_traj), C.byref(self.handle)))
        dims, count, cap = (C.c_uint32 * 12)(), C.c_size_t(0), C.c_uint32(0)
        _lib.check(ctx.lib.oakgpu_build_trainer_shape(self.handle, C.byref(dims), C.byref(count), C.byref(cap)))
        self.dims = [(int(dims[2 * k]), int(dims[2 * k + 1])) for k in range(6)]
        self.count, self.max_traj = int(count.value), int(cap.value)
        self.policy_hidden, self.value_hidden = self.dims[0][1], (self.dims[3][1], self.dims[4][1])

    def close(self):
        if self.handle:
            self.ctx.lib.oakgpu_build_trainer_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chunk(self, traj, targets, keep, gamma, lam, policy_loss_weight, value_loss_weight, entropy_loss_weight, total, remaining):
        mask = traj["mask"]
        code = {8: 0, 2: 1}[mask.element_size()]
        n, v = int(traj["action"].shape[0]), int(targets["n_valid"])
        total = v if total is None else int(total)
        held = [mask.contiguous(), traj["n_legal"].contiguous(), targets["valid"].contiguous(), targets["rewards"].contiguous(), targets["rows"].contiguous(),
                targets["state_cells"].contiguous(), targets["state_n"].contiguous(), None if keep is None else keep.contiguous()]
        if held[7] is not None and held[7].element_size() != 1:
            raise ValueError("keep must be a bool or uint8 tensor of one entry per valid row")
        ptr = [None if x is None else x.data_ptr() for x in held]
        c = _lib.BuildChunk(ptr[0], code, n, ptr[1], ptr[2], ptr[3], v, ptr[4], ptr[5], ptr[6], ptr[7], float(gamma), float(gamma) * float(lam),
                            float(policy_loss_weight), float(value_loss_weight), float(entropy_loss_weight), max(total, 1),
                            max(total, 1) if remaining is None else max(int(remaining), 0))
        return c, held, mask.device, v

    def forward(self, traj, targets, keep=None, gamma=0.99, lam=0.95, policy_loss_weight=1.0, value_loss_weight=0.5, entropy_loss_weight=0.01, total=None,
                remaining=None, out=None):
        """The forward outputs of every valid row: logits [V, 339] (NaN beyond n_legal), value, logp, gae, returns, forced f32 [V], selected
        uint8 [V], du f32 [V] (the loss's gradient at the value net's output before the sigmoid).  total None: V; remaining None: total.  out: the same dict preallocated by the caller."""
        import torch
        c, held, device, v = self._chunk(traj, targets, keep, gamma, lam, policy_loss_weight, value_loss_weight, entropy_loss_weight, total, remaining)
        if out is None:
            out = {name: torch.empty((v,), dtype=torch.float32, device=device) for name in ("value", "logp", "gae", "returns", "forced", "du")}
            out["logits"] = torch.empty((v, MAX_ACTIONS), dtype=torch.float32, device=device)
            out["selected"] = torch.empty((v,), dtype=torch.uint8, device=device)
        o = _lib.BuildTrainOutputs()
        for name in out:
            setattr(o, name, out[name].data_ptr())
        _on_stream(self.ctx, device, lambda: self.ctx.lib.oakgpu_build_trainer_forward_dev(self.ctx.handle, self.handle, C.byref(c), C.byref(o)))
        return out

    def accumulate(self, traj, targets, keep=None, gamma=0.99, lam=0.95, policy_loss_weight=1.0, value_loss_weight=0.5, entropy_loss_weight=0.01, total=None,
                   remaining=None):
        """loss.backward() of one chunk: its gradient is formed on its own and added to the gradient block."""
        c, held, device, _ = self._chunk(traj, targets, keep, gamma, lam, policy_loss_weight, value_loss_weight, entropy_loss_weight, total, remaining)
        _on_stream(self.ctx, device, lambda: self.ctx.lib.oakgpu_build_trainer_accumulate_dev(self.ctx.handle, self.handle, C.byref(c)))

    def zero_gradients(self):
        _lib.check(self.ctx.lib.oakgpu_build_trainer_zero_gradients_dev(self.ctx.handle, self.handle))

    def adam(self, lr):
        """torch.optim.Adam's defaults over all twelve tensors at lr."""
        _lib.check(self.ctx.lib.oakgpu_build_trainer_adam_dev(self.ctx.handle, self.handle, float(lr)))

    def average(self, gamma):
        """rolling_average: average = average * gamma + (1 - gamma) * parameters."""
        _lib.check(self.ctx.lib.oakgpu_build_trainer_average_dev(self.ctx.handle, self.handle, float(gamma)))

    def report(self):
        """Of the last forward / accumulate -- the only call that waits: {"rows" (V), "kept" (k), "n_cap", "policy_loss", "value_loss",
        "entropy", "loss", "steps"}."""
        r = _lib.BuildTrainReport()
        _lib.check(self.ctx.lib.oakgpu_build_trainer_report(self.ctx.handle, self.handle, C.byref(r)))
        return {name: getattr(r, name) for name in ("rows", "kept", "n_cap", "policy_loss", "value_loss", "entropy", "loss", "steps")}

    def split(self, flat):
        """A flat block in file order -> {name: array} over TRAINER_TENSORS (views; weights [out, in])."""
        out, at = {}, 0
        for k, (i, o) in enumerate(self.dims):
            out[TRAINER_TENSORS[2 * k]] = flat[at:at + o]
            out[TRAINER_TENSORS[2 * k + 1]] = flat[at + o:at + o + o * i].reshape(o, i)
            at += o * (i + 1)
        return out

    def read(self, which="parameters"):
        """One of TRAINER_PARTS as {name: float32 array} in file order (weights [out, in])."""
        flat = np.empty(self.count, np.float32)
        _lib.check(self.ctx.lib.oakgpu_build_trainer_read(self.ctx.handle, self.handle, TRAINER_PARTS.index(which), flat.ctypes.data_as(C.c_void_p), flat.size))
        return self.split(flat)

    def set_gradients(self, grads):
        """grads: a flat float32 array of `count` entries in file order, a scalar, or a dict as read() returns it."""
        if isinstance(grads, dict):
            flat = np.concatenate([np.asarray(grads[name], np.float32).reshape(-1) for name in TRAINER_TENSORS])
        else:
            flat = np.ascontiguousarray(np.broadcast_to(np.asarray(grads, np.float32), (self.count,)) if np.ndim(grads) == 0 else np.asarray(grads, np.float32))
        flat = np.ascontiguousarray(flat)
        _lib.check(self.ctx.lib.oakgpu_build_trainer_set_gradients(self.ctx.handle, self.handle, flat.ctypes.data_as(C.c_void_p), flat.size))

    def net_bytes(self, which="net"):
        """The bytes of a `.build.net`: the parameters ("net") or the rolling average ("average")."""
        code = {"net": 0, "parameters": 0, "average": 4}[which]
        size = C.c_size_t(0)
        _lib.check(self.ctx.lib.oakgpu_build_trainer_net_bytes(self.ctx.handle, self.handle, code, None, 0, C.byref(size)))
        buf = np.empty(size.value, np.uint8)
        _lib.check(self.ctx.lib.oakgpu_build_trainer_net_bytes(self.ctx.handle, self.handle, code, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(size)))
        return buf.tobytes()

    def save(self, path, which="net"):
        with open(path, "wb") as f:
            f.write(self.net_bytes(which))
