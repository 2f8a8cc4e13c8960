"""Whole games between two policies, in batches resident on the GPU (include/oakgpu.h: oakgpu_policy_games*).

  policy_games(ctx, seats, ...)  <- the per-game loop of the reference's `vs` (cpp/src/vs.cc:107-408) in the form that needs no tree:
                                    vs --budget=0 --bandit=pucb-1.0 --policy-mode=p --p1-eval=A --p2-eval=B
  match(ctx, net_a, net_b, ...)  <- its outer loop (vs.cc:355-377) and its report (vs.cc:66-68,424-427): W D L, score, Elo difference
  search_games(ctx, seats, ...)  <- the per-game loop with a budget (vs.cc:230-345): both seats SEARCH, each with its own agent, on the
                                    forest search (include/oakgpu.h: oakgpu_forest_match*)
  search_match(ctx, a, b, ...)   <- the outer loop and the report for two search agents

Nothing here computes on the CPU but the bookkeeping of a finished batch."""
import contextlib
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from .engine import Network

RANDOM = "random"
ELO_FACTOR = 400.0 / math.log(10.0)   # vs.cc:68


def _seat(s):
    """None / "random" -> a RANDOM seat; a Network, (network, temp, min) or dict(net=, temp=, min=) -> a POLICY seat."""
    if s is None or s == RANDOM:
        return _lib.Seat(0, None, 0.0, 0.0)
    if isinstance(s, dict):
        net, temp, mn = s["net"], s.get("temp", 1.0), s.get("min", 0.0)
    elif isinstance(s, (tuple, list)):
        net, temp, mn = (tuple(s) + (1.0, 0.0))[:3]
    else:
        net, temp, mn = s, 1.0, 0.0
    return _lib.Seat(1, getattr(net, "handle", net), float(temp), float(mn))


@contextlib.contextmanager
def _ordered(ctx, device):
    """The context's stream behind torch's current stream for the call, and torch's behind it afterwards."""
    import torch
    mine = torch.cuda.ExternalStream(ctx.stream_ptr(), device=device)
    theirs = torch.cuda.current_stream(device)
    mine.wait_stream(theirs)
    try:
        yield
    finally:
        theirs.wait_stream(mine)


def policy_games(ctx, seats, battles, durations, results, prng, max_turns=1000, poll=16, compact_below=0.0, log_turns=0, return_state=False):
    """n whole games from the given states (as Context.rollout takes them), seat p1 = seats[0] against seat p2 = seats[1].

    numpy arrays in -> numpy arrays out (staged over PCIe); torch tensors on the GPU in -> torch tensors out, nothing leaves the device
    but the four counters.  `prng` is not modified; the continuing streams come back as "prng".  Returns a dict: results uint8[n], turns
    uint32[n] (int32 bit patterns for torch), values float32[n], prng uint8[n, 8], counts = (wins, ties, losses of seat p1, stopped at
    max_turns), log uint8[n, log_turns, 2] (prefilled 0xFF; None without log_turns), and battles / durations with return_state.
    Raises OakGpuError -- "RuntimePolicy: zero policy, mode: p (game i ...)" -- when `min` zeroed a whole policy."""
    p = _lib.PolicyGamesParams(_seat(seats[0]), _seat(seats[1]), int(max_turns), int(poll), float(compact_below), int(log_turns))
    counts = (C.c_uint64 * 4)()
    on_device = not isinstance(battles, np.ndarray) and hasattr(battles, "data_ptr")   # a torch tensor (torch is imported for those only)
    if not on_device:
        battles = np.ascontiguousarray(battles, dtype=np.uint8)
        n = battles.shape[0]
        durations = np.ascontiguousarray(durations, dtype=np.uint8).reshape(n, 8)
        results = np.ascontiguousarray(results, dtype=np.uint8).reshape(n)
        out = dict(results=np.zeros(n, np.uint8), turns=np.zeros(n, np.uint32), values=np.zeros(n, np.float32),
                   prng=np.ascontiguousarray(prng, dtype=np.uint8).reshape(n, 8).copy(),
                   battles=np.zeros((n, 384), np.uint8) if return_state else None, durations=np.zeros((n, 8), np.uint8) if return_state else None,
                   log=np.full((n, log_turns, 2), 0xFF, np.uint8) if log_turns else None)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = ctx.lib.oakgpu_policy_games(ctx.handle, C.byref(p), ptr(battles), ptr(durations), ptr(results), ptr(out["prng"]), n, ptr(out["results"]),
                                         ptr(out["turns"]), ptr(out["values"]), ptr(out["battles"]), ptr(out["durations"]), ptr(out["log"]), counts)
    else:
        import torch
        dev = battles.device
        n = battles.shape[0]
        u8 = lambda t, shape: t.to(device=dev, dtype=torch.uint8).reshape(shape).contiguous()
        battles, durations, results = u8(battles, (n, 384)), u8(durations, (n, 8)), u8(results, (n,))
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        out = dict(results=new((n,), torch.uint8), turns=new((n,), torch.int32), values=new((n,), torch.float32), prng=u8(prng, (n, 8)).clone(),
                   battles=new((n, 384), torch.uint8) if return_state else None, durations=new((n, 8), torch.uint8) if return_state else None,
                   log=torch.full((n, log_turns, 2), 0xFF, dtype=torch.uint8, device=dev) if log_turns else None)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with _ordered(ctx, dev):
            rc = ctx.lib.oakgpu_policy_games_dev(ctx.handle, C.byref(p), ptr(battles), ptr(durations), ptr(results), ptr(out["prng"]), n, ptr(out["results"]),
                                                 ptr(out["turns"]), ptr(out["values"]), ptr(out["battles"]), ptr(out["durations"]), ptr(out["log"]), counts)
    _lib.check(rc)
    out["counts"] = tuple(int(x) for x in counts)
    if not return_state:
        del out["battles"], out["durations"]
    return out


def last_stats(ctx):
    """The schedule of this thread's last policy_games call: rows the evaluator and the tree step ran over summed over the turns, turns
    looped, compactions, polls."""
    out = (C.c_uint64 * 4)()
    _lib.check(ctx.lib.oakgpu_policy_games_last_stats(out))
    return dict(zip(("row_turns", "turns", "compactions", "polls"), (int(x) for x in out)))


# ---- matches between two SEARCH agents over the forest search (oakgpu_forest_match*; the rules are in include/oakgpu.h) -----------------
FM_STATUS = ("OK", "MAX_TURNS", "ZERO_POLICY", "EARLY_STOP")
TURN_DTYPE = np.dtype([("c1", "u1"), ("c2", "u1"), ("m", "u1"), ("n", "u1"), ("zero", "<u4"), ("ev_p1", "<f8"), ("ev_p2", "<f8")])   # oakgpu_match_turn
_BANDITS = {"ucb": 0, "pucb": 1, "ucb1": 2, "exp3": 3, "pexp3": 4}


def _match_seat(s):
    """A search seat from a dict: iterations, bandit "ucb" | "pucb", c, evaluator "mc" | "poke-engine" | a Network, policy_mode, policy_temp,
    policy_min, max_depth, root_rolls, other_rolls (has_net / matrix_ucb / duration_us: for the check alone)."""
    ev = s.get("evaluator", "mc")
    use_net = not isinstance(ev, str)
    seat = _lib.MatchSeat()
    seat.search = _lib.SearchParams(iterations=int(s["iterations"]), batch=1, ucb_c=float(s.get("c", 2.0)), bandit=_BANDITS[s.get("bandit", "ucb")],
                                    eval=1 if use_net or ev == "net" else {"mc": 0, "poke-engine": 2}[ev], max_depth=int(s.get("max_depth", 0)),
                                    root_rolls=int(s.get("root_rolls", 3)), other_rolls=int(s.get("other_rolls", 1)), seed=0,
                                    matrix_ucb=int(s.get("matrix_ucb", 0)), mucb_delay=0, mucb_minimum=0, mucb_c=0.0, exp3_alpha=-1.0,
                                    duration_us=int(s.get("duration_us", 0)))
    seat.net = getattr(ev, "handle", None) if use_net else (C.c_void_p(1) if s.get("has_net") else None)
    mode = s.get("policy_mode", "e").encode()
    if len(mode) > 15:
        raise ValueError("policy_mode: at most 15 characters")
    seat.policy_mode = mode
    seat.policy_temp, seat.policy_min = float(s.get("policy_temp", 1.0)), float(s.get("policy_min", 0.0))
    return seat


def _match_params(seats, max_turns, early_stop, log_turns, solve_nash):
    return _lib.ForestMatchParams(_match_seat(seats[0]), _match_seat(seats[1]), int(max_turns), float(early_stop), int(log_turns), _lib.nash_mode(solve_nash))


def forest_match_check(max_trees, max_iterations, contextual, seats, n=1, max_turns=0, early_stop=0.0, solve_nash=True):
    """oakgpu_forest_match_check alone (host only, no GPU): raises OakGpuError with the refusal's message.  A seat's evaluator may be "net"
    here, with has_net saying whether a network is given."""
    p = _match_params(seats, max_turns, early_stop, 0, solve_nash)
    _lib.check(_lib.load().oakgpu_forest_match_check(int(max_trees), int(max_iterations), int(bool(contextual)), C.byref(p), int(n)))


def match_pick_host(side, m, n, visit_matrix, value_matrix, iterations, rng, nash=None, prior=None, policy_mode="e", policy_temp=1.0, policy_min=0.0,
                    early_stop=0.0):
    """oakgpu_match_pick_host (no GPU): ONE seat's pick and early-stop sign from one root output.  side 0 / 1; nash / prior: that side's.
    Returns a dict: policy float64[9], index, empirical_value, sign, rng (advanced).  Raises OakGpuError for a zeroed policy or a bad mode."""
    vis = np.ascontiguousarray(visit_matrix, dtype=np.uint64).reshape(81)
    val = np.ascontiguousarray(value_matrix, dtype=np.float64).reshape(81)
    opt = lambda a: None if a is None else np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1), np.zeros(9)])[:9])
    na, pr = opt(nash), opt(prior)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    state, ev, idx, sign = C.c_uint64(int(rng)), C.c_double(0), C.c_int32(0), C.c_int32(0)
    pol = np.zeros(9)
    _lib.check(_lib.load().oakgpu_match_pick_host(int(side), int(m), int(n), vp(vis), vp(val), int(iterations), vp(na), vp(pr), policy_mode.encode(),
                                                  float(policy_temp), float(policy_min), float(early_stop), C.byref(state), vp(pol), C.byref(idx), C.byref(ev),
                                                  C.byref(sign)))
    return {"policy": pol, "index": idx.value, "empirical_value": ev.value, "sign": sign.value, "rng": state.value}


def _match_records(ctx, forest, n, dev=None):
    """Both seats' records of the forest's last match call (oakgpu_forest_match_records): (p1, p2), each a dict of stream (bytes; with
    dev a uint8 tensor there), offsets [n + 1] and n_frames [n]."""
    lib, seats = ctx.lib, []
    for seat in (0, 1):
        size = C.c_size_t(0)
        _lib.check(lib.oakgpu_forest_match_records(forest.handle, seat, None, 0, C.byref(size), None, None, None, None, 0))
        if dev is None:
            stream, offsets, n_frames = np.zeros(max(size.value, 1), np.uint8), np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint32)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            _lib.check(lib.oakgpu_forest_match_records(forest.handle, seat, vp(stream), size.value, C.byref(size), vp(offsets), vp(n_frames), None, None, 0))
            seats.append(dict(stream=stream[:size.value].tobytes(), offsets=offsets, n_frames=n_frames[:n]))
        else:
            import torch
            stream = torch.zeros(max(size.value, 1), dtype=torch.uint8, device=dev)
            offsets, n_frames = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            with _ordered(ctx, dev):
                _lib.check(lib.oakgpu_forest_match_records(forest.handle, seat, stream.data_ptr(), size.value, C.byref(size), offsets.data_ptr(),
                                                           n_frames.data_ptr(), None, None, 1))
            seats.append(dict(stream=stream[:size.value], offsets=offsets, n_frames=n_frames[:n]))
    return tuple(seats)


def search_games(ctx, seats, battles, durations, results, seeds, forest=None, max_turns=1000, early_stop=0.0, log_turns=0, solve_nash=True, stats=None,
                 records=False):
    """n whole games from the given states between two SEARCH agents on the forest search (oakgpu_forest_match*): seats = (p1, p2), each a
    dict as _match_seat takes it; seeds uint64[n], one per game.  forest: None (one made for this call, contextual when a seat is PUCB)
    or a search.Forest to reuse; stats: optional dict that receives turns, p1_rows, p2_rows, host_reads.  solve_nash: True / "host" (the exact
    Nash solves of the searched rows on the host's threads), "device" / 2 (on the GPU, on the stream: the same bytes in every output) or False.

    numpy arrays in -> numpy arrays out; torch tensors on the GPU in (seeds int64 bit patterns) -> torch tensors out, nothing leaves the
    device but the counters.  Returns a dict: results uint8[n], turns uint32[n] (int32 for torch), status uint8[n] (FM_STATUS), counts =
    (wins, ties, losses of seat p1 with early stops, stopped at max_turns), log: TURN_DTYPE [n, log_turns] prefilled with 0xFF bytes
    (torch: uint8 [n, log_turns, 24]); None without log_turns.
    records: the dict gains records = (p1, p2), each seat's `.battle.data` of the games (vs.cc:380-395) as a dict: stream (bytes, or a uint8
    tensor on the device), offsets [n + 1] and n_frames [n]; a game cut at max_turns or stopped by a zeroed policy has zero bytes in both,
    a seat that was not searched in a turn has iterations 0 there (include/oakgpu.h)."""
    from .search import Forest
    p = _match_params(seats, max_turns, early_stop, log_turns, solve_nash)
    counts = (C.c_uint64 * 4)()
    on_device = not isinstance(battles, np.ndarray) and hasattr(battles, "data_ptr")
    n = int(battles.shape[0]) if on_device else len(np.asarray(results).reshape(-1))
    own = forest is None
    if own:
        forest = Forest(ctx, max(n, 1), max(int(seats[0]["iterations"]), int(seats[1]["iterations"]), 1),
                        contextual="pucb" in (seats[0].get("bandit"), seats[1].get("bandit")))
    try:
        if records or not own:                   # (a forest of the caller's keeps its switch: set it either way)
            _lib.check(ctx.lib.oakgpu_forest_match_set_records(forest.handle, int(bool(records))))
        if not on_device:
            battles = np.ascontiguousarray(battles, dtype=np.uint8).reshape(n, 384)
            durations = np.ascontiguousarray(durations, dtype=np.uint8).reshape(n, 8)
            results = np.ascontiguousarray(results, dtype=np.uint8).reshape(n)
            seeds = np.ascontiguousarray(np.asarray(seeds).astype(np.uint64)).reshape(n)
            out = dict(results=np.zeros(n, np.uint8), turns=np.zeros(n, np.uint32), status=np.zeros(n, np.uint8),
                       log=np.frombuffer(bytearray(b"\xff" * (n * log_turns * 24)), dtype=TURN_DTYPE).reshape(n, log_turns) if log_turns else None)
            ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
            rc = ctx.lib.oakgpu_forest_match(forest.handle, C.byref(p), ptr(battles), ptr(durations), ptr(results), ptr(seeds), n, ptr(out["results"]),
                                             ptr(out["turns"]), ptr(out["status"]), ptr(out["log"]), counts)
        else:
            import torch
            dev = battles.device
            u8 = lambda t, shape: t.to(device=dev, dtype=torch.uint8).reshape(shape).contiguous()
            battles, durations, results, seeds = u8(battles, (n, 384)), u8(durations, (n, 8)), u8(results, (n,)), seeds.contiguous()
            new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
            out = dict(results=new((n,), torch.uint8), turns=new((n,), torch.int32), status=new((n,), torch.uint8),
                       log=torch.full((n, log_turns, 24), 0xFF, dtype=torch.uint8, device=dev) if log_turns else None)
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
            with _ordered(ctx, dev):
                rc = ctx.lib.oakgpu_forest_match_dev(forest.handle, C.byref(p), ptr(battles), ptr(durations), ptr(results), ptr(seeds), n, ptr(out["results"]),
                                                     ptr(out["turns"]), ptr(out["status"]), ptr(out["log"]), counts)
        _lib.check(rc)
        out["counts"] = tuple(int(x) for x in counts)
        if records:
            out["records"] = _match_records(ctx, forest, n, dev if on_device else None)
        if stats is not None:
            st = (C.c_uint64 * 4)()
            _lib.check(ctx.lib.oakgpu_forest_match_last_stats(forest.handle, C.byref(st)))
            stats.update(turns=int(st[0]), p1_rows=int(st[1]), p2_rows=int(st[2]), host_reads=int(st[3]))
        return out
    finally:
        if own:
            forest.close()


def search_match(ctx, agent_a, agent_b, teams, games, seed, mirror=False, max_turns=1000, early_stop=10.0, solve_nash=True, return_games=False,
                 records_dir=None):
    """`games` matches between search agents A and B (dicts as _match_seat takes them; an evaluator may also be a `.battle.net` path, loaded
    for the call, "discrete": True choosing the int8 form) as vs.cc:355-377 plays them: per match two teams drawn from `teams` (uint8
    [T, 6, 5]; one team for both sides with mirror), played in both seatings with the agents swapped unless mirror is set.  A drawn pair
    that fails the endless-battle check (oakgpu_endless_battle_check, on the host) is drawn again.  Every seating is one search_games batch.

    Returns a dict from A's point of view: W, D, L, games, score, elo, early_stops, stopped (games cut at max_turns: counted as draws), and
    zero_policy (games a zeroed policy stopped: counted nowhere else); with return_games the per-seating inputs and outputs.
    records_dir: every seating k also writes <dir>/p1/<k>.battle.data and <dir>/p2/<k>.battle.data, seat p1's and seat p2's records of its
    games (vs.cc:380-395; in seating 1 seat p1 is agent B); the result gains record_files, the paths in that order."""
    import torch
    lib = _lib.load()
    teams = np.ascontiguousarray(teams, dtype=np.uint8).reshape(-1, 6, 5)
    rng = np.random.default_rng(int(seed))
    pairs = int(games)
    pick = np.zeros((pairs, 2), np.int64)
    for g in range(pairs):
        for _ in range(1000):
            pick[g] = rng.integers(0, teams.shape[0], size=2)
            if mirror:
                pick[g, 1] = pick[g, 0]
            both = np.ascontiguousarray(np.concatenate([teams[pick[g, 0]].reshape(30), teams[pick[g, 1]].reshape(30)]))
            if not lib.oakgpu_endless_battle_check(both.ctypes.data_as(C.c_void_p)):
                break
        else:
            raise _lib.OakGpuError("search_match: every drawn team pair fails the endless-battle check")
    seatings = 1 if mirror else 2
    battle_seeds = rng.integers(1, 2 ** 63, size=(seatings, pairs), dtype=np.uint64)
    streams = rng.integers(1, 2 ** 63, size=(seatings, pairs), dtype=np.uint64)
    loaded = {}

    def agent_of(a):
        a = dict(a)
        ev = a.get("evaluator", "mc")
        if isinstance(ev, str) and ev not in ("mc", "poke-engine"):
            key = (ev, bool(a.get("discrete")))
            if key not in loaded:
                loaded[key] = Network(ctx, path=ev, discrete=key[1])
            a["evaluator"] = loaded[key]
        return a

    forest = None
    try:
        from .search import Forest
        a, b = agent_of(agent_a), agent_of(agent_b)
        forest = Forest(ctx, max(pairs, 1), max(int(a["iterations"]), int(b["iterations"]), 1), contextual="pucb" in (a.get("bandit"), b.get("bandit")))
        dev = torch.device("cuda", ctx.device)
        both = np.ascontiguousarray(np.stack([teams[pick[:, 0]], teams[pick[:, 1]]], axis=1).reshape(pairs, 60))
        d_teams = torch.from_numpy(both).to(dev)
        w = d = l = stopped = early = zeroed = 0
        played, files = [], []
        for s in range(seatings):
            d_seeds = torch.from_numpy(battle_seeds[s].view(np.int64)).to(dev)
            bt = torch.empty((pairs, 384), dtype=torch.uint8, device=dev)
            du = torch.empty((pairs, 8), dtype=torch.uint8, device=dev)
            rs = torch.empty((pairs,), dtype=torch.uint8, device=dev)
            with _ordered(ctx, dev):
                _lib.check(ctx.lib.oakgpu_init_battles_dev(ctx.handle, C.c_void_p(d_teams.data_ptr()), C.c_void_p(d_seeds.data_ptr()), pairs, 1,
                                                           C.c_void_p(bt.data_ptr()), C.c_void_p(du.data_ptr()), C.c_void_p(rs.data_ptr())))
            out = search_games(ctx, (a, b) if s == 0 else (b, a), bt, du, rs, torch.from_numpy(streams[s].view(np.int64)).to(dev), forest=forest,
                               max_turns=max_turns, early_stop=early_stop, solve_nash=solve_nash, records=records_dir is not None)
            if records_dir is not None:
                for name, rec in zip(("p1", "p2"), out["records"]):
                    os.makedirs(os.path.join(records_dir, name), exist_ok=True)
                    files.append(os.path.join(records_dir, name, "%d.battle.data" % s))
                    with open(files[-1], "wb") as fh:
                        fh.write(rec["stream"].cpu().numpy().tobytes())
            wins, ties, losses, cut = out["counts"]
            w += wins if s == 0 else losses
            l += losses if s == 0 else wins
            d += ties + cut
            stopped += cut
            status = out["status"].cpu().numpy()
            early += int((status == 3).sum())
            zeroed += int((status == 2).sum())
            if return_games:
                played.append(dict(a_is_p1=s == 0, teams=pick.copy(), battle_seeds=battle_seeds[s].copy(), streams=streams[s].copy(),
                                   results=out["results"].cpu().numpy(), turns=out["turns"].cpu().numpy(), status=status, counts=out["counts"]))
    finally:
        if forest is not None:
            forest.close()
        for net in loaded.values():
            net.close()
    total = w + d + l
    score = (w + 0.5 * d) / total if total else 0.5
    res = dict(W=w, D=d, L=l, games=total, score=score, elo=elo_difference(score), early_stops=early, stopped=stopped, zero_policy=zeroed)
    if return_games:
        res["seatings"] = played
    if records_dir is not None:
        res["record_files"] = files
    return res


def elo_difference(score):
    """inverse_sigmoid(score) * 400 / ln 10 (vs.cc:66-68,424-427); +-inf at a score of 1 / 0."""
    if score <= 0.0:
        return -math.inf
    if score >= 1.0:
        return math.inf
    return (math.log(score) - math.log(1.0 - score)) * ELO_FACTOR


def match(ctx, net_a, net_b, teams, games, seed, mirror=False, temp=1.0, min=0.0, discrete=(False, False), max_turns=1000, return_games=False):
    """`games` matches between net A and net B as vs.cc:355-377 plays them: per match two teams drawn from `teams` (uint8 [T, 6, 5]: species,
    four moves; one team for both sides with mirror), played in both seatings -- A in seat p1, then B in seat p1 from the same two teams --
    unless mirror is set, so 2 x games games (games with mirror).  The battles are built on the device (oakgpu_init_battles_dev with the
    opening update), every seating is one policy_games batch.  net_a / net_b: a Network, a `.battle.net` path (loaded for the call,
    discrete[i] choosing the int8 form) or None / "random".  temp / min: RuntimePolicy's options, for both nets.

    Returns a dict from net A's point of view -- the second seating's results are flipped: W, D, L, games, score = (W + D / 2) / games,
    elo = elo_difference(score), stopped (games cut at max_turns: they count as draws, as the rollout values them) -- and, with
    return_games, per seating the teams, seeds and policy_games outputs."""
    import torch
    teams = np.ascontiguousarray(teams, dtype=np.uint8).reshape(-1, 6, 5)
    rng = np.random.default_rng(int(seed))
    pairs = int(games)
    pick = rng.integers(0, teams.shape[0], size=(pairs, 2))
    if mirror:
        pick[:, 1] = pick[:, 0]
    seatings = 1 if mirror else 2
    battle_seeds = rng.integers(1, 2 ** 63, size=(seatings, pairs), dtype=np.uint64)
    streams = rng.integers(1, 2 ** 63, size=(seatings, pairs), dtype=np.uint64)
    loaded = {}

    def net_of(x, is_discrete):
        if x is None or x == RANDOM or isinstance(x, Network):
            return x
        key = (str(x), bool(is_discrete))       # (the same file in both seats is one handle: one evaluator call per turn)
        if key not in loaded:
            loaded[key] = Network(ctx, path=x, discrete=bool(is_discrete))
        return loaded[key]

    try:
        a, b = net_of(net_a, discrete[0]), net_of(net_b, discrete[1])
        seat = lambda net: RANDOM if net is None or net == RANDOM else (net, temp, min)
        dev = torch.device("cuda", ctx.device)
        both = np.ascontiguousarray(np.stack([teams[pick[:, 0]], teams[pick[:, 1]]], axis=1).reshape(pairs, 60))
        d_teams = torch.from_numpy(both).to(dev)
        w = d = l = stopped = 0
        played = []
        for s in range(seatings):
            d_seeds = torch.from_numpy(battle_seeds[s].view(np.int64)).to(dev)
            bt = torch.empty((pairs, 384), dtype=torch.uint8, device=dev)
            du = torch.empty((pairs, 8), dtype=torch.uint8, device=dev)
            rs = torch.empty((pairs,), dtype=torch.uint8, device=dev)
            with _ordered(ctx, dev):
                _lib.check(ctx.lib.oakgpu_init_battles_dev(ctx.handle, C.c_void_p(d_teams.data_ptr()), C.c_void_p(d_seeds.data_ptr()), pairs, 1,
                                                           C.c_void_p(bt.data_ptr()), C.c_void_p(du.data_ptr()), C.c_void_p(rs.data_ptr())))
            prng = torch.from_numpy(streams[s].view(np.uint8).reshape(pairs, 8)).to(dev)
            out = policy_games(ctx, (seat(a), seat(b)) if s == 0 else (seat(b), seat(a)), bt, du, rs, prng, max_turns=max_turns)
            wins, ties, losses, cut = out["counts"]
            w += wins if s == 0 else losses
            l += losses if s == 0 else wins
            d += ties + cut
            stopped += cut
            if return_games:
                played.append(dict(a_is_p1=s == 0, teams=pick.copy(), battle_seeds=battle_seeds[s].copy(), streams=streams[s].copy(),
                                   results=out["results"].cpu().numpy(), turns=out["turns"].cpu().numpy(), counts=out["counts"]))
    finally:
        for net in loaded.values():
            net.close()
    total = w + d + l
    score = (w + 0.5 * d) / total if total else 0.5
    res = dict(W=w, D=d, L=l, games=total, score=score, elo=elo_difference(score), stopped=stopped)
    if return_games:
        res["seatings"] = played
    return res
