"""Whole games between two policies, in batches resident on the GPU (include/oakgpu.h: oakgpu_policy_games*).

  policy_games(ctx, seats, ...)  <- the per-game loop of the reference's `vs` (cpp/src/vs.cc:107-408) in the form that needs no tree:
                                    vs --budget=0 --bandit=pucb-1.0 --policy-mode=p --p1-eval=A --p2-eval=B
  match(ctx, net_a, net_b, ...)  <- its outer loop (vs.cc:355-377) and its report (vs.cc:66-68,424-427): W D L, score, Elo difference

Nothing here computes on the CPU but the bookkeeping of a finished batch."""
import contextlib
import ctypes as C
import math

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
