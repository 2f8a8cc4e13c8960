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


def _set_fast(prm, fast_budget, fast_search_prob, fast_policy_mode):
    """The fast-search fields of oakgpu_selfplay_params (generate's --fast-budget / --fast-search-prob; all zero = off)."""
    mode = fast_policy_mode.encode()
    if len(mode) > 15:
        raise ValueError("fast_policy_mode: at most 15 characters")
    prm.fast_budget, prm.fast_search_prob, prm.fast_policy_mode = int(fast_budget), float(fast_search_prob), mode


def selfplay_game(ctx, teams, battle_seed, iterations=1 << 12, batch=1024, bandit="ucb", c=2.0, evaluator="mc", policy_mode="e",
                  policy_temp=1.0, policy_min=0.0, max_battle_length=0, seed=1, alpha=0.05, root_rolls=3, other_rolls=1, keep_node=False,
                  stats=None, fast_budget=0, fast_search_prob=0.0, fast_policy_mode=""):
    """One self-play game on the GPU path (oakgpu_selfplay_game).  teams: uint8[2, 6, 5] (species + 4 moves per set).
    keep_node: generate's --keep-node (one heap for the game, Heap::update after every turn); stats: optional dict that
    receives "nodes_kept".  fast_search_prob > 0: generate's fast searches -- each turn is, with that probability (one draw from the
    game's stream before the search seed), searched with fast_budget iterations (0 = iterations) and picked with fast_policy_mode
    ("" = policy_mode); every frame stores the iterations that ran.  Returns (record bytes, number of frames, final result byte)."""
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
    _set_fast(prm, fast_budget, fast_search_prob, fast_policy_mode)
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
                   threads_per_game=0, fast_budget=0, fast_search_prob=0.0, fast_policy_mode=""):
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
        _set_fast(prms[g], fast_budget, fast_search_prob, fast_policy_mode)
    t = np.ascontiguousarray(teams, dtype=np.uint8).reshape(n, 60)
    bs = (C.c_uint64 * n)(*[int(x) for x in battle_seeds])
    cap = 4 + 2 + 384 + 1 + 83 * (int(max_battle_length) or 2048)
    out = np.zeros((n, cap), dtype=np.uint8)
    written, frames, result = (C.c_size_t * n)(), (C.c_uint32 * n)(), (C.c_uint8 * n)()
    cp = (C.c_void_p * n)(*[c_.handle for c_ in ctxs])
    _lib.check(ctxs[0].lib.oakgpu_selfplay_games(cp, evaluator.handle if use_net else None, t.ctypes.data_as(C.c_void_p), bs, prms, n, int(threads_per_game),
                                                 out.ctypes.data_as(C.c_void_p), cap, written, frames, result))
    return [(out[g, :written[g]].tobytes(), int(frames[g]), int(result[g])) for g in range(n)]


# ---- self-play over the forest search (oakgpu_forest_selfplay*; the rules are in include/oakgpu.h) -------------------------------------
FSP_STATUS = ("OK", "MAX_LENGTH", "ZERO_POLICY", "SKIPPED")


def _selfplay_params(iterations, bandit, c, evaluator, policy_mode, policy_temp, policy_min, max_battle_length, root_rolls, other_rolls, max_depth):
    use_net = not isinstance(evaluator, str)
    prm = _lib.SelfplayParams()
    prm.search = _lib.SearchParams(iterations=int(iterations), batch=1, ucb_c=float(c), bandit={"ucb": 0, "pucb": 1, "ucb1": 2, "exp3": 3, "pexp3": 4}[bandit],
                                   eval=1 if use_net else {"mc": 0, "poke-engine": 2}[evaluator], max_depth=int(max_depth), root_rolls=int(root_rolls),
                                   other_rolls=int(other_rolls), seed=0, matrix_ucb=0, mucb_delay=0, mucb_minimum=0, mucb_c=0.0, exp3_alpha=-1.0,
                                   duration_us=0)
    mode = policy_mode.encode()
    if len(mode) > 15:
        raise ValueError("policy_mode: at most 15 characters")
    prm.policy_mode = mode
    prm.policy_temp, prm.policy_min = float(policy_temp), float(policy_min)
    prm.max_battle_length, prm.seed, prm.keep_node = int(max_battle_length), 0, 0
    return prm


def forest_selfplay(ctx, teams, battle_seeds, seeds, iterations, c=2.0, bandit="ucb", evaluator="mc", policy_mode="e", policy_temp=1.0,
                    policy_min=0.0, max_battle_length=0, root_rolls=3, other_rolls=1, max_depth=0, forest=None, solve_nash=True, stats=None,
                    keep_node=False, keep_arena=0, fast_budget=0, fast_search_prob=0.0, fast_policy_mode="", built=None, battle_skip_prob=0.0,
                    t1_budget=0):
    """n self-play games at once over the forest search, resident on the GPU (oakgpu_forest_selfplay*): game g is selfplay_game(ctx,
    teams[g], battle_seeds[g], batch=1, seed=seeds[g], ...).  teams uint8[n, 2, 6, 5]; forest: None (one made for this call) or a
    search.Forest to reuse; stats: optional dict that receives turns, rows searched, compactions and host reads (of the live count), and
    loop_syncs / loop_copies: the turn loop's stream synchronisations and host <-> device copies.
    solve_nash: True / "host" (the exact solves on the host's threads), "device" / 2 (on the GPU, on the stream: the same bits, two
    synchronisations and two copies fewer per turn) or False (the nash fields are zeros).
    keep_node: generate's --keep-node -- each game's tree goes on from turn to turn (a kept forest: one made with keep_arena nodes per tree,
    0 = 4 * iterations + 1, or the caller's Forest(keep_arena=...)); a sixth value is then returned, nodes_kept uint32[n] (selfplay_game's
    stats["nodes_kept"] per game), and stats also receives nodes_kept, dropped, mismatches and carried_nodes.
    fast_search_prob > 0: generate's fast searches, as in selfplay_game; each turn is ONE budgets search over the live rows, those of the
    larger budget first.  stats then also tells fast_frames, full_frames (the frames min_iterations = fast_budget + 1 keeps for training),
    launched and run (tree-iterations: equal, since no launch covers a finished tree).  A forest made here holds max(iterations,
    fast_budget, t1_budget) iterations.
    built: None, or uint8[n] (bit 0: p1's team was built, bit 1: p2's; a tensor with tensors in) -- generate's skipped battles: a game
    with a built seat is skipped with probability battle_skip_prob (selfplay_skip_host is the rule): searched once with t1_budget iterations
    (0 = iterations), status SKIPPED, zero bytes, no frames.  A game that is not skipped is the game of a call without the three, byte for
    byte.  Turn 1's rows are not sorted by budget, so launched may exceed run by that turn's slack.
    stats["matchup"]: float64[n] (a tensor with tensors in), the empirical value of each game's first search -- the value of a built
    seat's trajectory (p2's is 1 - it); NaN for a game never searched.
    numpy arrays in: (stream bytes, offsets uint64[n + 1], n_frames uint32[n], results uint8[n], status uint8[n]) -- the stream is the
    kept games' records in game order, a dropped game (status MAX_LENGTH / ZERO_POLICY, see FSP_STATUS) has zero bytes.
    torch GPU tensors in (teams uint8 [n, 60]; battle_seeds, seeds int64 bit patterns): the same five as tensors on that device; nothing
    but the stream's size is copied to the host."""
    from .search import Forest
    use_net = not isinstance(evaluator, str)
    prm = _selfplay_params(iterations, bandit, c, evaluator, policy_mode, policy_temp, policy_min, max_battle_length, root_rolls, other_rolls, max_depth)
    prm.keep_node = 1 if keep_node else 0
    _set_fast(prm, fast_budget, fast_search_prob, fast_policy_mode)
    skip = _lib.SelfplaySkip(int(t1_budget), float(battle_skip_prob))
    net = evaluator.handle if use_net else None
    on_device = hasattr(teams, "data_ptr")
    n = int(teams.shape[0]) if on_device else len(np.asarray(seeds).reshape(-1))
    own = forest is None
    if own:
        forest = Forest(ctx, max(n, 1), max(int(iterations), int(fast_budget), int(t1_budget), 1), contextual=bandit == "pucb", keep_arena=int(keep_arena) if keep_node else None)
    lib = ctx.lib
    try:
        size = C.c_size_t(0)
        if on_device:
            import torch
            dev = teams.device
            teams, battle_seeds, seeds = teams.contiguous().view(n, 60), battle_seeds.contiguous(), seeds.contiguous()
            mine, theirs = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev), torch.cuda.current_stream(dev)
            mine.wait_stream(theirs)
            if built is not None:
                built = built.contiguous().view(torch.uint8)
                if built.numel() != n:
                    raise ValueError("built: one byte per game")
            _lib.check(lib.oakgpu_forest_selfplay_build_dev(forest.handle, net, C.byref(prm), C.byref(skip), teams.data_ptr(), battle_seeds.data_ptr(), seeds.data_ptr(),
                                                            None if built is None or n == 0 else built.data_ptr(), n, _lib.nash_mode(solve_nash)))
            _lib.check(lib.oakgpu_forest_selfplay_records(forest.handle, None, 0, C.byref(size), None, None, None, None, 1))
            stream = torch.zeros(max(size.value, 1), dtype=torch.uint8, device=dev)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            n_frames = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            results, status = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev), torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
            _lib.check(lib.oakgpu_forest_selfplay_records(forest.handle, stream.data_ptr(), size.value, C.byref(size), offsets.data_ptr(),
                                                          n_frames.data_ptr(), results.data_ptr(), status.data_ptr(), 1))
            theirs.wait_stream(mine)
            out = (stream[:size.value], offsets, n_frames[:n], results[:n], status[:n])
            if keep_node:
                kept = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
                mine.wait_stream(theirs)
                _lib.check(lib.oakgpu_forest_selfplay_nodes_kept(forest.handle, kept.data_ptr(), 1))
                theirs.wait_stream(mine)
                out += (kept[:n],)
        else:
            t = np.ascontiguousarray(teams, dtype=np.uint8).reshape(n, 60)
            bs = np.ascontiguousarray(np.asarray(battle_seeds).astype(np.uint64)).reshape(n)
            sd = np.ascontiguousarray(np.asarray(seeds).astype(np.uint64)).reshape(n)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            bt = None if built is None else np.ascontiguousarray(np.asarray(built).astype(np.uint8)).reshape(n)
            _lib.check(lib.oakgpu_forest_selfplay_build(forest.handle, net, C.byref(prm), C.byref(skip), vp(t), vp(bs), vp(sd), None if bt is None or n == 0 else vp(bt), n,
                                                        _lib.nash_mode(solve_nash)))
            _lib.check(lib.oakgpu_forest_selfplay_records(forest.handle, None, 0, C.byref(size), None, None, None, None, 0))
            stream = np.zeros(max(size.value, 1), np.uint8)
            offsets, n_frames = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint32)
            results, status = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
            _lib.check(lib.oakgpu_forest_selfplay_records(forest.handle, vp(stream), size.value, C.byref(size), vp(offsets), vp(n_frames), vp(results),
                                                          vp(status), 0))
            out = (stream[:size.value].tobytes(), offsets, n_frames[:n], results[:n], status[:n])
            if keep_node:
                kept = np.zeros(max(n, 1), np.uint32)
                _lib.check(lib.oakgpu_forest_selfplay_nodes_kept(forest.handle, vp(kept), 0))
                out += (kept[:n],)
        if stats is not None:
            st = (C.c_uint64 * 4)()
            _lib.check(lib.oakgpu_forest_selfplay_last_stats(forest.handle, C.byref(st)))
            stats.update(turns=int(st[0]), rows=int(st[1]), compactions=int(st[2]), host_reads=int(st[3]))
            tr = (C.c_uint64 * 2)()
            _lib.check(lib.oakgpu_forest_selfplay_last_traffic(forest.handle, C.byref(tr)))
            stats.update(loop_syncs=int(tr[0]), loop_copies=int(tr[1]))
            _lib.check(lib.oakgpu_forest_selfplay_fast_stats(forest.handle, C.byref(st)))
            stats.update(fast_frames=int(st[0]), full_frames=int(st[1]), launched=int(st[2]), run=int(st[3]))
            if on_device:
                matchup = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
                mine.wait_stream(theirs)
                _lib.check(lib.oakgpu_forest_selfplay_matchup(forest.handle, matchup.data_ptr(), 1))
                theirs.wait_stream(mine)
            else:
                matchup = np.zeros(max(n, 1), np.float64)
                _lib.check(lib.oakgpu_forest_selfplay_matchup(forest.handle, vp(matchup), 0))
            stats["matchup"] = matchup[:n]
            if keep_node:
                _lib.check(lib.oakgpu_forest_selfplay_keep_stats(forest.handle, C.byref(st)))
                stats.update(nodes_kept=int(st[0]), dropped=int(st[1]), mismatches=int(st[2]), carried_nodes=int(st[3]))
        return out
    finally:
        if own:
            forest.close()


def forest_selfplay_check(max_trees, max_iterations, contextual, iterations, n=1, teams=None, c=2.0, bandit="ucb", evaluator="mc", policy_mode="e",
                          policy_temp=1.0, policy_min=0.0, max_battle_length=0, root_rolls=3, other_rolls=1, max_depth=0, solve_nash=True,
                          has_net=False, keep_node=False, matrix_ucb=0, duration_us=0, kept=False, fast_budget=0, fast_search_prob=0.0,
                          fast_policy_mode="", battle_skip_prob=0.0, t1_budget=0):
    """oakgpu_forest_selfplay_check alone (host only, no GPU): raises OakGpuError with the refusal's message.  evaluator "mc" | "poke-engine" |
    "net" (with has_net saying whether a network is given); kept: the limits are a kept forest's (oakgpu_forest_create_kept)."""
    prm = _selfplay_params(iterations, bandit, c, "mc" if evaluator == "net" else evaluator, policy_mode, policy_temp, policy_min, max_battle_length,
                           root_rolls, other_rolls, max_depth)
    if evaluator == "net":
        prm.search.eval = 1
    prm.keep_node, prm.search.matrix_ucb, prm.search.duration_us = int(bool(keep_node)), int(matrix_ucb), int(duration_us)
    _set_fast(prm, fast_budget, fast_search_prob, fast_policy_mode)
    t = None if teams is None else np.ascontiguousarray(teams, dtype=np.uint8).reshape(n, 60)
    _lib.check(_lib.load().oakgpu_forest_selfplay_check(int(max_trees), int(max_iterations), int(bool(contextual)) | (2 if kept else 0), C.byref(prm), int(bool(has_net)), int(n),
                                                        None if t is None else t.ctypes.data_as(C.c_void_p), _lib.nash_mode(solve_nash)))
    skip = _lib.SelfplaySkip(int(t1_budget), float(battle_skip_prob))     # (what the _build calls check next)
    _lib.check(_lib.load().oakgpu_forest_selfplay_skip_check(int(max_iterations), C.byref(skip)))


def selfplay_pick_host(m, n, visit_matrix, value_matrix, iterations, rng, p1_nash=None, p2_nash=None, nash_value=0.0, p1_prior=None, p2_prior=None,
                       p1_choices=None, p2_choices=None, policy_mode="e", policy_temp=1.0, policy_min=0.0):
    """oakgpu_selfplay_pick_host (no GPU): one turn's pick from a root output by the rule the device game loop compiles.  visit_matrix uint64
    [9, 9], value_matrix float64 [9, 9]; rng: the game's stream state.  Returns a dict: empirical_value, p1_empirical, p2_empirical, p1_policy,
    p2_policy (float64[9]), i, j, rng (advanced), update (bytes).  Raises OakGpuError for a zeroed policy or a bad mode."""
    lib = _lib.load()
    vis = np.ascontiguousarray(visit_matrix, dtype=np.uint64).reshape(81)
    val = np.ascontiguousarray(value_matrix, dtype=np.float64).reshape(81)
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=dt).reshape(-1), np.zeros(9, dt)])[:9])
    arrs = [opt(p1_nash, np.float64), opt(p2_nash, np.float64), opt(p1_prior, np.float64), opt(p2_prior, np.float64), opt(p1_choices, np.uint8),
            opt(p2_choices, np.uint8)]
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    state, ev, i, j, ulen = C.c_uint64(int(rng)), C.c_double(0), C.c_int32(0), C.c_int32(0), C.c_uint32(0)
    e1, e2, q1, q2 = (np.zeros(9) for _ in range(4))
    upd = np.zeros(83, np.uint8)
    _lib.check(lib.oakgpu_selfplay_pick_host(int(m), int(n), vp(vis), vp(val), int(iterations), vp(arrs[0]), vp(arrs[1]), float(nash_value), vp(arrs[2]),
                                             vp(arrs[3]), vp(arrs[4]), vp(arrs[5]), policy_mode.encode(), float(policy_temp), float(policy_min),
                                             C.byref(state), C.byref(ev), vp(e1), vp(e2), vp(q1), vp(q2), C.byref(i), C.byref(j), vp(upd), C.byref(ulen)))
    return {"empirical_value": ev.value, "p1_empirical": e1, "p2_empirical": e2, "p1_policy": q1, "p2_policy": q2, "i": i.value, "j": j.value,
            "rng": state.value, "update": upd[:ulen.value].tobytes()}


def selfplay_skip_host(seed, prob, built):
    """oakgpu_selfplay_skip_host (no GPU): whether the forest loop skips the game of this seed (generate's --battle-skip-prob), by the rule
    the device loop compiles: built != 0, prob > 0 and the first uniform of the stream seed ^ SKIP_STREAM_XOR below prob."""
    return bool(_lib.load().oakgpu_selfplay_skip_host(int(seed) & 0xFFFFFFFFFFFFFFFF, float(prob), int(built)))


def selfplay_prelude_host(rng, fast_search_prob):
    """oakgpu_selfplay_prelude_host (no GPU): the start of one turn on a game's stream, by the rule both game loops compile.  Returns
    (use_fast, search_seed, rng advanced)."""
    state, fast, seed = C.c_uint64(int(rng)), C.c_int32(0), C.c_uint64(0)
    _lib.check(_lib.load().oakgpu_selfplay_prelude_host(C.byref(state), float(fast_search_prob), C.byref(fast), C.byref(seed)))
    return bool(fast.value), int(seed.value), int(state.value)


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
