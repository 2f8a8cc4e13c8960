"""GPU: fast searches in self-play (oakgpu_selfplay_params: fast_budget, fast_search_prob, fast_policy_mode; the rule is selfplay_pick.hpp's
turn_prelude) -- the host loop is the referee of the device loop.
  1. UCB games of forest_selfplay equal selfplay_game's with the same fast fields, bytes, frame count and result, for every evaluator, and on a
     kept forest with keep_node, nodes_kept included; every frame's iterations are what the restatement of the game's stream dictates, and
     fast and full turns do stand side by side;
  2. PUCB games are held frame by frame to a standalone budgets search on the replayed state, that frame's budget and mode;
  3. probability 0 gives the bytes of a call without the fields, probability 1 those of the host loop at the fast budget and mode;
  4. the counters: launched == run tree-iterations, fast + full frames == the frames written; the loader with min_iterations = fast_budget + 1
     draws full-budget frames only, as many eligible as the full-frame counter says;
  5. a game does not depend on its neighbours or the forest;
  6. the pyoak and C++ faces equal the C call."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fast_search_ref as F
import forestplay_ref as R
from oak_amd.frames import forest_selfplay, replay_check, selfplay_game
from test_gpu_forest_selfplay import OK, games, network, records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# evaluator, games, budget, fast budget, probability (tests/test_fast_search_ref.py checks on the CPU that these games' seeds mix the two kinds)
CASES = [("poke-engine", 12, 16, 4, 0.5), ("mc", 5, 8, 2, 0.5), ("tiny", 5, 8, 2, 0.5), ("default_int8", 5, 8, 2, 0.5)]
MODES = dict(policy_mode="e0.5-n0.5", fast_policy_mode="x")
_CACHE = {}


def stored_iterations(record):
    return [struct.unpack_from("<I", u, 3)[0] for u in R.split_updates(record)]


def check_iterations(recs, seeds, iterations, fast_budget, prob):
    """every frame's iterations against the restatement of its game's stream; returns (fast frames, full frames) and asserts the mixing"""
    fast = full = 0
    turns = {}
    for g, rec in enumerate(recs):
        got = stored_iterations(rec)
        flags = F.fast_flags(int(seeds[g]), prob, len(got))
        assert got == [F.turn_budget(f, iterations, fast_budget) for f in flags], g
        fast += sum(flags)
        full += len(flags) - sum(flags)
        for t, f in enumerate(flags):
            turns.setdefault(t, set()).add(f)
    assert any(len(v) == 2 for v in turns.values())                               # fast and full rows in one turn's search
    assert any(len(set(stored_iterations(rec))) == 2 for rec in recs)             # and both kinds within one game
    return fast, full


# ---- 1. UCB: the host loop, byte for byte ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("evaluator, n, iterations, fast_budget, prob", CASES)
def test_ucb_games_with_fast_searches_are_the_host_loops(gpu_ctx, tmp_path, evaluator, n, iterations, fast_budget, prob):
    teams, battle_seeds, seeds = games(n)
    ev = evaluator if evaluator in ("mc", "poke-engine") else network(gpu_ctx, tmp_path, evaluator)
    fast_kw = dict(fast_budget=fast_budget, fast_search_prob=prob, **MODES)
    stats = {}
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=2.0, evaluator=ev, solve_nash=True, stats=stats, **fast_kw)
    recs = records(out)
    assert (out[4] == OK).all(), out[4]
    for g in range(n):
        want = selfplay_game(gpu_ctx, teams[g], int(battle_seeds[g]), iterations=iterations, batch=1, c=2.0, evaluator=ev, seed=int(seeds[g]), **fast_kw)
        assert recs[g] == want[0], (g, len(recs[g]), len(want[0]))
        assert (int(out[2][g]), int(out[3][g])) == want[1:], g
    fast, full = check_iterations(recs, seeds, iterations, fast_budget, prob)
    print(evaluator, "frames fast / full", fast, full, stats)
    assert (stats["fast_frames"], stats["full_frames"]) == (fast, full) and fast + full == int(out[2].sum())
    assert stats["launched"] == stats["run"] == fast * fast_budget + full * iterations
    assert stats["host_reads"] == stats["turns"] + 1 and stats["loop_copies"] == stats["loop_syncs"]
    if evaluator == "poke-engine":
        _CACHE["pe"] = (teams, battle_seeds, seeds, out, recs, stats)
    if not isinstance(ev, str):
        ev.close()


def test_keep_node_games_with_fast_searches_are_the_host_loops(gpu_ctx):
    n, iterations, fast_budget, prob = 12, 16, 4, 0.5
    teams, battle_seeds, seeds = games(n)
    fast_kw = dict(fast_budget=fast_budget, fast_search_prob=prob, **MODES)
    stats = {}
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=2.0, evaluator="poke-engine", solve_nash=True, keep_node=True, stats=stats, **fast_kw)
    recs = records(out)
    assert (out[4] == OK).all() and stats["dropped"] == 0
    for g in range(n):
        host = {}
        want = selfplay_game(gpu_ctx, teams[g], int(battle_seeds[g]), iterations=iterations, batch=1, c=2.0, evaluator="poke-engine", seed=int(seeds[g]),
                             keep_node=True, stats=host, **fast_kw)
        assert recs[g] == want[0] and (int(out[2][g]), int(out[3][g])) == want[1:], g
        assert int(out[5][g]) == host["nodes_kept"], g
    assert out[5].sum() > 0
    fast, full = check_iterations(recs, seeds, iterations, fast_budget, prob)
    assert stats["launched"] == stats["run"] == fast * fast_budget + full * iterations


# ---- 2. PUCB: held to a standalone budgets search on the replayed state ----------------------------------------------------------------
def test_pucb_games_with_fast_searches_follow_a_standalone_search(gpu_ctx, tmp_path):
    from oak_amd.search import forest_search
    n, iterations, fast_budget, prob = 6, 8, 2, 0.5
    modes = {False: "p0.5-n0.5", True: "e0.5-n0.5"}
    teams, battle_seeds, seeds = games(n, salt=1)
    net = network(gpu_ctx, tmp_path, "tiny")
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=1.5, bandit="pucb", evaluator=net, policy_mode=modes[False], solve_nash=True,
                          fast_budget=fast_budget, fast_search_prob=prob, fast_policy_mode=modes[True])
    assert (out[4] == OK).all()
    rep = replay_check(gpu_ctx, out[0])
    assert len(rep["reports"]) == n and (rep["reports"]["status"] == 0).all()
    recs = records(out)
    updates = {g: R.split_updates(recs[g]) for g in range(n)}
    state = {g: R.game_stream(int(seeds[g])) for g in range(n)}
    checked, kinds = 0, set()
    for t in range(max(len(u) for u in updates.values())):
        live = [g for g in range(n) if len(updates[g]) > t]
        blob = b"".join(struct.pack("<IH", R.HEAD_BYTES + sum(map(len, updates[g][:t])), t) + recs[g][6:R.HEAD_BYTES] + b"".join(updates[g][:t]) for g in live)
        rep = replay_check(gpu_ctx, blob, want_states=True)
        assert (rep["reports"]["status"] == 4).all() and (rep["reports"]["frame"] == t).all()
        tree_seeds, fast = [], []
        for g in live:
            state[g], f, s = F.turn_prelude(state[g], prob)
            tree_seeds.append(s)
            fast.append(f)
        budgets = np.array([F.turn_budget(f, iterations, fast_budget) for f in fast], np.uint32)
        res = forest_search(gpu_ctx, rep["battles"], rep["durations"], rep["reports"]["got"].astype(np.uint8), np.array(tree_seeds, dtype=np.uint64), iterations,
                            solve_nash=True, c=1.5, bandit="pucb", evaluator=net, budgets=budgets)
        for q, g in enumerate(live):
            raw = res[q]["raw"]
            assert raw.iterations == budgets[q]
            vis, val = np.array(raw.visit_matrix, dtype=np.uint64).reshape(9, 9), np.array(raw.value_matrix).reshape(9, 9)
            p = R.pick(raw.m, raw.n, vis, val, int(budgets[q]), state[g], p1_nash=list(raw.p1_nash), p2_nash=list(raw.p2_nash), nash_value=raw.nash_value,
                       p1_prior=list(raw.p1_prior), p2_prior=list(raw.p2_prior), p1_choices=list(raw.p1_choices), p2_choices=list(raw.p2_choices),
                       mode=modes[fast[q]])
            assert p is not None, (g, t)
            state[g] = p["rng"]
            assert updates[g][t] == p["update"], (g, t, fast[q])
            checked += 1
            kinds.add(fast[q])
    assert checked == int(out[2].sum()) and kinds == {False, True}
    net.close()


# ---- 3. the ends of the probability ----------------------------------------------------------------------------------------------------
def test_probability_zero_is_a_call_without_the_fields(gpu_ctx):
    teams, battle_seeds, seeds = games(7, salt=5)
    kw = dict(c=2.0, evaluator="poke-engine", policy_mode="e0.9-x0.1", solve_nash=True)
    plain = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, 8, **kw)
    stats = {}
    off = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, 8, fast_budget=2, fast_search_prob=0.0, fast_policy_mode="x", stats=stats, **kw)
    assert off[0] == plain[0] and all((a == b).all() for a, b in zip(off[1:], plain[1:]))
    assert stats["fast_frames"] == 0 and stats["full_frames"] == int(plain[2].sum()) and stats["launched"] == stats["run"] == 8 * int(plain[2].sum())
    host = selfplay_game(gpu_ctx, teams[3], int(battle_seeds[3]), iterations=8, batch=1, c=2.0, evaluator="poke-engine", policy_mode="e0.9-x0.1", seed=int(seeds[3]),
                         fast_budget=2, fast_search_prob=0.0, fast_policy_mode="x")
    assert host[0] == records(plain)[3]


def test_probability_one_is_the_host_loop_at_the_fast_budget_and_mode(gpu_ctx):
    teams, battle_seeds, seeds = games(7, salt=6)
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, 16, c=2.0, evaluator="poke-engine", policy_mode="e0.5-n0.5", solve_nash=True,
                          fast_budget=4, fast_search_prob=1.0, fast_policy_mode="e0.9-x0.1")
    recs = records(out)
    for g in range(7):   # the uniform game at 4 iterations and the fast mode; the host loop takes the turn's extra draw
        want = selfplay_game(gpu_ctx, teams[g], int(battle_seeds[g]), iterations=4, batch=1, c=2.0, evaluator="poke-engine", policy_mode="e0.9-x0.1",
                             seed=int(seeds[g]), fast_search_prob=1.0)
        assert recs[g] == want[0] and (int(out[2][g]), int(out[3][g])) == want[1:], g
        assert set(stored_iterations(recs[g])) == {4}


# ---- 4. counters and the loader's filter -------------------------------------------------------------------------------------------------
def test_the_loader_keeps_the_full_frames_only(gpu_ctx):
    from oak_amd.train import EncodedBattleFrames, FrameCorpus
    if "pe" not in _CACHE:
        n, iterations, fast_budget, prob = CASES[0][1:]
        teams, battle_seeds, seeds = games(n)
        stats = {}
        out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=2.0, evaluator="poke-engine", solve_nash=True, stats=stats,
                              fast_budget=fast_budget, fast_search_prob=prob, **MODES)
        _CACHE["pe"] = (teams, battle_seeds, seeds, out, records(out), stats)
    teams, battle_seeds, seeds, out, recs, stats = _CACHE["pe"]
    iterations, fast_budget = CASES[0][2], CASES[0][3]
    eligible = sum(sum(1 for it in stored_iterations(rec) if it >= fast_budget + 1) for rec in recs)
    assert eligible == stats["full_frames"] and stats["fast_frames"] + stats["full_frames"] == int(out[2].sum())
    corpus = FrameCorpus(gpu_ctx, out[0])
    enc = EncodedBattleFrames(512)
    assert corpus.sample(enc, seed=3, min_iterations=fast_budget + 1) == 512
    assert (enc.iterations[:, 0] == iterations).all()
    assert corpus.sample(enc, seed=3, min_iterations=1) == 512
    assert set(np.unique(enc.iterations[:, 0]).tolist()) == {fast_budget, iterations}
    corpus.close()


# ---- 5. independence -----------------------------------------------------------------------------------------------------------------------
def test_a_game_with_fast_searches_does_not_depend_on_its_neighbours_or_the_forest(gpu_ctx):
    from oak_amd.search import Forest
    teams, battle_seeds, seeds = games(300, salt=3)
    kw = dict(c=2.0, evaluator="poke-engine", solve_nash=True, fast_budget=2, fast_search_prob=0.6, **MODES)
    stats = {}
    ref = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, 8, stats=stats, **kw)       # more than one 256-row block: the partition crosses blocks
    recs = records(ref)
    assert (ref[4] == OK).all() and stats["launched"] == stats["run"]
    fast, full = check_iterations(recs, seeds, 8, 2, 0.6)
    assert (stats["fast_frames"], stats["full_frames"]) == (fast, full)
    sample = [0, 2, 63, 64, 255, 256, 299]
    g = 64
    one = forest_selfplay(gpu_ctx, teams[g:g + 1], battle_seeds[g:g + 1], seeds[g:g + 1], 8, **kw)
    assert one[0] == recs[g] and int(one[2][0]) == ref[2][g]
    rows = np.array(sample)
    seven = forest_selfplay(gpu_ctx, teams[rows], battle_seeds[rows], seeds[rows], 8, **kw)
    assert records(seven) == [recs[g] for g in rows] and (seven[2] == ref[2][rows]).all() and (seven[3] == ref[3][rows]).all()
    big = Forest(gpu_ctx, 64, 32)                                                       # a larger forest, after an unrelated call on it
    forest_selfplay(gpu_ctx, teams[:9], battle_seeds[:9] + np.uint64(99), seeds[:9], 20, forest=big, c=1.0, evaluator="mc", policy_mode="e0.9-x0.1")
    again = forest_selfplay(gpu_ctx, teams[rows], battle_seeds[rows], seeds[rows], 8, forest=big, **kw)
    assert records(again) == [recs[g] for g in rows]
    big.close()


def test_a_fast_budget_above_the_full_one_orders_the_fast_rows_first(gpu_ctx):
    teams, battle_seeds, seeds = games(12)
    stats = {}
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, 4, c=2.0, evaluator="poke-engine", solve_nash=True, stats=stats, fast_budget=16,
                          fast_search_prob=0.5, **MODES)
    recs = records(out)
    for g in (0, 7):
        want = selfplay_game(gpu_ctx, teams[g], int(battle_seeds[g]), iterations=4, batch=1, c=2.0, evaluator="poke-engine", seed=int(seeds[g]), fast_budget=16,
                             fast_search_prob=0.5, **MODES)
        assert recs[g] == want[0], g
    assert stats["launched"] == stats["run"] == 16 * stats["fast_frames"] + 4 * stats["full_frames"]


# ---- 6. faces --------------------------------------------------------------------------------------------------------------------------
def test_pyoak_face_with_fast_searches_equals_the_c_call(gpu_ctx):
    from oak_amd import pyoak
    n, iterations = 7, 8
    teams, battle_seeds, seeds = games(n, salt=4)
    fast_kw = dict(fast_budget=2, fast_search_prob=0.5, fast_policy_mode="x")
    want = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=1.0, evaluator="poke-engine", policy_mode="e0.9-x0.1", **fast_kw)
    agent = pyoak.Agent()
    agent.budget, agent.bandit, agent.eval = str(iterations), "ucb-1.0", "fp"
    got = pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, policy_mode="e0.9-x0.1", **fast_kw)
    assert got[0] == want[0] and all((np.asarray(a) == b).all() for a, b in zip(got[1:], want[1:]))
    assert len({it for rec in records(want) for it in stored_iterations(rec)}) == 2
    with pytest.raises(RuntimeError, match="fast_search_prob must be in"):
        pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, fast_search_prob=2.0)


def test_cpp_face_with_fast_searches_equals_the_c_call_and_the_host_loop(tmp_path):
    exe = str(tmp_path / "cpp_forest_fast_selfplay_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_forest_fast_selfplay_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
