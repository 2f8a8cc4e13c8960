"""GPU: self-play over the forest search (oak_amd/csrc/forestplay.hip; contract in include/oakgpu.h) -- a batch of games resident on the device.
  1. UCB games are the host loop's: record bytes, frame count and result equal selfplay_game(batch=1, seed=seeds[g]) for every evaluator;
  2. PUCB + net_tiny games replay OK, and frame by frame the stored fields are a standalone forest_search's output on the state the replay
     reaches, compressed, the stored choice the restatement's pick from it (tests/forestplay_ref.py);
  3. a game does not depend on n, on its neighbours, on the compaction schedule, on the forest's capacity or on earlier calls;
  4. max_battle_length drops exactly the longer games and leaves the others' records alone;
  5. solve_nash = 0 changes nothing but the nash fields, which are 0;
  6. policy_temp = 0.5 (the device's pow): every pick is the restatement's but for draws within BOUNDARY_EPS of a cumulative boundary;
  7. the pyoak, C++ and torch faces return the C call's bytes."""
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

import forestplay_ref as R
from oak_amd.frames import forest_selfplay, replay_check, replay_index, selfplay_game
from policy_games_ref import BOUNDARY_EPS, boundary_distance
from test_oracle_goldens import benchmark_teams

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, MAX_LENGTH, ZERO_POLICY = 0, 1, 2
_CACHE = {}


def games(n, salt=0):
    """teams [n, 60] (the benchmark pair), battle seeds and policy seeds of n games; game 5 (when there is one) is game 2 over again."""
    teams = np.stack([np.array(benchmark_teams(), dtype=np.uint8).reshape(60)] * n)
    battle_seeds = (np.arange(n, dtype=np.uint64) * np.uint64(0x2545F4914F6CDD1D) + np.uint64(7000 + salt)).astype(np.uint64)
    seeds = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(11 + salt)).astype(np.uint64)
    if n > 5:
        battle_seeds[5], seeds[5] = battle_seeds[2], seeds[2]
    return teams, battle_seeds, seeds


def records(out):
    """The per-game byte strings of a forest_selfplay result."""
    stream, offsets = out[0], out[1]
    return [stream[int(offsets[g]):int(offsets[g + 1])] for g in range(len(offsets) - 1)]


def network(ctx, tmp_path, name):
    from test_gpu_search_forest import network as load
    return load(ctx, tmp_path, name)


# ---- 1. UCB: the host loop, byte for byte ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["e", "e0.5-n0.5", "e0.9-x0.1"])
@pytest.mark.parametrize("evaluator, n, iterations", [("poke-engine", 12, 16), ("mc", 5, 8), ("tiny", 5, 8), ("default_int8", 5, 8)])
def test_ucb_games_are_the_host_loops(gpu_ctx, tmp_path, evaluator, n, iterations, mode):
    teams, battle_seeds, seeds = games(n)
    ev = evaluator if evaluator in ("mc", "poke-engine") else network(gpu_ctx, tmp_path, evaluator)
    stats = {}
    t0 = time.time()
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=2.0, evaluator=ev, policy_mode=mode, solve_nash=True, stats=stats)
    t1 = time.time()
    recs = records(out)
    assert (out[4] == OK).all(), out[4]                                        # no game is dropped
    for g in range(n):
        want = selfplay_game(gpu_ctx, teams[g], int(battle_seeds[g]), iterations=iterations, batch=1, c=2.0, evaluator=ev, policy_mode=mode,
                             seed=int(seeds[g]))
        assert recs[g] == want[0], (g, len(recs[g]), len(want[0]))
        assert (int(out[2][g]), int(out[3][g])) == want[1:], g
    print("%s %s: %d games, %d frames; forest loop %.2f s, host loop %.2f s; stats %s" % (evaluator, mode, n, int(out[2].sum()), t1 - t0, time.time() - t1, stats))
    assert stats["rows"] == int(out[2].sum()) and stats["host_reads"] == stats["turns"] + 1 and stats["turns"] == int(out[2].max())
    if n > 5:
        assert recs[5] == recs[2]
    if not isinstance(ev, str):
        ev.close()


# ---- 2. and 6.: held to a standalone search on the replayed state --------------------------------------------------------------------
def follow(ctx, out, seeds, iterations, search_kw, mode, temp=1.0, minp=0.0, exact_picks=True):
    """Turn by turn over every kept game: the state after t stored updates (the replay check's walk over the record cut to t frames), one
    forest_search over those states with the seeds of the restatement's chain, and the stored update against that output: every field, and
    the choice the restatement picks from it.  Returns (picks checked, picks left out near a boundary)."""
    from oak_amd.search import forest_search
    recs = records(out)
    n = len(recs)
    kept = [g for g in range(n) if out[4][g] == OK]
    updates = {g: R.split_updates(recs[g]) for g in kept}
    state = {g: R.game_stream(int(seeds[g])) for g in kept}
    checked = excluded = 0
    for t in range(max(len(u) for u in updates.values())):
        live = [g for g in kept if len(updates[g]) > t]
        blob = b"".join(struct.pack("<IH", R.HEAD_BYTES + sum(map(len, updates[g][:t])), t) + recs[g][6:R.HEAD_BYTES] + b"".join(updates[g][:t]) for g in live)
        rep = replay_check(ctx, blob, want_states=True)
        assert (rep["reports"]["status"] == 4).all() and (rep["reports"]["frame"] == t).all(), (t, rep["reports"])   # RESULT: not over yet
        tree_seeds = []
        for g in live:
            state[g], s = R.splitmix64(state[g])
            tree_seeds.append(s)
        res = forest_search(ctx, rep["battles"], rep["durations"], rep["reports"]["got"].astype(np.uint8), np.array(tree_seeds, dtype=np.uint64), iterations,
                            solve_nash=True, **search_kw)
        for q, g in enumerate(live):
            raw = res[q]["raw"]
            vis, val = np.array(raw.visit_matrix, dtype=np.uint64).reshape(9, 9), np.array(raw.value_matrix).reshape(9, 9)
            p = R.pick(raw.m, raw.n, vis, val, iterations, state[g], p1_nash=list(raw.p1_nash), p2_nash=list(raw.p2_nash), nash_value=raw.nash_value,
                       p1_prior=list(raw.p1_prior), p2_prior=list(raw.p2_prior), p1_choices=list(raw.p1_choices), p2_choices=list(raw.p2_choices),
                       mode=mode, temp=temp, minp=minp)
            assert p is not None, (g, t)
            state[g] = p["rng"]
            stored = updates[g][t]
            assert stored[:1] + stored[3:] == p["update"][:1] + p["update"][3:], (g, t)      # m, n, iterations, the empirical and nash fields
            near = min(boundary_distance(np.array(p["p1_policy"][:raw.m]), p["u1"]), boundary_distance(np.array(p["p2_policy"][:raw.n]), p["u2"])) <= BOUNDARY_EPS
            if not exact_picks and near:
                excluded += 1
                assert stored[1] in raw.p1_choices[:raw.m] and stored[2] in raw.p2_choices[:raw.n], (g, t)
            else:
                checked += 1
                assert stored[1:3] == p["update"][1:3], (g, t, stored[1:3], p["update"][1:3], p["u1"], p["u2"])
    return checked, excluded


def test_pucb_games_follow_a_standalone_search(gpu_ctx, tmp_path):
    n, iterations = 6, 8
    teams, battle_seeds, seeds = games(n, salt=1)
    net = network(gpu_ctx, tmp_path, "tiny")
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=1.5, bandit="pucb", evaluator=net, policy_mode="p0.5-n0.5", solve_nash=True)
    assert (out[4] == OK).all()
    rep = replay_check(gpu_ctx, out[0])
    assert len(rep["reports"]) == n and (rep["reports"]["status"] == 0).all() and rep["stopped_at"] == len(out[0])
    t0 = time.time()
    checked, excluded = follow(gpu_ctx, out, seeds, iterations, dict(c=1.5, bandit="pucb", evaluator=net), "p0.5-n0.5")
    print("pucb: %d games, %d frames, %d picks checked in %.2f s" % (n, int(out[2].sum()), checked, time.time() - t0))
    assert checked == int(out[2].sum()) and excluded == 0
    net.close()


def test_a_temperature_pick_is_the_restatements_but_near_a_boundary(gpu_ctx):
    n, iterations = 8, 8
    teams, battle_seeds, seeds = games(n, salt=2)
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=2.0, evaluator="poke-engine", policy_mode="e0.5-n0.5", policy_temp=0.5,
                          policy_min=0.05, solve_nash=True)
    assert (out[4] == OK).all()
    checked, excluded = follow(gpu_ctx, out, seeds, iterations, dict(c=2.0, evaluator="poke-engine"), "e0.5-n0.5", temp=0.5, minp=0.05, exact_picks=False)
    print("temp 0.5, min 0.05: %d picks checked, %d left out within %g of a boundary" % (checked, excluded, BOUNDARY_EPS))
    assert checked + excluded == int(out[2].sum()) and excluded <= 0.01 * (checked + excluded)


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------
N3, BUDGET3 = 300, 8


def reference(ctx):
    """300 games at budget 8, poke-engine, mode e: more than one 256-row block, not a multiple of 64.  Played once, shared."""
    if "ref" not in _CACHE:
        teams, battle_seeds, seeds = games(N3, salt=3)
        stats = {}
        t0 = time.time()
        out = forest_selfplay(ctx, teams, battle_seeds, seeds, BUDGET3, c=2.0, evaluator="poke-engine", policy_mode="e", solve_nash=True, stats=stats)
        print("reference: %d games, %d frames, lengths %d..%d in %.2f s; stats %s" % (N3, int(out[2].sum()), out[2].min(), out[2].max(), time.time() - t0, stats))
        _CACHE["ref"] = (teams, battle_seeds, seeds, out, records(out))
    return _CACHE["ref"]


def test_a_game_does_not_depend_on_its_neighbours_the_forest_or_earlier_calls(gpu_ctx):
    from oak_amd.search import Forest
    teams, battle_seeds, seeds, out, recs = reference(gpu_ctx)
    stream, offsets, n_frames, results, status = out
    assert (status == OK).all()
    idx = replay_index(stream)
    assert idx["stopped_at"] == len(stream) and len(idx["offsets"]) == N3 and not idx["malformed"].any()
    assert (idx["offsets"] == offsets[:-1]).all() and int(offsets[-1]) == len(stream)
    assert (idx["frames"] == n_frames).all() and int(n_frames.sum()) == int(idx["frames"].astype(np.int64).sum())
    assert all(recs[g][R.HEAD_BYTES - 1] == results[g] and (results[g] & 15) in (1, 2, 3) for g in range(N3))
    assert recs[5] == recs[2] and len(set(recs)) > N3 // 2
    kw = dict(c=2.0, evaluator="poke-engine", policy_mode="e", solve_nash=True)
    sample = [0, 2, 63, 64, 255, 256, 299, int(np.argmax(n_frames)), int(np.argmin(n_frames))]
    for g in sample[:5]:                                                        # alone
        one = forest_selfplay(gpu_ctx, teams[g:g + 1], battle_seeds[g:g + 1], seeds[g:g + 1], BUDGET3, **kw)
        assert one[0] == recs[g] and int(one[2][0]) == n_frames[g] and one[3][0] == results[g] and one[4][0] == OK, g
    rows = np.array(sample[2:9])                                                # n = 7, other neighbours, another order
    seven = forest_selfplay(gpu_ctx, teams[rows], battle_seeds[rows], seeds[rows], BUDGET3, **kw)
    assert records(seven) == [recs[g] for g in rows] and (seven[2] == n_frames[rows]).all() and (seven[3] == results[rows]).all()
    big = Forest(gpu_ctx, 64, 32)                                               # a larger forest, after an unrelated call on it
    forest_selfplay(gpu_ctx, teams[:9], battle_seeds[:9] + np.uint64(99), seeds[:9], 20, forest=big, c=1.0, evaluator="mc", policy_mode="e0.9-x0.1")
    rows = np.array(sample[:7])
    again = forest_selfplay(gpu_ctx, teams[rows], battle_seeds[rows], seeds[rows], BUDGET3, forest=big, **kw)
    assert records(again) == [recs[g] for g in rows] and (again[2] == n_frames[rows]).all()
    big.close()


# ---- 4. dropping -------------------------------------------------------------------------------------------------------------------
def test_the_length_cap_drops_the_longer_games_and_nothing_else(gpu_ctx):
    teams, battle_seeds, seeds, out, recs = reference(gpu_ctx)
    cap = int(np.median(out[2]))
    got = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET3, c=2.0, evaluator="poke-engine", policy_mode="e", solve_nash=True, max_battle_length=cap)
    stream, offsets, n_frames, results, status = got
    dropped = out[2] > cap                                                      # (a game of exactly `cap` frames is kept)
    assert dropped.any() and not dropped.all()
    assert (status[dropped] == MAX_LENGTH).all() and (status[~dropped] == OK).all()
    mine = records(got)
    for g in range(N3):
        assert mine[g] == (b"" if dropped[g] else recs[g]), g
    assert (n_frames[~dropped] == out[2][~dropped]).all() and (results[~dropped] == out[3][~dropped]).all()
    idx = replay_index(stream)
    assert idx["stopped_at"] == len(stream) and len(idx["offsets"]) == int((~dropped).sum())


# ---- 5. solve_nash = 0 ---------------------------------------------------------------------------------------------------------------
def test_without_the_nash_solve_only_the_nash_fields_change(gpu_ctx):
    teams, battle_seeds, seeds, out, recs = reference(gpu_ctx)
    got = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET3, c=2.0, evaluator="poke-engine", policy_mode="e", solve_nash=False)
    assert (got[1] == out[1]).all() and (got[2] == out[2]).all() and (got[3] == out[3]).all() and (got[4] == OK).all()
    some_nash = 0
    for g, (mine, theirs) in enumerate(zip(records(got), recs)):
        assert mine[:R.HEAD_BYTES] == theirs[:R.HEAD_BYTES], g
        for a, b in zip(R.split_updates(mine), R.split_updates(theirs)):
            m, n = (b[0] & 15) + 1, (b[0] >> 4) + 1
            want = bytearray(b)
            want[9:11] = b"\0\0"                                                  # the nash value
            want[11 + 2 * m:11 + 4 * m] = bytes(2 * m)                          # P1's nash policy
            want[11 + 4 * m + 2 * n:] = bytes(2 * n)                            # P2's
            some_nash += bytes(want) != b
            assert a == bytes(want), g
    assert some_nash > 0
    with pytest.raises(RuntimeError, match="word 'n' needs solve_nash"):
        forest_selfplay(gpu_ctx, teams[:2], battle_seeds[:2], seeds[:2], BUDGET3, evaluator="poke-engine", policy_mode="e0.5-n0.5", solve_nash=False)


# ---- 7. faces ----------------------------------------------------------------------------------------------------------------------
def test_pyoak_face_equals_the_c_call(gpu_ctx):
    from oak_amd import pyoak
    n, iterations = 7, 8
    teams, battle_seeds, seeds = games(n, salt=4)
    want = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=1.0, evaluator="poke-engine", policy_mode="e0.9-x0.1")
    agent = pyoak.Agent()
    agent.budget, agent.bandit, agent.eval = str(iterations), "ucb-1.0", "fp"
    got = pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, policy_mode="e0.9-x0.1")
    assert got[0] == want[0] and all((np.asarray(a) == b).all() for a, b in zip(got[1:], want[1:]))
    for text, kw in (("time budgets", dict(budget="10ms")), ("Exp3", dict(bandit="exp3-0.1"))):
        bad = pyoak.Agent()
        bad.budget, bad.bandit, bad.eval = str(iterations), "ucb-1.0", "mc"
        for k, v in kw.items():
            setattr(bad, k, v)
        with pytest.raises(RuntimeError, match=text):
            pyoak.selfplay_forest(teams, battle_seeds, seeds, bad)
    with pytest.raises(RuntimeError, match="policy mode 'b'"):
        pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, policy_mode="b")


def test_cpp_face_equals_the_c_call_and_the_host_loop(tmp_path):
    exe = str(tmp_path / "cpp_forest_selfplay_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_forest_selfplay_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "forest selfplay == c call == host loop" in out.stdout and out.stdout.strip().endswith("ok"), out.stdout


def test_torch_face_in_a_child_process():
    """forest_selfplay with torch tensors on the device, through tests/forest_selfplay_torch_check.py in a child process -- torch must
    initialise the GPU before the library does."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forest_selfplay_torch_check.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "forest selfplay torch ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
