"""GPU: matches between two search agents over the forest search (oak_amd/csrc/forestmatch.hip; contract in include/oakgpu.h), held to the
referee in tests/forest_match_ref.py, which replays every game with standalone searches:
  1. UCB seats with different agents: every game is the referee's, three of them also with the HOST tree search in the forest's place;
  2. PUCB + net_tiny against UCB + PokeEngine with unequal policy options and the Nash solve;
  3. the seats are not interchangeable;
  4. a game does not depend on n, its neighbours, the forest or earlier calls; n = 1; terminal inputs come back at turn 0;
  5. the early stop: which games, when, as which result;
  6. max_turns;
  7. a zeroed policy stops its game alone;
  8. the pyoak, C++ and torch faces return the C call's bytes."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import forest_match_ref as M
from oak_amd.arena import search_games
from policy_games_ref import BOUNDARY_EPS
from test_oracle_goldens import benchmark_teams

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = 400           # log capacity per game: above every game length met here (asserted where it matters)
_CACHE = {}

PE16 = dict(iterations=16, bandit="ucb", c=2.0, evaluator="poke-engine")
PE8 = dict(PE16, iterations=8)
MC8 = dict(iterations=8, bandit="ucb", c=2.0, evaluator="mc")


def openings(ctx, n, salt=0):
    """n games from the benchmark team pair's opening state (battle seeds differ) and their seeds; game 5 (when there is one) is game 2 again."""
    teams = np.stack([np.array(benchmark_teams(), dtype=np.uint8).reshape(60)] * n)
    battle_seeds = (np.arange(n, dtype=np.uint64) * np.uint64(0x2545F4914F6CDD1D) + np.uint64(9000 + salt)).astype(np.uint64)
    seeds = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(23 + salt)).astype(np.uint64)
    if n > 5:
        battle_seeds[5], seeds[5] = battle_seeds[2], seeds[2]
    b, d, r = ctx.battle(teams, battle_seeds)
    return b, d, r, seeds


def network(ctx, tmp_path, name):
    from test_gpu_search_forest import network as load
    return load(ctx, tmp_path, name)


def same(a, b, rows_a=None, rows_b=None):
    """The per-game outputs of two calls, row for row."""
    ra = slice(None) if rows_a is None else rows_a
    rb = slice(None) if rows_b is None else rows_b
    return all(a[k][ra].tobytes() == b[k][rb].tobytes() for k in ("results", "turns", "status", "log"))


def counts_of(out):
    res, st = out["results"], out["status"]
    scored = (st == M.OK) | (st == M.EARLY_STOP)
    return (int((scored & ((res & 15) == 1)).sum()), int((scored & ((res & 15) == 3)).sum()), int((scored & ((res & 15) == 2)).sum()), int((st == M.MAX_TURNS).sum()))


# ---- 1. UCB seats, different agents --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairing, n", [("pe16-mc8", 12), ("tiny-int8", 5)])
def test_ucb_games_are_the_referees(gpu_ctx, tmp_path, pairing, n):
    nets = []
    if pairing == "pe16-mc8":
        seats = (PE16, MC8)
    else:
        nets = [network(gpu_ctx, tmp_path, "tiny"), network(gpu_ctx, tmp_path, "default_int8")]
        seats = (dict(iterations=8, bandit="ucb", c=2.0, evaluator=nets[0]), dict(iterations=8, bandit="ucb", c=2.0, evaluator=nets[1], policy_mode="e0.9-x0.1"))
    b, d, r, seeds = openings(gpu_ctx, n)
    stats = {}
    t0 = time.time()
    out = search_games(gpu_ctx, seats, b, d, r, seeds, log_turns=LOG, stats=stats)
    t1 = time.time()
    assert int(out["turns"].max()) < LOG and (out["status"] == M.OK).all() and out["counts"] == counts_of(out)
    census = M.follow(gpu_ctx, seats, b, d, r, seeds, out)
    t2 = time.time()
    host = M.follow(gpu_ctx, seats, b, d, r, seeds, out, games=[0, 1, n - 1], host=True)      # anchored to the host search
    print("%s: %d games, %d turns; match %.2f s, referee %.2f s, host referee %.2f s; stats %s census %s" %
          (pairing, n, int(out["turns"].sum()), t1 - t0, t2 - t1, time.time() - t2, stats, census))
    assert host["turns"] == int(out["turns"][[0, 1, n - 1]].sum())
    row_turns = int(out["turns"].sum())
    assert census["turns"] == row_turns and (stats["p1_rows"], stats["p2_rows"]) == (census["p1_rows"], census["p2_rows"])
    assert census["m1"] > 0 and census["n1"] > 0, census                          # a forced switch after a faint: one seat is not searched
    assert stats["p1_rows"] + stats["p2_rows"] < 2 * row_turns
    assert stats["turns"] == int(out["turns"].max()) and stats["host_reads"] == stats["turns"] + 1
    if n > 5:
        assert same(out, out, [5], [2])
    for net in nets:
        net.close()


# ---- 2. PUCB against UCB, unequal options ----------------------------------------------------------------------------------------------
def test_pucb_against_ucb_with_unequal_options(gpu_ctx, tmp_path):
    n = 6
    net = network(gpu_ctx, tmp_path, "tiny")
    seats = (dict(iterations=8, bandit="pucb", c=1.5, evaluator=net, policy_mode="p0.5-n0.5"),
             dict(PE16, policy_mode="x", policy_temp=0.5))
    b, d, r, seeds = openings(gpu_ctx, n, salt=1)
    out = search_games(gpu_ctx, seats, b, d, r, seeds, log_turns=LOG, solve_nash=True)
    assert int(out["turns"].max()) < LOG and (out["status"] == M.OK).all()
    census = M.follow(gpu_ctx, seats, b, d, r, seeds, out, boundary_eps=BOUNDARY_EPS)
    print("pucb against ucb: %d turns, census %s" % (int(out["turns"].sum()), census))
    assert census["checked"] + census["excluded"] == census["p1_rows"] + census["p2_rows"]
    assert census["excluded"] <= 0.02 * (census["checked"] + census["excluded"])
    net.close()


# ---- 3. the seats are not interchangeable -------------------------------------------------------------------------------------------------
def test_swapped_agents_play_other_games(gpu_ctx):
    n = 5
    b, d, r, seeds = openings(gpu_ctx, n, salt=2)
    one = search_games(gpu_ctx, (PE16, MC8), b, d, r, seeds, log_turns=LOG)
    two = search_games(gpu_ctx, (MC8, PE16), b, d, r, seeds, log_turns=LOG)
    M.follow(gpu_ctx, (MC8, PE16), b, d, r, seeds, two)
    assert not same(one, two) and one["log"].tobytes() != two["log"].tobytes()
    with pytest.raises(AssertionError):
        M.follow(gpu_ctx, (PE16, MC8), b, d, r, seeds, two, games=[0])


# ---- 4. independence ----------------------------------------------------------------------------------------------------------------------
N4 = 300


def reference(ctx):
    """300 games at budget 8, PokeEngine against PokeEngine: more than one 256-row block, not a multiple of 64.  Played once, shared."""
    if "ref" not in _CACHE:
        b, d, r, seeds = openings(ctx, N4, salt=3)
        stats = {}
        t0 = time.time()
        out = search_games(ctx, (PE8, dict(PE8, policy_mode="e0.9-x0.1")), b, d, r, seeds, log_turns=LOG, stats=stats)
        print("reference: %d games, %d turns, lengths %d..%d in %.2f s; stats %s" % (N4, int(out["turns"].sum()), out["turns"].min(), out["turns"].max(),
                                                                                     time.time() - t0, stats))
        _CACHE["ref"] = (b, d, r, seeds, out)
    return _CACHE["ref"]


def test_a_game_does_not_depend_on_its_neighbours_the_forest_or_earlier_calls(gpu_ctx):
    from oak_amd.search import Forest
    b, d, r, seeds, out = reference(gpu_ctx)
    seats = (PE8, dict(PE8, policy_mode="e0.9-x0.1"))
    assert int(out["turns"].max()) < LOG and (out["status"] == M.OK).all() and out["counts"] == counts_of(out) and sum(out["counts"]) == N4
    assert same(out, out, [5], [2]) and len(set(out["log"][g].tobytes() for g in range(N4))) > N4 // 2
    turns = out["turns"]
    sample = [0, 2, 63, 64, 255, 256, 299, int(np.argmax(turns)), int(np.argmin(turns))]
    M.follow(gpu_ctx, seats, b, d, r, seeds, out, games=[255, 256, 299])
    for g in sample[:4]:                                                        # alone: n = 1
        one = search_games(gpu_ctx, seats, b[g:g + 1], d[g:g + 1], r[g:g + 1], seeds[g:g + 1], log_turns=LOG)
        assert same(one, out, [0], [g]), g
    rows = np.array(sample[2:9])                                                # n = 7, other neighbours, another order
    seven = search_games(gpu_ctx, seats, b[rows], d[rows], r[rows], seeds[rows], log_turns=LOG)
    assert same(seven, out, None, rows)
    big = Forest(gpu_ctx, 64, 32)                                               # a larger forest, after an unrelated call on it
    search_games(gpu_ctx, (MC8, PE16), b[:9], d[:9], r[:9], seeds[:9] + np.uint64(99), forest=big, max_turns=6)
    rows = np.array(sample[:7])
    again = search_games(gpu_ctx, seats, b[rows], d[rows], r[rows], seeds[rows], forest=big, log_turns=LOG)
    assert same(again, out, None, rows)
    big.close()


def test_terminal_inputs_come_back_at_turn_zero(gpu_ctx):
    b, d, r, seeds, out = reference(gpu_ctx)
    n = 9
    prng = (np.arange(n * 8, dtype=np.uint64) * np.uint64(37) + np.uint64(1)).astype(np.uint8).reshape(n, 8)
    done = gpu_ctx.rollout(b[:n].copy(), d[:n].copy(), r[:n].copy(), prng, max_steps=1000, return_state=True)
    assert ((done["results"] & 15) != 0).all()
    mb, md, mr = b[:n].copy(), d[:n].copy(), r[:n].copy()
    over = [1, 4, 8]
    mb[over], md[over], mr[over] = done["battles"][over], done["durations"][over], done["results"][over]
    seats = (PE8, dict(PE8, policy_mode="e0.9-x0.1"))
    got = search_games(gpu_ctx, seats, mb, md, mr, seeds[:n], log_turns=LOG)
    assert (got["turns"][over] == 0).all() and (got["results"][over] == mr[over]).all() and (got["status"][over] == M.OK).all()
    assert (got["log"][over].view(np.uint8) == 0xFF).all()
    rest = [g for g in range(n) if g not in over]
    assert same(got, out, rest, rest)
    all_over = search_games(gpu_ctx, seats, done["battles"], done["durations"], done["results"], seeds[:n], log_turns=4)
    assert (all_over["turns"] == 0).all() and (all_over["results"] == done["results"]).all() and sum(all_over["counts"][:3]) == n


# ---- 5. the early stop ----------------------------------------------------------------------------------------------------------------------
def late_states(ctx, b, d, r, back):
    """The states `back` steps before the end of a random playout of each game: a few Pokemon left a side.  (At budget 4 a seat visits its
    first four choices only -- from the opening those are switches, and such a game runs to the engine's turn-1,000 tie.)"""
    n = len(r)
    prng = (np.arange(n * 8, dtype=np.uint64) * np.uint64(41) + np.uint64(3)).astype(np.uint8).reshape(n, 8)
    full = ctx.rollout(b.copy(), d.copy(), r.copy(), prng.copy(), max_steps=1000)
    lb, ld, lr = b.copy(), d.copy(), r.copy()
    for g in range(n):
        k = max(int(full["steps"][g]) - back, 0)
        st = ctx.rollout(b[g:g + 1].copy(), d[g:g + 1].copy(), r[g:g + 1].copy(), prng[g:g + 1].copy(), max_steps=k, return_state=True)
        lb[g], ld[g], lr[g] = st["battles"][0], st["durations"][0], st["results"][0]
    return lb, ld, lr


def test_the_early_stop_is_the_referees(gpu_ctx):
    n, cap = 16, 40                              # (cut at `cap` turns: what a budget of 4 does not end by then it may never end)
    b, d, r, seeds = openings(gpu_ctx, n, salt=5)
    flip = np.stack([np.array(benchmark_teams(), dtype=np.uint8).reshape(2, 30)[::-1].reshape(60)] * n)
    fb, fd, fr = gpu_ctx.battle(flip, seeds ^ np.uint64(0xABCD))                  # the same pair with the teams swapped: seat p1 holds the other side
    odd = np.arange(n) % 2 == 1
    b[odd], d[odd], r[odd] = fb[odd], fd[odd], fr[odd]
    lb, ld, lr = late_states(gpu_ctx, b, d, r, back=6)                            # games 8 .. 15 start late in a playout of theirs
    b[8:], d[8:], r[8:] = lb[8:], ld[8:], lr[8:]
    assert ((r & 15) == 0).all()
    total = dict(early_win=0, early_lose=0, finished=0, ev01=0)
    pe, mc = dict(iterations=4, bandit="ucb", c=2.0, evaluator="poke-engine"), dict(iterations=4, bandit="ucb", c=2.0, evaluator="mc")
    for seats in ((pe, pe), (mc, mc)):
        name = seats[0]["evaluator"]
        out = search_games(gpu_ctx, seats, b, d, r, seeds, log_turns=LOG, early_stop=0.5, max_turns=cap)
        census = M.follow(gpu_ctx, seats, b, d, r, seeds, out, early_stop=0.5, max_turns=cap)
        print("early stop 0.5, %s seats: status %s results %s turns %s census %s" % (name, out["status"].tolist(), out["results"].tolist(), out["turns"].tolist(), census))
        assert out["counts"] == counts_of(out) and sum(out["counts"]) == n
        assert int((out["status"] == M.EARLY_STOP).sum()) == census["early_win"] + census["early_lose"]
        for k in total:
            total[k] += census[k]
        off = search_games(gpu_ctx, seats, b, d, r, seeds, log_turns=LOG, early_stop=0.0, max_turns=cap)
        assert (off["status"] != M.EARLY_STOP).all() and (off["turns"] >= out["turns"]).all()
        M.follow(gpu_ctx, seats, b, d, r, seeds, off, games=[0, 9], max_turns=cap)
    assert all(v > 0 for v in total.values()), total   # a stop each way, a game played to its end, a searched ev of exactly 0 or 1


# ---- 6. max_turns --------------------------------------------------------------------------------------------------------------------------
def test_max_turns_cuts_every_game(gpu_ctx):
    n = 9
    b, d, r, seeds = openings(gpu_ctx, n, salt=6)
    out = search_games(gpu_ctx, (PE8, MC8), b, d, r, seeds, log_turns=8, max_turns=5)
    assert (out["status"] == M.MAX_TURNS).all() and ((out["results"] & 15) == 0).all() and (out["turns"] == 5).all()
    assert out["counts"] == (0, 0, 0, n)
    census = M.follow(gpu_ctx, (PE8, MC8), b, d, r, seeds, out, max_turns=5)
    assert census["cut"] == n and census["turns"] == 5 * n


# ---- 7. a zeroed policy ----------------------------------------------------------------------------------------------------------------------
def test_a_zeroed_policy_stops_its_game_alone(gpu_ctx):
    n, cap = 16, 3
    b, d, r, seeds = openings(gpu_ctx, n, salt=7)
    # 16 iterations over p1's nine choices: a policy whose largest entry is 2 / 16 falls under the cut whole, one with a 3 / 16 survives it.
    # Playouts' values (0 or 1) draw the visits together in some games and leave them flat in others.
    seats = (dict(iterations=16, bandit="ucb", c=2.0, evaluator="mc", policy_min=0.15), PE8)
    out = search_games(gpu_ctx, seats, b, d, r, seeds, log_turns=LOG, max_turns=cap)
    census = M.follow(gpu_ctx, seats, b, d, r, seeds, out, max_turns=cap)
    print("policy_min 0.15: status %s turns %s census %s" % (out["status"].tolist(), out["turns"].tolist(), census))
    zeroed = out["status"] == M.ZERO_POLICY
    assert zeroed.any() and not zeroed.all(), out["status"]
    assert (out["results"][zeroed] == 0xFF).all() and out["counts"] == counts_of(out) and sum(out["counts"]) == n - int(zeroed.sum())
    rest = np.flatnonzero(~zeroed)                                               # the others are the games they are without their neighbours
    alone = search_games(gpu_ctx, seats, b[rest], d[rest], r[rest], seeds[rest], log_turns=LOG, max_turns=cap)
    assert same(alone, out, None, rest)


# ---- 8. faces --------------------------------------------------------------------------------------------------------------------------------
def test_pyoak_face_equals_the_c_call(gpu_ctx):
    from oak_amd import pyoak
    n = 7
    b, d, r, seeds = openings(gpu_ctx, n, salt=8)
    want = search_games(gpu_ctx, (dict(PE8, c=1.0), dict(MC8, c=1.0, iterations=4, policy_mode="e0.9-x0.1")), b, d, r, seeds, log_turns=LOG, early_stop=10.0)
    a1, a2 = pyoak.Agent(), pyoak.Agent()
    a1.budget, a1.bandit, a1.eval = "8", "ucb-1.0", "fp"
    a2.budget, a2.bandit, a2.eval = "4", "ucb-1.0", "mc"
    got = pyoak.match_forest(b, d, r, seeds, a1, a2, policy_p1="e", policy_p2="e0.9-x0.1", early_stop=10.0, log_turns=LOG)
    for k in ("results", "turns", "status", "log"):
        assert np.asarray(got[k]).tobytes() == want[k].tobytes(), k
    assert tuple(got["counts"]) == want["counts"]
    bad = pyoak.Agent()
    bad.budget, bad.bandit, bad.eval = "10ms", "ucb-1.0", "mc"
    with pytest.raises(RuntimeError, match="seat p2: .*time budgets"):
        pyoak.match_forest(b, d, r, seeds, a1, bad)
    with pytest.raises(RuntimeError, match="seat p1: policy mode 'b'"):
        pyoak.match_forest(b, d, r, seeds, a1, a2, policy_p1="b")


def test_cpp_face_equals_the_c_call(tmp_path):
    exe = str(tmp_path / "cpp_forest_match_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_forest_match_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "forest match == c call" in out.stdout and out.stdout.strip().endswith("ok"), out.stdout


def test_torch_face_in_a_child_process():
    """search_games with torch tensors on the device, through tests/forest_match_torch_check.py in a child process -- torch must initialise
    the GPU before the library does."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forest_match_torch_check.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "forest match torch ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
