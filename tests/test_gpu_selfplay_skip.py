"""GPU: matchup values and skipped battles in self-play over the forest search (oakgpu_forest_selfplay_build*, _matchup; the skip rule is
selfplay_pick.hpp's game_is_skipped, oakgpu_selfplay_skip_host on the host).  The call without the new fields and a standalone forest
search are the referees:
  (a) the skipped set is the host rule's;
  (b) a game that is not skipped has the record bytes, frame count, result and status of the same call with the new fields zero;
  (c) a skipped game has status SKIPPED, a zero-length slice, no frames, result byte 0 and a matchup equal bit for bit to the empirical
      value of a standalone search of the opening state with t1_budget iterations, seeded from the turn prelude on the game's stream;
  (d) a played game's matchup is the same standalone search at its own first-turn budget;
  (e) rows searched = the frames written + the games skipped;
  (f) probability 1 with every game built loops one turn and leaves an empty stream;
  (g) probability 1 with no game built is the plain call;
  (h) keep_node on a kept forest and fast searches, held to (b) and (c);
  (i) two calls give the same bits, and a game does not depend on its neighbours' built bits."""
import struct

import numpy as np
import pytest

import forestplay_ref as R
from oak_amd.frames import forest_selfplay, replay_check, selfplay_prelude_host, selfplay_skip_host
from test_gpu_forest_selfplay import OK, games, network, records

pytestmark = pytest.mark.gpu
SKIPPED = 3
BUDGET, T1_BUDGET, MAX_ITERATIONS, PROB = 8, 12, 16, 0.5
SALT = 0   # the seed base of games(): at n = 257 it gives >= 32 games of each kind (asserted below)
BANDITS = {"ucb": dict(c=2.0, bandit="ucb", evaluator="poke-engine", policy_mode="e0.9-x0.1"),
           "pucb": dict(c=1.5, bandit="pucb", evaluator="tiny", policy_mode="p0.5-n0.5")}


def built_bits(n):
    """none, p1, p2, both, in turn"""
    return (np.arange(n) % 4).astype(np.uint8)


def host_skips(seeds, built, prob):
    return np.array([selfplay_skip_host(int(s), prob, int(b)) for s, b in zip(seeds, built)], dtype=bool)


def opening_states(ctx, plain):
    """every game's state after the opening update: the replay check's walk over the plain call's records cut to no frame"""
    recs = records(plain)
    blob = b"".join(struct.pack("<IH", R.HEAD_BYTES, 0) + rec[6:R.HEAD_BYTES] for rec in recs)
    rep = replay_check(ctx, blob, want_states=True)
    assert (rep["reports"]["status"] == 4).all() and (rep["reports"]["frame"] == 0).all()
    return rep["battles"], rep["durations"], rep["reports"]["got"].astype(np.uint8)


def first_search_values(ctx, forest, states, seeds, budgets, fast_prob, search_kw):
    """process_output's empirical value of a standalone budgets search of each opening state, seeded from the turn prelude on the game's stream"""
    from oak_amd.search import forest_search
    tree_seeds = np.array([selfplay_prelude_host(R.game_stream(int(s)), fast_prob)[1] for s in seeds], dtype=np.uint64)
    res = forest_search(ctx, states[0], states[1], states[2], tree_seeds, MAX_ITERATIONS, forest=forest, budgets=np.asarray(budgets, np.uint32), **search_kw)
    assert all(int(r["raw"].iterations) == int(b) for r, b in zip(res, budgets))
    return np.array([r["raw"].empirical_value for r in res], dtype=np.float64)


def same_bits(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


def run_and_check(ctx, tmp_path, bandit, n, keep_node=False, fast=None, prob=PROB, built=None):
    """One plain call, one call with the new fields on the same forest, and (a) - (e).  Returns what the callers look at further."""
    from oak_amd.search import Forest
    kw = dict(BANDITS[bandit])
    net = network(ctx, tmp_path, kw["evaluator"]) if bandit == "pucb" else None
    if net is not None:
        kw["evaluator"] = net
    fast_kw = dict(fast_search_prob=fast[0], fast_budget=fast[1]) if fast else {}
    fast_prob, fast_budget = fast if fast else (0.0, 0)
    teams, battle_seeds, seeds = games(n, salt=SALT)
    built = built_bits(n) if built is None else built
    forest = Forest(ctx, n, MAX_ITERATIONS, contextual=bandit == "pucb", keep_arena=0 if keep_node else None)
    try:
        base = dict(forest=forest, solve_nash=True, keep_node=keep_node, **kw, **fast_kw)
        plain_stats, stats = {}, {}
        plain = forest_selfplay(ctx, teams, battle_seeds, seeds, BUDGET, stats=plain_stats, **base)
        out = forest_selfplay(ctx, teams, battle_seeds, seeds, BUDGET, stats=stats, built=built, battle_skip_prob=prob, t1_budget=T1_BUDGET, **base)
        want_skip = host_skips(seeds, built, prob)
        skipped = out[4] == SKIPPED
        assert (skipped == want_skip).all()                                                                  # (a)
        assert (plain[4] == OK).all()
        precs, recs = records(plain), records(out)
        for g in range(n):
            if skipped[g]:                                                                                   # (c)
                assert len(recs[g]) == 0 and out[2][g] == 0 and out[3][g] == 0, g
            else:                                                                                            # (b)
                assert recs[g] == precs[g] and out[2][g] == plain[2][g] and out[3][g] == plain[3][g] and out[4][g] == plain[4][g], g
                if keep_node:
                    assert out[5][g] == plain[5][g], g
        # (c), (d): the first search alone
        states = opening_states(ctx, plain)
        flags = np.array([selfplay_prelude_host(R.game_stream(int(s)), fast_prob)[0] for s in seeds], dtype=bool)
        own = np.where(flags & (fast_budget > 0), fast_budget, BUDGET)
        search_kw = dict(c=kw["c"], bandit=kw["bandit"], evaluator=kw["evaluator"])
        want = first_search_values(ctx, forest, states, seeds, np.where(skipped, T1_BUDGET, own), fast_prob, search_kw)
        assert not np.isnan(stats["matchup"]).any() and same_bits(stats["matchup"], want)
        want_plain = want if not skipped.any() else first_search_values(ctx, forest, states, seeds, own, fast_prob, search_kw)
        assert same_bits(plain_stats["matchup"], want_plain)
        if skipped.any() and not fast:
            assert not same_bits(stats["matchup"][skipped], plain_stats["matchup"][skipped])                 # (12 iterations are not 8)
        assert stats["rows"] == int(out[2].sum()) + int(skipped.sum())                                       # (e)
        assert plain_stats["rows"] == int(plain[2].sum())
        return dict(out=out, plain=plain, stats=stats, plain_stats=plain_stats, skipped=skipped, built=built, games=(teams, battle_seeds, seeds), base=kw)
    finally:
        forest.close()
        if net is not None:
            net.close()


def test_the_seed_base_mixes_the_three_kinds_of_game():
    _, _, seeds = games(257, salt=SALT)
    built = built_bits(257)
    skip = host_skips(seeds, built, PROB)
    assert skip.sum() >= 32 and ((built != 0) & ~skip).sum() >= 32 and (built == 0).sum() >= 32
    assert not skip[built == 0].any()


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("bandit", ["ucb", "pucb"])
def test_skipped_games_give_a_matchup_and_the_others_are_untouched(gpu_ctx, tmp_path, bandit, n):
    built = np.array([3], np.uint8) if n == 1 else None
    prob = 1.0 if n == 1 else PROB     # the one game is skipped
    r = run_and_check(gpu_ctx, tmp_path, bandit, n, prob=prob, built=built)
    assert r["skipped"].any()
    if n > 1:
        assert (~r["skipped"]).any() and (r["out"][2] > 0).any()


def test_one_game_that_is_not_skipped_is_the_plain_game(gpu_ctx, tmp_path):
    r = run_and_check(gpu_ctx, tmp_path, "ucb", 1, prob=PROB, built=np.array([0], np.uint8))
    assert not r["skipped"].any() and r["out"][0] == r["plain"][0]


def test_probability_one_with_every_game_built_loops_one_turn(gpu_ctx):                                     # (f)
    n = 65
    teams, battle_seeds, seeds = games(n, salt=SALT)
    stats = {}
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET, stats=stats, built=np.full(n, 1, np.uint8), battle_skip_prob=1.0, t1_budget=T1_BUDGET,
                          **BANDITS["ucb"])
    assert stats["turns"] == 1 and stats["rows"] == n and len(out[0]) == 0
    assert (out[1] == 0).all() and (out[2] == 0).all() and (out[3] == 0).all() and (out[4] == SKIPPED).all()
    assert not np.isnan(stats["matchup"]).any() and ((stats["matchup"] >= 0) & (stats["matchup"] <= 1)).all()
    assert stats["launched"] == stats["run"] == n * T1_BUDGET


def test_probability_one_with_no_game_built_is_the_plain_call(gpu_ctx):                                      # (g)
    n = 65
    teams, battle_seeds, seeds = games(n, salt=SALT)
    plain_stats, stats = {}, {}
    plain = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET, stats=plain_stats, **BANDITS["ucb"])
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET, stats=stats, built=np.zeros(n, np.uint8), battle_skip_prob=1.0, t1_budget=T1_BUDGET,
                          **BANDITS["ucb"])
    assert out[0] == plain[0] and all((a == b).all() for a, b in zip(out[1:], plain[1:]))
    assert same_bits(stats["matchup"], plain_stats["matchup"])
    none = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET, built=None, battle_skip_prob=1.0, t1_budget=T1_BUDGET, **BANDITS["ucb"])
    assert none[0] == plain[0] and all((a == b).all() for a, b in zip(none[1:], plain[1:]))


def test_keep_node_games_beside_skipped_ones(gpu_ctx, tmp_path):                                             # (h)
    r = run_and_check(gpu_ctx, tmp_path, "ucb", 65, keep_node=True)
    assert r["skipped"].any() and r["out"][5].sum() > 0 and (r["out"][5][r["skipped"]] == 0).all()


def test_fast_searches_beside_skipped_games(gpu_ctx, tmp_path):                                              # (h)
    r = run_and_check(gpu_ctx, tmp_path, "ucb", 65, fast=(0.5, 4))
    teams, battle_seeds, seeds = r["games"]
    first_fast = np.array([selfplay_prelude_host(R.game_stream(int(s)), 0.5)[0] for s in seeds], dtype=bool)
    assert (r["skipped"] & first_fast).any() and (r["skipped"] & ~first_fast).any()       # a skipped game's budget is t1_budget whatever the flag
    assert r["stats"]["launched"] >= r["stats"]["run"]                                    # (turn 1's rows are not sorted by budget)
    assert r["plain_stats"]["launched"] == r["plain_stats"]["run"]


def test_two_calls_give_the_same_bits_and_neighbours_do_not_matter(gpu_ctx, tmp_path):                       # (i)
    n = 65
    r = run_and_check(gpu_ctx, tmp_path, "ucb", n)
    teams, battle_seeds, seeds = r["games"]
    kw = dict(battle_skip_prob=PROB, t1_budget=T1_BUDGET, **BANDITS["ucb"])
    stats = {}
    again = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET, stats=stats, built=r["built"], **kw)
    assert again[0] == r["out"][0] and all((a == b).all() for a, b in zip(again[1:], r["out"][1:])) and same_bits(stats["matchup"], r["stats"]["matchup"])
    mine = np.array([0, 1, 2, 3, 31, 62, 63, 64])            # these keep their bits; every other game's are turned over
    other = np.where(r["built"] != 0, 0, 3).astype(np.uint8)
    other[mine] = r["built"][mine]
    stats2 = {}
    flipped = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET, stats=stats2, built=other, **kw)
    assert ((flipped[4] == SKIPPED) != r["skipped"]).any()
    a, b = records(flipped), records(r["out"])
    for g in mine:
        assert a[g] == b[g] and all(flipped[q][g] == r["out"][q][g] for q in (2, 3, 4)), g
    assert same_bits(stats2["matchup"][mine], r["stats"]["matchup"][mine])
    # a bit that differs within "built" (1, 2 or 3) changes nothing at all
    bits = np.where(r["built"] != 0, 4 - r["built"], 0).astype(np.uint8)
    stats3 = {}
    relabelled = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET, stats=stats3, built=bits, **kw)
    assert relabelled[0] == r["out"][0] and (relabelled[4] == r["out"][4]).all() and same_bits(stats3["matchup"], r["stats"]["matchup"])


def test_pyoak_face_skips_the_same_games(gpu_ctx):
    from oak_amd import pyoak
    n = 9
    teams, battle_seeds, seeds = games(n, salt=1)            # (games 6 and 7 of this base are skipped)
    built = built_bits(n)
    stats = {}
    want = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, BUDGET, c=1.0, evaluator="poke-engine", policy_mode="e0.9-x0.1", stats=stats, built=built,
                           battle_skip_prob=PROB, t1_budget=T1_BUDGET)
    agent = pyoak.Agent()
    agent.budget, agent.bandit, agent.eval = str(BUDGET), "ucb-1.0", "fp"
    got = pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, policy_mode="e0.9-x0.1", built=built, battle_skip_prob=PROB, t1_budget=T1_BUDGET, matchup=True)
    assert len(got) == 6 and got[0] == want[0] and all((np.asarray(a) == b).all() for a, b in zip(got[1:5], want[1:]))
    assert same_bits(got[5], stats["matchup"])
    assert (want[4] == SKIPPED).any() and (want[4] == OK).any()
    with pytest.raises(RuntimeError, match="battle_skip_prob must be in"):
        pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, built=built, battle_skip_prob=1.5)
