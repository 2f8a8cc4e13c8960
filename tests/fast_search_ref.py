"""The turn rule of fast searches, restated in Python (oak_amd/csrc/selfplay_pick.hpp: turn_prelude; generate.cc:292-299) on the streams of
tests/forestplay_ref.py.  A turn takes from the game's stream, in order: with fast_search_prob > 0 one uniform draw (the turn is fast when it is
below the probability), the search seed, and the two draws of the pick -- whatever the policies are, so a game's flags follow from its
seed alone."""
import forestplay_ref as R


def turn_prelude(state, fast_search_prob):
    """(new state, use_fast, search seed)"""
    fast = False
    if fast_search_prob > 0:
        state, u = R.uniform01(state)
        fast = u < fast_search_prob
    state, seed = R.splitmix64(state)
    return state, fast, seed


def turn_budget(fast, iterations, fast_budget):
    return fast_budget if fast and fast_budget else iterations


def fast_flags(seed, fast_search_prob, turns):
    """The flags of a game's first `turns` turns."""
    state, out = R.game_stream(seed), []
    for _ in range(turns):
        state, fast, _ = turn_prelude(state, fast_search_prob)
        state, _ = R.splitmix64(state)   # the pick: one uniform per side
        state, _ = R.splitmix64(state)
        out.append(fast)
    return out


def mixing(seeds, fast_search_prob, turns):
    """(some turn index below `turns` has fast and full games side by side, some game has both kinds within its first `turns` turns)"""
    flags = [fast_flags(int(s), fast_search_prob, turns) for s in seeds]
    by_turn = any(len({f[t] for f in flags}) == 2 for t in range(turns))
    by_game = any(len(set(f)) == 2 for f in flags)
    return by_turn, by_game
