"""A float64 referee for matches between two search agents (include/oakgpu.h: oakgpu_forest_match*), written from the contract's text:

  seat_pick / early_stop_sign : ONE seat's pick and early-stop sign from one root output, on forestplay_ref's splitmix64, process_output,
                                get_policy and sample_pdf; tests/test_forest_match_ref.py holds oakgpu_match_pick_host to it bit for bit
  follow                      : replays games from their input states through ctx.update; per turn the seeds in the stated order, a
                                STANDALONE search per seat over the rows that seat must search, the picks, and the comparison with the
                                call's turn_log, status, result and turn count

Python floats are IEEE doubles and every sum runs in the stated order, so with policy_temp = 1 every number here is the library's."""
import math

import numpy as np

import forestplay_ref as R

OK, MAX_TURNS, ZERO_POLICY, EARLY_STOP = 0, 1, 2, 3
WIN, LOSE = 1, 2


def _ln(x):
    """C's log on the whole line: -inf at 0, NaN below."""
    return -math.inf if x == 0 else math.nan if x < 0 else math.log(x)


def early_stop_sign(ev, early_stop):
    """+1 when t >= 1, -1 when t <= -1, else 0, with t = (log(ev) - log(1 - ev)) / early_stop; early_stop = 0 is off."""
    if not early_stop > 0:
        return 0
    t = (_ln(ev) - _ln(1.0 - ev)) / early_stop
    return 1 if t >= 1.0 else -1 if t <= -1.0 else 0


def seat_pick(side, m, n, visits, values, iterations, state, nash=None, prior=None, mode="e", temp=1.0, minp=0.0, early_stop=0.0):
    """One seat (side 0 = p1, 1 = p2) from one root output; nash / prior are that side's.  None for a zeroed policy (nothing drawn), else a
    dict: policy, index, empirical_value, sign, rng (advanced), u (the uniform drawn)."""
    pad = lambda a: [0.0] * 9 if a is None else ([float(x) for x in a] + [0.0] * 9)[:9]
    ev, e1, e2, _ = R.process_output(visits, values, m, n, iterations)
    k = n if side else m
    pol = R.get_policy(pad(prior), e2 if side else e1, pad(nash), k, R.parse_mode(mode), temp if temp > 0 else 1.0, minp)
    if pol is None:
        return None
    state, index, u = R.sample_pdf(pol, k, state)
    return {"policy": pol, "index": index, "empirical_value": ev, "sign": early_stop_sign(ev, early_stop), "rng": state, "u": u}


def _search_kw(seat):
    return dict(c=seat.get("c", 2.0), bandit=seat.get("bandit", "ucb"), evaluator=seat.get("evaluator", "mc"), max_depth=seat.get("max_depth", 0),
                root_rolls=seat.get("root_rolls", 3), other_rolls=seat.get("other_rolls", 1))


def _searches(ctx, seat, battles, durations, results, seeds, solve_nash, host):
    """The standalone searches of one seat's rows: the forest search (one call, tree k = row k), or the host tree search with batch = 1."""
    from oak_amd.search import forest_search, tree_search
    kw = _search_kw(seat)
    if not host:
        return forest_search(ctx, battles, durations, results, np.array(seeds, dtype=np.uint64), seat["iterations"], solve_nash=solve_nash, **kw)
    kw["max_depth"] = kw["max_depth"] or 100
    return [tree_search(ctx, battles[q], durations[q], int(results[q]), iterations=seat["iterations"], batch=1, seed=int(seeds[q]), **kw)
            for q in range(len(seeds))]


def follow(ctx, seats, battles, durations, results, seeds, out, games=None, max_turns=1000, early_stop=0.0, solve_nash=True, host=False,
           boundary_eps=None):
    """Replays games `games` (default: all) of a search_games call `out` (numpy, with a log that holds every turn) and asserts that each is
    the game the contract states.  The replay follows the LOGGED choices after checking them, so a pick left out near a cumulative boundary
    (boundary_eps: the distance below which a seat with policy_temp != 1 may differ, the device's pow) does not end the comparison.
    Returns the census of the referee's own walk: turns, p1_rows, p2_rows (rows searched), m1 (turns with m = 1 < n), n1 (n = 1 < m), ev01
    (searched ev exactly 0 or 1), checked / excluded picks, early_win, early_lose, finished, zeroed, cut."""
    from policy_games_ref import boundary_distance
    games = list(range(len(seeds))) if games is None else list(games)
    log = out["log"]
    b = np.ascontiguousarray(battles, dtype=np.uint8).reshape(-1, 384)[games].copy()
    d = np.ascontiguousarray(durations, dtype=np.uint8).reshape(-1, 8)[games].copy()
    r = np.ascontiguousarray(results, dtype=np.uint8).reshape(-1)[games].copy()
    state = [R.game_stream(int(seeds[g])) for g in games]
    turns = [0] * len(games)
    end = {}                                     # slot -> (status, result)
    census = dict(turns=0, p1_rows=0, p2_rows=0, m1=0, n1=0, ev01=0, checked=0, excluded=0, early_win=0, early_lose=0, finished=0, zeroed=0, cut=0)
    while True:
        for q in range(len(games)):
            if q in end:
                continue
            if r[q] & 15:
                end[q] = (OK, int(r[q]))
                census["finished"] += 1
            elif turns[q] >= max_turns:
                end[q] = (MAX_TURNS, int(r[q]))
                census["cut"] += 1
        live = [q for q in range(len(games)) if q not in end]
        if not live:
            break
        lb, ld, lr = np.ascontiguousarray(b[live]), np.ascontiguousarray(d[live]), np.ascontiguousarray(r[live])
        ch = [ctx.choices(lb, lr, 0), ctx.choices(lb, lr, 1)]
        count = [ch[0][1].astype(int), ch[1][1].astype(int)]
        tree_seed = [[None] * len(live), [None] * len(live)]
        for i, q in enumerate(live):             # seat p1 first, then seat p2; a seat with one choice draws nothing
            for s in (0, 1):
                if count[s][i] > 1:
                    state[q], tree_seed[s][i] = R.splitmix64(state[q])
        res = [[None] * len(live), [None] * len(live)]
        for s in (0, 1):
            rows = [i for i in range(len(live)) if count[s][i] > 1]
            census["p1_rows" if s == 0 else "p2_rows"] += len(rows)
            if rows:
                got = _searches(ctx, seats[s], lb[rows], ld[rows], lr[rows], [tree_seed[s][i] for i in rows], solve_nash, host)
                for i, o in zip(rows, got):
                    res[s][i] = o
        c = np.zeros((2, len(live)), np.uint8)
        stepped = []
        for i, q in enumerate(live):
            g, t = games[q], turns[q]
            m, n = count[0][i], count[1][i]
            census["turns"] += 1
            census["m1"] += int(m == 1 < n)
            census["n1"] += int(n == 1 < m)
            ev, sign, picks, zero = [0.0, 0.0], [0, 0], [None, None], False
            for s in (0, 1):
                if res[s][i] is None:            # not searched: its single choice, ev 0, sign 0
                    picks[s] = int(ch[s][0][i][0])
                    continue
                raw = res[s][i]["raw"]
                assert (raw.m, raw.n) == (m, n), (g, t)
                vis, val = np.array(raw.visit_matrix, dtype=np.uint64).reshape(9, 9), np.array(raw.value_matrix).reshape(9, 9)
                seat = seats[s]
                nash = (list(raw.p2_nash) if s else list(raw.p1_nash)) if solve_nash else None
                p = seat_pick(s, m, n, vis, val, seat["iterations"], state[q], nash=nash, prior=list(raw.p2_prior) if s else list(raw.p1_prior),
                              mode=seat.get("policy_mode", "e"), temp=seat.get("policy_temp", 1.0), minp=seat.get("policy_min", 0.0), early_stop=early_stop)
                if p is None:
                    zero = True
                    break
                state[q] = p["rng"]
                ev[s], sign[s] = p["empirical_value"], p["sign"]
                census["ev01"] += ev[s] in (0.0, 1.0)
                legal = list(raw.p2_choices if s else raw.p1_choices)[:n if s else m]
                picks[s] = (legal[p["index"]], legal, boundary_distance(np.array(p["policy"][:len(legal)]), p["u"]))
            if zero:
                end[q] = (ZERO_POLICY, 0xFF)
                census["zeroed"] += 1
                continue
            rec = log[g][t]
            assert (int(rec["m"]), int(rec["n"]), int(rec["zero"])) == (m, n, 0), (g, t, rec)
            assert (float(rec["ev_p1"]), float(rec["ev_p2"])) == (ev[0], ev[1]), (g, t, rec, ev)
            if sign[0] * sign[1] > 0:
                assert (int(rec["c1"]), int(rec["c2"])) == (0, 0), (g, t, rec)
                end[q] = (EARLY_STOP, WIN if sign[0] > 0 else LOSE)
                census["early_win" if sign[0] > 0 else "early_lose"] += 1
                continue
            for s, name in ((0, "c1"), (1, "c2")):
                stored = int(rec[name])
                if isinstance(picks[s], tuple):
                    want, legal, dist = picks[s]
                    loose = boundary_eps is not None and seats[s].get("policy_temp", 1.0) != 1.0 and dist <= boundary_eps
                    if loose:
                        census["excluded"] += 1
                        assert stored in legal, (g, t, name, stored, legal)
                    else:
                        census["checked"] += 1
                        assert stored == want, (g, t, name, stored, want, dist)
                else:
                    assert stored == picks[s], (g, t, name, stored, picks[s])
                c[s][i] = stored
            stepped.append(i)
        if stepped:
            sb, sd = np.ascontiguousarray(lb[stepped]), np.ascontiguousarray(ld[stepped])
            sr, _ = ctx.update(sb, c[0][stepped], c[1][stepped], sd, want_actions=False)
            for j, i in enumerate(stepped):
                q = live[i]
                b[q], d[q], r[q] = sb[j], sd[j], sr[j]
                turns[q] += 1
    for q, g in enumerate(games):
        status, result = end[q]
        assert (int(out["status"][g]), int(out["results"][g]), int(out["turns"][g])) == (status, result, turns[q]), \
            (g, out["status"][g], out["results"][g], out["turns"][g], status, result, turns[q])
        if log.shape[1] > turns[q] + 1:          # entries the game does not reach are not written
            tail = log[g][turns[q] + (1 if status == EARLY_STOP else 0):]
            assert (tail.view(np.uint8) == 0xFF).all(), g
    return census
