"""The inert-standstill proof (tests/inert_ref.py, the restatement of EngineR::inert_standstill) against the CPU oracle, which plays
every turn: a state the predicate accepts must, turn-step after turn-step, change nothing but the turn counter, battle.rng by exactly
the predicted number of draws, and a frozen side's freely chosen last-selected move / last-move index."""
import numpy as np

import inert_ref as R
import oracle_lib as O


def _accepted():
    b, d, p, res, total, fres = R.harvest()
    verdict = [R.inert(b[i], d[i], int(res[i])) for i in range(len(b))]
    return b, d, p, res, total, fres, verdict


def test_fixture_holds_stalemates_and_negatives():
    b, d, p, res, total, fres, verdict = _accepted()
    stalemate = total >= 999
    print("states %d, stalemates %d, ordinary %d, accepted %d" % (len(b), int(stalemate.sum()), int((~stalemate).sum()),
                                                                  sum(v is not None for v in verdict)))
    assert stalemate.sum() >= 135 and (~stalemate).sum() >= 100   # (half of what the oracle gives: 271 and 218)


def test_accepted_states_never_end_before_turn_1000_and_cover_the_stalemates():
    b, d, p, res, total, fres, verdict = _accepted()
    acc = np.array([v is not None for v in verdict])
    stalemate = total >= 999
    print("accepted %d of %d stalemates (%.1f %%); accepted non-stalemates %d" % (int((acc & stalemate).sum()), int(stalemate.sum()),
          100.0 * (acc & stalemate).sum() / stalemate.sum(), int((acc & ~stalemate).sum())))
    assert not (acc & ~stalemate).any(), "an accepted state ended before turn 1,000"
    assert (acc & stalemate).sum() >= 0.85 * stalemate.sum()
    forms = {"rage": 0, "struggle": 0, "frozen_free": 0, "frozen_locked": 0, "equal_speed_rage_pair": 0, "par": 0}
    for i in np.where(acc)[0]:
        c, (f1, f2) = verdict[i]
        x, y = R.side_view(b[i], d[i], 0), R.side_view(b[i], d[i], 1)
        for f in {f1, f2}:
            forms[f] += 1
        forms["equal_speed_rage_pair"] += f1 == f2 == "rage" and x["spe"] == y["spe"]
        forms["par"] += (f1 in ("rage", "struggle") and x["status"] == R.PAR) or (f2 in ("rage", "struggle") and y["status"] == R.PAR)
    print("forms among the accepted states:", forms)
    # (each bound: at most half of what the oracle gives in this fixture, printed above)
    assert all(n >= 8 for n in forms.values()), forms


def test_forty_oracle_steps_change_nothing_but_turn_rng_and_a_free_choice():
    b, d, p, res, total, fres, verdict = _accepted()
    idx = np.array([i for i, v in enumerate(verdict) if v is not None])
    cb, cd, cp, cr = b[idx].copy(), d[idx].copy(), p[idx].copy(), res[idx].copy()
    draws = [verdict[i][0] for i in idx]
    free = [[s for s in range(2) if verdict[i][1][s] == "frozen_free"] for i in idx]
    for step in range(40):
        pb = cb.copy()
        out, st = O.rollout_batch(cb, cd, cr, cp, max_steps=1, threads=8)
        assert (st == 1).all() and (out == R.RUNNING).all(), step
        assert (cd == d[idx]).all(), step
        for k in range(len(idx)):
            allowed = {R.TURN, R.TURN + 1} | set(range(R.RNG, R.RNG + 8))
            for s in free[k]:
                allowed |= {s * R.SIDE + R.LAST_SEL, R.LAST_MOVES + 2 * s}
            changed = set(np.where(pb[k] != cb[k])[0].tolist())
            assert changed <= allowed, (int(idx[k]), step, sorted(changed - allowed), verdict[idx[k]])
            assert R.u16(cb[k], R.TURN) == R.u16(pb[k], R.TURN) + 1
            was, now = int(pb[k, R.RNG:R.RNG + 8].view(np.uint64)[0]), int(cb[k, R.RNG:R.RNG + 8].view(np.uint64)[0])
            assert now == R.lcg(was, draws[k]), (int(idx[k]), step, draws[k], verdict[idx[k]])
