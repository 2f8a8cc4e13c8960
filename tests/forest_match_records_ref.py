"""A referee for the `.battle.data` records of a match between two search agents (include/oakgpu.h: oakgpu_forest_match_records), written
from the contract's text on forestplay_ref's encode_update / assemble_record:

  searched_entry / unsearched_entry : one seat's update of one turn -- its own root output with the turn's joint choice, or (a seat with one
                                      choice, not searched) the real m and n, iterations 0 and zero fields
  reference_unsearched_entry        : what the reference stores there instead (a value-initialised MCTS::Output: head byte 0xFF, 11 bytes),
                                      kept to show that no reader parses it
  seat_record / pack                : a seat's record of one game (none for a cut or zeroed game), and the stream, offsets and frame counts
                                      of a batch
  follow_records                    : forest_match_ref.follow with its standalone searches kept, so that the outputs it computes also give
                                      both seats' expected streams (GPU)"""
import numpy as np

import forest_match_ref as M
import forestplay_ref as R

ZEROS = [0.0] * 9


def _pad(a):
    return list(ZEROS) if a is None else ([float(x) for x in a] + ZEROS)[:9]


def searched_entry(m, n, c1, c2, iterations, visits, values, nash_value=0.0, p1_nash=None, p2_nash=None):
    """A searched seat's update: m, n, the joint choice, the search's iterations, empirical_value, nash_value, and both sides' empirical
    (process_output) and Nash strategies."""
    ev, e1, e2, _ = R.process_output(visits, values, m, n, iterations)
    return R.encode_update(m, n, c1, c2, iterations, ev, nash_value, e1, _pad(p1_nash), e2, _pad(p2_nash))


def unsearched_entry(m, n, c1, c2):
    return R.encode_update(m, n, c1, c2, 0, 0.0, 0.0, ZEROS, ZEROS, ZEROS, ZEROS)


def reference_unsearched_entry(c1, c2):
    """Update::write of a value-initialised output (m = n = 0): (0 - 1) | (0 - 1) << 4 is 0xFF in a byte, no strategy follows."""
    return bytes([0xFF, c1, c2]) + bytes(8)


def turn_entries(turn):
    """Both seats' updates of one counted turn: {"m", "n", "c1", "c2", "out": (p1's output | None, p2's output | None)}, an output being the
    keyword arguments of searched_entry after the joint choice."""
    m, n, c1, c2 = turn["m"], turn["n"], turn["c1"], turn["c2"]
    entries = []
    for s in (0, 1):
        o = turn["out"][s]
        if (n if s else m) == 1:
            assert o is None, "a seat with one choice is not searched"
            entries.append(unsearched_entry(m, n, c1, c2))
        else:
            entries.append(searched_entry(m, n, c1, c2, **o))
    return entries


def seat_record(seat, battle, status, result, turns):
    """Seat `seat`'s record of one game from its input battle, the call's status and result byte, and the counted turns (an early-stop or
    zeroed turn is not among them).  b"" for a game cut at max_turns or stopped by a zeroed policy.  An early stop's result byte is 1 or 2."""
    if status in (M.MAX_TURNS, M.ZERO_POLICY):
        return b""
    if status == M.EARLY_STOP:
        assert result in (M.WIN, M.LOSE)
    return R.assemble_record(battle, result, [turn_entries(t)[seat] for t in turns])


def pack(records):
    """(stream, offsets uint64[n + 1]) of records in game order."""
    offsets = np.zeros(len(records) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in records])
    return b"".join(records), offsets


def follow_records(ctx, seats, battles, durations, results, seeds, out, max_turns=1000, early_stop=0.0, solve_nash=True, host=False):
    """forest_match_ref.follow over every game of the call `out` (which asserts each game, its log included), with the standalone searches it
    runs kept by tree seed; then every game is walked again through its verified log -- the stream, the seeds in the stated order, the picks
    -- to pair each searched turn with its search's output.  Returns (census, (p1, p2)), each seat a dict of stream, offsets and n_frames;
    the census gains `both` (turns with both seats searched) and first_unsearched = [games whose first frame seat p1 / p2 did not search]."""
    kept = {}
    inner = M._searches

    def keeping(ctx_, seat, b, d, r, tree_seeds, solve, host_):
        got = inner(ctx_, seat, b, d, r, tree_seeds, solve, host_)
        for seed, o in zip(tree_seeds, got):
            assert int(seed) not in kept, "two trees drew one seed"
            kept[int(seed)] = o
        return got

    M._searches = keeping
    try:
        census = M.follow(ctx, seats, battles, durations, results, seeds, out, max_turns=max_turns, early_stop=early_stop, solve_nash=solve_nash, host=host)
    finally:
        M._searches = inner
    b = np.ascontiguousarray(battles, dtype=np.uint8).reshape(-1, 384)
    n = len(seeds)
    records = ([], [])
    census.update(both=0, first_unsearched=[0, 0])
    for g in range(n):
        state, turns = R.game_stream(int(seeds[g])), []
        for t in range(int(out["turns"][g])):
            rec = out["log"][g][t]
            m, n_, c1, c2 = int(rec["m"]), int(rec["n"]), int(rec["c1"]), int(rec["c2"])
            found = [None, None]
            for s in (0, 1):                     # seat p1's seed first, then seat p2's
                if (n_ if s else m) > 1:
                    state, seed = R.splitmix64(state)
                    found[s] = kept[seed]["raw"]
            outs = [None, None]
            for s in (0, 1):
                raw = found[s]
                if raw is None:
                    continue
                seat = seats[s]
                vis, val = np.array(raw.visit_matrix, dtype=np.uint64).reshape(9, 9), np.array(raw.value_matrix).reshape(9, 9)
                nash = (list(raw.p2_nash) if s else list(raw.p1_nash)) if solve_nash else None
                p = M.seat_pick(s, m, n_, vis, val, seat["iterations"], state, nash=nash, prior=list(raw.p2_prior) if s else list(raw.p1_prior),
                                mode=seat.get("policy_mode", "e"), temp=seat.get("policy_temp", 1.0), minp=seat.get("policy_min", 0.0), early_stop=early_stop)
                state = p["rng"]
                assert int(raw.iterations) == seat["iterations"], (g, t, s)
                outs[s] = dict(iterations=int(raw.iterations), visits=vis, values=val,
                               nash_value=float(raw.nash_value) if solve_nash else 0.0, p1_nash=list(raw.p1_nash) if solve_nash else None,
                               p2_nash=list(raw.p2_nash) if solve_nash else None)
            turns.append(dict(m=m, n=n_, c1=c1, c2=c2, out=tuple(outs)))
            census["both"] += m > 1 and n_ > 1
            if t == 0:
                census["first_unsearched"][0] += m == 1
                census["first_unsearched"][1] += n_ == 1
        for s in (0, 1):
            records[s].append(seat_record(s, b[g], int(out["status"][g]), int(out["results"][g]), turns))
    seats_out = []
    for s in (0, 1):
        stream, offsets = pack(records[s])
        seats_out.append(dict(stream=stream, offsets=offsets, n_frames=np.asarray(out["turns"], dtype=np.uint32).copy()))
    return census, tuple(seats_out)
