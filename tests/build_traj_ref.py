"""A numpy referee of the `.build.data` reader (oak_amd/csrc/build_traj.hpp, buildtraj.hip), written from the contract in include/oakgpu.h:
one record -> the seven arrays of the reference's Py::Build::Trajectories plus n_legal and a status, the two-stage draw, and the
network-free half of build.py's process_targets (valid, rows, get_state, old_logp, rewards).

Two decoders live here on purpose.  `decode` is the contract: lists built from Python lists the way the text describes them, a status where
the reference asserts or runs out of bounds, the last read step's action not applied.  `reference_write` is a literal restatement of
Py::Build::Trajectories::write, statement for statement, with no status and with a switch for applying the last action (a Python list grows
where the reference's std::array<SetHelper, 6> is written out of bounds): tests/test_build_traj_ref.py shows that the switch changes nothing
and that both agree with the reference's own arrays.  `mistake` plants one deliberate error by name in `decode`."""
import numpy as np

import build_ref as B

STEPS, MAX_ACTIONS, N_DIM, RECORD_BYTES = 31, B.MAX_ACTIONS, B.N_DIM, 128
OK, BAD_ACTION, NO_SPECIES, TEAM_FULL, NOT_LEGAL, LIST_OVERFLOW, N_STATUS = 0, 1, 2, 3, 4, 5, 6
STATUS_NAMES = ("OK", "BAD_ACTION", "NO_SPECIES", "TEAM_FULL", "NOT_LEGAL", "LIST_OVERFLOW")
F = np.float32
DEN = F(65535.0)
# old_logp is the device library's double log rounded to float once (include/oakgpu.h): the double log is within 3 ulp of double (OpenCL's
# bound), which is below 3 x 2^-29 ulp of float (ulp_f > |x| 2^-24), and the rounding adds half an ulp of float
OLD_LOGP_ULPS = 0.5 + 3 * 2.0 ** -29


def fields(record):
    r = np.frombuffer(bytes(record), np.uint8)
    assert r.size == RECORD_BYTES
    ups = r[4:].view("<u2").reshape(STEPS, 2)
    return int(r[0]), int(r[1]), int(r[2:4].view("<u2")[0]), ups[:, 0].astype(np.int64), ups[:, 1].astype(np.int64)


def is_none(action):
    return action < N_DIM and B.LIST[action][1] == 0


def bounds(action, prob):
    """start, end, swap, full as the loops of trajectories.h:159-187 take them."""
    start = full = swap = end = 0
    for i in range(STEPS):
        if prob[i] != 0:
            start = i
            break
    for i in range(STEPS - 1, -1, -1):
        if prob[i] != 0:
            none = is_none(int(action[i]))
            if end == 0:
                end = i + 1
                swap = end - (1 if none else 0)
            elif none:
                full = i + 1
                break
    return start, end, swap, full


class Helper:
    """TeamHelper / SetHelper: what is missing."""

    def __init__(self):
        self.sets = []                      # [species, remaining pool, counted moves]
        self.available = list(B.LEGAL)

    def fault(self, action):
        s, m = (int(x) for x in B.LIST[action])
        if m == 0:
            return TEAM_FULL if len(self.sets) >= 6 else OK
        return OK if any(x[0] == s for x in self.sets) else NO_SPECIES

    def apply(self, action):
        s, m = (int(x) for x in B.LIST[action])
        if m == 0:
            self.sets.append([s, list(B.POOLS[s]), 0])
            self.available = [x for x in self.available if x != s]
        else:
            st = next(x for x in self.sets if x[0] == s)
            if m in st[1]:
                st[1].remove(m)
                st[2] += 1

    @staticmethod
    def complete(st):
        return st[2] >= 4 or not st[1]

    def species(self):
        return [int(B.TABLE[s, 0]) for s in self.available]

    def moves(self):
        return [int(B.TABLE[st[0], m]) for st in self.sets if not self.complete(st) for m in st[1]]

    def swaps(self, mistake=None):
        sets = sorted(self.sets, key=lambda st: st[0]) if mistake == "swap_species_order" else self.sets
        return [int(B.TABLE[st[0], 0]) for st in sets]


def _values(score_byte, value_word, no_score):
    value = F(value_word) / DEN
    score = F(-1.0) if (no_score and score_byte == 255) else F(score_byte / 2.0)
    return value, score


def _ended(value, score, status):
    return {"action": -np.ones(STEPS, np.int64), "mask": -np.ones((STEPS, MAX_ACTIONS), np.int64), "n_legal": np.zeros(STEPS, np.uint16),
            "policy": np.zeros(STEPS, F), "value": value, "score": score, "start": 0, "end": 0, "status": status}


def decode(record, no_score=False, mistake=None):
    """One record by the contract.  A dict: action int64[31], mask int64[31, 339], n_legal uint16[31], policy f32[31], value, score, start,
    end, status."""
    _, score_byte, value_word, action, prob = fields(record)
    value, score = _values(score_byte, value_word, no_score)
    start, end, swap, full = bounds(action, prob)
    if any(int(action[i]) >= N_DIM for i in range(end)):
        return _ended(value, score, BAD_ACTION)
    out = _ended(value, score, OK)
    out["start"], out["end"] = start, end
    h = Helper()
    for i in range(end):
        a = int(action[i])
        if i >= start:
            if i < swap:
                row = (h.species() if (i < full or mistake == "species_past_full") else []) + h.moves()
            else:
                row = h.swaps(mistake)
            if len(row) > MAX_ACTIONS:
                return _ended(value, score, LIST_OVERFLOW)
            if a not in row:
                return _ended(value, score, NOT_LEGAL)
            if mistake != "action_not_moved":
                k = row.index(a)
                row[k], row[0] = row[0], row[k]
            out["action"][i], out["policy"][i], out["n_legal"][i] = a, F(prob[i]) / DEN, len(row)
            out["mask"][i, :len(row)] = row
        if i == end - 1 and mistake != "apply_last":
            break
        fault = h.fault(a)
        if fault != OK:
            return _ended(value, score, fault)
        h.apply(a)
    return out


def reference_write(record, apply_last=True):
    """Py::Build::Trajectories::write restated literally (no status: only for records on which the reference is defined, or -- in Python --
    harmlessly undefined).  The seven arrays of the reference, per record."""
    _, score_byte, value_word, action, prob = fields(record)
    start, end, swap, full = bounds(action, prob)
    out = {"action": np.zeros(STEPS, np.int64), "mask": np.zeros((STEPS, MAX_ACTIONS), np.int64), "policy": np.zeros(STEPS, F)}
    h = Helper()
    for i in range(STEPS):
        a = int(action[i])
        if i < start:
            out["action"][i], out["policy"][i] = -1, 0
            out["mask"][i] = -1
            h.apply(a)
        elif i < end:
            out["action"][i], out["policy"][i] = a, F(prob[i]) / DEN
            row = []
            if i < swap:
                if i < full:
                    row += h.species()
                row += h.moves()
            else:
                row += h.swaps()
            row = row + [-1] * (MAX_ACTIONS - len(row))
            k = row.index(a)
            row[k], row[0] = row[0], row[k]
            out["mask"][i] = row
            if apply_last or i != end - 1:
                h.apply(a)
        else:
            out["action"][i], out["policy"][i] = -1, 0
            out["mask"][i] = -1
    out["start"], out["end"] = start, end
    out["value"] = F(value_word) / DEN
    out["score"] = F(-1) if score_byte == 65535 else F(score_byte / 2.0)   # (an 8-bit score is never 65,535)
    return out


def decode_many(records, no_score=False):
    """records uint8[n, 128] -> the arrays stacked: action [n, 31], mask [n, 31, 339], ..., status uint8[n], t_max."""
    rows = [decode(r, no_score) for r in np.asarray(records, np.uint8).reshape(-1, RECORD_BYTES)]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in ("action", "mask", "n_legal", "policy")}
    out["value"], out["score"] = np.array([r["value"] for r in rows], F), np.array([r["score"] for r in rows], F)
    out["start"], out["end"] = np.array([r["start"] for r in rows], np.int64), np.array([r["end"] for r in rows], np.int64)
    out["status"] = np.array([r["status"] for r in rows], np.uint8)
    out["t_max"] = int(out["end"].max())
    return out


def status_of(records):
    return np.array([decode(r)["status"] for r in np.asarray(records, np.uint8).reshape(-1, RECORD_BYTES)], np.uint8)


# ---- the draw: the oracle's fast_prng (cpp/include/util/random.h:67-133) seeded with seed + i ---------------------------------------------
def draws(file_records, n, seed):
    """The picks (global record indices) of draws 0 .. n-1 over files of file_records[f] records each."""
    import oracle_lib as O
    first = np.concatenate([[0], np.cumsum(file_records)])
    out, state = np.zeros(n, np.uint32), np.zeros(8, np.uint8)
    for i in range(n):
        O.LIB.oracle_fast_prng_seed(O.ptr(state), (seed + i) & (2 ** 64 - 1))
        f = int(O.LIB.oracle_fast_prng_uniform_64(O.ptr(state))) % len(file_records)
        out[i] = first[f] + int(O.LIB.oracle_fast_prng_uniform_64(O.ptr(state))) % int(file_records[f])
    return out


# ---- the targets ------------------------------------------------------------------------------------------------------------------------
def get_state(action):
    """build.py's get_state on action int64[b, T]: float32 [b, T, N_DIM]; the state of step t holds the actions of the steps in front of it."""
    b, T = action.shape
    state = np.zeros((b, T, N_DIM + 1), F)
    np.put_along_axis(state, (action + 1)[:, :, None], 1.0, axis=2)
    state = np.minimum(np.cumsum(state, axis=1), 1.0)[:, :-1, 1:]
    return np.concatenate([np.zeros((b, 1, N_DIM), F), state], axis=1)


def targets(traj, value_weight):
    """valid, rows, state_cells / state_n, old_logp (float64: the exact side of the bound) and rewards from decoded arrays."""
    action, policy = traj["action"], traj["policy"]
    n = action.shape[0]
    valid = (action != -1) & (policy > 0)
    rows = np.argwhere(valid).astype(np.uint32)
    cells, counts = np.full((len(rows), STEPS), 0xFFFF, np.uint16), np.zeros(len(rows), np.uint8)
    for v, (b, t) in enumerate(rows):
        held = [int(a) for a in action[b, :t] if a != -1]
        cells[v, :len(held)], counts[v] = held, len(held)
    old_logp = np.log(policy[valid].astype(np.float64))
    rewards = np.zeros((n, STEPS), F)
    vw, sw = F(value_weight), F(1.0 - value_weight)
    r = (vw * traj["value"].astype(F)).astype(F) + (sw * traj["score"].astype(F)).astype(F)
    for b in range(n):
        if traj["end"][b] > 0:
            rewards[b, traj["end"][b] - 1] = r[b]
    return {"valid": valid, "rows": rows, "state_cells": cells, "state_n": counts, "old_logp": old_logp, "rewards": rewards}


# ---- inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------------------------
def rollout_record(team, size, rng, value=None, score=None, zero_prob=0.0):
    """One record of a build_ref.Rollout with seeded random picks and probabilities.  The first and the last probability are never 0 (a
    rollout's are not: compress_probability lifts them to 1); the ones between are 0 with probability zero_prob."""
    r, cells, probs = B.Rollout(team, size), [], []
    while r.legal() is not None:
        cells.append(r.advance(int(rng.integers(len(r.legal())))))
        probs.append(float(rng.choice([1.0, 1.0 / 65535, rng.random()])))
    if not cells:
        return None
    for k in range(1, len(cells) - 1):
        if rng.random() < zero_prob:
            probs[k] = 0.0
    return B.encode_record(team, size, cells, probs, rng.random() if value is None else value, score)


def rollout_records(count, seed, zero_prob=0.02):
    """About `count` records over the planted and sample teams at max_pokemon 1 .. 6, with deletions."""
    rng = np.random.default_rng(seed)
    pool = [t for _, t, _ in B.planted_teams()] + list(B.sample_teams())
    out = []
    while len(out) < count:
        team = np.array(pool[int(rng.integers(len(pool)))], np.uint8).reshape(6, 5).copy()
        present = [i for i in range(6) if team[i, 0]]
        size = int(rng.integers(1, 7))
        packed = np.zeros((6, 5), np.uint8)
        packed[:len(present)] = team[present]       # (the provider's pool teams are packed in the leading slots)
        packed[size:] = 0
        for i in range(size):
            if rng.random() < 0.35:
                packed[i] = 0
            else:
                packed[i, 1:][rng.random(4) < 0.4] = 0
        score = None if rng.random() < 0.2 else float(rng.integers(0, 3)) / 2
        rec = rollout_record(packed.reshape(30), size, rng, score=score, zero_prob=zero_prob)
        if rec is not None:
            out.append(np.frombuffer(rec, np.uint8))
    return np.stack(out)


def malformed_records():
    """[(name, expected status, record)]: one planted record per status that is not OK, each made from a sound one."""
    rng = np.random.default_rng(7)
    teams = {name: (team, size) for name, team, size in B.planted_teams()}
    base = np.frombuffer(rollout_record(*teams["one_missing_pokemon"], rng, score=1.0), np.uint8).copy()
    ups = lambda r: r[4:].view("<u2").reshape(STEPS, 2)
    out = []
    r = base.copy(); ups(r)[2, 0] = N_DIM
    out.append(("action_past_the_table", BAD_ACTION, r))
    r = base.copy(); ups(r)[30] = (0xFFFF, 1)
    out.append(("last_action_past_the_table", BAD_ACTION, r))
    # a move of a species that no set holds, before the start
    r = base.copy()
    other = next(s for s in B.LEGAL if int(B.TABLE[s, 0]) not in set(int(a) for a in ups(base)[:, 0]))
    ups(r)[1, 0] = int(B.TABLE[other, B.POOLS[other][0]])
    out.append(("move_without_its_species", NO_SPECIES, r))
    # seven species picks before the start
    r = np.zeros(RECORD_BYTES, np.uint8)
    for i, s in enumerate(B.LEGAL[:7]):
        ups(r)[i] = (int(B.TABLE[s, 0]), 0)
    ups(r)[7] = (int(B.TABLE[B.LEGAL[0], B.POOLS[B.LEGAL[0]][0]]), 9)
    out.append(("seven_sets", TEAM_FULL, r))
    # the taken action is a move the set already counted
    r = base.copy()
    start = int(np.flatnonzero(ups(base)[:, 1])[0])
    held = next(int(a) for a in ups(base)[:start, 0] if B.LIST[int(a)][1] != 0)
    ups(r)[start, 0] = held
    out.append(("taken_action_not_in_its_list", NOT_LEGAL, r))
    # the last species pick of a rollout from nothing with probability 0: `full` falls in front of it and its list holds no species
    r = np.frombuffer(rollout_record(*teams["empty"], rng, score=0.5), np.uint8).copy()
    picks = [i for i in range(STEPS) if ups(r)[i, 1] and B.LIST[int(ups(r)[i, 0])][1] == 0]
    ups(r)[picks[-2], 1] = 0          # (picks[-1] is the lead swap)
    out.append(("species_pick_past_full", NOT_LEGAL, r))
    # five sets of the species with the largest pool before the start, then a species pick: 148 + 5 x 42 entries
    big = max(B.LEGAL, key=lambda s: len(B.POOLS[s]))
    r = np.zeros(RECORD_BYTES, np.uint8)
    for i in range(5):
        ups(r)[i] = (int(B.TABLE[big, 0]), 0)
    ups(r)[5] = (int(B.TABLE[other, 0]), 5)
    ups(r)[6] = (int(B.TABLE[other, B.POOLS[other][0]]), 5)
    out.append(("duplicate_species_overflow_the_row", LIST_OVERFLOW, r))
    return out
