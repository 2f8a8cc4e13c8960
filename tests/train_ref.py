"""Test helper for the training-frame kernels (tests/test_train_ref.py on the CPU, tests/test_gpu_train_frames.py on the GPU): a numpy
restatement of a training row as include/oakgpu.h defines it -- the DENSE encoders of encode/battle/battle.h on states the CPU oracle
replays, Policy::get_index of the oracle's legal choices, the targets decoded from the frame bytes -- and of the sampling rule.
TEST INFRASTRUCTURE ONLY.

The dense rows are embed_ref's (which restates the sparse encoders, where a move held in two slots counts twice) with the move cells
recomputed by the dense rule: assigned slot by slot, so the last slot's bool(pp) stands."""
import struct

import numpy as np

import embed_ref as E
import oracle_lib as O
import policy_ref as P
import replay_oracle as R

F = np.float32
OK, COUNT, ILLEGAL, EARLY_END, RESULT, MALFORMED, RANGE = range(7)
POKEMON_IN, ACTIVE_IN, POLICY_DIM = 198, 229, 315
FIELDS = {
    "pokemon": ((2, 6, POKEMON_IN), np.float32), "active": ((2, 1, ACTIVE_IN), np.float32), "hp": ((2, 6, 1), np.float32),
    "choice_indices": ((2, 9), np.int64), "k": ((2, 1), np.uint8), "choice": ((2, 1), np.uint8), "iterations": ((1,), np.uint32),
    "empirical_policies": ((2, 9), np.float32), "nash_policies": ((2, 9), np.float32), "empirical_value": ((1,), np.float32),
    "nash_value": ((1,), np.float32), "score": ((1,), np.float32), "status": ((), np.uint8), "where": ((), np.uint32),
}
POSITION_FIELDS = ("pokemon", "active", "hp", "choice_indices", "k")


def empty(n):
    return {name: np.zeros((n,) + tail, dtype=dt) for name, (tail, dt) in FIELDS.items()}


# ---- the dense encoders -----------------------------------------------------------------------------------------------------------
def move_cells(slots, rule="last"):
    """The 164 move cells of MoveSlots::write from slots uint8[..., 8] ({id, pp} x 4).  rule: "last" = the dense overload (assigned
    slot by slot), "sum" = the sparse overload as a dense row (one per slot with PP), "or" = any slot with PP."""
    slots = np.asarray(slots)
    X = np.zeros(slots.shape[:-1] + (164,), dtype=F)
    for m in range(4):
        mid, pp = slots[..., 2 * m].astype(np.int64), slots[..., 2 * m + 1]
        it = np.nonzero((mid != 0) & (mid != 165))
        col = mid[it] - 1
        if rule == "last":
            X[it + (col,)] = (pp[it] != 0).astype(F)
        elif rule == "sum":
            np.add.at(X, it + (col,), (pp[it] != 0).astype(F))
        else:
            X[it + (col,)] = np.maximum(X[it + (col,)], (pp[it] != 0).astype(F))
    return X


def positions(battles, durations, rule="last"):
    """pokemon [n, 2, 6, 198], active [n, 2, 1, 229], hp [n, 2, 6, 1] of EncodedFrames::write for a batch of states."""
    battles, durations = np.ascontiguousarray(battles, np.uint8), np.ascontiguousarray(durations, np.uint8)
    n = battles.shape[0]
    party, act, order, _ = E._split(battles, durations)
    Xp, lp = E.encode_party(battles, durations)
    Xa, la = E.encode_actives(battles, durations)
    Xp, Xa = Xp.reshape(n, 2, 5, POKEMON_IN).copy(), Xa.copy()
    bench = E._stored(party, order[:, :, 1:])                                          # [n, 2, 5, 24]
    stored = E._stored(party, order[:, :, :1])[:, :, 0]                               # [n, 2, 24]
    Xp[..., 5:169] = move_cells(bench[..., 10:18], rule)
    Xa[..., 45:209] = move_cells(act[..., 24:32], rule)
    Xa[..., ACTIVE_IN + 5:ACTIVE_IN + 169] = move_cells(stored[..., 10:18], rule)
    Xp[~lp.reshape(n, 2, 5)] = 0
    Xa[~la] = 0
    hp_p, hp_a = E.hp_ratios(battles)
    pokemon = np.concatenate([Xa[:, :, None, ACTIVE_IN:], Xp], axis=2)
    hp = np.concatenate([hp_a.reshape(n, 2, 1), hp_p.reshape(n, 2, 5)], axis=2)[..., None]
    return np.ascontiguousarray(pokemon), np.ascontiguousarray(Xa[:, :, None, :ACTIVE_IN]), np.ascontiguousarray(hp.astype(F))


def choice_indices(battles, ch1, n1, ch2, n2, k1=None, k2=None):
    """[n, 2, 9] int64: Policy::get_index of the first k choices of each side (k: the engine's counts unless given), 315 behind them."""
    out = np.zeros((np.asarray(battles).shape[0], 2, 9), dtype=np.int64)
    for s, (ch, cnt, k) in enumerate(((ch1, n1, k1), (ch2, n2, k2))):
        rows = P.policy_rows(battles, ch, cnt if k is None else k, head=s)
        out[:, s] = np.where(rows >= 0, rows, POLICY_DIM)
    return out


def encode_states(battles, durations, results):
    """What oakgpu_encode_battles_dev writes: the position fields of a batch of states with the oracle's legal choices."""
    battles = np.ascontiguousarray(battles, np.uint8)
    n = battles.shape[0]
    live = (np.asarray(results) & 15) == 0
    ch, cnt = [np.zeros((n, 9), np.uint8) for _ in range(2)], [np.zeros(n, np.uint8) for _ in range(2)]
    for s in range(2):
        c, k = P.oracle_choices(battles[live], np.asarray(results)[live], s)
        ch[s][live], cnt[s][live] = c, k
    pokemon, active, hp = positions(battles, durations)
    return {"pokemon": pokemon, "active": active, "hp": hp, "choice_indices": choice_indices(battles, ch[0], cnt[0], ch[1], cnt[1]),
            "k": np.stack(cnt, axis=1)[:, :, None]}


# ---- records ----------------------------------------------------------------------------------------------------------------------
def uncompress(u16):
    return np.asarray(u16).astype(F) / F(65535.0)


def walk(rec):
    """One record replayed on the oracle: (frames, verdict).  frames[k] = the state in front of frame k -- (battle, durations, request
    byte, P1's choices, P2's choices, byte offset of the frame) -- for every frame that passes the per-frame checks; verdict = None, or
    (status, frame) of the first frame that fails one (replay_oracle's rules; MALFORMED and a non-terminal result byte come first)."""
    if R.check_record(rec) != "ok":
        return [], (MALFORMED, 0)
    total, nf = struct.unpack_from("<IH", rec, 0)
    if not 1 <= (rec[390] & 15) <= 3:
        return [], (RESULT, nf)
    battle = np.frombuffer(rec, np.uint8, 384, 6).copy()
    opt = O.Options()
    r = int(O.LIB.oracle_result_from_state(O.ptr(battle)))
    out, p = [], 391
    for k in range(nf):
        m, n, c1, c2 = (rec[p] & 15) + 1, (rec[p] >> 4) + 1, rec[p + 1], rec[p + 2]
        if r & 15:
            return out, (EARLY_END, k)
        l1, l2 = O.choices(battle, 0, (r >> 4) & 3), O.choices(battle, 1, (r >> 6) & 3)
        if len(l1) != m or len(l2) != n:
            return out, (COUNT, k)
        if c1 not in l1 or c2 not in l2:
            return out, (ILLEGAL, k)
        out.append((battle.copy(), opt.durations.copy(), r, l1, l2, p))
        opt.set()
        r = int(O.update(battle, c1, c2, opt))
        p += R.update_bytes(m, n)
    return out, None


def split_records(data):
    """The records of a buffer as oakgpu_replay_index cuts them: list of bytes."""
    out, pos = [], 0
    while pos < len(data):
        if R.check_record(data[pos:]) == "stop":
            break
        total = struct.unpack_from("<I", data, pos)[0]
        out.append(bytes(data[pos:pos + total]))
        pos += total
    return out


class Corpus:
    """Records walked once on the oracle (lazily, per record), shared by the tests."""

    def __init__(self, records):
        self.records = list(records)
        self._walks = {}

    def walked(self, r):
        if r not in self._walks:
            self._walks[r] = walk(self.records[r])
        return self._walks[r]

    def frames(self, r):
        return struct.unpack_from("<H", self.records[r], 4)[0]

    def expected(self, picks):
        """Every tensor of the rows of picks (n x 2), as a dict of arrays."""
        picks = np.asarray(picks, dtype=np.int64).reshape(-1, 2)
        n = picks.shape[0]
        out = empty(n)
        rows, states = [], []
        for i, (r, f) in enumerate(picks):
            if r >= len(self.records):
                out["status"][i], out["where"][i] = RANGE, f
                continue
            frames, verdict = self.walked(int(r))
            if verdict is not None and verdict[0] == MALFORMED:
                out["status"][i], out["where"][i] = verdict
            elif f >= self.frames(int(r)):
                out["status"][i], out["where"][i] = RANGE, f
            elif f >= len(frames):
                out["status"][i], out["where"][i] = verdict
            else:
                rows.append(i)
                out["where"][i] = f                                    # (the frame of the verdict, OK included)
                states.append((int(r),) + frames[int(f)])
        if rows:
            rows = np.array(rows)
            b = np.stack([s[1] for s in states])
            d = np.stack([s[2] for s in states])
            ch = [np.zeros((len(rows), 9), np.uint8) for _ in range(2)]
            cnt = [np.zeros(len(rows), np.uint8) for _ in range(2)]
            for j, s in enumerate(states):
                for side in range(2):
                    l = s[4 + side]
                    ch[side][j, :len(l)], cnt[side][j] = l, len(l)
            out["pokemon"][rows], out["active"][rows], out["hp"][rows] = positions(b, d)
            out["choice_indices"][rows] = choice_indices(b, ch[0], cnt[0], ch[1], cnt[1])
            for j, s in enumerate(states):
                i, rec, p = rows[j], self.records[s[0]], s[6]
                m, k = (rec[p] & 15) + 1, (rec[p] >> 4) + 1
                out["k"][i, :, 0] = (m, k)
                out["choice"][i, :, 0] = (rec[p + 1], rec[p + 2])
                out["iterations"][i, 0], ev, nv = struct.unpack_from("<IHH", rec, p + 3)
                out["empirical_value"][i, 0], out["nash_value"][i, 0] = uncompress(ev), uncompress(nv)
                probs = np.frombuffer(rec, "<u2", 2 * (m + k), p + 11)
                out["empirical_policies"][i, 0, :m], out["nash_policies"][i, 0, :m] = uncompress(probs[:m]), uncompress(probs[m:2 * m])
                out["empirical_policies"][i, 1, :k], out["nash_policies"][i, 1, :k] = uncompress(probs[2 * m:2 * m + k]), uncompress(probs[2 * m + k:])
                out["score"][i, 0] = {1: 1.0, 2: 0.0, 3: 0.5}[rec[390] & 15]
        return out

    # -- sampling --
    def valid_frames(self, r, min_iterations):
        """Frame indices of record r with iterations >= min_iterations ([] for a malformed record)."""
        rec = self.records[r]
        if R.check_record(rec) != "ok":
            return []
        out, p = [], 391
        for k in range(self.frames(r)):
            if struct.unpack_from("<I", rec, p + 3)[0] >= min_iterations:
                out.append(k)
            p += R.update_bytes((rec[p] & 15) + 1, (rec[p] >> 4) + 1)
        return out

    def draws(self, n, seed, max_battle_length=0, min_iterations=1, first=0):
        """Draws first .. first + n - 1 of the sampling rule: picks int64[n, 2]."""
        valid = [self.valid_frames(r, min_iterations) for r in range(len(self.records))]
        eligible = [r for r in range(len(self.records)) if valid[r] and (max_battle_length == 0 or self.frames(r) <= max_battle_length)]
        assert eligible
        out, state = np.zeros((n, 2), np.int64), np.zeros(8, np.uint8)
        for j in range(n):
            O.LIB.oracle_fast_prng_seed(O.ptr(state), (seed + first + j) & (2 ** 64 - 1))
            r = eligible[int(O.LIB.oracle_fast_prng_uniform_64(O.ptr(state))) % len(eligible)]
            out[j] = (r, valid[r][int(O.LIB.oracle_fast_prng_uniform_64(O.ptr(state))) % len(valid[r])])
        return out


def duplicated_move_sides(battles):
    """bool[n, 2, 7]: per side, whether the active's own slots (index 0) or the stored Pokemon at order position p (index 1 + p) hold
    one move id (not None, not Struggle) in two slots."""
    battles = np.ascontiguousarray(battles, np.uint8)
    party, act, order, _ = E._split(battles, np.zeros((battles.shape[0], 8), np.uint8))

    def dup(slots):
        ids = slots[..., 0::2].astype(np.int64)
        d = np.zeros(ids.shape[:-1], dtype=bool)
        for a in range(4):
            for b in range(a + 1, 4):
                d |= (ids[..., a] == ids[..., b]) & (ids[..., a] != 0) & (ids[..., a] != 165)
        return d
    pk = E._stored(party, order)                                                       # [n, 2, 6, 24]
    return np.concatenate([dup(act[..., 24:32])[..., None], dup(pk[..., 10:18]) & (order != 0)], axis=2)
