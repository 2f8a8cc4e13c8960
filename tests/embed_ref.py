"""Test helper for the embedding passes (tests/test_embed_ref.py on the CPU, tests/test_gpu_embedding.py on the GPU): the batched
dense form of nn_oracle's two encoders, a float64 evaluation of both embedding nets in the layout of write_battle_embedding, the
yardstick the kernels are held to (policy_ref.bound over E_ref and S), states that set every input the encoders have
(planted_states) and the census that proves it.  numpy only.

Byte layout (as oracle/nn_oracle.py): a side is 184 bytes -- six stored Pokemon of 24 (stats 0-9, four {move id, pp} 10-17, hp 18-19,
status 20, species 21, types 22, level 23), the active block of 32 at 144 (stats 0-9, species 10, types 11, six boost nibbles 12-14,
volatiles u64 16-23, four {move id, pp} 24-31), the order at 176.  A side's durations word: sleep turns of order position p in bits
3p .. 3p + 2, then four fields at bits 18 (3 bits, 5 inputs), 21 (4 bits, 8), 25 (3 bits, 3) and 28 (3 bits, 4)."""
import copy

import numpy as np

import policy_ref as P
from policy_ref import NN

F = np.float32
PARTY_IN, ACTIVE_IN = NN.POKEMON_IN, NN.ACTIVE_POKEMON_IN          # 198, 427
VOL_BITS = (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)     # the volatile bits the encoder reads, in input order
DURATION_FIELDS = ((18, 3, 5), (21, 4, 8), (25, 3, 3), (28, 3, 4))      # (shift, bits, inputs) of the four one-hot duration fields
DURATION_AT = (209, 214, 222, 225)                                       # their first active input
# F(num) / F(den) x F(1/4) (atk def spe spc) or x F(1/3) (acc eva), in fp32 as the reference computes them: [stat 0..5, stage + 6]
_MULT = np.array([F(n) / F(d) for n, d in NN.BOOSTS], dtype=F)
BOOST_VALUES = np.stack([_MULT * (F(1 / 4.0) if i < 4 else F(1 / 3.0)) for i in range(6)]).astype(F)
_STATUS_INDEX = np.full((256, 8), -1, dtype=np.int64)
for _st in range(1, 256):
    for _sl in range(8):
        _STATUS_INDEX[_st, _sl] = NN.status_index(_st, _sl)


# ---- fields ---------------------------------------------------------------------------------------------------------------------
def _split(battles, durations):
    """(party uint8[n, 2, 6, 24], active uint8[n, 2, 32], order int64[n, 2, 6], durations word int64[n, 2])."""
    b = np.ascontiguousarray(battles, dtype=np.uint8)
    n = b.shape[0]
    sides = b[:, :368].reshape(n, 2, 184)
    dur = np.ascontiguousarray(durations, dtype=np.uint8).reshape(n, 8).view("<u4").reshape(n, 2).astype(np.int64)
    return sides[:, :, :144].reshape(n, 2, 6, 24), sides[:, :, 144:176], sides[:, :, 176:182].astype(np.int64), dur


def _u16(x, off):
    return x[..., off].astype(np.int64) | (x[..., off + 1].astype(np.int64) << 8)


def _stored(party, ids):
    """The stored Pokemon named by 1-based ids (id 0: slot 1's bytes, to be masked by the caller): uint8[..., 24]."""
    return np.take_along_axis(party, np.maximum(ids - 1, 0)[..., None], axis=2)


def _put(X, where, col, val=F(1)):
    """X[item, col[item]] += val over the items of `where` (+=: the reference's sparse first layer adds a column once per entry, so a
    move held in two slots counts twice)."""
    it = np.nonzero(where)
    np.add.at(X, it + (col[it],), val)


def _encode_pokemon(pk, sleep, X, offset):
    """Encode::Battle::Pokemon::write of pk uint8[..., 24] with sleep turns int[...] into X[..., offset : offset + 198]."""
    every = np.ones(pk.shape[:-1], dtype=bool)
    X[..., offset] = _u16(pk, 0).astype(F) / F(703.0)
    for i in range(1, 5):
        X[..., offset + i] = _u16(pk, 2 * i).astype(F) / F(999.0)
    for m in range(4):
        mid, pp = pk[..., 10 + 2 * m].astype(np.int64), pk[..., 11 + 2 * m]
        _put(X, (mid != 165) & (mid != 0) & (pp != 0), offset + 5 + mid - 1)
    status = pk[..., 20].astype(np.int64)
    _put(X, status != 0, offset + 169 + _STATUS_INDEX[status, sleep])
    t1, t2 = pk[..., 22].astype(np.int64) % 16, pk[..., 22].astype(np.int64) // 16
    _put(X, every, offset + 183 + t1)
    _put(X, t2 != t1, offset + 183 + t2)


def encode_party(battles, durations):
    """The bench slots of a batch as dense encoder inputs: (X float32[n, 10, 198], live bool[n, 10]); item = side * 5 + order position
    - 1.  A slot is dead (row of zeros) when its order entry is 0 or its stored hp is 0, as write_battle_embedding skips it."""
    party, _, order, dur = _split(battles, durations)
    ids = order[:, :, 1:]
    pk = _stored(party, ids)                                                          # [n, 2, 5, 24]
    live = (ids != 0) & (_u16(pk, 18) != 0)
    sleep = (dur[:, :, None] >> (3 * np.arange(1, 6))[None, None, :]) & 7
    X = np.zeros(pk.shape[:-1] + (PARTY_IN,), dtype=F)
    _encode_pokemon(pk, sleep, X, 0)
    X[~live] = 0
    n = X.shape[0]
    return X.reshape(n, 10, PARTY_IN), live.reshape(n, 10)


def encode_actives(battles, durations):
    """The two actives of a batch as dense Encode::Battle::ActivePokemon inputs: (X float32[n, 2, 427], live bool[n, 2]); dead (zeros)
    when the stored Pokemon of order position 0 has hp 0."""
    party, act, order, dur = _split(battles, durations)
    pk = _stored(party, order[:, :, :1])[:, :, 0]                                     # [n, 2, 24]
    live = _u16(pk, 18) != 0
    every = np.ones(live.shape, dtype=bool)
    X = np.zeros(live.shape + (ACTIVE_IN,), dtype=F)
    X[..., 0] = _u16(act, 0).astype(F) / F(703.0)
    for i in range(1, 5):
        X[..., i] = _u16(act, 2 * i).astype(F) / F(999.0)
    t1, t2 = act[..., 11].astype(np.int64) % 16, act[..., 11].astype(np.int64) // 16
    _put(X, every, 5 + t1)
    _put(X, t2 != t1, 5 + t2)
    for i in range(6):
        nib = (act[..., 12 + (i >> 1)].astype(np.int64) >> (4 * (i & 1))) & 15
        X[..., 20 + i] = BOOST_VALUES[i][((nib ^ 8) - 8) + 6]
    vol = np.zeros(live.shape, dtype=np.uint64)
    for k in range(8):
        vol |= act[..., 16 + k].astype(np.uint64) << np.uint64(8 * k)
    for j, k in enumerate(VOL_BITS):
        X[..., 26 + j] = ((vol >> np.uint64(k)) & np.uint64(1)).astype(F)
    X[..., 42] = ((vol >> np.uint64(24)) & np.uint64(0xFFFF)).astype(F) / F(65535.0)
    X[..., 43] = ((vol >> np.uint64(40)) & np.uint64(0xFF)).astype(F) / F(706 // 4 + 1)
    X[..., 44] = ((vol >> np.uint64(59)) & np.uint64(31)).astype(F) / F(16.0)
    for m in range(4):
        mid, pp = act[..., 24 + 2 * m].astype(np.int64), act[..., 25 + 2 * m]
        _put(X, (mid != 165) & (mid != 0) & (pp != 0), 45 + mid - 1)
    for (sh, bits, _), at in zip(DURATION_FIELDS, DURATION_AT):
        v = (dur >> sh) & ((1 << bits) - 1)
        _put(X, v != 0, at + v - 1)
    _encode_pokemon(pk, dur & 7, X, NN.ACTIVE_IN)
    X[~live] = 0
    return X, live


def hp_ratios(battles):
    """F(hp) / F(max hp) of the twelve items of every leaf, 0 for a dead one: (party float32[n, 10], actives float32[n, 2])."""
    party, _, order, _ = _split(battles, np.zeros((np.asarray(battles).shape[0], 8), np.uint8))
    out = []
    for ids, bench in ((order[:, :, 1:], True), (order[:, :, :1], False)):
        pk = _stored(party, ids)
        hp, mx = _u16(pk, 18), _u16(pk, 0)
        live = (hp != 0) & ((ids != 0) | (not bench))
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(live, hp.astype(F) / mx.astype(F), F(0)).astype(F).reshape(hp.shape[0], -1))
    return out[0], out[1]


def sparse_to_dense(idx, val, dim):
    """nn_oracle's (indices, values) as the dense input they stand for."""
    x = np.zeros(dim, dtype=F)
    np.add.at(x, np.asarray(idx, dtype=np.int64), np.asarray(val, dtype=F))
    return x


def oracle_inputs(battle, durations):
    """nn_oracle's sparse encoders on one leaf, item by item as battle_embedding calls them: (party float32[10, 198], live[10],
    actives float32[2, 427], live[2])."""
    Xp, lp, Xa, la = np.zeros((10, PARTY_IN), F), np.zeros(10, bool), np.zeros((2, ACTIVE_IN), F), np.zeros(2, bool)
    for s in range(2):
        side = battle[184 * s:184 * (s + 1)]
        dur = int.from_bytes(bytes(durations[4 * s:4 * s + 4]), "little")
        sid = int(side[176]) - 1
        stored = side[24 * sid:24 * sid + 24]
        if NN._u16(stored, 18) != 0:
            Xa[s], la[s] = sparse_to_dense(*NN.encode_active_pokemon(stored, side[144:176], dur), ACTIVE_IN), True
        for slot in range(2, 7):
            pid = int(side[176 + slot - 1])
            if pid == 0 or NN._u16(side[24 * (pid - 1):24 * pid], 18) == 0:
                continue
            k = 5 * s + slot - 2
            Xp[k], lp[k] = sparse_to_dense(*NN.encode_pokemon(side[24 * (pid - 1):24 * pid], (dur >> (3 * (slot - 1))) & 7), PARTY_IN), True
    return Xp, lp, Xa, la


# ---- the float64 embedding ------------------------------------------------------------------------------------------------------
def _act64(kind):
    return (lambda x: np.maximum(x, 0.0)) if kind == 1 else (lambda x: np.clip(x, 0.0, 1.0))


def _net64(l0, l1, X, act, l1_operand=None, drop_column=None):
    W0 = l0.W.astype(np.float64)
    if drop_column is not None:
        W0 = W0.copy()
        W0[:, drop_column] = 0.0
    h = act(X.astype(np.float64) @ W0.T + l0.b.astype(np.float64))
    W1 = l1.W
    if l1_operand is not None:
        W1, h = l1_operand(W1), l1_operand(h.astype(F)).astype(np.float64)
    return act(h @ W1.astype(np.float64).T + l1.b.astype(np.float64))


def embedding_f64(onet, battles, durations, act_party=None, act_actives=None, l1_operand=None, drop_party=None, drop_active=None,
                  chunk=4096):
    """write_battle_embedding for a batch with both layers of both embedding nets in float64 from the fp32 weights as stored:
    float64[n, 2 * side_dim].  Activation from the file header, or per pass (1 ReLU, 2 clamp: the discrete handle embeds party slots
    with ReLU and actives with clamp).  The hp-ratio entries are the fp32 quotients the reference stores; dead items are zeros.
    l1_operand / drop_party / drop_active (the discrimination checks): a function applied to both operands of the second layers; a
    first-layer column (input index) of the party / active net taken as zeros."""
    battles, durations = np.asarray(battles), np.asarray(durations)
    n, pod, aod = battles.shape[0], onet.pod, onet.aod
    ap, aa = _act64(act_party or onet.activation), _act64(act_actives or onet.activation)
    out = np.zeros((n, 2, onet.side_dim), dtype=np.float64)
    for lo in range(0, n, chunk):
        b, d = battles[lo:lo + chunk], durations[lo:lo + chunk]
        m = b.shape[0]
        Xp, lp = encode_party(b, d)
        Xa, la = encode_actives(b, d)
        hp_p, hp_a = hp_ratios(b)
        ep = _net64(onet.p0, onet.p1, Xp.reshape(m * 10, PARTY_IN), ap, l1_operand, drop_party).reshape(m, 2, 5, pod)
        ea = _net64(onet.a0, onet.a1, Xa.reshape(m * 2, ACTIVE_IN), aa, l1_operand, drop_active).reshape(m, 2, aod)
        o = out[lo:lo + m]
        o[:, :, 0] = hp_a
        o[:, :, 1:1 + aod] = np.where(la[:, :, None], ea, 0.0)
        bench = np.zeros((m, 2, 5, 1 + pod))
        bench[..., 0] = hp_p.reshape(m, 2, 5)
        bench[..., 1:] = np.where(lp.reshape(m, 2, 5)[..., None], ep, 0.0)
        o[:, :, 1 + aod:] = bench.reshape(m, 2, 5 * (1 + pod))
    return out.reshape(n, 2 * onet.side_dim)


def dead_mask(onet, battles, durations):
    """bool[n, 2 * side_dim]: the entries of dead items (hp entry and block), which every form must write as exactly 0.0."""
    n = np.asarray(battles).shape[0]
    _, lp = encode_party(battles, durations)
    _, la = encode_actives(battles, durations)
    m = np.zeros((n, 2, onet.side_dim), dtype=bool)
    m[:, :, :1 + onet.aod] = ~la[:, :, None]
    m[:, :, 1 + onet.aod:] = np.repeat(~lp.reshape(n, 2, 5), 1 + onet.pod, axis=2)
    return m.reshape(n, 2 * onet.side_dim)


def oracle_embedding(onet, battles, durations, rows=None, act_party=None, act_actives=None):
    """nn_oracle.battle_embedding (fp32, leaf by leaf) on the given rows (all by default): float32[len(rows), dim].  With per-pass
    activations the blocks of each pass are taken from the oracle run under that activation."""
    rows = np.arange(np.asarray(battles).shape[0]) if rows is None else np.asarray(rows)
    keep, res = onet.activation, {}
    for kind in {act_party or keep, act_actives or keep}:
        net = copy.copy(onet)              # (a shallow copy: the layers are shared, the activation is this run's)
        net.activation = kind
        res[kind] = np.stack([NN.battle_embedding(net, battles[i], durations[i]) for i in rows]) if rows.size else np.zeros((0, 2 * onet.side_dim), F)
    out = res[act_party or keep].reshape(rows.size, 2, onet.side_dim).copy()
    out[:, :, :1 + onet.aod] = res[act_actives or keep].reshape(rows.size, 2, onet.side_dim)[:, :, :1 + onet.aod]
    return out.reshape(rows.size, 2 * onet.side_dim)


def yardstick(ref, oracle, rows=None):
    """(E_ref, S): the fp32 oracle's worst distance from the float64 embedding over the rows it was run on (a subset only makes E_ref
    smaller and the bound tighter), and S = max(1, max |f64 entry|) over every row."""
    r = ref if rows is None else ref[np.asarray(rows)]
    e_ref = float(np.abs(oracle.astype(np.float64) - r).max()) if r.size else 0.0
    return e_ref, max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)


def worst_error(got, ref):
    return float(np.abs(np.asarray(got).astype(np.float64) - ref).max()) if ref.size else 0.0


bound = P.bound


# ---- planted states -------------------------------------------------------------------------------------------------------------
def _pk(s, k):
    return 184 * s + 24 * k


def _act(s):
    return 184 * s + 144


def _stored_of(b, s, pos):
    """Byte offset of the stored Pokemon at order position pos of side s."""
    pid = int(b[184 * s + 176 + pos])
    assert pid != 0
    return _pk(s, pid - 1)


def _set_dur(d, s, shift, bits, v):
    w = int.from_bytes(bytes(d[4 * s:4 * s + 4]), "little")
    w = (w & ~(((1 << bits) - 1) << shift)) | (int(v) << shift)
    d[4 * s:4 * s + 4] = np.frombuffer(int(w).to_bytes(4, "little"), np.uint8)


def _set_vol(b, s, mask, value):
    o = _act(s) + 16
    v = int.from_bytes(bytes(b[o:o + 8]), "little")
    v = (v & ~mask) | value
    b[o:o + 8] = np.frombuffer(int(v).to_bytes(8, "little"), np.uint8)


def _put16(b, off, v):
    b[off], b[off + 1] = v & 255, v >> 8


# (status byte, sleep turns) for each of the 14 status indices -- psn, brn, frz, par, sleep with 1-7 public turns, self-inflicted sleep
# with counter 3, 2, 1 -- and toxic, which shares index 0 with psn
STATUS_PLANTS = [(0x08, 0), (0x10, 0), (0x20, 0), (0x40, 0)] + [(4, t) for t in range(1, 8)] + [(0x80 | c, 0) for c in (3, 2, 1)] + [(0x88, 0)]
ENCODED_VOL = sum(1 << k for k in VOL_BITS)
ALL_VOL = ENCODED_VOL | (0xFFFF << 24) | (0xFF << 40) | (31 << 59)


def _plants():
    """The list of (family, fn(b, d, s)): each fn overwrites one field of side s of one state (uint8[384], uint8[8]) in place."""
    out = []
    add = lambda family, fn, reps=1: out.extend([(family, fn)] * reps)

    def status(pos, st, turns):
        def fn(b, d, s):
            b[_stored_of(b, s, pos) + 20] = st
            _set_dur(d, s, 3 * pos, 3, turns)
        return fn
    for st, turns in STATUS_PLANTS:
        add("status", status(0, st, turns), 20)                      # the active: input 229 + 169 + index
        for pos in range(1, 6):
            add("status", status(pos, st, turns), 4)                 # each bench position: 5 x 4 items per party input
    for pos in range(6):                                               # every sleep-turn value at every order position, under a sleep status
        for turns in range(8):
            add("sleep_turns", status(pos, 4, turns), 2)

    def boost(i, stage):
        def fn(b, d, s):
            o = _act(s) + 12 + (i >> 1)
            b[o] = (int(b[o]) & (0x0F if i & 1 else 0xF0)) | ((stage & 15) << (4 * (i & 1)))
        return fn
    for i in range(6):
        for stage in range(-6, 7):
            add("boost", boost(i, stage), 3)

    for k in VOL_BITS:                                                 # each encoded bit alone
        add("volatile", lambda b, d, s, k=k: _set_vol(b, s, ENCODED_VOL, 1 << k), 20)
    add("volatile", lambda b, d, s: _set_vol(b, s, ALL_VOL, ALL_VOL), 20)
    for v in (0, 1, 65535):
        add("volatile", lambda b, d, s, v=v: _set_vol(b, s, 0xFFFF << 24, v << 24), 10)
    for v in (0, 1, 255):
        add("volatile", lambda b, d, s, v=v: _set_vol(b, s, 0xFF << 40, v << 40), 10)
    for v in range(32):
        add("volatile", lambda b, d, s, v=v: _set_vol(b, s, 31 << 59, v << 59), 2)

    for sh, bits, count in DURATION_FIELDS:                            # every value the field's one-hot has an input for, and 0
        for v in range(count + 1):
            add("duration", lambda b, d, s, sh=sh, bits=bits, v=v: _set_dur(d, s, sh, bits, v), 20 if v else 2)

    def move(where, slot, mid, pp=None):
        def fn(b, d, s):
            o = (_act(s) + 24 if where < 0 else _stored_of(b, s, where) + 10) + 2 * slot
            b[o] = mid
            b[o + 1] = max(int(b[o + 1]), 1) if pp is None else pp
        return fn
    for mid in range(1, 165):
        for slot in range(4):
            add("move", move(-1, slot, mid), 5)                        # the active's own slots: 4 x 5 items per active input
            add("move", move(0, slot, mid), 5)                         # the active's stored slots
            for pos in range(1, 6):
                add("move", move(pos, slot, mid))                      # each bench position: 4 x 5 items per party input
    for where in (-1, 0, 1, 2, 3, 4, 5):                               # id 0, Struggle's id and PP 0 contribute nothing
        for slot in range(4):
            add("move", move(where, slot, 0))
            add("move", move(where, slot, 165, 7))
            add("move", move(where, slot, 1 + 41 * slot, 0))

    def types(where, t1, t2):
        def fn(b, d, s):
            o = _act(s) + 11 if where < 0 else _stored_of(b, s, where) + 22
            cur = int(b[o])
            b[o] = (cur % 16 if t1 is None else t1) | ((cur // 16 if t2 is None else t2) << 4)
        return fn
    for where in (-1, 0, 1, 3, 5):
        for t in range(15):
            add("types", types(where, t, None))
            add("types", types(where, None, t))
            add("types", types(where, t, t))

    def stat(where, k, v, hp=None):
        def fn(b, d, s):
            o = _act(s) if where < 0 else _stored_of(b, s, where)
            _put16(b, o + 2 * k, v)
            if hp is not None:
                _put16(b, o + 18, hp)
        return fn
    for where in (-1, 0, 2, 4):
        for k in range(5):
            for v in (0, 1, 999):
                if k or where < 0:                                     # (a stored max hp of 0 would make the hp ratio a division by zero)
                    add("stats", stat(where, k, v))
        if where >= 0:                                                 # hp 1, hp full, and the largest max hp there is
            add("stats", stat(where, 0, 1, hp=1))
            add("stats", stat(where, 0, 999, hp=1))
            add("stats", stat(where, 0, 321, hp=321))
            add("stats", stat(where, 0, 703, hp=703))

    def hp_zero(pos):
        return lambda b, d, s: _put16(b, _stored_of(b, s, pos) + 18, 0)

    def team_of(size):
        def fn(b, d, s):
            b[184 * s + 176 + size:184 * s + 182] = 0
        return fn

    def active_in_slot(k):
        def fn(b, d, s):
            cur = int(b[184 * s + 176]) - 1
            if cur != k:
                a, c = b[_pk(s, cur):_pk(s, cur) + 24].copy(), b[_pk(s, k):_pk(s, k) + 24].copy()
                b[_pk(s, cur):_pk(s, cur) + 24], b[_pk(s, k):_pk(s, k) + 24] = c, a
                order = b[184 * s + 176:184 * s + 182]
                was_cur, was_k = order == cur + 1, order == k + 1
                order[was_cur], order[was_k] = k + 1, cur + 1
        return fn
    for pos in range(6):
        add("dead", hp_zero(pos), 4)
        add("dead", active_in_slot(pos), 4)
    for size in range(1, 6):
        add("dead", team_of(size), 4)
    return out


_PLANTED = {}


def planted_states(families=None):
    """(battles, durations, names): mid-game states of policy_ref.form_states() with all twelve Pokemon alive and some damage done,
    each with one encoder field overwritten on each side (side 0 takes plant 2j, side 1 plant 2j + 1 of _plants(); the rest is left as
    play made it).  No engine step is run on them: they are encodable, not reachable.  names[i] names the families of state i's two
    plants.  families: only the plants of these families (for the test that the census needs them).  Deterministic."""
    key = None if families is None else tuple(sorted(families))
    if key not in _PLANTED:
        b0, d0, _ = P.form_states()
        _, la = encode_actives(b0, d0)
        _, lp = encode_party(b0, d0)
        party, _, _, _ = _split(b0, d0)
        hurt = (_u16(party, 18) != _u16(party, 0)).any(axis=(1, 2))
        pool = np.nonzero(la.all(axis=1) & lp.all(axis=1) & hurt)[0]
        assert pool.size >= 256, pool.size
        pool = pool[np.random.default_rng(8).permutation(pool.size)]
        plants = [p for p in _plants() if families is None or p[0] in families]
        n = (len(plants) + 1) // 2
        src = pool[np.arange(n) % pool.size]
        b, d, names = b0[src].copy(), d0[src].copy(), []
        for j in range(n):
            mine = plants[2 * j:2 * j + 2]
            for s, (_, fn) in enumerate(mine):
                fn(b[j], d[j], s)
            names.append("+".join(f for f, _ in mine))
        _PLANTED[key] = (np.ascontiguousarray(b), np.ascontiguousarray(d), names)
    return _PLANTED[key]


def all_states():
    """form_states() followed by planted_states(): (battles, durations)."""
    b0, d0, _ = P.form_states()
    b1, d1, _ = planted_states()
    return np.concatenate([b0, b1]), np.concatenate([d0, d1])


# ---- census ---------------------------------------------------------------------------------------------------------------------
def feature_census(battles, durations):
    """What a set of states exercises: per encoder input the number of live items that set it (party[198], actives[427]); per (stat,
    boost stage) the live actives holding it (boosts[6, 13]); per duration field and value (durations: four arrays, index = value);
    the toxic counter's values (tox[32]); per order position the live Pokemon with non-zero sleep turns (sleep_turns[6]); the sides
    per team size (team_sizes[7]); bench items with an empty order entry (absent), with hp 0 (fainted), and dead actives."""
    Xp, lp = encode_party(battles, durations)
    Xa, la = encode_actives(battles, durations)
    _, act, order, dur = _split(battles, durations)
    boosts = np.zeros((6, 13), dtype=np.int64)
    for i in range(6):
        nib = (act[..., 12 + (i >> 1)].astype(np.int64) >> (4 * (i & 1))) & 15
        boosts[i] = np.bincount((((nib ^ 8) - 8) + 6)[la], minlength=13)[:13]
    durs = [np.bincount(((dur >> sh) & ((1 << bits) - 1))[la], minlength=1 << bits) for sh, bits, _ in DURATION_FIELDS]
    turns = (dur[:, :, None] >> (3 * np.arange(6))[None, None, :]) & 7
    live6 = np.concatenate([la[:, :, None], lp.reshape(-1, 2, 5)], axis=2)
    absent = (order[:, :, 1:] == 0).reshape(-1, 10)
    return dict(party=(Xp != 0)[lp].sum(axis=0), actives=(Xa != 0)[la].sum(axis=0), boosts=boosts, durations=durs,
                tox=np.bincount(((act[..., 23].astype(np.int64) >> 3) & 31)[la], minlength=32),
                sleep_turns=((turns != 0) & live6).sum(axis=(0, 1)), team_sizes=np.bincount((order != 0).sum(axis=2).ravel(), minlength=7),
                absent=int(absent.sum()), fainted=int((~lp & ~absent).sum()), dead_actives=int((~la).sum()))
