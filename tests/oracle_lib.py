"""ctypes binding of the CPU oracle (oracle/liboracle.so).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.environ.get("ORACLE_SO") or os.path.join(ROOT, "oracle", "liboracle.so")   # (ORACLE_SO: a variant build, tools/engine_variants.sh)


def build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "liboracle.so"])


def _load():
    if not os.path.exists(_SO):
        build()
    lib = C.CDLL(_SO)
    u8p = C.POINTER(C.c_uint8)
    lib.oracle_update.restype = C.c_uint8
    lib.oracle_update.argtypes = [C.c_void_p, C.c_uint8, C.c_uint8, C.c_void_p]
    lib.oracle_choices.restype = C.c_uint8
    lib.oracle_choices.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.oracle_options_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.oracle_init_battle.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.oracle_result_from_state.restype = C.c_uint8
    lib.oracle_result_from_state.argtypes = [C.c_void_p]
    lib.oracle_randomize_hidden_variables.argtypes = [C.c_void_p, C.c_void_p]
    lib.oracle_mt19937_seed.argtypes = [C.c_void_p, C.c_uint32]
    lib.oracle_mt19937_uniform_64.restype = C.c_uint64
    lib.oracle_mt19937_uniform_64.argtypes = [C.c_void_p]
    lib.oracle_fast_prng_seed.argtypes = [C.c_void_p, C.c_uint64]
    lib.oracle_fast_prng_next32.restype = C.c_uint32
    lib.oracle_fast_prng_next32.argtypes = [C.c_void_p]
    lib.oracle_fast_prng_uniform_64.restype = C.c_uint64
    lib.oracle_fast_prng_uniform_64.argtypes = [C.c_void_p]
    lib.oracle_fast_prng_seed_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    lib.oracle_fast_prng_spawn_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.oracle_rollout_fast.restype = C.c_uint8
    lib.oracle_rollout_fast.argtypes = [C.c_void_p, C.c_void_p, C.c_uint8, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.oracle_rollout_mt.restype = C.c_uint8
    lib.oracle_rollout_mt.argtypes = [C.c_void_p, C.c_void_p, C.c_uint8, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.oracle_rollout_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                         C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.oracle_set_ou_pools.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.oracle_make_random_ou_battle.restype = C.c_uint8
    lib.oracle_make_random_ou_battle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.oracle_nn_load.restype = C.c_void_p
    lib.oracle_nn_load.argtypes = [C.c_char_p]
    lib.oracle_nn_free.argtypes = [C.c_void_p]
    lib.oracle_nn_embedding.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.oracle_nn_value_inference.restype = C.c_float
    lib.oracle_nn_value_inference.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.oracle_nn_value_inference_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
    lib.oracle_hash64.restype = C.c_uint64
    lib.oracle_hash64.argtypes = [C.c_void_p, C.c_size_t]
    return lib


LIB = _load()
OPTIONS_SIZE = 40


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Options:
    def __init__(self, durations=None):
        self.buf = np.zeros(OPTIONS_SIZE, dtype=np.uint8)
        if durations is not None:
            self.buf[16:24] = durations

    @property
    def actions(self):
        return self.buf[0:16]

    @property
    def durations(self):
        return self.buf[16:24]

    def set(self, durations=None, overrides=None):
        d = None if durations is None else ptr(np.ascontiguousarray(durations, dtype=np.uint8))
        o = None if overrides is None else ptr(np.ascontiguousarray(overrides, dtype=np.uint8))
        LIB.oracle_options_set(ptr(self.buf), d, o)


def update(battle, c1, c2, options):
    return LIB.oracle_update(ptr(battle), c1, c2, ptr(options.buf))


def choices(battle, player, request):
    out = np.zeros(9, dtype=np.uint8)
    n = LIB.oracle_choices(ptr(battle), player, request, ptr(out), 9)
    return out[:n].copy()


def init_battle(teams, seed):
    """teams: array-like [2][6][5] (species, 4 moves)."""
    t = np.ascontiguousarray(np.array(teams, dtype=np.uint8).reshape(60))
    b = np.zeros(384, dtype=np.uint8)
    LIB.oracle_init_battle(ptr(b), ptr(t), C.c_uint64(seed))
    return b


_pools_set = False


def ensure_pools():
    global _pools_set
    if _pools_set:
        return
    import sys
    sys.path.insert(0, ROOT)
    from oak_amd import gamedata
    legal, pools, sizes = gamedata.ou_pools()
    LIB.oracle_set_ou_pools(ptr(legal), len(legal), ptr(np.ascontiguousarray(pools)), ptr(sizes))
    _pools_set = True


def make_random_ou_batch(n, seed0=0x0A4B00000000):
    """SURVEY 8(d) config 2 inputs: (battles[n,384], durations[n,8], prng[n,8], results[n])."""
    ensure_pools()
    battles = np.zeros((n, 384), dtype=np.uint8)
    durs = np.zeros((n, 8), dtype=np.uint8)
    prng = np.zeros((n, 8), dtype=np.uint8)
    res = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        res[i] = LIB.oracle_make_random_ou_battle(ptr(battles[i]), ptr(durs[i]), ptr(prng[i]), C.c_uint64(seed0 + i))
    return battles, durs, prng, res


def rollout_batch(battles, durs, results, prng, max_steps=1000, prep=False, threads=1):
    n = battles.shape[0]
    out = np.zeros(n, dtype=np.uint8)
    steps = np.zeros(n, dtype=np.uint32)
    LIB.oracle_rollout_batch(ptr(battles), ptr(durs), ptr(np.ascontiguousarray(results)), ptr(prng), n,
                             max_steps, 1 if prep else 0, ptr(out), ptr(steps), threads)
    return out, steps


class CNet:
    """oracle/nn_host.c: the plain-C fp32 leaf evaluator (second checker + bench.py's CPU baseline for leaf-evals/s)."""

    def __init__(self, path):
        self.h = LIB.oracle_nn_load(os.fsencode(path))
        if not self.h:
            raise RuntimeError("oracle_nn_load failed: %s" % path)

    def embedding(self, battle, durations, dim=768):
        out = np.zeros(dim, dtype=np.float32)
        LIB.oracle_nn_embedding(self.h, ptr(np.ascontiguousarray(battle)), ptr(np.ascontiguousarray(durations)), ptr(out))
        return out

    def value_inference_batch(self, battles, durations, threads=1):
        n = battles.shape[0]
        out = np.zeros(n, dtype=np.float32)
        LIB.oracle_nn_value_inference_batch(self.h, ptr(np.ascontiguousarray(battles)), ptr(np.ascontiguousarray(durations)), n, ptr(out), threads)
        return out

    def close(self):
        if self.h:
            LIB.oracle_nn_free(self.h)
            self.h = None


def root_steps_reference(root_b, root_d, root_r, lane_prng, reps, steps, slice, max_steps=1000, threads=4):
    """The oracle of oakgpu_root_steps (BASELINE configs[3] in slices): `steps` search steps over the given roots on the CPU, every
    playout run to terminal at once (mcts.h:250-263 prep + mcts.h:448-496 loop, oracle_rollout_batch) and credited by the rule the
    product documents -- a playout of len turn-steps started in step k belongs to step k + (len - 1) // slice (len = 0 or slice = 0:
    step k).  Lane (root, replica) owns a fast_prng stream that advances by ONE uniform_64 per step; that draw is the 8-byte state of
    the fresh playout's own stream (all-zero -> s1 = 1).  lane_prng [roots * reps, 8] is advanced in place.
    Returns (count, sum2, turn_steps): int64 [steps + tail, roots] each for the first two (tail = the drain steps the longest playout
    needs), and the list of turn-steps EXECUTED per step (what the launches of a sliced run execute, drain steps included)."""
    roots = root_b.shape[0]
    n = roots * reps
    lives = (max_steps + slice - 1) // slice if slice else 1
    total_steps = steps + lives
    count = np.zeros((total_steps, roots), dtype=np.int64)
    sum2 = np.zeros((total_steps, roots), dtype=np.int64)
    executed = np.zeros(total_steps, dtype=np.int64)
    rid = np.repeat(np.arange(roots), reps)
    for k in range(steps):
        pp = np.zeros((n, 8), dtype=np.uint8)
        assert lane_prng.flags["C_CONTIGUOUS"] and lane_prng.shape == (n, 8)
        LIB.oracle_fast_prng_spawn_batch(ptr(lane_prng), n, ptr(pp))
        b = np.ascontiguousarray(np.repeat(root_b, reps, axis=0))
        d = np.ascontiguousarray(np.repeat(root_d, reps, axis=0))
        r = np.ascontiguousarray(np.repeat(root_r, reps))
        out, ln = rollout_batch(b, d, r, pp, max_steps=max_steps, prep=True, threads=threads)
        t = out & 15
        v2 = np.where(t == 1, 2, np.where(t == 2, 0, 1)).astype(np.int64)
        ln = ln.astype(np.int64)
        when = k + (np.where(ln > 0, (ln - 1) // slice, 0) if slice else 0)
        np.add.at(count, (when, rid), 1)
        np.add.at(sum2, (when, rid), v2)
        if slice:
            for j in range(lives):      # slice j of a playout executes min(len - j * slice, slice) turn-steps in launch k + j
                executed[k + j] += int(np.clip(ln - j * slice, 0, slice).sum())
        else:
            executed[k] += int(ln.sum())
    return count, sum2, executed


# ---- the party-slot cache key (include/oakgpu.h, oakgpu_leaf_eval_cached_dev) ---------------------------------------------
_STATUS_KEY = None


def _status_key_table():
    """[status, sleep turns] -> the key's status byte: 0 for no status, else nn_oracle.status_index + 1."""
    global _STATUS_KEY
    if _STATUS_KEY is None:
        import sys
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import nn_oracle
        t = np.zeros((256, 8), dtype=np.uint8)
        for st in range(1, 256):
            for sl in range(8):
                t[st, sl] = nn_oracle.status_index(st, sl) + 1
        _STATUS_KEY = t
    return _STATUS_KEY


def party_slot_keys(battles, durations):
    """Host restatement of the cache's slot key, from the contract alone: bench slot q (0-4) of side s is the Pokemon named by order
    byte 177 + q of the side's 184 bytes; order id 0 or stored hp 0 -> dead; else the 24 stored bytes with hp (bytes 18-19) dropped,
    each move's PP byte reduced to has-PP and the status byte replaced by its encoder index + 1 (0: none), the sleep turns being
    (side's durations word >> 3 (q + 1)) & 7.  battles [n, 384], durations [n, 8] -> keys uint8 [n, 10, 24] (item = side * 5 + q;
    a dead slot's key is all 0xFF, which no live key is: its byte 19 is 0), live bool [n, 10]."""
    b = np.ascontiguousarray(battles, dtype=np.uint8)
    n = b.shape[0]
    sides = b[:, :368].reshape(n, 2, 184)
    ids = sides[:, :, 177:182].astype(np.int64)                                  # [n, 2, 5]
    party = sides[:, :, :144].reshape(n, 2, 6, 24)
    pk = np.take_along_axis(party, np.maximum(ids - 1, 0)[..., None], axis=2)     # [n, 2, 5, 24]
    hp = pk[..., 18].astype(np.uint32) | (pk[..., 19].astype(np.uint32) << 8)
    live = (ids != 0) & (hp != 0)
    dur = np.ascontiguousarray(durations, dtype=np.uint8).view("<u4").reshape(n, 2).astype(np.uint32)
    sleep = (dur[:, :, None] >> (3 * np.arange(1, 6, dtype=np.uint32))[None, None, :]) & 7    # [n, 2, 5]
    key = pk.copy()
    key[..., 18:20] = 0
    key[..., 11:18:2] = key[..., 11:18:2] != 0
    key[..., 20] = np.where(pk[..., 20] != 0, _status_key_table()[pk[..., 20], sleep], 0)
    key[~live] = 0xFF
    return key.reshape(n, 10, 24), live.reshape(n, 10)


def expected_recomputes(prev_keys, keys, live):
    """The slots a cached call must re-embed: the live ones whose key differs from the previous call's (every live slot on the first
    call, prev_keys None)."""
    if prev_keys is None:
        return int(live.sum())
    return int((live & (prev_keys != keys).any(axis=-1)).sum())


# ---- one field of one bench slot at a time (tests of the cache key) ----------------------------------------------------------
def bench_slot_choice(battles, seed):
    """Per lane, the (side, order position 1-5) of a live bench Pokemon, chosen at random (any bench position where none is live)."""
    rng = np.random.default_rng(seed)
    n = battles.shape[0]
    side, pos = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        cand = []
        for s in range(2):
            for p in range(1, 6):
                pid = int(battles[i, 184 * s + 176 + p])
                if pid and (int(battles[i, 184 * s + 24 * (pid - 1) + 18]) | int(battles[i, 184 * s + 24 * (pid - 1) + 19])):
                    cand.append((s, p))
        if not cand:
            cand = [(int(rng.integers(0, 2)), int(rng.integers(1, 6)))]
        side[i], pos[i] = cand[int(rng.integers(0, len(cand)))]
    return side, pos


def _other(rng, cur, lo, hi):
    """A random value in [lo, hi] other than cur."""
    v = int(rng.integers(lo, hi))
    return v + 1 if v >= cur else v


SLEEP_STATUS, REST = 0x07, 0x80


def bench_slot_mutations():
    """The mutation classes, in the order they are applied (several need the state the one before left: hp restored after hp 0, PP back
    from 0, a sleep after PAR ...).  Each is (name, fn(b, d, side, pos, rng, memo)) editing ONE bench slot of every lane in place
    (b [n, 384], d [n, 8]); only valid field values are written (type nibbles 0-14, move ids 0-165, real statuses)."""
    def pk_off(b, i, s, p):
        pid = int(b[i, 184 * s + 176 + p])
        return 184 * s + 24 * (pid - 1) if pid else None

    def each(f):
        def run(b, d, side, pos, rng, memo):
            for i in range(b.shape[0]):
                o = pk_off(b, i, int(side[i]), int(pos[i]))
                if o is not None:
                    f(b, d, i, int(side[i]), int(pos[i]), o, rng, memo)
        return run

    def u16(b, i, o):
        return int(b[i, o]) | (int(b[i, o + 1]) << 8)

    def put16(b, i, o, v):
        b[i, o], b[i, o + 1] = v & 0xFF, v >> 8

    def set_hp(b, d, i, s, p, o, rng, memo):
        if u16(b, i, o + 18):
            put16(b, i, o + 18, _other(rng, u16(b, i, o + 18), 1, max(u16(b, i, o), 2)))

    def hp_zero(b, d, i, s, p, o, rng, memo):
        memo["hp", i] = u16(b, i, o + 18)
        put16(b, i, o + 18, 0)

    def hp_restore(b, d, i, s, p, o, rng, memo):
        put16(b, i, o + 18, memo.get(("hp", i), 0))

    def stat(k):
        def f(b, d, i, s, p, o, rng, memo):
            put16(b, i, o + 2 * k, _other(rng, u16(b, i, o + 2 * k), 1, 999))
        return f

    def move(m):
        def f(b, d, i, s, p, o, rng, memo):
            b[i, o + 10 + 2 * m] = (0, 165, _other(rng, int(b[i, o + 10 + 2 * m]), 1, 164))[i % 3]
        return f

    def pp_slot(b, i, o):                  # a move slot with PP, slot i % 4 first: every slot's has-PP bit gets its turn
        for m in range(i, i + 4):
            if b[i, o + 11 + 2 * (m % 4)]:
                return m % 4
        return None

    def pp_change(b, d, i, s, p, o, rng, memo):
        m = pp_slot(b, i, o)
        if m is not None:
            b[i, o + 11 + 2 * m] = _other(rng, int(b[i, o + 11 + 2 * m]), 1, 63)

    def pp_zero(b, d, i, s, p, o, rng, memo):
        m = pp_slot(b, i, o)
        memo["pp", i] = (m, int(b[i, o + 11 + 2 * m])) if m is not None else None
        if m is not None:
            b[i, o + 11 + 2 * m] = 0

    def pp_back(b, d, i, s, p, o, rng, memo):
        if memo.get(("pp", i)) is not None:
            m, pp = memo["pp", i]
            b[i, o + 11 + 2 * m] = pp

    def set_turns(d, i, s, p, v):          # the sleep turns of order position p: bits 3p .. 3p + 2 of the side's durations word
        w = int.from_bytes(bytes(d[i, 4 * s:4 * s + 4]), "little")
        w = (w & ~(7 << (3 * p))) | (v << (3 * p))
        d[i, 4 * s:4 * s + 4] = np.frombuffer(w.to_bytes(4, "little"), np.uint8)

    def status(v, turns=None):
        def f(b, d, i, s, p, o, rng, memo):
            b[i, o + 20] = v(rng) if callable(v) else v
            if turns is not None:
                set_turns(d, i, s, p, turns)
        return f

    def turns_change(b, d, i, s, p, o, rng, memo):
        w = int.from_bytes(bytes(d[i, 4 * s:4 * s + 4]), "little")
        set_turns(d, i, s, p, _other(rng, (w >> (3 * p)) & 7, 0, 7))

    def sleep_counter(b, d, i, s, p, o, rng, memo):
        st = int(b[i, o + 20])
        b[i, o + 20] = (st & ~SLEEP_STATUS) | _other(rng, st & SLEEP_STATUS, 1, 7)

    def byte(k, lo, hi):
        def f(b, d, i, s, p, o, rng, memo):
            b[i, o + k] = _other(rng, int(b[i, o + k]), lo, hi)
        return f

    def types(b, d, i, s, p, o, rng, memo):
        t = int(b[i, o + 22])
        while int(b[i, o + 22]) == t:
            b[i, o + 22] = int(rng.integers(0, 15)) | (int(rng.integers(0, 15)) << 4)

    def swap_bench(b, d, side, pos, rng, memo):
        for i in range(b.shape[0]):
            a, c = 184 * int(side[i]) + 176 + int(pos[i]), 184 * int(side[i]) + 176 + 1 + int(pos[i]) % 5
            b[i, a], b[i, c] = b[i, c], b[i, a]

    def swap_active(b, d, side, pos, rng, memo):
        for i in range(b.shape[0]):
            a, c = 184 * int(side[i]) + 176, 184 * int(side[i]) + 176 + int(pos[i])
            b[i, a], b[i, c] = b[i, c], b[i, a]

    def empty(b, d, side, pos, rng, memo):
        for i in range(b.shape[0]):
            b[i, 184 * int(side[i]) + 176 + int(pos[i])] = 0

    clear = ("status_clear", each(status(0)))
    return [
        ("none", lambda *a: None),
        ("hp", each(set_hp)),
        ("hp_zero", each(hp_zero)),
        ("hp_restore", each(hp_restore)),
    ] + [("stat_%s" % nm, each(stat(k))) for k, nm in enumerate(("hp_max", "atk", "def", "spe", "spc"))] + [
        ("move_%d" % (m + 1), each(move(m))) for m in range(4)] + [
        ("pp_nonzero_to_nonzero", each(pp_change)),
        ("pp_to_zero", each(pp_zero)),
        ("pp_from_zero", each(pp_back)),
        clear, ("status_psn", each(status(0x08))),
        clear, ("status_brn", each(status(0x10))),
        clear, ("status_frz", each(status(0x20))),
        clear, ("status_par", each(status(0x40, turns=0))),
        ("par_to_sleep_turns_0", each(status(lambda rng: int(rng.integers(1, 8))))),
        ("sleep_counter", each(sleep_counter)),
        ("sleep_turns_asleep", each(turns_change)),
        clear, ("status_sleep", each(status(lambda rng: int(rng.integers(1, 8))))),
        clear, ("status_rest", each(status(lambda rng: REST | int(rng.integers(1, 3))))),
        ("sleep_turns_rest", each(turns_change)),
        clear, ("sleep_turns_awake", each(turns_change)),
        ("species", each(byte(21, 1, 151))),
        ("level", each(byte(23, 1, 100))),
        ("types", each(types)),
        ("swap_bench", swap_bench),
        ("swap_active", swap_active),
        ("empty_slot", empty),
    ]


def midgame_batch(n, seed0, steps=(20, 30, 40)):
    """n random OU battles, consecutive thirds advanced steps[0] / [1] / [2] random turn-steps on the oracle -> (battles, durations)."""
    b, d, p, r = make_random_ou_batch(n, seed0=seed0)
    parts = np.array_split(np.arange(n), len(steps))
    for k, idx in zip(steps, parts):
        bb, dd, pp, rr = (np.ascontiguousarray(x[idx]) for x in (b, d, p, r))
        rollout_batch(bb, dd, rr, pp, max_steps=k, threads=4)
        b[idx], d[idx] = bb, dd
    return b, d
