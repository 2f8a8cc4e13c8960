"""Test helper for the whole-game loop (tests/test_policy_games_ref.py on the CPU, tests/test_gpu_policy_games.py on the GPU): the
reference's fast_prng in Python, the policy rule of a POLICY seat in float64, the draw rules of a turn, and a game replayer over the
oracle.  numpy + the oracle only."""
import numpy as np

import oracle_lib as O

M32 = 0xFFFFFFFF
BOUNDARY_EPS = 1e-5     # a draw this close to a cumulative boundary of the float64 policy may fall either side on the device (fp32 expf)
RANDOM, POLICY = 0, 1


class FastPrng:
    """fast_prng (cpp/include/util/random.h:67-133) over its 8 state bytes."""

    def __init__(self, state8):
        s = bytes(bytearray(np.asarray(state8, dtype=np.uint8).reshape(8).tolist()))
        self.s0, self.s1 = int.from_bytes(s[:4], "little"), int.from_bytes(s[4:], "little")

    @staticmethod
    def _rotl(x, k):
        return ((x << k) | (x >> (32 - k))) & M32

    def next32(self):
        result = (self._rotl((self.s0 + self.s1) & M32, 9) + self.s0) & M32
        self.s1 ^= self.s0
        self.s0 = self._rotl(self.s0, 13) ^ self.s1 ^ ((self.s1 << 5) & M32)
        self.s1 = self._rotl(self.s1, 28)
        return result

    def next64(self):
        hi = self.next32()
        return (hi << 32) | self.next32()

    uniform_64 = next64

    def uniform(self):
        return (self.next64() >> 11) * (1.0 / (1 << 53))

    def state(self):
        return np.frombuffer(self.s0.to_bytes(4, "little") + self.s1.to_bytes(4, "little"), dtype=np.uint8).copy()


def policy(logits, temp=1.0, minp=0.0):
    """The policy of a POLICY seat over its k legal logits: prior_i = expf(l_i) / sum with the sum in fp32 in index order and the quotient
    in double (search/util/softmax.h:5-15 into MCTS::Output's doubles), pow(x, temp) renormalised when temp != 1, entries below `min`
    zeroed, renormalised (util/policy.h:70-95).  float64 [k], or None when every entry was zeroed."""
    l = np.asarray(logits, dtype=np.float32)
    ex = np.exp(l)
    s = np.float32(0)
    for y in ex:
        s = np.float32(s + y)
    p = ex.astype(np.float64) / np.float64(s)
    if temp != 1:
        p = np.power(p, temp)
        p = p / p.sum()
    p = np.where(p < minp, 0.0, p)
    total = p.sum()
    if total == 0:
        return None
    return p / total


def sample_pdf(p, u):
    """fast_prng::sample_pdf (random.h:123-132) of the draw u: subtract in double, the first index with p <= 0, else 0."""
    for i, x in enumerate(p):
        u -= float(x)
        if u <= 0.0:
            return i
    return 0


def boundary_distance(p, u):
    """How far the draw lies from the nearest interior cumulative boundary of the policy (inf for a single entry)."""
    if len(p) < 2:
        return np.inf
    return float(np.abs(np.cumsum(p)[:-1] - u).min())


def turn_draws(seats, stream, k1, k2, logits1=None, logits2=None):
    """One turn's draws from the game's stream.  seats: ((kind, temp, min), (kind, temp, min)).  Returns per seat (index, policy or
    None, draw or None): the rule's index into the seat's legal choices, with the policy and the uniform it was sampled with for a
    POLICY seat that had a choice."""
    if seats[0][0] == RANDOM and seats[1][0] == RANDOM:   # the rollout's rule: one draw for both (mcts.h:448-496)
        seed = stream.uniform_64()
        return (seed % k1, None, None), ((seed >> 32) % k2, None, None)
    out = []
    for (kind, temp, minp), k, logits in ((seats[0], k1, logits1), (seats[1], k2, logits2)):
        if kind == RANDOM:
            out.append((stream.uniform_64() % k, None, None))
        elif k == 1:
            out.append((0, None, None))                   # no draw (vs.cc:258,273)
        else:
            u = stream.uniform()
            p = policy(logits[:k], temp if temp else 1.0, minp)
            out.append((sample_pdf(p, u), p, u))
    return tuple(out)


def replay_game(battle, durations, result, log, turns):
    """One game's choice log on the oracle from its starting state.  Returns (states, final): states[t] = (battle, durations, result,
    p1 legal choices, p2 legal choices) in front of turn t for t < turns, final = (battle, durations, result).  Asserts that every
    logged choice is legal and that no turn is played from a finished state."""
    b, r = np.array(battle, dtype=np.uint8), int(result)
    opts = O.Options(np.asarray(durations, dtype=np.uint8))
    states = []
    for t in range(int(turns)):
        assert (r & 15) == 0, ("a turn was played after the game ended", t)
        o1, o2 = O.choices(b, 0, (r >> 4) & 3), O.choices(b, 1, (r >> 6) & 3)
        c1, c2 = int(log[t][0]), int(log[t][1])
        assert c1 in o1 and c2 in o2, ("illegal logged choice", t, c1, list(o1), c2, list(o2))
        states.append((b.copy(), opts.durations.copy(), r, o1, o2))
        r = int(O.update(b, c1, c2, opts))
    return states, (b, opts.durations.copy(), r)


def exclusion_share(picks, rng, stream, eps=BOUNDARY_EPS):
    """The share of `picks` synthetic picks -- a random policy over 2..9 choices, a uniform draw of the Python stream -- whose draw lies
    within eps of an interior cumulative boundary (the turns a GPU test may leave out)."""
    near = 0
    for _ in range(picks):
        k = int(rng.integers(2, 10))
        p = policy(rng.normal(0.0, 2.0, size=k).astype(np.float32))
        near += boundary_distance(p, stream.uniform()) <= eps
    return near / picks
