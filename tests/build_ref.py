"""A numpy referee of the team-building rollout (oak_amd/csrc/buildnet.hip), written from the contract in include/oakgpu.h:
the index tables from the JSON, the legal lists (Encode::Build::Actions), a float64 and a float32 forward of the policy net, the
softmax and pick rules with the reference's types (expf in float, the sum in double in list order, each quotient rounded to float;
sample_pdf walks the list with p -= (double)policy[i], stops at p <= 0 and falls back to 0), Omitter::delete_info, the provider's
prelude, and the CompressedTrajectory codec.

A team is uint8[30] (6 x {species, 4 moves}) with a size: the slots in play.  Every function that takes `mistake` plants one
deliberate error by name; tests/test_build_ref.py shows that the checks catch each of them."""
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = json.load(open(os.path.join(ROOT, "oak_amd", "data", "gen1_data.json")))
LEGAL = [int(s) for s in DATA["ou_legal_species"]]
POOLS = {int(k): [int(m) for m in v] for k, v in DATA["ou_move_pools"].items()}
F = np.float32
MASK = (1 << 64) - 1
MAX_STEPS = 31


def _tables():
    table = -np.ones((152, 166), np.int32)
    cells = []
    for s in LEGAL:
        for m in [0] + POOLS[s]:
            table[s, m] = len(cells)
            cells.append((s, m))
    return table, np.array(cells, np.uint8)


TABLE, LIST = _tables()
N_DIM = len(LIST)
MAX_ACTIONS = sum(sorted((len(POOLS[s]) for s in LEGAL), reverse=True)[:5]) + len(LEGAL) - 5
# the policy against the float64 softmax of the device's own logits, relative: expf is good to 1 ulp (2 x 2^-24 relative at worst) in the
# numerator and, as a weighted mean of the same errors, in the sum; the sum itself is accumulated in double (339 roundings of 2^-53:
# nothing); the quotient is rounded to float once (2^-24).  5 x 2^-24, rounded up to 6.  (forest_ref.PRIOR_BOUND's derivation with
# the fp32 sum's 8 roundings replaced by the double sum's.)
POLICY_BOUND = 6 * 2.0 ** -24


# ---- the stream: selfplay_pick.hpp's splitmix64 ---------------------------------------------------------------------------------------
class Stream:
    GOLDEN = 0x9E3779B97F4A7C15

    def __init__(self, seed):
        self.x = int(seed) & MASK

    def next(self):
        self.x = (self.x + self.GOLDEN) & MASK
        z = self.x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)

    def uniform(self):
        return (self.next() >> 11) * (1.0 / 9007199254740992.0)


# ---- teams ------------------------------------------------------------------------------------------------------------------------------
def team_of(sets):
    """[(species, [moves...]), ...] -> uint8[30]."""
    t = np.zeros((6, 5), np.uint8)
    for i, (s, moves) in enumerate(sets):
        t[i, 0] = s
        t[i, 1:1 + len(moves)] = moves
    return t.reshape(30)


def sample_teams():
    """The 16 sample teams as uint8[16, 30]."""
    from oak_amd import gamedata as G
    teams = json.load(open(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json")))["teams"]
    return np.stack([team_of([(G.species_id(r[0]), [G.move_id(m) for m in r[1:]]) for r in t]) for t in teams])


def write_x(team, size):
    """Tensorizer::write: the cells of every held (species, None) and (species, move)."""
    x = np.zeros(N_DIM, np.float64)
    t = np.asarray(team, np.uint8).reshape(6, 5)
    for i in range(size):
        if t[i, 0]:
            for m in (0,) + tuple(t[i, 1:]):
                x[TABLE[t[i, 0], m]] = 1.0
    return x


def additions(team, size, mistake=None):
    """Actions::get_singleton_additions as a list of (cell, slot, move_slot, species, move)."""
    t = np.asarray(team, np.uint8).reshape(6, 5)
    species, moves = [], []
    empty = [i for i in range(size) if t[i, 0] == 0]
    if empty:
        held = set(int(t[i, 0]) for i in range(size))
        species = [(int(TABLE[s, 0]), empty[0], 0, s, 0) for s in LEGAL if s not in held]
    for i in range(size):
        s = int(t[i, 0])
        free = [j for j in range(4) if t[i, 1 + j] == 0]
        if s and free:
            held = set(int(m) for m in t[i, 1:])
            moves += [(int(TABLE[s, m]), i, free[0], s, m) for m in POOLS[s] if m not in held]
    return moves + species if mistake == "species_after_moves" else species + moves


def lead_swaps(team, size):
    """Actions::get_lead_swaps as a list of (cell, lead)."""
    t = np.asarray(team, np.uint8).reshape(6, 5)
    return [(int(TABLE[t[i, 0], 0]), i) for i in range(1, size) if t[i, 0]]


def apply_addition(team, action):
    _, slot, move_slot, species, move = action
    t = team.reshape(6, 5)
    if t[slot, 0]:
        t[slot, 1 + move_slot] = move
    else:
        t[slot, 0] = species


def apply_swap(team, lead):
    t = team.reshape(6, 5)
    t[[0, lead]] = t[[lead, 0]]


# ---- the net ----------------------------------------------------------------------------------------------------------------------------
class Net:
    """The policy net of a `.build.net`: three Affine layers (u32 in, u32 out, out f32 biases, out x in f32 weights row-major); the value
    net behind it is read and unused."""

    def __init__(self, data):
        if not isinstance(data, (bytes, bytearray)):
            data = open(data, "rb").read()
        self.layers, pos = [], 0
        for _ in range(6):
            i, o = struct.unpack_from("<II", data, pos)
            b = np.frombuffer(data, "<f4", o, pos + 8)
            w = np.frombuffer(data, "<f4", o * i, pos + 8 + 4 * o).reshape(o, i)
            self.layers.append((w, b))
            pos += 8 + 4 * o + 4 * o * i
        assert pos == len(data)
        self.hidden = self.layers[0][0].shape[0]

    def forward(self, x, dtype=np.float64):
        h = np.asarray(x, dtype)
        for k, (w, b) in enumerate(self.layers[:3]):
            h = w.astype(dtype) @ h + b.astype(dtype)
            if k < 2:
                h = np.maximum(h, 0)
        return h

    def magnitude(self, x):
        """S = sum |w| |x| + |b| through the layers, per logit."""
        s = np.abs(np.asarray(x, np.float64))
        for w, b in self.layers[:3]:
            s = np.abs(w.astype(np.float64)) @ s + np.abs(b.astype(np.float64))
        return s

    def logit_bound(self, x, cells=None):
        """(l64, bound) at `cells` (all of them when None): the project's bound 4 max|l32 - l64| + 2e-7 S (tests/policy_ref.py).  The
        same numbers as forward / magnitude, computed only where they are asked for: x is a few ones, so layer 1 is a sum of columns."""
        cells = np.arange(N_DIM) if cells is None else np.asarray(cells, np.int64)
        nz = np.flatnonzero(np.asarray(x))
        xs = np.asarray(x, np.float64)[nz]
        out = []
        for dtype, absolute in ((np.float64, False), (np.float32, False), (np.float64, True)):
            f = (lambda a: np.abs(a.astype(dtype))) if absolute else (lambda a: a.astype(dtype))
            (w1, b1), (w2, b2), (w3, b3) = self.layers[:3]
            h = f(w1[:, nz]) @ xs.astype(dtype) + f(b1)
            h = h if absolute else np.maximum(h, 0)
            h = f(w2) @ h + f(b2)
            h = h if absolute else np.maximum(h, 0)
            out.append((f(w3[cells]) @ h + f(b3[cells])).astype(np.float64))
        l64, l32, s = out
        return l64, 4 * np.abs(l32 - l64).max() + 2e-7 * s


def softmax(logits):
    """TeamBuilding::softmax on std::vector<float>: expf in float, no maximum subtracted, the sum in double in list order, each quotient
    rounded to float."""
    e = np.exp(np.asarray(logits, F))
    total = 0.0
    for v in e:
        total += float(v)
    return np.array([F(float(v) / total) for v in e], F)


def softmax64(logits):
    y = np.exp(np.asarray(logits, np.float64))
    return y / y.sum()


def pick(policy, u, mistake=None):
    """device.sample_pdf (util/random.h:40-49)."""
    p = float(u)
    for i, q in enumerate(policy):
        p -= float(q)
        if p <= 0:
            return i
    return len(policy) - 1 if mistake == "fallback_last" else 0


# ---- the rollout ------------------------------------------------------------------------------------------------------------------------
class Rollout:
    """One team's rollout, step by step: legal() is the current list of cells (None when the rollout has ended), advance(index) applies
    entry `index` and the input update."""

    def __init__(self, team, size, input_update=0, mistake=None):
        self.team = np.array(team, np.uint8).reshape(30).copy()
        self.team.reshape(6, 5)[size:] = 0
        self.size, self.input_update, self.mistake = int(size), int(input_update), mistake
        self.x = write_x(self.team, self.size)
        self.swapped = False
        self.steps = 0
        self._list()

    def _list(self):
        self.actions = additions(self.team, self.size, self.mistake)
        self.swap = False
        if not self.actions and not self.swapped:
            self.swapped = True
            self.actions = lead_swaps(self.team, self.size)
            self.swap = True

    def legal(self):
        return [a[0] for a in self.actions] if self.actions else None

    def advance(self, index):
        a = self.actions[index]
        if self.swap:
            apply_swap(self.team, a[1])
        else:
            apply_addition(self.team, a)
        self.x[a[0] if (self.input_update == 1 or self.mistake == "x_cell") else index] = 1.0
        self.steps += 1
        if self.swap:
            self.actions = []
        else:
            self._list()
        return a[0]


def rollout(net, team, size, seed, input_update=0, mistake=None, dtype=np.float32):
    """The free-running referee: its own forward, softmax and picks.  Returns a dict shaped like one row of the device's outputs."""
    r, rng = Rollout(team, size, input_update, mistake), Stream(seed)
    out = {"action": [], "index": [], "n_legal": [], "prob": [], "legal": [], "policy": []}
    while r.legal() is not None:
        legal = r.legal()
        policy = softmax(net.forward(r.x, dtype)[legal].astype(F))
        index = pick(policy, rng.uniform(), mistake)
        out["legal"].append(legal)
        out["policy"].append(policy)
        out["index"].append(index)
        out["n_legal"].append(len(legal))
        out["prob"].append(policy[index])
        out["action"].append(r.advance(index))
    out.update(team=r.team, n_updates=r.steps, stream=rng.x)
    return out


# ---- the provider's prelude -------------------------------------------------------------------------------------------------------------
def delete_info(team, size, rng, pokemon_delete_prob, move_delete_prob):
    """Omitter::delete_info, in place; True when anything was deleted."""
    t, modified = team.reshape(6, 5), False
    for i in range(size):
        if t[i, 0] and rng.uniform() < pokemon_delete_prob:
            t[i] = 0
            modified = True
        else:
            for j in range(1, 5):
                if t[i, j] and rng.uniform() < move_delete_prob:
                    t[i, j] = 0
                    modified = True
    return modified


def prelude(pool, seed, max_pokemon=6, pokemon_delete_prob=0.0, move_delete_prob=0.0, team_modify_prob=0.0, mistake=None):
    """Provider::get_trajectory up to the rollout: (team_index, team, size, changed, stream state)."""
    rng = Stream(seed)
    pool = np.asarray(pool, np.uint8).reshape(-1, 30)
    index = rng.next() % pool.shape[0]
    team = pool[index].copy()
    count = int((team.reshape(6, 5)[:, 0] != 0).sum())
    size = min(count, max_pokemon)
    changed = size < count
    team.reshape(6, 5)[size:] = 0
    if rng.uniform() < team_modify_prob and (not changed or mistake == "delete_after_truncation"):
        changed = delete_info(team, size, rng, pokemon_delete_prob, move_delete_prob) or changed
    return index, team, size, changed, rng.x


# ---- records ----------------------------------------------------------------------------------------------------------------------------
def initial_cells(team, size):
    t = np.asarray(team, np.uint8).reshape(6, 5)
    cells = []
    for i in range(size):
        if t[i, 0]:
            cells.append(int(TABLE[t[i, 0], 0]))
            cells += [int(TABLE[t[i, 0], m]) for m in t[i, 1:] if m]
    return cells


def compress_probability(p):
    q = int(F(65535.0) * F(p))
    return 1 if (p != 0 and q == 0) else q


def encode_record(team, size, actions, probs, value, score):
    """One CompressedTrajectory NoTeam record (128 bytes).  score None: no score."""
    ups = [(c, 0) for c in initial_cells(team, size)] + [(int(a), compress_probability(p)) for a, p in zip(actions, probs)]
    assert len(ups) <= MAX_STEPS
    ups += [(0, 0)] * (MAX_STEPS - len(ups))
    head = struct.pack("<BBH", 0, 255 if score is None else int(F(2) * F(score)), int(F(value) * F(65535.0)))
    return head + b"".join(struct.pack("<HH", a, p) for a, p in ups)


def decode_record(data):
    _, score, value = struct.unpack_from("<BBH", data, 0)
    ups = np.frombuffer(data, "<u2", 62, 4).reshape(31, 2)
    return {"score": None if score == 255 else score / 2.0, "value": value / 65535.0, "action": ups[:, 0].copy(), "probability": ups[:, 1].copy()}


# ---- the planted teams of the tests and of tests/golden/make_build_goldens.py ---------------------------------------------------------
def planted_teams():
    """[(name, team uint8[30], size)]: the edge cases by name, then random deletions from the sample teams."""
    samples = sample_teams()
    by_size = sorted(LEGAL, key=lambda s: (len(POOLS[s]), s))
    one = next(s for s in by_size if len(POOLS[s]) == 1)                 # a pool of exactly one move
    small = next(s for s in by_size if 1 < len(POOLS[s]) < 4)            # a pool under four
    three = next(s for s in by_size if len(POOLS[s]) == 3)
    full = samples[0].copy()
    out = [("empty", np.zeros(30, np.uint8), 6), ("complete", full.copy(), 6), ("complete_size1", full.copy(), 1)]
    t = full.copy(); t.reshape(6, 5)[2, 3] = 0
    out.append(("one_missing_move", t, 6))
    t = full.copy(); t.reshape(6, 5)[4] = 0
    out.append(("one_missing_pokemon", t, 6))
    t = full.copy(); t.reshape(6, 5)[1] = 0; t.reshape(6, 5)[1, 0] = small
    out.append(("pool_under_four", t, 6))
    t = full.copy(); t.reshape(6, 5)[3] = 0; t.reshape(6, 5)[3, 0] = one
    out.append(("pool_of_one", t, 6))
    t = full.copy(); t.reshape(6, 5)[5] = [three] + POOLS[three] + [0]
    out.append(("pool_used_up", t, 6))
    t = full.copy(); t.reshape(6, 5)[0] = [one, POOLS[one][0], 0, 0, 0]; t.reshape(6, 5)[1] = 0
    out.append(("pool_of_one_used_up_and_a_gap", t, 6))
    t = full.copy(); t.reshape(6, 5)[1, 1:] = 0
    out.append(("size2", t, 2))
    t = full.copy(); t.reshape(6, 5)[3] = 0; t.reshape(6, 5)[0, 2] = 0
    out.append(("size5", t, 5))
    t = np.zeros(30, np.uint8); t.reshape(6, 5)[2] = full.reshape(6, 5)[2]
    out.append(("gap_before_a_pokemon", t, 6))
    t = full.copy(); t.reshape(6, 5)[0, 1] = 0; t.reshape(6, 5)[0, 3] = 0
    out.append(("move_gap_in_the_middle", t, 6))
    rng = np.random.default_rng(25)
    for k in range(11):
        t = samples[(k * 3 + 1) % 16].copy().reshape(6, 5)
        for i in range(6):
            if rng.random() < 0.3:
                t[i] = 0
            else:
                t[i, 1:][rng.random(4) < 0.4] = 0
        out.append(("deleted_%d" % k, t.reshape(30), 6 if k % 4 else 4))
    return out
