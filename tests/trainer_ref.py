"""Test helper for the trainer (tests/test_trainer_ref.py on the CPU, tests/test_gpu_trainer.py on the GPU): the forward on training
rows, battle.py's loss, its gradient and Adam, written from the contract in include/oakgpu.h ("Training the battle network") as a torch
CPU module -- in float64 as the referee, in float32 as the plain evaluation whose own distance from float64 sizes the bounds -- with
the gradient by autograd and Adam by formula; the referee's planted mistakes for the discrimination check; the rows both test files
use.  TEST INFRASTRUCTURE ONLY.

A batch is a dict of numpy arrays by the names of oak_amd.train.FIELDS (what train_ref.Corpus.expected returns).  loss = (wn, we, ws, pn,
value_weight, policy_weight), rounded to fp32 as the device reads them."""
import struct

import numpy as np
import torch

F = np.float32
LAYERS = ("p0", "p1", "a0", "a1", "fc0", "fc1", "v2", "v3", "q1a", "q1b", "q2a", "q2b")
GROUP = {"p0": 0, "p1": 0, "a0": 0, "a1": 0, "fc0": 0, "fc1": 0, "v2": 1, "v3": 1, "q1a": 2, "q1b": 2, "q2a": 2, "q2b": 2}
VARIANTS = ("nomask", "k", "mean_n", "swap", "bf16")
RAGGED = dict(pokemon_hidden=33, pokemon_out=7, active_hidden=65, active_out=9, hidden=31, value_hidden=5, policy_hidden=17)
B1, B2, EPS = 0.9, 0.999, 1e-8


def read_net(data):
    """(activation 1 relu / 2 clamp, [(bias [out], weight [out, in]) x 12]) of `.battle.net` bytes."""
    act, off, layers = data[0] + 1, 8, []
    for _ in range(12):
        n_in, n_out = struct.unpack_from("<II", data, off)
        off += 8
        b = np.frombuffer(data, "<f4", n_out, off).copy()
        off += 4 * n_out
        W = np.frombuffer(data, "<f4", n_out * n_in, off).copy().reshape(n_out, n_in)
        off += 4 * n_out * n_in
        layers.append((b, W))
    assert off == len(data)
    return act, layers


def flat(layers):
    """The 24 tensors back to back in file order (the device's block layout)."""
    return np.concatenate([np.concatenate([np.asarray(b).reshape(-1), np.asarray(W).reshape(-1)]) for b, W in layers])


class Ref(torch.nn.Module):
    """The network of a `.battle.net` in `dtype`.  run(batch, n, loss) -> dict with the forward outputs on the rows (0 for a row that is not
    OK), the report, and after backward() the gradients and the sums S the gradient bound is made of."""

    def __init__(self, data, dtype=torch.float64, variant=None):
        super().__init__()
        assert variant is None or variant in VARIANTS
        self.dtype, self.variant, self.keep, self.kept = dtype, variant, True, {}
        self.activation, layers = read_net(data)
        for name, (b, W) in zip(LAYERS, layers):
            self.register_parameter(name + "_b", torch.nn.Parameter(torch.tensor(b, dtype=dtype)))
            self.register_parameter(name + "_w", torch.nn.Parameter(torch.tensor(W, dtype=dtype)))

    def act(self, x):
        return torch.relu(x) if self.activation == 1 else torch.clamp(x, 0.0, 1.0)

    def affine(self, name, x, activate=True):
        """x W^T + b, kept (with its input) for the bound's sums."""
        z = x @ getattr(self, name + "_w").T + getattr(self, name + "_b")
        if self.keep:
            z.retain_grad()
            self.kept[name] = (x.detach().reshape(-1, x.shape[-1]), z)
        return self.act(z) if activate else z

    def masked(self, emb, mask):
        if self.variant == "nomask":   # the planted mistake: the hp mask applied to the forward only
            return emb + (emb * mask - emb).detach()
        return emb * mask

    def loss_of(self, pokemon, active, hp, idx, k, emp, nash, empirical_value, nash_value, score, denom, loss):
        """The loss of r OK rows from torch tensors on the module's device (pokemon [r,2,6,198], active [r,2,1,229], hp [r,2,6,1], idx int64
        [r,2,9], k int64 [r,2], policies [r,2,9], targets [r]) with the means taken over `denom` rows: (loss, (value, logits [r,2,9], sq_err,
        ce [r,2], mse, ce_p1, ce_p2))."""
        T = self.dtype
        wn, we, ws, pn, vw, pw = loss
        r = pokemon.shape[0]
        xp = pokemon[:, :, 1:6]
        xa = torch.cat([active[:, :, 0], pokemon[:, :, 0]], dim=2)
        ep = self.masked(self.affine("p1", self.affine("p0", xp)), (hp[:, :, 1:6] != 0).to(T))
        ea = self.masked(self.affine("a1", self.affine("a0", xa)), (hp[:, :, 0] != 0).to(T))
        sides = torch.cat([hp[:, :, 0], ea, torch.cat([hp[:, :, 1:6], ep], dim=3).reshape(r, 2, -1)], dim=2)
        h = self.affine("fc1", self.affine("fc0", sides.reshape(r, -1)))
        value = torch.sigmoid(self.affine("v3", self.affine("v2", h), activate=False))[:, 0]
        if self.variant == "swap":
            emp, nash = nash, emp
        vt = (wn * nash_value + we * empirical_value) + ws * score
        sq = (value - vt) ** 2
        live = torch.arange(9, device=k.device)[None, None, :] < k[:, :, None]
        safe = torch.where(live, idx, torch.zeros_like(idx))
        ces, logits = [], []
        for s, (a, b) in enumerate((("q1a", "q1b"), ("q2a", "q2b"))):
            full = self.affine(b, self.affine(a, h), activate=False)                       # [r, 315]
            lg = torch.gather(full, 1, safe[:, s])
            lg = torch.where(live[:, s], lg, torch.full_like(lg, -float("inf")))
            logp = torch.log_softmax(lg, dim=1)
            tg = torch.where(live[:, s], (1.0 - pn) * emp[:, s] + pn * nash[:, s], torch.zeros_like(lg))
            support = torch.clamp((tg != 0).sum(dim=1), min=1).to(T) if self.variant != "k" else k[:, s].to(T)
            ces.append(-(tg * torch.where(live[:, s], logp, torch.zeros_like(logp))).sum(dim=1) / support)
            logits.append(torch.where(live[:, s], lg, torch.zeros_like(lg)))
        mse, ce1, ce2 = sq.sum() / denom, ces[0].sum() / denom, ces[1].sum() / denom
        return vw * mse + pw * (ce1 + ce2), (value, torch.stack(logits, dim=1), sq, torch.stack(ces, dim=1), mse, ce1, ce2)

    def run(self, batch, n, loss):
        T = self.dtype
        wn, we, ws, pn, vw, pw = (float(F(x)) for x in loss)
        status = np.asarray(batch["status"][:n])
        ok = np.nonzero(status == 0)[0]
        t = lambda name: torch.tensor(np.asarray(batch[name][:n])[ok].astype(np.float64), dtype=T)
        self.kept = {}
        r = len(ok)
        out = {"value": np.zeros(n), "logits": np.zeros((n, 2, 9)), "sq_err": np.zeros(n), "ce": np.zeros((n, 2)), "rows": r, "ok": ok}
        self.out = out
        if r == 0:
            out.update(loss=0.0, mse=0.0, ce_p1=0.0, ce_p2=0.0)
            self.loss = None
            return out
        idx = torch.tensor(np.asarray(batch["choice_indices"][:n])[ok].astype(np.int64))
        k = torch.tensor(np.asarray(batch["k"][:n])[ok].astype(np.int64)).reshape(r, 2)
        self.loss, (value, logits, sq, ces, mse, ce1, ce2) = self.loss_of(
            t("pokemon"), t("active"), t("hp"), idx, k, t("empirical_policies"), t("nash_policies"), t("empirical_value")[:, 0], t("nash_value")[:, 0],
            t("score")[:, 0], float(n if self.variant == "mean_n" else r), (wn, we, ws, pn, vw, pw))
        self.weights = (vw, pw)
        out["value"][ok] = value.detach().double().numpy()
        out["logits"][ok] = logits.detach().double().numpy()
        out["sq_err"][ok] = sq.detach().double().numpy()
        out["ce"][ok] = ces.detach().double().numpy()
        out.update(loss=float(self.loss.detach()), mse=float(mse.detach()), ce_p1=float(ce1.detach()), ce_p2=float(ce2.detach()))
        return out

    def backward(self):
        """-> (grads, S): grads = 12 (bias, weight) pairs of float64 numpy (None for a group that received none); S = 12 (S_bias, S_weight):
        the largest over entries of sum_rows |dZ| and of sum_rows |dZ| |X| -- what one fp32 rounding of an entry's sum is measured in."""
        for p in self.parameters():
            p.grad = None
        grads, S = [], []
        if self.loss is None:
            shapes = [(getattr(self, n + "_b"), getattr(self, n + "_w")) for n in LAYERS]
            return [(np.zeros(b.shape), np.zeros(w.shape)) for b, w in shapes], [(0.0, 0.0)] * 12
        self.loss.backward()
        vw, pw = self.weights
        for name in LAYERS:
            b, w = getattr(self, name + "_b"), getattr(self, name + "_w")
            dead = (GROUP[name] == 1 and vw == 0.0) or (GROUP[name] == 2 and pw == 0.0)
            if dead:
                grads.append(None)
                S.append((0.0, 0.0))
                continue
            gw = w.grad.detach().double().numpy().copy()
            if self.variant == "bf16" and name == "fc0":
                gw = torch.tensor(gw).to(torch.bfloat16).double().numpy()
            grads.append((b.grad.detach().double().numpy().copy(), gw))
            x, z = self.kept[name]
            dz = z.grad.detach().double().abs().reshape(-1, z.shape[-1])
            S.append((float(dz.sum(dim=0).max()), float((dz.T @ x.double().abs()).max())))
        return grads, S

    def layers(self):
        return [(getattr(self, n + "_b").detach().double().numpy(), getattr(self, n + "_w").detach().double().numpy()) for n in LAYERS]


def gradient_bound(g32, g64, S):
    """max |g_dev - g64| allowed for one tensor: four times the fp32 referee's own distance from float64 plus 2e-7 of S."""
    return 4.0 * float(np.abs(np.asarray(g32) - np.asarray(g64)).max()) + 2e-7 * S


# ---- Adam by formula -----------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, t):
    """The two scalars the host computes in double per step and passes as floats: lr / (1 - b1^t), sqrt(1 - b2^t)."""
    return float(F(lr / (1.0 - B1 ** t))), float(F(np.sqrt(1.0 - B2 ** t)))


def adam_formula(p, g, m, v, t, lr, float_scalars=True, clamp=None):
    """One Adam step in float64 on arrays: -> (p, m, v, update).  float_scalars: the step size and the second bias correction rounded to fp32
    as the device receives them.  clamp: a boolean array, True where the parameter is clamped to [-2, 2] after the update."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    m = B1 * m + (1.0 - B1) * g
    v = B2 * v + (1.0 - B2) * g * g
    step, bc2 = adam_scalars(lr, t) if float_scalars else (lr / (1.0 - B1 ** t), np.sqrt(1.0 - B2 ** t))
    update = step * (m / (np.sqrt(v) / bc2 + EPS))
    p = p - update
    if clamp is not None:
        p = np.where(clamp, np.clip(p, -2.0, 2.0), p)
    return p, m, v, update


# ---- the rows of the tests ------------------------------------------------------------------------------------------------------------
def synthetic_rows(n=12, seed=5, pod_alive=True):
    """Rows built for the edges the real ones do not reach, as a batch dict (all OK): row 0 has k = 1 on side 0; row 1 an all-zero target on
    side 1 (support clamped to 1); row 2 every bench slot dead on both sides; row 3 hp 0 actives (their tensors zero, as the encoder
    leaves them); rows 4.. share one choice_indices value (7) at different positions; the rest are random.  Inputs are 0/1 patterns and
    quotients like the encoder's."""
    rng = np.random.default_rng(seed)
    b = {
        "pokemon": (rng.random((n, 2, 6, 198)) < 0.08).astype(F) * rng.choice(np.array([1.0, 0.5, 0.25], F), (n, 2, 6, 198)),
        "active": (rng.random((n, 2, 1, 229)) < 0.1).astype(F),
        "hp": rng.random((n, 2, 6, 1)).astype(F),
        "choice_indices": np.full((n, 2, 9), 315, np.int64),
        "k": rng.integers(2, 10, (n, 2, 1)).astype(np.uint8),
        "choice": np.zeros((n, 2, 1), np.uint8), "iterations": np.ones((n, 1), np.uint32),
        "empirical_policies": np.zeros((n, 2, 9), F), "nash_policies": np.zeros((n, 2, 9), F),
        "empirical_value": rng.random((n, 1)).astype(F), "nash_value": rng.integers(0, 2, (n, 1)).astype(F),
        "score": rng.choice(np.array([0.0, 0.5, 1.0], F), (n, 1)), "status": np.zeros(n, np.uint8), "where": np.zeros(n, np.uint32),
    }
    b["k"][0, 0, 0] = 1
    for i in range(n):
        for s in range(2):
            k = int(b["k"][i, s, 0])
            b["choice_indices"][i, s, :k] = rng.choice(315, k, replace=False)
            for name in ("empirical_policies", "nash_policies"):
                p = rng.dirichlet(np.ones(k)) * (rng.random(k) < 0.7)
                b[name][i, s, :k] = (np.round(p / max(p.sum(), 1e-9) * 65535.0).astype(F) / F(65535.0))
    b["empirical_policies"][1, 1] = 0
    b["nash_policies"][1, 1] = 0
    b["hp"][2, :, 1:] = 0
    b["pokemon"][2, :, 1:] = 0
    b["hp"][3, :, 0] = 0
    b["pokemon"][3, :, 0] = 0
    b["active"][3] = 0
    for i in range(4, n):                                   # one index named by many rows, at different positions
        for s in range(2):
            k = int(b["k"][i, s, 0])
            row = b["choice_indices"][i, s]
            if 7 not in row[:k]:
                row[(i + s) % k] = 7
    return b


def concat(batches):
    return {name: np.concatenate([b[name] for b in batches]) for name in batches[0]}


def take(batch, index):
    return {name: np.ascontiguousarray(a[index]) for name, a in batch.items()}


def spoil(batch, rows):
    """The batch with rows `rows` not OK and filled with NaN / garbage indices (status 2), and the same with zeros there: (nan, zero)."""
    nan, zero = {k: v.copy() for k, v in batch.items()}, {k: v.copy() for k, v in batch.items()}
    for name, a in nan.items():
        if name == "status":
            a[rows] = 2
            zero[name][rows] = 2
        elif a.dtype == F:
            a[rows] = np.nan
            zero[name][rows] = 0
        elif name == "choice_indices":
            a[rows] = -(1 << 40)
            zero[name][rows] = 315
        elif name == "k":
            a[rows] = 255
            zero[name][rows] = 0
    return nan, zero


_HOST = {}


def host_rows():
    """The rows the CPU tests run on, from the host restatement train_ref.Corpus: every frame of the six records with targets of the
    train-frames test world (its records 32 .. 37: games 0, 3, 7, 12, 20, 31 of its generator) and two picks out of range.  -> batch dict."""
    if "rows" not in _HOST:
        import oracle_lib as O
        import replay_oracle as R
        import train_ref as T
        from test_gpu_train_frames import _with_targets
        b, _, _, _ = O.make_random_ou_batch(32, seed0=0x5EED0000)
        recs = [_with_targets(R.play_random_game(b[i], seed=i), 100 + i) for i in (0, 3, 7, 12, 20, 31)]
        tref = T.Corpus(recs)
        picks = [(r, f) for r in range(len(recs)) for f in range(tref.frames(r))] + [(0, 60000), (99, 0)]
        _HOST["rows"] = tref.expected(np.array(picks, dtype=np.uint32))
    return _HOST["rows"]


def make_batch(real, seed=11):
    """The batch of the tests from the real rows (the last two not OK): the four built edge rows, a row that is not OK, the other built
    rows, then the real ones in a seeded order -- so that every prefix of 13 rows and more holds every edge."""
    syn = synthetic_rows()
    n_real = len(real["status"])
    assert (real["status"][-2:] != 0).all() and (real["status"][:-2] == 0).all()
    both = concat([syn, real])
    rest = np.concatenate([12 + np.arange(n_real - 2), [12 + n_real - 1]])
    rest = rest[np.random.default_rng(seed).permutation(len(rest))]
    order = np.concatenate([[0, 1, 2, 3, 12 + n_real - 2], np.arange(4, 12), rest])
    return take(both, order)


# ---- the symmetries (oakgpu_frames_symmetries_dev restated) ----------------------------------------------------------------------------
SIDE_FIELDS = ("pokemon", "active", "hp", "choice_indices", "k", "empirical_policies", "nash_policies")
VALUE_FIELDS = ("empirical_value", "nash_value", "score")


def symmetry_draws(seed, i):
    """Row i's (flip, source slot of every slot [6]) from fast_prng seeded seed + i: the lowest bit of the first uniform_64, then the
    Fisher-Yates permutation of the bench slots from four more (q = 4 .. 1: slot q <-> slot draw % (q + 1))."""
    import oracle_lib as O
    state = np.zeros(8, np.uint8)
    O.LIB.oracle_fast_prng_seed(O.ptr(state), (seed + i) & (2 ** 64 - 1))
    draws = [int(O.LIB.oracle_fast_prng_uniform_64(O.ptr(state))) & (2 ** 64 - 1) for _ in range(5)]
    src = list(range(6))
    for q in (4, 3, 2, 1):
        j = draws[5 - q] % (q + 1)
        src[1 + q], src[1 + j] = src[1 + j], src[1 + q]
    return draws[0] & 1, src


def symmetric(batch, n, seed, flip_sides=True, permute_bench=True, forced=None):
    """The first n rows of a batch after the symmetries, as a new batch dict.  forced: (flip, src) for every row in place of the draws."""
    out = {name: np.array(a[:n]) for name, a in batch.items()}
    for i in range(n):
        if batch["status"][i] != 0:
            continue
        flip, src = forced if forced is not None else symmetry_draws(seed, i)
        flip, src = (flip if flip_sides else 0), (src if permute_bench else list(range(6)))
        sides = [1, 0] if flip else [0, 1]
        for name in ("pokemon", "hp"):
            out[name][i] = batch[name][i][sides][:, src]
        if flip:
            for name in SIDE_FIELDS[1:]:
                if name != "hp":
                    out[name][i] = batch[name][i][sides]
            for name in VALUE_FIELDS:
                out[name][i] = F(1.0) - batch[name][i]
    return out
