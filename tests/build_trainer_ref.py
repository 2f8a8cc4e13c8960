"""A torch CPU referee of the build trainer (oak_amd/csrc/buildtrain.hip), written from the contract in include/oakgpu.h, "Training the build
network": the three-layer nets of a `.build.net`, and build.py's process_targets / compute_loss_from_targets transcribed statement for
statement -- get_state on dense states, the dense 3,749-wide products, gather, exp + normalize, the GAE loop, autograd.  It runs in float64
as the referee and in float32 to size the bounds (trainer_ref.gradient_bound: the project's own bound).  `mistake` plants one deliberate
error by name; tests/test_build_trainer_ref.py shows that each lands outside the bound."""
import struct

import numpy as np
import torch

import build_traj_ref as T
from trainer_ref import gradient_bound  # noqa: F401  (the tests take it from here)

N_DIM, MAX_ACTIONS, STEPS = T.N_DIM, T.MAX_ACTIONS, T.STEPS
NAMES = tuple("%s.fc%d.%s" % (net, k, part) for net in ("policy", "value") for k in (1, 2, 3) for part in ("bias", "weight"))
HYPER = dict(gamma=0.99, lam=0.95, policy_loss_weight=1.0, value_loss_weight=0.5, entropy_loss_weight=0.01)
MISTAKES = ("gae_detached", "mean_over_k", "gamma_for_gamma_lam", "entropy_sign", "force_clip_dropped", "max_subtracted", "state_includes_action")


def make_net(seed, h, v1, v2, shift=0.0):
    """The bytes of a seeded `.build.net` whose activations, logits and gradients are of order 1: the policy's last bias lies in one of the
    bands [-4, -2.6], [-1.2, 1.2], [2.6, 4] (+ shift) and its last weights are small, so the taken action's logit falls on both sides of
    the force's thresholds and not next to them."""
    rng = np.random.default_rng(seed)
    u = lambda shape, k: (rng.random(shape) * 2 * k - k).astype(np.float32)
    out = b""
    for net, (a, b) in (("policy", (h, h)), ("value", (v1, v2))):
        last = N_DIM if net == "policy" else 1
        layers = [(N_DIM, a, 0.3, 0.3), (a, b, 1.5 / np.sqrt(a), 0.3), (b, last, (0.5 if net == "policy" else 1.5) / np.sqrt(b), 0.3)]
        for k, (i, o, kw, kb) in enumerate(layers):
            bias = u(o, kb)
            if net == "policy" and k == 2:
                band = rng.integers(3, size=o)
                bias = np.where(band == 1, u(o, 1.2), np.sign(band - 1.0) * (3.3 + u(o, 0.7))).astype(np.float32) + np.float32(shift)
            out += struct.pack("<II", i, o) + bias.astype("<f4").tobytes() + u((o, i), kw).astype("<f4").tobytes()
    return out


def read_net(data):
    """`.build.net` bytes -> [(bias, weight [out, in])] x 6, float32."""
    buf, pos, out = bytes(data), 0, []
    for _ in range(6):
        i, o = struct.unpack_from("<II", buf, pos)
        b = np.frombuffer(buf, "<f4", o, pos + 8)
        w = np.frombuffer(buf, "<f4", o * i, pos + 8 + 4 * o).reshape(o, i)
        out.append((b.copy(), w.copy()))
        pos += 8 + 4 * o * (i + 1)
    assert pos == len(buf)
    return out


def net_bytes(layers):
    return b"".join(struct.pack("<II", w.shape[1], w.shape[0]) + np.asarray(b, "<f4").tobytes() + np.asarray(w, "<f4").tobytes() for b, w in layers)


def chunk(records, value_weight=0.7):
    """records uint8[n, 128] -> (traj, targets) as numpy, by the referee of the reader."""
    traj = T.decode_many(records, no_score=True)
    return traj, T.targets(traj, value_weight)


def test_records():
    """The 257 records of the tests, computed once: the longest sound record 24 times over and 40 more three times each (their cells'
    segments in the inverted indices grow past two pieces), 106 once each (cells with one entry), the seven malformed records in between."""
    rolled = T.rollout_records(147, 29)
    spans = [T.bounds(*T.fields(r)[3:5]) for r in rolled]
    longest = int(np.argmax([end - start for start, end, _, _ in spans]))
    bad = [r for _, _, r in T.malformed_records()]
    good = [rolled[longest]] * 24 + [rolled[i % 40] for i in range(120)] + [rolled[i] for i in range(40, 147) if i != longest][:106]
    order = np.random.default_rng(5).permutation(len(good))
    out, k = [], 0
    for i, g in enumerate(order):
        out.append(good[g])
        if i % 9 == 1 and k < len(bad):
            out.append(bad[k])
            k += 1
    return np.ascontiguousarray(np.stack(out)[:257])


def selected_rule(keep, v, remaining):
    """The rank rule of the contract on its own: (selected bool [V], k, n_cap)."""
    kept = np.ones(v, bool) if keep is None else np.asarray(keep, bool)
    k = int(kept.sum())
    n_cap = min(k, int(remaining))
    return kept & (np.cumsum(kept) - 1 < n_cap), k, n_cap


# ---- build.py, statement for statement ------------------------------------------------------------------------------------------------------
def get_state(actions, dtype, include_own=False):
    b, T_, _ = actions.shape
    state = torch.zeros((b, T_, N_DIM + 1), dtype=dtype)
    state = state.scatter(2, actions + 1, 1.0)
    state = torch.cumsum(state, dim=1).clamp_max(1.0)
    if include_own:                                   # (the planted mistake: the step's own action is in its state)
        return state[:, :, 1:]
    state = state[:, :-1, 1:]
    state = torch.concat([torch.zeros(state[:, :1].shape, dtype=dtype), state], dim=1)
    return state


def apply_force_with_threshold(decision_outputs, force, threshold, threshold_center):
    can_decrease = decision_outputs - threshold_center > -threshold
    can_increase = decision_outputs - threshold_center < threshold
    force_negative = torch.clamp(force, max=0.0)
    force_positive = torch.clamp(force, min=0.0)
    clipped_force = can_decrease * force_negative + can_increase * force_positive
    return decision_outputs * clipped_force.detach()


class Ref:
    def __init__(self, data, dtype=torch.float64, mistake=None):
        self.dtype, self.mistake = dtype, mistake
        self.params = [torch.tensor(x, dtype=dtype, requires_grad=True) for pair in read_net(data) for x in pair]
        self.loss, self.kept = None, {}

    def net(self, x, k):
        """Three Affine blocks (relu, relu, none); keeps every layer's input and pre-activation for the bound's S."""
        for q in range(3):
            b, w = self.params[6 * k + 2 * q], self.params[6 * k + 2 * q + 1]
            z = x @ w.T + b
            z.retain_grad()
            self.kept[NAMES[6 * k + 2 * q]] = (x, z)
            x = torch.relu(z) if q < 2 else z
        return x

    def run(self, traj, tg, keep=None, total=None, remaining=None, hyper=HYPER):
        """process_targets + the sampling mask + compute_loss_from_targets on one chunk.  -> the forward outputs of every valid row
        (float64 numpy; logits NaN beyond n_legal) with "loss" (None when nothing is kept: the reference's `continue`)."""
        dt, hp = self.dtype, hyper
        action = torch.from_numpy(np.asarray(traj["action"], np.int64)).unsqueeze(-1)            # [b, T, 1]
        policy = torch.from_numpy(np.asarray(traj["policy"], np.float32)).to(dt).unsqueeze(-1)
        mask = torch.from_numpy(np.asarray(traj["mask"]).astype(np.int64))
        b, T_, _ = mask.shape
        valid_actions = action != -1
        valid_choices = policy > 0
        valid = torch.logical_and(valid_actions, valid_choices).squeeze(-1)
        state = get_state(action, dt, self.mistake == "state_includes_action")
        valid_state = state[valid]
        logits_full, v = self.net(valid_state, 0), self.net(valid_state, 1)
        value = torch.sigmoid(v)
        value.retain_grad()
        valid_mask = mask[valid]
        mask_logits = torch.where(valid_mask >= 0, torch.gather(logits_full, 1, torch.clamp(valid_mask, min=0)), -torch.inf)
        mask_logits.retain_grad()
        logits = mask_logits[:, 0]
        if self.mistake == "max_subtracted":
            mask_weights = torch.exp(mask_logits - mask_logits.max(dim=1, keepdim=True).values)
        else:
            mask_weights = torch.exp(mask_logits)
        mask_probs = torch.nn.functional.normalize(mask_weights, dim=1, p=1)
        valid_logp = torch.log(mask_probs[:, 0]).unsqueeze(-1)
        rewards = torch.from_numpy(np.asarray(tg["rewards"], np.float32)).to(dt).unsqueeze(-1)
        value_full = torch.zeros_like(policy)
        value_full[valid] = value
        next_value_full = torch.cat([value_full[:, 1:], torch.zeros_like(value_full[:, -1:])], dim=1)
        deltas = rewards + hp["gamma"] * next_value_full - value_full
        carry = hp["gamma"] if self.mistake == "gamma_for_gamma_lam" else hp["gamma"] * hp["lam"]
        advantages = []
        advantage = torch.zeros((b, 1), dtype=dt)
        for t in reversed(range(T_)):
            advantage = deltas[:, t, :] * valid[:, t].unsqueeze(-1) + carry * advantage
            advantages.insert(0, advantage)
        gae = torch.stack(advantages, dim=1)
        returns = (gae.detach() if self.mistake == "gae_detached" else gae) + value_full
        threshold_center = torch.zeros_like(logits)
        if self.mistake == "force_clip_dropped":
            forced = logits * gae[valid].squeeze(-1).detach()
        else:
            forced = apply_force_with_threshold(logits, gae[valid].squeeze(-1), 2, threshold_center)
        logp = torch.ones_like(policy)
        logp[valid] = valid_logp
        surr, rets, values, logps = (forced,) + tuple(x[valid] for x in (returns, value_full, logp))
        nv = int(valid.sum())
        total = nv if total is None else total
        remaining = total if remaining is None else remaining
        out = {"logits": torch.where(valid_mask >= 0, mask_logits, torch.nan).detach().double().numpy(), "value": value.detach().double().numpy().reshape(-1),
               "logp": valid_logp.detach().double().numpy().reshape(-1), "gae": gae[valid].detach().double().numpy().reshape(-1),
               "returns": rets.detach().double().numpy().reshape(-1), "forced": forced.detach().double().numpy().reshape(-1)}
        out["selected"], out["kept"], out["n_cap"] = selected_rule(keep, nv, remaining)
        self.tensors = {"value": value, "mask_logits": mask_logits, "valid": valid.numpy(), "valid_mask": valid_mask.numpy()}
        m = torch.ones(nv, dtype=torch.bool) if keep is None else torch.from_numpy(np.asarray(keep, bool))
        surr, rets, values, logps = surr[m], rets[m], values[m], logps[m]
        self.loss = None
        if surr.numel():
            k = surr.shape[0]
            n = min(k, remaining)
            mean = (lambda x: x[:n].sum() / k) if self.mistake == "mean_over_k" else (lambda x: x[:n].mean())
            policy_loss = -mean(surr)
            value_loss = mean((rets - values) ** 2)
            entropy = -mean((logps * logps.exp()).sum(dim=-1, keepdim=True))
            sign = 1.0 if self.mistake == "entropy_sign" else -1.0
            self.loss = (n / total) * (hp["policy_loss_weight"] * policy_loss + hp["value_loss_weight"] * value_loss + sign * hp["entropy_loss_weight"] * entropy)
            out.update(policy_loss=float(policy_loss.detach()), value_loss=float(value_loss.detach()), entropy=float(entropy.detach()))
        out["loss"] = None if self.loss is None else float(self.loss.detach())
        return out

    def backward(self):
        """-> (grads, S): {name: float64 array} over NAMES (weights [out, in]) and {name: S}: the largest over a tensor's entries of
        sum_rows |dZ| |X| (|X| = 1 for a bias) -- what one fp32 rounding of an entry's sum is measured in."""
        for p in self.params:
            p.grad = None
        if self.loss is None:
            return {n: np.zeros(tuple(p.shape)) for n, p in zip(NAMES, self.params)}, dict.fromkeys(NAMES, 0.0)
        self.loss.backward()
        grads = {n: (np.zeros(tuple(p.shape)) if p.grad is None else p.grad.detach().double().numpy().copy()) for n, p in zip(NAMES, self.params)}
        S = {}
        for k in range(6):
            x, z = self.kept[NAMES[2 * k]]
            dz = torch.zeros_like(z).double() if z.grad is None else z.grad.detach().double().abs()
            S[NAMES[2 * k]] = float(dz.sum(dim=0).max())
            S[NAMES[2 * k + 1]] = float((dz.T @ x.detach().double().abs()).max())
        return grads, S


def closed_form(out, tg, traj, sel, total, hyper=HYPER):
    """The contract's gradient in float64 from the referee's forward: (dL/dvalue [V], dL/dz [V, 339] with 0 beyond the list)."""
    hp = hyper
    valid, rows = tg["valid"], tg["rows"].astype(np.int64)
    n, c, gl = valid.shape[0], 1.0 / total, hp["gamma"] * hp["lam"]
    r = out["returns"] - out["value"]
    G = np.zeros((n, STEPS))
    G[rows[:, 0], rows[:, 1]] = sel * 2 * c * hp["value_loss_weight"] * r
    A = np.zeros((n, STEPS))
    for t in range(STEPS):
        A[:, t] = G[:, t] + (gl * A[:, t - 1] if t else 0.0)
    D = valid * A
    dvf = -D
    dvf[:, 1:] += hp["gamma"] * D[:, :-1]
    z = out["logits"]
    legal = ~np.isnan(z)
    w = np.where(legal, np.exp(np.where(legal, z, 0.0)), 0.0)
    q = w / np.maximum(w.sum(axis=1, keepdims=True), 1e-12)
    z0, gae = z[:, 0], out["gae"]
    cf = (z0 > -2) * np.minimum(gae, 0) + (z0 < 2) * np.maximum(gae, 0)
    first = np.zeros_like(q)
    first[:, 0] = 1.0
    dz = (sel * c)[:, None] * (-hp["policy_loss_weight"] * cf[:, None] * first + hp["entropy_loss_weight"] * (q[:, 0] * (1 + out["logp"]))[:, None] * (first - q))
    return dvf[rows[:, 0], rows[:, 1]], np.where(legal, dz, 0.0)


def forward_scale(data, out, traj, tg):
    """What one fp32 rounding of a forward output is measured in: for the logits the largest |b3_j| + sum_k |W3[j, k]| |h2_k| over the legal
    entries (computed in float64 from the net), for the other outputs the larger of 1 and their own magnitude."""
    layers = [(b.astype(np.float64), w.astype(np.float64)) for b, w in read_net(data)]
    state = np.zeros((len(tg["rows"]), N_DIM))
    for i in range(len(tg["rows"])):
        state[i, tg["state_cells"][i, :tg["state_n"][i]].astype(np.int64)] = 1.0
    h = np.maximum(state @ layers[0][1].T + layers[0][0], 0)
    h = np.maximum(h @ layers[1][1].T + layers[1][0], 0)
    full = np.abs(h) @ np.abs(layers[2][1]).T + np.abs(layers[2][0])
    rows = tg["rows"].astype(np.int64)
    lists = np.asarray(traj["mask"])[rows[:, 0], rows[:, 1]].astype(np.int64)
    scale = {"logits": float(np.where(lists >= 0, np.take_along_axis(full, np.maximum(lists, 0), axis=1), 0.0).max())}
    for name in ("value", "logp", "gae", "returns", "forced"):
        scale[name] = max(1.0, float(np.abs(out[name]).max()))
    return scale


# ---- oak_amd/csrc/build_loss.hpp on the host ------------------------------------------------------------------------------------------------
def loss_check_program(directory, flags=("-O2",)):
    """tests/cpp_build_loss_check.cc compiled into `directory`: -> the executable's path."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(str(directory), "cpp_build_loss_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + list(flags) + [os.path.join(here, "cpp_build_loss_check.cc"), "-o", exe], check=True)
    return exe


def loss_check(exe, directory, gamma, gamma_lam, value_full, rewards, valid, G, z0):
    """The header's recursions on [n, 31] arrays in a child process: -> (gae, returns, d_value_full, clipped_force) float32 [n, 31], by bits."""
    import os
    import subprocess
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    n = value_full.shape[0]
    path = os.path.join(str(directory), "loss_check.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<Iff", n, np.float32(gamma), np.float32(gamma_lam)))
        f.write(f32(value_full).tobytes() + f32(rewards).tobytes() + np.ascontiguousarray(valid, np.uint8).tobytes() + f32(G).tobytes() + f32(z0).tobytes())
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    words = np.array([[int(w, 16) for w in line.split()] for line in run.stdout.splitlines()], np.uint32).reshape(n, STEPS, 4)
    return tuple(np.ascontiguousarray(words[:, :, k]).view(np.float32) for k in range(4))
