"""Test helper for the policy heads (tests/test_policy_ref.py on the CPU, tests/test_gpu_policy.py on the GPU): a batched float64
evaluation of both heads from a given fp32 embedding, a vectorised Encode::Battle::Policy::get_index, the yardstick the kernels
are held to, the mid-game states the choice forms are counted over, and small .battle.net rewriters.  numpy only."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nn_oracle as NN  # noqa: E402
import oracle_lib as O  # noqa: E402

F = np.float32
GOLDEN = {tag: os.path.join(ROOT, "tests", "golden", "net_%s.battle.net" % tag) for tag in ("default", "tiny", "256")}
# (turn-steps, seed0) of the six groups of form_states, in this order
STEP_SEEDS = ((0, 1000), (5, 2000), (12, 3000), (30, 4000), (60, 5000), (120, 6000))
FORMS = ("pass_only", "forced_move_0", "switches_only", "moves_only", "nine_choices",
         "switch_to_2", "switch_to_3", "switch_to_4", "switch_to_5", "switch_to_6", "order_changed")
MIN_PER_FORM = 20

_STATES = {}


def result_bytes(b):
    return np.array([O.LIB.oracle_result_from_state(O.ptr(b[i])) for i in range(b.shape[0])], dtype=np.uint8)


def form_states(per=2048):
    """Random OU battles advanced 0, 5, 12, 30, 60 and 120 random turn-steps on the oracle, `per` of each (seed0 = 1000 ... 6000),
    finished battles dropped: (battles, durations, results).  The generator is deterministic."""
    if per not in _STATES:
        bs, ds = [], []
        for steps, seed0 in STEP_SEEDS:
            b, d, p, r = O.make_random_ou_batch(per, seed0=seed0)
            O.rollout_batch(b, d, r, p, max_steps=steps, threads=8)
            bs.append(b)
            ds.append(d)
        b, d = np.concatenate(bs), np.concatenate(ds)
        r = result_bytes(b)
        keep = (r & 15) == 0
        _STATES[per] = (np.ascontiguousarray(b[keep]), np.ascontiguousarray(d[keep]), np.ascontiguousarray(r[keep]))
    return _STATES[per]


def batch_of(n, seed=1):
    """n leaves drawn from form_states(): a seeded permutation of them, repeated when n is larger (every step count in any prefix)."""
    b, d, r = form_states()
    idx = np.random.default_rng(seed).permutation(b.shape[0])[np.arange(n) % b.shape[0]]
    return np.ascontiguousarray(b[idx]), np.ascontiguousarray(d[idx]), np.ascontiguousarray(r[idx])


def oracle_choices(b, r, player):
    """The oracle's legal choices of one player, in the layout of Context.choices: (choices uint8[n, 9], counts uint8[n])."""
    n = b.shape[0]
    out, cnt = np.zeros((n, 9), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        c = O.choices(b[i], player, (int(r[i]) >> (4 + 2 * player)) & 3)
        cnt[i] = len(c)
        out[i, :len(c)] = c
    return out, cnt


def policy_rows(battles, choices, counts, head=0):
    """Encode::Battle::Policy::get_index (encode/battle/policy.h:29-58) for a whole batch: the fc3 row of every live entry of
    `choices` (n x 9, `counts` of them live) of side `head`, -1 at and past the count.  Restates nn_oracle.policy_index."""
    side = np.asarray(battles)[:, 184 * head:184 * head + 184].astype(np.int64)
    c = np.asarray(choices).astype(np.int64)
    n = side.shape[0]
    lane = np.arange(n)[:, None]
    kind, data = c & 3, c >> 2
    live = np.arange(9)[None, :] < np.asarray(counts).astype(np.int64)[:, None]
    is_move, is_switch = live & (kind == 1) & (data > 0), live & (kind == 2)
    # move: side.stored().moves[data - 1].id - 1 (0 for an empty slot)
    sid = side[:, 176][:, None] - 1
    mid = side[lane, np.where(is_move, 24 * sid + 10 + 2 * (data - 1), 0)]
    move_row = np.where(mid == 0, 0, mid - 1)
    # switch: 164 + species of the Pokemon at order[data - 1] - 1
    pid = side[lane, np.where(is_switch, 176 + data - 1, 176)]
    species = side[lane, np.where(is_switch, 24 * (pid - 1) + 21, 0)]
    rows = np.where(is_move, move_row, np.where(is_switch, 164 + species - 1, 0))
    return np.where(live, rows, -1)


def choice_forms(battles, choices, counts, head):
    """How many leaves show each of FORMS for side `head` (the shapes k_policy_rows' row gather and k_policy_i8's lanes branch on)."""
    c = np.asarray(choices).astype(np.int64)
    cnt = np.asarray(counts).astype(np.int64)
    live = np.arange(9)[None, :] < cnt[:, None]
    kind = c & 3
    out = {
        "pass_only": (cnt == 1) & (c[:, 0] == 0),
        "forced_move_0": (cnt == 1) & (c[:, 0] == 1),
        "switches_only": (cnt >= 1) & ((live & (kind != 2)).sum(axis=1) == 0),
        "moves_only": (cnt >= 1) & ((live & ((kind != 1) | (c >> 2 == 0))).sum(axis=1) == 0),
        "nine_choices": cnt == 9,
        "order_changed": (np.asarray(battles)[:, 184 * head + 176:184 * head + 182] != np.arange(1, 7, dtype=np.uint8)[None, :]).any(axis=1),
    }
    for slot in range(2, 7):
        out["switch_to_%d" % slot] = (live & (c == ((slot << 2) | 2))).any(axis=1)
    return {k: int(out[k].sum()) for k in FORMS}


def trunc16(x):
    """fp32 values cut to their 16 most significant bits (the h + m of a bf16 triple by truncation: what is left when the l part is lost)."""
    return (np.ascontiguousarray(x, dtype=F).view(np.uint32) & np.uint32(0xFFFFFF00)).view(F)


def logits_f64(onet, emb, fc2_operand=None):
    """Both heads' 315 logits in float64 from fp32 embeddings (n x in_dim): fc0, fc1 and each head's fc2 / fc3 with the weights as
    stored and the activation of the file header -- what test_gpu_leafnet._main_value_f64 is to the value.  fc2_operand (the
    discrimination check): applied to fc2's weights and to its fp32 input row in place of the identity."""
    act = (lambda x: np.maximum(x, 0.0)) if onet.activation == 1 else (lambda x: np.clip(x, 0.0, 1.0))
    h = np.asarray(emb, dtype=np.float64)
    for layer in (onet.fc0, onet.fc1):
        h = act(h @ layer.W.astype(np.float64).T + layer.b.astype(np.float64))
    out = []
    for fc2, fc3 in ((onet.q1a, onet.q1b), (onet.q2a, onet.q2b)):
        W2, x = fc2.W, h
        if fc2_operand is not None:
            W2, x = fc2_operand(W2), fc2_operand(h.astype(F)).astype(np.float64)
        p = act(x @ W2.astype(np.float64).T + fc2.b.astype(np.float64))
        out.append(p @ fc3.W.astype(np.float64).T + fc3.b.astype(np.float64))
    return out[0], out[1]


def oracle_logits(onet, emb):
    """The fp32 numpy oracle's logits (nn_oracle.Net.policy_logits, row by row as the oracle computes them): (n x 315, n x 315)."""
    n = emb.shape[0]
    l1, l2 = np.zeros((n, 315), F), np.zeros((n, 315), F)
    for i in range(n):
        l1[i], l2[i] = onet.policy_logits(emb[i])
    return l1, l2


def gather(full, rows):
    """full[i, rows[i, j]] (n x 9), 0 where rows is -1."""
    return np.where(rows >= 0, np.take_along_axis(full, np.maximum(rows, 0), axis=1), 0)


def yardstick(ref_pairs, oracle_pairs, rows_pairs):
    """(E_ref, S, entries): the oracle's worst distance from float64 over the live entries of both heads, S = max(1, max |f64 logit|)
    over them, and how many there are.  *_pairs = (head 1, head 2)."""
    e_ref, s, cnt = 0.0, 1.0, 0
    for ref, orc, rows in zip(ref_pairs, oracle_pairs, rows_pairs):
        live = rows >= 0
        if not live.any():
            continue
        r = gather(ref, rows)[live]
        if orc is not None:
            e_ref = max(e_ref, float(np.abs(gather(orc.astype(np.float64), rows)[live] - r).max()))
        s = max(s, float(np.abs(r).max()))
        cnt += int(live.sum())
    return e_ref, s, cnt


def bound(e_ref, s):
    """max |kernel - float64| allowed: four times the fp32 oracle's own worst error plus 2e-7 of the logits' scale (the factor and
    the floor test_gpu_leafnet.py applies to the value, there with S = 1)."""
    return 4.0 * e_ref + 2e-7 * s


def worst_error(got_pairs, ref_pairs, rows_pairs):
    """max |got - float64| over the live entries of both heads."""
    w = 0.0
    for got, ref, rows in zip(got_pairs, ref_pairs, rows_pairs):
        live = rows >= 0
        if live.any():
            w = max(w, float(np.abs(got.astype(np.float64)[live] - gather(ref, rows)[live]).max()))
    return w


def rewrite_net(src, dst, edit=None, header0=None):
    """Copy a .battle.net with edit(layer, b, W) -> (b, W) applied to its 12 Affine blocks (pokemon_net 0-1, active_net 2-3, fc0 4,
    fc1 5, value_fc2 6, value_fc3 7, p1 fc2 8, p1 fc3 9, p2 fc2 10, p2 fc3 11) and, if given, header byte 0 set (1 = clamp)."""
    raw = open(src, "rb").read()
    out, off = [raw[:8] if header0 is None else bytes([header0]) + raw[1:8]], 8
    for i in range(12):
        n_in, n_out = struct.unpack_from("<II", raw, off)
        off += 8
        b = np.frombuffer(raw, "<f4", n_out, off).copy()
        off += 4 * n_out
        W = np.frombuffer(raw, "<f4", n_out * n_in, off).copy().reshape(n_out, n_in)
        off += 4 * n_out * n_in
        if edit is not None:
            b, W = edit(i, b, W)
        out += [struct.pack("<II", n_in, n_out), np.asarray(b, "<f4").tobytes(), np.asarray(W, "<f4").tobytes()]
    assert off == len(raw)
    open(dst, "wb").write(b"".join(out))
    return dst


def scale_heads(fc2_log2=0, fc3_log2=0, fc3_bias=False):
    """An edit for rewrite_net: both heads' fc2 (weights and bias) times 2^fc2_log2, fc3's weights (and its bias if asked) times
    2^fc3_log2.  Powers of two are exact in fp32; behind ReLU, fc2 x 2^-s with fc3 x 2^+s is the same function."""
    def edit(i, b, W):
        if i in (8, 10):
            return b * F(2.0 ** fc2_log2), W * F(2.0 ** fc2_log2)
        if i in (9, 11):
            return (b * F(2.0 ** fc3_log2) if fc3_bias else b), W * F(2.0 ** fc3_log2)
        return b, W
    return edit


def spread_main_net(i, b, W):
    """Main-net weights stretched over (-1.9, 1.9) (int8 -121..121) and biases over +-0.6, for the quantized network: every byte
    value of the weights occurs (as tests/test_gpu_discrete.py)."""
    if i < 4:
        return b, W
    return (b / np.abs(b).max() * F(0.6)).astype(F), (W / np.abs(W).max() * F(1.9)).astype(F)
