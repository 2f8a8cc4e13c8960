"""numpy restatement of the quantized ("discrete") battle network (nn/battle/quantized/{affine,clipped_relu,main-net}.h,
nn/battle/cache.h, network.h:131-175): the test oracle of oakgpu_net_load_discrete* and k_mainnet_i8.

Integer arithmetic is int64 here (every int32 of the reference fits); the fp32 steps (quantization, the byte cast, the division by
8128 and the sigmoid) are float32 operations in the reference's order.  Embeddings come from oracle/nn_oracle.py as it stands,
through copies of its Net whose .activation is set per pass: party slots with ReLU, actives with clamp."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nn_oracle as NN  # noqa: E402

F = np.float32
CONV = F(127 * 64)  # main-net.h: 127 * (1 << 6)


class NotClamped(ValueError):
    pass


def quantize_weights(W):
    """int8 = trunc(w * 64) (affine.h:89-90); refused unless strictly inside (-2, 2), NaN included."""
    W = np.asarray(W, dtype=F)
    ok = (W < F(2)) & (W > F(-2))
    if not ok.all():
        i = int(np.flatnonzero(~ok.ravel())[0])
        raise NotClamped("%dnon clamped%f" % (i, float(W.ravel()[i])))
    return np.trunc(W * F(64)).astype(np.int64)


def quantize_biases(b):
    """int32 = trunc((b * 64) * 127) (affine.h:86-87), two fp32 operations."""
    x = (np.asarray(b, dtype=F) * F(64)) * F(127)
    if not ((x >= F(-2147483648.0)) & (x < F(2147483648.0))).all():
        raise ValueError("bias outside int32")
    return np.trunc(x).astype(np.int64)


def cast_u8(f):
    """static_cast<uint8_t>(127 * f) as g++ -O3 -mavx2 compiles the reference's std::transform (vcvttps2dq, low byte):
    the int32 truncation's low 8 bits, 0 for values outside int32 (and NaN)."""
    v = F(127) * np.asarray(f, dtype=F)
    inside = (v >= F(-2147483648.0)) & (v < F(2147483648.0))
    i = np.where(inside, np.trunc(np.where(inside, v, F(0))), F(-2147483648.0)).astype(np.int64)
    return (i & 0xFF).astype(np.uint8)


def affine(W, b, x, stats=None):
    """AffineTransform::propagate (affine.h:102-144) for a batch x [n, in] of bytes: pairs (2k, 2k+1) through
    _mm256_maddubs_epi16 -- u[2k] w[2k] + u[2k+1] w[2k+1] saturated to int16 (simd.h:31-38) -- summed in int32, plus the bias.
    stats (dict, optional) counts the pairs that saturated under 'saturated'."""
    x = np.asarray(x, dtype=np.int64)
    out = np.empty((x.shape[0], W.shape[0]), dtype=np.int64)
    sat = 0
    step = max(1, (1 << 22) // max(1, W.size))
    for s in range(0, x.shape[0], step):
        xs = x[s:s + step]
        p = xs[:, None, 0::2] * W[None, :, 0::2] + xs[:, None, 1::2] * W[None, :, 1::2]
        c = np.clip(p, -32768, 32767)
        sat += int((c != p).sum())
        out[s:s + step] = c.sum(axis=2) + b[None, :]
    if stats is not None:
        stats["saturated"] = stats.get("saturated", 0) + sat
    return out


def crelu(x):
    """ClippedReLU (clipped_relu.h:54-98): clamp(x >> 6, 0, 127), arithmetic shift."""
    return np.clip(np.asarray(x, dtype=np.int64) >> 6, 0, 127)


def expf(x):
    """glibc's expf (the reference's std::exp of a float): the double exponential rounded to float."""
    return np.exp(np.asarray(x, dtype=F).astype(np.float64)).astype(F)


def sigmoid(x):
    """1 / (1 + expf(-x)) in fp32 (network.h value_inference)."""
    x = np.asarray(x, dtype=F)
    return (F(1) / (F(1) + expf(-x))).astype(F)


class QuantNet:
    """The quantized network of a clamp-header `.battle.net` (search.cc:100-147)."""

    def __init__(self, path):
        net = NN.Net(path)
        if net.activation != 2:
            raise ValueError("Agent: .discrete was specified but the parsed header does not encode clamped activations.")
        self.relu = copy.copy(net)
        self.relu.activation = 1
        self.clamp = copy.copy(net)
        self.clamp.activation = 2
        self.net = net
        self.H, self.VH, self.PH = net.fc0.out_dim, net.v2.out_dim, net.q1a.out_dim
        q = {}
        for name in ("fc0", "fc1", "v2", "v3", "q1a", "q2a", "q1b", "q2b"):
            layer = getattr(net, name)
            q[name] = (quantize_weights(layer.W), quantize_biases(layer.b))
        self.q = q

    def embedding(self, battle, durations):
        """fp32 battle embedding: party slots from the ReLU network, actives (and their hp) from the clamp network."""
        e = NN.battle_embedding(self.relu, battle, durations)
        a = NN.battle_embedding(self.clamp, battle, durations)
        side, aod = self.net.side_dim, self.net.aod
        for s in range(2):
            e[s * side:s * side + 1 + aod] = a[s * side:s * side + 1 + aod]
        return e

    def embedding_bytes(self, battle, durations):
        return cast_u8(self.embedding(battle, durations))

    def trunk(self, u, stats=None):
        """fc0 -> crelu -> fc1 -> crelu for a batch of embedding bytes [n, 768]: the fc1 bytes."""
        h = crelu(affine(*self.q["fc0"], u, stats))
        return crelu(affine(*self.q["fc1"], h))

    def value_acc(self, u, stats=None):
        h = self.trunk(u, stats)
        h = crelu(affine(*self.q["v2"], h))
        return affine(*self.q["v3"], h)[:, 0]

    def value(self, u, stats=None):
        return sigmoid(self.value_acc(u, stats).astype(F) / CONV)

    def policy_logits(self, u, battles, p1_choices, p1_counts, p2_choices, p2_counts):
        """value_policy_inference's logits: propagate_single(row) / 8128 for each legal choice's row (affine.h:173-184)."""
        h = self.trunk(u)
        out = []
        for head, (ch, cnt) in enumerate(((p1_choices, p1_counts), (p2_choices, p2_counts))):
            W2, b2 = self.q["q1a" if head == 0 else "q2a"]
            W3, b3 = self.q["q1b" if head == 0 else "q2b"]
            h2 = crelu(affine(W2, b2, h))
            lg = np.zeros((u.shape[0], 9), dtype=F)
            for i in range(u.shape[0]):
                side = battles[i][184 * head:184 * (head + 1)]
                for j in range(int(cnt[i])):
                    r = NN.policy_index(side, int(ch[i][j]))
                    lg[i, j] = F(int(W3[r] @ h2[i] + b3[r])) / CONV
            out.append(lg)
        return out
