"""Test helper for the main net's value path (tests/test_mainnet_ref.py on the CPU, tests/test_gpu_mainnet.py on the GPU): a batched
float64 evaluation of fc0, fc1, value_fc2, value_fc3 and the sigmoid from a given fp32 embedding, the fp32 oracle's values, the
bound the kernels are held to, and the table of networks that reach every template width, padded block count, ragged width and
ring parity of k_mainnet_pair / k_mainnet_split / k_mainnet_wave.  numpy only."""
import os

import numpy as np

import policy_ref as P
from policy_ref import NN

F = np.float32
LAYERS = ("fc0", "fc1", "v2")

# name -> (hidden, value_hidden, pokemon_out, active_out, activation (1 relu, 2 clamp), seed, log2 of value_fc3's scale); None = the
# default width of netfile.layer_dims.  The seed is the first one whose pre-sigmoid sums over the first leaves of batch_of(700, SEED)
# have both signs (a random value_fc3 behind non-negative activations mostly gives one sign only), the scale the smallest power of
# two that then stretches them over [-8, 8] on the first 128 leaves, a factor two to spare -- tests/test_mainnet_ref.py asserts the span.
RANDOM_NETS = {
    "h32_k60": (32, 32, 1, 19, 2, 5, 9),
    "h33_v1_k320": (33, 1, 27, 19, 1, 316, 13),
    "h100_v40_k320": (100, 40, 27, 19, 2, 13, 13),
    "h96_v160_k536": (96, 160, 33, 97, 1, 16, 11),
    "h200_v72_k536": (200, 72, 33, 97, 2, 33, 12),
    "h255_v255": (255, 255, None, None, 1, 30, 13),
    "h64_v64_k1256": (64, 64, 99, 127, 1, 123, 11),
    "h128_v128": (128, 128, None, None, 2, 22, 12),
}
GOLDEN_NETS = ("256", "default", "tiny")
ODD_PAIR_PHASES = ("h33_v1_k320", "h100_v40_k320", "h96_v160_k536", "h200_v72_k536")
SEED = 5               # batch_of's seed for every leaf batch of the two test files
SIGMOID_SEED = 1        # ... of the sigmoid test: the first seed whose 700 leaves hold y < -90 on SIGMOID_NET
SIGMOID_NET = "256_v3_x1024"   # net_256 with value_fc3 (weights and bias) times 2^10: |y| beyond where expf overflows


def up32(x):
    return (x + 31) // 32 * 32


def shape_of(k, hidden, value_hidden):
    """What oakgpu_net_load derives from the dims: the padded widths, the block count of the split / pair kernels (3 blocks run as
    4, 5 to 7 as 8), fc0's 64-column chunks and the phases one 128-row group takes from k_mainnet_pair's weight ring."""
    H, VH = up32(hidden), up32(value_hidden)
    nbr = max(H, VH) // 32
    NB = 8 if nbr > 4 else 4 if nbr > 2 else nbr
    chunks = (k + 63) // 64
    T0, G = 4 * chunks, 4 if NB >= 2 else 2
    return dict(K=k, hidden=hidden, value_hidden=value_hidden, H=H, VH=VH, NB=NB, chunks=chunks, T0=T0, pair_phases=(T0 + 4 * NB) // G,
                split_phases=(T0 + 4 * NB) // 2)


def _random_dims(name):
    h, vh, po, ao = RANDOM_NETS[name][:4]
    dims = dict(hidden=h, value_hidden=vh)
    if po is not None:
        dims.update(pokemon_out=po, active_out=ao)
    return dims


def _table():
    from oak_amd import netfile
    out = {}
    for name in RANDOM_NETS:
        dims = _random_dims(name)
        out[name] = shape_of(netfile.layer_dims(**dims)[4][0], dims["hidden"], dims["value_hidden"])
    for tag in GOLDEN_NETS:
        o = NN.Net(P.GOLDEN[tag])
        out[tag] = shape_of(o.fc0.in_dim, o.fc0.out_dim, o.v2.out_dim)
    return out


NETS = _table()
ALL_NETS = tuple(sorted(RANDOM_NETS)) + GOLDEN_NETS


def scale_value_fc3(log2):
    """An edit for policy_ref.rewrite_net: value_fc3's weights and bias times 2^log2 (exact in fp32)."""
    def edit(i, b, W):
        return (b * F(2.0 ** log2), W * F(2.0 ** log2)) if i == 7 else (b, W)
    return edit


def write_net(name, directory, log2=None, seed=None):
    """The .battle.net of a net of the table: the golden files as they are, SIGMOID_NET rewritten from net_256, the random ones
    written by netfile.write_random_net and their value_fc3 scaled by 2^k (log2 / seed: in place of the table's, for choosing them)."""
    from oak_amd import netfile
    directory = str(directory)
    if name in P.GOLDEN:
        return P.GOLDEN[name]
    if name == SIGMOID_NET:
        return P.rewrite_net(P.GOLDEN["256"], os.path.join(directory, name + ".battle.net"), scale_value_fc3(10))
    act, s, k = RANDOM_NETS[name][4:]
    src = os.path.join(directory, name + ".src.battle.net")
    netfile.write_random_net(src, seed=s if seed is None else seed, activation=act, **_random_dims(name))
    return P.rewrite_net(src, os.path.join(directory, name + ".battle.net"), scale_value_fc3(k if log2 is None else log2))


def value_f64(onet, emb, operand=None):
    """(value, y) in float64 from fp32 embeddings [n, K]: fc0, fc1, value_fc2 with the weights as stored and the activation of the
    file header, y = value_fc3's sum, value = 1 / (1 + exp(-y)) -- test_gpu_leafnet._main_value_f64 for a whole batch.
    operand = (layer of LAYERS, fn) (the discrimination check): fn applied to that layer's weights and to its fp32 input."""
    act = (lambda x: np.maximum(x, 0.0)) if onet.activation == 1 else (lambda x: np.clip(x, 0.0, 1.0))
    h = np.asarray(emb, dtype=np.float64)
    for name in LAYERS:
        layer = getattr(onet, name)
        W, x = layer.W, h
        if operand is not None and operand[0] == name:
            W, x = operand[1](W), operand[1](h.astype(F)).astype(np.float64)
        h = act(x @ W.astype(np.float64).T + layer.b.astype(np.float64))
    y = h @ onet.v3.W.astype(np.float64)[0] + np.float64(onet.v3.b[0])
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-y)), y


def oracle_values(onet, emb):
    """nn_oracle.Net.main_value row by row, as the fp32 oracle computes it."""
    with np.errstate(over="ignore"):
        return np.array([onet.main_value(emb[i]) for i in range(emb.shape[0])], dtype=F)


def hold(values, onet, emb, oracle_rows=None):
    """(worst, E_ref, bound): max |values - float64| over every row, the fp32 oracle's worst distance from float64 on the first
    `oracle_rows` rows (a maximum over fewer rows is no larger, so the bound only tightens), and policy_ref.bound(E_ref, 1) =
    4 E_ref + 2e-7, the bound test_gpu_leafnet.py applies to the value."""
    ref = value_f64(onet, emb)[0]
    k = emb.shape[0] if oracle_rows is None else min(emb.shape[0], oracle_rows)
    e_ref = float(np.abs(oracle_values(onet, emb[:k]).astype(np.float64) - ref[:k]).max())
    return float(np.abs(np.asarray(values).astype(np.float64) - ref).max()), e_ref, P.bound(e_ref, 1.0)


def trunc(bits):
    """fp32 values cut to their `bits` most significant bits (policy_ref.trunc16 at 16)."""
    if bits == 16:
        return P.trunc16
    mask = np.uint32(0xFFFFFFFF ^ ((1 << (24 - bits)) - 1))
    return lambda x: (np.ascontiguousarray(x, dtype=F).view(np.uint32) & mask).view(F)


def oracle_embeddings(onet, b, d):
    return np.stack([NN.battle_embedding(onet, b[i], d[i]) for i in range(b.shape[0])])
