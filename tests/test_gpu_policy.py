"""GPU: the policy heads of value_policy_inference -- k_policy_rows<PB, TRIPLE> (fp32 results: fc2 as bf16 triples or on fp32 MFMA)
and k_policy_i8 (the quantized network) -- held to what the value half of the leaf call is held to: a float64 evaluation of the
same embedding (tests/policy_ref.py) under the bound 4 E_ref + 2e-7 S, at every template width, main-net mode, batch size around
the tiles and the grid-stride sweeps, and choice form; the int8 heads bit for bit against tests/quant_oracle.py.

E_ref is the fp32 numpy oracle's own worst distance from float64 on the compared entries (never a kernel's), S = max(1, max |logit|).
tests/test_policy_ref.py shows on the CPU that an fc2 which lost its low bf16 part breaks this bound by a factor of 15 or more.

Measured on an MI355X (profiles/r07_policy_accuracy.json holds every figure): see the docstrings below."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import policy_ref as P
import quant_oracle as Q
from policy_ref import NN

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ("pair", "split", "fp32")
RECORDS = {}


@pytest.fixture(scope="module", autouse=True)
def _accuracy_records():
    """OAK_POLICY_ACCURACY_JSON=<file>: write what the tests of this module measured (the source of profiles/r07_policy_accuracy.json)."""
    yield
    out = os.environ.get("OAK_POLICY_ACCURACY_JSON")
    if out and RECORDS:
        with open(out, "w") as f:
            json.dump({"bound": "max|gpu - f64| <= 4 * E_ref + 2e-7 * S", "cases": RECORDS}, f, indent=1, sort_keys=True)


# ---- networks -------------------------------------------------------------------------------------------------------------------
# random nets: name -> (hidden, value_hidden, policy_hidden, activation); PB = k_policy_rows' block count (policy_hidden padded / 32)
RANDOM_NETS = {
    "ph24_h32_clamp": (32, 32, 24, 2),       # PB 1
    "ph24_h256_relu": (256, 64, 24, 1),      # PB 1
    "ph64_h96_relu": (96, 64, 64, 1),        # PB 2, fc3 rows in LDS
    "ph64_h128_clamp": (128, 128, 64, 2),    # PB 2
    "ph96_h128_clamp": (128, 64, 96, 2),     # PB 4, fc3 from global memory
    "ph96_h64_relu": (64, 32, 96, 1),        # PB 4
    "ph160_h256_relu": (256, 64, 160, 1),    # PB 8
    "ph160_h128_relu": (128, 64, 160, 1),    # PB 8
    "ph192_h64_clamp": (64, 64, 192, 2),     # PB 8
}


def net_path(tmp_path, name):
    if name in P.GOLDEN:
        return P.GOLDEN[name]
    if name == "256_fc3_x64":      # large logits: fc3 (weights and bias) of both heads times 2^6
        return P.rewrite_net(P.GOLDEN["256"], str(tmp_path / "fc3x64.battle.net"), P.scale_heads(0, 6, fc3_bias=True))
    if name == "default_int8":     # the quantized network of tests/test_gpu_discrete.py's default shape
        return P.rewrite_net(P.GOLDEN["default"], str(tmp_path / "default_clamp.battle.net"), P.spread_main_net, header0=1)
    h, vh, ph, act = RANDOM_NETS[name]
    src = str(tmp_path / (name + ".src.battle.net"))
    NN.write_random_net(src, hidden=h, value_hidden=vh, policy_hidden=ph, seed=23, activation=act)
    # fc3 (weights and bias) times 8: U(-1/sqrt(in), 1/sqrt(in)) heads give logits below 0.3, where the bound's floor 2e-7 max(1, .) would
    # be most of it (an fc2 cut to 16 bits: 3-6 bounds away); with logits of order 1, as trained heads have, it is 10 or more
    return P.rewrite_net(src, str(tmp_path / (name + ".battle.net")), P.scale_heads(0, 3, fc3_bias=True))


def gpu_choices(ctx, b, r):
    return [ctx.choices(b, r, pl) for pl in range(2)]


def policy_call(net, b, d, ch):
    return net.value_policy_inference(b, d, ch[0][0], ch[0][1], ch[1][0], ch[1][1])


def assert_zero_past_the_counts(logits, ch):
    for lg, (_, cnt) in zip(logits, ch):
        dead = np.arange(9)[None, :] >= cnt.astype(np.int64)[:, None]
        assert (lg.view(np.uint32)[dead] == 0).all()


def hold_to_float64(net, onet, b, d, ch, key, oracle_rows=None):
    """One policy call against policy_ref.logits_f64 of the call's own embedding; every live entry of both heads.  E_ref from the
    numpy oracle on the same rows (on the first `oracle_rows` of them if given: a maximum over fewer rows is no larger, so the bound
    only tightens).  Values bit-equal to the plain call's.  Records and returns (logits, worst error, bound)."""
    n = b.shape[0]
    vals, emb = net.value_inference(b, d, return_embedding=True)
    v2, l1, l2 = policy_call(net, b, d, ch)
    assert v2.shape == (n,) and l1.shape == (n, 9) and l2.shape == (n, 9)
    assert np.array_equal(v2, vals)
    assert_zero_past_the_counts((l1, l2), ch)
    rows = [P.policy_rows(b, c, cnt, head) for head, (c, cnt) in enumerate(ch)]
    with np.errstate(over="ignore"):
        ref = P.logits_f64(onet, emb)
    k = n if oracle_rows is None else min(n, oracle_rows)
    e_ref = P.yardstick([x[:k] for x in ref], P.oracle_logits(onet, emb[:k]), [x[:k] for x in rows])[0]
    _, s, cnt = P.yardstick(ref, (None, None), rows)
    worst, lim = P.worst_error((l1, l2), ref, rows), P.bound(e_ref, s)
    RECORDS["|".join(key)] = dict(E_ref=e_ref, worst=worst, S=s, bound=lim, logits=cnt, leaves=n)
    print("%s: worst %.3g, E_ref %.3g, S %.3g, bound %.3g over %d logits" % (" ".join(key), worst, e_ref, s, lim, cnt))
    assert np.isfinite(l1).all() and np.isfinite(l2).all()
    assert worst <= lim, (key, worst, e_ref, s, lim)
    return (l1, l2), worst, lim


# ---- 2. accuracy of every kernel form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "tiny", "256", "256_fc3_x64"] + sorted(RANDOM_NETS))
def test_every_kernel_form_against_float64(gpu_ctx, tmp_path, name):
    """The three golden nets, the 256-wide net with fc3 x 2^6 (logits up to ~60: the bound scales with S and nothing else changes)
    and random nets over PB = 1, 2, 4, 8 (fc3 in LDS and from global memory), both activations, hidden widths 32 ... 256, each in
    the main-net modes pair, split (TRIPLE heads behind two writers of the fc1 rows) and fp32 (fp32-MFMA heads): 700 mid-game leaves,
    max |gpu - f64| <= 4 E_ref + 2e-7 S.
    The random nets' fc3 is scaled by 8 (net_path) so that their logits, too, are of order 1.
    Measured (MI355X, profiles/r07_policy_accuracy.json): worst error 0.7e-7 ... 4.0e-7 x S against E_ref 0.5e-7 ... 1.6e-7 x S;
    every case (the compensated heads below included) uses between 16 % and 57 % of its bound (net_256: 1.96e-7 / 2.62e-7 /
    2.33e-7 for pair / split / fp32 against 6.33e-7; fc3 x 2^6, S = 42.4: 1.26e-5 / 1.68e-5 / 1.49e-5 against 3.62e-5).  With one of
    the six MFMAs of the TRIPLE branch removed (h . l) every net fails by a factor 4 to 16 (net_256: 4.9e-6) while the 2e-5 tests
    of test_gpu_leafnet.py and test_oakside_goldens.py still pass."""
    from oak_amd.engine import Network
    path = net_path(tmp_path, name)
    net, onet = Network(gpu_ctx, path=path), NN.Net(path)
    b, d, r = P.batch_of(700, seed=5)
    ch = gpu_choices(gpu_ctx, b, r)
    got = {}
    for mode in MODES:
        net.set_main_precision(mode)
        assert net.main_precision()[0] == mode
        assert net.policy_form() == ("fp32" if mode == "fp32" else "triple")
        got[mode], _, lim = hold_to_float64(net, onet, b, d, ch, (name, mode, "n700"))
    # the mode switch really switches the heads' fc2
    assert any((got["split"][h] != got["fp32"][h]).any() for h in range(2))
    net.close()


# name -> (fc2 x 2^a, fc3 x 2^b, fc2 of the heads beside a main net on pairs)
COMPENSATED = {
    "down20_up20": (-20, 20, "triple"),
    "down110_up110": (-110, 110, "fp32"),
    "down120_up120": (-120, 120, "fp32"),
    "up21_down21": (21, -21, "triple"),
    "up24_down24": (24, -24, "fp32"),
}


@pytest.mark.parametrize("case", sorted(COMPENSATED))
def test_compensated_heads(gpu_ctx, tmp_path, case):
    """fc2 (and its bias) of both heads of the 256-wide ReLU net times 2^a, fc3's weights times 2^-a: the same function (ReLU commutes
    with a positive scale; checked bit for bit on the fp32 oracle), each held to the float64 bound AND to the unscaled net's logits.
      * down20_up20: no weight above 2^20, the heads stay on the triples.
      * down110_up110, down120_up120: fc2's weights are ~2^-114 / ~2^-124, the low parts of their triples are bf16 subnormals or
        nothing, and fc3 (~2^108 / ~2^118) multiplies what they lose back up.  The loader used to look at fc2 alone, so such heads ran
        on the triples.  Measured with that loader: s = 110 still met the bound (worst 3.29e-7 against 5.74e-7: the bf16 pipe keeps
        subnormal parts, only those below 2^-133 are lost), s = 120 -- the scale the main net's own test runs
        (test_bf16_triple_main_net_at_the_edges_of_the_exponent_range) -- did not: 2.26e-4 against 6.09e-7.  The loader now counts
        fc3's weights too (what include/oakgpu.h says of the main net: "unless later layers multiply it back up"): both run on fp32
        MFMA (2.13e-7 and 2.04e-7 beside a main net on pairs), and down120_up120 is the regression test of that rule.
      * up21_down21: the largest fc2 weight of this net is 0.125 x 2^21 = 2^18, so 2^21 does NOT cross the loader's 2^20 -- the heads
        stay on the triples and must meet the bound there.
      * up24_down24: 0.125 x 2^24 is above 2^20: the heads run on fp32 MFMA while the main net stays on pairs."""
    from oak_amd.engine import Network
    a, c, form = COMPENSATED[case]
    path = P.rewrite_net(P.GOLDEN["256"], str(tmp_path / (case + ".battle.net")), P.scale_heads(a, c))
    net, onet, plain = Network(gpu_ctx, path=path), NN.Net(path), Network(gpu_ctx, path=P.GOLDEN["256"])
    big = max(float(np.abs(x.W).max()) for x in (onet.q1a, onet.q2a, onet.q1b, onet.q2b))
    assert (big > 2.0 ** 20) == (form == "fp32")              # the premise of the expected form
    b, d, r = P.batch_of(700, seed=6)
    ch = gpu_choices(gpu_ctx, b, r)
    assert net.main_precision() == ("pair", True)             # the heads' weights do not move the main net
    for mode in MODES:
        net.set_main_precision(mode)
        plain.set_main_precision(mode)
        assert net.main_precision()[0] == mode
        got, _, lim = hold_to_float64(net, onet, b, d, ch, ("256_" + case, mode, "n700"))
        assert net.policy_form() == ("fp32" if mode == "fp32" else form)
        _, p1, p2 = policy_call(plain, b, d, ch)
        assert max(np.abs(got[0] - p1).max(), np.abs(got[1] - p2).max()) <= 2 * lim
    net.close()
    plain.close()


# ---- 3. sizes -------------------------------------------------------------------------------------------------------------------
COMMON_SIZES = (1, 31, 32, 33, 255, 257, 16384)
FP32_SIZES = [("256", n) for n in COMMON_SIZES + (65535, 65536, 65569)] + [("ph160_h128_relu", n) for n in COMMON_SIZES + (32767, 32801, 65536)]
INT8_SIZES = (1, 3, 4, 5, 4095, 4097, 16384, 65536)


@pytest.mark.parametrize("name,n", FP32_SIZES)
def test_fp32_heads_at_every_size(gpu_ctx, tmp_path, name, n):
    """k_policy_rows around its 32-leaf wave tiles, across workgroups (every one stages fc3's rows into its own LDS) and into the
    second grid-stride sweep: above 65,536 leaves at PB <= 2 (8 waves x 256 workgroups x 32), above 32,768 at PB >= 4 (4 waves).
    EVERY row of every size under the float64 bound (E_ref from the oracle on the first 4,096 rows), values bit-equal to
    value_inference.  Measured: worst error 2.74e-7 (net_256) and 2.27e-7 (PB 8) over the 933,718 logits of 65,536 leaves against
    bounds of 6.93e-7 and 7.25e-7.  With the tile loop cut to its first sweep, 65,569 (PB 2) and 32,801 / 65,536 (PB 8) fail here and
    4,097 / 16,384 / 65,536 in test_int8_heads_at_every_size; every smaller size passes."""
    from oak_amd.engine import Network
    path = net_path(tmp_path, name)
    net, onet = Network(gpu_ctx, path=path), NN.Net(path)
    assert net.policy_form() == "triple"
    b, d, r = P.batch_of(n, seed=2)
    hold_to_float64(net, onet, b, d, gpu_choices(gpu_ctx, b, r), (name, "pair", "n%d" % n), oracle_rows=4096)
    net.close()


def raw_eval(ctx, net, b, d):
    """oakgpu_leaf_eval_discrete_raw_dev: the quantized network's embedding bytes [n, 768]."""
    from hipmem import Dev
    from oak_amd import _lib
    n = b.shape[0]
    gb, gd = Dev(b), Dev(d)
    qe, va = Dev(np.zeros((n, 768), np.uint8), fill=0xAB), Dev(np.zeros(n, np.int32), fill=0x7F)
    _lib.check(ctx.lib.oakgpu_leaf_eval_discrete_raw_dev(ctx.handle, net.handle, gb.p, gd.p, n, qe.p, va.p))
    ctx.synchronize()
    out = qe.host()
    for x in (gb, gd, qe, va):
        x.free()
    return out


def assert_int8_rows_exact(qn, qe, b, ch, logits, idx):
    e1, e2 = qn.policy_logits(qe[idx], b[idx], ch[0][0][idx], ch[0][1][idx], ch[1][0][idx], ch[1][1][idx])
    for got, exp in ((logits[0][idx], e1), (logits[1][idx], e2)):
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), np.argwhere(got != exp)[:4]


@pytest.mark.parametrize("n", INT8_SIZES)
def test_int8_heads_at_every_size(gpu_ctx, tmp_path, n):
    """k_policy_i8 (one wave per leaf, 4 leaves x 1,024 workgroups per sweep): around a workgroup, around one sweep, and 4 and 16
    sweeps.  Bit-equal to quant_oracle.QuantNet.policy_logits on the GPU's own embedding bytes -- every row up to 4,097 leaves;
    beyond, a seeded sample of 4,096 rows with the first and last 64, and every row equal to its copy in the first 4,096 (the batch
    repeats a 4,096-leaf batch)."""
    from oak_amd.engine import Network
    path = net_path(tmp_path, "default_int8")
    net, qn = Network(gpu_ctx, path=path, discrete=True), Q.QuantNet(path)
    assert net.policy_form() == "int8"
    b0, d0, r0 = P.batch_of(4096, seed=3)
    tile = np.arange(n) % 4096
    b, d, r = np.ascontiguousarray(b0[tile]), np.ascontiguousarray(d0[tile]), np.ascontiguousarray(r0[tile])
    ch = gpu_choices(gpu_ctx, b, r)
    vals, l1, l2 = policy_call(net, b, d, ch)
    assert np.array_equal(vals, net.value_inference(b, d))
    assert_zero_past_the_counts((l1, l2), ch)
    qe = raw_eval(gpu_ctx, net, b, d)
    if n <= 4097:
        idx = np.arange(n)
    else:
        ends = np.concatenate([np.arange(64), np.arange(n - 64, n)])
        rest = np.random.default_rng(n).choice(np.arange(64, n - 64), 4096 - 128, replace=False)
        idx = np.sort(np.concatenate([ends, rest]))
        for lg in (l1, l2):
            assert (lg.reshape(n // 4096, 4096, 9).view(np.uint32) == lg[:4096].view(np.uint32)[None]).all()
    assert_int8_rows_exact(qn, qe, b, ch, (l1, l2), idx)
    net.close()


KERNELS = ["256", "ph160_h128_relu", "default_int8"]        # k_policy_rows at PB 2 (fc3 in LDS) and PB 8, k_policy_i8


def _kernel_net(gpu_ctx, tmp_path, name):
    from oak_amd.engine import Network
    return Network(gpu_ctx, path=net_path(tmp_path, name), discrete=name.endswith("int8"))


@pytest.mark.parametrize("name", KERNELS)
def test_full_size_batch_properties_of_the_logits(gpu_ctx, tmp_path, name):
    """65,536 leaves, bit for bit: the call is repeatable; a permuted batch gives the permuted logits; a leaf evaluated alone (n = 1)
    gives its entry of the batch -- no logit depends on the batch around its leaf or on the lane, wave, tile, workgroup or sweep the
    leaf lands in."""
    net = _kernel_net(gpu_ctx, tmp_path, name)
    n = 65536
    b, d, r = P.batch_of(n, seed=11)
    ch = gpu_choices(gpu_ctx, b, r)
    v0, l1, l2 = policy_call(net, b, d, ch)
    assert np.isfinite(l1).all() and np.isfinite(l2).all() and (l1 != 0).any() and (l2 != 0).any()
    for got, want in zip(policy_call(net, b, d, ch), (v0, l1, l2)):
        assert np.array_equal(got, want)
    perm = np.random.default_rng(5).permutation(n)
    chp = [(c[perm], cnt[perm]) for c, cnt in ch]
    for got, want in zip(policy_call(net, b[perm], d[perm], chp), (v0, l1, l2)):
        assert np.array_equal(got, want[perm])
    for i in (0, 1, 31, 32, 4095, 4096, 32767, 32768, 40000, 65535):
        one = policy_call(net, b[i:i + 1], d[i:i + 1], [(c[i:i + 1], cnt[i:i + 1]) for c, cnt in ch])
        for got, want in zip(one, (v0, l1, l2)):
            assert np.array_equal(got[0], want[i]), i
    net.close()


@pytest.mark.parametrize("name", KERNELS)
def test_poisoned_output_buffers(gpu_ctx, tmp_path, name):
    """oakgpu_leaf_eval_policy_dev on logits buffers preset to 0x7F bytes, 1,003 leaves (not a multiple of a wave tile, nor of the
    int8 kernel's 4 leaves): every entry at and past its count is exactly 0.0f, the live ones are the host call's, and a guard band
    of 64 floats behind each buffer keeps the preset bytes."""
    from hipmem import Dev
    from oak_amd import _lib
    net = _kernel_net(gpu_ctx, tmp_path, name)
    n, guard = 1003, 64
    b, d, r = P.batch_of(n, seed=13)
    ch = gpu_choices(gpu_ctx, b, r)
    v0, l1, l2 = policy_call(net, b, d, ch)
    gb, gd, gv = Dev(b), Dev(d), Dev(np.zeros(n, F), fill=0x7F)
    gc = [(Dev(c), Dev(cnt)) for c, cnt in ch]
    gl = [Dev(np.zeros(n * 9 + guard, F), fill=0x7F) for _ in range(2)]
    _lib.check(gpu_ctx.lib.oakgpu_leaf_eval_policy_dev(gpu_ctx.handle, net.handle, gb.p, gd.p, n, gc[0][0].p, gc[0][1].p, gc[1][0].p, gc[1][1].p,
                                                       gv.p, gl[0].p, gl[1].p))
    gpu_ctx.synchronize()
    assert np.array_equal(gv.host(), v0)
    for buf, want, (_, cnt) in zip(gl, (l1, l2), ch):
        raw = buf.host()
        assert (raw[n * 9:].view(np.uint32) == 0x7F7F7F7F).all()
        got = raw[:n * 9].reshape(n, 9)
        dead = np.arange(9)[None, :] >= cnt.astype(np.int64)[:, None]
        assert dead.any() and (got.view(np.uint32)[dead] == 0).all()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for x in [gb, gd, gv] + gl + [y for pair in gc for y in pair]:
        x.free()
    net.close()


# ---- 4. choice forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["256", "default_int8"])
def test_every_choice_form(gpu_ctx, tmp_path, name):
    """6 x 2,048 battles after 0, 5, 12, 30, 60 and 120 turn-steps (finished ones dropped), the GPU's own legal choices: the batch must
    hold, for each head, at least 20 leaves of every form the row gather branches on -- pass only, a forced move with data 0, switches
    only, moves only, all nine choices, a switch to each of slots 2-6, an order other than 1..6 -- and at least 600 distinct (head, row)
    pairs; every logit under the float64 bound (k_policy_rows) / bit-equal to the quantized oracle (k_policy_i8)."""
    b, d, r = P.form_states()
    ch = gpu_choices(gpu_ctx, b, r)
    pairs = set()
    for head, (c, cnt) in enumerate(ch):
        forms = P.choice_forms(b, c, cnt, head)
        print("head %d: %s" % (head, forms))
        assert min(forms.values()) >= P.MIN_PER_FORM, (head, forms)
        rows = P.policy_rows(b, c, cnt, head)
        pairs |= {(head, int(x)) for x in np.unique(rows[rows >= 0])}
    assert len(pairs) >= 600, len(pairs)
    net = _kernel_net(gpu_ctx, tmp_path, name)
    if name.endswith("int8"):
        path = net_path(tmp_path, name)
        vals, l1, l2 = policy_call(net, b, d, ch)
        assert_zero_past_the_counts((l1, l2), ch)
        assert_int8_rows_exact(Q.QuantNet(path), raw_eval(gpu_ctx, net, b, d), b, ch, (l1, l2), np.arange(b.shape[0]))
    else:
        hold_to_float64(net, NN.Net(net_path(tmp_path, name)), b, d, ch, (name, "pair", "forms%d" % b.shape[0]))
    net.close()
