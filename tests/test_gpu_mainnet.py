"""GPU: the main net of the leaf call -- k_mainnet_pair<1|2|4|8> (fp32 values as scaled fp16 pairs, the default), k_mainnet_split<1|2|4|8>
(bf16 triples) and k_mainnet_wave (fp32 MFMA) -- held to what the policy heads and the embedding passes are held to: a float64
evaluation of the kernel's own embedding (tests/mainnet_ref.py) under the bound 4 E_ref + 2e-7, in all three modes, at every template
width, padded block count and ragged hidden width, at embedding dims from 60 to 1256, around the 32-row wave tiles and the 128-row
groups, into the second grid-stride sweep (where k_mainnet_pair's groups start on either ring buffer), over the whole range of the
sigmoid, and into poisoned output buffers.

E_ref is the fp32 numpy oracle's own worst distance from float64 on the compared rows (never a kernel's).  tests/test_mainnet_ref.py
shows on the CPU that a layer whose operands lost their low part (16 significant bits left) breaks this bound on every net and layer.
The random nets' value_fc3 is scaled so that the pre-sigmoid sums cover [-4, 4] and beyond; E_ref grows with it (the sums' fp32
rounding is relative), and so does what a lost part costs.

Measured on an MI355X (profiles/r11_mainnet_accuracy.json holds all 168 cases; here the batches of 31 rows or more): the golden
nets' worst error is 5.7e-8 ... 9.1e-8 against E_ref 6.4e-8 ... 7.8e-8, 12 % to 18 % of the bound; the random nets (|y| up to 30)
2.1e-6 ... 1.8e-5 against E_ref 2.5e-6 ... 1.1e-5, 21 % to 58 %; net_256 with value_fc3 x 2^10 2.0e-5 ... 2.7e-5 against 3.6e-5, at
most 76 %.  No case of any mode failed: the tests found no fault in the kernels or the loader.  What they would find was tried on two deliberately wrong builds:
  * "lost part" -- the l . h MFMA removed from k_mainnet_pair's and k_mainnet_split's k-step: 53 of the 59 tests fail (net_256 in pair
    mode 2.0e-5 against a bound of 4.9e-7, the random nets 1e-3 ... 9e-3 against 1e-5 ... 3e-5; each test stops at its first mode,
    pair); the repeat / permutation / single-leaf test and the poisoned buffers pass, as they should (the wrong values are still a
    pure function of the leaf);
  * "position" -- every group of k_mainnet_pair made to start on ring buffer 0: nothing changes for a net with an even phase count,
    so all of net_256 passes, and 11 second-sweep cases of the three odd nets fail (values up to 1.0 off) with
    test_value_is_a_pure_function_of_the_leaf[h33_v1_k320]; every case of at most 32,768 rows passes."""
import json
import os

import numpy as np
import pytest

import mainnet_ref as M
import policy_ref as P
from policy_ref import NN

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ("pair", "split", "fp32")
RECORDS = {}
_PATHS = {}
_SHARED = {}


@pytest.fixture(scope="module", autouse=True)
def _accuracy_records():
    """OAK_MAINNET_ACCURACY_JSON=<file>: write what the tests of this module measured (the source of profiles/r11_mainnet_accuracy.json)."""
    yield
    out = os.environ.get("OAK_MAINNET_ACCURACY_JSON")
    if out and RECORDS:
        with open(out, "w") as f:
            json.dump({"bound": "max|gpu - f64| <= 4 * E_ref + 2e-7", "cases": RECORDS}, f, indent=1, sort_keys=True)


def load(gpu_ctx, tmp_path_factory, name):
    """(Network, oracle net) of a net of mainnet_ref's table; the file is written once per process."""
    from oak_amd.engine import Network
    if name not in _PATHS:
        _PATHS[name] = M.write_net(name, tmp_path_factory.mktemp("mainnet"))
    net, onet = Network(gpu_ctx, path=_PATHS[name]), NN.Net(_PATHS[name])
    if name in M.NETS:
        t = M.NETS[name]
        assert net.shape()[:3] == (t["K"], t["hidden"], t["value_hidden"])
    assert net.main_precision() == ("pair", True), name       # a random U(-k, k) net is pair- and split-safe
    return net, onet


def switch(net, mode):
    net.set_main_precision(mode)
    assert net.main_precision()[0] == mode


def hold(net, onet, b, d, key, oracle_rows=None):
    """One value call in the mode in effect against mainnet_ref.value_f64 of the call's own embedding, every row; records and returns
    (values, embedding)."""
    vals, emb = net.value_inference(b, d, return_embedding=True)
    assert vals.shape == (b.shape[0],) and vals.dtype == F and np.isfinite(vals).all() and (vals >= 0).all() and (vals <= 1).all()
    worst, e_ref, lim = M.hold(vals, onet, emb, oracle_rows)
    RECORDS["|".join(key)] = dict(worst=worst, E_ref=e_ref, bound=lim, rows=int(b.shape[0]))
    print("%s: worst %.3g, E_ref %.3g, bound %.3g over %d rows" % (" ".join(key), worst, e_ref, lim, b.shape[0]))
    assert worst <= lim, (key, worst, e_ref, lim)
    return vals, emb


# ---- 1. every form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.ALL_NETS)
def test_every_form_against_float64(gpu_ctx, tmp_path_factory, name):
    """Holes 1, 2, 5 and 7: every net of the table (NB 1, 2, 4, 8; 5 and 7 blocks run as 8; hidden widths 33, 100, 200, 255 and value
    widths 1, 40, 72, 255 off the 32-unit blocks; K = 60 -- one partly masked chunk -- up to 1256; pre-sigmoid sums over [-4, 4] and
    beyond) and the three golden nets, in pair, split and fp32 mode: 700 leaves, every row under 4 E_ref + 2e-7.  A layer that lost
    its low part is 1.6 to 32 bounds away (tests/test_mainnet_ref.py)."""
    net, onet = load(gpu_ctx, tmp_path_factory, name)
    b, d, _ = P.batch_of(700, seed=M.SEED)
    got = {}
    for mode in MODES:
        switch(net, mode)
        got[mode], emb = hold(net, onet, b, d, (name, mode, "n700"))
    y = M.value_f64(onet, emb)[1]
    assert name in M.GOLDEN_NETS or (y.min() <= -4 and y.max() >= 4)
    # the mode switch really switches
    assert (got["pair"] != got["split"]).any() or (got["split"] != got["fp32"]).any()
    net.close()


# ---- 2. padded hidden widths into the policy heads ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h100_v40_k320", "h255_v255"])
def test_padded_hidden_widths_into_the_policy_heads(gpu_ctx, tmp_path_factory, name):
    """Hole 2: fc1's activations are handed to the policy heads in rows of the PADDED width (128 for 100 units, 256 for 255).  Every
    live logit of both heads under policy_ref.bound against policy_ref.logits_f64 of the call's own embedding, in the three modes;
    the values bit-equal to the plain call's.  A row stride of the unpadded width would shift every leaf after the first."""
    net, onet = load(gpu_ctx, tmp_path_factory, name)
    assert M.NETS[name]["H"] != M.NETS[name]["hidden"]
    b, d, r = P.batch_of(700, seed=M.SEED)
    ch = [gpu_ctx.choices(b, r, pl) for pl in range(2)]
    rows = [P.policy_rows(b, c, cnt, head) for head, (c, cnt) in enumerate(ch)]
    for mode in MODES:
        switch(net, mode)
        vals, emb = hold(net, onet, b, d, (name, mode, "policy_values_n700"))
        v2, l1, l2 = net.value_policy_inference(b, d, ch[0][0], ch[0][1], ch[1][0], ch[1][1])
        assert np.array_equal(v2.view(np.uint32), vals.view(np.uint32))
        for lg, (_, cnt) in zip((l1, l2), ch):
            assert np.isfinite(lg).all() and (lg.view(np.uint32)[np.arange(9)[None, :] >= cnt.astype(np.int64)[:, None]] == 0).all()
        ref = P.logits_f64(onet, emb)
        e_ref, s, cnt = P.yardstick(ref, P.oracle_logits(onet, emb), rows)
        worst, lim = P.worst_error((l1, l2), ref, rows), P.bound(e_ref, s)
        RECORDS["|".join((name, mode, "policy_logits_n700"))] = dict(worst=worst, E_ref=e_ref, S=s, bound=lim, logits=cnt, rows=700)
        print("%s %s logits: worst %.3g, E_ref %.3g, S %.3g, bound %.3g over %d logits" % (name, mode, worst, e_ref, s, lim, cnt))
        assert cnt > 5000 and worst <= lim, (name, mode, worst, e_ref, s, lim)
    net.close()


# ---- 3. sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h33_v1_k320", "256"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 96, 97, 127, 128, 129, 257])
def test_sizes_around_the_tiles_in_every_mode(gpu_ctx, tmp_path_factory, name, n):
    """Hole 6: the 32-row wave tiles and the 128-row groups in pair, split and fp32 mode.  At 1, 31, 32, 33, 96, 129 and 257 rows one
    to three of a workgroup's four waves have no rows and still feed the weight ring and the barriers."""
    net, onet = load(gpu_ctx, tmp_path_factory, name)
    b, d, _ = P.batch_of(n, seed=M.SEED)
    for mode in MODES:
        switch(net, mode)
        hold(net, onet, b, d, (name, mode, "n%d" % n))
    net.close()


# ---- 4. the second grid-stride sweep --------------------------------------------------------------------------------------------
def _first_rows(name, onet, emb):
    """The oracle's values on the first 4,096 rows of a net's batch, computed once per net (batch_of's batches share their prefix)."""
    e = np.ascontiguousarray(emb[:4096])
    if name not in _SHARED or not np.array_equal(_SHARED[name][0], e):
        _SHARED[name] = (e, M.oracle_values(onet, e))
    return _SHARED[name][1]


def _per_leaf(net, name, mode):
    """The values of every leaf of form_states() (batch_of's seeded order) from calls of at most 4,096 rows, once per net and mode."""
    if (name, mode) not in _SHARED:
        total = P.form_states()[0].shape[0]
        b, d, _ = P.batch_of(total, seed=M.SEED)
        _SHARED[name, mode] = np.concatenate([net.value_inference(b[i:i + 4096], d[i:i + 4096]) for i in range(0, total, 4096)])
    return _SHARED[name, mode]


@pytest.mark.parametrize("name", ["h33_v1_k320", "h100_v40_k320", "h96_v160_k536", "256"])
@pytest.mark.parametrize("n", [32768, 32769, 32801, 65536, 65569])
def test_second_sweep_in_every_mode(gpu_ctx, tmp_path_factory, name, n):
    """Holes 3 and 4: the grid is 256 workgroups of 128 rows, so above 32,768 rows a workgroup takes a second group while its weight
    ring keeps running.  The three random nets take an ODD number of ring phases per group in k_mainnet_pair (7, 9, 17 at NB 2, 4,
    8): their second groups start on ring buffer 1 with the phase counter wrapped; net_256 takes 20.  EVERY row under the bound in
    pair, split and fp32 mode (E_ref from the oracle on the first 4,096 rows), and every row bit-equal to the same leaf's value
    from a call of at most 4,096 rows (the batch repeats form_states()' leaves): a second group that read the wrong buffer, or a
    value that depends on the sweep, fails both."""
    net, onet = load(gpu_ctx, tmp_path_factory, name)
    t = M.NETS[name]
    assert (t["pair_phases"] % 2 == 1) == (name != "256") and n > 32767
    b, d, _ = P.batch_of(n, seed=M.SEED)
    total = P.form_states()[0].shape[0]
    ref = None
    for mode in MODES:
        switch(net, mode)
        vals, emb = net.value_inference(b, d, return_embedding=True)
        if ref is None or not np.array_equal(emb, emb0):
            ref, emb0 = M.value_f64(onet, emb)[0], emb
        e_ref = float(np.abs(_first_rows(name, onet, emb).astype(np.float64) - ref[:4096]).max())
        worst, lim = float(np.abs(vals.astype(np.float64) - ref).max()), P.bound(e_ref, 1.0)
        RECORDS["|".join((name, mode, "n%d" % n))] = dict(worst=worst, E_ref=e_ref, bound=lim, rows=n)
        print("%s %s n%d: worst %.3g, E_ref %.3g, bound %.3g" % (name, mode, n, worst, e_ref, lim))
        assert np.isfinite(vals).all() and worst <= lim, (name, mode, n, worst, e_ref, lim, int(np.abs(vals - ref).argmax()))
        small = _per_leaf(net, name, mode)
        bad = np.nonzero(vals.view(np.uint32) != small[np.arange(n) % total].view(np.uint32))[0]
        assert bad.size == 0, (name, mode, n, bad.size, bad[:8])
    net.close()


# ---- 5. a pure function of the leaf ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h32_k60", "h33_v1_k320", "256"])
def test_value_is_a_pure_function_of_the_leaf(gpu_ctx, tmp_path_factory, name):
    """Hole 9: 40,000 leaves (a second sweep for 57 workgroups) in pair, split and fp32 mode, bit for bit: the call repeated 8 times;
    a permuted batch gives the permuted values; rows 0, 31, 32, 127, 128, 32,767, 32,768 and 39,999 evaluated alone give their entry.
    The two narrow nets have the shortest ring phases (k_mainnet_pair<1>: 8 MFMAs, <2>: 24) -- where a phase could start on bytes
    still in flight (ms_next_phase's comment: stale reads on 64-wide nets, about one run in twelve)."""
    net, onet = load(gpu_ctx, tmp_path_factory, name)
    n = 40000
    b, d, _ = P.batch_of(n, seed=M.SEED)
    perm = np.random.default_rng(5).permutation(n)
    bp, dp = np.ascontiguousarray(b[perm]), np.ascontiguousarray(d[perm])
    for mode in MODES:
        switch(net, mode)
        v0 = net.value_inference(b, d).view(np.uint32)
        for rep in range(8):
            assert np.array_equal(net.value_inference(b, d).view(np.uint32), v0), (mode, rep)
        assert np.array_equal(net.value_inference(bp, dp).view(np.uint32), v0[perm]), mode
        for i in (0, 31, 32, 127, 128, 32767, 32768, 39999):
            assert net.value_inference(b[i:i + 1], d[i:i + 1]).view(np.uint32)[0] == v0[i], (mode, i)
    net.close()


# ---- 6. the sigmoid -------------------------------------------------------------------------------------------------------------
def test_sigmoid_over_its_whole_range(gpu_ctx, tmp_path_factory):
    """Hole 7: net_256 with value_fc3 x 2^10 -- pre-sigmoid sums from below -90 to above 90 (tests/test_mainnet_ref.py asserts both on
    the CPU), past where expf overflows (88.7).  Every value is finite, in [0, 1] and under the float64 bound; exactly 0.0 where
    float64 says < 1e-38 and exactly 1.0 where it says > 1 - 1e-8; the three modes saturate on the same rows."""
    net, onet = load(gpu_ctx, tmp_path_factory, M.SIGMOID_NET)
    b, d, _ = P.batch_of(700, seed=M.SIGMOID_SEED)
    sat = {}
    for mode in MODES:
        switch(net, mode)
        vals, emb = hold(net, onet, b, d, (M.SIGMOID_NET, mode, "n700"))
        ref, y = M.value_f64(onet, emb)
        assert (y < -90).any() and (y > 90).any()
        assert (vals[ref < 1e-38] == 0.0).all() and (vals[ref > 1 - 1e-8] == 1.0).all()
        sat[mode] = (vals == 0.0).astype(np.int8) + 2 * (vals == 1.0)
        assert (sat[mode] == 1).any() and (sat[mode] == 2).any() and (sat[mode] == 0).any()
    assert np.array_equal(sat["pair"], sat["split"]) and np.array_equal(sat["pair"], sat["fp32"])
    net.close()


# ---- 7. poisoned output buffers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h100_v40_k320", "256"])
def test_poisoned_output_buffers(gpu_ctx, tmp_path_factory, name):
    """Hole 8: oakgpu_leaf_eval_dev on a values buffer of n + 64 floats and an embedding buffer of n K + 64 floats preset to 0x7F
    bytes, 1,003 leaves (7 full groups and a ragged one of 107 rows): per mode the first n values are the host call's bit for bit,
    none is the preset pattern, and both guard bands keep it."""
    from hipmem import Dev
    from oak_amd import _lib
    net, onet = load(gpu_ctx, tmp_path_factory, name)
    n, guard, K = 1003, 64, M.NETS[name]["K"]
    b, d, _ = P.batch_of(n, seed=M.SEED)
    gb, gd = Dev(b), Dev(d)
    for mode in MODES:
        switch(net, mode)
        v0, e0 = net.value_inference(b, d, return_embedding=True)
        gv, ge = Dev(np.zeros(n + guard, F), fill=0x7F), Dev(np.zeros(n * K + guard, F), fill=0x7F)
        _lib.check(gpu_ctx.lib.oakgpu_leaf_eval_dev(gpu_ctx.handle, net.handle, gb.p, gd.p, n, gv.p, ge.p))
        gpu_ctx.synchronize()
        v, e = gv.host().view(np.uint32), ge.host().view(np.uint32)
        gv.free(); ge.free()
        assert (v[n:] == 0x7F7F7F7F).all() and (e[n * K:] == 0x7F7F7F7F).all(), mode
        assert (v[:n] != 0x7F7F7F7F).all() and (e[:n * K] != 0x7F7F7F7F).all(), mode
        assert np.array_equal(v[:n], v0.view(np.uint32)) and np.array_equal(e[:n * K], e0.view(np.uint32).ravel()), mode
    gb.free(); gd.free()
    net.close()
