"""GPU: the quantized ("discrete") battle network -- oakgpu_net_load_discrete*, k_mainnet_i8, k_policy_i8 and the discrete Agent --
against tests/quant_oracle.py.  The main net is integer arithmetic, so it is held bit-exact: value_fc3's int32 for every leaf
(on the GPU's own embedding bytes), the policy logits bit for bit, the values within 2 ulp (expf)."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nn_oracle as NN  # noqa: E402
import oracle_lib as O  # noqa: E402
import quant_oracle as Q  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
NET_DEFAULT = os.path.join(ROOT, "tests", "golden", "net_default.battle.net")
NET256 = os.path.join(ROOT, "tests", "golden", "net_256.battle.net")


def rewrite(src, dst, edit=None, header0=1):
    """Copy a .battle.net with header byte 0 set (1 = clamp) and edit(layer, b, W) -> (b, W) applied to its 12 Affine blocks
    (pokemon_net 0-1, active_net 2-3, fc0 4, fc1 5, value_fc2 6, value_fc3 7, policy heads 8-11)."""
    raw = open(src, "rb").read()
    out, off = [bytes([header0]) + raw[1:8]], 8
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
    open(dst, "wb").write(b"".join(out))
    return dst


def spread_main_net(i, b, W):
    """Main-net weights stretched over (-1.9, 1.9) (int8 -121..121) and biases over +-0.6: every byte value of the weights occurs."""
    if i < 4:
        return b, W
    return (b / np.abs(b).max() * F(0.6)).astype(F), (W / np.abs(W).max() * F(1.9)).astype(F)


def make_net(tmp_path, name, hidden, value_hidden, policy_hidden, seed=5, edit=spread_main_net):
    from oak_amd import netfile
    src = str(tmp_path / ("src_" + name))
    netfile.write_random_net(src, seed=seed, activation=2, hidden=hidden, value_hidden=value_hidden, policy_hidden=policy_hidden)
    return rewrite(src, str(tmp_path / name), edit)


_STATES = {}


def midgame(n, seed0=4100):
    """n random OU battles advanced 0-90 random turn-steps on the oracle (fainted slots, statuses, boosts, volatiles)."""
    key = (n, seed0)
    if key not in _STATES:
        bs, ds, rs = [], [], []
        groups = [(0, 1), (8, 2), (30, 3), (90, 4)]
        per = (n + len(groups) - 1) // len(groups)
        for steps, k in groups:
            b, d, p, r = O.make_random_ou_batch(per, seed0=seed0 + 1000 * k)
            O.rollout_batch(b, d, r, p, max_steps=steps, threads=8)
            bs.append(b)
            ds.append(d)
            rs.append(np.asarray(r, np.uint8).reshape(-1))
        _STATES[key] = (np.concatenate(bs)[:n].copy(), np.concatenate(ds)[:n].copy(), np.concatenate(rs)[:n].copy())
    return _STATES[key]


def raw_eval(ctx, net, b, d):
    """oakgpu_leaf_eval_discrete_raw_dev: (embedding bytes [n, 768], value_acc [n])."""
    from hipmem import Dev
    from oak_amd import _lib
    n = b.shape[0]
    gb, gd = Dev(b), Dev(d)
    qe, va = Dev(np.zeros((n, 768), np.uint8), fill=0xAB), Dev(np.zeros(n, np.int32), fill=0x7F)
    _lib.check(ctx.lib.oakgpu_leaf_eval_discrete_raw_dev(ctx.handle, net.handle, gb.p, gd.p, n, qe.p, va.p))
    ctx.synchronize()
    out = qe.host(), va.host()
    for x in (gb, gd, qe, va):
        x.free()
    return out


def ulp_diff(a, b):
    a = np.asarray(a, F).view(np.int32).astype(np.int64)
    b = np.asarray(b, F).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def load_error(ctx, path):
    from oak_amd import _lib
    from oak_amd.engine import Network
    with pytest.raises(_lib.OakGpuError) as e:
        Network(ctx, path=path, discrete=True)
    return str(e.value)


def test_loader_refusals_carry_the_reference_texts(gpu_ctx, tmp_path):
    from oak_amd.engine import Network
    assert "Agent: .discrete was specified but the parsed header does not encode clamped activations." in load_error(gpu_ctx, NET_DEFAULT)
    msg = load_error(gpu_ctx, rewrite(NET256, str(tmp_path / "c256.net")))
    assert "Invalid layer size for quantized net Hidden: 256 (check code for valid sizes)." in msg, msg
    msg = load_error(gpu_ctx, make_net(tmp_path, "vh.net", 64, 128, 64))
    assert "Invalid layer size for quantized net Value hidden cannot be larger than hidden. (check code for valid sizes)." in msg, msg
    for val, text in ((2.0, "2.000000"), (-2.0, "-2.000000"), (np.nan, "nan")):
        def edit(i, b, W, val=val):
            if i == 5:     # fc1[3][7]: flat index 3 * 64 + 7
                W = W.copy()
                W[3, 7] = val
            return b, W
        msg = load_error(gpu_ctx, rewrite(NET_DEFAULT, str(tmp_path / "w.net"), edit))
        assert msg.split(": ", 1)[1].startswith("%dnon clamped" % (3 * 64 + 7)) and text in msg, msg
    # an embedding-net weight above 2 is fine (the embedding nets stay fp32)
    path = rewrite(NET_DEFAULT, str(tmp_path / "e.net"), lambda i, b, W: (b, W * F(40)) if i == 1 else (b, W))
    net = Network(gpu_ctx, path=path, discrete=True)
    assert gpu_ctx.lib.oakgpu_net_is_discrete(net.handle) == 1
    assert net.main_precision()[0] == "int8"
    assert gpu_ctx.lib.oakgpu_net_set_main_precision(net.handle, 2) == -1
    net.close()
    fp = Network(gpu_ctx, path=path)
    assert gpu_ctx.lib.oakgpu_net_is_discrete(fp.handle) == 0 and fp.main_precision()[0] == "pair"
    fp.close()


SHAPES = [("default", None), ("h32", (32, 32, 32)), ("h128", (128, 128, 128)), ("h128_64_32", (128, 32, 64))]


def shape_net(tmp_path, tag, dims):
    if dims is None:
        return rewrite(NET_DEFAULT, str(tmp_path / "default_clamp.net"), spread_main_net)
    return make_net(tmp_path, tag + ".net", *dims)


@pytest.mark.parametrize("tag,dims", SHAPES)
def test_integer_main_net_is_bit_exact(gpu_ctx, tmp_path, tag, dims):
    from oak_amd.engine import Network
    path = shape_net(tmp_path, tag, dims)
    net, qn = Network(gpu_ctx, path=path, discrete=True), Q.QuantNet(path)
    assert net.shape()[1:] == (qn.H, qn.VH, qn.PH)
    b, d, r = midgame(4096)
    qe, va = raw_eval(gpu_ctx, net, b, d)
    stats = {}
    exp = qn.value_acc(qe, stats)
    bad = np.flatnonzero(exp != va)
    assert bad.size == 0, (tag, bad.size, int(bad[0]), int(va[bad[0]]), int(exp[bad[0]]))
    vals = net.value_inference(b, d)
    assert ulp_diff(vals, Q.sigmoid(exp.astype(F) / Q.CONV)).max() <= 2
    # policy logits, bit for bit
    c1, n1 = gpu_ctx.choices(b, r, 0)
    c2, n2 = gpu_ctx.choices(b, r, 1)
    k = 512
    v2, l1, l2 = net.value_policy_inference(b[:k], d[:k], c1[:k], n1[:k], c2[:k], n2[:k])
    assert (v2 == vals[:k]).all()
    e1, e2 = qn.policy_logits(qe[:k], b[:k], c1[:k], n1[:k], c2[:k], n2[:k])
    assert (l1 == e1).all() and (l2 == e2).all(), (np.argwhere(l1 != e1)[:4], np.argwhere(l2 != e2)[:4])
    print("shape %s: %d leaves exact, %d saturated fc0 pairs" % (tag, len(b), stats.get("saturated", 0)))
    net.close()


def _byte_mismatches(qn, qe, b, d, n):
    """Leaves' embedding bytes against the oracle's; differences are allowed only where the oracle's 127 f lies within 1e-4
    (relative) of an integer (the fp32 embedding is held to ~1e-6, not bit for bit)."""
    edge = bad = total = 0
    for i in range(n):
        e = qn.embedding(b[i], d[i])
        ob = Q.cast_u8(e)
        diff = np.flatnonzero(ob != qe[i])
        total += e.size
        if diff.size:
            v = F(127) * e[diff].astype(F)
            near = np.abs(v - np.round(v)) <= 1e-4 * np.maximum(np.abs(v), 1)
            edge += int(near.sum())
            bad += int((~near).sum())
    return edge, bad, total


def test_embedding_bytes_match_the_oracle(gpu_ctx, tmp_path):
    from oak_amd.engine import Network
    path = shape_net(tmp_path, "default", None)
    net, qn = Network(gpu_ctx, path=path, discrete=True), Q.QuantNet(path)
    b, d, _ = midgame(4096)
    qe, _ = raw_eval(gpu_ctx, net, b, d)
    edge, bad, total = _byte_mismatches(qn, qe, b, d, 384)
    print("embedding bytes: %d boundary cases of %d" % (edge, total))
    assert bad == 0 and edge <= total // 1000
    # embedding_out keeps its meaning: the fp32 embedding before quantization
    vals, emb = net.value_inference(b[:64], d[:64], return_embedding=True)
    assert (Q.cast_u8(emb) == qe[:64]).all()
    net.close()


def test_hot_net_saturates_and_stays_exact(gpu_ctx, tmp_path):
    """The pokemon net's second layer scaled up: many bench bytes above 127, many past 255 (wrapped), fc0 pairs saturate."""
    from oak_amd.engine import Network
    path = rewrite(NET_DEFAULT, str(tmp_path / "hot.net"), lambda i, b, W: (b * F(12), W * F(12)) if i == 1 else spread_main_net(i, b, W))
    net, qn = Network(gpu_ctx, path=path, discrete=True), Q.QuantNet(path)
    b, d, _ = midgame(4096)
    qe, va = raw_eval(gpu_ctx, net, b, d)
    stats = {}
    exp = qn.value_acc(qe, stats)
    high = int((qe > 127).sum())
    print("hot net: %d bytes above 127, %d saturated fc0 pairs" % (high, stats["saturated"]))
    assert high > 0 and stats["saturated"] > 0
    assert (exp == va).all(), np.flatnonzero(exp != va)[:8]
    edge, bad, total = _byte_mismatches(qn, qe, b, d, 64)
    assert bad == 0 and edge <= total // 1000
    net.close()


def test_ragged_and_large_batches(gpu_ctx, tmp_path):
    from oak_amd.engine import Network
    path = shape_net(tmp_path, "default", None)
    net, qn = Network(gpu_ctx, path=path, discrete=True), Q.QuantNet(path)
    b, d, _ = midgame(4096)
    for n in (1, 31, 32, 33, 129, 257):
        qe, va = raw_eval(gpu_ctx, net, b[:n], d[:n])
        assert (qn.value_acc(qe) == va).all(), n
        vals = net.value_inference(b[:n], d[:n])
        assert ulp_diff(vals, Q.sigmoid(va.astype(F) / Q.CONV)).max() <= 2, n
    reps = 65536 // 4096
    bb, dd = np.tile(b, (reps, 1)), np.tile(d, (reps, 1))
    qe, va = raw_eval(gpu_ctx, net, bb, dd)
    vals = net.value_inference(bb, dd)
    assert np.isfinite(vals).all() and ((vals > 0) & (vals < 1)).all()
    idx = np.random.default_rng(3).choice(65536, 512, replace=False)
    assert (qn.value_acc(qe[idx]) == va[idx]).all()
    assert (va.reshape(reps, 4096) == va[:4096][None, :]).all()
    net.close()


def test_cached_path_equals_plain_eval(gpu_ctx, tmp_path):
    from hipmem import Dev
    from oak_amd import _lib
    from oak_amd.engine import Network
    path = shape_net(tmp_path, "default", None)
    net = Network(gpu_ctx, path=path, discrete=True)
    n = 1000
    b, d, p, r = O.make_random_ou_batch(n, seed0=9100)
    vp, vc = Dev(np.zeros(n, F)), Dev(np.zeros(n, F))
    ep, ec = Dev(np.zeros((n, 768), F)), Dev(np.zeros((n, 768), F), fill=0x7F)
    tags = Dev(np.zeros((n, 10, 6), np.uint32), fill=0xFF)
    for turn in range(12):
        gb, gd = Dev(b), Dev(d)
        _lib.check(gpu_ctx.lib.oakgpu_leaf_eval_dev(gpu_ctx.handle, net.handle, gb.p, gd.p, n, vp.p, ep.p))
        _lib.check(gpu_ctx.lib.oakgpu_leaf_eval_cached_dev(gpu_ctx.handle, net.handle, gb.p, gd.p, n, vc.p, ec.p, tags.p))
        gpu_ctx.synchronize()
        assert (ep.host() == ec.host()).all() and (vp.host() == vc.host()).all(), turn
        gb.free(); gd.free()
        O.rollout_batch(b, d, r, p, max_steps=1, threads=8)
    for x in (vp, vc, ep, ec, tags):
        x.free()
    net.close()


def test_discrete_agent_search(gpu_ctx, tmp_path):
    from oak_amd import _lib
    from oak_amd.engine import Network
    from oak_amd.parse import parse_battle, result_from_state
    from oak_amd.search import _output_dict
    path = shape_net(tmp_path, "default", None)
    qn = Q.QuantNet(path)
    b, d = parse_battle("starmie surf recover psychic thunderwave | rhydon earthquake rockslide bodyslam substitute")
    res = result_from_state(b)

    def run(budget, discrete, seed=11, bandit=b"pucb-1.0", p=path):
        out = _lib.SearchOutput()
        agent = _lib.Agent(budget=budget, bandit=bandit, eval=p.encode(), matrix_ucb=b"", discrete=discrete, table=0)
        _lib.check(gpu_ctx.lib.oakgpu_search_agent(gpu_ctx.handle, b.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), int(res),
                                                   C.byref(agent), 0, seed, C.byref(out)))
        return _output_dict(out)

    o = run(b"0", 1)
    u = Q.cast_u8(qn.embedding(b, d))[None, :]
    c1, n1 = gpu_ctx.choices(b[None, :], np.array([res], np.uint8), 0)
    c2, n2 = gpu_ctx.choices(b[None, :], np.array([res], np.uint8), 1)
    e1, e2 = qn.policy_logits(u, b[None, :], c1, n1, c2, n2)
    assert abs(o["initial_value"] - float(qn.value(u)[0])) <= 2e-7
    assert np.array_equal(np.asarray(o["p1_logit"][:o["m"]], F), e1[0, :o["m"]])
    assert np.array_equal(np.asarray(o["p2_logit"][:o["n"]], F), e2[0, :o["n"]])
    # the fp32 network of the same path is another handle (the g_nets key includes the flag)
    of = run(b"0", 0)
    net = Network(gpu_ctx, path=path)
    assert abs(of["initial_value"] - float(net.value_inference(b[None, :], d[None, :])[0])) <= 1e-6
    assert of["initial_value"] != o["initial_value"]
    net.close()
    assert run(b"0", 1)["initial_value"] == o["initial_value"]
    # deterministic for a seed
    s1, s2 = run(b"4096", 1, seed=5), run(b"4096", 1, seed=5)
    assert s1["iterations"] == 4096 and np.array_equal(s1["visit_matrix"], s2["visit_matrix"])
    assert np.array_equal(s1["value_matrix"], s2["value_matrix"])
    # a ReLU file is refused with the reference's text
    with pytest.raises(_lib.OakGpuError) as e:
        run(b"0", 1, p=NET_DEFAULT)
    assert "Agent: .discrete was specified but the parsed header does not encode clamped activations." in str(e.value)
    gpu_ctx.lib.oakgpu_agent_networks_clear(gpu_ctx.handle)


def test_pyoak_cpp_inference_discrete(gpu_ctx, tmp_path):
    from oak_amd import pyoak
    from oak_amd.engine import Context, Network
    from oak_amd.frames import read_frames, selfplay_game
    path = shape_net(tmp_path, "default", None)
    qn = Q.QuantNet(path)
    ctx = Context(0)
    teams = np.array([[[143, 34, 156, 0, 0]] + [[0] * 5] * 5, [[121, 94, 86, 105, 0]] + [[0] * 5] * 5], dtype=np.uint8)
    rec, n_frames, _ = selfplay_game(ctx, teams, battle_seed=7, iterations=512, batch=128, evaluator="mc", seed=3)
    out = pyoak.cpp_inference(bytes(rec), path, discrete=True)
    fp = pyoak.cpp_inference(bytes(rec), path)
    assert out["value"].shape == (n_frames,) and ((out["value"] > 0) & (out["value"] < 1)).all()
    assert not np.array_equal(out["value"], fp["value"])
    battle = read_frames(rec)[0]["battle"]
    u = Q.cast_u8(qn.embedding(battle, np.zeros(8, np.uint8)))[None, :]
    assert abs(out["value"][0] - float(qn.value(u)[0])) <= 2e-7
    # frame 0 again through a discrete Network handle: the same integer path as the discrete agent's
    net = Network(ctx, path=path, discrete=True)
    assert abs(out["value"][0] - float(net.value_inference(battle.reshape(1, 384), np.zeros((1, 8), np.uint8))[0])) <= 2e-7
    net.close()
    ctx.close()
