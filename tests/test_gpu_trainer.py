"""GPU: the trainer (oak_amd.train.Trainer, oak_amd/csrc/trainer.hip) against its referee tests/trainer_ref.py: forward, loss terms and
every gradient entry under the project's rule (4 x the fp32 referee's own distance from float64 + 2e-7 of the scale), the rows that are
not OK, repeatability, Adam alone against the formula, step = gradients + adam, the learning check, the `.battle.net` round trip and
the training tool.  The referee itself is held in tests/test_trainer_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import policy_ref as P
import train_ref as T
import trainer_ref as TR
from oak_amd import _lib, netfile
from oak_amd.train import EncodedBattleFrames, FIELDS, Trainer, train_loss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LOSS = (0.25, 0.25, 0.5, 0.25, 1.0, 0.5)
NETS = ("tiny", "default", "256", "ragged")
# the edges of a 32-row MFMA block and of the 64-row tile, one past a 256-row chain / partial
ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 257)
MAX_ROWS = 257
_CACHE = {}


def _loss(t=LOSS):
    return train_loss(*t)


def _net_bytes(tag):
    if ("net", tag) not in _CACHE:
        if tag == "ragged":
            import tempfile
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "ragged.battle.net")
                netfile.write_random_net(path, seed=11, activation=2, **TR.RAGGED)
                _CACHE["net", tag] = open(path, "rb").read()
        else:
            _CACHE["net", tag] = open(P.GOLDEN[tag], "rb").read()
    return _CACHE["net", tag]


def _real(ctx):
    """Every frame of records 32 .. 38 of the train-frames test world (the records with targets) and two picks out of range, encoded on
    the device: (batch dict, picks)."""
    if "real" not in _CACHE:
        from test_gpu_train_frames import _all_picks, _world
        games, recs, tref, corpus = _world(ctx)
        picks = np.concatenate([_all_picks(tref, range(32, 39)), np.array([(32, 60000), (9999, 0)], np.uint32)])
        enc = EncodedBattleFrames(len(picks))
        assert corpus.encode(enc, picks) == len(picks) - 2
        _CACHE["real"] = ({name: getattr(enc, name).copy() for name in FIELDS}, picks)
    return _CACHE["real"]


def _batch(ctx):
    if "batch" not in _CACHE:
        _CACHE["batch"] = TR.make_batch(_real(ctx)[0])
    return _CACHE["batch"]


def _frames(batch, n, device="cuda:0"):
    """The first n rows of a batch dict as an EncodedBattleFrames on the device (or numpy for device=None)."""
    enc = EncodedBattleFrames(max(n, 1), device)
    for name in FIELDS:
        src = np.ascontiguousarray(batch[name][:n])
        dst = getattr(enc, name)
        if device is None:
            dst[:n] = src
        elif src.dtype == np.uint32:
            dst.view(torch.int32)[:n].copy_(torch.from_numpy(src.view(np.int32)))
        else:
            dst[:n].copy_(torch.from_numpy(src))
    return enc


def _trainer(ctx, tag):
    """One trainer per network, shared by the tests that change no parameter."""
    if ("trainer", tag) not in _CACHE:
        _CACHE["trainer", tag] = Trainer(ctx, _net_bytes(tag), MAX_ROWS)
    return _CACHE["trainer", tag]


def _referee(ctx, tag, n, loss=LOSS):
    """The float64 and float32 referees on the first n rows of the batch: forward outputs, gradients and the sums S, computed once."""
    key = ("ref", tag, n, loss)
    if key not in _CACHE:
        batch = _batch(ctx)
        r64, r32 = TR.Ref(_net_bytes(tag)), TR.Ref(_net_bytes(tag), torch.float32)
        o64, o32 = r64.run(batch, n, loss), r32.run(batch, n, loss)
        (g64, S), (g32, _) = r64.backward(), r32.backward()
        _CACHE[key] = (o64, o32, g64, g32, S)
    return _CACHE[key]


def test_the_batch_holds_its_edges(gpu_ctx):
    b = _batch(gpu_ctx)
    assert b["k"][0, 0, 0] == 1 and not b["empirical_policies"][1, 1].any() and not b["hp"][2, :, 1:].any() and not b["hp"][3, :, 0].any()
    assert b["status"][4] != 0 and (b["status"][:13] == 0).sum() == 12 and (b["status"] != 0).sum() == 2
    assert sum(7 in b["choice_indices"][i, 0, :int(b["k"][i, 0, 0])] for i in range(13)) >= 2   # one fc3 row named by several rows
    assert len(b["status"]) >= MAX_ROWS and (b["k"][:MAX_ROWS] == 9).any()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("tag", NETS)
def test_forward_and_terms(gpu_ctx, tag, n):
    """Value, every legal logit, sq_err and ce of every row against the float64 referee: 4 x the fp32 referee's worst distance from
    float64 over the batch + 2e-7 x the scale (1 for the value and sq_err, max(1, max |logit|) for the logits and ce).  The outputs are
    written into NaN-filled buffers with a guard row on either side; the rows that are not OK read 0."""
    batch = _batch(gpu_ctx)
    o64, o32 = _referee(gpu_ctx, tag, n)[:2]
    tr = _trainer(gpu_ctx, tag)
    shapes = {"value": (), "logits": (2, 9), "sq_err": (), "ce": (2,)}
    guarded = {name: torch.full((n + 2,) + tail, float("nan"), device="cuda:0") for name, tail in shapes.items()}
    tr.forward(_frames(batch, n), n, _loss(), out={name: t[1:n + 1] for name, t in guarded.items()})
    rep = tr.report()
    scale = max(1.0, float(np.abs(o64["logits"]).max()))
    for name in shapes:
        g = guarded[name].cpu().numpy().astype(np.float64)
        assert np.isnan(g[0]).all() and np.isnan(g[-1]).all(), name
        got = g[1:n + 1]
        assert np.isfinite(got).all(), name
        e_ref = float(np.abs(o32[name] - o64[name]).max())
        bound = P.bound(e_ref, 1.0 if name in ("value", "sq_err") else scale)
        worst = float(np.abs(got - o64[name]).max())
        print("%s n=%d %s: worst %.3g, bound %.3g (%.2f)" % (tag, n, name, worst, bound, worst / bound))
        assert worst <= bound, (name, worst, bound)
        assert (got[batch["status"][:n] != 0] == 0).all()
        live = np.arange(9)[None, None, :] < batch["k"][:n]
        if name == "logits":
            assert (got[~live] == 0).all()
    assert rep["rows"] == o64["rows"]
    for name in ("loss", "mse", "ce_p1", "ce_p2"):
        assert abs(rep[name] - o64[name]) <= P.bound(abs(o32[name] - o64[name]), max(1.0, scale)), name


def _check_gradients(tr, refs, tag, n, loss):
    o64, o32, g64, g32, S = refs
    got = tr.read("gradients")
    shares = {}
    for i, name in enumerate(TR.LAYERS):
        if g64[i] is None:
            continue
        for j, kind in enumerate(("bias", "weight")):
            assert np.isfinite(got[i][j]).all(), (name, kind)
            bound = TR.gradient_bound(g32[i][j], g64[i][j], S[i][j])
            worst = float(np.abs(got[i][j].astype(np.float64) - g64[i][j]).max())
            shares[name + "." + kind] = worst / bound if bound else 0.0
            assert worst <= bound, (tag, n, name, kind, worst, bound)
            untouched = g64[i][j] == 0                       # (entries no OK row reaches: policy rows no legal choice names, dead inputs)
            assert (got[i][j][untouched & (np.abs(g32[i][j]) == 0)] == 0).all(), (name, kind)
    print("%s n=%d gradient shares of the bound: max %.3f (%s)" % (tag, n, max(shares.values()), max(shares, key=shares.get)))
    return shares


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("tag", NETS)
def test_gradients(gpu_ctx, tag, n):
    """Every entry of all 24 tensors: per tensor max |g_dev - g64| <= 4 max |g32 - g64| + 2e-7 S, S = the largest over entries of
    sum_rows |dZ| |X| (weights) or sum_rows |dZ| (biases), from the referee.  Entries that no OK row reaches are exactly 0 -- among them
    the fc3 rows of policy indices that no legal choice names, weights and biases alike."""
    batch = _batch(gpu_ctx)
    refs = _referee(gpu_ctx, tag, n)
    tr = _trainer(gpu_ctx, tag)
    tr.set_gradients(np.full(tr.count, np.nan, F))
    tr.gradients(_frames(batch, n), n, _loss())
    _check_gradients(tr, refs, tag, n, LOSS)
    ok = batch["status"][:n] == 0
    got = tr.read("gradients")
    for s, layer in enumerate((9, 11)):
        named = np.zeros(315, bool)
        for i in np.nonzero(ok)[0]:
            named[batch["choice_indices"][i, s, :int(batch["k"][i, s, 0])]] = True
        assert (got[layer][0][~named] == 0).all() and (got[layer][1][~named] == 0).all()
    rep = tr.report()
    assert rep["rows"] == refs[0]["rows"] and rep["steps"] == {"trunk": 0, "value": 0, "policy": 0}


@pytest.mark.parametrize("loss", [(0.0, 0.0, 1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0, 2.0, 0.0)])
def test_gradients_of_one_head_alone(gpu_ctx, loss):
    """A zero loss weight: the other head's gradient reaches the trunk alone, within the same bound, and the group without a gradient keeps
    its gradient block's bits."""
    batch, n = _batch(gpu_ctx), 65
    refs = _referee(gpu_ctx, "tiny", n, loss)
    tr = _trainer(gpu_ctx, "tiny")
    planted = np.random.default_rng(1).standard_normal(tr.count).astype(F)
    tr.set_gradients(planted)
    tr.gradients(_frames(batch, n), n, _loss(loss))
    _check_gradients(tr, refs, "tiny", n, loss)
    got, kept = tr.read("gradients"), tr.split(planted)
    for i, name in enumerate(TR.LAYERS):
        if refs[2][i] is None:
            assert got[i][0].tobytes() == kept[i][0].tobytes() and got[i][1].tobytes() == kept[i][1].tobytes(), name


def test_rows_that_are_not_ok_may_hold_anything(gpu_ctx):
    """NaN in every float tensor and garbage indices and counts in the rows that are not OK: the same gradient and report bits as zeros there."""
    batch, n = _batch(gpu_ctx), 65
    bad = np.concatenate([np.nonzero(batch["status"][:n] != 0)[0], [0, 9, 33, 64]])
    nan, zero = TR.spoil(batch, bad)
    tr = _trainer(gpu_ctx, "default")
    out = []
    for b in (nan, zero):
        tr.gradients(_frames(b, n), n, _loss())
        out.append((tr.read("gradients", flat=True), tr.report()))
    assert np.isfinite(out[0][0]).all() and out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1] == out[1][1] and out[0][1]["rows"] == n - len(bad) and np.isfinite(out[0][1]["loss"])
    fwd = tr.forward(_frames(nan, n), n, _loss())
    for name, t in fwd.items():
        assert (t.cpu().numpy()[bad] == 0).all(), name


def test_no_ok_row_changes_nothing(gpu_ctx):
    batch, n = _batch(gpu_ctx), 5
    b = TR.take(batch, np.arange(n))
    b["status"][:] = 3
    tr = Trainer(gpu_ctx, _net_bytes("tiny"), 8)
    before = [tr.read(w, flat=True) for w in ("parameters", "m", "v")]
    tr.step(_frames(b, n), n, _loss(), lr=1e-2)
    rep = tr.report()
    assert rep["rows"] == 0 and rep["loss"] == 0.0 and rep["steps"] == {"trunk": 0, "value": 0, "policy": 0}
    for w, x in zip(("parameters", "m", "v"), before):
        assert tr.read(w, flat=True).tobytes() == x.tobytes(), w
    assert not tr.read("gradients", flat=True).any()
    tr.close()


def test_repeatable_and_no_stale_workspace(gpu_ctx):
    """A second call gives the same bits; n = 1 after n = 257 equals a fresh trainer's n = 1; the numpy (staged) rows give the device rows' bits."""
    batch = _batch(gpu_ctx)
    tr = _trainer(gpu_ctx, "default")
    runs = []
    for device in ("cuda:0", "cuda:0", None):
        tr.set_gradients(np.full(tr.count, np.nan, F))
        tr.gradients(_frames(batch, 257, device), 257, _loss())
        runs.append((tr.read("gradients", flat=True), tr.report()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() == runs[2][0].tobytes() and runs[0][1] == runs[1][1] == runs[2][1]
    tr.gradients(_frames(batch, 1), 1, _loss())
    after = (tr.read("gradients", flat=True), tr.report(), {k: v.cpu().numpy() for k, v in tr.forward(_frames(batch, 1), 1, _loss()).items()})
    fresh = Trainer(gpu_ctx, _net_bytes("default"), 1)
    fresh.gradients(_frames(batch, 1), 1, _loss())
    assert fresh.read("gradients", flat=True).tobytes() == after[0].tobytes() and fresh.report() == after[1]
    for k, v in fresh.forward(_frames(batch, 1), 1, _loss()).items():
        assert v.cpu().numpy().tobytes() == after[2][k].tobytes(), k
    fresh.close()


def test_refusals_on_the_device(gpu_ctx):
    tr = _trainer(gpu_ctx, "tiny")
    batch = _batch(gpu_ctx)
    with pytest.raises(_lib.OakGpuError, match="exceed max_rows"):
        tr.gradients(EncodedBattleFrames(MAX_ROWS + 1, "cuda:0"), MAX_ROWS + 1, _loss())
    with pytest.raises(_lib.OakGpuError, match="both zero"):
        tr.step(_frames(batch, 2), 2, train_loss(value_weight=0.0, policy_weight=0.0), lr=1e-3)
    with pytest.raises(_lib.OakGpuError, match="embedding widths above 128"):
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            netfile.write_random_net(os.path.join(d, "w.battle.net"), pokemon_out=129)
            Trainer(gpu_ctx, os.path.join(d, "w.battle.net"), 4)


# ---- Adam alone ----------------------------------------------------------------------------------------------------------------------
PLANTED = np.array([0.0, 1e-20, -1e-20, 1e-12, -1e-12, 1.0, -1.0, 1e4, -1e4], F)


def _kinds(tr):
    """Per parameter: (group 0..2, is a weight)."""
    group, weight = [], []
    for i, (n_in, n_out) in enumerate(tr.dims):
        g = TR.GROUP[TR.LAYERS[i]]
        group += [g] * (n_out * (n_in + 1))
        weight += [False] * n_out + [True] * (n_out * n_in)
    return np.array(group), np.array(weight)


@pytest.mark.parametrize("clamp", [False, True])
def test_adam_alone(gpu_ctx, clamp):
    """Five updates from one planted gradient block (0, +-1e-20, +-1e-12, +-1, +-1e4 in turn over the entries) against the float64 formula
    fed the same fp32 gradients and the two host scalars as the floats the kernel receives.  After step t,
        |p_dev - p_ref| <= sum over the steps s <= t of  ulp(p_s) / 2 + |update_s| c_s 2^-24,   c_s = 6.5 s + 6,
    counted from k_adam (u = 2^-24 relative; the gradient keeps its sign, so m's two terms never cancel):
      m = fma(b1, m, (1-b1) g): the product, the fma, and the fp32 constants b1 and 1-b1: 4 u per step, 4 s u after s steps;
      v = fma(b2, v, ((1-b2) g) g): two products, the fma, two constants: 5 u per step, 5 s u after s steps, halved by the square root;
      denom = sqrtf(v) / bc2 + eps: the root, the quotient, the sum, eps as a float: 4 u;   m / denom: 1 u;   step_size * that: 1 u;
      p - update: ulp(p) / 2.
    (Where g g falls below fp32's normal range, sqrt(v) < 1e-18 is far below eps u and its relative error does not reach denom.)
    lr = 0.5 with clamping, so that +-1e4 and +-1 drive weights into the clamp: it touches weights only.  Zero gradient with zero state
    moves nothing."""
    tr = Trainer(gpu_ctx, _net_bytes("tiny"), 1)
    lr = 0.5 if clamp else 1e-3
    g = PLANTED[np.arange(tr.count) % len(PLANTED)]
    group, weight = _kinds(tr)
    p0 = tr.read(flat=True)
    p, m, v = p0.astype(np.float64), np.zeros(tr.count), np.zeros(tr.count)
    allowed = np.zeros(tr.count)
    worst = 0.0
    for t in range(1, 6):
        tr.set_gradients(g)
        tr.adam(lr, clamp_parameters=clamp, groups=("trunk", "value", "policy"))
        before = p
        p, m, v, upd = TR.adam_formula(p, g, m, v, t, lr, clamp=weight if clamp else None)
        got = tr.read(flat=True)
        ulp = np.spacing(np.maximum(np.abs(before), np.abs(before - upd)).astype(F)).astype(np.float64)
        allowed += ulp / 2 + np.abs(upd) * (6.5 * t + 6) * 2.0 ** -24
        err = np.abs(got.astype(np.float64) - p)
        worst = max(worst, float((err / np.maximum(allowed, 1e-300)).max()))
        assert (err <= allowed).all(), (t, int(np.argmax(err - allowed)))
        assert got[g == 0].tobytes() == p0[g == 0].tobytes()
    if clamp:
        assert np.abs(got[weight]).max() == 2.0 and np.abs(got[~weight]).max() > 2.0
    print("adam clamp=%s: worst share of the bound %.3f" % (clamp, worst))
    gm, gv = tr.read("m", flat=True), tr.read("v", flat=True)
    assert np.abs(gm - m).max() <= 20 * 2.0 ** -24 * np.abs(m).max() and (gm[g == 0] == 0).all() and (gv[g == 0] == 0).all()
    assert tr.report()["steps"] == {"trunk": 5, "value": 5, "policy": 5}
    tr.close()


@pytest.mark.parametrize("groups, loss", [(("trunk", "policy"), (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)), (("trunk", "value"), (0.0, 0.0, 1.0, 0.0, 1.0, 0.0))])
def test_a_group_without_gradient_is_untouched(gpu_ctx, groups, loss):
    """adam on two groups, and step with a zero loss weight: the third group's parameters, m, v and step count stay bit for bit."""
    tr = Trainer(gpu_ctx, _net_bytes("tiny"), 64)
    group, _ = _kinds(tr)
    missing = ({"trunk", "value", "policy"} - set(groups)).pop()
    dead = group == {"trunk": 0, "value": 1, "policy": 2}[missing]
    tr.set_gradients(np.ones(tr.count, F))
    tr.adam(1e-2, groups=("trunk", "value", "policy"))                  # every group has state now
    before = {w: tr.read(w, flat=True) for w in ("parameters", "m", "v")}
    tr.set_gradients(np.full(tr.count, 0.5, F))
    tr.adam(1e-2, groups=groups)
    tr.step(_frames(_batch(gpu_ctx), 64), 64, _loss(loss), lr=1e-2)
    steps = tr.report()["steps"]
    for w, x in before.items():
        now = tr.read(w, flat=True)
        assert now[dead].tobytes() == x[dead].tobytes(), w
        assert (now[~dead] != x[~dead]).any(), w
    assert sorted(steps.values()) == [1, 3, 3] and steps[missing] == 1
    tr.close()


# ---- steps -----------------------------------------------------------------------------------------------------------------------------
def test_step_is_gradients_then_adam(gpu_ctx):
    """8 x step equals 8 x (gradients; adam) bit for bit, parameters and state; and the step calls return while the device is still busy --
    a spin kernel in front of them is still running when the last one has returned -- so only the report read waits."""
    batch, n = _batch(gpu_ctx), 64
    frames = _frames(batch, n)
    a, b = Trainer(gpu_ctx, _net_bytes("tiny"), n), Trainer(gpu_ctx, _net_bytes("tiny"), n)
    torch.cuda.synchronize()
    torch.cuda._sleep(1_000_000_000)                                    # some tenths of a second of device time in front of the steps
    for i in range(8):
        a.step(frames, n, _loss(), lr=1e-3 * 0.9 ** i, clamp_parameters=True)
    assert not torch.cuda.current_stream().query(), "the step calls waited for the device"
    rep = a.report()
    assert torch.cuda.current_stream().query()
    for i in range(8):
        b.gradients(frames, n, _loss())
        b.adam(1e-3 * 0.9 ** i, clamp_parameters=True)
    assert rep == b.report() and rep["steps"] == {"trunk": 8, "value": 8, "policy": 8}
    for w in ("parameters", "gradients", "m", "v"):
        assert a.read(w, flat=True).tobytes() == b.read(w, flat=True).tobytes(), w
    a.close()
    b.close()


def test_learning_check(gpu_ctx):
    """30 steps at lr 1e-3 on one fixed batch of 64 real rows of `tiny`: the device's loss decrease is at least half the float64 referee's on
    the same schedule (a sign or a scale wrong across steps shows here, not in the entrywise checks)."""
    real = _real(gpu_ctx)[0]
    batch = TR.take(real, np.random.default_rng(2).choice(len(real["status"]) - 2, 64, replace=False))
    n, lr = 64, 1e-3
    tr = Trainer(gpu_ctx, _net_bytes("tiny"), n)
    frames = _frames(batch, n)
    ref = TR.Ref(_net_bytes("tiny"))
    ms = [[np.zeros(b.shape), np.zeros(w.shape)] for b, w in ref.layers()]
    vs = [[np.zeros(b.shape), np.zeros(w.shape)] for b, w in ref.layers()]
    first = ref.run(batch, n, LOSS)["loss"]
    tr.forward(frames, n, _loss(), want=())
    dev_first = tr.report()["loss"]
    for t in range(1, 31):
        ref.run(batch, n, LOSS)
        grads, _ = ref.backward()
        with torch.no_grad():
            for i, name in enumerate(TR.LAYERS):
                for j, suffix in enumerate(("_b", "_w")):
                    par = getattr(ref, name + suffix)
                    p, ms[i][j], vs[i][j], _ = TR.adam_formula(par.detach().numpy(), grads[i][j], ms[i][j], vs[i][j], t, lr)
                    par.copy_(torch.tensor(p))
        tr.step(frames, n, _loss(), lr=lr)
    last = ref.run(batch, n, LOSS)["loss"]
    tr.forward(frames, n, _loss(), want=())
    dev_last = tr.report()["loss"]
    print("learning check: referee %.6f -> %.6f, device %.6f -> %.6f" % (first, last, dev_first, dev_last))
    assert first - last > 0.01
    assert dev_first - dev_last >= 0.5 * (first - last)
    tr.close()


@pytest.mark.parametrize("tag", NETS)
def test_round_trip(gpu_ctx, tag):
    """net_bytes() before any step is the file.  After 3 steps the bytes load into the evaluator, whose value_inference on the rows' states
    agrees with the trainer's forward within the 1e-5 the training rows are held to -- on rows without a twice-held move, where the dense
    training encoder and the sparse inference encoder differ by design."""
    from oak_amd.engine import Network
    from test_gpu_train_frames import _world
    real, picks = _real(gpu_ctx)
    n = 200
    tr = Trainer(gpu_ctx, _net_bytes(tag), n)
    assert tr.net_bytes() == _net_bytes(tag)
    frames = _frames(real, n)
    for _ in range(3):
        tr.step(frames, n, _loss(), lr=1e-3)
    data = tr.net_bytes()
    assert len(data) == len(_net_bytes(tag)) and data != _net_bytes(tag) and data[:8] == _net_bytes(tag)[:8]
    value = tr.forward(frames, n, _loss(), want=("value",))["value"].cpu().numpy()
    try:
        net = Network(gpu_ctx, data=data)
    except _lib.OakGpuError:
        if tag == "ragged":
            pytest.skip("the evaluator refuses the ragged widths")
        raise
    tref = _world(gpu_ctx)[2]
    states = [tref.walked(int(r))[0][int(f)] for r, f in picks[:n]]
    b, d = np.stack([s[0] for s in states]), np.stack([s[1] for s in states])
    leaf = net.value_inference(b, d)
    dup = T.duplicated_move_sides(b)[:, :, :2].any(axis=(1, 2))
    assert (~dup).sum() >= 150
    assert np.abs(value - leaf)[~dup].max() <= 1e-5
    tr.close()


@pytest.mark.parametrize("n", [1, 65])
def test_symmetries(gpu_ctx, n):
    """The side flip and the bench permutation on the device against the numpy restatement, bit for bit, row by row; a row's result does not
    depend on n (row i of the 65 equals the single row drawn with seed + i); each switch alone; nothing behind row n moves."""
    from oak_amd.train import apply_symmetries
    batch = _batch(gpu_ctx)
    seed = 0xABCDEF0123
    for flip, perm in ((True, True), (True, False), (False, True)):
        enc = _frames(batch, n + 1)
        apply_symmetries(gpu_ctx, enc, seed, n=n, flip_sides=flip, permute_bench=perm)
        exp = TR.symmetric(batch, n, seed, flip, perm)
        for name in FIELDS:
            t = getattr(enc, name)
            got = (t.view(torch.int32) if t.dtype == torch.uint32 else t).cpu().numpy().view(batch[name].dtype)
            assert got[:n].tobytes() == exp[name].tobytes(), (name, flip, perm)
            assert got[n:].tobytes() == batch[name][n:n + 1].tobytes(), name
    if n > 1:
        i = 37
        one = _frames(TR.take(batch, np.arange(i, i + 1)), 1)
        apply_symmetries(gpu_ctx, one, seed + i)
        exp = TR.symmetric(batch, n, seed)
        for name in ("pokemon", "hp", "active", "choice_indices", "score"):
            assert getattr(one, name).cpu().numpy().tobytes() == exp[name][i:i + 1].tobytes(), name


def test_training_tool(gpu_ctx, tmp_path):
    """tools/train_battle_net.py: 3 steps at batch 64 on the test corpus leave initial.battle.net and a loadable 3.battle.net."""
    from oak_amd.engine import Network
    from test_gpu_train_frames import _world
    recs = _world(gpu_ctx)[1]
    data_dir = tmp_path / "data"
    data_dir.mkdir()
    (data_dir / "a.battle.data").write_bytes(b"".join(recs[32:39]))
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_battle_net.py"), "--data-dir", str(data_dir), "--dir", str(out), "--network-path", P.GOLDEN["tiny"],
           "--batch-size", "64", "--lr", "1e-3", "--steps", "3", "--checkpoint", "3", "--seed", "5", "--value-empirical-weight", "0.5",
           "--value-score-weight", "0.5", "--p-nash-weight", "0.5"]
    plain = subprocess.run(cmd + ["--no-apply-symmetries", "--dir", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert (out / "initial.battle.net").read_bytes() == open(P.GOLDEN["tiny"], "rb").read()
    trained = (out / "3.battle.net").read_bytes()
    assert trained != (out / "initial.battle.net").read_bytes()
    Network(gpu_ctx, data=trained)
    assert (tmp_path / "plain" / "3.battle.net").read_bytes() not in (trained, (out / "initial.battle.net").read_bytes())
