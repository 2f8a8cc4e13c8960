"""CPU: the trainer's referee (tests/trainer_ref.py) tied to code that is already pinned -- the float64 forward of
test_gpu_train_frames.test_training_rows_give_the_inference_value, corpus_eval_ref.row_terms, torch.optim.Adam -- its planted mistakes
held against the gradient bound the GPU tests use, and the host-only check of the trainer's refusals."""
import os

import numpy as np
import pytest
import torch

import corpus_eval_ref as CE
import policy_ref as P
import trainer_ref as TR
from oak_amd import _lib, netfile
from oak_amd.train import train_loss, trainer_check

F = np.float32
LOSS = (0.25, 0.25, 0.5, 0.25, 1.0, 0.5)


def _net(tag):
    return open(P.GOLDEN[tag], "rb").read()


def test_value_is_the_pinned_float64_forward():
    """The referee's float64 value against the forward test_training_rows_give_the_inference_value holds (restated here line by line,
    numpy float64) on the host restatement's rows: same formula in the same precision, only the order of the sums differs."""
    rows = TR.host_rows()
    n = 200
    onet = P.NN.Net(P.GOLDEN["default"])
    act = (lambda x: np.maximum(x, 0.0)) if onet.activation == 1 else (lambda x: np.clip(x, 0.0, 1.0))
    f64 = lambda layer, x: x @ layer.W.astype(np.float64).T + layer.b.astype(np.float64)
    xp = rows["pokemon"][:n, :, 1:].astype(np.float64)
    xa = np.concatenate([rows["active"][:n, :, 0], rows["pokemon"][:n, :, 0]], axis=2).astype(np.float64)
    hp = rows["hp"][:n].astype(np.float64)
    ep = act(f64(onet.p1, act(f64(onet.p0, xp)))) * (hp[:, :, 1:] != 0)
    ea = act(f64(onet.a1, act(f64(onet.a0, xa)))) * (hp[:, :, 0] != 0)
    sides = np.concatenate([hp[:, :, 0], ea, np.concatenate([hp[:, :, 1:], ep], axis=3).reshape(n, 2, -1)], axis=2)
    h = act(f64(onet.v2, act(f64(onet.fc1, act(f64(onet.fc0, sides.reshape(n, -1)))))))
    value = 1.0 / (1.0 + np.exp(-f64(onet.v3, h)[:, 0]))
    got = TR.Ref(_net("default")).run(rows, n, LOSS)
    assert got["rows"] == n
    assert np.abs(got["value"] - value).max() <= 1e-12


def test_row_terms_are_the_corpus_evaluation_s():
    """Per-row sq_err and ce against corpus_eval_ref.row_terms fed the referee's value and logits.  row_terms rounds what it is handed to
    fp32 (the evaluator's outputs are fp32), so the two agree to that rounding: 2^-24 relative on the value and on each logit moves sq_err
    by at most 2^-24 * 2 |d| <= 2^-23 and a log-probability by at most 2 * 2^-24 * max |logit|, hence ce by that (sum t <= 1)."""
    rows = TR.host_rows()
    n = 120
    got = TR.Ref(_net("tiny")).run(rows, n, LOSS)
    for i in range(n):
        m, k = int(rows["k"][i, 0, 0]), int(rows["k"][i, 1, 0])
        tg = {"m": m, "n": k, "nash_value": rows["nash_value"][i, 0], "empirical_value": rows["empirical_value"][i, 0],
              "emp": rows["empirical_policies"][i], "nash": rows["nash_policies"][i]}
        exp = CE.row_terms(F(got["value"][i]), got["logits"][i].astype(F), tg, float(rows["score"][i, 0]), LOSS[:4])
        scale = max(1.0, float(np.abs(got["logits"][i]).max()))
        assert abs(got["sq_err"][i] - exp["sq_err"]) <= 2.0 ** -23
        assert np.abs(got["ce"][i] - exp["ce"]).max() <= 2.0 ** -23 * scale


def test_rows_that_are_not_ok_count_for_nothing():
    rows = TR.make_batch(TR.host_rows())
    n = 64
    bad = np.nonzero(rows["status"][:n] != 0)[0]
    assert len(bad) >= 1
    nan, zero = TR.spoil(rows, np.concatenate([bad, [7, 20]]))
    a, b = TR.Ref(_net("tiny")), TR.Ref(_net("tiny"))
    ra, rb = a.run(nan, n, LOSS), b.run(zero, n, LOSS)
    assert ra["rows"] == n - len(bad) - 2 and ra["loss"] == rb["loss"] and np.isfinite(ra["loss"])
    for (ba, wa), (bb, wb) in zip(a.backward()[0], b.backward()[0]):
        assert (ba == bb).all() and (wa == wb).all()
    assert (ra["value"][bad] == 0).all() and (ra["ce"][bad] == 0).all()


def test_adam_by_formula_is_torch_optim_adam():
    """float64 both, the same formula: five steps agree to 1e-12 relative (operation order alone differs)."""
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(500)
    grads = [rng.standard_normal(500) * 10.0 ** rng.integers(-6, 3, 500) for _ in range(5)]
    tp = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([tp], lr=3e-3)
    p, m, v = p0.copy(), np.zeros(500), np.zeros(500)
    for t, g in enumerate(grads, 1):
        tp.grad = torch.tensor(g)
        opt.step()
        p, m, v, _ = TR.adam_formula(p, g, m, v, t, 3e-3, float_scalars=False)
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-12 * np.abs(p).max()
    st = opt.state[tp]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-12 * np.abs(m).max()
    assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-12 * np.abs(v).max()


def test_adam_clamp_and_zero_state():
    p = np.array([1.9999, -1.9999, 0.5, 3.0])
    g = np.array([-1.0, 1.0, 0.0, 0.0])
    q, m, v, u = TR.adam_formula(p, g, np.zeros(4), np.zeros(4), 1, 1e-2, clamp=np.array([True, True, True, False]))
    assert q[0] == 2.0 and q[1] == -2.0 and q[2] == 0.5 and q[3] == 3.0 and u[2] == 0.0 and m[2] == 0.0 and v[2] == 0.0


@pytest.mark.parametrize("dead, loss", [(1, (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)), (2, (0.0, 0.0, 1.0, 0.0, 1.0, 0.0))])
def test_group_rule(dead, loss):
    """A zero loss weight: the referee hands out no gradient for that head's group (autograd's are exactly zero there), and the trunk's
    gradient is the other head's alone."""
    rows = TR.host_rows()
    ref = TR.Ref(_net("tiny"))
    ref.run(rows, 40, loss)
    grads, S = ref.backward()
    for name, g in zip(TR.LAYERS, grads):
        if TR.GROUP[name] == dead:
            assert g is None
            assert float(getattr(ref, name + "_w").grad.abs().max()) == 0.0
        else:
            assert g is not None and np.abs(g[1]).max() > 0


def test_planted_mistakes_break_the_gradient_bound():
    """Each planted mistake must leave the GPU tests' gradient bound (per tensor: 4 x the fp32 referee's distance from float64 + 2e-7 S) on
    their inputs -- here without the self-play record, which needs a GPU to make.  Measured, in bounds of the worst tensor (tiny, 257 rows):
    nomask 4.2e+05, k 5.7e+05, mean_n 1.1e+04, swap 6.5e+05, bf16 1.4e+03."""
    rows = TR.make_batch(TR.host_rows())
    n = 257
    data = _net("tiny")
    r64, r32 = TR.Ref(data), TR.Ref(data, torch.float32)
    r64.run(rows, n, LOSS)
    r32.run(rows, n, LOSS)
    (g64, S), (g32, _) = r64.backward(), r32.backward()
    bounds = [[TR.gradient_bound(g32[i][j], g64[i][j], S[i][j]) for j in range(2)] for i in range(12)]
    assert all(b > 0 for pair in bounds for b in pair)
    for variant in TR.VARIANTS:
        bad = TR.Ref(data, variant=variant)
        bad.run(rows, n, LOSS)
        g, _ = bad.backward()
        worst = max(float(np.abs(g[i][j] - g64[i][j]).max()) / bounds[i][j] for i in range(12) for j in range(2))
        print("planted %-7s: %.3g bounds" % (variant, worst))
        assert worst > 10.0, (variant, worst)


def test_untouched_policy_rows_have_exactly_zero_gradient():
    rows = TR.make_batch(TR.host_rows())
    n = 33
    ref = TR.Ref(_net("tiny"))
    ref.run(rows, n, LOSS)
    grads, _ = ref.backward()
    ok = rows["status"][:n] == 0
    for s, layer in enumerate((9, 11)):
        named = np.zeros(315, bool)
        for i in np.nonzero(ok)[0]:
            named[rows["choice_indices"][i, s, :int(rows["k"][i, s, 0])]] = True
        assert named.any() and not named.all()
        assert (grads[layer][0][~named] == 0).all() and (grads[layer][1][~named] == 0).all()


def test_symmetries_restated():
    """Every flip is an involution on the row (bit for bit: the inputs are u16 / 65535 quotients and scores, 1 - (1 - x) == x for all of them
    that the rows hold is checked, not assumed), the bench permutation is a permutation of the slots 1 .. 5 that leaves slot 0 alone, applying
    it and then its inverse gives the row back, hp moves with its Pokemon, and both kinds of draw occur."""
    rows = TR.make_batch(TR.host_rows())
    n = 80
    flips, perms = set(), set()
    for i in range(n):
        flip, src = TR.symmetry_draws(1234, i)
        assert src[0] == 0 and sorted(src[1:]) == [1, 2, 3, 4, 5]
        flips.add(flip)
        perms.add(tuple(src))
    assert flips == {0, 1} and len(perms) > 20
    ident = list(range(6))
    once = TR.symmetric(rows, n, 0, forced=(1, ident))
    twice = TR.symmetric(once, n, 0, forced=(1, ident))
    exact = np.array([F(1.0) - (F(1.0) - rows[name][:n]) == rows[name][:n] for name in TR.VALUE_FIELDS]).all(axis=(0, 2))
    assert exact.sum() >= n // 2
    for name in rows:
        a, b = twice[name], rows[name][:n]
        keep = np.ones(n, bool) if name not in TR.VALUE_FIELDS else exact
        assert a[keep].tobytes() == b[keep].tobytes(), name
    assert (once["k"][:, 0] == rows["k"][:n, 1]).all() and (once["pokemon"][:, 1] == rows["pokemon"][:n, 0]).all()
    src = [0, 3, 1, 5, 2, 4]
    inv = [src.index(s) for s in range(6)]
    there = TR.symmetric(rows, n, 0, forced=(0, src))
    back = TR.symmetric(there, n, 0, forced=(0, inv))
    for name in rows:
        assert back[name].tobytes() == rows[name][:n].tobytes(), name
    assert (there["hp"][:, :, 1] == rows["hp"][:n, :, 3]).all() and (there["pokemon"][:, :, 1] == rows["pokemon"][:n, :, 3]).all()
    assert there["active"].tobytes() == rows["active"][:n].tobytes()
    bad = np.nonzero(rows["status"][:n] != 0)[0]
    drawn = TR.symmetric(rows, n, 99)
    assert len(bad) and all((drawn[name][bad] == rows[name][bad]).all() for name in rows)


def test_host_check_names_every_refusal(tmp_path):
    """oakgpu_trainer_check, host only: widths over the loader's limits, a truncated file, n > max_rows, both weights zero."""
    good = _net("tiny")
    trainer_check(good, 64, 64, train_loss())
    cases = [(dict(pokemon_hidden=129), "embedding widths above 128"), (dict(active_out=129), "embedding widths above 128"),
             (dict(hidden=257, value_hidden=32), "main-net widths above 256"), (dict(value_hidden=257), "main-net widths above 256"),
             (dict(policy_hidden=257), "policy hidden width above 256")]
    for dims, text in cases:
        path = str(tmp_path / "wide.battle.net")
        netfile.write_random_net(path, **dims)
        with pytest.raises(_lib.OakGpuError, match=text):
            trainer_check(open(path, "rb").read(), 64)
    with pytest.raises(_lib.OakGpuError, match="truncated inside p2_policy_fc3"):
        trainer_check(good[:-4], 64)
    with pytest.raises(_lib.OakGpuError, match="truncated header"):
        trainer_check(good[:5], 64)
    with pytest.raises(_lib.OakGpuError, match="trailing bytes"):
        trainer_check(good + b"\0\0\0\0", 64)
    with pytest.raises(_lib.OakGpuError, match="n = 65 rows exceed max_rows = 64"):
        trainer_check(good, 64, 65)
    with pytest.raises(_lib.OakGpuError, match="both zero"):
        trainer_check(good, 64, 1, train_loss(value_weight=0.0, policy_weight=0.0))
    with pytest.raises(_lib.OakGpuError, match="max_rows must be"):
        trainer_check(good, 0)
    ragged = str(tmp_path / "ragged.battle.net")
    netfile.write_random_net(ragged, activation=2, **TR.RAGGED)
    trainer_check(open(ragged, "rb").read(), 257, 257, train_loss())
