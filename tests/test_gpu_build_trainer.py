"""GPU: oak_amd.build.Trainer (oak_amd/csrc/buildtrain.hip) against the torch referee of tests/build_trainer_ref.py -- build.py's
process_targets / compute_loss_from_targets on dense states with autograd, float64 as the referee and float32 to size the bounds.

The bound of a gradient tensor is the project's own (trainer_ref.gradient_bound): max |dev - g64| <= 4 max |g32 - g64| + 2e-7 S, S the largest
per-entry sum |dZ| |X|.  A forward output is held to the same form, with S from build_trainer_ref.forward_scale.  The conditions on the
inputs (no logit next to the force's thresholds, segments of the inverted indices longer than two pieces, ...) are asserted on the CPU in
tests/test_build_trainer_ref.py.  With OAK_BUILD_TRAINER_ACCURACY=path the measured shares of the bounds are written there as JSON."""
import atexit
import json
import os

import numpy as np
import pytest
import torch

import build_ref as B
import build_trainer_ref as R
import trainer_ref as TR
from oak_amd import build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NETS = {"h128": ((128, 128, 128), 2), "ragged": ((33, 5, 7), 2), "h256": ((256, 256, 256), 1), "one": ((1, 1, 1), 2)}   # widths, seed (the census holds)
CASES = [(1, "h128", "int64"), (2, "h128", "int16"), (63, "h128", "int64"), (64, "h128", "int16"), (65, "h128", "int64"), (257, "h128", "int16"),
         (65, "ragged", "int16"), (257, "ragged", "int64"), (65, "h256", "int64"), (65, "one", "int16"), (257, "one", "int64")]
TOTAL = 3000          # the batch size of the loss: any number, the same on both sides
_CACHE, _SHARES = {}, {}


@atexit.register
def _write_shares():
    path = os.environ.get("OAK_BUILD_TRAINER_ACCURACY")
    if path and _SHARES:
        with open(path, "w") as f:
            json.dump({"bound": "max|dev - f64| <= 4 max|f32 - f64| + 2e-7 S; the figures are the largest measured share of it", "shares": _SHARES}, f, indent=1, sort_keys=True)


def _net(name):
    if ("net", name) not in _CACHE:
        widths, seed = NETS[name]
        _CACHE["net", name] = R.make_net(seed, *widths)
    return _CACHE["net", name]


def _records():
    if "records" not in _CACHE:
        _CACHE["records"] = R.test_records()
    return _CACHE["records"]


def _host(lo, hi):
    """(traj, targets) of records lo .. hi-1 by the numpy referee of the reader; computed once, left unchanged."""
    if ("host", lo, hi) not in _CACHE:
        _CACHE["host", lo, hi] = R.chunk(_records()[lo:hi])
    return _CACHE["host", lo, hi]


def _device(ctx, lo, hi, mask_dtype):
    if ("dev", lo, hi, mask_dtype) not in _CACHE:
        if "corpus" not in _CACHE:
            _CACHE["corpus"] = build.TrajectoryCorpus(ctx, _records().tobytes())
        traj = _CACHE["corpus"].decode(torch.arange(lo, hi, dtype=torch.int32, device="cuda"), mask_dtype=mask_dtype, no_score=True)
        _CACHE["dev", lo, hi, mask_dtype] = (traj, build.targets(ctx, traj, 0.7))
    return _CACHE["dev", lo, hi, mask_dtype]


def _keep(v, seed=3):
    """(keep, remaining): a random mask of about 0.8 and a cap below its count, so that the [:n] slice cuts."""
    keep = np.random.default_rng(seed).random(v) < 0.8
    if v < 4:
        keep[:] = True
    return keep, max(1, int(keep.sum()) - max(1, v // 10))


def _referee(lo, hi, net, keep, remaining, hyper=R.HYPER, total=TOTAL):
    key = ("ref", lo, hi, net, None if keep is None else keep.tobytes(), remaining, tuple(sorted(hyper.items())), total)
    if key not in _CACHE:
        traj, tg = _host(lo, hi)
        res = {}
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            ref = R.Ref(_net(net), dt)
            res["out" + tag] = ref.run(traj, tg, keep, total, remaining, hyper)
            res["g" + tag], res["S" + tag] = ref.backward()
        res["scale"] = R.forward_scale(_net(net), res["out64"], traj, tg)
        _CACHE[key] = res
    return _CACHE[key]


def _share(tag, name, value):
    _SHARES.setdefault(tag, {})[name] = max(_SHARES.get(tag, {}).get(name, 0.0), float(value))


def _guarded(v, guard=64):
    """Forward outputs inside NaN / 0xAA prefilled buffers with guard bands: (out, check)."""
    out, whole = {}, {}
    for name, width in (("logits", R.MAX_ACTIONS), ("value", 1), ("logp", 1), ("gae", 1), ("returns", 1), ("forced", 1), ("du", 1)):
        whole[name] = torch.full((v * width + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
        out[name] = whole[name][guard:guard + v * width].view((v, width) if width > 1 else (v,))
    whole["selected"] = torch.full((v + 2 * guard,), 0xAA, dtype=torch.uint8, device="cuda")
    out["selected"] = whole["selected"][guard:guard + v]

    def check():
        for name, w in whole.items():
            band = torch.cat([w[:guard], w[-guard:]])
            assert bool(torch.isnan(band).all()) if name != "selected" else bool((band == 0xAA).all()), name
    return out, check


def _kw(keep, remaining, hyper=R.HYPER, total=TOTAL):
    kw = dict(hyper, total=total, remaining=remaining)
    kw["keep"] = None if keep is None else torch.from_numpy(keep).cuda()
    return kw


def _check_forward(tag, got, ref, n_legal):
    o64, o32, scale = ref["out64"], ref["out32"], ref["scale"]
    for name in ("logits", "value", "logp", "gae", "returns", "forced"):
        dev = got[name].cpu().numpy().astype(np.float64)
        if name == "logits":
            pad = np.arange(R.MAX_ACTIONS)[None, :] >= n_legal[:, None]
            assert np.array_equal(np.isnan(dev), pad) and np.array_equal(np.isnan(o64[name]), pad)
        else:
            assert np.isfinite(dev).all(), name
        err = np.nanmax(np.abs(dev - o64[name]))
        bound = 4.0 * np.nanmax(np.abs(o32[name] - o64[name])) + 2e-7 * scale[name]
        print("%s forward %-8s err %.3e bound %.3e" % (tag, name, err, bound))
        _share(tag, "forward." + name, err / bound)
        assert err <= bound, (name, err, bound)
    assert np.array_equal(got["selected"].cpu().numpy().astype(bool), o64["selected"])


def _check_gradients(tag, got, ref):
    for name in R.NAMES:
        err = float(np.abs(got[name].astype(np.float64) - ref["g64"][name]).max())
        bound = TR.gradient_bound(ref["g32"][name], ref["g64"][name], ref["S64"][name])
        print("%s gradient %-18s err %.3e bound %.3e" % (tag, name, err, bound))
        if bound > 0:
            _share(tag, "gradient." + name, err / bound)
        assert err <= bound, (name, err, bound)


def _unreached(host, selected):
    """(cells in no valid row's state, cells in no selected row's list) as boolean [3749]."""
    traj, tg = host
    in_state, in_list = np.zeros(R.N_DIM, bool), np.zeros(R.N_DIM, bool)
    cells = tg["state_cells"]
    in_state[cells[cells < R.N_DIM].astype(np.int64)] = True
    rows = tg["rows"].astype(np.int64)[selected]
    lists = np.asarray(traj["mask"])[rows[:, 0], rows[:, 1]]
    in_list[lists[lists >= 0].astype(np.int64)] = True
    return ~in_state, ~in_list


@pytest.mark.parametrize("n, net, mask_dtype", CASES)
def test_forward_and_gradients(gpu_ctx, n, net, mask_dtype):
    """Every forward output of every valid row and every entry of the twelve gradient tensors inside the bound; selection exact; entries
    that no row reaches exactly 0 after set_gradients(NaN) + zero_gradients."""
    host, (traj, tg) = _host(0, n), _device(gpu_ctx, 0, n, mask_dtype)
    v = tg["n_valid"]
    assert v == len(host[1]["rows"]) > 0
    keep, remaining = _keep(v)
    ref = _referee(0, n, net, keep, remaining)
    tag = "%s/n%d/%s" % (net, n, mask_dtype)
    n_legal = host[0]["n_legal"][host[1]["valid"]].astype(np.int64)
    with build.Trainer(gpu_ctx, _net(net), max(n, 2)) as tr:
        out, check = _guarded(v)
        tr.forward(traj, tg, out=out, **_kw(keep, remaining))
        check()
        _check_forward(tag, out, ref, n_legal)
        tr.set_gradients(np.nan)
        assert all(np.isnan(x).all() for x in tr.read("gradients").values())
        tr.zero_gradients()
        tr.accumulate(traj, tg, **_kw(keep, remaining))
        got = tr.read("gradients")
        _check_gradients(tag, got, ref)
        no_state, no_list = _unreached(host, ref["out64"]["selected"])
        assert no_state.any() and no_list.any()
        for k in ("policy", "value"):
            assert not got[k + ".fc1.weight"][:, no_state].any()
        assert not got["policy.fc3.weight"][no_list].any() and not got["policy.fc3.bias"][no_list].any()
        rep = tr.report()
        assert (rep["rows"], rep["kept"], rep["n_cap"]) == (v, ref["out64"]["kept"], ref["out64"]["n_cap"])
        assert abs(rep["loss"] - ref["out64"]["loss"]) <= 1e-5 * max(1.0, abs(ref["out64"]["loss"]))


def test_selection_is_the_rank_rule(gpu_ctx):
    """keep null, all zero (k = 0: nothing changes), random with remaining < k and with remaining >= k: `selected` exactly."""
    n = 65
    traj, tg = _device(gpu_ctx, 0, n, "int16")
    v = tg["n_valid"]
    rnd = np.random.default_rng(8).random(v) < 0.5
    with build.Trainer(gpu_ctx, _net("ragged"), n) as tr:
        for keep, remaining in ((None, v + 10), (None, v // 3), (np.zeros(v, bool), 100), (rnd, int(rnd.sum()) - 7), (rnd, int(rnd.sum())), (rnd, int(rnd.sum()) + 7)):
            want, k, n_cap = R.selected_rule(keep, v, remaining)
            got = tr.forward(traj, tg, **_kw(keep, remaining))["selected"].cpu().numpy().astype(bool)
            assert np.array_equal(got, want)
            rep = tr.report()
            assert (rep["rows"], rep["kept"], rep["n_cap"]) == (v, k, n_cap)
        tr.set_gradients(F(0.25))
        tr.accumulate(traj, tg, **_kw(np.zeros(v, bool), 100))
        assert all((x == F(0.25)).all() for x in tr.read("gradients").values())


def test_recursions_equal_the_header_on_the_host(gpu_ctx, tmp_path):
    """gae / returns / forced / du of the device equal build_loss.hpp's host bits when fed the device's own value_full, logits and
    selection: G is rebuilt on the host in float with k_traj's expression, the header's adjoint runs on it in a child process, and the
    sigmoid's factor is applied in float.  The chunk holds trajectories with an invalid step between valid ones."""
    n = 257
    host, (traj, tg) = _host(0, n), _device(gpu_ctx, 0, n, "int16")
    keep, remaining = _keep(tg["n_valid"])
    with build.Trainer(gpu_ctx, _net("h128"), n) as tr:
        out = {k: x.cpu().numpy() for k, x in tr.forward(traj, tg, **_kw(keep, remaining)).items()}
    rows, valid = host[1]["rows"].astype(np.int64), host[1]["valid"]
    at = (rows[:, 0], rows[:, 1])

    def full(x):
        a = np.zeros((n, R.STEPS), F)
        a[at] = x
        return a
    selected = out["selected"].astype(bool)
    assert selected.any() and not selected.all()
    coef = (F(2.0) * (F(1.0) / F(TOTAL))) * F(R.HYPER["value_loss_weight"])
    G = np.where(selected, coef * (out["returns"] - out["value"]), F(0.0)).astype(F)
    exe = R.loss_check_program(tmp_path)
    gae, ret, dvf, cf = R.loss_check(exe, tmp_path, R.HYPER["gamma"], R.HYPER["gamma"] * R.HYPER["lam"], full(out["value"]), host[1]["rewards"], valid,
                                     full(G), full(out["logits"][:, 0]))
    assert out["gae"].tobytes() == gae[at].tobytes() and out["returns"].tobytes() == ret[at].tobytes()
    assert out["forced"].tobytes() == (out["logits"][:, 0] * cf[at]).astype(F).tobytes()
    du = dvf[at] * (out["value"] * (F(1.0) - out["value"]))
    assert du.dtype == F and np.abs(du).max() > 0 and np.abs(du[~selected]).max() > 0          # unselected rows receive value gradient
    assert out["du"].tobytes() == du.tobytes()
    gapped = [b for b in range(n) if valid[b].any() and not valid[b, np.flatnonzero(valid[b])[0]:np.flatnonzero(valid[b])[-1] + 1].all()]
    assert gapped and np.abs(du[np.isin(rows[:, 0], gapped)]).max() > 0


def test_two_chunks_accumulate_to_the_rounded_sum(gpu_ctx):
    a, b = _device(gpu_ctx, 0, 65, "int64"), _device(gpu_ctx, 65, 130, "int64")
    with build.Trainer(gpu_ctx, _net("ragged"), 65) as tr:
        singles = []
        for traj, tg in (a, b):
            tr.zero_gradients()
            tr.accumulate(traj, tg, **_kw(None, TOTAL))
            singles.append(tr.read("gradients"))
        tr.zero_gradients()
        for traj, tg in (a, b):
            tr.accumulate(traj, tg, **_kw(None, TOTAL))
        both = tr.read("gradients")
    for name in R.NAMES:
        assert np.abs(singles[0][name]).max() > 0 and both[name].tobytes() == (singles[0][name] + singles[1][name]).astype(F).tobytes(), name


@pytest.mark.parametrize("zero", ("policy_loss_weight", "value_loss_weight", "entropy_loss_weight", "policy_and_entropy"))
def test_one_weight_zero(gpu_ctx, zero):
    n = 65
    traj, tg = _device(gpu_ctx, 0, n, "int16")
    keep, remaining = _keep(tg["n_valid"])
    hyper = dict(R.HYPER)
    for name in (("policy_loss_weight", "entropy_loss_weight") if zero == "policy_and_entropy" else (zero,)):
        hyper[name] = 0.0
    ref = _referee(0, n, "ragged", keep, remaining, hyper)
    with build.Trainer(gpu_ctx, _net("ragged"), n) as tr:
        tr.accumulate(traj, tg, **_kw(keep, remaining, hyper))
        got = tr.read("gradients")
    _check_gradients("zero/" + zero, got, ref)
    dead = "value" if zero == "value_loss_weight" else "policy" if zero == "policy_and_entropy" else None
    for name in R.NAMES:
        if dead and name.startswith(dead):
            assert not got[name].any() and not ref["g64"][name].any(), name
        else:
            assert np.abs(ref["g64"][name]).max() > 0, name


PLANTED = np.array([0.0, 1e-20, -1e-20, 1e-12, -1e-12, 1.0, -1.0, 1e4, -1e4], F)


def test_adam_alone(gpu_ctx):
    """Five updates from one planted gradient block against the float64 formula fed the same fp32 gradients and host scalars; the bound is
    the one counted for k_adam in tests/test_gpu_trainer.py: after step t, sum over s <= t of ulp(p_s) / 2 + |update_s| (6.5 s + 6) 2^-24."""
    with build.Trainer(gpu_ctx, _net("ragged"), 1) as tr:
        flat = lambda which: np.concatenate([x.reshape(-1) for x in tr.read(which).values()])
        g = PLANTED[np.arange(tr.count) % len(PLANTED)]
        p0 = flat("parameters")
        p, m, v, allowed, worst = p0.astype(np.float64), np.zeros(tr.count), np.zeros(tr.count), np.zeros(tr.count), 0.0
        for t in range(1, 6):
            tr.set_gradients(g)
            tr.adam(1e-3)
            before = p
            p, m, v, upd = TR.adam_formula(p, g, m, v, t, 1e-3)
            got = flat("parameters")
            ulp = np.spacing(np.maximum(np.abs(before), np.abs(before - upd)).astype(F)).astype(np.float64)
            allowed += ulp / 2 + np.abs(upd) * (6.5 * t + 6) * 2.0 ** -24
            err = np.abs(got.astype(np.float64) - p)
            worst = max(worst, float((err / np.maximum(allowed, 1e-300)).max()))
            assert (err <= allowed).all(), (t, int(np.argmax(err - allowed)))
            assert got[g == 0].tobytes() == p0[g == 0].tobytes()
        _share("adam", "parameters", worst)
        assert tr.report()["steps"] == 5
        assert flat("average").tobytes() == p0.tobytes()


def test_rolling_average(gpu_ctx):
    """avg = avg g + (1 - g) p: two products and a sum, three roundings -- |dev - f64| <= 1.5 ulp of the largest of the three magnitudes,
    plus the two constants g and 1 - g as floats (a relative 2^-24 each)."""
    with build.Trainer(gpu_ctx, _net("ragged"), 1) as tr:
        flat = lambda which: np.concatenate([x.reshape(-1) for x in tr.read(which).values()]).astype(np.float64)
        avg = flat("average")
        for step in range(3):
            tr.set_gradients(PLANTED[np.arange(tr.count) % len(PLANTED)])
            tr.adam(0.01)
            tr.average(0.99)
            p = flat("parameters")
            want = avg * 0.99 + (1 - 0.99) * p
            big = np.maximum(np.abs(avg * 0.99), np.maximum(np.abs(0.01 * p), np.abs(want)))
            allowed = 1.5 * np.spacing(big.astype(F)).astype(np.float64) + 2 * 2.0 ** -24 * big
            got = flat("average")
            assert (np.abs(got - want) <= allowed).all()
            _share("average", "step%d" % step, float((np.abs(got - want) / allowed).max()))
            avg = got
        assert np.abs(flat("average") - flat("parameters")).max() > 0


def test_repeatability_and_no_stale_workspace(gpu_ctx):
    """accumulate + adam on the 257-trajectory chunk (over a hundred blocks of the list index, cells of more than two pieces, passes that
    share a cell) twice from fresh trainers give the same gradients and parameters, bit for bit, also in a trainer with four times the
    capacity; a large call followed by a small one gives the small one's bits."""
    big, small = _device(gpu_ctx, 0, 257, "int16"), _device(gpu_ctx, 0, 2, "int16")
    runs = []
    for order, capacity in (((small,), 257), ((big, small), 257), ((big, small), 257), ((big,), 257), ((big,), 257), ((big,), 1028)):
        with build.Trainer(gpu_ctx, _net("h128"), capacity) as tr:
            for traj, tg in order:
                tr.zero_gradients()
                keep, remaining = _keep(tg["n_valid"])
                tr.accumulate(traj, tg, **_kw(keep, remaining))
            grads = tr.read("gradients")
            tr.adam(1e-3)
            runs.append((grads, tr.net_bytes()))
    for name in R.NAMES:
        assert runs[0][0][name].tobytes() == runs[1][0][name].tobytes() == runs[2][0][name].tobytes(), name
        assert runs[3][0][name].tobytes() == runs[4][0][name].tobytes() == runs[5][0][name].tobytes() != runs[0][0][name].tobytes(), name
    assert runs[0][1] == runs[1][1] == runs[2][1] and runs[3][1] == runs[4][1] == runs[5][1] != runs[0][1]


def test_rows_do_not_depend_on_their_neighbours(gpu_ctx):
    """A trajectory's forward rows are the same bits alone, and among other trajectories."""
    whole_t, whole_g = _device(gpu_ctx, 0, 65, "int64")
    part_t, part_g = _device(gpu_ctx, 40, 65, "int64")
    with build.Trainer(gpu_ctx, _net("ragged"), 65) as tr:
        a = {k: x.cpu().numpy() for k, x in tr.forward(whole_t, whole_g, **_kw(None, TOTAL)).items()}
        b = {k: x.cpu().numpy() for k, x in tr.forward(part_t, part_g, **_kw(None, TOTAL)).items()}
    first = int((whole_g["rows"][:, 0].cpu().numpy() < 40).sum())
    assert part_g["n_valid"] == whole_g["n_valid"] - first > 0
    for name in ("logits", "value", "logp", "gae", "returns", "forced"):
        assert a[name][first:].tobytes() == b[name].tobytes(), name


def test_round_trip_into_the_rollout(gpu_ctx):
    """net_bytes -> oakgpu_build_net_check -> BuildNetwork -> rollout, equal to the rollout of the same parameters written by numpy."""
    traj, tg = _device(gpu_ctx, 0, 65, "int16")
    with build.Trainer(gpu_ctx, _net("ragged"), 65) as tr:
        assert tr.net_bytes() == _net("ragged") == tr.net_bytes("average")
        tr.accumulate(traj, tg, **_kw(None, TOTAL))
        tr.adam(1e-2)
        tr.average(0.9)
        data, avg = tr.net_bytes(), tr.net_bytes("average")
        params = tr.read("parameters")
    assert data != _net("ragged") and avg != data
    build.check_net(data)
    build.check_net(avg)
    by_numpy = R.net_bytes([(params[R.NAMES[2 * k]], params[R.NAMES[2 * k + 1]]) for k in range(6)])
    assert by_numpy == data
    teams = np.array(B.sample_teams(), np.uint8).reshape(-1, 30)[:8]
    teams[:, 5:] = 0
    seeds = np.arange(len(teams), dtype=np.uint64) + np.uint64(11)
    rolls = []
    for blob in (data, by_numpy):
        with build.BuildNetwork(gpu_ctx, blob) as net:
            rolls.append(build.rollout(gpu_ctx, net, teams, seeds))
    assert rolls[0]["n_updates"].sum() > 0
    for name in ("teams_out", "n_updates", "action", "prob"):
        assert np.array_equal(rolls[0][name], rolls[1][name])


def test_the_clamped_denominator(gpu_ctx):
    """Every logit near -40: S < 1e-12, normalize's eps is the denominator, and the log-probability depends on z_0 alone -- the one
    path the census keeps out of the other tests.  The entropy term alone carries the policy's gradient."""
    n, shift = 65, -40.0
    widths, seed = NETS["ragged"]
    net = R.make_net(seed, *widths, shift=shift)
    host, (traj, tg) = _host(0, n), _device(gpu_ctx, 0, n, "int16")
    hyper = dict(R.HYPER, policy_loss_weight=0.0, entropy_loss_weight=1.0)
    keep, remaining = _keep(tg["n_valid"])
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        ref = R.Ref(net, dt)
        res["out" + tag] = ref.run(host[0], host[1], keep, TOTAL, remaining, hyper)
        res["g" + tag], res["S" + tag] = ref.backward()
    res["scale"] = R.forward_scale(net, res["out64"], *host)
    assert np.nansum(np.exp(res["out64"]["logits"]), axis=1).max() < 1e-12 and np.abs(res["g64"]["policy.fc3.bias"]).max() > 0
    n_legal = host[0]["n_legal"][host[1]["valid"]].astype(np.int64)
    with build.Trainer(gpu_ctx, net, n) as tr:
        _check_forward("clamped", tr.forward(traj, tg, **_kw(keep, remaining, hyper)), res, n_legal)
        tr.accumulate(traj, tg, **_kw(keep, remaining, hyper))
        _check_gradients("clamped", tr.read("gradients"), res)


def test_tool_three_steps(gpu_ctx, tmp_path):
    """tools/train_build_net.py: three steps on a `.build.data` made by provide -> records leave initial.build.net and loadable
    3.build.net / 3.avg.build.net, and the tool loads what it wrote."""
    import subprocess
    import sys
    from oak_amd import netfile
    start = str(tmp_path / "start.build.net")
    netfile.write_random_build_net(start, 3, policy_hidden=16, value_hidden=8)
    seeds = np.arange(200, dtype=np.uint64) + np.uint64(7)
    with build.BuildNetwork(gpu_ctx, start) as net:
        rolled = build.provide(gpu_ctx, net, B.sample_teams(), seeds, team_modify_prob=0.9, pokemon_delete_prob=0.3, move_delete_prob=0.3)
    data = build.records(gpu_ctx, rolled, np.linspace(0, 1, len(seeds)).astype(F), 0.5)
    data_dir = tmp_path / "data"
    data_dir.mkdir()
    (data_dir / "0.build.data").write_bytes(data)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_build_net.py"), "--data-dir", str(data_dir), "--batch-size", "600", "--lr", "1e-3",
           "--trajectories-per-step", "64", "--keep-prob", "0.8", "--steps", "3", "--checkpoint", "3", "--seed", "5", "--print-window", "3"]
    out = tmp_path / "run"
    res = subprocess.run(cmd + ["--network-path", start, "--dir", str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    report = json.loads(res.stdout.splitlines()[-1])
    assert report["step"] == 3 and report["steps"] == 3 and report["rows"] > 0 and np.isfinite(report["loss"])
    initial, trained, avg = ((out / name).read_bytes() for name in ("initial.build.net", "3.build.net", "3.avg.build.net"))
    assert initial == open(start, "rb").read() and trained != initial and avg not in (initial, trained)
    for blob in (trained, avg):
        build.check_net(blob)
        build.BuildNetwork(gpu_ctx, blob).close()
    again = subprocess.run(cmd + ["--network-path", str(out / "3.build.net"), "--dir", str(tmp_path / "again"), "--steps", "1", "--checkpoint", "1"],
                           capture_output=True, text=True, timeout=300)
    assert again.returncode == 0, again.stdout + again.stderr
    assert (tmp_path / "again" / "initial.build.net").read_bytes() == trained
