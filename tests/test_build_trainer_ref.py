"""CPU: the referee of the build trainer (tests/build_trainer_ref.py) and the inputs of tests/test_gpu_build_trainer.py, checked without a GPU --
the contract's closed-form gradient equals the referee's autograd; each planted mistake lands outside the bound; the census of the inputs;
oakgpu_build_trainer_check's refusals; oak_amd/csrc/build_loss.hpp in a stand-alone program under the sanitizers."""
import numpy as np
import pytest
import torch

import build_traj_ref as T
import build_trainer_ref as R
import trainer_ref as TR
from oak_amd import _lib, build

F = np.float32
NETS = {"h128": ((128, 128, 128), 2), "ragged": ((33, 5, 7), 2), "h256": ((256, 256, 256), 1), "one": ((1, 1, 1), 2)}   # as tests/test_gpu_build_trainer.py
TOTAL = 3000
_CACHE = {}


def _chunk(n):
    if n not in _CACHE:
        _CACHE[n] = R.chunk(R.test_records()[:n])
    return _CACHE[n]


def _keep(v):
    keep = np.random.default_rng(3).random(v) < 0.8
    return keep, int(keep.sum()) - v // 10


def _run(n, net, keep, remaining, dtype=torch.float64, mistake=None, hyper=R.HYPER, shift=0.0):
    widths, seed = NETS[net]
    traj, tg = _chunk(n)
    ref = R.Ref(R.make_net(seed, *widths, shift=shift), dtype, mistake)
    out = ref.run(traj, tg, keep, TOTAL, remaining, hyper)
    grads, S = ref.backward()
    return ref, out, grads, S


def _record(mistake, tensor, distance):
    """With OAK_BUILD_TRAINER_MISTAKES=path the distances of the planted mistakes are kept there as JSON (profiles/r29_build_trainer_mistakes.json)."""
    import json
    import os
    path = os.environ.get("OAK_BUILD_TRAINER_MISTAKES")
    if not path:
        return
    held = json.load(open(path)) if os.path.exists(path) else {"unit": "the farthest gradient tensor's distance from the float64 referee, in bounds of that tensor", "mistakes": {}}
    held["mistakes"][mistake] = {"tensor": tensor, "bounds_away": float("%.4g" % distance)}
    with open(path, "w") as f:
        json.dump(held, f, indent=1, sort_keys=True)


def test_closed_form_gradient_equals_autograd():
    """G -> A -> D -> d value_full and the dz formula of the contract against the referee's autograd in float64, to 1e-12 relative."""
    n = 65
    traj, tg = _chunk(n)
    keep, remaining = _keep(len(tg["rows"]))
    ref, out, _, _ = _run(n, "ragged", keep, remaining)
    dval, dz = R.closed_form(out, tg, traj, out["selected"], TOTAL)
    auto_val = ref.tensors["value"].grad.numpy().reshape(-1)
    auto_z = np.where(ref.tensors["valid_mask"] >= 0, ref.tensors["mask_logits"].grad.numpy(), 0.0)
    assert np.abs(auto_val).max() > 0 and np.abs(auto_z).max() > 0
    assert np.abs(dval - auto_val).max() <= 1e-12 * np.abs(auto_val).max()
    assert np.abs(dz - auto_z).max() <= 1e-12 * np.abs(auto_z).max()
    unselected = ~out["selected"]
    assert unselected.any() and np.abs(auto_val[unselected]).max() > 0 and not auto_z[unselected].any()   # value gradient reaches unselected rows


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistakes_land_outside_the_bound(mistake):
    """The referee with one deliberate error against the referee, in units of the bound the device is held to: each is more than a
    thousand bounds away on some tensor (the figures: profiles/r29_build_trainer_mistakes.json)."""
    n = 65
    keep, remaining = _keep(len(_chunk(n)[1]["rows"]))
    hyper, shift = R.HYPER, 0.0
    if mistake == "max_subtracted":   # it shows only where normalize's eps is the denominator: every logit near -40, the entropy term alone
        hyper, shift = dict(R.HYPER, policy_loss_weight=0.0, value_loss_weight=0.0, entropy_loss_weight=1.0), -40.0
    _, out64, g64, S = _run(n, "ragged", keep, remaining, hyper=hyper, shift=shift)
    _, _, g32, _ = _run(n, "ragged", keep, remaining, torch.float32, hyper=hyper, shift=shift)
    _, _, bad, _ = _run(n, "ragged", keep, remaining, mistake=mistake, hyper=hyper, shift=shift)
    if mistake == "max_subtracted":
        assert np.nansum(np.exp(out64["logits"]), axis=1).max() < 1e-12
    far = {}
    for name in R.NAMES:
        bound = TR.gradient_bound(g32[name], g64[name], S[name])
        if bound > 0:
            far[name] = float(np.abs(bad[name] - g64[name]).max() / bound)
    worst = max(far, key=far.get)
    print("%s: %s is %.3g bounds away" % (mistake, worst, far[worst]))
    _record(mistake, worst, far[worst])
    assert far[worst] > 1000.0, far


def test_census_of_the_inputs():
    """Conditions on the inputs of the GPU tests, not tolerances: fp32 and fp64 must take the same branches, and every path must be walked."""
    traj, tg = _chunk(257)
    v = len(tg["rows"])
    for net in NETS:
        _, out, grads, _ = _run(257, net, None, TOTAL)
        z, z0 = out["logits"], out["logits"][:, 0]
        assert (z0 > 2).mean() >= 0.1 and (z0 < -2).mean() >= 0.1 and (np.abs(z0) < 2).mean() >= 0.1, net
        assert np.abs(np.abs(z0) - 2).min() >= 1e-3 and np.abs(out["gae"]).min() >= 1e-6 and np.nanmax(np.abs(z)) <= 10, net
        assert all(np.abs(grads[name]).max() > 0 for name in R.NAMES), net
    cells = tg["state_cells"]
    in_states = np.bincount(cells[cells < R.N_DIM].astype(np.int64), minlength=R.N_DIM)
    rows = tg["rows"].astype(np.int64)
    lists = traj["mask"][rows[:, 0], rows[:, 1]]
    in_lists = np.bincount(lists[lists >= 0].astype(np.int64), minlength=R.N_DIM)
    for count in (in_states, in_lists):
        assert count.max() > 2 * build.TRAINER_SEGMENT and (count == 1).any() and (count == 0).any()
    valid = tg["valid"]
    assert any(valid[b].any() and not valid[b, np.flatnonzero(valid[b])[0]:np.flatnonzero(valid[b])[-1] + 1].all() for b in range(len(valid)))
    status = T.status_of(R.test_records())
    assert set(status.tolist()) == set(range(T.N_STATUS)) and not valid[status != T.OK].any()
    assert v > 3000 and (traj["n_legal"][valid] == 1).any() and traj["n_legal"].max() > 256


def test_check_refuses_by_name():
    good = R.make_net(1, 8, 4, 6)
    build.check_trainer(good, 1)
    build.check_trainer(R.make_net(1, 33, 5, 7), 32768)
    layers = R.read_net(good)
    nan = [(b.copy(), w.copy()) for b, w in layers]
    nan[4][1][0, 0] = np.nan
    wide = [(b, w) for b, w in R.read_net(R.make_net(1, 8, 8, 8))]
    wide[0] = (np.zeros(300, F), np.zeros((300, R.N_DIM), F))
    wide[1] = (np.zeros(300, F), np.zeros((300, 300), F))
    wide[2] = (wide[2][0], np.zeros((R.N_DIM, 300), F))
    cases = [(b"", 1, "null bytes"), (good[:-4], 1, "truncated file"), (good + b"\0\0\0\0", 1, "trailing bytes"), (R.net_bytes(nan), 1, "NaN parameter"),
             (R.net_bytes(wide), 1, "policy hidden width above 256"), (R.make_net(1, 8, 257, 6), 1, "value hidden width above 256"),
             (R.make_net(1, 8, 6, 257), 1, "value hidden width above 256"), (good, 0, "max_traj must be in"), (good, 32769, "max_traj must be in")]
    for data, max_traj, text in cases:
        with pytest.raises(_lib.OakGpuError, match=text):
            build.check_trainer(data, max_traj)


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitizers"))
def test_build_loss_header_on_the_host(tmp_path, flags):
    """oak_amd/csrc/build_loss.hpp in a stand-alone program (a child process; nothing loaded into Python runs under a sanitizer): its
    recursions on 200 trajectories, fed the float32 referee's values, equal that referee's gae / returns / clipped force within the bound
    of a forward output, and its adjoint equals the closed form in float64 to the roundings counted (two per step, 31 steps)."""
    n = 200
    traj, tg = _chunk(n)
    _, o64, _, _ = _run(n, "h128", None, TOTAL)
    _, o32, _, _ = _run(n, "h128", None, TOTAL, torch.float32)
    rows, valid = tg["rows"].astype(np.int64), tg["valid"]
    at = (rows[:, 0], rows[:, 1])

    def full(x):
        a = np.zeros((n, R.STEPS), F)
        a[at] = x
        return a
    G = full(np.random.default_rng(4).standard_normal(len(rows)) * (np.random.default_rng(5).random(len(rows)) < 0.7))
    gamma, gl = R.HYPER["gamma"], R.HYPER["gamma"] * R.HYPER["lam"]
    exe = R.loss_check_program(tmp_path, flags)
    gae, ret, dvf, cf = R.loss_check(exe, tmp_path, gamma, gl, full(o32["value"]), tg["rewards"], valid, G, full(o32["logits"][:, 0]))
    for name, got in (("gae", gae[at]), ("returns", ret[at]), ("forced", (o32["logits"][:, 0] * cf[at].astype(np.float64)))):
        err = np.abs(got.astype(np.float64) - o64[name]).max()
        bound = 4.0 * np.abs(o32[name] - o64[name]).max() + 2e-7 * max(1.0, np.abs(o64[name]).max())
        print("%s: err %.3e bound %.3e" % (name, err, bound))
        assert err <= bound, name
    assert not gae[~valid & (np.arange(R.STEPS)[None, :] >= traj["end"][:, None])].any()     # steps past the end contribute 0
    g64, fgl, fg = G.astype(np.float64), float(F(gl)), float(F(gamma))
    A = np.zeros((n, R.STEPS))
    for t in range(R.STEPS):
        A[:, t] = g64[:, t] + (fgl * A[:, t - 1] if t else 0.0)
    D = valid * A
    want = -D
    want[:, 1:] += fg * D[:, :-1]
    assert np.abs(want).max() > 0 and np.abs(dvf - want).max() <= 64 * 2.0 ** -24 * np.abs(A).max()
