"""GPU: the team-building rollout, provider and records (oak_amd.build, oak_amd/csrc/buildnet.hip) against the referee tests/build_ref.py,
itself held to the reference in tests/test_build_ref.py.

Every traced row is REPLAYED: the referee keeps the team and the input x, and at every step
  * its legal list equals the device's exactly;
  * the device's logits lie within 4 max|l32 - l64| + 2e-7 S of the float64 forward on the x the trajectory implies (the project's
    bound, tests/policy_ref.py: l32 the referee's fp32 forward, S = sum |w||x| + |b| through the layers);
  * the device's policy lies within build_ref.POLICY_BOUND (relative) of the float64 softmax of the device's own logits;
  * index equals EXACTLY the pick rule applied to the device's own policy and the row's stream, prob == policy[index], action == legal[index];
and at the end n_updates, teams_out (the referee applying the traced actions), that the terminal team has no additions left, and that
every cell past the end still holds what the buffers were prefilled with (0xFF bytes / NaN), guard rows around them included.

Row counts 1, 63, 64, 65 and 257 (a row is a block: there is no tile to straddle, the counts are the issue's).  Nets: random with hidden
128, 8 and 7 (layer 3 reads its rows as float4 only when the width is a multiple of 4), all zeros (uniform policies, where the
free-running referee must agree bit for bit), and one built so that the input_update rule changes the outcome.  The worst bound ratios go to the file named by OAKGPU_BUILD_ACCURACY_OUT when it is set."""
import json
import os

import numpy as np
import pytest
import torch

import build_ref as B
from oak_amd import build, netfile

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 63, 64, 65, 257)
_CACHE = {}
WORST = {}


def _net_bytes(tag):
    if tag not in _CACHE:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "t.build.net")
            if tag == "h128":
                netfile.write_random_build_net(path, 1)
            elif tag == "zero":
                netfile.write_random_build_net(path, 2, policy_hidden=16, value_hidden=4)
            elif tag == "h7":                               # no multiple of 4: layer 3 takes its scalar path
                netfile.write_random_build_net(path, 5, policy_hidden=7, value_hidden=3)
            else:
                netfile.write_random_build_net(path, 3, policy_hidden=8, value_hidden=4)
            data = bytearray(open(path, "rb").read())
        if tag == "zero":                                   # every parameter of the policy net zero: logits 0, policies exactly 1 / k
            for pos, count in _policy_blocks(16):
                data[pos:pos + 4 * count] = bytes(4 * count)
        if tag == "built":                                  # one large W1 column at a low cell, and first-layer weights big enough to matter:
            w1 = np.frombuffer(data, "<f4", 8 * 3749, 8 + 4 * 8).reshape(8, 3749).copy()   # x[index] (a low position) and x[cell] part ways
            w1[:, :64] = np.linspace(2.0, 6.0, 8)[:, None] * np.where(np.arange(64) % 2, -1.0, 1.0)[None, :]
            data[8 + 4 * 8:8 + 4 * 8 + 4 * 8 * 3749] = w1.astype("<f4").tobytes()
        _CACHE[tag] = bytes(data)
    return _CACHE[tag]


def _policy_blocks(h):
    pos = 0
    for i, o in ((3749, h), (h, h), (h, 3749)):
        yield pos + 8, o + o * i
        pos += 8 + 4 * (o + o * i)


def _nets(ctx, tag):
    if ("net", tag) not in _CACHE:
        _CACHE["net", tag] = (build.BuildNetwork(ctx, _net_bytes(tag)), B.Net(_net_bytes(tag)))
    return _CACHE["net", tag]


def _rows(n):
    """n rows: the planted teams in turn, row g's seed a function of g alone."""
    planted = B.planted_teams()
    teams = np.stack([planted[g % len(planted)][1] for g in range(n)])
    sizes = np.array([planted[g % len(planted)][2] for g in range(n)], np.uint8)
    seeds = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xB5AD4ECEDA1CE2A9)
    return teams, sizes, seeds


def _prefilled(n, trace=True, device="cuda"):
    """(the output dict as views of rows 1 .. n of buffers with one guard row on each side, the buffers)."""
    big, out = {}, {}
    shapes = {"teams_out": ((30,), torch.uint8), "n_updates": ((), torch.uint8), "action": ((31,), torch.int16), "index": ((31,), torch.int16),
              "n_legal": ((31,), torch.int16), "prob": ((31,), torch.float32)}
    if trace:
        shapes.update(trace_legal=((31, 339), torch.int16), trace_logits=((31, 339), torch.float32), trace_policy=((31, 339), torch.float32))
    for name, (shape, dtype) in shapes.items():
        big[name] = torch.full((n + 2,) + shape, float("nan") if dtype == torch.float32 else (255 if dtype == torch.uint8 else -1), dtype=dtype, device=device)
        out[name] = big[name][1:n + 1]
    return out, big


def _untouched(a):
    a = np.asarray(a)
    return np.isnan(a).all() if a.dtype == np.float32 else (a.view(np.uint8) == 255).all()


def _call(ctx, net, teams, sizes, seeds, input_update=0, trace=True):
    n = len(seeds)
    out, big = _prefilled(n, trace)
    t, s = torch.from_numpy(teams).cuda(), torch.from_numpy(sizes).cuda()
    sd = torch.from_numpy(seeds.view(np.int64)).cuda()
    got = build.rollout(ctx, net, t, sd, sizes=s, input_update=input_update, trace=trace, out=out)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in got.items() if k in big}
    for name, b in big.items():
        assert _untouched(b[0].cpu().numpy()) and _untouched(b[n + 1].cpu().numpy()), "guard row of %s written" % name
    return host


def _replay(ref, team, size, seed, input_update, row, key, logits=True):
    """Hold one traced row to the referee; returns the number of steps."""
    r, rng, k = B.Rollout(team, size, input_update), B.Stream(seed), 0
    n_updates = int(row["n_updates"])
    worst = WORST.setdefault(key, {"logit": 0.0, "policy": 0.0, "steps": 0})
    while r.legal() is not None:
        legal = r.legal()
        nl = len(legal)
        assert k < n_updates and int(row["n_legal"][k]) == nl, (key, k)
        assert (row["trace_legal"][k, :nl] == legal).all() and _untouched(row["trace_legal"][k, nl:]), (key, k)
        dev_logits, policy = row["trace_logits"][k, :nl], row["trace_policy"][k, :nl]
        assert _untouched(row["trace_logits"][k, nl:]) and _untouched(row["trace_policy"][k, nl:])
        if logits:
            l64, bound = ref.logit_bound(r.x, legal)
            err = np.abs(dev_logits.astype(np.float64) - l64)
            assert (err <= bound).all(), "%s step %d: logit off by %.3g, bound %.3g" % (key, k, err.max(), bound[err.argmax()])
            worst["logit"] = max(worst["logit"], float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
        want = B.softmax64(dev_logits)
        rel = np.abs(policy.astype(np.float64) - want) / want
        assert rel.max() <= B.POLICY_BOUND, "%s step %d: policy off by %.3g relative" % (key, k, rel.max())
        worst["policy"] = max(worst["policy"], float(rel.max() / B.POLICY_BOUND))
        index = B.pick(policy, rng.uniform())
        assert int(row["index"][k]) == index, "%s step %d: index %d, the pick rule on the device's policy gives %d" % (key, k, row["index"][k], index)
        assert row["prob"][k] == policy[index] and int(row["action"][k]) == legal[index]
        r.advance(index)
        k += 1
    worst["steps"] += k
    assert k == n_updates == r.steps, (key, k, n_updates)
    assert (row["teams_out"] == r.team).all(), key
    assert not B.additions(r.team, size), key
    for name in ("action", "index", "n_legal", "prob"):
        assert _untouched(row[name][k:]), (key, name)
    assert _untouched(row["trace_legal"][k:]) and _untouched(row["trace_logits"][k:]) and _untouched(row["trace_policy"][k:])
    return k


def _row(host, g):
    return {k: v[g] for k, v in host.items()}


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    for name in a:
        x, y = a[name][rows_a], b[name][rows_b]
        assert x.tobytes() == y.tobytes(), name


def _big(ctx, tag):
    """The traced 257-row call of a net, made once."""
    if ("big", tag) not in _CACHE:
        teams, sizes, seeds = _rows(257)
        _CACHE["big", tag] = (teams, sizes, seeds, _call(ctx, _nets(ctx, tag)[0], teams, sizes, seeds))
    return _CACHE["big", tag]


@pytest.mark.parametrize("tag", ("h128", "h8", "h7", "zero"))
def test_every_row_and_step_against_the_referee(gpu_ctx, tag):
    teams, sizes, seeds, host = _big(gpu_ctx, tag)
    ref = _nets(gpu_ctx, tag)[1]
    steps = {}
    for g in range(257):                                     # logits on the first 65 rows (every planted team, two and a half times over)
        steps[g] = _replay(ref, teams[g], int(sizes[g]), int(seeds[g]), 0, _row(host, g), tag, logits=g < 65)
    names = [p[0] for p in B.planted_teams()]
    assert steps[names.index("empty")] == 31 and steps[names.index("complete")] == 1 and steps[names.index("complete_size1")] == 0
    assert steps[names.index("one_missing_move")] == 2 and steps[names.index("pool_used_up")] == 1


def test_uniform_net_equals_the_free_running_referee(gpu_ctx):
    teams, sizes, seeds, host = _big(gpu_ctx, "zero")
    ref = _nets(gpu_ctx, "zero")[1]
    for g in range(48):
        want = B.rollout(ref, teams[g], int(sizes[g]), int(seeds[g]))
        k = want["n_updates"]
        assert host["n_updates"][g] == k and (host["teams_out"][g] == want["team"]).all()
        assert (host["action"][g, :k] == want["action"]).all() and (host["index"][g, :k] == want["index"]).all()
        assert host["prob"][g, :k].tobytes() == np.array(want["prob"], np.float32).tobytes()
        assert all(host["prob"][g, j] == np.float32(1.0) / np.float32(host["n_legal"][g, j]) for j in range(k))


@pytest.mark.parametrize("n", ROWS)
def test_row_counts_repeatability_and_independence(gpu_ctx, n):
    """A call of n rows gives the first n rows of the 257-row call bit for bit (a row depends on its team and seed alone), twice."""
    teams, sizes, seeds, host = _big(gpu_ctx, "h128")
    net = _nets(gpu_ctx, "h128")[0]
    first = _call(gpu_ctx, net, teams[:n], sizes[:n], seeds[:n])
    again = _call(gpu_ctx, net, teams[:n], sizes[:n], seeds[:n])
    _same(first, again)
    _same(first, host, rows_b=slice(0, n))
    if n == 1:
        for g in (5, 64, 130, 256):                         # row g alone
            alone = _call(gpu_ctx, net, teams[g:g + 1], sizes[g:g + 1], seeds[g:g + 1])
            _same(alone, host, rows_b=slice(g, g + 1))


def test_numpy_path_and_default_size(gpu_ctx):
    teams, sizes, seeds, host = _big(gpu_ctx, "h128")
    net = _nets(gpu_ctx, "h128")[0]
    got = build.rollout(gpu_ctx, net, teams[:65], seeds[:65], sizes=sizes[:65], trace=True)
    k = host["n_updates"][:65]
    assert (got["n_updates"] == k).all() and (got["teams_out"] == host["teams_out"][:65]).all()
    for g in range(65):
        for name in ("action", "index", "n_legal", "prob"):
            assert got[name][g, :k[g]].tobytes() == host[name][g, :k[g]].tobytes()
            assert not got[name][g, k[g]:].any()                                  # the face's own arrays start as zeros
        for j in range(k[g]):
            nl = int(host["n_legal"][g, j])
            assert got["trace_legal"][g, j, :nl].tobytes() == host["trace_legal"][g, j, :nl].tobytes() and (got["trace_legal"][g, j, nl:] == -1).all()
            assert got["trace_policy"][g, j, :nl].tobytes() == host["trace_policy"][g, j, :nl].tobytes()
    six = sizes[:24] == 6
    plain = build.rollout(gpu_ctx, net, teams[:24][six], seeds[:24][six])          # sizes=None means 6, and no trace
    assert (plain["teams_out"] == host["teams_out"][:24][six]).all() and "trace_legal" not in plain


def test_input_update_rule(gpu_ctx):
    """input_update 0 (x at the position in the list, the reference's) against 1 (x at the action's cell): each equals its referee, and on the
    built net they part ways."""
    net, ref = _nets(gpu_ctx, "built")
    teams, sizes, seeds = _rows(48)
    got = [_call(gpu_ctx, net, teams, sizes, seeds, input_update=u) for u in (0, 1)]
    for u in (0, 1):
        for g in range(48):
            _replay(ref, teams[g], int(sizes[g]), int(seeds[g]), u, _row(got[u], g), "built_update%d" % u)
    differ = [g for g in range(48) if got[0]["teams_out"][g].tobytes() != got[1]["teams_out"][g].tobytes()]
    assert len(differ) >= 8, differ
    assert (got[0]["action"][:, 0] == got[1]["action"][:, 0]).all()               # the first step has seen no update yet


PROVIDER_CASES = {"unmodified": dict(team_modify_prob=0.0, pokemon_delete_prob=0.5, move_delete_prob=0.5),
                  "modified": dict(team_modify_prob=1.0, pokemon_delete_prob=0.3, move_delete_prob=0.4),
                  "sometimes": dict(team_modify_prob=0.5, pokemon_delete_prob=0.1, move_delete_prob=0.1),
                  "truncated": dict(team_modify_prob=1.0, pokemon_delete_prob=0.5, move_delete_prob=0.5, max_pokemon=3),
                  "one_pokemon": dict(team_modify_prob=1.0, pokemon_delete_prob=0.5, move_delete_prob=0.5, max_pokemon=1)}


@pytest.mark.parametrize("case", sorted(PROVIDER_CASES))
def test_provider_against_the_referee(gpu_ctx, case):
    """The prelude exactly (team_index, the team after truncation and deletion, changed), then the rollout of the changed rows: the same bits as
    rollout() on teams_init from the stream where the prelude left it; with the uniform net also the free-running referee's actions."""
    kw = PROVIDER_CASES[case]
    pool = B.sample_teams()
    n = 96
    seeds = np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(12345)
    for tag in ("h8", "zero"):
        net, ref = _nets(gpu_ctx, tag)
        got = build.provide(gpu_ctx, net, torch.from_numpy(pool).cuda(), torch.from_numpy(seeds.view(np.int64)).cuda(), **kw)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        streams, built = np.zeros(n, np.uint64), np.zeros(n, bool)
        for g in range(n):
            index, team, size, changed, stream = B.prelude(pool, int(seeds[g]), kw.get("max_pokemon", 6), kw["pokemon_delete_prob"], kw["move_delete_prob"],
                                                           kw["team_modify_prob"])
            assert got["team_index"][g] == (-1 if changed else index), (case, g)
            assert (got["teams_init"][g] == team).all() and got["sizes"][g] == size, (case, g)
            streams[g], built[g] = stream, changed
            if not changed:
                assert got["n_updates"][g] == 0 and (got["teams_out"][g] == team).all()
            elif tag == "zero":
                want = B.rollout(ref, team, size, stream)
                k = want["n_updates"]
                assert got["n_updates"][g] == k and (got["teams_out"][g] == want["team"]).all() and (got["action"][g, :k].view(np.uint16) == want["action"]).all()
        if case == "unmodified":
            assert not built.any()
        elif case in ("modified", "truncated"):
            assert built.all() if case == "truncated" else built.sum() > n * 0.9
        elif case == "sometimes":
            assert 10 < built.sum() < n - 10
        if built.any():
            again = build.rollout(gpu_ctx, net, got["teams_init"][built], streams[built], sizes=got["sizes"][built])
            assert (again["n_updates"] == got["n_updates"][built]).all() and (again["teams_out"] == got["teams_out"][built]).all()
            for name in ("action", "index", "n_legal", "prob"):
                assert again[name].tobytes() == np.ascontiguousarray(got[name][built]).tobytes(), (case, name)
        if case == "one_pokemon":                            # one complete Pokemon: nothing to add, nothing to swap
            assert (got["n_updates"] == 0).all() and (got["team_index"] == -1).all()


def test_records_against_the_referee_codec(gpu_ctx):
    net, _ = _nets(gpu_ctx, "h8")
    pool = B.sample_teams()
    n = 80
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(99)
    value = np.linspace(0, 1, n).astype(np.float32)
    score = np.array([(0.0, 0.5, 1.0, -1.0)[g % 4] for g in range(n)], np.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    got = build.provide(gpu_ctx, net, t(pool), t(seeds.view(np.int64)), team_modify_prob=0.6, pokemon_delete_prob=0.3, move_delete_prob=0.3)
    dev = build.records(gpu_ctx, got, t(value), t(score))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in got.items()}
    want = b"".join(B.encode_record(host["teams_init"][g], int(host["sizes"][g]), host["action"][g, :k].view(np.uint16), host["prob"][g, :k], value[g],
                                    None if score[g] < 0 else float(score[g]))
                    for g, k in enumerate(host["n_updates"]) if k)
    assert 0 < len(want) < n * 128 and dev.cpu().numpy().tobytes() == want
    host["action"] = host["action"].view(np.uint16)
    assert build.records(gpu_ctx, host, value, score) == want                     # the numpy path
    built = [g for g in range(n) if host["n_updates"][g]]
    for d, g in zip(build.decode_records(want), built):
        k, first = int(host["n_updates"][g]), len(B.initial_cells(host["teams_init"][g], int(host["sizes"][g])))
        assert d["score"] == (None if score[g] < 0 else score[g]) and abs(d["value"] - value[g]) <= 1 / 65535
        assert (d["action"][first:first + k] == host["action"][g, :k]).all() and not d["action"][first + k:].any()
        # initial cells plus updates rebuild the terminal team's cells (as a set: the swap repeats a species cell)
        assert set(d["action"][:first + k].tolist()) == set(B.initial_cells(host["teams_out"][g], int(host["sizes"][g])))
    # the reference's own bytes for hand-written trajectories, through the device packer
    G = np.load(os.path.join(ROOT, "tests", "golden", "build_goldens.npz"))
    traj = {"teams_init": G["traj_teams"], "sizes": G["traj_sizes"], "n_updates": G["traj_n"], "action": G["traj_cells"], "prob": G["traj_probs"]}
    assert build.records(gpu_ctx, traj, G["traj_value"], G["traj_score"]) == G["records"].tobytes()


def test_write_worst_ratios(gpu_ctx):
    """Last in the file: the worst bound ratios seen above (run alone: of the hidden-8 net), for profiles/r25_build_accuracy.json."""
    if not WORST:
        test_every_row_and_step_against_the_referee(gpu_ctx, "h8")
    for key, w in WORST.items():
        assert w["policy"] <= 1.0 and w["logit"] <= 1.0, (key, w)
    path = os.environ.get("OAKGPU_BUILD_ACCURACY_OUT")
    if path:
        json.dump({"bounds": {"logit": "4 max|l32 - l64| + 2e-7 S", "policy": "6 x 2^-24 relative to the float64 softmax of the device's logits"},
                   "worst_ratio_of_bound": WORST}, open(path, "w"), indent=1, sort_keys=True)
