"""CPU: the team-building referee tests/build_ref.py and the generated oak_amd/csrc/build_tables.inc against the reference's own
tables, legal lists and CompressedTrajectory bytes (tests/golden/build_goldens.npz, made by tests/golden/make_build_goldens.py); the
host-only refusals by their texts; the `.build.net` round trip; and four planted mistakes in the referee, each caught by a check.

The golden file holds no logits of NN::Build::Network::inference (its generator says why); the referee's float64 forward is held to
torch's float64 linear layers instead, and its restricted form (logit_bound at the legal cells) to the full one."""
import os

import numpy as np
import pytest

import build_ref as B
from oak_amd import _lib, build, netfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "build_goldens.npz"))


def _net(tmp_path, seed=5, hidden=8):
    path = str(tmp_path / "t.build.net")
    netfile.write_random_build_net(path, seed, policy_hidden=hidden, value_hidden=4)
    return open(path, "rb").read()


def test_tables_equal_the_reference():
    assert int(G["n_dim"]) == B.N_DIM == build.N_DIM == 3749 and int(G["max_actions"]) == B.MAX_ACTIONS == build.MAX_ACTIONS == 339
    assert (G["species_move_list"] == B.LIST).all()
    legal, cells, table = build.tables()                      # the generated header, through the library
    assert (cells == G["species_move_list"]).all() and list(legal) == B.LEGAL and (table == B.TABLE).all()
    for c, (s, m) in enumerate(G["species_move_list"]):
        assert table[s, m] == c
    assert (table >= 0).sum() == B.N_DIM


def test_generated_header_is_current():
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_build_tables as T
    data = json.load(open(os.path.join(ROOT, "oak_amd", "data", "gen1_data.json")))
    assert T.render(data) == open(os.path.join(ROOT, "oak_amd", "csrc", "build_tables.inc")).read()


def test_legal_lists_equal_the_reference():
    planted = B.planted_teams()
    assert [p[0] for p in planted] == list(G["team_names"])
    for t, (name, team, size) in enumerate(planted):
        assert (team == G["teams"][t]).all() and size == G["sizes"][t]
        got = B.additions(team, size)
        want = G["additions"][t]
        k = int((want[:, 0] >= 0).sum())
        assert k == len(got) and all(tuple(want[i]) == got[i][:3] for i in range(k)), name
        swaps = B.lead_swaps(team, size)
        want = G["lead_swaps"][t]
        k = int((want[:, 0] >= 0).sum())
        assert k == len(swaps) and all(tuple(want[i]) == swaps[i] for i in range(k)), name


def test_records_equal_the_reference():
    bumped = 0
    for i in range(len(G["records"])):
        n, score = int(G["traj_n"][i]), float(G["traj_score"][i])
        got = B.encode_record(G["traj_teams"][i], int(G["traj_sizes"][i]), G["traj_cells"][i, :n], G["traj_probs"][i, :n], G["traj_value"][i],
                              None if score < 0 else score)
        assert got == G["records"][i].tobytes(), i
        d = build.decode_records(got)[0]
        ref = B.decode_record(got)
        assert d["score"] == ref["score"] == (None if score < 0 else score)
        assert (d["action"] == ref["action"]).all() and (d["probability"] == ref["probability"]).all()
        k = len(B.initial_cells(G["traj_teams"][i], int(G["traj_sizes"][i])))
        assert (d["action"][k:k + n] == G["traj_cells"][i, :n]).all() and (d["probability"][:k] == 0).all()
        bumped += int(((d["probability"][k:k + n] == 1) & (G["traj_probs"][i, :n] * np.float32(65535) < 1)).sum())
    assert bumped >= 2               # probabilities small enough to round to 0 were bumped to 1


def test_forward_against_torch_float64(tmp_path):
    import torch
    net = B.Net(_net(tmp_path))
    rng = np.random.default_rng(1)
    for k in range(4):
        x = np.zeros(B.N_DIM)
        x[rng.choice(B.N_DIM, 5 + 10 * k, replace=False)] = 1.0
        h = torch.tensor(x, dtype=torch.float64)
        for j, (w, b) in enumerate(net.layers[:3]):
            h = torch.nn.functional.linear(h, torch.tensor(w, dtype=torch.float64), torch.tensor(b, dtype=torch.float64))
            h = torch.relu(h) if j < 2 else h
        l64 = net.forward(x)
        assert np.abs(l64 - h.numpy()).max() <= 1e-13
        cells = rng.choice(B.N_DIM, 40, replace=False)
        at, bound = net.logit_bound(x, cells)
        assert np.abs(at - l64[cells]).max() <= 1e-13
        l32 = net.forward(x, np.float32).astype(np.float64)
        assert (bound >= 2e-7 * np.abs(l64[cells])).all() and np.abs(l32 - l64)[cells].max() <= bound.min()


def test_net_file_round_trip_and_refusals(tmp_path):
    data = _net(tmp_path)
    build.check_net(data)
    net = B.Net(data)
    assert [w.shape for w, _ in net.layers] == [(8, 3749), (8, 8), (3749, 8), (4, 3749), (4, 4), (1, 4)]
    dims = np.frombuffer(data, "<u4", 2)
    assert tuple(dims) == (3749, 8)

    def refused(bad, text):
        with pytest.raises(_lib.OakGpuError, match=text):
            build.check_net(bad)
    refused(data[:-1], "truncated file")
    refused(data[:100], "truncated file")
    refused(b"", "null bytes")
    refused(data + b"\0", "trailing bytes")
    bad = bytearray(data)
    bad[12:16] = np.array([np.nan], "<f4").tobytes()
    refused(bytes(bad), "NaN parameter")
    # a policy net that ends at 8 instead of n_dim: rebuilt with consistent lengths
    path = str(tmp_path / "short.build.net")
    rng = np.random.default_rng(0)
    with open(path, "wb") as f:
        for i, o in [(3749, 8), (8, 8), (8, 8), (3749, 4), (4, 4), (4, 1)]:
            f.write(np.array([i, o], "<u4").tobytes() + rng.random(o + o * i).astype("<f4").tobytes())
    refused(open(path, "rb").read(), "does not end at n_dim")
    with open(path, "wb") as f:
        for i, o in [(3749, 8), (9, 8), (8, 3749), (3749, 4), (4, 4), (4, 1)]:
            f.write(np.array([i, o], "<u4").tobytes() + rng.random(o + o * i).astype("<f4").tobytes())
    refused(open(path, "rb").read(), "do not chain")
    with open(path, "wb") as f:
        for i, o in [(3748, 8), (8, 8), (8, 3749), (3749, 4), (4, 4), (4, 1)]:
            f.write(np.array([i, o], "<u4").tobytes() + rng.random(o + o * i).astype("<f4").tobytes())
    refused(open(path, "rb").read(), "does not start at n_dim")


def test_team_and_provider_refusals():
    planted = B.planted_teams()
    teams, sizes = np.stack([p[1] for p in planted]), np.array([p[2] for p in planted], np.uint8)
    build.check_teams(teams, sizes)
    build.check_teams(teams[:2])
    full = planted[1][1]

    def refused(text, fn, *args, **kw):
        with pytest.raises(_lib.OakGpuError, match=text):
            fn(*args, **kw)
    refused("n == 0", build.check_teams, np.zeros((0, 30), np.uint8))
    t = full.copy(); t[0] = 150                                                   # Mewtwo is not OU-legal
    refused("team 0: a species outside legal_species", build.check_teams, t)
    t = full.copy(); t[0] = 200
    refused("a species outside legal_species", build.check_teams, t)
    t = full.copy(); t[1] = next(m for m in range(1, 166) if m not in B.POOLS[int(full[0])])
    refused("a move outside its species' pool", build.check_teams, np.stack([full, t]))
    t = full.copy(); t[0] = 0
    refused("a move outside its species' pool", build.check_teams, t)              # moves without a species
    t = full.copy(); t[25:30] = t[0:5]
    refused("team 0: a duplicate species", build.check_teams, t)
    build.check_teams(t, [5])                                                      # ... unless the slot is out of play
    refused("size > 6", build.check_teams, full, [7])
    refused("input_update outside", build.check_teams, full, None, 2)
    pool = B.sample_teams()
    build.check_provide(pool, 4, 3, 0.5, 0.5, 1.0)
    refused("n == 0", build.check_provide, pool, 0)
    refused("an empty pool", build.check_provide, np.zeros((0, 30), np.uint8), 4)
    refused("max_pokemon outside 1..6", build.check_provide, pool, 4, 0)
    refused("max_pokemon outside 1..6", build.check_provide, pool, 4, 7)
    refused("pokemon_delete_prob outside", build.check_provide, pool, 4, 6, 1.5)
    refused("move_delete_prob outside", build.check_provide, pool, 4, 6, 0.0, -0.1)
    refused("team_modify_prob outside", build.check_provide, pool, 4, 6, 0.0, 0.0, float("nan"))
    t = pool.copy(); t[3, 5:10] = 0
    refused("pool team 3: an empty slot before a Pokemon", build.check_provide, t, 4)


# ---- the planted mistakes: each is caught by a check the GPU tests also make ----------------------------------------------------------
def test_planted_species_after_moves_is_caught():
    t = list(G["team_names"]).index("size5")                        # a missing Pokemon and a missing move: both kinds of addition
    want = [int(c) for c in G["additions"][t][:, 0] if c >= 0]
    assert [a[0] for a in B.additions(G["teams"][t], 5)] == want
    assert [a[0] for a in B.additions(G["teams"][t], 5, mistake="species_after_moves")] != want
    t = list(G["team_names"]).index("deleted_3")
    want = [int(c) for c in G["additions"][t][:, 0] if c >= 0]
    assert [a[0] for a in B.additions(G["teams"][t], int(G["sizes"][t]), mistake="species_after_moves")] != want


def test_planted_fallback_to_the_last_entry_is_caught():
    policy = np.array([0.25, 0.25, 0.25], np.float32)                # sums to 0.75: u = 0.9 falls off the end
    assert B.pick(policy, 0.9) == 0 and B.pick(policy, 0.9, mistake="fallback_last") == 2
    assert B.pick(policy, 0.6) == B.pick(policy, 0.6, mistake="fallback_last") == 2
    assert B.pick(policy, 0.25) == 0 and B.pick(policy, 0.2500001) == 1


def test_planted_x_at_the_cell_is_caught(tmp_path):
    """With x[cell] in place of x[index] the next step's logits leave the bound."""
    net = B.Net(_net(tmp_path, seed=9))
    team, size = next((p[1], p[2]) for p in B.planted_teams() if p[0] == "empty")
    good, bad = B.Rollout(team, size), B.Rollout(team, size, mistake="x_cell")
    one = B.Rollout(team, size, input_update=1)
    for r in (good, bad, one):
        r.advance(100)
    assert good.x[100] == 1 and bad.x[100] == 0 and (bad.x == one.x).all() and good.x.sum() == bad.x.sum() == 1
    legal = good.legal()
    assert legal == bad.legal()
    l64, bound = net.logit_bound(good.x, legal)
    wrong, _ = net.logit_bound(bad.x, legal)
    assert (np.abs(wrong - l64) / bound).max() > 100


def test_planted_delete_after_truncation_is_caught():
    pool = B.sample_teams()
    hits = 0
    for seed in range(40):
        index, team, size, changed, _ = B.prelude(pool, seed, 3, 0.5, 0.5, 1.0)
        assert changed and size == 3 and (team[:15] == pool[index][:15]).all() and not team[15:].any()
        _, wrong, _, _, _ = B.prelude(pool, seed, 3, 0.5, 0.5, 1.0, mistake="delete_after_truncation")
        hits += int((wrong != team).any())
    assert hits >= 30
    # without a truncation the deletion runs, and a modify draw at or above the probability leaves the team alone
    index, team, size, changed, _ = B.prelude(pool, 1, 6, 0.5, 0.5, 1.0)
    assert changed and (team != pool[index]).any()
    index, team, size, changed, _ = B.prelude(pool, 1, 6, 0.5, 0.5, 0.0)
    assert not changed and (team == pool[index]).all()


def test_referee_rollout_ends_complete(tmp_path):
    net = B.Net(_net(tmp_path))
    for name, team, size in B.planted_teams()[:13]:
        out = B.rollout(net, team, size, seed=77)
        assert not B.additions(out["team"], size), name
        t = out["team"].reshape(6, 5)
        assert (t[:size, 0] != 0).all() and not t[size:].any()
        want = 0 if (size == 1 and name == "complete_size1") else None
        assert want is None or out["n_updates"] == want
        assert out["n_updates"] <= B.MAX_STEPS
        build.check_teams(out["team"], [size])


def test_pyoak_attributes():
    """The reference's module attributes (pyoak.cc:598-620) and build_teams' refusals, without a GPU."""
    from oak_amd import pyoak
    assert (pyoak.build_policy_hidden_dim, pyoak.build_value_hidden_dim, pyoak.build_max_actions) == (128, 128, 339)
    assert [tuple(p) for p in pyoak.species_move_list] == [(int(s), int(m)) for s, m in G["species_move_list"]]
    assert (np.array(pyoak.species_move_table) == B.TABLE).all()
    with pytest.raises(RuntimeError, match="max_pokemon outside 1..6"):
        pyoak.build_teams(b"", B.sample_teams(), np.arange(3, dtype=np.uint64), max_pokemon=9)
    with pytest.raises(RuntimeError, match="an empty pool"):
        pyoak.build_teams(b"", np.zeros((0, 30), np.uint8), np.arange(3, dtype=np.uint64))


def test_cpp_face_compiles_and_links(tmp_path):
    import subprocess
    exe = str(tmp_path / "cpp_build_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_build_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
