"""GPU: the whole `generate` loop with team building -- provide (both seats) -> endless-battle-check redraw -> forest_selfplay at the
smallest batch and budget tests/test_gpu_forest_selfplay.py uses (5 games, 8 iterations, Monte-Carlo leaves) -> records.  The
`.battle.data` passes the replay check; every built seat of a kept game has one record; its score byte is the game's result from that
seat; its initial cells plus updates are the cells of the team the game was played with, and a closing lead swap names that team's lead."""
import numpy as np
import pytest

import build_ref as B
from oak_amd import build, netfile
from oak_amd.frames import forest_selfplay, replay_check

pytestmark = pytest.mark.gpu
SCORE = {1: 1.0, 2: 0.0, 3: 0.5}


@pytest.mark.parametrize("max_pokemon", (6, 3))
def test_built_teams_play_and_their_records_carry_the_result(gpu_ctx, tmp_path, max_pokemon):
    path = str(tmp_path / "t.build.net")
    netfile.write_random_build_net(path, 4, policy_hidden=8, value_hidden=4)
    n, iterations = 5, 8
    seeds = (np.arange(2 * n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(31)).reshape(n, 2)
    with build.BuildNetwork(gpu_ctx, path) as net:
        teams, seats = build.provide_pairs(gpu_ctx, net, B.sample_teams(), seeds, max_pokemon=max_pokemon, team_modify_prob=0.8, pokemon_delete_prob=0.3,
                                           move_delete_prob=0.3)
    assert teams.shape == (n, 60) and (teams[:, :30] == seats[0]["teams_out"]).all() and (teams[:, 30:] == seats[1]["teams_out"]).all()
    for s in (0, 1):                                          # what provide_pairs kept is what provide gives for the seeds it reports
        for g in range(n):
            index, team, size, changed, _ = B.prelude(B.sample_teams(), int(seats[s]["seeds"][g]), max_pokemon, 0.3, 0.3, 0.8)
            assert (seats[s]["teams_init"][g] == team).all() and seats[s]["team_index"][g] == (-1 if changed else index)
            build.check_teams(teams[g, 30 * s:30 * s + 30], [size])
            assert (teams[g].reshape(2, 6, 5)[s, :size, 0] != 0).all() and not teams[g].reshape(2, 6, 5)[s, size:].any()
    battle_seeds = np.arange(n, dtype=np.uint64) + np.uint64(700)
    stream, offsets, n_frames, results, status = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds[:, 0] ^ np.uint64(5), iterations, c=2.0, evaluator="mc",
                                                                 policy_mode="e")
    assert (status == 0).all() and (n_frames > 0).all()
    rep = replay_check(gpu_ctx, stream)
    assert len(rep["reports"]) == n and (rep["reports"]["status"] == 0).all(), rep["reports"]
    score = np.array([SCORE[int(r) & 15] for r in results], np.float32)
    built_any = 0
    for s in (0, 1):
        data = build.records(gpu_ctx, seats[s], 0.5, score if s == 0 else 1 - score)
        built = [g for g in range(n) if seats[s]["n_updates"][g] > 0]
        built_any += len(built)
        recs = build.decode_records(data)
        assert len(recs) == len(built) and len(data) == 128 * len(built)
        for d, g in zip(recs, built):
            assert d["score"] == (score[g] if s == 0 else 1 - score[g]) and abs(d["value"] - 0.5) < 1e-4
            size = int(seats[s]["sizes"][g])
            k = len(B.initial_cells(seats[s]["teams_init"][g], size)) + int(seats[s]["n_updates"][g])
            played = teams[g, 30 * s:30 * s + 30]
            assert set(d["action"][:k].tolist()) == set(B.initial_cells(played, size)) and not d["action"][k:].any()
            assert (d["probability"][:k - int(seats[s]["n_updates"][g])] == 0).all() and (d["probability"][k - int(seats[s]["n_updates"][g]):k] > 0).all()
            if size > 1:                                      # the last update of a built team is the lead swap
                assert B.LIST[d["action"][k - 1]][0] == played[0] and B.LIST[d["action"][k - 1]][1] == 0
    assert built_any >= 4


def test_cpp_and_pyoak_faces_equal_the_python_face(gpu_ctx, tmp_path):
    """OakGPU::BuildNet (tests/cpp_build_smoke.cc, a child process) and pyoak.build_teams give oak_amd.build's arrays."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    net_path, pool_path, out_path, exe = (str(tmp_path / x) for x in ("t.build.net", "pool.bin", "out.bin", "cpp_build_smoke"))
    netfile.write_random_build_net(net_path, 6, policy_hidden=8, value_hidden=4)
    pool = B.sample_teams()
    pool.tofile(pool_path)
    n = 40
    seeds = np.uint64(1000) + np.uint64(17) * np.arange(n, dtype=np.uint64)
    kw = dict(max_pokemon=5, pokemon_delete_prob=0.3, move_delete_prob=0.3, team_modify_prob=0.7)
    with build.BuildNetwork(gpu_ctx, net_path) as net:
        want = build.provide(gpu_ctx, net, pool, seeds, **kw)
        score = np.array([-1.0 if g % 3 == 2 else 0.5 * (g % 3) for g in range(n)], np.float32)
        want_records = build.records(gpu_ctx, want, 0.5, score)
        again = build.rollout(gpu_ctx, net, want["teams_init"], seeds, sizes=want["sizes"], input_update=1)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp_build_smoke.cc"), "-L",
                           os.path.join(root, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(root, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe, net_path, pool_path, out_path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    expected = b"".join(np.ascontiguousarray(a).tobytes() for a in (want["teams_out"], want["n_updates"], want["teams_init"], want["sizes"], want["team_index"],
                                                                      want["action"], want["prob"], again["teams_out"], again["n_updates"])) + want_records
    assert open(out_path, "rb").read() == expected and len(want_records) > 0
    from oak_amd import pyoak
    got = pyoak.build_teams(open(net_path, "rb").read(), pool, seeds, **kw)
    assert (got["teams"] == want["teams_out"]).all() and (got["team_index"] == want["team_index"]).all() and (got["n_updates"] == want["n_updates"]).all()
    for name in ("teams_init", "sizes", "action", "index", "n_legal", "prob"):
        assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(want[name]).tobytes(), name
