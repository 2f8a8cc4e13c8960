"""GPU: the reinforcement loop with the build network's side (oak_amd/rl.py) at toy size -- 3 rounds of 32 games (PUCB + net_tiny, budget 8),
a random `.build.net` of hidden 8 / 4, every team modified and rebuilt, battle_skip_prob 0.5, both windows of 48 records, one step of each
trainer per round.
  1. two runs give the same bytes: both final networks, both windows' records;
  2. every build record's value and score are its game's under oakgpu_build_game_targets_host, recomputed from the round's outputs, and the
     build window is the newest 48 of the rounds' records;
  3. skipped games give build records (without a score) and no battle record;
  4. without the build arguments the loop gives the bytes of a battle loop written here from the pieces that are as they were."""
import numpy as np
import pytest

from oak_amd import build, netfile, rl
from test_gpu_rl_loop import _net_bytes, _pool, _records

pytestmark = pytest.mark.gpu
ROUNDS, GAMES, BUDGET, WINDOW, BATCH, SEED, LENGTH = 3, 32, 8, 48, 64, 9, 150
OK, SKIPPED = 0, 3
KW = dict(bandit="pucb-1.0", policy_mode="e", max_battle_length=LENGTH, checkpoint=1, seed=SEED)
BUILD_KW = dict(team_modify_prob=1.0, pokemon_delete_prob=0.3, move_delete_prob=0.3, battle_skip_prob=0.5, t1_budget=12, build_data_window=WINDOW, build_steps=1,
                build_batch_size=32, build_lr=1e-3, build_trajectories_per_step=16, build_keep_prob=0.8)
_CACHE = {}


def _build_net(tmp_path):
    if "net" not in _CACHE:
        path = str(tmp_path / "t.build.net")
        netfile.write_random_build_net(path, 4, policy_hidden=8, value_hidden=4)
        _CACHE["net"] = open(path, "rb").read()
    return _CACHE["net"]


def _run(ctx, tmp_path):
    if "run" not in _CACHE:
        rows = []
        res = rl.run(ctx, _net_bytes(), _pool(), ROUNDS, GAMES, BUDGET, 1, BATCH, 1e-3, WINDOW, keep_records=True, log=rows.append,
                     build_net_bytes=_build_net(tmp_path), **BUILD_KW, **KW)
        _CACHE["run"] = (res, rows)
    return _CACHE["run"]


def test_two_runs_give_the_same_bytes(gpu_ctx, tmp_path):
    res, rows = _run(gpu_ctx, tmp_path)
    again = rl.run(gpu_ctx, _net_bytes(), _pool(), ROUNDS, GAMES, BUDGET, 1, BATCH, 1e-3, WINDOW, keep_records=True, build_net_bytes=_build_net(tmp_path),
                   **BUILD_KW, **KW)
    for name in ("net", "build_net", "build_avg_net", "records", "build_records", "checkpoints", "build_checkpoints"):
        assert res[name] == again[name], name
    assert res["net"] != _net_bytes() and res["build_net"] != _build_net(tmp_path) and res["build_avg_net"] != res["build_net"]
    assert sorted(res["build_checkpoints"]) == [1, 2, 3] and res["build_checkpoints"][3] == res["build_net"] != res["build_checkpoints"][2]
    assert all(r["build_rows"] > 0 and np.isfinite(r["build_loss"]) for r in rows), rows
    print(rows)


def test_every_build_record_carries_its_games_matchup(gpu_ctx, tmp_path):
    res, rows = _run(gpu_ctx, tmp_path)
    history, seen_skipped = b"", 0
    for rnd, (r, row) in enumerate(zip(res["build_rounds"], rows)):
        recs = build.decode_records(r["records"])
        q = no_score = 0
        for g in range(GAMES):
            for seat in (0, 1):
                if not (r["built"][g] >> seat) & 1:
                    continue
                want = build.game_targets(r["status"][g], r["results"][g], r["matchup"][g], seat)
                if want is None:
                    continue
                value, score = want
                m = r["matchup"][g] if seat == 0 else 1.0 - r["matchup"][g]
                assert value == float(np.float32(m))
                assert recs[q]["value"] == int(np.float32(value) * np.float32(65535.0)) / 65535.0 and recs[q]["score"] == score, (rnd, g, seat)
                no_score += score is None
                q += 1
        assert q == len(recs) == row["build_records"] and q > 0
        skipped = r["status"] == SKIPPED
        # 3. skipped games: records without a score, one per built seat; no battle record
        assert no_score == sum(bin(int(b)).count("1") for b in r["built"][skipped]) and row["skipped"] == int(skipped.sum())
        assert row["games"] == int((r["status"] == OK).sum())
        assert not np.isnan(r["matchup"]).any() and (r["built"] == 3).all()      # team_modify_prob 1: both seats of every game are built
        seen_skipped += int(skipped.sum())
        history += r["records"]
    assert seen_skipped >= 16 and sum(row["games"] for row in rows) >= 16        # (about half of 96 games either way)
    assert len(history) // 128 > WINDOW and res["build_records"] == history[-WINDOW * 128:]
    assert res["build_window"] == dict(records=WINDOW, appended=len(history) // 128, evicted=len(history) // 128 - WINDOW, rejected=0)
    assert len(_records(res["records"])) == min(WINDOW, sum(row["games"] for row in rows))


def test_without_the_build_arguments_the_loop_is_the_battle_loop(gpu_ctx, tmp_path):
    from oak_amd.engine import Network
    from oak_amd.search import Forest
    from oak_amd.train import EncodedBattleFrames, FrameCorpus, Trainer, apply_symmetries, train_loss
    res = rl.run(gpu_ctx, _net_bytes(), _pool(), ROUNDS, GAMES, BUDGET, 1, BATCH, 1e-3, WINDOW, keep_records=True, **KW)
    assert "build_net" not in res
    off = rl.run(gpu_ctx, _net_bytes(), _pool(), ROUNDS, GAMES, BUDGET, 1, BATCH, 1e-3, WINDOW, keep_records=True, build_net_bytes=_build_net(tmp_path),
                 team_modify_prob=0.0, battle_skip_prob=0.5, **KW)                # (use_build needs team_modify_prob > 0)
    assert "build_net" not in off and off["net"] == res["net"] and off["records"] == res["records"]
    pool, current, history, step, checkpoints = _pool(), _net_bytes(), [], 0, {}
    enc = EncodedBattleFrames(BATCH, "cuda:0")
    trainer = Trainer(gpu_ctx, current, BATCH)
    forest = Forest(gpu_ctx, GAMES, BUDGET, contextual=True)
    loss = train_loss()
    for rnd in range(ROUNDS):
        net = Network(gpu_ctx, data=current)
        out = rl.selfplay_round(gpu_ctx, forest, net, pool, GAMES, SEED, rnd, BUDGET, "pucb-1.0", "e", max_battle_length=LENGTH)
        net.close()
        stream, offsets = out[0].cpu().numpy().tobytes(), out[1].cpu().numpy()
        history += [stream[int(offsets[g]):int(offsets[g + 1])] for g in range(GAMES) if offsets[g + 1] > offsets[g]]
        corpus = FrameCorpus(gpu_ctx, b"".join(history[-WINDOW:]))
        s = rl.sample_seed(SEED, step, BATCH)
        corpus.sample(enc, s, LENGTH, 1, count_ok=False)
        apply_symmetries(gpu_ctx, enc, s)
        trainer.step(enc, BATCH, loss, 1e-3)
        step += 1
        checkpoints[step] = trainer.net_bytes()
        current = trainer.net_bytes()
        corpus.close()
    forest.close()
    trainer.close()
    assert checkpoints == res["checkpoints"] and current == res["net"] and res["records"] == b"".join(history[-WINDOW:])
