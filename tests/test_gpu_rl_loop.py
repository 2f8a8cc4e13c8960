"""GPU: the reinforcement loop on one device (oak_amd/rl.py) -- three rounds of 64 self-play games (PUCB + net_tiny, budget 8), a window of 96
records so that round 3 evicts, 2 steps of 256 rows per round.
  1. two runs give the same checkpoint bytes;
  2. the checkpoints equal those of a loop over host bytes written here: the same self-play calls with the same seeds, the records taken to
     the host, the newest 96 concatenated into FrameCorpus(ctx, bytes), the same sample -> apply_symmetries -> step.  That holds the loop, the
     window's order and eviction, and the evaluator's refresh at once;
  3. --save-data leaves files whose concatenation is the window's history: its newest 96 records are the window."""
import os

import numpy as np
import pytest
import torch

import policy_ref as P
from oak_amd import rl
from oak_amd.engine import Network
from oak_amd.frames import replay_index
from oak_amd.search import Forest
from oak_amd.train import EncodedBattleFrames, FrameCorpus, Trainer, apply_symmetries, train_loss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, GAMES, BUDGET, WINDOW, BATCH, STEPS, SEED, LENGTH = 3, 64, 8, 96, 256, 2, 5, 150
KW = dict(bandit="pucb-1.0", policy_mode="e", max_battle_length=LENGTH, checkpoint=2, seed=SEED)
_CACHE = {}


def _pool():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from policy_match import team_bytes
    return team_bytes(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json")).reshape(-1, 30)


def _net_bytes():
    return open(P.GOLDEN["tiny"], "rb").read()


def _run(ctx, tmp_path):
    """The run every test looks at (made once): with --save-data and the window's bytes kept."""
    if "run" not in _CACHE:
        rows = []
        res = rl.run(ctx, _net_bytes(), _pool(), ROUNDS, GAMES, BUDGET, STEPS, BATCH, 1e-3, WINDOW, save_data=str(tmp_path / "data"), keep_records=True,
                     log=rows.append, **KW)
        _CACHE["run"] = (res, rows, str(tmp_path / "data"))
    return _CACHE["run"]


def _records(data):
    idx = replay_index(data)
    assert idx["stopped_at"] == len(data)
    ends = list(idx["offsets"][1:]) + [len(data)]
    return [data[int(a):int(b)] for a, b in zip(idx["offsets"], ends)]


def test_two_runs_give_the_same_checkpoints(gpu_ctx, tmp_path):
    res, rows, _ = _run(gpu_ctx, tmp_path)
    again = rl.run(gpu_ctx, _net_bytes(), _pool(), ROUNDS, GAMES, BUDGET, STEPS, BATCH, 1e-3, WINDOW, **KW)
    assert sorted(res["checkpoints"]) == [2, 4, 6] and res["checkpoints"] == again["checkpoints"] and res["net"] == again["net"]
    assert res["checkpoints"][2] != res["checkpoints"][4] != res["checkpoints"][6] and res["net"] == res["checkpoints"][6] != _net_bytes()
    assert [r["window"] for r in rows][-1] == WINDOW and rows[-1]["evicted"] > 0 and rows[0]["evicted"] == 0     # round 3 evicts
    assert all(r["rows"] > 0 and np.isfinite(r["loss"]) for r in rows) and res["window"]["rejected"] == 0
    print(rows)


def test_the_loop_equals_a_loop_over_host_bytes(gpu_ctx, tmp_path):
    res, rows, _ = _run(gpu_ctx, tmp_path)
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
        for _ in range(STEPS):
            s = rl.sample_seed(SEED, step, BATCH)
            corpus.sample(enc, s, LENGTH, 1, count_ok=False)
            apply_symmetries(gpu_ctx, enc, s)
            trainer.step(enc, BATCH, loss, 1e-3)
            step += 1
            if step % 2 == 0:
                checkpoints[step] = trainer.net_bytes()
        current = trainer.net_bytes()
        corpus.close()
    forest.close()
    trainer.close()
    assert len(history) > WINDOW and [r["games"] for r in rows] and sum(r["games"] for r in rows) == len(history)
    assert checkpoints == res["checkpoints"] and current == res["net"]
    assert res["records"] == b"".join(history[-WINDOW:])


def test_saved_data_is_the_windows_history(gpu_ctx, tmp_path):
    res, rows, data_dir = _run(gpu_ctx, tmp_path)
    files = [os.path.join(data_dir, "%d.battle.data" % r) for r in range(ROUNDS)]
    assert sorted(os.listdir(data_dir)) == sorted(os.path.basename(f) for f in files)
    recs = _records(b"".join(open(f, "rb").read() for f in files))
    assert len(recs) == res["window"]["appended"] and res["window"]["evicted"] == len(recs) - WINDOW
    assert b"".join(recs[-WINDOW:]) == res["records"]
    assert [len(_records(open(f, "rb").read())) for f in files] == [r["games"] for r in rows]
