"""Child process of tests/test_gpu_replay.py::test_scale_gpu_built_corpus_with_one_percent_damaged (GPU box only): 65,536 random-play
games built on the GPU (tools/replay_bench.py), a byte outside every choice list planted at a seeded frame of 1 % of them.  Exactly the
damaged games fail, at the planted frame or later; a seeded sample of 256 records (64 damaged) agrees with tests/replay_oracle.py."""
import os
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
torch.cuda.init()
import replay_bench as RB  # noqa: E402
import replay_oracle as R  # noqa: E402
from oak_amd.engine import Context  # noqa: E402
from oak_amd.frames import replay_check  # noqa: E402

ctx = Context(0)
first, results, frames, lengths = RB.play_corpus(ctx, 65536, seed=3)
buf, offs = RB.assemble(first, results, frames, lengths)
rng = np.random.default_rng(21)
where = {}
for g in np.sort(rng.choice(np.nonzero(lengths >= 2)[0], 655, replace=False)):
    k = int(rng.integers(0, lengths[g]))
    p = int(offs[g]) + 391 + int((11 + 4 * (frames[:k, g, 0].astype(np.int64) + frames[:k, g, 1])).sum())
    buf[p + 1] = 0xFF
    where[int(g)] = k
blob = buf.tobytes()
out = replay_check(ctx, blob, want_states=True)
st = out["reports"]["status"]
assert len(st) == 65536 and set(np.nonzero(st != R.OK)[0].tolist()) == set(where), sorted(set(np.nonzero(st != R.OK)[0].tolist()) ^ set(where))[:10]
assert all(out["reports"]["frame"][g] >= k for g, k in where.items())
sample = sorted(set(rng.choice(65536, 192, replace=False).tolist()) | set(list(where)[:64]))
for g in sample:
    lo = int(offs[g])
    st_, pl, fr, ex, got, b, d = R.replay(blob[lo:lo + struct.unpack_from("<I", blob, lo)[0]])
    rep = out["reports"][g]
    assert (rep["status"], rep["player"], rep["frame"], rep["expected"], rep["got"]) == (st_, pl, fr, ex, got), (g, rep, st_, pl, fr, ex, got)
    assert (out["battles"][g] == b).all() and (out["durations"][g] == d).all(), g
print("replay scale ok: %d games, %d frames, %d damaged, %d checked against the oracle" % (len(st), int(lengths.sum()), len(where), len(sample)))
