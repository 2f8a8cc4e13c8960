"""GPU: build.BuildWindow (oakgpu_build_window_*, oak_amd/csrc/buildwindow.hip) -- the newest 64 `.build.data` records, appended to in
batches of 0, 1, 63, 1, 64, 65 and 200.  A plain Python list is the referee of what the window holds and counts; after every append a
TrajectoryCorpus made from the referee's bytes as one file is the referee of every corpus call: info, decode of every record with both mask
dtypes, and sample(257, seed) with its picks for two seeds, all bit for bit.  Some records are malformed (tests/build_traj_ref.py's), and
the batch of 65 holds two records whose format byte is not 0: those are rejected."""
import numpy as np
import pytest

import build_traj_ref as T
from oak_amd import _lib, build

pytestmark = pytest.mark.gpu
MAX_RECORDS = 64
BATCHES = (0, 1, 63, 1, 64, 65, 200)
DEVICE_BATCHES = (2, 6)          # these go in as GPU tensors (oakgpu_build_window_append_dev), the others as host bytes
_CACHE = {}


def pool():
    """394 records: rollouts with the malformed records spread among them"""
    if "pool" not in _CACHE:
        rolled = np.asarray(T.rollout_records(sum(BATCHES), 28))[:sum(BATCHES)]
        bad = np.stack([r for _, _, r in T.malformed_records()])
        records = rolled.copy()
        at = np.linspace(2, len(records) - 3, len(bad)).astype(int)
        records[at] = bad
        assert (records[:, 0] == 0).all()
        records.setflags(write=False)
        _CACHE["pool"] = (records, at)
    return _CACHE["pool"]


def same(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


def compare(ctx, window, held, counters):
    data = b"".join(held)
    assert window.records() == data
    assert window.stats() == dict(records=len(held), **counters)
    if not held:
        assert window.info()["records"] == 0
        with pytest.raises(_lib.OakGpuError, match="holds no record"):
            window.sample(4, 1)
        return
    with build.TrajectoryCorpus(ctx, data) as corpus:
        assert window.info() == corpus.info() and corpus.info()["files"] == 1
        picks = np.arange(len(held), dtype=np.uint32)
        for mask_dtype in ("int64", "int16"):
            same(window.decode(picks, mask_dtype=mask_dtype), corpus.decode(picks, mask_dtype=mask_dtype))
        for seed in (3, 0x9E3779B97F4A7C15):
            got, want = window.sample(257, seed, mask_dtype="int16"), corpus.sample(257, seed, mask_dtype="int16")
            same(got, want)
            assert got["picks"].max() < len(held)


def test_the_window_is_a_corpus_of_the_surviving_records(gpu_ctx):
    import torch
    records, bad_at = pool()
    held, counters, at = [], dict(appended=0, evicted=0, rejected=0), 0
    malformed_seen = 0
    with build.BuildWindow(gpu_ctx, MAX_RECORDS) as window:
        compare(gpu_ctx, window, held, counters)
        for k, size in enumerate(BATCHES):
            batch = records[at:at + size].copy()
            at += size
            if size == 65:
                batch[3, 0], batch[40, 0] = 1, 7                     # two records of another format
            if k in DEVICE_BATCHES:
                window.append(torch.from_numpy(batch).to(torch.device("cuda", gpu_ctx.device)))
            else:
                window.append(batch.tobytes())
            accepted = [r.tobytes() for r in batch if r[0] == 0]
            counters["rejected"] += len(batch) - len(accepted)
            counters["appended"] += len(accepted)
            held += accepted
            counters["evicted"] += max(0, len(held) - MAX_RECORDS)
            held = held[-MAX_RECORDS:] if len(held) > MAX_RECORDS else held
            compare(gpu_ctx, window, held, counters)
            status = window.info()["status"]
            malformed_seen += sum(v for name, v in status.items() if name != "OK")
        assert counters["rejected"] == 2 and counters["evicted"] > 200 and len(held) == MAX_RECORDS and malformed_seen > 0
        window.append(b"")                                           # and an append of nothing changes nothing
        compare(gpu_ctx, window, held, counters)


def test_append_takes_the_game_records_and_their_count_word(gpu_ctx, tmp_path):
    import torch
    from test_gpu_build_game_records import game_outputs, seats_of
    n = 65
    seats = seats_of(gpu_ctx, tmp_path, n)
    status, results, matchup = game_outputs(n)
    want = build.game_records(gpu_ctx, seats, status, results, matchup)
    dev = torch.device("cuda", gpu_ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).to(dev)
    dseats = tuple({k: up(seat[k]) for k in ("teams_init", "sizes", "n_updates", "action", "prob")} for seat in seats)
    out = torch.full((2 * n, 128), 0xA5, dtype=torch.uint8, device=dev)      # (what lies beyond count has another format byte: it must not be read as records)
    records, count = build.game_records(gpu_ctx, dseats, up(status), up(results), up(matchup), out=out)
    total = len(want) // 128
    assert total > 8
    for max_records in (8, 256):
        with build.BuildWindow(gpu_ctx, max_records) as window:
            window.append(records, count)
            keep = min(total, max_records)
            assert window.records() == want[(total - keep) * 128:]
            assert window.stats() == dict(records=keep, appended=total, evicted=total - keep, rejected=0)
            window.append(records, count)
            keep2 = min(2 * total, max_records)
            assert window.records() == (want + want)[(2 * total - keep2) * 128:]


def test_refusals(gpu_ctx):
    with pytest.raises(_lib.OakGpuError, match="max_records == 0"):
        build.BuildWindow(gpu_ctx, 0)
    with build.BuildWindow(gpu_ctx, 4) as window:
        with pytest.raises(_lib.OakGpuError, match="100 bytes is not a multiple of 128"):
            window.append(bytes(100))
        assert window.stats() == dict(records=0, appended=0, evicted=0, rejected=0)
