"""GPU: the later passes of game_rows.hpp's 1,024-lane scan (oak_amd/csrc/game_rows.hpp), which the game loops reach only above 1,024
items -- blocks of 256 rows in k_rows_offsets, live rows in the match prelude, games in the scan of the record lengths:
  1. policy games over 1,025 blocks against the rollout kernel: the block offsets take two passes, then one as the games end;
  2. a match of 3,100 games with recording on, a third of them over before they start: three passes of the prelude, four of the record
     lengths; the games either side of every pass boundary against the same call on them alone, the record bases against the stated sizes."""
import time

import numpy as np
import pytest

import forest_match_ref as M
from oak_amd import arena
from oak_amd.arena import search_games
from test_gpu_forest_match import counts_of, openings, same
from test_gpu_policy_games import play, random_batch

pytestmark = pytest.mark.gpu


def test_block_offsets_past_1024_blocks(gpu_ctx):
    n = 1024 * 256 + 65                       # 1,025 blocks of 256 rows, the last of 65: not a multiple of 64
    pool = random_batch()
    idx = np.arange(n) % len(pool[3])
    b, d, r = (np.ascontiguousarray(x[idx]) for x in (pool[0], pool[1], pool[3]))
    p = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)).view(np.uint8).reshape(n, 8).copy()
    assert p.view(np.uint64).all() and len(np.unique(p.view(np.uint64))) == n    # every stream its own, none zero
    t0 = time.time()
    got = play(gpu_ctx, (None, None), (b, d, p, r), max_turns=1000, poll=1, compact_below=2.0)
    stats = arena.last_stats(gpu_ctx)
    t1 = time.time()
    roll = gpu_ctx.rollout(b, d, r, p, max_steps=1000, prep=False, return_state=True)
    print("%d rows, %d blocks: policy games %.2f s, rollout %.2f s; stats %s" % (n, (n + 255) // 256, t1 - t0, time.time() - t1, stats))
    assert (got["results"] == roll["results"]).all() and (got["turns"] == roll["steps"]).all()
    assert (got["values"].view(np.uint32) == roll["values"].view(np.uint32)).all()
    assert (got["prng"] == roll["prng"]).all() and (got["battles"] == roll["battles"]).all() and (got["durations"] == roll["durations"]).all()
    t = got["results"] & 15
    assert got["counts"] == (int((t == 1).sum()), int((t >= 3).sum()), int((t == 2).sum()), int((t == 0).sum()))
    assert stats["compactions"] >= 2


def test_match_prelude_and_record_bases_past_two_passes(gpu_ctx):
    n = 3100
    seat = dict(iterations=4, bandit="ucb", c=2.0, evaluator="poke-engine")
    b, d, r, seeds = openings(gpu_ctx, n)
    prng = (np.arange(9 * 8, dtype=np.uint64) * np.uint64(37) + np.uint64(1)).astype(np.uint8).reshape(9, 8)
    done = gpu_ctx.rollout(b[:9].copy(), d[:9].copy(), r[:9].copy(), prng, max_steps=1000, return_state=True)
    assert ((done["results"] & 15) != 0).all()
    over = np.flatnonzero(np.arange(n) % 3 == 1)
    rest = np.flatnonzero(np.arange(n) % 3 != 1)
    assert len(rest) in (2066, 2067)          # the rows live at turn 0: three passes of the prelude's scan
    tile = np.arange(len(over)) % 9
    b[over], d[over], r[over] = done["battles"][tile], done["durations"][tile], done["results"][tile]
    kw = dict(max_turns=3, early_stop=0.0, log_turns=4)
    t0 = time.time()
    got = search_games(gpu_ctx, (seat, seat), b, d, r, seeds, records=True, **kw)
    print("%d games, %d live at turn 0: %.2f s" % (n, len(rest), time.time() - t0))
    assert (got["turns"][over] == 0).all() and (got["status"][over] == M.OK).all() and (got["results"][over] == r[over]).all()
    assert (got["status"][rest] == M.MAX_TURNS).all() and (got["turns"][rest] == 3).all()
    assert got["counts"] == counts_of(got)
    S = np.array([0, 1, 2, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 3071, 3072, 3073, 3099])
    alone = search_games(gpu_ctx, (seat, seat), b[S], d[S], r[S], seeds[S], **kw)
    assert same(alone, got, None, S)
    terminal = np.arange(n) % 3 == 1
    for rec in got["records"]:
        offsets = np.asarray(rec["offsets"]).astype(np.int64)
        assert (np.diff(offsets) == np.where(terminal, 391, 0)).all()
        assert int(offsets[n]) == len(rec["stream"]) == 391 * len(over)
        kept = np.frombuffer(rec["stream"], np.uint8).reshape(len(over), 391)
        assert (kept[:, :4].copy().view("<u4").reshape(-1) == 391).all() and (kept[:, 4:6] == 0).all()       # length, frame count
        assert (kept[:, 6:390] == b[over]).all() and (kept[:, 390] == r[over]).all()                         # the input battle, the result byte
    assert got["records"][0]["stream"] == got["records"][1]["stream"]
