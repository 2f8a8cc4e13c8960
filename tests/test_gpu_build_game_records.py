"""GPU: both seats' `.build.data` records of a batch of games in one launch (oakgpu_build_game_records_dev; build.game_records) against
build.records per seat with the host rule's value and score (oakgpu_build_game_targets_host), interleaved game-major, p1 before p2, by a few
lines of numpy.  Seats from build.provide on the golden sample teams; synthetic status / results / matchup arrays that cover every status,
every result type and the matchups 0, 1 and one whose product with 65535 sits on a rounding edge.  n = 1, one past a wave, one past the
kernel's block of 256 (where its scan carries a base into the next pass)."""
import numpy as np
import pytest

import build_ref as B
from oak_amd import build, netfile

pytestmark = pytest.mark.gpu
OK, MAX_LENGTH, ZERO_POLICY, SKIPPED = 0, 1, 2, 3
# 0.5 * 65535 = 32767.5 truncates; 2 / 65535 in float32 times 65535.f lands on either side of 2 depending on the rounding of the product
MATCHUPS = np.array([0.0, 1.0, 0.5, 2.0 / 65535.0, 0.3, 1.0 - 2.0 / 65535.0, 0.999999999, 1e-9], np.float64)
_CACHE = {}


def seats_of(ctx, tmp_path, n):
    if n not in _CACHE:
        path = str(tmp_path / "t.build.net")
        netfile.write_random_build_net(path, 4, policy_hidden=8, value_hidden=4)
        seeds = (np.arange(2 * n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(31)).reshape(n, 2)
        with build.BuildNetwork(ctx, path) as net:
            _CACHE[n] = tuple(build.provide(ctx, net, B.sample_teams(), seeds[:, s], max_pokemon=6, team_modify_prob=0.7, pokemon_delete_prob=0.3, move_delete_prob=0.3)
                              for s in (0, 1))
    return _CACHE[n]


def game_outputs(n):
    g = np.arange(n)
    status = np.array([OK, SKIPPED, OK, MAX_LENGTH, OK, ZERO_POLICY, SKIPPED, OK], np.uint8)[g % 8]
    results = np.array([1, 2, 3, 0x11, 0x22, 0x33, 2], np.uint8)[g % 7]       # win, lose, tie, alone and with the upper nibble set
    matchup = MATCHUPS[(g // 2) % len(MATCHUPS)].copy()
    if n == 1:
        status[0], matchup[0] = OK, 0.3
    return status, results, matchup


def referee(ctx, seats, status, results, matchup):
    """build.records per seat with the host rule's targets; rows the rule gives no record are taken out by zeroing their n_updates"""
    n = len(status)
    per_seat = []
    for s in (0, 1):
        t = [build.game_targets(status[g], results[g], matchup[g], s) for g in range(n)]
        keep = np.array([x is not None for x in t])
        value = np.array([x[0] if x else 0.0 for x in t], np.float32)
        score = np.array([-1.0 if x is None or x[1] is None else x[1] for x in t], np.float32)
        seat = dict(seats[s])
        seat["n_updates"] = np.where(keep, seats[s]["n_updates"], 0).astype(np.uint8)
        data = build.records(ctx, seat, value, score)
        rows = [g for g in range(n) if seat["n_updates"][g] > 0]
        assert len(data) == 128 * len(rows)
        per_seat.append({g: data[128 * i:128 * i + 128] for i, g in enumerate(rows)})
    return b"".join(per_seat[s][g] for g in range(n) for s in (0, 1) if g in per_seat[s])


@pytest.mark.parametrize("n", [1, 65, 257])
def test_game_records_equal_the_per_seat_records_interleaved(gpu_ctx, tmp_path, n):
    import torch
    seats = seats_of(gpu_ctx, tmp_path, n)
    status, results, matchup = game_outputs(n)
    want = referee(gpu_ctx, seats, status, results, matchup)
    built = sum(int((seats[s]["n_updates"] > 0).sum()) for s in (0, 1))
    assert 0 < len(want) // 128 <= built and (n == 1 or len(want) // 128 < built)      # (some built seats sit in dropped games)
    assert build.game_records(gpu_ctx, seats, status, results, matchup) == want       # numpy in: bytes out
    dev = torch.device("cuda", gpu_ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).to(dev)
    dseats = tuple({k: up(seat[k]) for k in ("teams_init", "sizes", "n_updates", "action", "prob")} for seat in seats)
    out = torch.full((2 * n, 128), 0xA5, dtype=torch.uint8, device=dev)
    records, count = build.game_records(gpu_ctx, dseats, up(status), up(results), up(matchup), out=out)
    torch.cuda.synchronize()
    assert records.data_ptr() == out.data_ptr() and int(count.item()) == len(want) // 128
    got = out.cpu().numpy().reshape(-1)
    assert got[:len(want)].tobytes() == want
    assert (got[len(want):] == 0xA5).all()                                             # the buffer beyond count is untouched


def test_the_values_and_scores_are_the_host_rules(gpu_ctx, tmp_path):
    n = 65
    seats = seats_of(gpu_ctx, tmp_path, n)
    status, results, matchup = game_outputs(n)
    recs = build.decode_records(build.game_records(gpu_ctx, seats, status, results, matchup))
    q, seen = 0, set()
    for g in range(n):
        for s in (0, 1):
            if seats[s]["n_updates"][g] == 0 or status[g] not in (OK, SKIPPED):
                continue
            value, score = build.game_targets(status[g], results[g], matchup[g], s)
            m = np.float32(matchup[g]) if s == 0 else np.float32(1.0 - matchup[g])
            assert value == float(m) and recs[q]["score"] == score and recs[q]["value"] == int(np.float32(m) * np.float32(65535.0)) / 65535.0, (g, s)
            if status[g] == SKIPPED:
                assert score is None
            else:
                first = {1: 1.0, 2: 0.0, 3: 0.5}[int(results[g]) & 15]
                assert score == (first if s == 0 else 1.0 - first)
            seen.add((int(status[g]), s, recs[q]["score"]))
            q += 1
    assert q == len(recs)
    assert {x[2] for x in seen if x[0] == OK} == {0.0, 0.5, 1.0} and {x[2] for x in seen if x[0] == SKIPPED} == {None}


def test_refusals(gpu_ctx, tmp_path):
    from oak_amd import _lib
    seats = seats_of(gpu_ctx, tmp_path, 1)
    with pytest.raises(ValueError, match="one row per game"):
        build.game_records(gpu_ctx, seats, np.zeros(2, np.uint8), np.zeros(2, np.uint8), np.zeros(2))
    with pytest.raises(_lib.OakGpuError, match="oakgpu_build_game_records_dev: null argument"):
        _lib.check(gpu_ctx.lib.oakgpu_build_game_records_dev(gpu_ctx.handle, None, None, None, None, None, 1, None, None))
