"""GPU: the replay check of `.battle.data` records (oakgpu_replay_records, k_replay_records) against its CPU restatement
tests/replay_oracle.py -- reports, and the battle and durations at every verdict, byte for byte."""
import os
import struct

import numpy as np
import pytest

import oracle_lib as O
import replay_oracle as R
from oak_amd.frames import replay_check, replay_check_files, replay_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ghost_battle(seed):
    from oak_amd import gamedata as G
    blunt = [94, G.match_move("hypnosis"), G.match_move("bodyslam"), G.match_move("leer"), G.match_move("growl")]
    b = O.init_battle([[blunt] * 6, [blunt] * 6], seed)
    O.update(b, 0, 0, O.Options())                                      # the opening update
    return b


_CORPUS = {}


def _oracle_corpus():
    """~600 random-play games stepped by the oracle (random OU pairs) + 4 Ghost-vs-Ghost stalemates to turn 1,000."""
    if "c" not in _CORPUS:
        b, _, _, _ = O.make_random_ou_batch(600, seed0=0x5EED0000)
        games = [R.play_random_game(b[i], seed=i) for i in range(600)]
        games += [R.play_random_game(_ghost_battle(77 + i), seed=9000 + i) for i in range(4)]
        recs = [R.make_record(g[0], g[1], g[2]) for g in games]
        _CORPUS["c"] = (games, recs)
    return _CORPUS["c"]


def _check_against_oracle(out, blob):
    exp, stop = R.replay_buffer(blob)
    assert out["stopped_at"] == stop and len(out["reports"]) == len(exp)
    for i, (off, (st, pl, fr, ex, got, b, d)) in enumerate(exp):
        rep = out["reports"][i]
        assert (int(rep["offset"]), rep["status"], rep["player"], rep["frame"], rep["expected"], rep["got"]) == (off, st, pl, fr, ex, got), i
        assert (out["battles"][i] == b).all() and (out["durations"][i] == d).all(), i


def test_oracle_played_corpus_replays_ok_in_one_call(gpu_ctx):
    games, recs = _oracle_corpus()
    blob = b"".join(recs)
    out = replay_check(gpu_ctx, blob, want_states=True)
    rep = out["reports"]
    assert len(rep) == len(games) and (rep["status"] == R.OK).all()
    assert list(rep["frame"]) == [len(g[2]) for g in games] and max(rep["frame"]) >= 999
    for i, g in enumerate(games):
        assert (out["battles"][i] == g[3]).all() and (out["durations"][i] == g[4]).all(), i


def test_selfplay_records_replay_ok(gpu_ctx):
    from oak_amd.frames import selfplay_game, selfplay_games
    from oak_amd.engine import Context
    from test_oracle_goldens import benchmark_teams
    teams = np.array(benchmark_teams(), dtype=np.uint8)
    blob = b""
    for g, (bandit, mode, ev) in enumerate((("ucb", "e", "mc"), ("exp3", "n", "mc"), ("ucb", "e0.9-x0.1", "poke-engine"))):
        rec, _, _ = selfplay_game(gpu_ctx, teams, battle_seed=3000 + g, iterations=128, batch=128, bandit=bandit,
                                  c=2.0 if bandit == "ucb" else 0.3, evaluator=ev, policy_mode=mode, seed=g + 1)
        blob += rec
    ctxs = [Context(0) for _ in range(2)]
    try:
        blob += b"".join(r[0] for r in selfplay_games(ctxs, np.stack([teams] * 2), [4000, 4001], [1, 2], iterations=128, batch=128))
    finally:
        for c in ctxs:
            c.close()
    out = replay_check(gpu_ctx, blob, want_states=True)
    assert len(out["reports"]) == 5 and (out["reports"]["status"] == R.OK).all()
    _check_against_oracle(out, blob)


def _frame_offsets(rec):
    frames = struct.unpack_from("<H", rec, 4)[0]
    offs, p = [], 391
    for _ in range(frames):
        offs.append(p)
        p += R.update_bytes((rec[p] & 15) + 1, (rec[p] >> 4) + 1)
    return offs


def _planted(games, recs, seed=5):
    """One damaged record of each kind (at a seeded frame of a seeded game) mixed with clean ones."""
    rng = np.random.default_rng(seed)
    long_games = [i for i, g in enumerate(games) if len(g[2]) >= 6]
    out, kinds = [], []

    def pick():
        i = int(rng.choice(long_games))
        rec = bytearray(recs[i])
        offs = _frame_offsets(rec)
        return i, rec, offs, int(rng.integers(1, len(offs)))
    for kind in ("m", "n", "c1_outside", "c2_outside", "c1_other_legal", "result", "drop_last", "append", "rng"):
        i, rec, offs, k = pick()
        p = offs[k]
        m, n = (rec[p] & 15) + 1, (rec[p] >> 4) + 1
        if kind == "m":                                                 # m -> m + 1 (9 -> 1), the frame's size with it
            rec = bytearray(R.make_record(games[i][0], games[i][1], [(m % 9 + 1 if j == k else a, b, c, d) for j, (a, b, c, d) in enumerate(games[i][2])]))
        elif kind == "n":
            rec = bytearray(R.make_record(games[i][0], games[i][1], [(a, n % 9 + 1 if j == k else b, c, d) for j, (a, b, c, d) in enumerate(games[i][2])]))
        elif kind == "c1_outside":
            rec[p + 1] = 0xFF
        elif kind == "c2_outside":
            rec[p + 2] = 0xFE
        elif kind == "c1_other_legal":
            b = np.array(games[i][0], np.uint8).copy()
            opt = O.Options()
            r = int(O.LIB.oracle_result_from_state(O.ptr(b)))
            for j, (_, _, c1, c2) in enumerate(games[i][2]):
                l1 = O.choices(b, 0, (r >> 4) & 3)
                if len(l1) > 1:
                    rec[offs[j] + 1] = int([x for x in l1 if x != c1][0])
                    break
                opt.set()
                r = int(O.update(b, c1, c2, opt))
        elif kind == "result":
            rec[390] ^= 0x03
        elif kind == "drop_last":
            rec = bytearray(R.make_record(games[i][0], games[i][1], games[i][2][:-1]))
        elif kind == "append":
            rec = bytearray(R.make_record(games[i][0], games[i][1], games[i][2] + [(1, 1, 1, 1)]))
        elif kind == "rng":
            rec[6 + 376 + int(rng.integers(0, 8))] ^= 0x5A                # battle.rng: the last 8 bytes of the battle
        out.append(bytes(rec))
        kinds.append(kind)
    return out, kinds


def test_planted_damage_is_reported_like_the_oracle(gpu_ctx):
    games, recs = _oracle_corpus()
    bad, kinds = _planted(games, recs)
    clean = recs[:40]
    blob = b"".join(clean[:20] + bad + clean[20:])
    out = replay_check(gpu_ctx, blob, want_states=True)
    _check_against_oracle(out, blob)
    st = out["reports"]["status"]
    assert (st[:20] == R.OK).all() and (st[20 + len(bad):] == R.OK).all()
    got = dict(zip(kinds, out["reports"][20:20 + len(bad)]))
    assert (got["m"]["status"], got["m"]["player"]) == (R.COUNT, 1)
    assert (got["n"]["status"], got["n"]["player"]) == (R.COUNT, 2)
    assert (got["c1_outside"]["status"], got["c1_outside"]["player"]) == (R.ILLEGAL, 1)
    assert (got["c2_outside"]["status"], got["c2_outside"]["player"]) == (R.ILLEGAL, 2)
    assert got["result"]["status"] == R.RESULT and got["drop_last"]["status"] == R.RESULT and (got["drop_last"]["got"] & 15) == 0
    assert got["append"]["status"] == R.EARLY_END


def test_reports_do_not_depend_on_the_batch(gpu_ctx):
    games, recs = _oracle_corpus()
    bad, _ = _planted(games, recs, seed=9)
    recs = recs[:120] + bad
    one = replay_check(gpu_ctx, b"".join(recs), want_states=True)
    fields = ("status", "player", "frame", "expected", "got")
    key = lambda o, i: tuple(int(o["reports"][f][i]) for f in fields) + (o["battles"][i].tobytes(), o["durations"][i].tobytes())
    ref = [key(one, i) for i in range(len(recs))]
    again = replay_check(gpu_ctx, b"".join(recs), want_states=True)
    assert [key(again, i) for i in range(len(recs))] == ref
    rev = replay_check(gpu_ctx, b"".join(recs[::-1]), want_states=True)
    assert [key(rev, i) for i in range(len(recs))][::-1] == ref
    singles = [key(replay_check(gpu_ctx, r, want_states=True), 0) for r in recs[:16] + recs[-9:]]
    assert singles == ref[:16] + ref[-9:]
    cuts = [0, 7, 8, 50, 51, 99, len(recs)]
    split = []
    for lo, hi in zip(cuts, cuts[1:]):
        o = replay_check(gpu_ctx, b"".join(recs[lo:hi]), want_states=True)
        split += [key(o, i) for i in range(hi - lo)]
    assert split == ref


def _shortest_singles(gpu_ctx):
    """The ~20 shortest games' records and the single-record replay of each (report fields, battle, durations)."""
    if "short" not in _CORPUS:
        games, recs = _oracle_corpus()
        short = [recs[i] for i in sorted(range(len(recs)), key=lambda i: len(games[i][2]))[:20]]
        singles = []
        for r in short:
            o = replay_check(gpu_ctx, r, want_states=True)
            singles.append((tuple(int(o["reports"][f][0]) for f in ("frame", "status", "player", "expected", "got")),
                            o["battles"][0].tobytes(), o["durations"][0].tobytes()))
        _CORPUS["short"] = (short, singles)
    return _CORPUS["short"]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 513])
def test_queue_take_hands_every_record_out_once(gpu_ctx, n):
    """The eight-head queue at its edges: fewer records than heads (heads whose limit is 0), a head that runs dry inside a take, a
    queue longer than one take per head (513 = 8 x 64 + 1).  A take that drops a record leaves its report at the fill; one that hands
    a record out twice or to the wrong lane shows as another record's report or state."""
    from hipmem import Dev
    from oak_amd import _lib
    short, singles = _shortest_singles(gpu_ctx)
    assert len({s[1] for s in singles}) == len(singles)                 # the games end in different states: a swap would show
    blob = b"".join(short[i % len(short)] for i in range(n))
    idx = replay_index(blob)
    assert len(idx["offsets"]) == n and not idx["malformed"].any()
    fill = 0xEE
    raw = np.dtype([("frame", "<u4"), ("status", "u1"), ("player", "u1"), ("expected", "u1"), ("got", "u1")])
    devs = [Dev(np.frombuffer(blob, np.uint8)), Dev(idx["offsets"]), Dev(idx["frames"]), Dev(idx["malformed"].astype(np.uint8)),
            Dev(np.zeros(n, raw), fill=fill), Dev(np.zeros((n, 384), np.uint8), fill=fill), Dev(np.zeros((n, 8), np.uint8), fill=fill)]
    try:
        _lib.check(gpu_ctx.lib.oakgpu_replay_records_dev(gpu_ctx.handle, *(d.p for d in devs[:4]), n, *(d.p for d in devs[4:])))
        gpu_ctx.synchronize()
        rep, battles, durations = (d.host() for d in devs[4:])
    finally:
        for d in devs:
            d.free()
    assert not (rep.view(np.uint8).reshape(n, 8) == fill).all(1).any()  # every report was written
    for i in range(n):
        got = (tuple(int(rep[f][i]) for f in ("frame", "status", "player", "expected", "got")), battles[i].tobytes(), durations[i].tobytes())
        assert got == singles[i % len(short)], i


def test_scale_gpu_built_corpus_with_one_percent_damaged():
    """65,536 games built on the GPU as tools/replay_bench.py builds them, 1 % damaged: through tests/replay_scale_check.py in a child
    process -- the corpus is played with torch tensors, and torch must initialise the GPU before the library does."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "replay_scale_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "replay scale ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_files_map_reports_to_file_and_offset(gpu_ctx, tmp_path):
    games, recs = _oracle_corpus()
    parts = [recs[0:30], recs[30:31], recs[31:90], recs[90:100]]
    paths = []
    for i, p in enumerate(parts):
        path = tmp_path / ("f%d.battle.data" % i)
        data = b"".join(p)
        if i == 2:
            data += recs[100][:len(recs[100]) // 2]                     # truncated mid-record
        path.write_bytes(data)
        paths.append(str(path))
    out = replay_check_files(gpu_ctx, paths, chunk_bytes=20000)
    rep = out["reports"]
    assert len(rep) == 100 and (rep["status"] == R.OK).all()
    for fi, p in enumerate(parts):
        sel = rep[rep["file"] == fi]
        assert list(sel["offset"]) == list(np.cumsum([0] + [len(r) for r in p[:-1]]))
        assert list(sel["frame"]) == [struct.unpack_from("<H", r, 4)[0] for r in p]
    assert [f["stopped_at"] for f in out["files"]] == [None, None, sum(len(r) for r in parts[2]), None]
    assert sum(f["records"] for f in out["files"]) == 100


def test_cli_oracle_and_extract(tmp_path):
    import json
    import subprocess
    import sys
    games, recs = _oracle_corpus()
    bad, kinds = _planted(games, recs, seed=13)
    (tmp_path / "clean").mkdir()
    (tmp_path / "clean" / "a.battle.data").write_bytes(b"".join(recs[:60]))
    cli = [sys.executable, os.path.join(ROOT, "tools", "verify_battle_data.py")]
    p = subprocess.run(cli + [str(tmp_path / "clean"), "--oracle", "32"], capture_output=True, text=True, timeout=600)
    s = json.loads(p.stdout)
    assert p.returncode == 0 and s["counts"]["OK"] == 60 and s["oracle"]["agree"] == s["oracle"]["checked"] == 32, p.stdout + p.stderr
    (tmp_path / "dirty").mkdir()
    (tmp_path / "dirty" / "b.battle.data").write_bytes(b"".join(recs[:10] + bad))
    p = subprocess.run(cli + [str(tmp_path / "dirty"), "--oracle", "8", "--extract", str(tmp_path / "x")], capture_output=True, text=True, timeout=600)
    s = json.loads(p.stdout)
    n_bad = sum(1 for k in kinds if k != "c1_other_legal")
    assert p.returncode == 1 and s["oracle"]["agree"] == s["oracle"]["checked"], p.stdout + p.stderr
    assert len(s["failures"]) >= n_bad
    ext = (tmp_path / "x" / "failures.battle.data").read_bytes()
    assert len(replay_index(ext)["offsets"]) == len(s["failures"]) and ext.count(bad[0]) == 1
