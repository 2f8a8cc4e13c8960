"""GPU: training batches from `.battle.data` records (oak_amd.train, oak_amd/csrc/trainframes.hip) against their numpy restatement
tests/train_ref.py -- every tensor bit for bit -- and the sampling rule against its CPU restatement.  The restatement itself is held to
the reference's dense encoders in tests/test_train_ref.py."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import replay_oracle as R
import train_ref as T
from hipmem import Dev
from oak_amd import _lib
from oak_amd.train import EncodedBattleFrames, FrameCorpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORLD = {}


def _with_targets(game, seed):
    """A record of the game with iterations, values and probabilities drawn from a seeded generator (frames.write_frames)."""
    from oak_amd.frames import write_frames
    rng = np.random.default_rng(seed)
    ups = []
    for m, n, c1, c2 in game[2]:
        ups.append({"m": m, "n": n, "c1": c1, "c2": c2, "iterations": int(rng.integers(0, 1 << 20)) if rng.random() < 0.8 else 0,
                    "empirical_value": rng.random(), "nash_value": float(rng.integers(0, 2)), "p1_empirical": rng.dirichlet(np.ones(m)),
                    "p1_nash": rng.dirichlet(np.ones(m)), "p2_empirical": rng.dirichlet(np.ones(n)), "p2_nash": rng.dirichlet(np.ones(n))})
    return write_frames(game[0], game[1], ups)


def _world(ctx):
    """The corpus of these tests: 32 oracle-played random games (records 0..31, no targets), 6 of them again with targets (32..37), one
    self-play record (38), a 0-frame and a 1-frame record (39, 40); its restatement; its device copy."""
    if "w" not in _WORLD:
        from oak_amd.frames import selfplay_game
        from test_oracle_goldens import benchmark_teams
        b, _, _, _ = O.make_random_ou_batch(32, seed0=0x5EED0000)
        games = [R.play_random_game(b[i], seed=i) for i in range(32)]
        recs = [R.make_record(g[0], g[1], g[2]) for g in games]
        recs += [_with_targets(games[i], 100 + i) for i in (0, 3, 7, 12, 20, 31)]
        sp, _, _ = selfplay_game(ctx, np.array(benchmark_teams(), dtype=np.uint8), battle_seed=3000, iterations=128, batch=128, seed=1)
        recs += [sp, R.make_record(games[1][0], 1, []), R.make_record(games[2][0], 2, games[2][2][:1])]
        _WORLD["w"] = (games, recs, T.Corpus(recs), FrameCorpus(ctx, b"".join(recs)))
    return _WORLD["w"]


def _all_picks(tref, records=None):
    return np.array([(r, f) for r in (range(len(tref.records)) if records is None else records) for f in range(tref.frames(r))], dtype=np.uint32)


def _same(enc, exp, n, fields=tuple(T.FIELDS)):
    for name in fields:
        got = getattr(enc, name)[:n] if not isinstance(enc, dict) else enc[name][:n]
        assert got.dtype == exp[name].dtype and got.shape == exp[name].shape, name
        if got.tobytes() != exp[name].tobytes():
            bad = np.nonzero((got != exp[name]).reshape(n, -1).any(axis=1))[0]
            raise AssertionError("%s differs in %d rows, first %d" % (name, bad.size, bad[0]))


def test_corpus_info(gpu_ctx):
    games, recs, tref, corpus = _world(gpu_ctx)
    info = corpus.info()
    assert info == {"records": len(recs), "malformed": 0, "frames": sum(tref.frames(r) for r in range(len(recs))), "stopped_at": sum(map(len, recs))}
    assert sum(len(g[2]) for g in games) == 2802 and min(len(g[2]) for g in games) == 53 and max(len(g[2]) for g in games) == 195


def test_every_frame_of_the_corpus_in_one_call(gpu_ctx):
    games, recs, tref, corpus = _world(gpu_ctx)
    picks = _all_picks(tref)
    enc = EncodedBattleFrames(len(picks))
    assert corpus.encode(enc, picks) == len(picks)
    exp = tref.expected(picks)
    assert (exp["status"] == T.OK).all()
    _same(enc, exp, len(picks))
    # what the corpus exercises: forced switches, single choices, nine choices, duplicated moves, targets
    k = exp["k"][:, :, 0]
    dup = T.duplicated_move_sides(np.stack([tref.walked(int(r))[0][int(f)][0] for r, f in picks[:2802]]))
    assert (k == 1).any() and (k == 9).any() and dup[:, :, :2].any() and (exp["iterations"] != 0).any() and (exp["nash_policies"] != 0).any()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 257, 513])
def test_pick_counts(gpu_ctx, n):
    """Fewer picks than a wave, the wave's edges, several waves, more than one take per queue head (513 = 8 x 64 + 1); frame 0 and a record's last frame are among them."""
    games, recs, tref, corpus = _world(gpu_ctx)
    every = _all_picks(tref)
    rng = np.random.default_rng(n)
    picks = every[rng.integers(0, len(every), n)]
    picks[0] = (n % 32, 0)
    picks[-1] = (5, tref.frames(5) - 1)
    enc = EncodedBattleFrames(n)
    assert corpus.encode(enc, picks) == n
    _same(enc, tref.expected(picks), n)


def test_rows_depend_on_their_own_pick_alone(gpu_ctx):
    games, recs, tref, corpus = _world(gpu_ctx)
    every = _all_picks(tref)
    rng = np.random.default_rng(77)
    picks = every[rng.integers(0, len(every), 200)]
    picks[10] = picks[150]                                             # a duplicated pick
    one, two, perm = EncodedBattleFrames(200), EncodedBattleFrames(200), EncodedBattleFrames(200)
    corpus.encode(one, picks)
    corpus.encode(two, picks)
    order = rng.permutation(200)
    corpus.encode(perm, picks[order])
    for name in T.FIELDS:
        a = getattr(one, name)
        assert a.tobytes() == getattr(two, name).tobytes(), name
        assert (getattr(perm, name) == a[order]).all(), name
        assert (a[10] == a[150]).all(), name


def _device_frames(n, guard=1, fill=0xFF):
    """Device tensors of n rows with `guard` rows in front of and behind them, every byte `fill` (NaN as a float): (buffers by field,
    the oakgpu_encoded_frames pointing at row `guard`)."""
    bufs, ptrs = {}, {}
    for name, (tail, dt) in T.FIELDS.items():
        bufs[name] = Dev(np.zeros((n + 2 * guard,) + tail, dtype=dt), fill=fill)
        ptrs[name] = bufs[name].p.value + guard * int(np.prod(tail, dtype=np.int64)) * np.dtype(dt).itemsize
    return bufs, _lib.EncodedFrames(**ptrs)


def test_nan_prefilled_buffers_and_guard_bands(gpu_ctx):
    """The device entry point on buffers full of 0xFF: every cell of rows 0 .. n-1 is written (and finite), no byte outside them is."""
    games, recs, tref, corpus = _world(gpu_ctx)
    every = _all_picks(tref)
    n = 131
    picks = every[np.random.default_rng(5).integers(0, len(every), n)]
    picks[3], picks[60] = (len(recs) + 5, 0), (0, 60000)                # two rows that are not OK: zeros, not leftovers
    bufs, ptrs = _device_frames(n)
    dp = Dev(picks)
    _lib.check(gpu_ctx.lib.oakgpu_frames_encode_dev(gpu_ctx.handle, corpus.handle, dp.p, n, C.byref(ptrs)))
    gpu_ctx.synchronize()
    exp = tref.expected(picks)
    assert list(exp["status"][[3, 60]]) == [T.RANGE, T.RANGE]
    for name in T.FIELDS:
        host = bufs[name].host()
        assert (host[:1].view(np.uint8) == 0xFF).all() and (host[-1:].view(np.uint8) == 0xFF).all(), name
        if host.dtype == np.float32:
            assert np.isfinite(host[1:-1]).all(), name
        assert host[1:-1].tobytes() == exp[name].tobytes(), name
    for b in list(bufs.values()) + [dp]:
        b.free()


def test_encode_battles_on_every_encoder_state(gpu_ctx):
    """oakgpu_encode_battles_dev on embed_ref.all_states() (mid-game + planted: every encoder input), the golden states (duplicated moves
    with the last slot at PP 0, disabled slots) and states where both sides must switch."""
    import embed_ref as E
    import policy_ref as P
    b, d = E.all_states()
    g = np.load(os.path.join(ROOT, "tests", "golden", "train_goldens.npz"))
    both = b[:64].copy()
    for i in range(64):
        for s in range(2):
            E._put16(both[i], E._stored_of(both[i], s, 0) + 18, 0)
    b, d = np.concatenate([b, g["battles"], both]), np.concatenate([d, g["durations"], d[:64]])
    r = P.result_bytes(b)
    assert (r[-64:] == 0xA0).all() and b.shape[0] >= 16000
    finished = np.array([0x01, 0x02, 0x03], np.uint8)                  # finished battles: no choices, k = 0
    b, d, r = np.concatenate([b, b[:3]]), np.concatenate([d, d[:3]]), np.concatenate([r, finished])
    n = b.shape[0]
    db, dd, dr = Dev(b), Dev(d), Dev(r)
    bufs, ptrs = _device_frames(n)
    _lib.check(gpu_ctx.lib.oakgpu_encode_battles_dev(gpu_ctx.handle, db.p, dd.p, dr.p, n, ptrs.pokemon, ptrs.active, ptrs.hp, ptrs.choice_indices, ptrs.k))
    gpu_ctx.synchronize()
    exp = T.encode_states(b, d, r)
    assert (exp["k"][-3:] == 0).all() and (exp["choice_indices"][-3:] == T.POLICY_DIM).all()
    assert T.duplicated_move_sides(b).any() and (exp["k"][:, :, 0] == 9).any()
    for name in T.POSITION_FIELDS:
        host = bufs[name].host()
        assert (host[:1].view(np.uint8) == 0xFF).all() and (host[-1:].view(np.uint8) == 0xFF).all(), name
        _same({name: host[1:-1]}, exp, n, fields=(name,))
    for name in set(T.FIELDS) - set(T.POSITION_FIELDS):                 # the targets are not this call's
        assert (bufs[name].host().view(np.uint8) == 0xFF).all(), name
    for x in list(bufs.values()) + [db, dd, dr]:
        x.free()


def _damaged(games, recs):
    """(records, kinds): one damaged record of each kind, the damage at frame 5 of games 4..9 where it has a frame."""
    out, kinds = [], []
    for j, kind in enumerate(("m", "n", "c1", "c2", "early_end", "result", "malformed")):
        g = games[4 + j]
        fr = list(g[2])
        rec = bytearray(recs[4 + j])
        p = 391 + sum(R.update_bytes(m, n) for m, n, _, _ in fr[:5])
        if kind == "m":
            rec = bytearray(R.make_record(g[0], g[1], [(a % 9 + 1 if i == 5 else a, b, c, d) for i, (a, b, c, d) in enumerate(fr)]))
        elif kind == "n":
            rec = bytearray(R.make_record(g[0], g[1], [(a, b % 9 + 1 if i == 5 else b, c, d) for i, (a, b, c, d) in enumerate(fr)]))
        elif kind == "c1":
            rec[p + 1] = 0xFF
        elif kind == "c2":
            rec[p + 2] = 0xFE
        elif kind == "early_end":
            rec = bytearray(R.make_record(g[0], g[1], fr + [(1, 1, 1, 1), (1, 1, 1, 1)]))
        elif kind == "result":
            rec[390] = 0x50                                              # a request, not a result: there is no score
        elif kind == "malformed":
            struct.pack_into("<H", rec, 4, len(fr) + 1)                  # "frame count does not match the record"
        out.append(bytes(rec))
        kinds.append(kind)
    return out, kinds


def test_damaged_records(gpu_ctx):
    games, recs, tref, _ = _world(gpu_ctx)
    bad, kinds = _damaged(games, recs)
    mixed = recs[:3] + bad + recs[3:5]
    tbad = T.Corpus(mixed)
    corpus = FrameCorpus(gpu_ctx, b"".join(mixed))
    try:
        assert corpus.info()["malformed"] == 1
        nf = [tbad.frames(r) for r in range(len(mixed))]
        picks = np.array([(r, f) for r in range(len(mixed)) for f in range(nf[r] + 2)] + [(len(mixed), 0), (2 ** 32 - 1, 2 ** 32 - 1)], dtype=np.uint32)
        enc = EncodedBattleFrames(len(picks))
        ok = corpus.encode(enc, picks)
        exp = tbad.expected(picks)
        assert ok == int((exp["status"] == T.OK).sum())
        _same(enc, exp, len(picks))
        want = {"m": T.COUNT, "n": T.COUNT, "c1": T.ILLEGAL, "c2": T.ILLEGAL, "early_end": T.EARLY_END, "result": T.RESULT, "malformed": T.MALFORMED}
        for j, kind in enumerate(kinds):
            r = 3 + j
            st, wh = enc.status[picks[:, 0] == r], enc.where[picks[:, 0] == r]
            frames = picks[picks[:, 0] == r][:, 1]
            inside = frames < nf[r]
            assert (st[~inside] == (T.MALFORMED if kind == "malformed" else T.RANGE)).all(), kind
            if kind in ("m", "n", "c1", "c2"):                           # OK in front of the damage, the oracle's verdict from it on
                assert (st[inside & (frames < 5)] == T.OK).all() and (st[inside & (frames >= 5)] == want[kind]).all() and (wh[inside & (frames >= 5)] == 5).all()
            elif kind == "early_end":                                    # the game's own frames are fine; the appended ones come after its end
                assert (st[frames < nf[r] - 2] == T.OK).all() and (st[inside & (frames >= nf[r] - 2)] == T.EARLY_END).all()
                assert (wh[inside & (frames >= nf[r] - 2)] == nf[r] - 2).all()
            elif kind == "result":
                assert (st[inside] == T.RESULT).all() and (wh[inside] == nf[r]).all()
            else:
                assert (st == T.MALFORMED).all() and (wh == 0).all()
        for name in T.FIELDS:                                            # a row that is not OK is all zero
            if name not in ("status", "where"):
                assert not getattr(enc, name)[:len(picks)][enc.status[:len(picks)] != T.OK].any(), name
    finally:
        corpus.close()


def test_sampling_follows_the_cpu_draw_rule(gpu_ctx):
    games, recs, tref, corpus = _world(gpu_ctx)
    longest = max(tref.frames(r) for r in range(len(recs)))
    for seed, max_len, min_it in ((1, 0, 0), (0xFFFFFFFFFFFFFFF0, 120, 0), (7, 0, 1), (2 ** 40 + 3, longest - 1, 5000)):
        enc, small = EncodedBattleFrames(257), EncodedBattleFrames(64)
        assert corpus.sample(enc, seed, max_len, min_it) == 257 and corpus.sample(small, seed, max_len, min_it) == 64
        want = tref.draws(257, seed, max_len, min_it)
        assert (enc.picks == want).all() and (small.picks == want[:64]).all()      # draw i is the same at n = 64 and n = 257
        _same(enc, tref.expected(want), 257)
        for name in T.FIELDS:
            assert getattr(small, name).tobytes() == getattr(enc, name)[:64].tobytes(), name
        if max_len:
            assert all(tref.frames(int(r)) <= max_len for r in want[:, 0])
        assert (enc.iterations[:, 0] >= min_it).all()
        if min_it:
            assert set(want[:, 0]) <= set(range(32, 39))                             # only the records with targets have iterations


def test_sampling_is_uniform_over_records_and_frames(gpu_ctx):
    """8 eligible records, 65,536 draws: every record's count within 5 sigma of n / 8 (sigma = sqrt(n * 1/8 * 7/8) = 84.7: +-424), and
    inside one record every valid frame's count within 5 sigma of its binomial."""
    games, recs, tref, _ = _world(gpu_ctx)
    short = sorted(range(32), key=lambda r: tref.frames(r))[:8]
    sub = [recs[r] for r in short]
    tsub = T.Corpus(sub)
    corpus = FrameCorpus(gpu_ctx, b"".join(sub))
    n = 65536
    bufs, ptrs = _device_frames(n, guard=0, fill=0)
    dp = Dev(np.zeros((n, 2), np.uint32))
    try:
        _lib.check(gpu_ctx.lib.oakgpu_frames_sample_dev(gpu_ctx.handle, corpus.handle, n, 12345, 0, 0, dp.p, C.byref(ptrs)))
        gpu_ctx.synchronize()
        picks = dp.host()
        assert (bufs["status"].host() == T.OK).all()
        assert (picks[:4096] == tsub.draws(4096, 12345, 0, 0)).all()
        counts = np.bincount(picks[:, 0], minlength=8)
        assert counts.shape == (8,) and (np.abs(counts - n / 8) <= 424).all(), counts
        for r in range(8):
            v = tsub.frames(r)
            per = np.bincount(picks[picks[:, 0] == r][:, 1], minlength=v)
            assert per.shape == (v,), r
            sigma = np.sqrt(counts[r] * (1 / v) * (1 - 1 / v))
            assert (np.abs(per - counts[r] / v) <= 5 * sigma).all(), r
    finally:
        for x in list(bufs.values()) + [dp]:
            x.free()
        corpus.close()


def test_sampling_without_an_eligible_record_raises(gpu_ctx):
    games, recs, tref, corpus = _world(gpu_ctx)
    enc = EncodedBattleFrames(8)
    with pytest.raises(_lib.OakGpuError, match="no eligible record"):
        corpus.sample(enc, 1, max_battle_length=0, min_iterations=1 << 30)
    with pytest.raises(_lib.OakGpuError, match="no eligible record"):
        corpus.sample(enc, 1, max_battle_length=1, min_iterations=1)     # (the 1-frame record has no iterations)
    empty = FrameCorpus(gpu_ctx, b"")
    with pytest.raises(_lib.OakGpuError, match="no eligible record"):
        empty.sample(enc, 1, 0, 0)
    assert empty.encode(enc, np.array([(0, 0)], np.uint32)) == 0 and enc.status[0] == T.RANGE
    empty.close()


def test_training_rows_give_the_inference_value(gpu_ctx):
    """The encoded rows pushed through a float64 forward of net_default.battle.net the way the reference's torch mirror consumes them
    (dense first layers, hp masks: src/oak/torch.py:399-430) against oakgpu_leaf_eval of the same states: within the project's 1e-5
    leaf bound on every frame without a move held twice by an active (the sparse inference encoder counts such a move twice; the
    dense training encoder assigns it) -- those frames are counted, and must stay under 5 %."""
    import policy_ref as P
    from oak_amd.engine import Network
    games, recs, tref, corpus = _world(gpu_ctx)
    picks = _all_picks(tref, range(16))
    enc = EncodedBattleFrames(len(picks))
    corpus.encode(enc, picks)
    states = [tref.walked(int(r))[0][int(f)] for r, f in picks]
    b, d = np.stack([s[0] for s in states]), np.stack([s[1] for s in states])
    onet = P.NN.Net(P.GOLDEN["default"])
    act = (lambda x: np.maximum(x, 0.0)) if onet.activation == 1 else (lambda x: np.clip(x, 0.0, 1.0))
    f64 = lambda layer, x: x @ layer.W.astype(np.float64).T + layer.b.astype(np.float64)
    n = len(picks)
    xp = enc.pokemon[:, :, 1:].astype(np.float64)
    xa = np.concatenate([enc.active[:, :, 0], enc.pokemon[:, :, 0]], axis=2).astype(np.float64)
    hp = enc.hp.astype(np.float64)
    ep = act(f64(onet.p1, act(f64(onet.p0, xp)))) * (hp[:, :, 1:] != 0)
    ea = act(f64(onet.a1, act(f64(onet.a0, xa)))) * (hp[:, :, 0] != 0)
    sides = np.concatenate([hp[:, :, 0], ea, np.concatenate([hp[:, :, 1:], ep], axis=3).reshape(n, 2, -1)], axis=2)
    h = act(f64(onet.v2, act(f64(onet.fc1, act(f64(onet.fc0, sides.reshape(n, -1)))))))
    value = 1.0 / (1.0 + np.exp(-f64(onet.v3, h)[:, 0]))
    net = Network(gpu_ctx, path=P.GOLDEN["default"])
    leaf = net.value_inference(b, d).astype(np.float64)
    dup = T.duplicated_move_sides(b)[:, :, :2].any(axis=(1, 2))          # the active's own slots or its stored Pokemon's
    assert 0 < dup.sum() <= 0.05 * n, (int(dup.sum()), n)
    assert np.abs(value - leaf)[~dup].max() <= 1e-5


def test_pyoak_from_bytes_and_sample(gpu_ctx, tmp_path):
    """The pybind11 face: EncodedBattleFrames.from_bytes on one record equals the ctypes path on the picks (0, 0 .. frames-1); sample fills
    `size` rows that honour both filters; the indexer lists (offset, frame count) per record and follows prune."""
    from oak_amd import pyoak
    games, recs, tref, corpus = _world(gpu_ctx)
    rec = recs[33]                                                       # a record with targets
    nf = tref.frames(33)
    got = pyoak.EncodedBattleFrames.from_bytes(rec, nf + 3)
    one = FrameCorpus(gpu_ctx, rec)
    enc = EncodedBattleFrames(nf + 3)
    assert one.encode(enc, np.array([(0, f) for f in range(nf)], np.uint32)) == nf
    one.close()
    for name in T.FIELDS:
        a = getattr(got, name)
        assert a.dtype == getattr(enc, name).dtype and a.shape == getattr(enc, name).shape, name
        assert a.tobytes() == getattr(enc, name).tobytes(), name        # (rows behind the record's frames stay zero in both)
    with pytest.raises(RuntimeError, match="more frames"):
        pyoak.EncodedBattleFrames.from_bytes(rec, nf - 1)
    paths = [str(tmp_path / "a.battle.data"), str(tmp_path / "b.battle.data")]
    open(paths[0], "wb").write(b"".join(recs[32:36]))
    open(paths[1], "wb").write(b"".join(recs[36:41]))
    indexer = pyoak.SampleIndexer()
    assert [tuple(x) for x in indexer.get(paths[0])] == list(zip(np.cumsum([0] + [len(r) for r in recs[32:35]]).tolist(), [tref.frames(r) for r in range(32, 36)]))
    indexer.get(paths[1])
    assert indexer.size() == 2
    # the indexer's corpus is the two files in path order: its record i is record 32 + i here.  Records 32..37 carry iterations, the
    # self-play record (38) has 128 a frame, the 0-frame and 1-frame records (39, 40) have none
    lens = {r: tref.frames(r) for r in range(32, 41)}

    def drawn(frames, limit, min_iterations, eligible):
        assert eligible, "the case needs an eligible record"
        assert pyoak.sample(frames, indexer, 4, limit, min_iterations) == frames.size
        picks = frames.picks.astype(np.int64) + (32, 0)
        valid = {r: set(tref.valid_frames(r, min_iterations)) for r in lens}
        assert (frames.status == T.OK).all() and (frames.where == picks[:, 1]).all()
        assert set(picks[:, 0].tolist()) == set(eligible)              # (300 draws miss one of at most 7 records with p < 1e-19)
        for r, f in picks:
            assert (limit in (0, 1 << 20) or lens[r] <= limit) and f in valid[r], (r, f)
        assert (frames.iterations[:, 0] >= min_iterations).all()
        _same(frames, tref.expected(picks.astype(np.uint32)), frames.size)   # every row is its pick's row

    frames = pyoak.EncodedBattleFrames(300)
    limit = sorted(lens[r] for r in range(32, 38))[3]                    # both filters bite: longer records out, and 38..40
    drawn(frames, limit, 2000, [r for r in range(32, 38) if lens[r] <= limit])
    assert len({lens[r] for r in range(32, 38)}) == 6 and any(lens[r] > limit for r in range(32, 38))
    shortest = min(range(32, 38), key=lens.get)                          # a limit that leaves one record
    drawn(frames, lens[shortest], 2000, [shortest])
    drawn(frames, 0, 1, list(range(32, 39)))                             # no limit: the self-play record joins
    drawn(frames, 1 << 20, 1, list(range(32, 39)))                       # a limit no record can reach is no limit
    with pytest.raises(RuntimeError, match="no eligible record"):
        pyoak.sample(frames, indexer, 4, 0, 1 << 40)                     # (more iterations than a frame can hold)
    with pytest.raises(RuntimeError, match="no eligible record"):
        pyoak.sample(frames, indexer, 4, 1, 2000)                        # (the filters the other way round would find records)
    indexer.prune(paths[:1])
    assert indexer.size() == 1
    again = pyoak.EncodedBattleFrames(64)
    assert pyoak.sample(again, indexer, 1, 0, 1) == 64 and (again.iterations[:, 0] >= 1).all()
    frames.clear()
    assert not frames.pokemon.any() and not frames.status.any()


def test_torch_tensors_in_a_child_process():
    """oak_amd.train with torch tensors on the device (EncodedBattleFrames(size, "cuda:0"): sample, encode, encode_battles) through
    tests/train_frames_check.py in a child process -- torch must initialise the GPU before the library does."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "train_frames_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "train frames ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
