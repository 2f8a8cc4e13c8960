"""GPU: the replay window (oak_amd.train.ReplayWindow; oak_amd/csrc/replaywindow.hip; contract in include/oakgpu.h) against its referee: after
every append the window answers every corpus call as FrameCorpus does on the concatenation of the records tests/window_ref.py says survive.
  1. the window equals the freshly made corpus: info, frame_bases, records(), sample (picks and all 14 tensors, into 0xFF-prefilled buffers,
     at four filter pairs, the refusal of an empty eligible list included), encode on picks that name malformed and missing records,
     inference with net_tiny and evaluate's terms -- at record caps around a wave, a block and the scan's pass, byte caps that cut inside a
     batch and below a record, batches of 1, 64, 65 and 300 slices and an all-dropped one, through both entry points;
  2. the same appends give the same window, and a window depends on neither its capacity beyond the cut nor on what was evicted;
  3. tensors straight from forest_selfplay are appended without touching the host, and the replay check passes every record;
  4. the refusals that need a context."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import policy_ref as P
import window_ref as W
from oak_amd import _lib
from oak_amd.frames import forest_selfplay, replay_check_files
from oak_amd.train import EncodedBattleFrames, FIELDS, FrameCorpus, ReplayWindow
from test_oracle_goldens import benchmark_teams

pytestmark = pytest.mark.gpu
N_POOL, BUDGET, LENGTH_CAP = 48, 8, 110
ROWS = 97
BIG = 1 << 30
_CACHE = {}


def _games(n, salt=0):
    teams = np.stack([np.array(benchmark_teams(), dtype=np.uint8).reshape(60)] * n)
    battle_seeds = (np.arange(n, dtype=np.uint64) * np.uint64(0x2545F4914F6CDD1D) + np.uint64(8100 + salt)).astype(np.uint64)
    seeds = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(23 + salt)).astype(np.uint64)
    return teams, battle_seeds, seeds


def _pool(ctx):
    """One forest_selfplay of 48 games: (kept records as bytes, the call's five outputs)."""
    if "pool" not in _CACHE:
        teams, battle_seeds, seeds = _games(N_POOL)
        out = forest_selfplay(ctx, teams, battle_seeds, seeds, BUDGET, c=2.0, evaluator="poke-engine", policy_mode="e", solve_nash="device",
                              max_battle_length=LENGTH_CAP)
        stream, offsets = out[0], out[1]
        recs = [stream[int(offsets[g]):int(offsets[g + 1])] for g in range(N_POOL)]
        print("pool: frames %s, status %s" % (sorted(int(f) for f in out[2]), list(out[4])))
        assert any(len(r) == 0 for r in recs) and (out[4] != 0).any(), "no game of the pool was dropped: lower LENGTH_CAP"
        assert sum(1 for r in recs if r) >= 24
        _CACHE["pool"] = ([r for r in recs if r], out)
    return _CACHE["pool"]


def _net(ctx):
    if "net" not in _CACHE:
        from oak_amd.engine import Network
        _CACHE["net"] = Network(ctx, path=P.GOLDEN["tiny"])
    return _CACHE["net"]


def _batch(pool, rng, n, rejected=True, dropped=True):
    """n slices drawn from the pool (tiled and permuted), every 11th a damaged copy (each malformed class, both kinds of rejected length --
    below the fixed part, and not the slice's), every 17th a dropped game."""
    order = rng.permutation(len(pool))
    kinds = W.MALFORMED_KINDS + (W.REJECTED_KINDS if rejected else ())
    out = []
    for i in range(n):
        rec = pool[int(order[i % len(order)])]
        if dropped and i % 17 == 5:
            rec = b""
        elif i % 11 == 3:
            rec = W.damage(rec, kinds[int(rng.integers(len(kinds)))], rng)
        out.append(rec)
    return out


def _append(window, pieces, entry):
    if entry == "host":
        return window.append(b"".join(pieces))
    stream, offsets = W.slices(pieces)
    s = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy() if stream else np.zeros(1, np.uint8)).cuda()
    # (an odd byte in front: the batch starts at an odd address, as a record inside a stream does)
    s = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda"), s])
    return window.append(s, torch.from_numpy((offsets + np.uint64(1)).view(np.int64).copy()).cuda())


def _filled(n):
    enc = EncodedBattleFrames(n)
    for name in FIELDS:
        getattr(enc, name).view(np.uint8).fill(0xFF)
    enc.picks.view(np.uint8).fill(0xFF)
    return enc


def _same_rows(a, b, n, what):
    assert a.picks[:n].tobytes() == b.picks[:n].tobytes(), (what, "picks")
    for name in FIELDS:
        assert getattr(a, name)[:n].tobytes() == getattr(b, name)[:n].tobytes(), (what, name)


def _compare(ctx, window, ref, length_cap, seed):
    """Every corpus call on the window against FrameCorpus over the referee's bytes."""
    data = ref.bytes()
    assert window.records() == data and window.stats() == ref.stats()
    corpus = FrameCorpus(ctx, data)
    try:
        assert window.info() == corpus.info() == ref.info()
        assert (window.frame_bases() == corpus.frame_bases()).all()
        for max_len, min_it in ((0, 1), (0, BUDGET + 1), (length_cap, 1), (0, 1 << 30)):
            a, b = _filled(ROWS), _filled(ROWS)
            try:
                want = corpus.sample(b, seed, max_len, min_it)
            except _lib.OakGpuError as e:
                assert "no eligible record" in str(e)
                with pytest.raises(_lib.OakGpuError, match="no eligible record"):
                    window.sample(a, seed, max_len, min_it)
                continue
            assert window.sample(a, seed, max_len, min_it) == want == ROWS
            _same_rows(a, b, ROWS, ("sample", max_len, min_it))
            if max_len:
                assert (np.diff(corpus.frame_bases())[a.picks[:, 0]] <= max_len).all()
        n = len(ref.items)
        bad = [r for r, item in enumerate(ref.items) if item[2]][:8]
        picks = [(r, 0) for r in bad] + [(n + 3, 0), (0, 60000), (n, 0)] + [(r, 1) for r in range(0, n, max(1, n // 16))]
        picks = np.array(picks, dtype=np.uint32)
        a, b = _filled(len(picks)), _filled(len(picks))
        assert window.encode(a, picks) == corpus.encode(b, picks)
        _same_rows(a, b, len(picks), "encode")
        if n:
            net = _net(ctx)
            x, y = window.inference(net), corpus.inference(net)
            for name in ("value", "policy_logit", "policy", "k", "choices", "status", "where", "picks"):
                assert getattr(x, name).tobytes() == getattr(y, name).tobytes(), ("inference", name)
            assert window.evaluate(net, 0.25, 0.25, 0.5, 0.5, per_record=True) == corpus.evaluate(net, 0.25, 0.25, 0.5, 0.5, per_record=True)
            lo, k = n // 3, max(1, n // 4)
            sx, sy = window.states(lo, k), corpus.states(lo, k)
            assert all(sx[name].tobytes() == sy[name].tobytes() for name in sx)
    finally:
        corpus.close()


# the batches of a case: 1, 64, 65 and 300 slices, an all-dropped one, and enough behind them to pass 1,025 records
SIZES = (64, 1, 300, 65, -5, 300, 300, 300)


def _run(ctx, max_records, max_bytes, entry, sizes=SIZES, seed=1):
    pool, _ = _pool(ctx)
    rng = np.random.default_rng(1000 + seed)
    window, ref = ReplayWindow(ctx, max_records, max_bytes), W.Window(max_records, max_bytes)
    lengths = sorted(np.frombuffer(r[4:6], np.uint16)[0] for r in pool)
    try:
        for i, n in enumerate(sizes):
            pieces = [b""] * -n if n < 0 else _batch(pool, rng, n, rejected=entry == "dev", dropped=entry == "dev")
            ref.append(pieces)
            got = _append(window, pieces, entry)
            assert got == ref.stats(), (i, n)
            _compare(ctx, window, ref, int(lengths[len(lengths) // 2]), seed=77 + i)
        return ref.stats()
    finally:
        window.close()


# ---- 1. the window equals the freshly made corpus ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_records", [1, 63, 64, 65, 257, 1023, 1024, 1025])
def test_record_caps(gpu_ctx, max_records):
    st = _run(gpu_ctx, max_records, BIG, "dev")
    assert st["records"] == max_records and st["evicted"] > 0 and st["rejected"] > 0 and st["appends"] == len(SIZES)


@pytest.mark.parametrize("which", ["inside_a_batch", "below_a_record", "one_minimal_record"])
def test_byte_caps(gpu_ctx, which):
    pool, _ = _pool(gpu_ctx)
    sizes = sorted(len(r) for r in pool)
    # ~20 records (the cut falls inside every larger batch); the median record (a larger one empties the window); 391 bytes (nothing fits)
    max_bytes = {"inside_a_batch": 20 * sizes[len(sizes) // 2] + 7, "below_a_record": sizes[len(sizes) // 2], "one_minimal_record": 391}[which]
    st = _run(gpu_ctx, 1 << 20, max_bytes, "dev", sizes=(64, 1, 65, -5, 300, 1, 1, 1, 1, 1, 1), seed=2)
    assert st["bytes"] <= max_bytes and st["evicted"] > 0 and (which != "one_minimal_record" or st["records"] == 0)


@pytest.mark.parametrize("max_records,max_bytes", [(65, BIG), (1024, BIG), (1 << 20, 50000)])
def test_host_bytes_give_the_same_window(gpu_ctx, max_records, max_bytes):
    st = _run(gpu_ctx, max_records, max_bytes, "host", seed=3)
    assert st["rejected"] == 0 and st["evicted"] > 0
    # and the two entry points on the same batches
    pool, _ = _pool(gpu_ctx)
    rng = np.random.default_rng(5)
    a, b = ReplayWindow(gpu_ctx, max_records, max_bytes), ReplayWindow(gpu_ctx, max_records, max_bytes)
    for n in (65, 300, 64, 300):
        pieces = _batch(pool, rng, n, rejected=False, dropped=False)
        assert _append(a, pieces, "dev") == _append(b, pieces, "host")
    assert a.records() == b.records() and a.info() == b.info()
    ea, eb = _filled(ROWS), _filled(ROWS)
    assert a.sample(ea, 9) == b.sample(eb, 9)
    _same_rows(ea, eb, ROWS, "dev against host")
    a.close()
    b.close()


def test_a_cut_tail_of_host_bytes_is_left_out(gpu_ctx):
    pool, _ = _pool(gpu_ctx)
    window = ReplayWindow(gpu_ctx, 8, BIG)
    data = pool[0] + pool[1] + pool[2][:-5]                     # (a cut record can only be the buffer's last)
    st = window.append(data)
    assert (st["records"], st["appended"], st["rejected"]) == (2, 2, 0) and window.records() == pool[0] + pool[1]
    plain = FrameCorpus(gpu_ctx, data)
    assert window.info() == plain.info()
    plain.close()
    window.close()


# ---- 2. independence and repeatability -----------------------------------------------------------------------------------------------
def test_windows_repeat_and_do_not_remember(gpu_ctx):
    pool, _ = _pool(gpu_ctx)
    rng = np.random.default_rng(6)
    b1, b2, b3, other = (_batch(pool, rng, n) for n in (65, 64, 100, 300))
    first, again, short, wide = (ReplayWindow(gpu_ctx, *caps) for caps in ((64, BIG), (64, BIG), (64, BIG), (257, 600000)))
    for w, batches in ((first, (b1, b2, b3)), (again, (b1, b2, b3)), (short, (other, b3)), (wide, (other, b1, b3))):
        for pieces in batches:
            _append(w, pieces, "dev")
    data = first.records()
    assert first.info()["records"] == 64 and again.records() == data and short.records() == data and wide.records().endswith(data)
    rows = []
    for w in (first, again, short):
        enc = _filled(ROWS)
        assert w.sample(enc, 4242, 0, 1) == ROWS
        rows.append(enc)
    _same_rows(rows[0], rows[1], ROWS, "the same appends")
    _same_rows(rows[0], rows[2], ROWS, "other evicted records")
    for w in (first, again, short, wide):
        w.close()


# ---- 3. straight from self-play ------------------------------------------------------------------------------------------------------
def test_tensors_from_selfplay_are_appended_on_the_device(gpu_ctx, tmp_path):
    _, want = _pool(gpu_ctx)
    teams, battle_seeds, seeds = _games(N_POOL)
    dev = torch.device("cuda:0")
    out = forest_selfplay(gpu_ctx, torch.from_numpy(teams).to(dev), torch.from_numpy(battle_seeds.view(np.int64)).to(dev),
                          torch.from_numpy(seeds.view(np.int64)).to(dev), BUDGET, c=2.0, evaluator="poke-engine", policy_mode="e", solve_nash="device",
                          max_battle_length=LENGTH_CAP)
    window = ReplayWindow(gpu_ctx, 1 << 16, BIG)
    st = window.append(out[0], out[1])
    status = out[4].cpu().numpy()
    kept = int((status == 0).sum())
    assert st == {"records": kept, "bytes": len(want[0]), "appended": kept, "evicted": 0, "rejected": 0, "appends": 1} and kept < N_POOL
    assert window.records() == want[0] and window.records(device=dev).cpu().numpy().tobytes() == want[0]
    path = str(tmp_path / "window.battle.data")
    assert window.save(path) == len(want[0])
    res = replay_check_files(gpu_ctx, [path])
    assert len(res["reports"]) == kept and (res["reports"]["status"] == 0).all() and res["files"][0]["stopped_at"] is None
    assert window.info() == {"records": kept, "malformed": 0, "frames": int(want[2][status == 0].sum()), "stopped_at": len(want[0])}
    window.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_argument(gpu_ctx):
    from oak_amd.engine import Context
    pool, _ = _pool(gpu_ctx)
    lib = gpu_ctx.lib
    for args, text in (((0, BIG), "max_records must be at least 1"), ((4, 390), "max_bytes is below one minimal record")):
        with pytest.raises(_lib.OakGpuError, match=text):
            ReplayWindow(gpu_ctx, *args)
    plain, window = FrameCorpus(gpu_ctx, pool[0]), ReplayWindow(gpu_ctx, 4, BIG)
    offsets = torch.zeros(4, dtype=torch.int64, device="cuda")
    stream = torch.zeros(16, dtype=torch.uint8, device="cuda")
    msg = lambda rc: (rc, lib.oakgpu_last_error().decode())
    rc, m = msg(lib.oakgpu_corpus_append_dev(gpu_ctx.handle, plain.handle, stream.data_ptr(), offsets.data_ptr(), 1))
    assert rc != 0 and "oakgpu_corpus_append_dev: corpus was not made by oakgpu_corpus_create_window" in m
    rc, m = msg(lib.oakgpu_corpus_append(gpu_ctx.handle, plain.handle, None, 0))
    assert rc != 0 and "oakgpu_corpus_append: corpus was not made by oakgpu_corpus_create_window" in m
    rc, m = msg(lib.oakgpu_corpus_append_dev(gpu_ctx.handle, window.handle, stream.data_ptr(), offsets.data_ptr() + 4, 1))
    assert rc != 0 and "offsets must be an 8-byte aligned device array" in m
    rc, m = msg(lib.oakgpu_corpus_append_dev(gpu_ctx.handle, window.handle, stream.data_ptr(), None, 1))
    assert rc != 0 and "offsets must be" in m
    other = Context(0)
    rc, m = msg(lib.oakgpu_corpus_append_dev(other.handle, window.handle, stream.data_ptr(), offsets.data_ptr(), 1))
    assert rc != 0 and "oakgpu_corpus_append_dev: corpus belongs to another ctx" in m
    size = C.c_size_t(0)
    rc, m = msg(lib.oakgpu_corpus_records(other.handle, window.handle, None, 0, C.byref(size), 0))
    assert rc != 0 and "oakgpu_corpus_records: corpus belongs to another ctx" in m
    other.close()
    assert window.stats() == {"records": 0, "bytes": 0, "appended": 0, "evicted": 0, "rejected": 0, "appends": 0}
    window.append(pool[0])
    buf = np.zeros(8, np.uint8)
    rc, m = msg(lib.oakgpu_corpus_records(gpu_ctx.handle, window.handle, buf.ctypes.data, 8, C.byref(size), 0))
    assert rc != 0 and "capacity is below the window's bytes" in m and size.value == len(pool[0])
    plain.close()
    window.close()
