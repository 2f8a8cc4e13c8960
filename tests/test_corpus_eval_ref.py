"""CPU: the host side of the corpus evaluation -- oakgpu_corpus_chunks against its restatement, the float64 restatement of the loss
terms (tests/corpus_eval_ref.py) against battle.py's formulas written out once more and against the variants it must tell apart, and
the new symbols in the library and the header.  No GPU."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import corpus_eval_ref as CE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("oakgpu_corpus_frame_bases", "oakgpu_corpus_chunks", "oakgpu_corpus_states_dev", "oakgpu_corpus_states", "oakgpu_corpus_inference_dev",
               "oakgpu_corpus_loss_dev", "oakgpu_corpus_inference", "oakgpu_corpus_evaluate")
W = (0.25, 0.25, 0.5, 0.25)                                              # wn, we, ws, pn: exact in fp32


def _lib():
    import __graft_entry__ as g
    g.build()
    from oak_amd import _lib
    return _lib, _lib.load()


def _chunks(lib_mod, lib, frames, chunk_rows, malformed=None):
    fr = np.ascontiguousarray(frames, dtype=np.uint16)
    mal = None if malformed is None else np.ascontiguousarray(malformed, dtype=np.uint8)
    count = C.c_uint32(0)
    mp = None if mal is None else mal.ctypes.data
    lib_mod.check(lib.oakgpu_corpus_chunks(fr.ctypes.data, mp, len(fr), chunk_rows, None, 0, C.byref(count)))
    firsts = np.full(count.value + 1, 0xFFFFFFFF, dtype=np.uint32)
    lib_mod.check(lib.oakgpu_corpus_chunks(fr.ctypes.data, mp, len(fr), chunk_rows, firsts.ctypes.data, len(firsts), C.byref(count)))
    return firsts.tolist()


def test_new_symbols_are_exported_and_declared():
    lib_mod, lib = _lib()
    header = open(os.path.join(ROOT, "include", "oakgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in lib_mod.SYMBOLS and getattr(lib, name) is not None, name
        assert name + "(" in header, name
    for name in ("oakgpu_corpus_eval", "oakgpu_loss_params", "oakgpu_corpus_terms", "oakgpu_corpus_losses"):
        assert "} %s;" % name in header, name
    from oak_amd.train import FrameCorpus
    for name in ("frame_bases", "states", "inference", "evaluate"):
        assert callable(getattr(FrameCorpus, name)), name
    from oak_amd import pyoak
    assert callable(pyoak.corpus_inference) and callable(pyoak.cpp_inference)


def test_chunks_follow_the_restatement():
    lib_mod, lib = _lib()
    rng = np.random.default_rng(1)
    cases = [([], 0, None), ([0], 5, None), ([5], 5, None), ([0, 0, 0], 1, None), ([1, 0, 0, 1, 1, 0], 1, None), ([0, 1, 0, 1], 1, None),
             ([3, 4, 5, 0, 5, 1, 4], 5, None), ([3, 4, 5, 0, 5, 1, 4], 9, None), ([7, 7, 7], 0, None), ([65535, 1, 65535], 0, None),
             ([9, 3, 9, 2], 5, [1, 0, 1, 0]), ([2, 2, 2], 4, [0, 1, 0])]
    for _ in range(40):
        n = int(rng.integers(1, 300))
        fr = rng.integers(0, 40, n)
        fr[rng.random(n) < 0.2] = 0
        mal = (rng.random(n) < 0.1).astype(np.uint8) if rng.random() < 0.5 else None
        top = int(np.where(mal == 1, 0, fr).max()) if mal is not None else int(fr.max())
        cases.append((fr.tolist(), int(rng.integers(max(top, 1), 200)), None if mal is None else mal.tolist()))
    for frames, chunk_rows, mal in cases:
        want = CE.chunks(frames, chunk_rows, mal)
        got = _chunks(lib_mod, lib, frames, chunk_rows, mal)
        assert got == want, (frames, chunk_rows, mal)
        limit = chunk_rows or 65536                                      # every chunk fits, and the next record would not have
        eff = [0 if mal is not None and mal[r] else f for r, f in enumerate(frames)]
        for a, b in zip(got[:-1], got[1:]):
            assert a < b and sum(eff[a:b]) <= limit
            assert b == len(frames) or sum(eff[a:b + 1]) > limit
    assert _chunks(lib_mod, lib, [1, 0, 0, 1, 1, 0], 1) == [0, 3, 4, 6]


def test_chunks_refuse_a_record_longer_than_the_chunk():
    lib_mod, lib = _lib()
    assert _chunks(lib_mod, lib, [4, 7, 2], 7) == [0, 1, 2, 3]              # exactly chunk_rows long: fits
    with pytest.raises(lib_mod.OakGpuError, match=r"record 1 has 8 frames, more than chunk_rows 7"):
        _chunks(lib_mod, lib, [4, 8, 2], 7)
    with pytest.raises(ValueError, match=r"record 1 has 8 frames"):
        CE.chunks([4, 8, 2], 7)
    assert _chunks(lib_mod, lib, [4, 8, 2], 7, [0, 1, 0]) == [0, 3]       # (a malformed record has no rows)
    with pytest.raises(lib_mod.OakGpuError, match="capacity"):
        fr = np.array([4, 7, 2], np.uint16)
        firsts, count = np.zeros(2, np.uint32), C.c_uint32(0)
        lib_mod.check(lib.oakgpu_corpus_chunks(fr.ctypes.data, None, 3, 7, firsts.ctypes.data, 2, C.byref(count)))


def _rows_with_targets():
    """(record, frame offset) of every frame of the test corpus' well-formed records, and seeded logits / values for them."""
    games, recs = CE.world()
    import replay_oracle as R
    rows = []
    for rec in recs:
        if R.check_record(rec) == "ok" and 1 <= (rec[390] & 15) <= 3:
            rows += [(rec, p) for p in CE.record_rows(rec)[1]]
    rng = np.random.default_rng(9)
    logits = (rng.standard_normal((len(rows), 2, 9)) * 3).astype(np.float32)
    values = rng.random(len(rows)).astype(np.float32)
    return rows, logits, values


def test_the_corpus_is_what_the_checks_need():
    games, recs = CE.world()
    import replay_oracle as R
    assert len(recs) == 148 and all(50 <= len(g[2]) <= 200 for g in games)
    assert [R.check_record(r) for r in recs[144:]] == ["ok", "ok", "malformed", "ok"] and recs[147][390] & 15 == 0
    assert [struct.unpack_from("<H", r, 4)[0] for r in recs[12:14]] == [0, 1]
    assert sorted({struct.unpack_from("<H", r, 4)[0] for r in recs[14:144]}) == [1, 2, 3, 4, 5]
    rows, _, _ = _rows_with_targets()
    tgs = [CE.frame_targets(rec, p) for rec, p in rows]
    assert any(t["m"] == 1 and t["emp"][0, 0] == 1 for t in tgs) and any(t["m"] == 9 or t["n"] == 9 for t in tgs)
    assert any(t["iterations"] == 0 for t in tgs) and any(t["iterations"] >= 2 for t in tgs) and any(not t["emp"].any() for t in tgs)


def test_terms_restate_battle_py():
    """The restatement against battle.py's lines written out directly in float64 on full nine-wide rows with -inf behind k, as torch
    sees them (masked_cross_entropy, loss: battle.py:203-209, 227-245)."""
    rows, logits, values = _rows_with_targets()
    for i in range(0, len(rows), 7):
        rec, p = rows[i]
        tg, sc = CE.frame_targets(rec, p), CE.score(rec)
        got = CE.row_terms(values[i], logits[i], tg, sc, W)
        wn, we, ws, pn = W
        vt = wn * float(tg["nash_value"]) + we * float(tg["empirical_value"]) + ws * sc
        assert abs(got["sq_err"] - (float(values[i]) - vt) ** 2) <= 1e-15
        for s, k in enumerate((tg["m"], tg["n"])):
            full = np.full(9, -np.inf)
            full[:k] = logits[i, s, :k].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                log_probs = full - full[:k].max() - np.log(np.exp(full - full[:k].max()).sum())
            log_probs[np.isneginf(log_probs)] = 0
            target = (1 - pn) * tg["emp"][s].astype(np.float64) + pn * tg["nash"][s].astype(np.float64)
            want = (-target * log_probs).sum() / max(1, int((target != 0).sum()))
            assert abs(got["ce"][s] - want) <= 1e-13 * max(1.0, abs(want))
            assert abs(got["policy"][s].sum() - 1) <= 1e-15 and not got["policy"][s, k:].any()
            assert np.abs(got["policy"][s, :k] - np.exp(log_probs[:k])).max() <= 1e-15


def test_terms_tell_the_variants_apart():
    """Mixing nash and empirical the other way round, or dividing by k instead of by the support size, moves the corpus sums by more
    than the bound the GPU test allows a row -- summed over the rows, so by far more than any row's bound."""
    rows, logits, values = _rows_with_targets()
    base = np.zeros(2)
    moved = {"swap": np.zeros(2), "k": np.zeros(2)}
    allowed = 0.0
    differs = {"swap": 0, "k": 0}
    for i, (rec, p) in enumerate(rows):
        tg, sc = CE.frame_targets(rec, p), CE.score(rec)
        if tg["iterations"] < 1:
            continue
        ref, f32 = CE.row_terms(values[i], logits[i], tg, sc, W), CE.row_terms(values[i], logits[i], tg, sc, W, dtype=np.float32)
        b = [CE.bound(f32["ce"][s], ref["ce"][s], ref["ce_scale"][s]) for s in range(2)]
        allowed += sum(b)
        base += ref["ce"]
        for variant in moved:
            other = CE.row_terms(values[i], logits[i], tg, sc, W, variant=variant)
            moved[variant] += other["ce"]
            differs[variant] += any(abs(other["ce"][s] - ref["ce"][s]) > b[s] for s in range(2))
    assert allowed > 0
    for variant in moved:
        assert np.abs(moved[variant] - base).max() > 100 * allowed, variant
        assert differs[variant] >= 50, (variant, differs[variant])      # and row by row: many rows sit outside their own bound


def test_record_sums_and_flags():
    sq = np.array([1, 2, 3, 4, 5], np.float32)
    ce = np.array([[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]], np.float32)
    sums, counts = CE.record_sums(sq, ce, np.array([0, 1, 0, 2, 0]), [0, 3, 3, 5])
    assert sums.tolist() == [[4, 6, 8], [0, 0, 0], [5, 9, 10]] and counts.tolist() == [[2, 1, 0], [0, 0, 0], [1, 0, 1]]
