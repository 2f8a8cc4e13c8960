"""Test helper for the corpus evaluation (tests/test_corpus_eval_ref.py on the CPU, tests/test_gpu_corpus_eval.py on the GPU): the
chunk rule, the per-row terms of battle.py's loss (src/oak/battle.py:203-262) and the per-record sums restated in numpy -- in float64
as the yardstick, in float32 as the plain evaluation whose own error sizes the bound -- and the small corpus both test files use.
TEST INFRASTRUCTURE ONLY.

A row's inputs are what the GPU path reads: the evaluator's fp32 value and legal logits, the frame's targets as the training rows carry
them (u16 / 65535.0f in fp32), the record's score, and the weights rounded to fp32."""
import struct

import numpy as np

import replay_oracle as R

F = np.float32
OK, COUNT, ILLEGAL, EARLY_END, RESULT, MALFORMED = range(6)
DEFAULT_CHUNK_ROWS = 65536


# ---- chunks -------------------------------------------------------------------------------------------------------------------------
def chunks(frames, chunk_rows, malformed=None):
    """oakgpu_corpus_chunks restated: the first record of every chunk, then len(frames).  Raises ValueError naming the record that
    alone has more frames than chunk_rows."""
    chunk_rows = chunk_rows or DEFAULT_CHUNK_ROWS
    firsts, rows = [], 0
    for r, f in enumerate(frames):
        f = 0 if malformed is not None and malformed[r] else int(f)
        if f > chunk_rows:
            raise ValueError("record %d has %d frames, more than chunk_rows %d" % (r, f, chunk_rows))
        if r == 0 or rows + f > chunk_rows:
            firsts.append(r)
            rows = 0
        rows += f
    return firsts + [len(frames)]


# ---- records ------------------------------------------------------------------------------------------------------------------------
def frame_targets(rec, p):
    """The targets of the frame at byte p of a record: dict of m, n, iterations, empirical_value, nash_value (fp32) and emp / nash
    (fp32 [2, 9], zero behind the counts)."""
    m, n = (rec[p] & 15) + 1, (rec[p] >> 4) + 1
    it, ev, nv = struct.unpack_from("<IHH", rec, p + 3)
    probs = np.frombuffer(rec, "<u2", 2 * (m + n), p + 11).astype(F) / F(65535.0)
    emp, nash = np.zeros((2, 9), F), np.zeros((2, 9), F)
    emp[0, :m], nash[0, :m], emp[1, :n], nash[1, :n] = probs[:m], probs[m:2 * m], probs[2 * m:2 * m + n], probs[2 * m + n:]
    return {"m": m, "n": n, "iterations": it, "empirical_value": F(ev) / F(65535.0), "nash_value": F(nv) / F(65535.0), "emp": emp, "nash": nash}


def record_rows(rec):
    """(frame count, [byte offset of every frame]) of a well-formed record."""
    nf = struct.unpack_from("<H", rec, 4)[0]
    out, p = [], 391
    for _ in range(nf):
        out.append(p)
        p += R.update_bytes((rec[p] & 15) + 1, (rec[p] >> 4) + 1)
    return nf, out


def score(rec):
    return {1: 1.0, 2: 0.0, 3: 0.5}[rec[390] & 15]


# ---- the terms ----------------------------------------------------------------------------------------------------------------------
def side_terms(logit, k, emp, nash, pn, dtype=np.float64, variant=None):
    """(policy [9], ce, scale) of one side in `dtype`: softmax and log-softmax over the first k logits, the target mix
    (1 - pn) * emp + pn * nash, ce = -sum t * logp / max(1, #{t != 0}).  variant (the discrimination check): "swap" mixes nash and
    empirical the other way round, "k" divides by k instead of the support size.  scale = the largest |log-probability| the sum is
    made of (at least 1)."""
    T = dtype
    l = np.asarray(logit[:k], dtype=F).astype(T)
    pn = T(F(pn))
    sh = l - l.max()
    ex = np.exp(sh)
    s = ex.sum(dtype=T)
    policy = np.zeros(9, T)
    policy[:k] = ex / s
    logp = sh - np.log(s)
    e, n = np.asarray(emp[:k], F).astype(T), np.asarray(nash[:k], F).astype(T)
    if variant == "swap":
        e, n = n, e
    t = (T(1) - pn) * e + pn * n
    support = max(1, int((t != 0).sum())) if variant != "k" else k
    ce = (-t * logp).sum(dtype=T) / T(support)
    return policy, ce, max(1.0, float(np.abs(logp.astype(np.float64)).max()))


def row_terms(value, logits, tg, sc, w, dtype=np.float64, variant=None):
    """One row: value fp32, logits fp32 [2, 9], tg = frame_targets(...), sc = the record's score, w = (wn, we, ws, pn).
    -> {"policy" [2, 9], "sq_err", "ce" [2], "ce_scale" [2]} in `dtype`."""
    T = dtype
    wn, we, ws, pn = (T(F(x)) for x in w)
    vt = (wn * T(tg["nash_value"]) + we * T(tg["empirical_value"])) + ws * T(F(sc))
    d = T(F(value)) - vt
    out = {"sq_err": d * d, "policy": np.zeros((2, 9), T), "ce": np.zeros(2, T), "ce_scale": np.ones(2)}
    for s, k in enumerate((tg["m"], tg["n"])):
        out["policy"][s], out["ce"][s], out["ce_scale"][s] = side_terms(logits[s], k, tg["emp"][s], tg["nash"][s], pn, T, variant)
    return out


def bound(f32, f64, scale):
    """The project's rule (tests/policy_ref.bound): four times the plain fp32 evaluation's own distance from float64 on this row plus
    2e-7 of the row's scale."""
    return 4.0 * abs(float(f32) - float(f64)) + 2e-7 * scale


def record_sums(sq_err, ce, excluded, bases):
    """float64 sums over each record's included rows (excluded == 0) in frame order, and the counts of excluded == 0, 1, 2:
    (sums [records, 3], counts [records, 3])."""
    n = len(bases) - 1
    sums, counts = np.zeros((n, 3)), np.zeros((n, 3), np.int64)
    for r in range(n):
        for row in range(int(bases[r]), int(bases[r + 1])):
            x = int(excluded[row])
            counts[r, x] += 1
            if x == 0:
                sums[r] += (float(sq_err[row]), float(ce[row, 0]), float(ce[row, 1]))
    return sums, counts


def excluded_flags(world_records, status, bases, min_iterations):
    """The restatement of `excluded` per row: 2 for a row that is not OK, 1 for iterations < min_iterations, else 0."""
    out = np.zeros(int(bases[-1]), np.uint8)
    for r, rec in enumerate(world_records):
        if bases[r + 1] == bases[r]:
            continue
        _, offs = record_rows(rec)
        for f, p in enumerate(offs):
            row = int(bases[r]) + f
            out[row] = 2 if status[row] != OK else (1 if struct.unpack_from("<I", rec, p + 3)[0] < min_iterations else 0)
    return out


# ---- the corpus of the tests --------------------------------------------------------------------------------------------------------
_WORLD = {}
N_GAMES, N_SHORT = 12, 130


def with_sparse_targets(game, seed):
    """test_gpu_train_frames._with_targets with about half of every side's choices at probability zero in BOTH policies (a search
    that never visited them), so that the support size is below k on most frames."""
    from oak_amd.frames import write_frames
    rng = np.random.default_rng(seed)

    def pair(k):
        keep = rng.random(k) < 0.5
        keep[rng.integers(k)] = True
        out = []
        for _ in range(2):
            p = rng.dirichlet(np.ones(k)) * keep
            out.append(p / p.sum())
        return out
    ups = []
    for m, n, c1, c2 in game[2]:
        (e1, n1), (e2, n2) = pair(m), pair(n)
        ups.append({"m": m, "n": n, "c1": c1, "c2": c2, "iterations": int(rng.integers(1, 1 << 20)), "empirical_value": rng.random(),
                    "nash_value": rng.random(), "p1_empirical": e1, "p1_nash": n1, "p2_empirical": e2, "p2_nash": n2})
    return write_frames(game[0], game[1], ups)


def world():
    """The records both test files use, built on the CPU oracle: 12 random OU games (records 0..11; the odd ones with seeded targets,
    3 and 9 of them with sparse ones), a 0-frame and a 1-frame record (12, 13), 130 records cut to 1..5 frames (14..143, every third
    with targets, every sixth sparse), a COUNT, an ILLEGAL and a MALFORMED record made by test_gpu_train_frames._damaged (144..146), and
    a record whose result byte has no type (147).  -> (games, records)."""
    if "w" not in _WORLD:
        import oracle_lib as O
        from test_gpu_train_frames import _damaged, _with_targets
        b, _, _, _ = O.make_random_ou_batch(N_GAMES, seed0=0x5EED0000)
        games = [R.play_random_game(b[i], seed=i) for i in range(N_GAMES)]
        plain = [R.make_record(g[0], g[1], g[2]) for g in games]
        recs = [(with_sparse_targets if i in (3, 9) else _with_targets)(games[i], 100 + i) if i % 2 else plain[i] for i in range(N_GAMES)]
        recs += [R.make_record(games[1][0], 1, []), R.make_record(games[2][0], 2, games[2][2][:1])]
        for j in range(N_SHORT):
            g = games[j % N_GAMES]
            cut = (g[0], g[1], g[2][:1 + j % 5])
            recs.append((with_sparse_targets if j % 6 == 0 else _with_targets)(cut, 500 + j) if j % 3 == 0 else R.make_record(*cut))
        bad, kinds = _damaged(games, plain)
        recs += [bad[kinds.index(kind)] for kind in ("m", "c1", "malformed", "result")]
        _WORLD["w"] = (games, recs)
    return _WORLD["w"]
