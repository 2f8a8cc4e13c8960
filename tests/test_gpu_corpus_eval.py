"""GPU: a network evaluated on every frame of a corpus (oak_amd.train.FrameCorpus.states / inference / evaluate,
oak_amd/csrc/corpuseval.hip) -- the walked states byte for byte against the CPU oracle's walk, the evaluation bit for bit against the
plain leaf call on those states, the policies and loss terms against their float64 restatement tests/corpus_eval_ref.py, the sums
against float64 numpy sums of the returned terms, and the Python faces.

Measured on an MI355X (the worst ratio of |kernel - float64| to the bound 4 x |fp32 numpy - float64| + 2e-7 x scale, over the rows of
the test corpus, net_default): see profiles/r10_corpus_inference.json."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus_eval_ref as CE
import policy_ref as P
import train_ref as T
from hipmem import Dev
from oak_amd import _lib
from oak_amd.train import STATE_FIELDS, EncodedBattleFrames, FrameCorpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = (0.25, 0.25, 0.5, 0.25)                                              # wn, we, ws, pn: exact in fp32
_CACHE = {}


def _world(ctx):
    """(records, their oracle walks, the device corpus, frame bases, the states of every row)."""
    if "w" not in _CACHE:
        games, recs = CE.world()
        corpus = FrameCorpus(ctx, b"".join(recs))
        bases = corpus.frame_bases()
        _CACHE["w"] = (recs, T.Corpus(recs), corpus, bases, corpus.states(0, len(recs)))
    return _CACHE["w"]


def _net(ctx, tmp_path_factory, name):
    from oak_amd.engine import Network
    if name not in _CACHE:
        if name == "clamp":                                              # the quantized network of tests/test_gpu_discrete.py's default shape
            path = P.rewrite_net(P.GOLDEN["default"], str(tmp_path_factory.mktemp("nets") / "default_clamp.battle.net"), P.spread_main_net, header0=1)
        elif name == "wide":                                             # both heads' fc3 (weights and bias) times 2^8: logits spread over more than 88
            path = P.rewrite_net(P.GOLDEN["256"], str(tmp_path_factory.mktemp("nets") / "fc3x256.battle.net"), P.scale_heads(0, 8, fc3_bias=True))
        else:
            path = P.GOLDEN[name]
        _CACHE[name] = (Network(ctx, path=path, discrete=name == "clamp"), path)
    return _CACHE[name]


def _frames(bases):
    return np.diff(bases).astype(np.int64)


# ---- 1. states ----------------------------------------------------------------------------------------------------------------------
def test_states_are_the_oracle_walk(gpu_ctx):
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    info = corpus.info()
    assert int(bases[-1]) == info["frames"] and info["malformed"] == 1 and len(bases) == len(recs) + 1
    assert bases[147] == bases[146]                                      # the malformed record has no rows
    seen = set()
    for r in range(len(recs)):
        frames, verdict = tref.walked(r)
        nf = int(bases[r + 1] - bases[r])
        assert nf == (0 if verdict is not None and verdict[0] == T.MALFORMED else tref.frames(r))
        for f in range(nf):
            row = int(bases[r]) + f
            if f < len(frames):
                battle, dur, req, l1, l2, _ = frames[f]
                assert st["status"][row] == T.OK and st["where"][row] == f, (r, f)
                assert st["battles"][row].tobytes() == battle.tobytes() and st["durations"][row].tobytes() == dur.tobytes(), (r, f)
                assert st["results"][row] == req, (r, f)
                for side, l in (("p1", l1), ("p2", l2)):
                    assert st[side + "_counts"][row] == len(l) and st[side + "_choices"][row, :len(l)].tolist() == list(l), (r, f, side)
                    assert not st[side + "_choices"][row, len(l):].any()
            else:                                                        # from the verdict on: its status and frame, and zeros
                assert (st["status"][row], st["where"][row]) == verdict, (r, f)
                seen.add(verdict[0])
                for name in STATE_FIELDS:
                    if name not in ("status", "where"):
                        assert not st[name][row].any(), (r, f, name)
    assert seen == {T.COUNT, T.ILLEGAL, T.RESULT}
    # status / where are the training loader's for the same picks
    picks = np.array([(r, f) for r in range(len(recs)) for f in range(int(bases[r + 1] - bases[r]))], dtype=np.uint32)
    enc = EncodedBattleFrames(len(picks))
    corpus.encode(enc, picks)
    assert (enc.status == st["status"]).all() and (enc.where == st["where"]).all()


# ---- 2. chunk independence and edges ----------------------------------------------------------------------------------------------
def _guarded(rows, guard, fill):
    bufs = {name: Dev(np.zeros((rows + 2 * guard,) + tail, dtype=dt), fill=fill) for name, (tail, dt) in STATE_FIELDS.items()}
    ptrs = lambda row: [bufs[name].p.value + (guard + row) * int(np.prod(STATE_FIELDS[name][0], dtype=np.int64)) * np.dtype(STATE_FIELDS[name][1]).itemsize
                        for name in STATE_FIELDS]
    return bufs, ptrs


def _states_dev(ctx, corpus, bases, chunk_list, fill, guard=2, capacity=None):
    rows = int(bases[-1])
    bufs, ptrs = _guarded(rows, guard, fill)
    for first, n in chunk_list:
        crows = int(bases[first + n] - bases[first])
        _lib.check(ctx.lib.oakgpu_corpus_states_dev(ctx.handle, corpus.handle, first, n, crows if capacity is None else capacity,
                                                    *ptrs(int(bases[first]))))
    ctx.synchronize()
    out = {name: bufs[name].host() for name in STATE_FIELDS}
    for b in bufs.values():
        b.free()
    return out


def test_chunking_changes_nothing_and_nothing_outside_the_rows_is_touched(gpu_ctx):
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    fr, n = _frames(bases), len(recs)
    longest = int(fr.max())
    lists = {"one": [(0, n)], "longest": corpus.chunks(longest), "default": corpus.chunks(65536), "single": corpus.chunks(longest + 1)}
    assert lists["default"] == [(0, n)] and len(lists["longest"]) > 3
    assert [c for c in lists["longest"]] == [(a, b - a) for a, b in zip(CE.chunks(fr, longest)[:-1], CE.chunks(fr, longest)[1:])]
    assert any(k == 1 for _, k in lists["single"]) and any(k == 1 for _, k in lists["longest"])   # a boundary behind a single record
    for tag, chunk_list in lists.items():
        for fill in (0xFF, 0x00):                                        # every cell of the rows is written: the prefill does not show
            got = _states_dev(gpu_ctx, corpus, bases, chunk_list, fill, capacity=65536 if tag == "default" else None)
            for name in STATE_FIELDS:
                assert (got[name][:2].view(np.uint8) == fill).all() and (got[name][-2:].view(np.uint8) == fill).all(), (tag, name)
                assert got[name][2:-2].tobytes() == st[name].tobytes(), (tag, name)


def test_chunks_of_63_64_and_65_records(gpu_ctx):
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    for first, n in ((14, 63), (14, 64), (14, 65), (79, 65), (12, 2), (12, 1), (146, 1)):
        got = corpus.states(first, n)
        lo, hi = int(bases[first]), int(bases[first + n])
        for name in STATE_FIELDS:
            assert got[name].tobytes() == st[name][lo:hi].tobytes(), (first, n, name)


def test_a_capacity_below_the_chunk_is_refused_and_writes_nothing(gpu_ctx):
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    fr = _frames(bases)
    r = int(fr.argmax())
    bufs, ptrs = _guarded(int(fr[r]), 1, 0xFF)
    with pytest.raises(_lib.OakGpuError, match=r"records %d \.\. %d hold %d frames, more than rows_capacity %d" % (r, r, fr[r], fr[r] - 1)):
        _lib.check(gpu_ctx.lib.oakgpu_corpus_states_dev(gpu_ctx.handle, corpus.handle, r, 1, int(fr[r]) - 1, *ptrs(0)))
    gpu_ctx.synchronize()
    for name, b in bufs.items():
        assert (b.host().view(np.uint8) == 0xFF).all(), name
        b.free()
    with pytest.raises(_lib.OakGpuError, match="not all in the corpus"):
        corpus.states(len(recs) - 1, 2)
    with pytest.raises(_lib.OakGpuError, match=r"record %d has %d frames, more than chunk_rows %d" % (r, fr[r], fr[r] - 1)):
        corpus.chunks(int(fr[r]) - 1)


# ---- 3. inference equals the plain call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "default", "clamp"])
def test_inference_is_the_plain_call_on_the_chunk(gpu_ctx, tmp_path_factory, name):
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    net, path = _net(gpu_ctx, tmp_path_factory, name)
    out = corpus.inference(net)
    rows = int(bases[-1])
    assert out.value.shape == (rows, 1) and out.policy_logit.shape == (rows, 2, 9) and out.policy.shape == (rows, 2, 9)
    ok = st["status"] == T.OK
    v, l1, l2 = net.value_policy_inference(st["battles"], st["durations"], st["p1_choices"], st["p1_counts"], st["p2_choices"], st["p2_counts"])
    assert out.value[ok, 0].tobytes() == v[ok].tobytes()
    assert out.policy_logit[ok, 0].tobytes() == l1[ok].tobytes() and out.policy_logit[ok, 1].tobytes() == l2[ok].tobytes()
    assert (~ok).sum() > 100                                             # the rows that are not OK: zeros, whatever the evaluator made of a zero state
    for field in ("value", "policy_logit", "policy", "k", "choices"):
        assert not getattr(out, field)[~ok].any(), field
    assert (out.status == st["status"]).all() and (out.where == st["where"]).all()
    assert (out.k[:, 0] == st["p1_counts"]).all() and (out.k[:, 1] == st["p2_counts"]).all()
    assert (out.choices[:, 0] == st["p1_choices"]).all() and (out.choices[:, 1] == st["p2_choices"]).all()
    fr = _frames(bases)
    assert (out.picks[:, 0] == np.repeat(np.arange(len(recs)), fr)).all() and (out.picks[:, 1] == np.concatenate([np.arange(f) for f in fr])).all()
    # other chunk sizes: the plain call's row i does not depend on n (measured on the parent commit, profiles/r10_corpus_inference.json),
    # so the results are the same bits
    longest = int(fr.max())
    for chunk_rows in (longest, longest + 1):
        other = corpus.inference(net, chunk_rows=chunk_rows)
        for field in ("value", "policy_logit", "policy", "k", "choices", "status", "where"):
            assert getattr(other, field).tobytes() == getattr(out, field).tobytes(), (chunk_rows, field)
    part = corpus.inference(net, records=(14, 65))
    lo, hi = int(bases[14]), int(bases[79])
    assert part.value.tobytes() == out.value[lo:hi].tobytes() and part.policy.tobytes() == out.policy[lo:hi].tobytes()
    assert (part.picks == out.picks[lo:hi]).all()


def test_one_record_equals_cpp_inference(gpu_ctx, tmp_path_factory):
    """The old route, one zero-iteration search per frame, on a record with targets: the same value and legal logits (both go through
    the leaf evaluator; a batch of one and a batch of a chunk take the same kernels row by row) and the same policy to fp32 rounding
    (cpp_inference's softmax is the search's, in double)."""
    from oak_amd import pyoak
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    net, path = _net(gpu_ctx, tmp_path_factory, "default")
    r = 1
    assert st["results"][int(bases[r])] == 0x50                          # cpp_inference starts from None | Move | Move
    old = pyoak.cpp_inference(recs[r], path)
    new = corpus.inference(net, records=(r, 1))
    assert old["value"].shape == (tref.frames(r),) and new.value.shape == (tref.frames(r), 1)
    assert new.value[:, 0].tobytes() == old["value"].tobytes()
    assert new.policy_logit.tobytes() == old["policy_logit"].tobytes()
    assert np.abs(new.policy.astype(np.float64) - old["policy"]).max() <= 4e-7


# ---- 4. policies and terms against float64 ----------------------------------------------------------------------------------------
def _loss_dev(ctx, corpus, net, bases, first, n, w, min_iterations, want_out=True):
    """oakgpu_corpus_loss_dev on records first .. first + n - 1: (outputs by name, terms by name), host copies."""
    rows = int(bases[first + n] - bases[first])
    shapes = {"value": ((rows,), np.float32), "policy_logit": ((rows, 2, 9), np.float32), "policy": ((rows, 2, 9), np.float32), "k": ((rows, 2), np.uint8),
              "choices": ((rows, 2, 9), np.uint8), "status": ((rows,), np.uint8), "where": ((rows,), np.uint32)}
    tshapes = {"sq_err": ((rows,), np.float32), "ce": ((rows, 2), np.float32), "excluded": ((rows,), np.uint8), "record_sums": ((n, 3), np.float64),
               "record_counts": ((n, 3), np.uint32)}
    out = {k: Dev(np.zeros(s, d), fill=0xFF) for k, (s, d) in shapes.items()} if want_out else {}
    terms = {k: Dev(np.zeros(s, d), fill=0xFF) for k, (s, d) in tshapes.items()}
    po = _lib.CorpusEval(**{k: v.p.value for k, v in out.items()})
    pt = _lib.CorpusTerms(**{k: v.p.value for k, v in terms.items()})
    p = _lib.LossParams(*w, min_iterations)
    _lib.check(ctx.lib.oakgpu_corpus_loss_dev(ctx.handle, net.handle, corpus.handle, first, n, rows, C.byref(p), C.byref(po) if want_out else None, C.byref(pt)))
    ctx.synchronize()
    res = {k: v.host() for k, v in out.items()}, {k: v.host() for k, v in terms.items()}
    for b in list(out.values()) + list(terms.values()):
        b.free()
    return res


def _check_terms(recs, bases, out, terms, w, min_iterations):
    """Every row's policy, sq_err and ce against the float64 restatement fed the returned value and logits; returns the worst ratio of
    the error to its bound, per quantity."""
    worst = {"policy": 0.0, "sq_err": 0.0, "ce": 0.0}
    facts = {"k1_exact": 0, "zero_targets": 0, "included": 0}
    for r, rec in enumerate(recs):
        if bases[r + 1] == bases[r]:
            continue
        _, offs = CE.record_rows(rec)
        for f, p in enumerate(offs):
            row = int(bases[r]) + f
            if out["status"][row] != T.OK:
                assert terms["excluded"][row] == 2 and not terms["sq_err"][row] and not terms["ce"][row].any() and not out["policy"][row].any()
                continue
            tg = CE.frame_targets(rec, p)
            assert (out["k"][row] == (tg["m"], tg["n"])).all()
            ref = CE.row_terms(out["value"][row], out["policy_logit"][row], tg, CE.score(rec), w)
            f32 = CE.row_terms(out["value"][row], out["policy_logit"][row], tg, CE.score(rec), w, dtype=np.float32)
            for s, k in enumerate((tg["m"], tg["n"])):
                assert not out["policy"][row, s, k:].any() and np.isfinite(out["policy"][row, s]).all()
                for i in range(k):
                    b = CE.bound(f32["policy"][s, i], ref["policy"][s, i], 1.0)
                    worst["policy"] = max(worst["policy"], abs(float(out["policy"][row, s, i]) - ref["policy"][s, i]) / b)
                if k == 1:
                    assert out["policy"][row, s, 0] == 1.0
            included = tg["iterations"] >= min_iterations
            assert terms["excluded"][row] == (0 if included else 1)
            if not included:
                assert not terms["sq_err"][row] and not terms["ce"][row].any()
                continue
            facts["included"] += 1
            b = CE.bound(f32["sq_err"], ref["sq_err"], max(1.0, float(ref["sq_err"])))
            worst["sq_err"] = max(worst["sq_err"], abs(float(terms["sq_err"][row]) - ref["sq_err"]) / b)
            for s, k in enumerate((tg["m"], tg["n"])):
                assert np.isfinite(terms["ce"][row, s])
                b = CE.bound(f32["ce"][s], ref["ce"][s], ref["ce_scale"][s])
                worst["ce"] = max(worst["ce"], abs(float(terms["ce"][row, s]) - ref["ce"][s]) / b)
                t = (1 - np.float32(w[3])) * tg["emp"][s] + np.float32(w[3]) * tg["nash"][s]
                if k == 1 and t[0] == 1:                                 # one legal choice with the whole target: log 1
                    assert terms["ce"][row, s] == 0
                    facts["k1_exact"] += 1
                if not t.any():                                          # no target at all: the support clamps to 1
                    assert terms["ce"][row, s] == 0
                    facts["zero_targets"] += 1
    return worst, facts


@pytest.mark.parametrize("name,min_iterations", [("default", 1), ("default", 0), ("wide", 1)])
def test_policies_and_terms_against_float64(gpu_ctx, tmp_path_factory, name, min_iterations):
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    net, _ = _net(gpu_ctx, tmp_path_factory, name)
    out, terms = _loss_dev(gpu_ctx, corpus, net, bases, 0, len(recs), W, min_iterations)
    if name == "wide":                                                   # an unshifted expf would overflow: exp(88.7) is fp32's largest
        live = np.arange(9)[None, None, :] < out["k"][:, :, None]
        spread = np.where(live, out["policy_logit"], -np.inf).max(axis=2) - np.where(live, out["policy_logit"], np.inf).min(axis=2)
        assert spread[out["status"] == T.OK].max() > 88 and np.abs(out["policy_logit"]).max() > 88
    worst, facts = _check_terms(recs, bases, out, terms, W, min_iterations)
    print("corpus terms %s min_iterations=%d: worst error / bound %s; %s" % (name, min_iterations, json.dumps(worst), json.dumps(facts)))
    assert max(worst.values()) <= 1.0, worst
    assert facts["k1_exact"] > 0 and facts["included"] > 300
    if min_iterations == 0:
        assert facts["zero_targets"] > 100                               # the records without targets are in


# ---- 5. sums ------------------------------------------------------------------------------------------------------------------------
def test_record_sums_and_totals(gpu_ctx, tmp_path_factory):
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    net, _ = _net(gpu_ctx, tmp_path_factory, "default")
    n, fr = len(recs), _frames(bases)
    longest = int(fr.max())
    for min_iterations in (0, 1, 1 << 20):
        out, terms = _loss_dev(gpu_ctx, corpus, net, bases, 0, n, W, min_iterations)
        flags = CE.excluded_flags(recs, out["status"], bases, min_iterations)
        assert (terms["excluded"] == flags).all()
        sums, counts = CE.record_sums(terms["sq_err"], terms["ce"], terms["excluded"], bases)
        assert (terms["record_counts"] == counts).all()
        assert np.abs(terms["record_sums"] - sums).max() <= 1e-12 * max(1.0, np.abs(sums).max())
        assert (np.abs(terms["record_sums"] - sums) <= 1e-12 * np.maximum(np.abs(sums), 1e-300)).all()
        # chunked: the same bits, per record and in total
        per = []
        for first, k in corpus.chunks(longest) if min_iterations == 1 else corpus.chunks(longest + 1):
            _, t = _loss_dev(gpu_ctx, corpus, net, bases, first, k, W, min_iterations, want_out=False)
            per.append((t["record_sums"], t["record_counts"]))
        assert np.concatenate([p[0] for p in per]).tobytes() == terms["record_sums"].tobytes()
        assert np.concatenate([p[1] for p in per]).tobytes() == terms["record_counts"].tobytes()
        totals = [corpus.evaluate(net, *W, min_iterations=min_iterations, chunk_rows=c, per_record=True) for c in (0, longest, longest + 1)]
        want = np.zeros(3)
        for r in range(n):                                               # record order
            want += terms["record_sums"][r]
        for tot in totals:
            assert (tot["sq_err"], tot["ce1"], tot["ce2"]) == tuple(want)
            assert (tot["rows"], tot["excluded"], tot["failed"]) == tuple(int(x) for x in counts.sum(axis=0))
            assert tot["rows"] == int((flags == 0).sum()) and tot["excluded"] == int((flags == 1).sum()) and tot["failed"] == int((flags == 2).sum())
            d = max(tot["rows"], 1)
            assert (tot["mse"], tot["ce_p1"], tot["ce_p2"]) == (want[0] / d, want[1] / d, want[2] / d)
            assert [(x["sq_err"], x["ce1"], x["ce2"]) for x in tot["records"]] == [tuple(x) for x in terms["record_sums"]]
            assert [(x["rows"], x["excluded"], x["failed"]) for x in tot["records"]] == [tuple(x) for x in counts]
        if min_iterations == 1 << 20:
            assert totals[0]["rows"] == 0 and totals[0]["mse"] == 0


# ---- 6. Python faces ----------------------------------------------------------------------------------------------------------------
def test_torch_tensors_in_a_child_process():
    """FrameCorpus.inference into torch tensors on the device through tests/corpus_eval_check.py in a child process -- torch must
    initialise the GPU before the library does."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "corpus_eval_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "corpus eval ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_pyoak_corpus_inference_and_the_tool(gpu_ctx, tmp_path_factory, tmp_path):
    from oak_amd import pyoak
    recs, tref, corpus, bases, st = _world(gpu_ctx)
    net, path = _net(gpu_ctx, tmp_path_factory, "default")
    data = tmp_path / "games"
    data.mkdir()
    paths = [str(data / "a.battle.data"), str(data / "b.battle.data")]
    open(paths[0], "wb").write(b"".join(recs[:40]))
    open(paths[1], "wb").write(b"".join(recs[40:]))
    want = corpus.inference(net)
    got = pyoak.corpus_inference(paths, path)
    for field in ("value", "policy_logit", "policy", "k", "status", "where", "picks"):
        a = getattr(want, field)
        assert got[field].dtype == a.dtype and got[field].shape == a.shape and got[field].tobytes() == a.tobytes(), field
    one = pyoak.corpus_inference(recs[1], path)
    assert one["value"].tobytes() == want.value[int(bases[1]):int(bases[2])].tobytes()
    js = str(tmp_path / "out.json")
    tool = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate_battle_data.py"), str(data), "--network", path, "--value-nash-weight", "0.25",
                           "--value-empirical-weight", "0.25", "--value-score-weight", "0.5", "--p-nash-weight", "0.25", "--policy-loss-weight", "0.5",
                           "--per-record", "--json", js], capture_output=True, text=True, timeout=600)
    assert tool.returncode == 0, tool.stdout[-2000:] + tool.stderr[-4000:]
    rep = json.load(open(js))
    tot = corpus.evaluate(net, *W, min_iterations=1, per_record=True)
    assert (rep["mse"], rep["ce_p1"], rep["ce_p2"]) == (tot["mse"], tot["ce_p1"], tot["ce_p2"])
    assert rep["loss"] == tot["mse"] + 0.5 * (tot["ce_p1"] + tot["ce_p2"])
    assert (rep["rows"], rep["excluded"], rep["failed"], rep["records"], rep["malformed"]) == (tot["rows"], tot["excluded"], tot["failed"], len(recs), 1)
    assert rep["frames"] == int(bases[-1]) and rep["frames_per_s"] > 0 and len(rep["per_record"]) == len(recs)
    assert [x["sq_err"] for x in rep["per_record"]] == [x["sq_err"] for x in tot["records"]]
