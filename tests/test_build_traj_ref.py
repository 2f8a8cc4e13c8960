"""CPU: the `.build.data` reader's referee (tests/build_traj_ref.py) against the reference's own arrays (tests/golden/build_traj_goldens.npz,
made by tests/golden/make_build_traj_goldens.py), the argument that the last read action need not be applied, the invariants on the records
the reference cannot supply arrays for (teams of six), the host form of oak_amd/csrc/build_traj.hpp (oakgpu_build_traj_check and the
stand-alone tests/cpp_build_traj_check.cc, plain and under sanitizers) against the referee, and the refusals of the corpus by name."""
import os
import subprocess

import numpy as np
import pytest

import build_ref as B
import build_traj_ref as T
from oak_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "build_traj_goldens.npz"))
OLD = np.load(os.path.join(ROOT, "tests", "golden", "build_goldens.npz"))
SEVEN = ("action", "mask", "policy", "value", "score", "start", "end")


def _seven(rows):
    """a list of per-record dicts -> the reference's seven arrays in its shapes"""
    n = len(rows)
    return {"action": np.stack([r["action"] for r in rows]).reshape(n, 31, 1), "mask": np.stack([r["mask"] for r in rows]),
            "policy": np.stack([r["policy"] for r in rows]).reshape(n, 31, 1), "value": np.array([[r["value"]] for r in rows], np.float32),
            "score": np.array([[r["score"]] for r in rows], np.float32), "start": np.array([[r["start"]] for r in rows], np.int64),
            "end": np.array([[r["end"]] for r in rows], np.int64)}


def _equal(got, mistake=None):
    return all(got[k].shape == G[k].shape and np.array_equal(got[k], G[k].astype(got[k].dtype)) for k in SEVEN)


def test_goldens_cover_what_they_promise():
    sizes = set()
    for r in G["records"]:
        _, _, _, action, prob = T.fields(r)
        start, end, swap, full = T.bounds(action, prob)
        sets = sum(1 for i in range(swap) if B.LIST[int(action[i])][1] == 0)
        assert swap == end or sets < 6            # the reference is defined on every golden record
        sizes.add(sets)
    assert sizes == {1, 2, 3, 4, 5}
    probs = G["records"][:, 4:].view("<u2").reshape(-1, 31, 2)[:, :, 1]
    assert (probs == 1).any() and (probs == 65535).any() and (G["records"][:, 1] == 255).any()
    assert G["policy"].dtype == np.float32 and G["action"].dtype == np.int64 and G["start"].dtype == np.int64


def test_referee_equals_the_reference_on_every_entry():
    rows = [T.decode(r) for r in G["records"]]
    assert all(r["status"] == T.OK for r in rows)
    assert _equal(_seven(rows))
    # the score of a record without one reads as 127.5 in the reference; no_score gives the -1 it meant and changes nothing else
    intended = [T.decode(r, no_score=True) for r in G["records"]]
    for r, a, b in zip(G["records"], rows, intended):
        assert b["score"] == (-1.0 if r[1] == 255 else a["score"]) and (a["score"] == 127.5) == (r[1] == 255)
        assert all(np.array_equal(a[k], b[k]) for k in ("action", "mask", "policy", "n_legal"))


@pytest.mark.parametrize("apply_last", (True, False))
def test_literal_restatement_equals_the_reference_with_and_without_the_last_action(apply_last):
    assert _equal(_seven([T.reference_write(r, apply_last) for r in G["records"]]))


def test_the_last_action_changes_nothing_on_teams_of_six_either():
    """In Python the seventh set is a list append, harmless: the arrays with and without it are the same, which is why it can be left out."""
    for r in OLD["records"]:
        a, b = T.reference_write(r, True), T.reference_write(r, False)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        d = T.decode(r)
        assert d["status"] == T.OK and all(np.array_equal(np.asarray(b[k]), np.asarray(d[k])) for k in b)


def _replay(record, row):
    """The invariants of one decoded record against build_ref.Rollout: returns the number of read steps checked."""
    _, _, _, action, prob = T.fields(record)
    start, end = row["start"], row["end"]
    cells = [int(a) for a in action[:start]]
    team, slots = np.zeros((6, 5), np.uint8), {}
    for c in cells:                              # the initial team: species in the order they come, moves in theirs
        s, m = (int(x) for x in B.LIST[c])
        if m == 0:
            slots[s] = len(slots)
            team[slots[s], 0] = s
        else:
            free = int(np.flatnonzero(team[slots[s], 1:] == 0)[0])
            team[slots[s], 1 + free] = m
    size = None
    for size in range(max(len(slots), 1), 7):    # the size is not in the record: the one whose rollout has as many steps
        r, k = B.Rollout(team.reshape(30), size), 0
        ok = True
        for i in range(start, end):
            legal = r.legal()
            if legal is None or int(action[i]) not in legal:
                ok = False
                break
            r.advance(legal.index(int(action[i])))
        if ok and r.legal() is None:
            break
    else:
        raise AssertionError("no size replays the record")
    r = B.Rollout(team.reshape(30), size)
    for i in range(start, end):
        legal, n = r.legal(), int(row["n_legal"][i])
        got = [int(c) for c in row["mask"][i, :n]]
        if r.swap:        # write_swaps lists EVERY set, the lead's too (trajectories.h:95-100); get_lead_swaps leaves the lead out
            legal_here = legal + [int(B.TABLE[r.team[0], 0])]
        else:
            legal_here = legal
        assert set(got) == set(legal_here) and len(got) == len(legal_here) and (row["mask"][i, n:] == -1).all()
        a = int(action[i])
        assert got[0] == a and row["action"][i] == a
        # otherwise in order: species cells ascending, then the sets in the order they joined the team, each set's moves ascending; at the
        # swap the sets in that order.  The exchange is the only departure from it.
        joined = []
        for c in action[:i]:
            if B.LIST[int(c)][1] == 0:
                joined.append(int(B.LIST[int(c)][0]))
        key = lambda c: (joined.index(int(B.LIST[c][0])),) if r.swap else ((0, c) if B.LIST[c][1] == 0 else (1, joined.index(int(B.LIST[c][0])), c))
        want = sorted(got, key=key)
        k = want.index(a)
        want[k], want[0] = want[0], want[k]
        assert got == want
        r.advance(legal.index(a))
    assert r.legal() is None
    return end - start


def test_old_records_six_of_them_teams_of_six_hold_the_invariants():
    checked = 0
    for rec in OLD["records"]:
        row = T.decode(rec)
        assert row["status"] == T.OK
        checked += _replay(rec, row)
    assert checked > 40


@pytest.mark.parametrize("mistake", ("apply_last", "species_past_full", "swap_species_order", "action_not_moved"))
def test_planted_mistakes_are_caught(mistake):
    if mistake == "apply_last":                   # a team of six: the seventh set is the reference's out-of-bounds write, TEAM_FULL here
        rows = [T.decode(r, mistake=mistake) for r in OLD["records"]]
        sound = [T.decode(r) for r in OLD["records"]]
        assert any(a["status"] != b["status"] or not np.array_equal(a["mask"], b["mask"]) for a, b in zip(rows, sound))
        assert sum(a["status"] == T.TEAM_FULL for a in rows) == 6
        return
    assert not _equal(_seven([T.decode(r, mistake=mistake) for r in G["records"]]))


def _all_records():
    bad = T.malformed_records()
    recs = np.concatenate([G["records"], OLD["records"], np.stack([r for _, _, r in bad]), T.rollout_records(150, 5)])
    return recs, bad


def test_malformed_records_have_their_status():
    bad = T.malformed_records()
    assert {s for _, s, _ in bad} == {T.BAD_ACTION, T.NO_SPECIES, T.TEAM_FULL, T.NOT_LEGAL, T.LIST_OVERFLOW}
    for name, status, rec in bad:
        row = T.decode(rec)
        assert row["status"] == status, name
        assert row["start"] == 0 and row["end"] == 0 and (row["action"] == -1).all() and (row["mask"] == -1).all() and not row["policy"].any()


def test_host_check_equals_the_referee():
    recs, _ = _all_records()
    want = T.status_of(recs)
    assert len(set(want.tolist())) == T.N_STATUS
    assert np.array_equal(build.check_records(recs.tobytes()), want)
    assert np.array_equal(build.check_records(recs), want)


def test_host_check_refusals():
    rec = G["records"][0].tobytes()
    for data, text in ((b"", "no records"), (rec[:-1], "127 bytes is not a multiple of 128"), (rec + b"\x01" + rec[1:], "record 1: format byte 1")):
        with pytest.raises(_lib.OakGpuError, match=text):
            build.check_records(data)


def test_corpus_refusals_by_name():
    class NoContext:
        lib, handle = _lib.load(), None
    rec = G["records"][:3].tobytes()
    wrong = rec[:256] + b"\x02" + rec[257:]
    for files, text in (([], "an empty corpus"), ([rec, b""], "file 1: an empty file"), ([rec, rec[:200]], "file 1: 200 bytes is not a multiple of 128"),
                        ([rec, wrong], "file 1, record 2: format byte 2")):
        with pytest.raises(_lib.OakGpuError, match=text):
            build.TrajectoryCorpus(NoContext, files)
    with pytest.raises(_lib.OakGpuError, match="null argument"):      # sound files get as far as the context
        build.TrajectoryCorpus(NoContext, [rec])


def _digest(row):
    weights = (np.arange(31, dtype=np.uint64)[:, None] + 1) * (np.arange(T.MAX_ACTIONS, dtype=np.uint64)[None, :] + 1)
    read = np.zeros(31, bool)
    read[row["start"]:row["end"]] = True
    return int(((weights * (row["mask"] + 1).astype(np.uint64))[read].sum()) % (1 << 32))


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitizers"))
def test_standalone_program(tmp_path, flags):
    recs, _ = _all_records()
    exe, data = str(tmp_path / "check"), str(tmp_path / "records.bin")
    subprocess.run(["g++", "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "cpp_build_traj_check.cc"), "-o", exe], check=True)
    open(data, "wb").write(recs.tobytes())
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    want = []
    for r in recs:
        row = T.decode(r)
        want.append((int(row["status"]), int(row["n_legal"].sum()), _digest(row)))
    assert got == want


def test_tables_are_what_the_header_relies_on():
    """LEGAL_SPECIES ascends (the bisection), a pool is the contiguous cells behind its species cell, and no pool has more than 64 moves."""
    assert B.LEGAL == sorted(B.LEGAL)
    for s in B.LEGAL:
        base = int(B.TABLE[s, 0])
        assert [int(B.TABLE[s, m]) for m in B.POOLS[s]] == list(range(base + 1, base + 1 + len(B.POOLS[s]))) and len(B.POOLS[s]) <= 64


def test_targets_referee_equals_get_state():
    rows = T.decode_many(np.concatenate([G["records"], OLD["records"]]))
    t = T.targets(rows, 0.75)
    state = T.get_state(rows["action"])[t["valid"]]
    assert state.shape == (len(t["rows"]), T.N_DIM)
    for v in range(len(t["rows"])):
        want = np.zeros(T.N_DIM, np.float32)
        want[t["state_cells"][v, :t["state_n"][v]]] = 1.0
        assert np.array_equal(state[v], want)
    assert (t["rewards"] != 0).sum() <= len(rows["end"]) and t["valid"].sum() == len(t["rows"])
