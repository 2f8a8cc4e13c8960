"""CPU: the referee for a match's `.battle.data` records (tests/forest_match_records_ref.py) against the library's host code -- a searched
seat's update is oakgpu_selfplay_pick_host's update for the same output and joint choice, an unsearched seat's update decodes to the real m
and n with iterations 0, a record of mixed updates goes through frames.read_frames, the reference's 11-byte 0xFF form does not -- and the
refusals of the two new calls that need no device.  No GPU involved."""
import ctypes as C
import struct

import numpy as np
import pytest

import forest_match_records_ref as F
import forest_match_ref as M
import forestplay_ref as R
from oak_amd import _lib
from oak_amd._lib import OakGpuError
from oak_amd.frames import read_frames, selfplay_pick_host
from test_forestplay_ref import _cases


def test_a_searched_update_is_the_self_play_picks_update_for_the_same_output():
    seen = {"nash": 0, "plain": 0, "total": 0}
    for q, case in enumerate(_cases(512, 20311)):
        m, n = case["m"], case["n"]
        nash = q % 3 != 0
        kw = dict(p1_nash=case["p1_nash"], p2_nash=case["p2_nash"], nash_value=case["nash_value"]) if nash else {}
        try:
            got = selfplay_pick_host(m, n, case["visits"], case["values"], case["iterations"], case["rng"], p1_choices=case["c1"],
                                     p2_choices=case["c2"], **kw)
        except OakGpuError:
            continue
        c1, c2 = int(case["c1"][got["i"]]), int(case["c2"][got["j"]])
        want = F.searched_entry(m, n, c1, c2, case["iterations"], case["visits"], case["values"], **kw)
        assert want == got["update"], (q, m, n)
        assert len(want) == 11 + 4 * (m + n)
        seen["nash" if nash else "plain"] += 1
        seen["total"] += 1
    assert seen["nash"] > 100 and seen["plain"] > 50, seen


@pytest.mark.parametrize("m, n", [(1, 1), (1, 2), (9, 1), (1, 9), (4, 1)])
def test_an_unsearched_update_decodes_to_the_real_counts_and_zero_fields(m, n):
    u = F.unsearched_entry(m, n, 7, 3)
    assert len(u) == 11 + 4 * (m + n)
    rec = R.assemble_record(bytes(384), 1, [u])
    d = R.decode_update(R.split_updates(rec)[0])
    assert (d["m"], d["n"], d["c1"], d["c2"], d["iterations"], d["empirical_value"], d["nash_value"]) == (m, n, 7, 3, 0, 0, 0)
    assert not any(d["p1_empirical"]) and not any(d["p1_nash"]) and not any(d["p2_empirical"]) and not any(d["p2_nash"])


def _mixed_turns():
    """Both seats searched; seat p1 forced (a 1 x n root: only seat p2 searches); seat p2 forced; nobody has a choice.  process_output reads
    the m x n live cells only, so one root output serves every shape."""
    case = next(c for c in _cases(64, 977) if c["m"] > 2 and c["n"] > 2)
    out = dict(iterations=case["iterations"], visits=case["visits"], values=case["values"], nash_value=case["nash_value"], p1_nash=case["p1_nash"],
               p2_nash=case["p2_nash"])
    m, n = case["m"], case["n"]
    return [dict(m=m, n=n, c1=1, c2=2, out=(out, out)), dict(m=1, n=n, c1=0, c2=5, out=(None, out)), dict(m=m, n=1, c1=4, c2=0, out=(out, None)),
            dict(m=1, n=1, c1=0, c2=0, out=(None, None))]


def test_a_record_of_mixed_updates_round_trips_through_read_frames():
    turns = _mixed_turns()
    battle = (np.arange(384) * 7 % 251).astype(np.uint8)
    for seat in (0, 1):
        rec = F.seat_record(seat, battle, M.OK, 2, turns)
        games = read_frames(rec)
        assert len(games) == 1 and games[0]["result"] == 2 and (games[0]["battle"] == battle).all()
        ups = games[0]["updates"]
        assert len(ups) == len(turns)
        for t, u in zip(turns, ups):
            assert (u["m"], u["n"], u["c1"], u["c2"]) == (t["m"], t["n"], t["c1"], t["c2"])
            searched = (t["n"] if seat else t["m"]) > 1
            assert (u["iterations"] > 0) == searched
            if not searched:
                assert u["empirical_value"] == 0 and u["nash_value"] == 0 and not u["p1_empirical"].any() and not u["p2_empirical"].any()
                assert not u["p1_nash"].any() and not u["p2_nash"].any()
        assert [len(x) for x in R.split_updates(rec)] == [11 + 4 * (t["m"] + t["n"]) for t in turns]
    # the two seats' records of one game: the same length, frame count, battle, result and per-frame (c1, c2, m, n)
    a, b = F.seat_record(0, battle, M.OK, 2, turns), F.seat_record(1, battle, M.OK, 2, turns)
    assert len(a) == len(b) and a != b
    key = lambda rec: [(u["c1"], u["c2"], u["m"], u["n"]) for u in read_frames(rec)[0]["updates"]]
    assert key(a) == key(b)


def test_the_early_stop_result_byte_and_the_games_without_a_record():
    turns = _mixed_turns()[:2]
    battle = np.zeros(384, np.uint8)
    for result in (M.WIN, M.LOSE):
        rec = F.seat_record(0, battle, M.EARLY_STOP, result, turns)
        g = read_frames(rec)[0]
        assert g["result"] == result and len(g["updates"]) == 2
    with pytest.raises(AssertionError):
        F.seat_record(0, battle, M.EARLY_STOP, 0, turns)
    assert F.seat_record(0, battle, M.MAX_TURNS, 0, turns) == b"" and F.seat_record(1, battle, M.ZERO_POLICY, 0xFF, turns) == b""
    empty = F.seat_record(1, battle, M.OK, 3, [])                # a game whose input was terminal: a record with 0 frames
    assert len(empty) == R.HEAD_BYTES and read_frames(empty)[0]["updates"] == [] and read_frames(empty)[0]["result"] == 3
    stream, offsets = F.pack([empty, b"", F.seat_record(0, battle, M.OK, 1, turns)])
    assert offsets.tolist() == [0, R.HEAD_BYTES, R.HEAD_BYTES, len(stream)] and len(read_frames(stream)) == 2


def test_the_references_unsearched_form_does_not_round_trip():
    """The departure on record: a value-initialised output is written as head byte 0xFF and 11 bytes; a reader takes 0xFF for m = n = 16."""
    ref = F.reference_unsearched_entry(0, 5)
    assert len(ref) == 11 and ref[0] == 0xFF
    good = F.unsearched_entry(1, 3, 0, 5)
    rec = R.assemble_record(bytes(384), 1, [ref, good])
    with pytest.raises((OakGpuError, AssertionError, struct.error)):
        got = read_frames(rec)
        ups = got[0]["updates"]
        assert [(u["m"], u["n"]) for u in ups] == [(1, 3), (1, 3)]
    with pytest.raises((AssertionError, struct.error)):
        R.split_updates(rec)
    assert len(read_frames(R.assemble_record(bytes(384), 1, [good, good]))[0]["updates"]) == 2


def test_the_new_calls_refuse_by_name_without_a_device():
    lib = _lib.load()
    with pytest.raises(OakGpuError, match="oakgpu_forest_match_set_records: null argument"):
        _lib.check(lib.oakgpu_forest_match_set_records(None, 1))
    size = C.c_size_t(0)
    with pytest.raises(OakGpuError, match="oakgpu_forest_match_records: null argument"):
        _lib.check(lib.oakgpu_forest_match_records(None, 0, None, 0, C.byref(size), None, None, None, None, 0))
