"""GPU: the `.battle.data` records of a match between two search agents (oakgpu_forest_match_set_records / _records, forestmatch.hip; the
contract is in include/oakgpu.h), held to the referee in tests/forest_match_records_ref.py, which wraps forest_match_ref.follow:
  1. both seats' streams, offsets and frame counts byte for byte, over agents, budgets, the Nash solve and the host tree search;
  2. an early stop keeps its frames and a result byte of 1 or 2, a game cut at max_turns has no record;
  3. the streams pass the replay check, the two seats agree on what was played, a loader skips exactly the unsearched turns;
  4. recording off is the call as it was, and the accessor refuses by name after it;
  5. a game's records do not depend on its neighbours;
  6. the pyoak and C++ faces and tools/search_match.py --dir."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import forest_match_records_ref as F
import forest_match_ref as M
from oak_amd import _lib
from oak_amd._lib import OakGpuError
from oak_amd.arena import search_games
from oak_amd.frames import read_frames, replay_check
from test_gpu_forest_match import MC8, PE8, PE16, late_states, network, openings, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = 200           # log capacity per game: above every game length met here (asserted)
N = 33
_CACHE = {}


def states(ctx):
    """N games that start late in a random playout of theirs (a few Pokemon left a side: they end within a few dozen turns), chosen from a
    pool so that in two of them seat p1 has one choice at the start and in two others seat p2 has (a forced switch after a faint: the
    other side can only wait).  No pool of N random late states is sure to hold one of each, so they are planted in rows 3, 4, 20 and 21."""
    if "states" not in _CACHE:
        pool = 160
        b, d, r, seeds = openings(ctx, pool, salt=11)
        seeds[5] ^= np.uint64(0x5555)            # (openings repeats game 2 as game 5: not here)
        parts = [late_states(ctx, b[q::4], d[q::4], r[q::4], back=back) for q, back in enumerate((5, 8, 12, 16))]
        for q, (lb, ld, lr) in enumerate(parts):
            b[q::4], d[q::4], r[q::4] = lb, ld, lr
        live = (r & 15) == 0
        m, n = ctx.choices(b, r, 0)[1].astype(int), ctx.choices(b, r, 1)[1].astype(int)
        p1_forced, p2_forced = np.flatnonzero(live & (m == 1) & (n > 1)), np.flatnonzero(live & (n == 1) & (m > 1))
        assert len(p1_forced) >= 2 and len(p2_forced) >= 2, (len(p1_forced), len(p2_forced))
        planted = list(p1_forced[:2]) + list(p2_forced[:2])
        rest = [g for g in np.flatnonzero(live) if g not in planted][:N - 4]
        order = rest[:3] + planted[:2] + rest[3:18] + planted[2:] + rest[18:]
        assert len(order) == N
        order = np.array(order)
        _CACHE["states"] = (b[order].copy(), d[order].copy(), r[order].copy(), seeds[order].copy())
    return _CACHE["states"]


def same_records(got, want):
    for s in (0, 1):
        stream = got[s]["stream"]
        assert np.asarray(got[s]["offsets"]).astype(np.uint64).tolist() == np.asarray(want[s]["offsets"]).astype(np.uint64).tolist(), s
        assert np.asarray(got[s]["n_frames"]).astype(np.uint32).tolist() == np.asarray(want[s]["n_frames"]).astype(np.uint32).tolist(), s
        assert len(stream) == len(want[s]["stream"]), (s, len(stream), len(want[s]["stream"]))
        if stream != want[s]["stream"]:
            at = next(i for i in range(len(stream)) if stream[i] != want[s]["stream"][i])
            game = int(np.searchsorted(np.asarray(want[s]["offsets"]).astype(np.int64), at, side="right")) - 1
            raise AssertionError("seat p%d: the streams differ at byte %d (game %d, byte %d of its record)" % (s + 1, at, game, at - int(want[s]["offsets"][game])))


def record_of(rec, g):
    return rec["stream"][int(rec["offsets"][g]):int(rec["offsets"][g + 1])]


def reference(ctx):
    """The N games, PokeEngine at 16 iterations against Monte-Carlo at 8 with the Nash solve, no early stop; played once with recording on."""
    if "ref" not in _CACHE:
        b, d, r, seeds = states(ctx)
        stats = {}
        out = search_games(ctx, (PE16, MC8), b, d, r, seeds, log_turns=LOG, stats=stats, records=True)
        assert int(out["turns"].max()) < LOG, out["turns"]
        _CACHE["ref"] = (out, stats)
    return _CACHE["ref"]


# ---- 1. byte for byte against the referee --------------------------------------------------------------------------------------------------
def test_ucb_pokeengine_against_monte_carlo_is_the_referees(gpu_ctx):
    b, d, r, seeds = states(gpu_ctx)
    out, stats = reference(gpu_ctx)
    assert (out["status"] == M.OK).all(), out["status"]
    census, want = F.follow_records(gpu_ctx, (PE16, MC8), b, d, r, seeds, out)
    print("pe16 against mc8: %d games, turns %s, stats %s, census %s, %d bytes a seat" % (N, out["turns"].tolist(), stats, census, len(out["records"][0]["stream"])))
    same_records(out["records"], want)
    assert census["m1"] > 0 and census["n1"] > 0 and census["both"] > 0, census
    assert census["first_unsearched"][0] >= 2 and census["first_unsearched"][1] >= 2, census
    assert out["records"][0]["stream"] != out["records"][1]["stream"]            # each seat stores its own search


@pytest.mark.parametrize("case", ["pucb-tiny", "budgets-no-nash", "host"])
def test_other_agents_are_the_referees(gpu_ctx, tmp_path, case):
    from oak_amd.search import Forest
    b, d, r, seeds = states(gpu_ctx)
    net, forest, host, solve_nash = None, None, False, True
    if case == "pucb-tiny":                      # PUCB + the golden tiny net against UCB, on a contextual forest, unequal budgets and modes
        rows = np.arange(2, 9)
        net = network(gpu_ctx, tmp_path, "tiny")
        seats = (dict(iterations=8, bandit="pucb", c=1.5, evaluator=net, policy_mode="p0.5-n0.5"), dict(PE16, policy_mode="e0.9-x0.1"))
        forest = Forest(gpu_ctx, 16, 16, contextual=True)
    elif case == "budgets-no-nash":              # different budgets, the Nash fields stored as zeros
        rows, seats, solve_nash = np.arange(17, 26), (PE8, dict(PE16, c=1.0)), False
    else:                                        # three games, the host tree search in the forest's place
        rows, seats, host = np.array([3, 20, 30]), (PE16, MC8), True
    gb, gd, gr, gs = b[rows], d[rows], r[rows], seeds[rows]
    out = search_games(gpu_ctx, seats, gb, gd, gr, gs, forest=forest, log_turns=LOG, solve_nash=solve_nash, records=True)
    assert int(out["turns"].max()) < LOG and (out["status"] == M.OK).all(), (out["turns"], out["status"])
    census, want = F.follow_records(gpu_ctx, seats, gb, gd, gr, gs, out, solve_nash=solve_nash, host=host)
    print("%s: turns %s census %s" % (case, out["turns"].tolist(), census))
    same_records(out["records"], want)
    assert census["both"] > 0 and census["m1"] + census["n1"] > 0, census
    if not solve_nash:
        for game in read_frames(out["records"][0]["stream"]):
            assert all(u["nash_value"] == 0 and not u["p1_nash"].any() and not u["p2_nash"].any() for u in game["updates"])
    if forest is not None:
        forest.close()
    if net is not None:
        net.close()


# ---- 2. the early stop, max_turns -------------------------------------------------------------------------------------------------------------
def test_an_early_stop_keeps_its_frames_and_a_cut_game_has_no_record(gpu_ctx):
    b, d, r, seeds = states(gpu_ctx)
    n = 16
    pe = dict(iterations=8, bandit="ucb", c=2.0, evaluator="poke-engine")
    out = search_games(gpu_ctx, (pe, pe), b[:n], d[:n], r[:n], seeds[:n], log_turns=LOG, early_stop=0.5, records=True)
    census, want = F.follow_records(gpu_ctx, (pe, pe), b[:n], d[:n], r[:n], seeds[:n], out, early_stop=0.5)
    print("early stop 0.5: status %s results %s turns %s census %s" % (out["status"].tolist(), out["results"].tolist(), out["turns"].tolist(), census))
    stopped = np.flatnonzero(out["status"] == M.EARLY_STOP)
    assert len(stopped) > 0 and census["early_win"] + census["early_lose"] == len(stopped)
    same_records(out["records"], want)
    for s in (0, 1):
        games = read_frames(out["records"][s]["stream"])
        assert len(games) == n
        for g in stopped:
            assert len(games[g]["updates"]) == int(out["turns"][g]) == int(out["records"][s]["n_frames"][g])
            assert games[g]["result"] in (M.WIN, M.LOSE) and games[g]["result"] == int(out["results"][g])
    cut = search_games(gpu_ctx, (pe, pe), b[:n], d[:n], r[:n], seeds[:n], log_turns=LOG, max_turns=2, records=True)
    census, want = F.follow_records(gpu_ctx, (pe, pe), b[:n], d[:n], r[:n], seeds[:n], cut, max_turns=2)
    gone = np.flatnonzero(cut["status"] == M.MAX_TURNS)
    assert len(gone) > 0 and census["cut"] == len(gone)
    same_records(cut["records"], want)
    for s in (0, 1):
        rec = cut["records"][s]
        for g in gone:
            assert record_of(rec, g) == b"" and int(rec["n_frames"][g]) == 2
        assert len(read_frames(rec["stream"])) == n - len(gone)


# ---- 3. the files are what the rest of the project reads ---------------------------------------------------------------------------------------
def test_the_streams_replay_agree_and_load(gpu_ctx, tmp_path):
    from oak_amd.train import FrameCorpus
    b, d, r, seeds = states(gpu_ctx)
    out, _ = reference(gpu_ctx)
    p1, p2 = out["records"]
    for rec in (p1, p2):
        rep = replay_check(gpu_ctx, rec["stream"])
        assert rep["stopped_at"] == len(rec["stream"]) and len(rep["reports"]) == N and (rep["reports"]["status"] == 0).all(), rep["reports"]
    one, two = read_frames(p1["stream"]), read_frames(p2["stream"])
    key = lambda game: [(u["c1"], u["c2"], u["m"], u["n"]) for u in game["updates"]]
    searched = unsearched = 0
    for g in range(N):
        assert (one[g]["battle"] == two[g]["battle"]).all() and (one[g]["battle"] == b[g]).all()
        assert one[g]["result"] == two[g]["result"] == int(out["results"][g])
        assert len(one[g]["updates"]) == len(two[g]["updates"]) == int(out["turns"][g])
        assert key(one[g]) == key(two[g]) == [(int(t["c1"]), int(t["c2"]), int(t["m"]), int(t["n"])) for t in out["log"][g][:int(out["turns"][g])]]
        for t in out["log"][g][:int(out["turns"][g])]:
            searched += int(t["m"]) > 1
            unsearched += int(t["m"]) == 1
    assert unsearched > 0
    net = network(gpu_ctx, tmp_path, "tiny")
    corpus = FrameCorpus(gpu_ctx, p1["stream"])
    assert corpus.info() == {"records": N, "malformed": 0, "frames": searched + unsearched, "stopped_at": len(p1["stream"])}
    got = corpus.evaluate(net, 0.5, 0.5, 0.0, 0.5, min_iterations=1)
    assert (got["rows"], got["excluded"], got["failed"]) == (searched, unsearched, 0), got
    corpus.close()
    net.close()


# ---- 4. off means untouched ----------------------------------------------------------------------------------------------------------------------
def test_recording_off_is_the_call_as_it_was(gpu_ctx):
    from oak_amd.search import Forest
    b, d, r, seeds = states(gpu_ctx)
    on, on_stats = reference(gpu_ctx)
    forest = Forest(gpu_ctx, N, 16)
    off_stats = {}
    off = search_games(gpu_ctx, (PE16, MC8), b, d, r, seeds, forest=forest, log_turns=LOG, stats=off_stats)
    assert "records" not in off and same(off, on) and off["counts"] == on["counts"] and off_stats == on_stats
    size = C.c_size_t(0)
    with pytest.raises(OakGpuError, match="oakgpu_forest_match_records: the forest holds no finished match call made with recording on"):
        _lib.check(gpu_ctx.lib.oakgpu_forest_match_records(forest.handle, 0, None, 0, C.byref(size), None, None, None, None, 0))
    again = search_games(gpu_ctx, (PE16, MC8), b, d, r, seeds, forest=forest, log_turns=LOG, records=True)      # the same forest, switched on
    same_records(again["records"], on["records"])
    with pytest.raises(OakGpuError, match="oakgpu_forest_match_records: seat must be 0"):
        _lib.check(gpu_ctx.lib.oakgpu_forest_match_records(forest.handle, 2, None, 0, C.byref(size), None, None, None, None, 0))
    with pytest.raises(OakGpuError, match="oakgpu_forest_match_set_records: on must be 0 or 1"):
        _lib.check(gpu_ctx.lib.oakgpu_forest_match_set_records(forest.handle, 2))
    search_games(gpu_ctx, (PE16, MC8), b[:3], d[:3], r[:3], seeds[:3], forest=forest, max_turns=2)               # off again: the records are gone
    with pytest.raises(OakGpuError, match="oakgpu_forest_match_records: "):
        _lib.check(gpu_ctx.lib.oakgpu_forest_match_records(forest.handle, 1, None, 0, C.byref(size), None, None, None, None, 0))
    forest.close()


# ---- 5. independence ----------------------------------------------------------------------------------------------------------------------------
def test_a_games_records_do_not_depend_on_its_neighbours(gpu_ctx):
    b, d, r, seeds = states(gpu_ctx)
    out, _ = reference(gpu_ctx)
    back = np.arange(N)[::-1]
    rev = search_games(gpu_ctx, (PE16, MC8), b[back], d[back], r[back], seeds[back], log_turns=LOG, records=True)
    for s in (0, 1):
        for g in range(N):
            assert record_of(rev["records"][s], N - 1 - g) == record_of(out["records"][s], g), (s, g)
    for g in (0, 3, 20, N - 1):
        one = search_games(gpu_ctx, (PE16, MC8), b[g:g + 1], d[g:g + 1], r[g:g + 1], seeds[g:g + 1], log_turns=LOG, records=True)
        for s in (0, 1):
            assert one["records"][s]["stream"] == record_of(out["records"][s], g), (s, g)
            assert one["records"][s]["offsets"].tolist() == [0, len(one["records"][s]["stream"])]


# ---- 6. faces -------------------------------------------------------------------------------------------------------------------------------------
def test_pyoak_and_cpp_faces_return_the_c_calls_bytes(gpu_ctx, tmp_path):
    from oak_amd import pyoak
    b, d, r, seeds = states(gpu_ctx)
    n = 7
    b, d, r, seeds = b[:n], d[:n], r[:n], seeds[:n]
    want = search_games(gpu_ctx, (PE8, MC8), b, d, r, seeds, log_turns=LOG, records=True)
    a1, a2 = pyoak.Agent(), pyoak.Agent()
    a1.budget, a1.bandit, a1.eval = "8", "ucb-2.0", "fp"
    a2.budget, a2.bandit, a2.eval = "8", "ucb-2.0", "mc"
    got = pyoak.match_forest(b, d, r, seeds, a1, a2, log_turns=LOG, records=True)
    for k in ("results", "turns", "status", "log"):
        assert np.asarray(got[k]).tobytes() == want[k].tobytes(), k
    same_records(got["records"], want["records"])
    assert "records" not in pyoak.match_forest(b, d, r, seeds, a1, a2, max_turns=2)
    exe, data, prefix = str(tmp_path / "cpp_forest_match_records_smoke"), str(tmp_path / "in.bin"), str(tmp_path / "out")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_forest_match_records_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    with open(data, "wb") as f:
        f.write(np.uint32(n).tobytes() + b.tobytes() + d.tobytes() + r.tobytes() + seeds.astype(np.uint64).tobytes())
    run = subprocess.run([exe, data, prefix], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    for s, name in enumerate((".p1", ".p2")):
        raw = open(prefix + name, "rb").read()
        tail = 8 * (n + 1) + 4 * n
        rec = want["records"][s]
        assert raw[:-tail] == rec["stream"], name
        assert raw[-tail:] == np.asarray(rec["offsets"]).astype(np.uint64).tobytes() + np.asarray(rec["n_frames"]).astype(np.uint32).tobytes(), name


def test_the_tool_writes_files_the_replay_check_accepts(tmp_path):
    """tools/search_match.py --dir in a child process (torch initialises the GPU before the library does), then tools/verify_battle_data.py
    over what it wrote."""
    out_dir = str(tmp_path / "match")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "search_match.py"), "--budget", "8", "--eval", "fp", "--max-games", "4", "--max-turns", "300",
                          "--dir", out_dir], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    files = [os.path.join(out_dir, seat, "%d.battle.data" % k) for k in (0, 1) for seat in ("p1", "p2")]
    for path in files:
        assert os.path.getsize(path) > 0 and ("wrote " + path) in run.stdout, run.stdout
    assert open(files[0], "rb").read() != open(files[1], "rb").read()
    check = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "verify_battle_data.py")] + files, capture_output=True, text=True, timeout=300)
    assert check.returncode == 0, check.stdout[-2000:] + check.stderr[-4000:]
    print(run.stdout, check.stdout)
