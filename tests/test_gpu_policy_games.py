"""GPU: batches of whole games between two policies (oakgpu_policy_games*, oak_amd/arena.py) -- random seats against the rollout kernel
and the oracle byte for byte, every output against every schedule, network seats against the stated draw and policy rules replayed on
the oracle with float64 policies, discrete networks, poisoned buffers, the refusals, and arena.match's accounting."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import policy_games_ref as R
from hipmem import Dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = {tag: os.path.join(ROOT, "tests", "golden", "net_%s.battle.net" % tag) for tag in ("tiny", "default")}
SIZES = (1, 63, 64, 65, 257, 1000)
KEYS = ("results", "turns", "values", "prng", "battles", "durations")

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def random_batch():
    return cached("random", lambda: O.make_random_ou_batch(1000))


def team_bytes():
    from oak_amd import gamedata as G
    teams = json.load(open(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json")))["teams"]
    return np.array([[[G.match_species(s[0])] + [G.match_move(m) for m in s[1:]] for s in t] for t in teams], dtype=np.uint8)


def team_batch(n=300):
    """n games from the sample teams: game i is team i % 16 against team (i // 16 + 5 i) % 16, init_battles with seed i + 1; streams seeded
    i + 1 as well."""
    def make():
        tb = team_bytes()
        b, r = np.zeros((n, 384), np.uint8), np.zeros(n, np.uint8)
        prng = np.zeros((n, 8), np.uint8)
        opts = []
        for i in range(n):
            b[i] = O.init_battle(np.stack([tb[i % 16], tb[(i // 16 + 5 * i) % 16]]), i + 1)
            o = O.Options()
            r[i] = O.update(b[i], 0, 0, o)
            opts.append(o.durations.copy())
            O.LIB.oracle_fast_prng_seed(O.ptr(prng[i]), C.c_uint64(i + 1))
        return b, np.stack(opts), prng, r
    return cached(("teams", n), make)


def nets(ctx):
    from oak_amd.engine import Network
    return cached("nets", lambda: dict(tiny=Network(ctx, path=NET["tiny"]), default=Network(ctx, path=NET["default"]),
                                       default_again=Network(ctx, path=NET["default"])))


def play(ctx, seats, batch, idx=None, **kw):
    from oak_amd import arena
    b, d, p, r = batch
    if idx is not None:
        b, d, p, r = (np.ascontiguousarray(x[idx]) for x in (b, d, p, r))
    kw.setdefault("return_state", True)
    return arena.policy_games(ctx, seats, b, d, r, p, **kw)


def same(a, b, keys=KEYS + ("log",)):
    for k in keys:
        if a.get(k) is None and b.get(k) is None:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "values":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape and (x == y).all(), (k, np.argwhere(x != y)[:4].tolist())
    assert a["counts"] == b["counts"]


# ---- 1. random seats are the rollout kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_turns", (1000, 37))
@pytest.mark.parametrize("n", SIZES)
def test_random_seats_equal_the_rollout_kernel(gpu_ctx, n, max_turns):
    b, d, p, r = (x[:n] for x in random_batch())
    got = play(gpu_ctx, (None, None), (b, d, p, r), max_turns=max_turns)
    roll = gpu_ctx.rollout(b, d, r, p, max_steps=max_turns, prep=False, return_state=True)
    assert (got["results"] == roll["results"]).all() and (got["turns"] == roll["steps"]).all()
    assert (got["values"].view(np.uint32) == roll["values"].view(np.uint32)).all()
    assert (got["prng"] == roll["prng"]).all() and (got["battles"] == roll["battles"]).all() and (got["durations"] == roll["durations"]).all()
    t = got["results"] & 15
    assert got["counts"] == (int((t == 1).sum()), int((t >= 3).sum()), int((t == 2).sum()), int((t == 0).sum()))
    if max_turns == 37:
        capped = t == 0
        assert (capped.any() or n < 63) and (got["turns"][capped] == 37).all() and (got["values"][capped] == 0.5).all() and (got["turns"][~capped] <= 37).all()
    if n == 257:
        ob, od, op = b.copy(), d.copy(), p.copy()
        out, steps = O.rollout_batch(ob, od, r, op, max_steps=max_turns, threads=4)
        assert (got["results"] == out).all() and (got["turns"] == steps).all() and (got["battles"] == ob).all()
        assert (got["durations"] == od).all() and (got["prng"] == op).all()


# ---- 2. nothing depends on the schedule ----------------------------------------------------------------------------------------------
def schedule_cases(ctx):
    return {"random": ((None, None), random_batch()), "net": ((nets(ctx)["tiny"], nets(ctx)["tiny"]), team_batch())}


def schedule_base(ctx, which):
    seats, batch = schedule_cases(ctx)[which]
    return cached(("base", which), lambda: play(ctx, seats, batch, log_turns=1000))


@pytest.mark.parametrize("compact_below", (-1.0, 0.0, 2.0))
@pytest.mark.parametrize("poll", (1, 7, 64))
@pytest.mark.parametrize("which", ("random", "net"))
def test_outputs_do_not_depend_on_poll_or_compaction(gpu_ctx, which, poll, compact_below):
    from oak_amd import arena
    seats, batch = schedule_cases(gpu_ctx)[which]
    got = play(gpu_ctx, seats, batch, log_turns=1000, poll=poll, compact_below=compact_below)
    stats = arena.last_stats(gpu_ctx)
    same(schedule_base(gpu_ctx, which), got)
    if compact_below < 0:
        assert stats["compactions"] == 0
    else:
        assert stats["compactions"] >= 1
    if compact_below > 1:   # every poll that found a finished game compacted: no row of a retired game is evaluated past the next poll
        assert stats["row_turns"] <= int(got["turns"].astype(np.int64).sum()) + (poll + 1) * len(got["turns"])


@pytest.mark.parametrize("which", ("random", "net"))
def test_outputs_do_not_depend_on_the_batch(gpu_ctx, which):
    seats, batch = schedule_cases(gpu_ctx)[which]
    base = schedule_base(gpu_ctx, which)
    n = len(base["turns"])
    turns = base["turns"].astype(np.int64)
    for i in sorted({int(turns.argmax()), int(turns.argmin()), n // 2}):     # the longest game, the shortest, one in between: alone
        alone = play(gpu_ctx, seats, batch, idx=[i], log_turns=1000)
        same({k: (np.asarray(v)[i:i + 1] if k != "counts" else alone["counts"]) for k, v in base.items()}, alone)
    rev = play(gpu_ctx, seats, batch, idx=np.arange(n)[::-1].copy(), log_turns=1000)
    same({k: (np.asarray(v)[::-1] if k != "counts" else v) for k, v in base.items()}, rev)


# ---- 3. network seats play the stated rule -------------------------------------------------------------------------------------------
def seat_spec(s):
    """(kind, temp, min) of an arena seat."""
    if s is None:
        return (R.RANDOM, 1.0, 0.0)
    if isinstance(s, tuple):
        return (R.POLICY, float(s[1]), float(s[2]))
    return (R.POLICY, 1.0, 0.0)


def check_games(ctx, seats, batch, got, log_turns, label):
    """The checks of a network pairing: the log replays on the oracle to the outputs; every pick is the rule's on the replayed states'
    logits, the Python stream and the float64 policy -- except within BOUNDARY_EPS of a cumulative boundary, at most 1 % of the picks."""
    b, d, p, r = batch
    n = b.shape[0]
    spec = (seat_spec(seats[0]), seat_spec(seats[1]))
    rows, owner = [], []
    finals = []
    for g in range(n):
        turns = int(got["turns"][g])
        assert turns <= log_turns
        states, final = R.replay_game(b[g], d[g], r[g], got["log"][g], turns)
        assert (got["log"][g, turns:] == 0xFF).all(), (label, g, "the log goes on past the game's end")
        assert final[2] == int(got["results"][g]), (label, g, "result", final[2], int(got["results"][g]))
        assert (final[0] == got["battles"][g]).all() and (final[1] == got["durations"][g]).all(), (label, g, "final state")
        assert (final[2] & 15) != 0 or turns == log_turns, (label, g, "stopped early")
        finals.append(final)
        rows += states
        owner += [g] * turns
    total = len(rows)
    sb = np.stack([s[0] for s in rows])
    sd = np.stack([s[1] for s in rows])
    ch = [np.zeros((total, 9), np.uint8), np.zeros((total, 9), np.uint8)]
    cn = [np.zeros(total, np.uint8), np.zeros(total, np.uint8)]
    for i, s in enumerate(rows):
        for side in (0, 1):
            o = s[3 + side]
            ch[side][i, :len(o)] = o
            cn[side][i] = len(o)
    logits = [None, None]
    for side in (0, 1):        # a leaf's logits do not depend on its batch (tests/test_gpu_policy.py)
        net = seats[side][0] if isinstance(seats[side], tuple) else seats[side]
        if net is not None:
            logits[side] = net.value_policy_inference(sb, sd, ch[0], cn[0], ch[1], cn[1])[1 + side]
    picks = excluded = 0
    i = 0
    for g in range(n):
        stream = R.FastPrng(p[g])
        for t in range(int(got["turns"][g])):
            o = (rows[i][3], rows[i][4])
            draws = R.turn_draws(spec, stream, len(o[0]), len(o[1]), None if logits[0] is None else logits[0][i], None if logits[1] is None else logits[1][i])
            for side in (0, 1):
                want, pol, u = draws[side]
                actual = int(np.nonzero(o[side] == got["log"][g, t, side])[0][0])
                if pol is None:
                    assert actual == want, (label, g, t, side, "forced or random pick", actual, want)
                    continue
                picks += 1
                assert pol[actual] > 0.0, (label, g, t, side, "a pick of rule probability 0", actual, pol.tolist())
                if R.boundary_distance(pol, u) <= R.BOUNDARY_EPS:
                    excluded += 1
                    continue
                assert actual == want, (label, g, t, side, actual, want, u, pol.tolist())
            i += 1
        assert (stream.state() == got["prng"][g]).all(), (label, g, "the stream's final state")
    print("%s: %d games, %d turns, %d sampled picks, %d left out near a boundary" % (label, n, total, picks, excluded))
    assert excluded <= 0.01 * max(picks, 1), (label, excluded, picks)
    return picks


def pairings(ctx):
    N = nets(ctx)
    return {"tiny_vs_default": (N["tiny"], N["default"]), "default_vs_itself_two_handles": (N["default"], N["default_again"]),
            "tiny_vs_random": (N["tiny"], None)}


@pytest.mark.parametrize("options", ("plain", "temp_min"))
@pytest.mark.parametrize("name", ("tiny_vs_default", "default_vs_itself_two_handles", "tiny_vs_random"))
def test_network_seats_play_the_stated_rule(gpu_ctx, name, options):
    seats = pairings(gpu_ctx)[name]
    if options == "temp_min":
        seats = ((seats[0], 0.5, 0.05), seats[1])
    batch = team_batch()
    got = play(gpu_ctx, seats, batch, log_turns=1000)
    assert check_games(gpu_ctx, seats, batch, got, 1000, name + "/" + options) > 1000
    if name == "default_vs_itself_two_handles":    # ... and as ONE handle (one evaluator call per turn): the same outputs bitwise
        one = nets(gpu_ctx)["default"]
        same(got, play(gpu_ctx, ((one, 0.5, 0.05), one) if options == "temp_min" else (one, one), batch, log_turns=1000))


# ---- 4. discrete networks ------------------------------------------------------------------------------------------------------------
def test_discrete_network_seat(gpu_ctx, tmp_path):
    from oak_amd.engine import Network
    from test_gpu_discrete import shape_net
    q = Network(gpu_ctx, path=shape_net(tmp_path, "games", None), discrete=True)
    seats = (q, nets(gpu_ctx)["tiny"])
    batch = tuple(np.ascontiguousarray(x[:64]) for x in team_batch())
    got = play(gpu_ctx, seats, batch, log_turns=1000)
    assert check_games(gpu_ctx, seats, batch, got, 1000, "discrete_vs_tiny") > 200
    q.close()


# ---- 5. poisoned buffers -------------------------------------------------------------------------------------------------------------
def test_poisoned_buffers_and_a_short_log(gpu_ctx):
    from oak_amd import _lib
    n, log_turns, G = 65, 8, 256
    b, d, p, r = (np.ascontiguousarray(x[:n]) for x in team_batch())
    seats = (nets(gpu_ctx)["tiny"], None)
    base = play(gpu_ctx, seats, (b, d, p, r), log_turns=1000)
    sizes = dict(results=n, turns=4 * n, values=4 * n, battles=384 * n, durations=8 * n, log=2 * log_turns * n, prng=8 * n)
    bufs = {k: Dev(np.zeros(G + s + G, np.uint8), fill=0xAA) for k, s in sizes.items()}
    at = lambda k: C.c_void_p(bufs[k].p.value + G)
    nan = np.full(n, np.nan, np.float32).view(np.uint8)
    image = np.full(G + 4 * n + G, 0xAA, np.uint8)
    image[G:G + 4 * n] = nan
    bufs["values"].put(image)
    image = np.full(G + 8 * n + G, 0xAA, np.uint8)
    image[G:G + 8 * n] = p.reshape(-1)
    bufs["prng"].put(image)
    gb, gd, gr = Dev(b), Dev(d), Dev(r)
    params = _lib.PolicyGamesParams(_lib.Seat(1, seats[0].handle, 0.0, 0.0), _lib.Seat(0, None, 0.0, 0.0), 0, 0, 0.0, log_turns)
    counts = (C.c_uint64 * 4)()
    _lib.check(gpu_ctx.lib.oakgpu_policy_games_dev(gpu_ctx.handle, C.byref(params), gb.p, gd.p, gr.p, at("prng"), n, at("results"), at("turns"), at("values"),
                                                   at("battles"), at("durations"), at("log"), counts))
    out = {k: v.host() for k, v in bufs.items()}
    for k, s in sizes.items():
        assert (out[k][:G] == 0xAA).all() and (out[k][G + s:] == 0xAA).all(), (k, "guard band")
    body = lambda k: out[k][G:G + sizes[k]]
    assert (body("results") == base["results"]).all() and (body("turns").view(np.uint32) == base["turns"]).all()
    assert (body("values").view(np.uint32) == base["values"].view(np.uint32)).all()
    assert (body("battles").reshape(n, 384) == base["battles"]).all() and (body("durations").reshape(n, 8) == base["durations"]).all()
    assert (body("prng").reshape(n, 8) == base["prng"]).all()
    log = body("log").reshape(n, log_turns, 2)
    assert (base["turns"] > log_turns).any()
    for g in range(n):
        k = min(int(base["turns"][g]), log_turns)
        assert (log[g, :k] == base["log"][g, :k]).all(), (g, "the first turns")
        assert (log[g, k:] == 0xAA).all(), (g, "entries past the game's end keep the prefill")
    assert tuple(counts) == base["counts"]
    for x in list(bufs.values()) + [gb, gd, gr]:
        x.free()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu_ctx):
    from oak_amd import _lib
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    n = 4
    b, d, p, r = (np.ascontiguousarray(x[:n]) for x in team_batch())
    gb, gd, gr, gp = Dev(b), Dev(d), Dev(r), Dev(p)
    outs = [Dev(np.zeros(s, np.uint8), fill=0xAA) for s in (n, 4 * n, 4 * n)]
    net = nets(gpu_ctx)["tiny"].handle
    counts = (C.c_uint64 * 4)()

    def call(params, count=n):
        return lib.oakgpu_policy_games_dev(h, None if params is None else C.byref(params), gb.p, gd.p, gr.p, gp.p, count, outs[0].p, outs[1].p, outs[2].p, None,
                                           None, None, counts)

    def refused(params, text):
        rc = call(params)
        assert rc != 0 and text in lib.oakgpu_last_error().decode(), (rc, lib.oakgpu_last_error())
        gpu_ctx.synchronize()
        assert all((o.host() == 0xAA).all() for o in outs) and (gp.host() == p).all(), "something was launched"

    P, S = _lib.PolicyGamesParams, _lib.Seat
    ok = S(1, net, 1.0, 0.0)
    refused(None, "null params")
    refused(P(S(1, None, 1.0, 0.0), ok, 0, 0, 0.0, 0), "needs a network")
    refused(P(ok, S(1, None, 1.0, 0.0), 0, 0, 0.0, 0), "seat p2")
    refused(P(S(7, net, 1.0, 0.0), ok, 0, 0, 0.0, 0), "unknown kind")
    refused(P(ok, S(-1, None, 1.0, 0.0), 0, 0, 0.0, 0), "unknown kind")
    refused(P(S(1, net, -0.5, 0.0), ok, 0, 0, 0.0, 0), "temp")
    refused(P(ok, S(1, net, 1.0, 1.5), 0, 0, 0.0, 0), "zero policy")
    if lib.oakgpu_device_count() > 1:      # a network belongs to a device: another context of the SAME device may use it (oakgpu_search_many does)
        from oak_amd.engine import Context, Network
        far = Context(1)
        other = Network(far, path=NET["tiny"])
        refused(P(S(1, other.handle, 1.0, 0.0), ok, 0, 0, 0.0, 0), "another device")
        other.close()
        far.close()
    assert call(P(ok, ok, 0, 0, 0.0, 0), count=0) == 0
    assert call(P(S(0, None, 0.0, 0.0), S(0, None, 0.0, 0.0), 0, 0, 0.0, 0), count=0) == 0
    gpu_ctx.synchronize()
    assert all((o.host() == 0xAA).all() for o in outs)
    for x in [gb, gd, gr, gp] + outs:
        x.free()


def test_a_zeroed_policy_flags_its_game(gpu_ctx):
    """min = 0.6: a turn whose largest prior is below 0.6 has no entry left (policy.h:81-92).  Those games stop there -- NaN, 0xFF, in no
    counter -- the call fails with the reference's text and the lowest such game, and every other game is complete and unchanged."""
    from oak_amd import _lib
    batch = tuple(np.ascontiguousarray(x[:65]) for x in team_batch())
    tiny = nets(gpu_ctx)["tiny"]
    b, d, p, r = batch
    n = b.shape[0]
    out = dict(results=np.zeros(n, np.uint8), turns=np.zeros(n, np.uint32), values=np.zeros(n, np.float32), prng=p.copy())
    params = _lib.PolicyGamesParams(_lib.Seat(1, tiny.handle, 1.0, 0.6), _lib.Seat(0, None, 0.0, 0.0), 0, 0, 0.0, 0)
    counts = (C.c_uint64 * 4)()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = gpu_ctx.lib.oakgpu_policy_games(gpu_ctx.handle, C.byref(params), ptr(b), ptr(d), ptr(r), ptr(out["prng"]), n, ptr(out["results"]), ptr(out["turns"]),
                                         ptr(out["values"]), None, None, None, counts)
    flagged = out["results"] == 0xFF
    assert flagged.any(), "no game met a flat policy: the case is not exercised"
    text = gpu_ctx.lib.oakgpu_last_error().decode()
    assert rc != 0 and "RuntimePolicy: zero policy, mode: p" in text and "game %d;" % int(np.nonzero(flagged)[0][0]) in text, text
    assert np.isnan(out["values"][flagged]).all() and not np.isnan(out["values"][~flagged]).any()
    t = out["results"][~flagged] & 15
    assert tuple(counts) == (int((t == 1).sum()), int((t >= 3).sum()), int((t == 2).sum()), int((t == 0).sum())) and sum(counts) == n - int(flagged.sum())


# ---- the pybind11 face ---------------------------------------------------------------------------------------------------------------
def test_pyoak_policy_games_equals_the_host_call(gpu_ctx):
    from oak_amd import pyoak
    batch = tuple(np.ascontiguousarray(x[:65]) for x in team_batch())
    base = play(gpu_ctx, (nets(gpu_ctx)["tiny"], None), batch, log_turns=16)
    b, d, p, r = batch
    got = pyoak.policy_games(b, d, r, p, p1_network=NET["tiny"], log_turns=16)
    got["counts"] = tuple(int(x) for x in got["counts"])
    same(base, got)
    both = pyoak.policy_games(b, d, r, p, p1_network=NET["tiny"], p2_network=NET["tiny"], p1_temp=0.5, p1_min=0.05)
    assert sum(both["counts"]) == 65 and both["log"].shape == (65, 0, 2)


# ---- 7. arena.match ------------------------------------------------------------------------------------------------------------------
def test_match_accounts_both_seatings_from_net_a():
    """arena.match and the torch-tensor form of arena.policy_games through tests/policy_match_check.py in a child process -- torch must
    initialise the GPU before the library does."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "policy_match_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "policy match ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
