"""GPU: `.build.data` records into training tensors (oak_amd.build.TrajectoryCorpus / targets / dense_state, oak_amd/csrc/buildtraj.hip)
against the referee tests/build_traj_ref.py, itself held to the reference's own arrays in tests/test_build_traj_ref.py.  Every comparison
is exact except old_logp, which is held to float64 within the ulp bound stated for it in include/oakgpu.h.

The inputs: the reference goldens, the 8 records of build_goldens.npz (six of them teams of six), about 2,000 trajectories of
build_ref.Rollout with seeded random picks over the planted and sample teams at sizes 1 .. 6 with deletions, and the malformed records in
between.  A census on the CPU, before any GPU call, asserts that every step kind and every status occurs."""
import os

import numpy as np
import pytest
import torch

import build_ref as B
import build_traj_ref as T
from oak_amd import build, netfile

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 63, 64, 65, 257)
PER_STEP = ("action", "mask", "n_legal", "policy")
ALL = PER_STEP + ("value", "score", "start", "end", "status")
_CACHE = {}


def _inputs():
    """(records uint8[n, 128], the referee's arrays for no_score 0 and 1 with the mask as int16) -- computed once, never changed."""
    if "inputs" not in _CACHE:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "build_traj_goldens.npz"))["records"]
        old = np.load(os.path.join(ROOT, "tests", "golden", "build_goldens.npz"))["records"]
        rolled = T.rollout_records(2000, 28)
        bad = np.stack([r for _, _, r in T.malformed_records()])
        parts, at = [gold, old], 0
        for k in range(len(bad)):                      # the malformed records in between
            parts += [rolled[at:at + 250], bad[k:k + 1]]
            at += 250
        parts.append(rolled[at:])
        records = np.ascontiguousarray(np.concatenate(parts))
        refs = []
        for no_score in (False, True):
            ref = T.decode_many(records, no_score)
            ref["mask"] = ref["mask"].astype(np.int16)
            for v in ref.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            refs.append(ref)
        _CACHE["inputs"] = (records, refs)
    return _CACHE["inputs"]


def _corpus(ctx):
    if "corpus" not in _CACHE:
        _CACHE["corpus"] = build.TrajectoryCorpus(ctx, _inputs()[0].tobytes())
    return _CACHE["corpus"]


def test_census_of_the_inputs():
    """A condition on the inputs, checked on the CPU before any GPU call: not a tolerance."""
    records, (ref, _) = _inputs()
    kinds = dict.fromkeys(("pre_start", "species_and_moves", "moves_only", "swap", "ended"), 0)
    for r, status in zip(records, ref["status"]):
        if status != T.OK:
            continue
        _, _, _, action, prob = T.fields(r)
        start, end, swap, full = T.bounds(action, prob)
        kinds["pre_start"] += start
        kinds["species_and_moves"] += max(0, min(full, swap) - start)
        kinds["moves_only"] += max(0, swap - max(full, start))
        kinds["swap"] += end - swap
        kinds["ended"] += 31 - end
    assert min(kinds.values()) >= 20, kinds
    assert set(ref["status"].tolist()) == set(range(T.N_STATUS))
    assert (records[:, 1] == 255).any() and (records[:, 1] != 255).any()


def _guarded(n, mask_dtype, shift):
    """Output tensors on the device inside one poisoned byte buffer each, with guard bands before and after; `shift` moves the arrays off
    the 16-byte grid (by their own entry size).  Returns (out dict, check) -- check() asserts the guards are intact."""
    mdt = {"int64": torch.int64, "int16": torch.int16}[mask_dtype]
    shapes = [("action", (n, 31), torch.int64), ("mask", (n, 31, 339), mdt), ("n_legal", (n, 31), torch.int16), ("policy", (n, 31), torch.float32),
              ("value", (n,), torch.float32), ("score", (n,), torch.float32), ("start", (n,), torch.int64), ("end", (n,), torch.int64),
              ("status", (n,), torch.uint8), ("t_max", (1,), torch.int32)]
    out, raws = {}, []
    for name, shape, dtype in shapes:
        size = torch.empty((), dtype=dtype).element_size()
        body = int(np.prod(shape)) * size
        front = 4096 + (size if shift else 0)
        raw = torch.full((front + body + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        out[name] = raw[front:front + body].view(dtype).view(shape)
        raws.append((name, raw, front, body))

    def check():
        for name, raw, front, body in raws:
            assert bool((raw[:front] == 0xA5).all()) and bool((raw[front + body:] == 0xA5).all()), "guard band of " + name
    return out, check


def _compare(got, ref, picks, mask=True):
    for name in ALL:
        if name == "mask" and not mask:
            continue
        g = got[name].cpu().numpy() if hasattr(got[name], "cpu") else got[name]
        want = ref[name][picks]
        assert g.shape == want.shape, name
        if name == "policy" or name in ("value", "score"):
            assert np.array_equal(g.view(np.uint32), want.astype(np.float32).view(np.uint32)), name     # bit for bit
        else:
            assert np.array_equal(g.astype(np.int64), want.astype(np.int64)), name
    t_max = int(got["t_max"][0])
    assert t_max == int(ref["end"][picks].max())


@pytest.mark.parametrize("mask_dtype", ("int64", "int16"))
@pytest.mark.parametrize("n", ROWS)
def test_explicit_picks_against_the_referee(gpu_ctx, n, mask_dtype):
    records, refs = _inputs()
    corpus = _corpus(gpu_ctx)
    rng = np.random.default_rng(1000 + n)
    bad_at = np.flatnonzero(refs[0]["status"] != T.OK)
    picks = rng.integers(0, len(records), n).astype(np.uint32)
    if n > 8:
        picks[rng.choice(n, len(bad_at), replace=False)] = bad_at     # every malformed record among them
    for no_score in (False, True):
        out, check = _guarded(n, mask_dtype, shift=(n % 2 == 1))
        got = corpus.decode(torch.from_numpy(picks.astype(np.int32)).cuda(), mask_dtype=mask_dtype, no_score=no_score, out=out)
        torch.cuda.synchronize()
        check()
        _compare(got, refs[int(no_score)], picks)       # (a poison byte left inside would differ from the referee: every entry is compared)


def test_every_record_once_and_the_numpy_path(gpu_ctx):
    records, refs = _inputs()
    corpus = _corpus(gpu_ctx)
    picks = np.arange(len(records), dtype=np.uint32)
    got = corpus.decode(torch.from_numpy(picks.astype(np.int32)).cuda(), mask_dtype="int16")
    _compare(got, refs[0], picks)
    host = corpus.decode(picks[:70], mask_dtype="int64", no_score=True)
    assert isinstance(host["mask"], np.ndarray) and host["mask"].dtype == np.int64
    _compare(host, refs[1], picks[:70])
    cheap = corpus.decode(picks[:70], mask=False, trim=True)
    assert "mask" not in cheap and cheap["action"].shape == (70, int(refs[0]["end"][:70].max()))
    info = corpus.info()
    assert info["records"] == len(records) and info["files"] == 1
    assert [info["status"][k] for k in build.TRAJ_STATUS] == np.bincount(refs[0]["status"], minlength=T.N_STATUS).tolist()
    with pytest.raises(Exception, match="pick 1: record"):
        corpus.decode(np.array([0, len(records)], np.uint32))
    # a pick outside the corpus on the device path reads nothing and says so
    out = corpus.decode(torch.tensor([3, len(records)], dtype=torch.int32).cuda(), mask_dtype="int16")
    assert out["status"].cpu().tolist() == [int(refs[0]["status"][3]), 255] and bool((out["mask"][1] == -1).all()) and int(out["end"][1]) == 0


def test_sampling_rule_repeatability_and_independence(gpu_ctx):
    records, refs = _inputs()
    sizes = (37, 5, 211)                                 # three files of unequal size
    files, at = [], 0
    for s in sizes:
        files.append(records[at:at + s].tobytes())
        at += s
    with build.TrajectoryCorpus(gpu_ctx, files) as corpus:
        want = T.draws(sizes, 300, 0xFFFFFFFFFFFFFF00)    # (seed + i wraps around 2^64)
        a = corpus.sample(300, 0xFFFFFFFFFFFFFF00, mask_dtype="int16", device="cuda")
        b = corpus.sample(300, 0xFFFFFFFFFFFFFF00, mask_dtype="int16", device="cuda")
        short = corpus.sample(41, 0xFFFFFFFFFFFFFF00, mask_dtype="int16", device="cuda")
        torch.cuda.synchronize()
        picks = a["picks"].cpu().numpy().view(np.uint32)
        assert np.array_equal(picks, want) and len(set((np.searchsorted(np.cumsum(sizes), picks, "right")).tolist())) == 3
        _compare(a, refs[0], picks)
        for name in ALL + ("picks",):
            assert torch.equal(a[name], b[name]), name                      # two calls give the same bits
            assert torch.equal(a[name][:41], short[name]), name             # draw i does not depend on n
        alone = corpus.decode(a["picks"][17:18].clone(), mask_dtype="int16")  # a row depends on its record alone
        for name in ALL:
            assert torch.equal(alone[name][0], a[name][17]), name
        host = corpus.sample(9, 5)                                          # numpy out, picks included
        assert np.array_equal(host["picks"], T.draws(sizes, 9, 5))
        _compare(host, refs[0], host["picks"])


def _torch_get_state(actions):
    """build.py's get_state, as written there (actions [b, T, 1] on the CPU)."""
    b, T_, _ = actions.shape
    state = torch.zeros((b, T_, T.N_DIM + 1), dtype=torch.float32)
    state = state.scatter(2, actions + 1, 1.0)
    state = torch.cumsum(state, dim=1).clamp_max(1.0)
    state = state[:, :-1, 1:]
    return torch.concat([torch.zeros(state[:, :1].shape), state], dim=1)


@pytest.mark.parametrize("on_device", (True, False))
def test_targets(gpu_ctx, on_device):
    records, refs = _inputs()
    corpus = _corpus(gpu_ctx)
    picks = np.arange(0, len(records), 7, dtype=np.uint32)[:257]
    ref = {k: (v[picks] if isinstance(v, np.ndarray) else v) for k, v in refs[0].items()}
    want = T.targets(ref, 0.7)
    traj = corpus.decode(torch.from_numpy(picks.astype(np.int32)).cuda() if on_device else picks, mask=False)
    got = build.targets(gpu_ctx, traj, 0.7)
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    assert host["n_valid"] == len(want["rows"]) > 500
    assert np.array_equal(host["valid"], want["valid"])
    assert np.array_equal(host["rows"].astype(np.int64), want["rows"].astype(np.int64))            # order included
    assert np.array_equal(host["state_n"], want["state_n"])
    assert np.array_equal(host["state_cells"].view(np.uint16), want["state_cells"])
    assert np.array_equal(host["rewards"].view(np.uint32), want["rewards"].view(np.uint32))
    assert (want["rewards"] != 0).sum() > 100
    # old_logp against float64: at most OLD_LOGP_ULPS ulps of float (the ulp of the binade that holds the exact logarithm), and exactly 0 at policy 1
    exact = want["old_logp"]
    got_logp = host["old_logp"].astype(np.float64)
    zero = exact == 0
    ulp = 2.0 ** (np.floor(np.log2(np.abs(np.where(zero, 1.0, exact)))) - 23)
    err = np.abs(got_logp - exact)
    print("old_logp: worst error %.4f ulp over %d rows" % (float((err / ulp)[~zero].max()), len(exact)))
    assert zero.any() and (got_logp[zero] == 0).all() and (err[~zero] <= T.OLD_LOGP_ULPS * ulp[~zero]).all()
    # the dense state of a chunk equals build.py's get_state(action)[valid], bit for bit
    state = _torch_get_state(torch.from_numpy(ref["action"].copy()).unsqueeze(-1))[torch.from_numpy(want["valid"])]
    for lo, hi in ((0, 1), (5, 300), (host["n_valid"] - 130, host["n_valid"])):
        dense = build.dense_state(gpu_ctx, got, lo, hi)
        dense = dense.cpu() if on_device else torch.from_numpy(dense)
        assert torch.equal(dense, state[lo:hi])


def test_round_trip_of_real_rollouts(gpu_ctx):
    """build.provide -> build.records -> TrajectoryCorpus.decode: the writer and the reader agree."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.build.net")
        netfile.write_random_build_net(path, 3, policy_hidden=8, value_hidden=4)
        net = build.BuildNetwork(gpu_ctx, path)
    n = 120
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(7)
    rolled = build.provide(gpu_ctx, net, B.sample_teams(), seeds, team_modify_prob=0.9, pokemon_delete_prob=0.3, move_delete_prob=0.3)
    data = build.records(gpu_ctx, rolled, np.linspace(0, 1, n).astype(np.float32), 0.5)
    net.close()
    built = np.flatnonzero(rolled["n_updates"])
    assert len(built) > 60 and len(data) == 128 * len(built)
    with build.TrajectoryCorpus(gpu_ctx, data) as corpus:
        got = corpus.decode(np.arange(len(built), dtype=np.uint32))
    assert (got["status"] == 0).all()
    for row, g in enumerate(built):
        k, start, end = int(rolled["n_updates"][g]), int(got["start"][row]), int(got["end"][row])
        assert start == len(B.initial_cells(rolled["teams_init"][g], int(rolled["sizes"][g]))) and end == start + k
        assert np.array_equal(got["action"][row, start:end], rolled["action"][g, :k].astype(np.int64))
        want = np.array([B.compress_probability(p) for p in rolled["prob"][g, :k]], np.float32) / np.float32(65535.0)
        assert np.array_equal(got["policy"][row, start:end], want)
        assert np.array_equal(got["mask"][row, start:end, 0], got["action"][row, start:end])            # every taken action is in its list
        # the lists are as long as the rollout's own, but for the lead swap: the reader's swap list holds the lead's set too (write_swaps)
        extra = np.zeros(k, np.int64)
        extra[k - 1] = 1 if _is_swap(rolled, g, k) else 0
        assert np.array_equal(got["n_legal"][row, start:end].astype(np.int64), rolled["n_legal"][g, :k].astype(np.int64) + extra)


def _is_swap(rolled, g, k):
    """The last action is a (species, None) cell of a species the finished team already held before it: a swap, not an addition."""
    last = int(rolled["action"][g, k - 1])
    held = set(B.initial_cells(rolled["teams_init"][g], int(rolled["sizes"][g]))) | set(int(a) for a in rolled["action"][g, :k - 1])
    return last in held
