"""GPU: the embedding passes of the leaf evaluator -- k_embed_both (k_embed_prows + k_embed_arows in one launch), the two row kernels
launched alone, the tile kernel k_embed_lds and the work-list forms behind k_party_tags -- held to what the value path and the
policy heads are held to: a float64 evaluation (tests/embed_ref.py) under max |gpu - f64| <= 4 E_ref + 2e-7 S (policy_ref.bound),
on EVERY entry of EVERY row, in every routing and at every template width, on states that set every input the encoders have
(policy_ref.form_states + embed_ref.planted_states: tests/test_embed_ref.py holds the census).

What the kernels do (leafnet.hip): the row kernels add the one-hot and move rows of the first layer in fp32, multiply its dense part
(stats, boosts, volatiles) as exact bf16 triples, and multiply the second layer as scaled fp16 PAIRS (three fp16 MFMAs per block, fp32
accumulation: embed_layer2); the tile kernel runs both layers on fp32 MFMA.  E_ref is the fp32 oracle's own worst distance from
float64 on a seeded sample of the compared rows (nn_oracle.battle_embedding; the C oracle at full size) -- never a kernel's output;
a sample can only make E_ref smaller and the bound tighter.  S = max(1, max |f64 entry|).

Every call writes into a buffer pre-filled with NaN words between two guard bands: every entry finite afterwards, the entries of dead
items (fainted or absent: hp entry and block) exactly +0.0, the bands untouched.

Measured on an MI355X (profiles/r08_embed_accuracy.json holds all 46 float64 cases): worst error 3.7e-8 to 2.9e-7 against E_ref 2.5e-8
to 1.3e-7 (S = 1 everywhere: no embedding entry of these nets passes 1), 12 % to 42 % of the bound in every case -- the row kernels at
most 42 % (the 256-wide net at 65,569 leaves: 2.84e-7 against 6.78e-7), the tile kernel at most 39 %.  Every form meets the bound;
embedding_out is filled for the discrete handle (2.61e-7 against 6.70e-7).  tests/test_embed_ref.py shows on the CPU that second
layers cut to 16 bits would be 25 to 32 bounds away."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import embed_ref as E
import oracle_lib as O
import policy_ref as P
from policy_ref import NN

pytestmark = pytest.mark.gpu
F = np.float32
TESTS = os.path.dirname(os.path.abspath(__file__))
NET256 = P.GOLDEN["256"]
TILE, ROWS, FUSED = 1, 2, 3              # OAKGPU_EMBED_FORM_* (include/oakgpu.h)
GUARD = 64                               # floats in front of and behind the embedding buffer
NAN_WORD = 0xFFFFFFFF
ORACLE_ROWS = 384                        # rows the numpy oracle is run on for E_ref (all of them in a smaller batch)
# leafnet.hip: ER_ITEMS items per mini-tile, PR_WAVES / AR_WAVES mini-tiles per workgroup and sweep, at most 256 workgroups per pass
ER_ITEMS, PR_WAVES, AR_WAVES, MAX_WGS = 32, 8, 8, 256
FULL = 65536 + 33
RECORDS = {}


@pytest.fixture(scope="module", autouse=True)
def _accuracy_records():
    """OAK_EMBED_ACCURACY_JSON=<file>: write what the tests of this module measured (the source of profiles/r08_embed_accuracy.json)."""
    yield
    out = os.environ.get("OAK_EMBED_ACCURACY_JSON")
    if out and RECORDS:
        with open(out, "w") as f:
            json.dump({"bound": "max|gpu - f64| <= 4 * E_ref + 2e-7 * S", "cases": RECORDS}, f, indent=1, sort_keys=True)


# ---- the call under test --------------------------------------------------------------------------------------------------------
def embed_forms(ctx, net):
    from oak_amd import _lib
    f = [C.c_int(-1) for _ in range(3)]
    _lib.check(ctx.lib.oakgpu_leaf_embed_forms(ctx.handle, net.handle, *[C.byref(x) for x in f]))
    return tuple(x.value for x in f)


def expected_forms(onet, safe=True, timing=False, forced_tile=False):
    """embed_route's rule: the row kernels take hidden widths up to 128, party outputs up to 64 and active outputs up to 96 of a
    network whose embedding nets are safe on the 16-bit pipes; both in one launch unless an event has to sit between the passes."""
    rows = safe and not forced_tile
    prow = rows and onet.p0.out_dim <= 128 and onet.pod <= 64
    arow = rows and onet.a0.out_dim <= 128 and onet.aod <= 96
    blocks = (1 if onet.pod <= 32 else 2) if prow else 0
    if prow and arow and not timing:
        return (FUSED, FUSED, blocks)
    return (ROWS if prow else TILE, ROWS if arow else TILE, blocks)


class Guarded:
    """A device buffer of n x dim floats pre-filled with NaN words, with GUARD such words in front and behind."""

    def __init__(self, n, dim):
        from hipmem import Dev
        self.n, self.dim = n, dim
        self.buf = Dev(np.zeros(n * dim + 2 * GUARD, F), fill=0xFF)
        self.p = C.c_void_p(self.buf.p.value + 4 * GUARD)

    def host(self):
        raw = self.buf.host()
        bits = raw.view(np.uint32)
        assert (bits[:GUARD] == NAN_WORD).all() and (bits[GUARD + self.n * self.dim:] == NAN_WORD).all(), "a guard band was written"
        return raw[GUARD:GUARD + self.n * self.dim].reshape(self.n, self.dim).copy()

    def free(self):
        self.buf.free()


def gpu_embedding(ctx, net, b, d):
    """oakgpu_leaf_eval_dev's embedding_out for a batch: (embedding float32[n, dim], values)."""
    from hipmem import Dev
    from oak_amd import _lib
    n = b.shape[0]
    gb, gd, gv, ge = Dev(b), Dev(d), Dev(np.zeros(n, F), fill=0xFF), Guarded(n, net.shape()[0])
    _lib.check(ctx.lib.oakgpu_leaf_eval_dev(ctx.handle, net.handle, gb.p, gd.p, n, gv.p, ge.p))
    ctx.synchronize()
    emb, vals = ge.host(), gv.host()
    for x in (gb, gd, gv, ge):
        x.free()
    return emb, vals


def check_embedding(emb, onet, b, d, key, forms, act_party=None, act_actives=None, e_ref_net=None, cnet_path=None, oracle_rows=ORACLE_ROWS):
    """One embedding against embed_ref.embedding_f64 of `onet`: every entry of every row under the bound, dead entries +0.0, all
    finite.  E_ref from the numpy oracle of e_ref_net (default: onet) -- or the C oracle of cnet_path -- on a seeded sample of rows."""
    n = b.shape[0]
    ref = E.embedding_f64(onet, b, d, act_party, act_actives)
    assert emb.shape == ref.shape
    rows = np.arange(n) if n <= oracle_rows else np.sort(np.random.default_rng(n).choice(n, oracle_rows, replace=False))
    if cnet_path is not None:
        cnet = O.CNet(cnet_path)
        orc = np.stack([cnet.embedding(b[i], d[i], dim=ref.shape[1]) for i in rows])
        cnet.close()
    else:
        orc = E.oracle_embedding(e_ref_net or onet, b, d, rows, act_party, act_actives)
    e_ref, s = E.yardstick(ref, orc, rows)
    worst, lim = E.worst_error(emb, ref), E.bound(e_ref, s)
    dead = E.dead_mask(onet, b, d)
    RECORDS["|".join(key)] = dict(E_ref=e_ref, worst=worst, S=s, bound=lim, share=worst / lim, forms=list(forms), leaves=n,
                                  entries=int(ref.size), dead_entries=int(dead.sum()))
    print("%s: worst %.3g, E_ref %.3g, S %.3g, bound %.3g (%.0f %%) over %d entries, forms %s"
          % (" ".join(key), worst, e_ref, s, lim, 100 * worst / lim, ref.size, forms))
    assert np.isfinite(emb).all(), (key, int((~np.isfinite(emb)).sum()), np.argwhere(~np.isfinite(emb))[:4])
    assert (emb.view(np.uint32)[dead] == 0).all(), (key, np.argwhere(dead & (emb.view(np.uint32) != 0))[:4])
    assert worst <= lim, (key, worst, e_ref, s, lim, np.unravel_index(np.abs(emb - ref).argmax(), ref.shape))


def hold_to_float64(ctx, net, onet, b, d, key, forms, **kw):
    assert embed_forms(ctx, net) == forms, (key, embed_forms(ctx, net), forms)
    emb, vals = gpu_embedding(ctx, net, b, d)
    assert np.isfinite(vals).all()
    check_embedding(emb, onet, b, d, key, forms, **kw)
    return emb


# ---- networks -------------------------------------------------------------------------------------------------------------------
# name -> (party out, active out, party hidden, active hidden): every NBO of both row kernels (party 1 / 2 blocks, actives 1 / 2 / 3)
# with a full and a ragged last block, the hand-over to the tile kernel on either side of 64 / 96, hidden widths 32 ... 128
# (the loader wants an embedding width that is a multiple of 4: party and active outputs of the same parity)
WIDTHS = {
    "p1_a19": (1, 19, 32, 64),
    "p8_a32": (8, 32, 64, 32),
    "p27_a33": (27, 33, 72, 100),
    "p32_a64": (32, 64, 100, 72),
    "p33_a83": (33, 83, 128, 128),
    "p59_a97": (59, 97, 72, 32),       # rows + tile actives
    "p64_a96": (64, 96, 100, 128),
    "p64_a128": (64, 128, 64, 96),     # rows + tile actives
    "p99_a83": (99, 83, 128, 72),      # tile party + rows actives
    "p99_a97": (99, 97, 32, 100),      # tile + tile by width
}


def width_net(tmp_path, name, activation):
    from oak_amd import netfile
    po, ao, ph, ah = WIDTHS[name]
    path = str(tmp_path / ("%s_%d.battle.net" % (name, activation)))
    netfile.write_random_net(path, seed=31, activation=activation, hidden=64, value_hidden=32, pokemon_out=po, active_out=ao,
                             pokemon_hidden=ph, active_hidden=ah)
    return path


def golden_net(tmp_path, tag):
    """default / tiny / 256 as they are (ReLU, clamp, ReLU), or 256_clamp: the 256-wide net with the header's activation byte set."""
    if tag == "256_clamp":
        return P.rewrite_net(NET256, str(tmp_path / "256_clamp.battle.net"), header0=1)
    return P.GOLDEN[tag]


def scale_embedding_nets(s):
    """An edit for policy_ref.rewrite_net: first layers (weights and bias) of both embedding nets x 2^-s, second layers' weights x 2^+s.
    Behind ReLU the same function (powers of two are exact, ReLU commutes with a positive scale)."""
    def edit(i, b, W):
        if i in (0, 2):
            return b * F(2.0 ** -s), W * F(2.0 ** -s)
        if i in (1, 3):
            return b, W * F(2.0 ** s)
        return b, W
    return edit


# ---- 1. forms x nets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", [1, 2], ids=["relu", "clamp"])
@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_every_width_and_routing_against_float64(gpu_ctx, tmp_path, name, activation):
    """Random nets over every output width class of the two row kernels and the tile kernel, both activations, on form_states +
    planted_states (about 16,000 leaves: 160,000 party items = past two sweeps of the party pass's 256 workgroups)."""
    from oak_amd.engine import Network
    path = width_net(tmp_path, name, activation)
    net, onet = Network(gpu_ctx, path=path), NN.Net(path)
    b, d = E.all_states()
    hold_to_float64(gpu_ctx, net, onet, b, d, (name, "relu" if activation == 1 else "clamp", "n%d" % b.shape[0]), expected_forms(onet))
    net.close()


@pytest.mark.parametrize("tag", ["default", "tiny", "256", "256_clamp"])
def test_golden_nets_against_float64(gpu_ctx, tmp_path, tag):
    """The three nets written by the reference's torch mirror (ReLU, clamp, ReLU) and the 256-wide one as a clamp net: k_embed_both."""
    from oak_amd.engine import Network
    path = golden_net(tmp_path, tag)
    net, onet = Network(gpu_ctx, path=path), NN.Net(path)
    b, d = E.all_states()
    hold_to_float64(gpu_ctx, net, onet, b, d, (tag, "fused", "n%d" % b.shape[0]), (FUSED, FUSED, 1 if onet.pod <= 32 else 2))
    net.close()


@pytest.mark.parametrize("tag", ["256", "256_clamp"])
def test_row_kernels_launched_alone_against_float64(tmp_path, tag):
    """A context with kernel timing on puts an event between the passes: k_embed_prows and k_embed_arows as two launches."""
    from oak_amd import _lib
    from oak_amd.engine import Context, Network
    ctx = Context(0)
    _lib.check(ctx.lib.oakgpu_set_kernel_timing(ctx.handle, 1))
    path = golden_net(tmp_path, tag)
    net, onet = Network(ctx, path=path), NN.Net(path)
    b, d = E.all_states()
    hold_to_float64(ctx, net, onet, b, d, (tag, "rows_timing", "n%d" % b.shape[0]), (ROWS, ROWS, 2))
    net.close()
    ctx.close()


def _child_embedding(path, bpath, dpath, out, forms):
    """Runs in the child process of test_forced_tile_form_against_float64."""
    from oak_amd.engine import Context, Network
    ctx = Context(0)
    net = Network(ctx, path=path)
    assert embed_forms(ctx, net) == tuple(forms), embed_forms(ctx, net)
    emb, vals = gpu_embedding(ctx, net, np.load(bpath), np.load(dpath))
    assert np.isfinite(vals).all()
    np.save(out, emb)
    net.close()
    ctx.close()


@pytest.mark.parametrize("tag", ["256", "256_clamp", "tiny"])
def test_forced_tile_form_against_float64(tmp_path, tag):
    """OAKGPU_EMBED_TILE=1 sends both passes of a network the row kernels would take through k_embed_lds (fp32 MFMA): a second
    implementation of the same function, held to the same bound.  The variable is read once per process: a child, with its own timeout."""
    path = golden_net(tmp_path, tag)
    b, d = E.all_states()
    bp, dp, out = str(tmp_path / "b.npy"), str(tmp_path / "d.npy"), str(tmp_path / "emb.npy")
    np.save(bp, b)
    np.save(dp, d)
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_embedding as T; T._child_embedding(%r, %r, %r, %r, %r)"
            % (P.ROOT, TESTS, path, bp, dp, out, (TILE, TILE, 0)))
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, OAKGPU_EMBED_TILE="1"), timeout=300)
    check_embedding(np.load(out), NN.Net(path), b, d, (tag, "forced_tile", "n%d" % b.shape[0]), (TILE, TILE, 0))


# ---- 2. sizes -------------------------------------------------------------------------------------------------------------------
def batch_of(n, seed=7):
    """n leaves of form_states + planted_states: a seeded permutation, repeated when n is larger."""
    b, d = E.all_states()
    idx = np.random.default_rng(seed).permutation(b.shape[0])[np.arange(n) % b.shape[0]]
    return np.ascontiguousarray(b[idx]), np.ascontiguousarray(d[idx])


@pytest.mark.parametrize("n", [1, 3, 4, 7, 13, 32, 33, 205, 257, 3001, FULL])
def test_every_size_against_float64(gpu_ctx, n):
    """k_embed_both on the 256-wide net around its 32-item mini-tiles -- a leaf is 10 party items and 2 actives, so 3 leaves stay
    inside one party mini-tile, 4 and 7 cut a leaf across a tile edge, 13 and 32 / 33 do the same to the actives' -- across workgroups,
    and at 65,569 leaves past one sweep of the 256-workgroup grid in BOTH passes: a sweep is 256 x PR_WAVES x ER_ITEMS = 65,536 party
    items (6,553 leaves) and 256 x AR_WAVES x ER_ITEMS = 65,536 actives (32,768 leaves).  3,001 leaves, the most an embedding was
    compared at before, end inside the first sweep of either pass.  EVERY row of every size; E_ref at full size from the C oracle on
    2,048 sampled rows."""
    from oak_amd.engine import Network
    sweep_p, sweep_a = MAX_WGS * PR_WAVES * ER_ITEMS, MAX_WGS * AR_WAVES * ER_ITEMS
    assert FULL * 10 > sweep_p and FULL * 2 > sweep_a and 3001 * 10 <= sweep_p
    net, onet = Network(gpu_ctx, path=NET256), NN.Net(NET256)
    b, d = batch_of(n)
    kw = dict(cnet_path=NET256, oracle_rows=2048) if n == FULL else {}
    hold_to_float64(gpu_ctx, net, onet, b, d, ("256", "fused", "n%d" % n), (FUSED, FUSED, 2), **kw)
    net.close()


# ---- 3. scaled nets -------------------------------------------------------------------------------------------------------------
def _switch_exponent():
    """The largest s for which the second layers of the 256-wide net's embedding nets, times 2^s, hold no weight above 2^20."""
    onet = NN.Net(NET256)
    big = max(float(np.abs(x.W).max()) for x in (onet.p1, onet.a1))
    s = int(np.floor(20 - np.log2(big)))
    assert big * 2.0 ** s <= 2.0 ** 20 < big * 2.0 ** (s + 1)
    return s


@pytest.mark.parametrize("case", ["down20_up20", "below_the_switch", "above_the_switch", "down110_up110"])
def test_scaled_embedding_nets_against_float64(gpu_ctx, tmp_path, case):
    """First layers of both embedding nets of the 256-wide ReLU net x 2^-s, second layers x 2^+s: the same function, so the float64
    reference, E_ref (the numpy oracle) and S are the UNSCALED net's.  s = 20 stays on the row kernels; the loader sends a network
    with a second-layer weight above 2^20 through k_embed_lds (what a flushed low part of the first layer's bf16 triples loses would
    come back multiplied up) -- held on both sides of that switch, one power of two apart, and at s = 110."""
    from oak_amd.engine import Network
    edge = _switch_exponent()
    s = {"down20_up20": 20, "below_the_switch": edge, "above_the_switch": edge + 1, "down110_up110": 110}[case]
    path = P.rewrite_net(NET256, str(tmp_path / (case + ".battle.net")), scale_embedding_nets(s))
    net, onet, scaled = Network(gpu_ctx, path=path), NN.Net(NET256), NN.Net(path)
    assert (max(float(np.abs(x.W).max()) for x in (scaled.p1, scaled.a1)) > 2.0 ** 20) == (s > edge)     # the premise of the expected form
    b, d = E.all_states()
    same = E.embedding_f64(scaled, b[:512], d[:512])
    # (the premise: the same function.  Exactly so up to s ~ 100; at s = 110 the smallest first-layer weights of the FILE are fp32
    # subnormals and the two float64 evaluations differ by 3e-13, a millionth of the bound)
    assert np.abs(same - E.embedding_f64(onet, b[:512], d[:512])).max() <= 1e-11
    hold_to_float64(gpu_ctx, net, onet, b, d, ("256_" + case, "s%d" % s, "n%d" % b.shape[0]), expected_forms(onet, safe=s <= edge))
    net.close()


def test_clamp_net_with_a_weight_above_the_switch_against_float64(gpu_ctx, tmp_path):
    """The tile + tile routing on a clamp net: the 256-wide net as a clamp net with its embedding nets scaled by 2^-+110.  Behind a clamp
    that is another function than the unscaled net's, so reference and oracle are the scaled file's own."""
    from oak_amd.engine import Network
    path = P.rewrite_net(NET256, str(tmp_path / "clamp110.battle.net"), scale_embedding_nets(110), header0=1)
    net, onet = Network(gpu_ctx, path=path), NN.Net(path)
    b, d = E.all_states()
    hold_to_float64(gpu_ctx, net, onet, b, d, ("256_clamp_down110_up110", "s110", "n%d" % b.shape[0]), (TILE, TILE, 0))
    net.close()


# ---- 4. the discrete handle -----------------------------------------------------------------------------------------------------
def test_discrete_handle_embedding_against_float64(gpu_ctx, tmp_path):
    """A network loaded with discrete=True keeps fp32 embedding nets -- party slots with ReLU, actives with clamp -- and embedding_out
    is that fp32 embedding before quantization (include/oakgpu.h): the same bound, with reference and oracle run per pass."""
    from oak_amd.engine import Network
    path = P.rewrite_net(P.GOLDEN["default"], str(tmp_path / "default_int8.battle.net"), P.spread_main_net, header0=1)
    net, onet = Network(gpu_ctx, path=path, discrete=True), NN.Net(path)
    b, d = E.all_states()
    hold_to_float64(gpu_ctx, net, onet, b, d, ("default_int8", "party_relu_actives_clamp", "n%d" % b.shape[0]), expected_forms(onet),
                    act_party=1, act_actives=2)
    net.close()


# ---- 5. properties at full size, and the cached call ------------------------------------------------------------------------------
ROUTINGS = {
    "fused_nbo2": (FUSED, FUSED, 2),
    "fused_nbo1": (FUSED, FUSED, 1),
    "rows_timing": (ROWS, ROWS, 2),
    "rows_tile_actives": (ROWS, TILE, 2),
    "tile_party_rows": (TILE, ROWS, 0),
    "tile_tile": (TILE, TILE, 0),
}


class _Routing:
    """Context, network and oracle net of one of ROUTINGS."""

    def __init__(self, gpu_ctx, tmp_path, case):
        from oak_amd import _lib
        from oak_amd.engine import Context, Network
        self.ctx, self.own = gpu_ctx, None
        path = {"fused_nbo2": NET256, "fused_nbo1": P.GOLDEN["tiny"], "rows_timing": NET256}.get(case)
        if case == "rows_tile_actives":
            path = width_net(tmp_path, "p64_a128", 1)
        elif case == "tile_party_rows":
            path = width_net(tmp_path, "p99_a83", 2)
        elif case == "tile_tile":
            path = P.rewrite_net(NET256, str(tmp_path / "unsafe.battle.net"), scale_embedding_nets(110))
        if case == "rows_timing":
            self.ctx = self.own = Context(0)
            _lib.check(self.ctx.lib.oakgpu_set_kernel_timing(self.ctx.handle, 1))
        self.net, self.onet = Network(self.ctx, path=path), NN.Net(path)
        assert embed_forms(self.ctx, self.net) == ROUTINGS[case], (case, embed_forms(self.ctx, self.net))

    def close(self):
        self.net.close()
        if self.own is not None:
            self.own.close()


@pytest.mark.parametrize("case", sorted(ROUTINGS))
def test_full_size_batch_is_repeatable_and_permutes(gpu_ctx, tmp_path, case):
    """65,569 leaves in every routing, bit for bit: the call is repeatable, and a permuted batch gives the permuted rows -- no entry
    depends on the lane, wave, mini-tile, workgroup or sweep its leaf lands in.  (The batch repeats the 16,000 states the tests above
    hold to float64 row by row, so this extends their bound to every row of the full size.)"""
    r = _Routing(gpu_ctx, tmp_path, case)
    b, d = batch_of(FULL, seed=11)
    e0, v0 = gpu_embedding(r.ctx, r.net, b, d)
    assert np.isfinite(e0).all() and (e0.view(np.uint32)[E.dead_mask(r.onet, b, d)] == 0).all()
    e1, v1 = gpu_embedding(r.ctx, r.net, b, d)
    assert np.array_equal(e0.view(np.uint32), e1.view(np.uint32)) and np.array_equal(v0, v1)
    perm = np.random.default_rng(5).permutation(FULL)
    e2, v2 = gpu_embedding(r.ctx, r.net, np.ascontiguousarray(b[perm]), np.ascontiguousarray(d[perm]))
    assert np.array_equal(e2.view(np.uint32), e0.view(np.uint32)[perm]) and np.array_equal(v2, v0[perm])
    r.close()


@pytest.mark.parametrize("case", sorted(ROUTINGS))
def test_cached_call_on_the_planted_batch(gpu_ctx, tmp_path, case):
    """oakgpu_leaf_eval_cached_dev on form_states + planted_states, from tags of 0xFF bytes (the contract's start) and an embedding buffer
    of NaN words between guard bands: bit-identical to the plain call -- so every entry is written, dead ones as +0.0 -- and it
    re-embeds exactly the live slots; called again it re-embeds none; with every leaf moved one lane on it re-embeds the slots whose
    key differs from the lane's previous one (oracle_lib.expected_recomputes), still bit-identical to the plain call."""
    from hipmem import Dev
    from oak_amd import _lib
    r = _Routing(gpu_ctx, tmp_path, case)
    b, d = E.all_states()
    n, dim = b.shape[0], r.net.shape()[0]
    gb, gd, gv = Dev(b), Dev(d), Dev(np.zeros(n, F), fill=0xFF)
    ge, tags = Guarded(n, dim), Dev(np.zeros((n, 10, 6), np.uint32), fill=0xFF)
    prev = None
    for step, (bb, dd) in enumerate(((b, d), (b, d), (np.roll(b, 1, axis=0), np.roll(d, 1, axis=0)))):
        bb, dd = np.ascontiguousarray(bb), np.ascontiguousarray(dd)
        gb.put(bb)
        gd.put(dd)
        _lib.check(r.ctx.lib.oakgpu_leaf_eval_cached_dev(r.ctx.handle, r.net.handle, gb.p, gd.p, n, gv.p, ge.p, tags.p))
        got = C.c_uint32()
        _lib.check(r.ctx.lib.oakgpu_leaf_cache_last_count(r.ctx.handle, C.byref(got)))
        r.ctx.synchronize()
        cached, vals = ge.host(), gv.host()
        plain, pvals = gpu_embedding(r.ctx, r.net, bb, dd)
        bad = np.nonzero((plain.view(np.uint32) != cached.view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, (case, step, int(bad[0]))
        assert np.array_equal(vals, pvals)
        keys, live = O.party_slot_keys(bb, dd)
        want = O.expected_recomputes(prev, keys, live)
        assert got.value == want and (step != 1 or want == 0) and (step == 1 or want > 0), (case, step, got.value, want)
        prev = keys
    for x in (gb, gd, gv, ge, tags):
        x.free()
    r.close()
