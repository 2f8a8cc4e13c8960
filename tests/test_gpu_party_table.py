"""GPU: the per-search bench-slot embedding table (include/oakgpu.h, oakgpu_party_table_*: NN::Battle::PokemonCache filled once per
root, k_party_variants + the party kernel's work-list form, looked up by k_party_lookup).  A table row is produced by the very
arithmetic of the plain party pass, so every comparison here is BITWISE against oakgpu_leaf_eval_dev / oakgpu_leaf_eval_policy_dev
on the same device buffers; the numpy network oracle is consulted on every 97th lane only."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nn_oracle as NN  # noqa: E402
import oracle_lib as O  # noqa: E402
import party_table_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
NET_DEFAULT = os.path.join(ROOT, "tests", "golden", "net_default.battle.net")
NET256 = os.path.join(ROOT, "tests", "golden", "net_256.battle.net")
GUARD = 1024      # floats on either side of an output buffer

# The forms of the party pass (OAKGPU_EMBED_FORM_*, include/oakgpu.h), as tests/test_gpu_leafnet.py::CACHE_FORMS names them: case ->
# (party pass, actives' pass, output blocks per wave of the party row kernel) as oakgpu_leaf_embed_forms reports them.  The table's
# fill and its miss fallback run the work-list instantiation of the party kernel named.
FUSED, ROWS, TILE = 3, 2, 1
FORMS = {
    "rows_nbo2": (FUSED, FUSED, 2),            # NET256: party out 59
    "rows_nbo1": (FUSED, FUSED, 1),            # net_tiny: party out 8
    "prows_timing": (ROWS, ROWS, 2),           # NET256 on a context with kernel timing on (an event between the passes)
    "tile_list_wide": (TILE, ROWS, 0),         # party out 99
    "tile_list_unsafe": (TILE, TILE, 0),       # second-layer weights above 2^20: not embed_safe
}


def _rewrite_net(src, dst, edit):
    raw = open(src, "rb").read()
    out, off = [raw[:8]], 8
    for i in range(12):
        n_in, n_out = struct.unpack_from("<II", raw, off)
        off += 8
        b = np.frombuffer(raw, "<f4", n_out, off).copy()
        off += 4 * n_out
        W = np.frombuffer(raw, "<f4", n_out * n_in, off).copy().reshape(n_out, n_in)
        off += 4 * n_out * n_in
        b, W = edit(i, b, W)
        out += [struct.pack("<II", n_in, n_out), b.astype("<f4").tobytes(), W.astype("<f4").tobytes()]
    assert off == len(raw)
    open(dst, "wb").write(b"".join(out))


class _Case:
    """The network (and context) of one FORMS case, its oracle, and the check that the case runs the forms it is named after."""

    def __init__(self, gpu_ctx, tmp_path, case, discrete_path=None):
        from oak_amd import _lib, netfile
        from oak_amd.engine import Context, Network
        self.ctx, self.own_ctx = gpu_ctx, None
        path = oracle_path = NET256
        if case == "rows_nbo1":
            path = oracle_path = os.path.join(ROOT, "tests", "golden", "net_tiny.battle.net")
        elif case == "tile_list_wide":
            path = oracle_path = str(tmp_path / "wide_party.battle.net")
            netfile.write_random_net(path, seed=3, hidden=64, value_hidden=32, pokemon_out=99)
        elif case == "tile_list_unsafe":       # the same function as NET256, its embedding nets' layers scaled by 2^-110 / 2^+110
            path = str(tmp_path / "unsafe.battle.net")
            _rewrite_net(NET256, path, lambda i, b, W: (b * np.float32(2.0 ** -110), W * np.float32(2.0 ** -110)) if i in (0, 2)
                         else (b, W * np.float32(2.0 ** 110)) if i in (1, 3) else (b, W))
        if case == "prows_timing":
            self.ctx = self.own_ctx = Context(0)
            _lib.check(self.ctx.lib.oakgpu_set_kernel_timing(self.ctx.handle, 1))
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        if discrete_path is not None:
            self.net, self.onet = Network(self.ctx, path=discrete_path, discrete=True), None
        else:
            self.net, self.onet = Network(self.ctx, path=path), NN.Net(oracle_path)
            forms = [C.c_int(-1), C.c_int(-1), C.c_int(-1)]
            _lib.check(self.lib.oakgpu_leaf_embed_forms(self.h, self.net.handle, *[C.byref(f) for f in forms]))
            assert tuple(f.value for f in forms) == FORMS[case], (case, [f.value for f in forms])
        self.emb_dim = self.net.shape()[0]

    def close(self):
        self.net.close()
        if self.own_ctx is not None:
            self.own_ctx.close()


class _Guarded:
    """n x width floats on the device between two guard bands, everything prefilled with 0x7F bytes."""

    def __init__(self, n, width):
        from hipmem import Dev
        self.n, self.width = n, width
        self.dev = Dev(np.zeros(2 * GUARD + n * width, np.float32), fill=0x7F)
        self.p = C.c_void_p(self.dev.p.value + 4 * GUARD)

    def refill(self):
        from hipmem import hip
        assert hip().hipMemset(self.dev.p, 0x7F, self.dev.nbytes) == 0

    def host(self):
        """The payload as uint32 bit patterns [n, width]; asserts the guard bands untouched."""
        raw = self.dev.host().view(np.uint32)
        assert (raw[:GUARD] == 0x7F7F7F7F).all() and (raw[GUARD + self.n * self.width:] == 0x7F7F7F7F).all(), "guard band written"
        return raw[GUARD:GUARD + self.n * self.width].reshape(self.n, self.width)

    def free(self):
        self.dev.free()


class _TableAndPlain:
    """call(): oakgpu_leaf_eval_dev and oakgpu_leaf_eval_table_dev on the same device battles; asserts embeddings and values
    bit-identical, every float of the table call's output written, the guard bands untouched; returns (embedding bits, values,
    misses) of the table call."""

    def __init__(self, cc, table, n):
        self.cc, self.table, self.n = cc, table, n
        self.e_plain, self.e_table = _Guarded(n, cc.emb_dim), _Guarded(n, cc.emb_dim)
        self.v_plain, self.v_table = _Guarded(n, 1), _Guarded(n, 1)

    def call(self, gb, gd, what, root_of=None, expect_bad_roots=False):
        from oak_amd import _lib
        cc, n = self.cc, self.n
        for g in (self.e_plain, self.e_table, self.v_plain, self.v_table):
            g.refill()
        _lib.check(cc.lib.oakgpu_leaf_eval_dev(cc.h, cc.net.handle, gb.p, gd.p, n, self.v_plain.p, self.e_plain.p))
        _lib.check(cc.lib.oakgpu_leaf_eval_table_dev(cc.h, cc.net.handle, self.table.handle, None if root_of is None else root_of.p, gb.p, gd.p, n,
                                                     self.v_table.p, self.e_table.p))
        got = C.c_uint32(0xFFFFFFFF)
        rc = cc.lib.oakgpu_party_table_last_misses(cc.h, self.table.handle, C.byref(got))
        if expect_bad_roots:
            assert rc != 0 and b"root_of" in cc.lib.oakgpu_last_error(), what
        else:
            _lib.check(rc)
        cc.ctx.synchronize()
        ep, et = self.e_plain.host(), self.e_table.host()
        bad = np.nonzero((ep != et).any(axis=1))[0]
        assert bad.size == 0, (what, "lane", int(bad[0]), "floats", np.nonzero(ep[bad[0]] != et[bad[0]])[0][:8], "of", bad.size, "lanes")
        vp, vt = self.v_plain.host(), self.v_table.host()
        assert (vp == vt).all(), what
        return et, vt.view(np.float32).reshape(n), got.value

    def free(self):
        for x in (self.e_plain, self.e_table, self.v_plain, self.v_table):
            x.free()


def _oracle_check(cc, vals, b, d, what):
    for i in range(0, b.shape[0], 97):
        assert abs(float(vals[i]) - float(NN.value_inference(cc.onet, b[i], d[i]))) <= TOL, (what, i)


def _descendants(root_b, root_d, root_r, n, steps, seed):
    """n copies of a root advanced steps[k] random turn-steps on the CPU oracle (consecutive parts), one prng stream per lane."""
    b, d = np.repeat(root_b.reshape(1, 384), n, axis=0), np.repeat(root_d.reshape(1, 8), n, axis=0)
    r = np.full(n, int(root_r), dtype=np.uint8)
    p = np.random.default_rng(seed).integers(1, 1 << 63, size=n, dtype=np.uint64).view(np.uint8).reshape(n, 8).copy()
    for k, idx in zip(steps, np.array_split(np.arange(n), len(steps))):
        if k:
            bb, dd, pp, rr = (np.ascontiguousarray(x[idx]) for x in (b, d, p, r))
            O.rollout_batch(bb, dd, rr, pp, max_steps=k, threads=4)
            b[idx], d[idx] = bb, dd
    return b, d


@pytest.mark.parametrize("case", list(FORMS))
def test_every_table_row_equals_the_plain_pass_on_that_variant(gpu_ctx, tmp_path, case):
    """The 2,880 variants of a root's twelve Pokemon (tests/party_table_ref.py: the reference's enumeration) placed in the bench slots of
    288 synthetic leaves -- the root with its actives kept, variant 10 L + q in bench slot q of leaf L -- and evaluated by the plain
    call: each slot's block equals row `key` of that Pokemon in oakgpu_party_table_rows, bit for bit."""
    from hipmem import Dev
    from oak_amd import _lib
    from oak_amd.engine import PartyTable
    cc = _Case(gpu_ctx, tmp_path, case)
    rb, rd, rp, rr = O.make_random_ou_batch(1, seed0=0x7AB1E0)
    O.rollout_batch(rb, rd, rr, rp, max_steps=12)
    root = rb[0].copy()
    table = PartyTable(cc.ctx, cc.net).fill(root)
    p_out = table.width
    assert p_out == cc.onet.pod
    rows = np.stack([table.rows(0, p // 6, p % 6) for p in range(12)]).view(np.uint32)          # [12, 240, p_out]
    n = 288
    b, d = np.repeat(root.reshape(1, 384), n, axis=0), np.repeat(rd[0].reshape(1, 8), n, axis=0)
    keys = np.zeros((n, 10), np.int64)
    for p in range(12):
        base = root[184 * (p // 6) + 24 * (p % 6):184 * (p // 6) + 24 * (p % 6 + 1)]
        for v, sleep in R.variants(base):
            k = R.key(v, sleep)
            item = p * 240 + k
            leaf, q = item // 10, item % 10
            s, pos = q // 5, q % 5 + 1
            t = int(b[leaf, 184 * s + 176 + pos]) - 1
            assert t >= 0
            v = v.copy()
            if not (v[18] | v[19]):
                v[18] = 1                      # (a Pokemon fainted at the root: hp is no input of the embedding)
            b[leaf, 184 * s + 24 * t:184 * s + 24 * (t + 1)] = v
            w = int.from_bytes(bytes(d[leaf, 4 * s:4 * s + 4]), "little")
            w = (w & ~(7 << (3 * pos))) | (sleep << (3 * pos))
            d[leaf, 4 * s:4 * s + 4] = np.frombuffer(w.to_bytes(4, "little"), np.uint8)
            keys[leaf, q] = k
    gb, gd = Dev(b), Dev(d)
    vals, emb = Dev(np.zeros(n, np.float32)), Dev(np.zeros((n, cc.emb_dim), np.float32), fill=0x7F)
    _lib.check(cc.lib.oakgpu_leaf_eval_dev(cc.h, cc.net.handle, gb.p, gd.p, n, vals.p, emb.p))
    cc.ctx.synchronize()
    e = emb.host().view(np.uint32)
    side_dim = cc.emb_dim // 2
    aod = side_dim - 1 - 5 * (1 + p_out)
    for leaf in range(n):
        for q in range(10):
            o = (q // 5) * side_dim + (1 + aod) + (q % 5) * (1 + p_out)
            p = (leaf * 10 + q) // 240
            assert (e[leaf, o + 1:o + 1 + p_out] == rows[p, keys[leaf, q]]).all(), (case, leaf, q, p, int(keys[leaf, q]))
    for x in (gb, gd, vals, emb):
        x.free()
    table.close()
    cc.close()


@pytest.mark.parametrize("case,n", [(c, n) for c in FORMS for n in (3001, 1, 205)])
def test_descendants_of_the_root_hit_every_slot(gpu_ctx, tmp_path, case, n):
    """n lanes start from one random OU root and are stepped 45 turns on the device: every turn the table call's values and whole
    embedding equal the plain call's, no slot misses (a stored Pokemon's identity never changes), the 0x7F prefill is gone and the
    guard bands are untouched."""
    from hipmem import Dev
    from oak_amd import _lib
    from oak_amd.engine import PartyTable
    cc = _Case(gpu_ctx, tmp_path, case)
    rb, rd, rp, rr = O.make_random_ou_batch(1, seed0=0xDE5CE0)
    table = PartyTable(cc.ctx, cc.net).fill(rb[0])
    _, _, p, _ = O.make_random_ou_batch(n, seed0=0xDE5CE1)
    gb, gd = Dev(np.repeat(rb, n, axis=0)), Dev(np.repeat(rd, n, axis=0))
    gp, gr = Dev(p), Dev(np.repeat(np.asarray(rr, np.uint8).reshape(1), n))
    steps, vals = Dev(np.zeros(n, np.uint32)), Dev(np.zeros(n, np.float32))
    tp = _TableAndPlain(cc, table, n)
    for turn in range(45):
        _lib.check(cc.lib.oakgpu_rollout_dev(cc.h, gb.p, gd.p, gr.p, gp.p, n, 1, 0, gr.p, steps.p, vals.p, gb.p, gd.p))   # one turn, in place
        cc.ctx.synchronize()
        et, vt, misses = tp.call(gb, gd, (case, turn))
        assert misses == 0, (case, turn, misses)
        assert not (et == 0x7F7F7F7F).any(), (case, turn)
    _oracle_check(cc, vt, gb.host(), gd.host(), case)
    for x in (gb, gd, gp, gr, steps, vals):
        x.free()
    tp.free()
    table.close()
    cc.close()


@pytest.mark.parametrize("case", list(FORMS))
def test_several_roots_and_root_of(gpu_ctx, tmp_path, case):
    """Three roots with different teams, their descendants shuffled over the batch with root_of naming each leaf's root: identical to
    the plain call with no miss; root_of = NULL with a one-root table; and root_of entries beyond the filled roots are reported by
    the diagnostic call, not followed -- those leaves' slots are embedded as misses and the results are still the plain call's."""
    from hipmem import Dev
    from oak_amd.engine import PartyTable
    cc = _Case(gpu_ctx, tmp_path, case)
    rb, rd, rp, rr = O.make_random_ou_batch(3, seed0=0x3007)
    per = 100
    parts = [_descendants(rb[k], rd[k], rr[k], per, (0, 7, 25, 60), 50 + k) for k in range(3)]
    b, d = np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])
    root_of = np.repeat(np.arange(3, dtype=np.uint32), per)
    perm = np.random.default_rng(9).permutation(3 * per)
    b, d, root_of = b[perm].copy(), d[perm].copy(), root_of[perm].copy()
    n = 3 * per
    table = PartyTable(cc.ctx, cc.net, max_roots=4).fill(rb)
    gb, gd, gro = Dev(b), Dev(d), Dev(root_of)
    tp = _TableAndPlain(cc, table, n)
    et, vt, misses = tp.call(gb, gd, (case, "three roots"), root_of=gro)
    assert misses == 0 == R.expected_misses(rb, root_of, b)
    _oracle_check(cc, vt, b, d, case)
    # every leaf looked up in root 0: the other roots' descendants miss, and are embedded
    et, vt, misses = tp.call(gb, gd, (case, "all in root 0"))
    assert misses == R.expected_misses(rb, None, b) > 0
    # out of range: roots 3 (allocated, never filled) and 2^31
    bad = root_of.copy()
    bad[::7], bad[3::11] = 3, 1 << 31
    gro.put(bad)
    et, vt, misses = tp.call(gb, gd, (case, "root_of out of range"), root_of=gro, expect_bad_roots=True)
    assert misses == R.expected_misses(rb, bad, b) > 0
    # NULL root_of with a one-root table
    one = PartyTable(cc.ctx, cc.net).fill(rb[1])
    sel = np.nonzero(root_of == 1)[0]
    g1b, g1d = Dev(b[sel]), Dev(d[sel])
    tp1 = _TableAndPlain(cc, one, sel.size)
    et, vt, misses = tp1.call(g1b, g1d, (case, "one root, NULL"))
    assert misses == 0
    for x in (gb, gd, gro, g1b, g1d):
        x.free()
    tp.free(); tp1.free()
    table.close(); one.close()
    cc.close()


@pytest.mark.parametrize("case", list(FORMS))
def test_slots_the_table_does_not_hold_are_embedded(gpu_ctx, tmp_path, case):
    """A table filled from root A; 512 leaves, half descended from A and half from other teams; one field of one bench slot of every
    lane changed per call (oracle_lib.bench_slot_mutations: species, level, each stat, each move id, types, PP, statuses, order
    swaps, an emptied slot, hp 0 and back ...): always identical to the plain call, the misses counted are the restatement's, an
    hp-0 or emptied slot's block is all zeros (hp cell included) and the hp-ratio cell follows hp."""
    from hipmem import Dev
    from oak_amd.engine import PartyTable
    cc = _Case(gpu_ctx, tmp_path, case)
    n = 512
    rb, rd, rp, rr = O.make_random_ou_batch(1, seed0=0xA11CE)
    ba, da = _descendants(rb[0], rd[0], rr[0], n // 2, (0, 10, 30), 77)
    bo, do = O.midgame_batch(n // 2, seed0=0x5107)
    b, d = np.concatenate([ba, bo]), np.concatenate([da, do])
    table = PartyTable(cc.ctx, cc.net).fill(rb[0])
    side, pos = O.bench_slot_choice(b, seed=11)
    rng, memo = np.random.default_rng(12), {}
    gb, gd = Dev(b), Dev(d)
    tp = _TableAndPlain(cc, table, n)
    p_out = table.width
    side_dim = cc.emb_dim // 2
    block = side * side_dim + (side_dim - 5 * (1 + p_out)) + (pos - 1) * (1 + p_out)      # the chosen slot's block: hp ratio, embedding
    lanes = np.arange(n)
    seen = []
    for name, fn in [("fill", None)] + O.bench_slot_mutations():
        if fn is not None:
            fn(b, d, side, pos, rng, memo)
            gb.put(b); gd.put(d)
        et, vt, misses = tp.call(gb, gd, (case, name))
        exp = R.expected_misses(rb, None, b)
        assert misses == exp, (case, name, misses, exp)
        seen.append(misses)
        _oracle_check(cc, vt, b, d, (case, name))
        if name in ("hp_zero", "empty_slot"):
            assert (et[lanes[:, None], block[:, None] + np.arange(1 + p_out)] == 0).all(), name
        if name == "hp":
            pid = b[lanes, 184 * side + 176 + pos].astype(np.int64)
            pk = b[lanes[:, None], 184 * side[:, None] + 24 * np.maximum(pid - 1, 0)[:, None] + np.arange(24)]
            hp, mx = pk[:, 18] + 256 * pk[:, 19].astype(np.int64), pk[:, 0] + 256 * pk[:, 1].astype(np.int64)
            live = (pid > 0) & (hp > 0)
            assert (et[lanes, block].view(np.float32)[live] == (hp[live].astype(np.float32) / mx[live].astype(np.float32))).all()
    # A's descendants all hit at first and the other teams' live slots all miss; the identity mutations turn hits into misses
    assert seen[0] == int(R.bench_slots(bo)[2].sum()) and R.expected_misses(rb, None, b[:n // 2]) > 0 and len(set(seen)) > 1
    gb.free(); gd.free()
    tp.free()
    table.close()
    cc.close()


@pytest.mark.parametrize("case", list(FORMS))
def test_short_teams_a_fainted_root_pokemon_and_a_duplicate_move(gpu_ctx, tmp_path, case):
    """A root with teams of four and three (empty team slots get an identity nothing matches), a bench Pokemon fainted at the root,
    and one with the same move id in two slots, one of them at PP 0: fill and lookup stay identical to the plain call, no miss."""
    from hipmem import Dev
    from oak_amd.engine import PartyTable
    from test_oracle_goldens import benchmark_teams
    cc = _Case(gpu_ctx, tmp_path, case)
    teams = np.array(benchmark_teams(), dtype=np.uint8).reshape(2, 6, 5).copy()
    teams[0, 4:] = 0
    teams[1, 3:] = 0
    root = O.init_battle(teams, 0x51DE)
    rd = np.zeros(8, np.uint8)
    assert root[24 * 4 + 21] == 0 and root[184 + 24 * 3 + 21] == 0          # species 0: empty team slots
    t = int(root[176 + 2]) - 1                                              # side 0, bench position 2: fainted at the root
    root[24 * t + 18:24 * t + 20] = 0
    t = int(root[176 + 1]) - 1                                              # side 0, bench position 1: move 2 := move 1, at PP 0
    root[24 * t + 12], root[24 * t + 13] = root[24 * t + 10], 0
    n = 64
    b, d = _descendants(root, rd, 0, n, (0, 1, 6, 20), 5)
    table = PartyTable(cc.ctx, cc.net).fill(root)
    assert (table.rows(0, 0, 5) == 0).all() and (table.rows(0, 1, 3) == 0).all()      # an empty team slot's rows
    gb, gd = Dev(b), Dev(d)
    tp = _TableAndPlain(cc, table, n)
    et, vt, misses = tp.call(gb, gd, "short teams")
    assert misses == 0 == R.expected_misses(root, None, b)
    _oracle_check(cc, vt, b, d, "short teams")
    # a leaf that gives an empty team slot of the root a live Pokemon: a miss, embedded
    b2 = b.copy()
    b2[:, 24 * 4:24 * 5] = b2[:, 0:24]
    b2[:, 24 * 4 + 18] |= 1
    b2[:, 176 + 5] = 5
    gb.put(b2)
    et, vt, misses = tp.call(gb, gd, "empty team slot made live")
    assert misses == R.expected_misses(root, None, b2) >= n
    gb.free(); gd.free()
    tp.free()
    table.close()
    cc.close()


def test_discrete_network_through_the_table(gpu_ctx, tmp_path):
    """The quantized network (party slots embedded with ReLU, as the reference's cache fills them): values and fp32 embeddings through
    the table equal the plain call's."""
    from hipmem import Dev
    from oak_amd.engine import PartyTable
    from test_gpu_discrete import make_net
    cc = _Case(gpu_ctx, tmp_path, "rows_nbo2", discrete_path=make_net(tmp_path, "q128.battle.net", 128, 64, 64))
    rb, rd, rp, rr = O.make_random_ou_batch(1, seed0=0xD15C)
    n = 205
    b, d = _descendants(rb[0], rd[0], rr[0], n, (0, 5, 20, 50), 3)
    table = PartyTable(cc.ctx, cc.net).fill(rb[0])
    gb, gd = Dev(b), Dev(d)
    tp = _TableAndPlain(cc, table, n)
    et, vt, misses = tp.call(gb, gd, "discrete")
    assert misses == 0 and 0 < float(vt.min()) and float(vt.max()) < 1 and np.unique(vt).size > 10
    gb.free(); gd.free()
    tp.free()
    table.close()
    cc.close()


@pytest.mark.parametrize("case", list(FORMS))
def test_policy_form_through_the_table(gpu_ctx, tmp_path, case):
    """oakgpu_leaf_eval_policy_table_dev at n = 205: value and both logit arrays equal oakgpu_leaf_eval_policy_dev's."""
    from hipmem import Dev
    from oak_amd import _lib
    from oak_amd.engine import PartyTable
    cc = _Case(gpu_ctx, tmp_path, case)
    rb, rd, rp, rr = O.make_random_ou_batch(1, seed0=0x9011C)
    n = 205
    b, d = _descendants(rb[0], rd[0], rr[0], n, (0, 5, 20), 4)
    res = np.array([O.LIB.oracle_result_from_state(O.ptr(b[i])) for i in range(n)], dtype=np.uint8)
    c1, n1 = cc.ctx.choices(b, res, 0)
    c2, n2 = cc.ctx.choices(b, res, 1)
    table = PartyTable(cc.ctx, cc.net).fill(rb[0])
    gb, gd = Dev(b), Dev(d)
    gc = [Dev(np.ascontiguousarray(x, dtype=np.uint8)) for x in (c1, n1, c2, n2)]
    outs = []
    for use_table in (False, True):
        v, l1, l2 = _Guarded(n, 1), _Guarded(n, 9), _Guarded(n, 9)
        if use_table:
            _lib.check(cc.lib.oakgpu_leaf_eval_policy_table_dev(cc.h, cc.net.handle, table.handle, None, gb.p, gd.p, n, gc[0].p, gc[1].p, gc[2].p,
                                                                gc[3].p, v.p, l1.p, l2.p))
            assert table.last_misses() == 0
        else:
            _lib.check(cc.lib.oakgpu_leaf_eval_policy_dev(cc.h, cc.net.handle, gb.p, gd.p, n, gc[0].p, gc[1].p, gc[2].p, gc[3].p, v.p, l1.p, l2.p))
        cc.ctx.synchronize()
        outs.append((v.host(), l1.host(), l2.host()))
        for x in (v, l1, l2):
            x.free()
    for a, t in zip(*outs):
        assert (a == t).all()
    assert np.unique(outs[1][1]).size > n                    # (logits were computed)
    # the host layer's table= option is the same call
    v, l1, l2 = cc.net.value_policy_inference(b, d, c1, n1, c2, n2, table=table)
    assert (v.view(np.uint32) == outs[1][0][:, 0]).all() and (l1.view(np.uint32) == outs[1][1]).all() and (l2.view(np.uint32) == outs[1][2]).all()
    v2, e2 = cc.net.value_inference(b, d, return_embedding=True, table=table, root_of=np.zeros(n, np.uint32))
    v3, e3 = cc.net.value_inference(b, d, return_embedding=True)
    assert (v2.view(np.uint32) == v3.view(np.uint32)).all() and (e2.view(np.uint32) == e3.view(np.uint32)).all()
    for x in [gb, gd] + gc:
        x.free()
    table.close()
    cc.close()


def _same_output(a, b):
    """Every field of the two oakgpu_search_output structs but the wall-clock duration, as bytes (both matrices, the values, the Nash
    and empirical strategies, logits and priors, node and depth counts)."""
    from oak_amd import _lib
    for name, _ in _lib.SearchOutput._fields_:
        if name == "duration_us":
            continue
        x, y = getattr(a["raw"], name), getattr(b["raw"], name)
        x, y = (bytes(x), bytes(y)) if hasattr(x, "_length_") else (struct.pack("<d", x), struct.pack("<d", y)) if isinstance(x, float) else (x, y)
        assert x == y, name


def test_search_and_selfplay_do_not_change_with_the_switch(gpu_ctx, tmp_path):
    """Same seed, same thread count, 4,096 iterations: a value-only bandit with the network evaluator, a contextual bandit and a
    value-only bandit with a quantized network, the context's switch off against on -- every field of the oakgpu_search_output is
    equal; and one short self-play game, whose record is byte-identical.  oakgpu_search_party_table_stats shows that the switch-on
    searches did fill a table and sent every one of their batches through it, and the switch-off ones none."""
    from test_gpu_discrete import make_net
    from oak_amd import gamedata as G
    from oak_amd.engine import Context, Network
    from oak_amd.frames import selfplay_game
    from oak_amd.search import tree_search
    ctx = Context(0)                                  # (a context of its own: the switch is per context)
    net = Network(ctx, path=NET_DEFAULT)
    qnet = Network(ctx, path=make_net(tmp_path, "q64.battle.net", 64, 32, 32), discrete=True)
    rb, rd, rp, rr = O.make_random_ou_batch(1, seed0=0x5EA7C4)
    O.rollout_batch(rb, rd, rr, rp, max_steps=9)
    team = lambda rows: [[G.match_species(s)] + [G.match_move(m) for m in ms] for s, ms in rows] + [[0] * 5] * (6 - len(rows))
    teams = np.array([team([("Tauros", ("bodyslam", "hyperbeam", "earthquake", "blizzard")), ("Starmie", ("surf", "thunderbolt", "blizzard", "psychic")),
                            ("Zapdos", ("thunderbolt", "drillpeck", "skyattack", "hyperbeam"))]),
                      team([("Snorlax", ("bodyslam", "hyperbeam", "earthquake", "selfdestruct")), ("Alakazam", ("psychic", "seismictoss", "megakick", "triattack")),
                            ("Rhydon", ("earthquake", "rockslide", "bodyslam", "submission"))])], dtype=np.uint8)
    got = {}
    try:
        for on in (False, True):
            ctx.set_search_party_table(on)
            got[on] = [tree_search(ctx, rb[0], rd[0], int(rr[0]), iterations=4096, batch=512, bandit=bandit, evaluator=ev, c=1.5, seed=21)
                       for bandit, ev in (("ucb", net), ("pucb", net), ("ucb", qnet))]
            # three searches of 4,096 / 512 = 8 batches each went through a table of their own -- or none did
            assert ctx.search_party_table_stats() == ((3, 24) if on else (0, 0))
            got[on].append(selfplay_game(ctx, teams, battle_seed=31, iterations=256, batch=128, bandit="pucb", c=1.5, evaluator=net, seed=7))
        assert ctx.set_search_party_table(False) is True              # returns the previous value
        fills, evals = ctx.search_party_table_stats()
        assert fills >= 3 + 3 and evals >= 24 + 3 * 2                 # the game's searches too: one fill each, 256 / 128 batches
        old = os.environ.get("OAKGPU_PARTY_TABLE")
        os.environ["OAKGPU_PARTY_TABLE"] = "1"                        # the default of contexts created while it is set
        try:
            born_on = Context(0)
            assert born_on.set_search_party_table(False) is True
            born_on.close()
        finally:
            os.environ.pop("OAKGPU_PARTY_TABLE") if old is None else os.environ.__setitem__("OAKGPU_PARTY_TABLE", old)
    finally:
        ctx.set_search_party_table(False)
    for k in range(3):
        _same_output(got[False][k], got[True][k])
        assert got[True][k]["iterations"] == 4096
    rec_off, frames_off, result_off = got[False][3]
    rec_on, frames_on, result_on = got[True][3]
    assert 3 <= frames_off <= 30, frames_off
    assert rec_off == rec_on and (frames_off, result_off) == (frames_on, result_on)
    net.close(); qnet.close()
    ctx.close()


def test_refusals(gpu_ctx):
    """Every refusal of the table's entry points, each with its message."""
    from hipmem import Dev
    from oak_amd import _lib
    from oak_amd._lib import OakGpuError
    from oak_amd.engine import Network, PartyTable
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    net, other = Network(gpu_ctx, path=NET_DEFAULT), Network(gpu_ctx, path=NET256)
    rb, rd, rp, rr = O.make_random_ou_batch(3, seed0=0x4EF)
    n = 3
    gb, gd, gv = Dev(rb), Dev(rd), Dev(np.zeros(n, np.float32))
    gc, gl = Dev(np.zeros((n, 9), np.uint8)), Dev(np.zeros((n, 9), np.float32))

    def refused(rc, text):
        assert rc != 0 and text in lib.oakgpu_last_error().decode(), (rc, lib.oakgpu_last_error())

    out = C.c_void_p()
    refused(lib.oakgpu_party_table_create(h, net.handle, 1, None), "null pointer")
    refused(lib.oakgpu_party_table_create(None, net.handle, 1, C.byref(out)), "null pointer")
    refused(lib.oakgpu_party_table_create(h, None, 1, C.byref(out)), "null pointer")
    refused(lib.oakgpu_party_table_create(h, net.handle, 0, C.byref(out)), "max_roots")
    table = PartyTable(gpu_ctx, net, max_roots=2)
    t = table.handle
    # a lookup before any fill
    refused(lib.oakgpu_leaf_eval_table_dev(h, net.handle, t, None, gb.p, gd.p, n, gv.p, None), "has not been filled")
    refused(lib.oakgpu_leaf_eval_policy_table_dev(h, net.handle, t, None, gb.p, gd.p, n, gc.p, gc.p, gc.p, gc.p, gv.p, gl.p, gl.p), "has not been filled")
    refused(lib.oakgpu_party_table_rows(h, t, 0, 0, 0, gv.p), "beyond the filled roots")
    refused(lib.oakgpu_party_table_last_misses(h, t, C.byref(C.c_uint32())), "not an eval through this table")
    # n_roots
    refused(lib.oakgpu_party_table_fill(h, t, rb.ctypes.data_as(C.c_void_p), 3), "max_roots")
    refused(lib.oakgpu_party_table_fill_dev(h, t, gb.p, 3), "max_roots")
    refused(lib.oakgpu_party_table_fill(h, t, rb.ctypes.data_as(C.c_void_p), 0), "max_roots")
    # null pointers
    refused(lib.oakgpu_party_table_fill(h, t, None, 1), "null pointer")
    refused(lib.oakgpu_party_table_fill_dev(h, None, gb.p, 1), "null pointer")
    refused(lib.oakgpu_party_table_last_misses(h, t, None), "null pointer")
    refused(lib.oakgpu_party_table_rows(h, t, 0, 0, 0, None), "null pointer")
    _lib.check(lib.oakgpu_party_table_fill_dev(h, t, gb.p, 2))
    gpu_ctx.synchronize()
    refused(lib.oakgpu_leaf_eval_table_dev(h, net.handle, None, None, gb.p, gd.p, n, gv.p, None), "null ctx/net/table")
    refused(lib.oakgpu_leaf_eval_table_dev(h, net.handle, t, None, None, gd.p, n, gv.p, None), "null required pointer")
    refused(lib.oakgpu_leaf_eval_policy_table_dev(h, net.handle, t, None, gb.p, gd.p, n, None, gc.p, gc.p, gc.p, gv.p, gl.p, gl.p), "null pointer")
    # a table made for another network
    refused(lib.oakgpu_leaf_eval_table_dev(h, other.handle, t, None, gb.p, gd.p, n, gv.p, None), "another network")
    refused(lib.oakgpu_leaf_eval_policy_table_dev(h, other.handle, t, None, gb.p, gd.p, n, gc.p, gc.p, gc.p, gc.p, gv.p, gl.p, gl.p), "another network")
    # ... or device (where there is a second one)
    if lib.oakgpu_device_count() > 1:
        from oak_amd.engine import Context
        far = Context(1)
        refused(lib.oakgpu_leaf_eval_table_dev(far.handle, net.handle, t, None, gb.p, gd.p, n, gv.p, None), "another device")
        refused(lib.oakgpu_party_table_fill_dev(far.handle, t, gb.p, 1), "another device")
        far.close()
    # rows out of range; the filled table works
    refused(lib.oakgpu_party_table_rows(h, t, 2, 0, 0, gl.p), "beyond the filled roots")
    refused(lib.oakgpu_party_table_rows(h, t, 0, 2, 0, gl.p), "out of range")
    _lib.check(lib.oakgpu_leaf_eval_table_dev(h, net.handle, t, None, gb.p, gd.p, n, gv.p, None))
    assert table.last_misses() == R.expected_misses(rb[:2], None, rb)
    # the counters are the context's last work-list call's: after a cached call they are no longer this table's
    ge, gt = Dev(np.zeros((n, net.shape()[0]), np.float32)), Dev(np.zeros((n, 10, 6), np.uint32), fill=0xFF)
    _lib.check(lib.oakgpu_leaf_eval_cached_dev(h, net.handle, gb.p, gd.p, n, gv.p, ge.p, gt.p))
    refused(lib.oakgpu_party_table_last_misses(h, t, C.byref(C.c_uint32())), "not an eval through this table")
    ge.free(); gt.free()
    with pytest.raises(OakGpuError):
        PartyTable(gpu_ctx, net, max_roots=0)
    for x in (gb, gd, gv, gc, gl):
        x.free()
    table.close()
    net.close(); other.close()
