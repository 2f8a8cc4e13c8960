"""CPU: the host restatement of the party-slot cache key (tests/oracle_lib.py party_slot_keys, from include/oakgpu.h's contract of
oakgpu_leaf_eval_cached_dev) against the numpy encoder: the key determines what Encode::Battle::Pokemon feeds the embedding net, so a
cache hit can never serve a stale embedding.  The GPU tests hold the kernel's recompute counts to this restatement."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nn_oracle as NN  # noqa: E402
import oracle_lib as O  # noqa: E402

# mutated slots each class re-embeds by the contract (per lane whose chosen slot is live; a move / order byte may already hold the
# value written, and a swap of two equal keys re-embeds nothing, so the classes of 1 and 2 are upper bounds met by most lanes)
CONTRACT = {"none": 0, "hp": 0, "hp_zero": 0, "hp_restore": 1, "pp_nonzero_to_nonzero": 0, "pp_to_zero": 1, "pp_from_zero": 1,
            "status_psn": 1, "status_brn": 1, "status_frz": 1, "status_par": 1, "par_to_sleep_turns_0": 0, "sleep_counter": 0,
            "sleep_turns_asleep": 1, "status_sleep": 1, "status_rest": 1, "sleep_turns_rest": 0, "sleep_turns_awake": 0,
            "species": 1, "level": 1, "types": 1, "swap_bench": 2, "swap_active": 1, "empty_slot": 0,
            "status_clear": 1}                   # (1 where the slot had a status: an upper bound only)
CONTRACT.update({"stat_" + s: 1 for s in ("hp_max", "atk", "def", "spe", "spc")})
CONTRACT.update({"move_%d" % m: 1 for m in range(1, 5)})


def _features(battles, durations, live):
    """{(lane, item): Encode::Battle::Pokemon's sparse input} for every live bench slot (nn_oracle.encode_pokemon)."""
    out = {}
    for i in range(battles.shape[0]):
        for s in range(2):
            dur = int.from_bytes(bytes(durations[i, 4 * s:4 * s + 4]), "little")
            for q in range(5):
                if live[i, 5 * s + q]:
                    pid = int(battles[i, 184 * s + 177 + q])
                    pk = battles[i, 184 * s + 24 * (pid - 1):184 * s + 24 * pid]
                    idx, val = NN.encode_pokemon(pk, (dur >> (3 * (q + 1))) & 7)
                    out[i, 5 * s + q] = (tuple(idx), tuple(float(v) for v in val))
    return out


def test_party_slot_key_determines_the_encoder_input():
    """Over random mid-game states and every mutation class of the cache tests (each applied to one bench slot of every lane): any two
    live slots with equal keys have equal encoder inputs, and wherever a mutation changes a slot's encoder input its key changes.
    Each class re-embeds what the contract says (hp, PP amounts, the hidden sleep counter, sleep turns outside a non-Rest sleep and
    PAR -> sleep at 0 turns are outside the key; stats, moves, has-PP, species, level, types and the status index are in it)."""
    b, d = O.midgame_batch(192, seed0=0x4B3E0000)
    side, pos = O.bench_slot_choice(b, seed=1)
    rng, memo = np.random.default_rng(2), {}
    keys, live = O.party_slot_keys(b, d)
    feats = _features(b, d, live)
    seen = {}

    def record(keys, live, feats):
        for (i, it), f in feats.items():
            k = keys[i, it].tobytes()
            assert seen.setdefault(k, f) == f, ("two slots with one key encode differently", i, it)
    record(keys, live, feats)
    assert O.expected_recomputes(None, keys, live) == int(live.sum()) > 1000
    changed_input = 0
    for name, fn in O.bench_slot_mutations():
        fn(b, d, side, pos, rng, memo)
        k2, l2 = O.party_slot_keys(b, d)
        f2 = _features(b, d, l2)
        record(k2, l2, f2)
        for (i, it), f in f2.items():
            if (i, it) in feats and feats[i, it] != f:
                changed_input += 1
                assert (keys[i, it] != k2[i, it]).any(), (name, i, it)
        got = O.expected_recomputes(keys, k2, l2)
        chosen = (np.arange(b.shape[0]), 5 * side + pos - 1)
        lanes = int((live[chosen] | l2[chosen]).sum())
        bound = CONTRACT[name] * lanes
        assert got <= bound and (got >= 0.6 * bound or name == "status_clear"), (name, got, bound)
        keys, live, feats = k2, l2, f2
    assert changed_input > 2000


def test_party_slot_keys_edges():
    """Empty order byte and stored hp 0 are dead; hp and PP amounts are outside the key; the status byte is index + 1 with the slot's
    own sleep turns (order position q + 1 of the side's durations word), so PAR and a sleep seen 0 turns share a key."""
    b, d = O.midgame_batch(8, seed0=77, steps=(0,))
    k0, l0 = O.party_slot_keys(b, d)
    assert l0.all() and (k0[..., 18:20] == 0).all() and set(np.unique(k0[..., 11:18:2])) <= {0, 1}
    pid = int(b[0, 177 + 2])                 # side 0, bench slot q = 2
    o = 24 * (pid - 1)
    b2, d2 = b.copy(), d.copy()
    b2[0, o + 18:o + 20] = (7, 0)            # hp 7
    b2[0, o + 11] = max(1, int(b2[0, o + 11]) // 2)
    assert (O.party_slot_keys(b2, d2)[0] == k0).all()
    b2[0, o + 20] = 0x40                     # PAR: index 3
    kp = O.party_slot_keys(b2, d2)[0][0, 2]
    assert kp[20] == 4
    w = d2[0, :4].view("<u4")                # side 0's durations word; slot q = 2's sleep turns are bits 9-11
    b2[0, o + 20] = 0x03                     # asleep, seen 0 turns: index 3 + 0
    w[0] &= ~np.uint32(7 << 9)
    assert (O.party_slot_keys(b2, d2)[0][0, 2] == kp).all()
    w[0] |= np.uint32(2 << 9)                # seen 2 turns: index 5
    assert O.party_slot_keys(b2, d2)[0][0, 2, 20] == 3 + 2 + 1
    b2[0, 177 + 2] = 0
    k3, l3 = O.party_slot_keys(b2, d2)
    assert not l3[0, 2] and (k3[0, 2] == 0xFF).all() and l3[0, [0, 1, 3, 4]].all()
    assert O.expected_recomputes(k0, k3, l3) == 0
