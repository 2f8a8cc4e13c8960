"""The bench-slot table's key and variant enumeration on the host (oakgpu_party_key / oakgpu_party_variant: the inline functions
the table's kernels use) against the reference's own pokemon_key recorded in tests/golden/oakside_goldens.json.gz and against the
numpy restatement tests/party_table_ref.py.  No GPU."""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import oracle_lib as O  # noqa: E402
import party_table_ref as R  # noqa: E402
from oak_amd import gamedata as G  # noqa: E402
from oak_amd.engine import party_key, party_variant  # noqa: E402

with gzip.open(os.path.join(HERE, "golden", "oakside_goldens.json.gz"), "rt") as f:
    STATES = json.load(f)["states"]


def _bytes(h):
    return np.frombuffer(bytes.fromhex(h), dtype=np.uint8).copy()


def _golden_slots():
    """(24 stored bytes, sleep turns, the reference's key) of every live bench slot of the golden states."""
    for st in STATES:
        b, d = _bytes(st["battle"]), _bytes(st["durations"])
        for s in range(2):
            side = b[184 * s:184 * (s + 1)]
            dur = int.from_bytes(bytes(d[4 * s:4 * s + 4]), "little")
            for pos in range(1, 6):
                ref = st["sides"][s]["slots"][pos - 1]
                if ref is None:
                    continue
                pid = int(side[176 + pos])
                yield side[24 * (pid - 1):24 * pid], (dur >> (3 * pos)) & 7, ref["key"]


def _sample_team_pokemon():
    """The stored Pokemon of the sample teams, as the engine initialises them (team k against team k + 1)."""
    sample = json.load(open(os.path.join(HERE, "golden", "ou_sample_teams.json")))["teams"]
    tb = [[[G.match_species(s[0])] + [G.match_move(m) for m in s[1:]] for s in t] for t in sample]
    for k in range(0, len(tb), 2):
        b = O.init_battle([tb[k], tb[k + 1]], 0x5EED + k)
        for s in range(2):
            for t in range(6):
                yield b[184 * s + 24 * t:184 * s + 24 * (t + 1)].copy()


def test_party_key_equals_the_reference_keys_and_the_restatement():
    n, seen = 0, set()
    for pk, sleep, ref in _golden_slots():
        got = party_key(pk, sleep)
        assert got == ref, (bytes(pk).hex(), sleep, got, ref)
        assert got == R.key(pk, sleep)
        seen.add(got)
        n += 1
    assert n > 1000 and len(seen) >= 30


def test_every_variant_round_trips_through_the_key_and_changes_pp_and_status_only():
    changeable = [11, 13, 15, 17, 20]
    fixed = [i for i in range(24) if i not in changeable]
    pokemon = list(_sample_team_pokemon())
    assert len(pokemon) == 96
    for base in pokemon:
        by_key = R.variant_by_key(base)
        for k in range(R.N_KEYS):
            v, sleep = party_variant(base, k)
            assert party_key(v, sleep) == k
            assert np.array_equal(v[fixed], base[fixed]), k
            rv, rsleep = by_key[k]                     # and it IS the variant the reference's fill stores under that key
            assert np.array_equal(v, rv) and sleep == rsleep, (k, bytes(v).hex(), bytes(rv).hex())
            assert np.array_equal(R.identity(v), R.identity(base))
    for k in (240, 255):
        try:
            party_variant(pokemon[0], k)
        except ValueError:
            continue
        raise AssertionError("key %d must be refused" % k)


def test_key_stays_below_240_on_every_status_the_mutations_write():
    """oracle_lib.bench_slot_mutations' statuses -- PAR -> sleep at 0 turns included (its key is PAR's) -- on a midgame batch."""
    n = 96
    b, d = O.midgame_batch(n, seed0=0x7AB1E)
    side, pos = O.bench_slot_choice(b, seed=5)
    rng, memo = np.random.default_rng(6), {}
    seen = set()
    for name, fn in O.bench_slot_mutations():
        fn(b, d, side, pos, rng, memo)
        pid, pk, live = R.bench_slots(b)
        dur = d.view("<u4").reshape(n, 2)
        for i in range(n):
            s, q = int(side[i]), int(pos[i]) - 1
            if not live[i, s, q]:
                continue
            sleep = (int(dur[i, s]) >> (3 * (q + 1))) & 7
            k = party_key(pk[i, s, q], sleep)
            assert k < R.N_KEYS and k == R.key(pk[i, s, q], sleep), (name, i, k)
            if name == "par_to_sleep_turns_0":
                assert k >> 4 == 4, (name, i, k)     # Sleep at 0 public turns encodes as index 3, PAR's (battle.h:103-123)
            seen.add(k >> 4)
    # every status field of the key except Rest3's (index 11 + 1), which the mutations never write: it exists mid-update only
    assert seen == set(range(15)) - {12}, sorted(seen)
