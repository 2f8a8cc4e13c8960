"""numpy restatement of the bench-slot embedding table's contract (include/oakgpu.h, oakgpu_party_table_*), from the reference's text
alone: the 8-bit key (encode/battle/key.h:22-30, 65-71), the 240 variants a fill enumerates (nn/battle/cache.h:81-126), the stored
identity a lookup compares, and the misses a lookup must count.  A stored Pokemon is 24 bytes: stats 5 x u16 (0-9), four
{move id, pp} pairs (10-17), hp u16 (18-19), status (20), species (21), types (22), level (23)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nn_oracle as NN  # noqa: E402

N_KEYS = 240
PSN, BRN, FRZ, PAR, SLEEP1, REST = 0x08, 0x10, 0x20, 0x40, 0x01, 0x80
# cache.h:30-32 status_array, then Sleep1 with 1..7 public sleep turns (:121-124)
_NO_SLEEP = (0, PSN, BRN, FRZ, PAR, REST | 1, REST | 2, REST | 3)


def key(pokemon, sleep):
    """Encode::Battle::pokemon_key: bit i = move slot i has PP; bits 4-7 = status index + 1, 0 without a status."""
    pk = np.asarray(pokemon, dtype=np.uint8)
    k = sum(1 << i for i in range(4) if pk[11 + 2 * i])
    if pk[20]:
        k |= (NN.status_index(int(pk[20]), int(sleep)) + 1) << 4
    return k


def variants(base):
    """PokemonCache::fill's enumeration in ITS order: 16 has-PP patterns x (8 statuses at sleep 0, then Sleep1 at 1..7 turns) ->
    list of (24 bytes, sleep turns).  PP of move slot i = m & (1 << i)."""
    out = []
    for m in range(16):
        pk = np.array(base, dtype=np.uint8).copy()
        for i in range(4):
            pk[11 + 2 * i] = m & (1 << i)
        for st in _NO_SLEEP:
            v = pk.copy()
            v[20] = st
            out.append((v, 0))
        for sleep in range(1, 8):
            v = pk.copy()
            v[20] = SLEEP1
            out.append((v, sleep))
    return out


def variant_by_key(base):
    """key -> (24 bytes, sleep turns): the enumeration indexed by the key of each variant (all 240 distinct)."""
    table = {}
    for v, sleep in variants(base):
        k = key(v, sleep)
        assert k not in table and k < N_KEYS
        table[k] = (v, sleep)
    assert len(table) == N_KEYS
    return table


def identity(pokemon):
    """What no variant changes and every embedding depends on: the 24 bytes without PP (11, 13, 15, 17), hp (18-19) and status (20)."""
    pk = np.array(pokemon, dtype=np.uint8).copy()
    pk[[11, 13, 15, 17, 18, 19, 20]] = 0
    return pk


def bench_slots(battles):
    """battles [n, 384] -> (pid [n, 2, 5] team index + 1 of bench positions 1..5 (0: none), pk [n, 2, 5, 24], live [n, 2, 5])."""
    b = np.ascontiguousarray(battles, dtype=np.uint8)
    n = b.shape[0]
    sides = b[:, :368].reshape(n, 2, 184)
    pid = sides[:, :, 177:182].astype(np.int64)
    party = sides[:, :, :144].reshape(n, 2, 6, 24)
    pk = np.take_along_axis(party, np.maximum(pid - 1, 0)[..., None], axis=2)
    hp = pk[..., 18].astype(np.int64) | (pk[..., 19].astype(np.int64) << 8)
    return pid, pk, (pid != 0) & (hp != 0)


_IDENTITY = np.ones(24, dtype=bool)
_IDENTITY[[11, 13, 15, 17, 18, 19, 20]] = False


def expected_misses(roots, root_of, battles):
    """The bench slots a lookup must embed itself: live (order id != 0, hp != 0) and with an identity other than that of the root's
    Pokemon at the same (side, team index) -- an empty team slot of the root (species 0) matches nothing.  roots [R, 384]; root_of
    [n] (None: all 0); a root_of entry >= R makes every live slot of the leaf a miss."""
    roots = np.ascontiguousarray(roots, dtype=np.uint8).reshape(-1, 384)
    nr = roots.shape[0]
    pid, pk, live = bench_slots(battles)
    n = pid.shape[0]
    ro = np.zeros(n, np.int64) if root_of is None else np.asarray(root_of, dtype=np.int64)
    party = roots[:, :368].reshape(nr, 2, 184)[:, :, :144].reshape(nr, 2, 6, 24)
    base = party[np.minimum(ro, nr - 1)[:, None, None], np.arange(2)[None, :, None], np.maximum(pid - 1, 0)]      # [n, 2, 5, 24]
    same = (base[..., _IDENTITY] == pk[..., _IDENTITY]).all(axis=-1) & (base[..., 21] != 0) & (ro < nr)[:, None, None]
    return int((live & ~same).sum())
