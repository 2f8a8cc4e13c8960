"""Generator of tests/golden/train_goldens.npz: the reference's DENSE training encoders (cpp/include/encode/battle/battle.h:
Pokemon::write, Active::write with float *), uncompress_probs (train/battle/compressed-frame.h:27-33) and PKMN::score run on fixed
states.  Run by hand where the reference tree exists:

    python tests/golden/make_train_goldens.py /path/to/reference

It writes a small harness of its own into a temporary directory (nothing of the reference is copied or kept), compiled with
g++ -std=c++2b -I<reference>/cpp/include -I include, feeds it the states below and stores inputs and outputs -- data only -- in the
.npz.  tests/test_train_ref.py holds tests/train_ref.py to every float in it.  Per state and side the harness writes, as
EncodedFrames::write calls them (py/battle/encoded-frames.h:65-99):
  * Pokemon::write of the Pokemon at each order position with that position's sleep turns, into a cleared row (zeros for an empty
    position or hp 0);
  * Active::write into a cleared buffer of 229 + 165 cells (zeros when the active's stored hp is 0) -- and once more into the same
    buffer prefilled with a sentinel, which shows every cell the writer touches: the zero it stores for a disabled move lands behind
    the move block, at cell 209 + id.
The states: positions of oracle-played games, and planted ones -- a move held twice with the last slot at PP 0 (and with the first),
a disabled slot whose move id is below 20 and one at or above 20, a fainted active, equal types, every status.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "train_goldens.npz")
SENTINEL = -7.0
TAIL = 165

HARNESS = r'''
#include <encode/battle/battle.h>
#include <encode/battle/policy.h>
#include <train/battle/compressed-frame.h>
#include <libpkmn/pkmn.h>
#include <cstdio>
#include <cstring>
#include <vector>
// (the one libpkmn function PKMN::score calls: the low four bits of a result are its type)
extern "C" pkmn_result_kind pkmn_result_type(pkmn_result result) { return static_cast<pkmn_result_kind>(result & 15); }
int main(int argc, char **argv) {
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  uint32_t n, n_probs;
  if (fread(&n, 4, 1, in) != 1 || fread(&n_probs, 4, 1, in) != 1) return 2;
  constexpr int P = Encode::Battle::Pokemon::n_dim, A = Encode::Battle::Active::n_dim, T = 165;
  static_assert(P == 198 && A == 229);
  for (uint32_t i = 0; i < n; ++i) {
    pkmn_gen1_battle b;
    pkmn_gen1_chance_durations d;
    if (fread(b.bytes, 1, 384, in) != 384 || fread(d.bytes, 1, 8, in) != 8) return 2;
    const auto &battle = PKMN::view(b);
    const auto &durations = PKMN::view(d);
    for (int s = 0; s < 2; ++s) {
      const auto &side = battle.sides[s];
      const auto &duration = durations.get(s);
      for (int slot = 1; slot <= 6; ++slot) {
        float row[P] = {};
        const auto id = side.order[slot - 1];
        if (id != 0 && side.pokemon[id - 1].hp != 0) Encode::Battle::Pokemon::write(side.pokemon[id - 1], duration.sleep(slot - 1), row);
        fwrite(row, 4, P, out);
      }
      float clear[A + T] = {}, marked[A + T];
      for (auto &x : marked) x = SENTINEL;
      if (side.stored().hp != 0) Encode::Battle::Active::write(side.active, duration, clear);
      Encode::Battle::Active::write(side.active, duration, marked);
      fwrite(clear, 4, A + T, out);
      fwrite(marked, 4, A + T, out);
    }
  }
  std::vector<uint16_t> u(n_probs);
  if (fread(u.data(), 2, n_probs, in) != n_probs) return 2;
  for (const auto x : u) { const float f = Train::Battle::uncompress_probs<uint16_t, float>(x); fwrite(&f, 4, 1, out); }
  for (uint8_t r = 1; r <= 3; ++r) { const float f = PKMN::score(static_cast<pkmn_result>(r)); fwrite(&f, 4, 1, out); }
  const int32_t n_dim = Encode::Battle::Policy::n_dim;
  fwrite(&n_dim, 4, 1, out);
  fclose(out);
  return 0;
}
'''


def states():
    """(battles uint8[n, 384], durations uint8[n, 8], names)."""
    import embed_ref as E
    import oracle_lib as O
    import replay_oracle as R
    import train_ref as T
    b0, _, _, _ = O.make_random_ou_batch(4, seed0=0x5EED0000)
    bs, ds, names = [], [], []
    for g in range(4):
        first, result, frames, _, _ = R.play_random_game(b0[g], seed=g)
        walked, verdict = T.walk(R.make_record(first, result, frames))
        assert verdict is None
        for k in np.linspace(0, len(walked) - 1, 10).astype(int):
            bs.append(walked[k][0])
            ds.append(walked[k][1])
            names.append("game%d_frame%d" % (g, k))
    base = [i for i in range(len(bs)) if i % 10 in (3, 6)]        # mid-game states to plant on

    def plant(name, src, fn):
        b, d = bs[src].copy(), ds[src].copy()
        fn(b, d)
        bs.append(b)
        ds.append(d)
        names.append(name)

    def dup(where, pp_first, pp_last, mid=30):
        def fn(b, d):
            for s in range(2):
                o = (E._act(s) + 24) if where < 0 else E._stored_of(b, s, where) + 10
                b[o], b[o + 1], b[o + 6], b[o + 7] = mid, pp_first, mid, pp_last
        return fn
    for j, where in enumerate((-1, 0, 2)):
        plant("dup_last_pp0_at%d" % where, base[j], dup(where, 5, 0))
        plant("dup_first_pp0_at%d" % where, base[j], dup(where, 0, 5))
        plant("dup_both_pp_at%d" % where, base[j], dup(where, 3, 4))

    def disable(slot, mid, turns):
        def fn(b, d):
            for s in range(2):
                o = E._act(s) + 24 + 2 * (slot - 1)
                b[o], b[o + 1] = mid, 9
                E._set_vol(b, s, (7 << 56) | (15 << 52), (slot << 56) | (3 << 52))
                E._set_dur(d, s, 21, 4, turns)
        return fn
    plant("disable_id_below_20_duration_on_it", base[3], disable(2, 10, 6))     # the stray zero at 209 + 10 = 214 + 6 - 1: the duration writer puts its own 1 there
    plant("disable_id_below_20", base[4], disable(1, 12, 1))                    # 209 + 12 = 221: stays a zero inside the row's duration block
    plant("disable_id_19", base[5], disable(4, 19, 2))                          # 228: the row's last cell
    plant("disable_id_20", base[6], disable(3, 20, 3))                          # 229: the first cell behind the row
    plant("disable_id_164", base[7], disable(2, 164, 8))                        # 373

    def faint(b, d):
        E._put16(b, E._stored_of(b, 0, 0) + 18, 0)
        E._put16(b, E._stored_of(b, 1, 3) + 18, 0)
    plant("fainted_active_and_bench", base[0], faint)

    def same_types(b, d):
        for s in range(2):
            b[E._act(s) + 11] = 0x33 + 0x11 * s
            b[E._stored_of(b, s, 0) + 22] = 0x77
            b[E._stored_of(b, s, 1) + 22] = 0x00
    plant("equal_types", base[1], same_types)
    for j, (st, turns) in enumerate(E.STATUS_PLANTS):
        def status(b, d, st=st, turns=turns, j=j):
            for s in range(2):
                pos = (j + s) % 6
                b[E._stored_of(b, s, pos) + 20] = st
                E._set_dur(d, s, 3 * pos, 3, turns)
        plant("status_%02x_%d" % (st, turns), base[j % len(base)], status)
    return np.stack(bs), np.stack(ds), names


def main(reference):
    b, d, names = states()
    n = b.shape[0]
    probs = np.unique(np.concatenate([[0, 1, 2, 3, 32767, 32768, 65533, 65534, 65535], np.arange(0, 65536, 257),
                                      np.random.default_rng(3).integers(0, 65536, 192)])).astype(np.uint16)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, fin, fout = (os.path.join(tmp, x) for x in ("harness.cc", "harness", "in.bin", "out.bin"))
        open(src, "w").write(HARNESS.replace("SENTINEL", "%rf" % SENTINEL))
        subprocess.check_call(["g++", "-std=c++2b", "-O1", "-I", os.path.join(reference, "cpp", "include"), "-I", os.path.join(ROOT, "include"),
                               src, "-o", exe])
        with open(fin, "wb") as f:
            f.write(np.array([n, probs.size], np.uint32).tobytes())
            for i in range(n):
                f.write(b[i].tobytes() + d[i].tobytes())
            f.write(probs.tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = np.fromfile(fout, dtype=np.uint8)
    per_side = 6 * 198 + 2 * (229 + TAIL)
    body = raw[:n * 2 * per_side * 4].view(np.float32).reshape(n, 2, per_side)
    rest = raw[n * 2 * per_side * 4:]
    assert rest.size == 4 * probs.size + 12 + 4
    np.savez_compressed(
        OUT, battles=b, durations=d, names=np.array(names),
        pokemon=body[:, :, :6 * 198].reshape(n, 2, 6, 198).copy(),
        active_clear=body[:, :, 6 * 198:6 * 198 + 229 + TAIL].copy(), active_marked=body[:, :, 6 * 198 + 229 + TAIL:].copy(),
        sentinel=np.float32(SENTINEL), probs_u16=probs, probs_f32=rest[:4 * probs.size].view(np.float32).copy(),
        scores=rest[4 * probs.size:4 * probs.size + 12].view(np.float32).copy(), policy_dim=rest[-4:].view(np.int32).copy())
    print("wrote %s: %d states, %d bytes" % (OUT, n, os.path.getsize(OUT)))


if __name__ == "__main__":
    main(sys.argv[1])
