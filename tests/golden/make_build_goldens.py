"""Generator of tests/golden/build_goldens.npz: the reference's team-building index tables (Encode::Build::Tensorizer<Format::OU>,
cpp/include/encode/build/tensorizer.h), its legal lists (Encode::Build::Actions::get_singleton_additions / get_lead_swaps,
encode/build/actions.h) on the planted teams of tests/build_ref.py, and the 128 bytes of CompressedTrajectory<> NoTeam records
(encode/build/compressed-trajectory.h) of hand-written trajectories.  Run by hand where the reference tree exists:

    python tests/golden/make_build_goldens.py /path/to/reference

It writes a small harness of its own into a temporary directory (nothing of the reference is copied or kept), compiled with
g++ -std=c++2b -I<reference>/cpp/include -I include, and stores inputs and outputs -- data only -- in the .npz.
tests/test_build_ref.py holds tests/build_ref.py and the generated oak_amd/csrc/build_tables.inc to everything in it.

NOT here: NN::Build::Network::inference on a tiny `.build.net`.  The reference's network headers need Eigen, which the machine the
goldens were made on does not have; the forward is held to a float64 restatement of its three Affine layers instead.
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
OUT = os.path.join(HERE, "build_goldens.npz")

HARNESS = r'''
#include <encode/build/compressed-trajectory.h>
#include <cstdio>
#include <cstring>
#include <vector>
using Tz = Encode::Build::Tensorizer<>;
using Ac = Encode::Build::Actions<>;
using namespace Train::Build;
static std::vector<PKMN::Set> read_team(FILE *in) {
  uint8_t size, raw[30];
  if (fread(&size, 1, 1, in) != 1 || fread(raw, 1, 30, in) != 30) exit(2);
  std::vector<PKMN::Set> team(size);
  for (int i = 0; i < size; ++i) {
    team[i].species = static_cast<PKMN::Data::Species>(raw[5 * i]);
    for (int j = 0; j < 4; ++j) team[i].moves[j] = static_cast<PKMN::Data::Move>(raw[5 * i + 1 + j]);
  }
  return team;
}
static void put16(FILE *out, int v) { const uint16_t u = (uint16_t)v; fwrite(&u, 2, 1, out); }
int main(int argc, char **argv) {
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  const int32_t head[2] = {(int32_t)Tz::n_dim, (int32_t)Tz::max_actions};
  fwrite(head, 4, 2, out);
  for (int c = 0; c < (int)Tz::n_dim; ++c) {
    const auto pair = Tz::species_move_list(c);
    const uint8_t sm[2] = {static_cast<uint8_t>(pair.first), static_cast<uint8_t>(pair.second)};
    fwrite(sm, 1, 2, out);
  }
  uint32_t n_teams, n_traj;
  if (fread(&n_teams, 4, 1, in) != 1 || fread(&n_traj, 4, 1, in) != 1) return 2;
  for (uint32_t t = 0; t < n_teams; ++t) {
    const auto team = read_team(in);
    const auto add = Ac::get_singleton_additions(team);
    put16(out, (int)add.size());
    for (const auto &a : add) { put16(out, Tz::action_index(a)); put16(out, a[0].slot); put16(out, a[0].move_slot); }
    const auto swaps = Ac::get_lead_swaps(team);
    put16(out, (int)swaps.size());
    for (const auto &a : swaps) { put16(out, Tz::action_index(a)); put16(out, a[0].lead); }
  }
  for (uint32_t t = 0; t < n_traj; ++t) {
    Trajectory tr{};
    tr.initial = read_team(in);
    uint32_t k;
    float value, score;
    if (fread(&k, 4, 1, in) != 1 || fread(&value, 4, 1, in) != 1 || fread(&score, 4, 1, in) != 1) return 2;
    tr.value = value;
    if (score >= 0) tr.score = score;
    for (uint32_t u = 0; u < k; ++u) {
      uint16_t cell;
      float p;
      if (fread(&cell, 2, 1, in) != 1 || fread(&p, 4, 1, in) != 1) return 2;
      const auto pair = Tz::species_move_list(cell);
      tr.updates.push_back(Trajectory::Update{{Action{BasicAction{0, 0, 0, pair.first, pair.second}}}, 0, p});
    }
    Encode::Build::CompressedTrajectory<> ct{tr};
    char bytes[Encode::Build::CompressedTrajectory<>::size_no_team];
    static_assert(sizeof bytes == 128);
    ct.write(bytes);
    fwrite(bytes, 1, 128, out);
  }
  fclose(out);
  return 0;
}
'''


def trajectories():
    """Hand-written (team, size, cells, probs, value, score or -1)."""
    import build_ref as B
    planted = {name: (team, size) for name, team, size in B.planted_teams()}
    out = []
    for name, probs, value, score in (("one_missing_move", [0.25, 1.0], 0.5, 1.0), ("one_missing_pokemon", [1e-9, 0.5, 0.3, 7.6e-6, 1.6e-5, 0.999999], 0.5, 0.5),
                                      ("empty", list(np.linspace(1e-7, 1.0, 31)), 0.5, 0.0), ("complete", [0.2], 0.5, -1.0),
                                      ("size2", [0.5, 2.0 ** -17, 2.0 ** -16, 1.5 * 2.0 ** -16, 0.1], 0.0, 1.0), ("pool_of_one", [1.0, 0.3], 1.0, 0.5),
                                      ("deleted_3", [0.01 * (k + 1) for k in range(14)], 0.25, -1.0), ("size5", [1 / 3.0] * 7, 0.75, 0.0)):
        team, size = planted[name]
        r, cells = B.Rollout(team, size), []
        while r.legal() is not None:
            cells.append(r.advance((7 * len(cells) + 3) % len(r.legal())))
        assert len(cells) == len(probs), (name, len(cells))
        out.append((team, size, cells, probs, value, score))
    return out


def main(reference):
    import build_ref as B
    planted = B.planted_teams()
    trajs = trajectories()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, fin, fout = (os.path.join(tmp, x) for x in ("harness.cc", "harness", "in.bin", "out.bin"))
        open(src, "w").write(HARNESS)
        subprocess.check_call(["g++", "-std=c++2b", "-O1", "-I", os.path.join(reference, "cpp", "include"), "-I", os.path.join(ROOT, "include"),
                               src, "-o", exe])
        with open(fin, "wb") as f:
            f.write(np.array([len(planted), len(trajs)], np.uint32).tobytes())
            for _, team, size in planted:
                f.write(bytes([size]) + np.asarray(team, np.uint8).tobytes())
            for team, size, cells, probs, value, score in trajs:
                f.write(bytes([size]) + np.asarray(team, np.uint8).tobytes())
                f.write(np.array([len(cells)], np.uint32).tobytes() + np.array([value, score], np.float32).tobytes())
                for c, p in zip(cells, probs):
                    f.write(np.array([c], np.uint16).tobytes() + np.array([p], np.float32).tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    n_dim, max_actions = np.frombuffer(raw, np.int32, 2)
    pos = 8
    cells = np.frombuffer(raw, np.uint8, 2 * n_dim, pos).reshape(n_dim, 2).copy()
    pos += 2 * n_dim
    add, swaps = -np.ones((len(planted), int(max_actions), 3), np.int16), -np.ones((len(planted), 5, 2), np.int16)
    for t in range(len(planted)):
        k = int(np.frombuffer(raw, np.uint16, 1, pos)[0])
        add[t, :k] = np.frombuffer(raw, np.uint16, 3 * k, pos + 2).reshape(k, 3)
        pos += 2 + 6 * k
        k = int(np.frombuffer(raw, np.uint16, 1, pos)[0])
        swaps[t, :k] = np.frombuffer(raw, np.uint16, 2 * k, pos + 2).reshape(k, 2)
        pos += 2 + 4 * k
    records = np.frombuffer(raw, np.uint8, 128 * len(trajs), pos).reshape(len(trajs), 128).copy()
    assert pos + 128 * len(trajs) == len(raw)
    tc, tp = np.zeros((len(trajs), 31), np.uint16), np.zeros((len(trajs), 31), np.float32)
    for i, (_, _, c, p, _, _) in enumerate(trajs):
        tc[i, :len(c)], tp[i, :len(p)] = c, p
    np.savez_compressed(
        OUT, n_dim=np.int32(n_dim), max_actions=np.int32(max_actions), species_move_list=cells,
        team_names=np.array([p[0] for p in planted]), teams=np.stack([p[1] for p in planted]), sizes=np.array([p[2] for p in planted], np.uint8),
        additions=add, lead_swaps=swaps,
        traj_teams=np.stack([t[0] for t in trajs]), traj_sizes=np.array([t[1] for t in trajs], np.uint8), traj_n=np.array([len(t[2]) for t in trajs], np.uint8),
        traj_cells=tc, traj_probs=tp, traj_value=np.array([t[4] for t in trajs], np.float32), traj_score=np.array([t[5] for t in trajs], np.float32),
        records=records)
    print("wrote %s: %d cells, %d teams, %d records, %d bytes" % (OUT, n_dim, len(planted), len(trajs), os.path.getsize(OUT)))


if __name__ == "__main__":
    main(sys.argv[1])
