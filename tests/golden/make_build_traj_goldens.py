"""Generator of tests/golden/build_traj_goldens.npz: `.build.data` records in, the seven arrays of the reference's
Py::Build::Trajectories::write (cpp/include/py/build/trajectories.h) out.  Run by hand where the reference tree exists:

    python tests/golden/make_build_traj_goldens.py /path/to/reference

It writes a small pybind11 harness of its own into a temporary directory (nothing of the reference is copied or kept), compiled with
g++ -std=c++2b -I<reference>/cpp/include -I include, which copies each record into a CompressedTrajectory<> as read_build_trajectories does
(cpp/src/pyoak.cc:291-306) and calls write.  Data only goes into the .npz.

The reference's helper writes a seventh set out of bounds when the last read action -- the lead swap -- is applied to a team of six
(trajectories.h:65), so it can supply expected arrays only for trajectories whose team holds fewer than six sets when the swap is taken, or
that take no swap: only those are run.  The others are held by tests/test_build_traj_ref.py through invariants.

The records: build_ref.Rollout runs with seeded random picks over planted and sample teams at sizes 1 .. 5, chosen so that every final team
size 1 .. 5 occurs, a species with a pool below four moves, a first read step that is a species pick and one that is a move, a score byte
of 255, and probabilities of 1 and of 65,535."""
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "build_traj_goldens.npz")

HARNESS = r'''
#include <encode/build/compressed-trajectory.h>
#include <cstring>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
namespace py = pybind11;
#include <py/build/trajectories.h>
static py::dict run(py::bytes data) {
  const std::string raw = data;
  constexpr size_t size = Encode::Build::CompressedTrajectory<>::size_no_team;
  static_assert(size == 128);
  const size_t n = raw.size() / size;
  Py::Build::Trajectories t{n};
  t.clear();
  for (size_t i = 0; i < n; ++i) {
    Encode::Build::CompressedTrajectory<> traj;
    std::memcpy(reinterpret_cast<char *>(&traj), raw.data() + i * size, size);
    t.write(i, traj);
  }
  py::dict out;
  out["action"] = t.action; out["mask"] = t.mask; out["policy"] = t.policy; out["value"] = t.value; out["score"] = t.score;
  out["start"] = t.start; out["end"] = t.end;
  return out;
}
PYBIND11_MODULE(traj_harness, m) { m.def("run", &run); }
'''


def records():
    """[(name, record bytes)] with the coverage the docstring promises, checked here."""
    import build_ref as B
    import build_traj_ref as T
    rng = np.random.default_rng(28)
    planted = {name: (team, size) for name, team, size in B.planted_teams()}
    samples = B.sample_teams()
    out = []

    def add(name, team, size, **kw):
        rec = T.rollout_record(np.asarray(team, np.uint8).reshape(30), size, rng, **kw)
        assert rec is not None, name
        out.append((name, rec))

    def cut(team, size, drop_moves=()):
        t = np.array(team, np.uint8).reshape(6, 5).copy()
        t[size:] = 0
        for i, j in drop_moves:
            t[i, 1 + j] = 0
        return t.reshape(30)

    for size in range(1, 6):
        add("empty_size%d" % size, np.zeros(30, np.uint8), size, score=0.5)                       # the first read step is a species pick
        add("moves_missing_size%d" % size, cut(samples[size], size, [(0, 1), (size - 1, 3)]), size, score=1.0)   # ... is a move
        t = cut(samples[2 * size], size)
        t.reshape(6, 5)[size - 1] = 0
        add("last_pokemon_missing_size%d" % size, t, size, score=None if size % 2 else 0.0)      # score byte 255
    small = cut(planted["pool_under_four"][0], 5)
    small.reshape(6, 5)[1, 1:] = 0
    add("pool_under_four_size5", small, 5, score=0.0)
    one = cut(planted["pool_of_one"][0], 5)
    one.reshape(6, 5)[3, 1:] = 0
    add("pool_of_one_size5", one, 5, score=None)
    add("size2", *planted["size2"], score=1.0)
    add("size5", *planted["size5"], score=0.5, zero_prob=0.5)                                     # probabilities of 0 between the ends
    add("complete_size1", cut(samples[0], 1, [(0, 2)]), 1, value=1.0, score=None)
    recs = np.stack([np.frombuffer(r, np.uint8) for _, r in out])
    ref = T.decode_many(recs)
    assert (ref["status"] == T.OK).all()
    sizes, first_kinds, probs = set(), set(), set()
    for r in recs:
        _, _, _, action, prob = T.fields(r)
        start, end, swap, full = T.bounds(action, prob)
        sets = sum(1 for i in range(swap) if B.LIST[int(action[i])][1] == 0)
        assert swap == end or sets < 6, "the reference is not defined on this record"
        sizes.add(sets)
        first_kinds.add(int(B.LIST[int(action[start])][1]) == 0)
        probs |= set(int(p) for p in prob)
    assert sizes == {1, 2, 3, 4, 5} and first_kinds == {True, False} and {1, 65535} <= probs and (recs[:, 1] == 255).any()
    under_four = {int(B.TABLE[s, 0]) for s in B.LEGAL if len(B.POOLS[s]) < 4}
    assert any(under_four & set(int(a) for a in T.fields(r)[3]) for r in recs)
    return [name for name, _ in out], recs


def main(reference):
    import pybind11
    names, recs = records()
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "traj_harness.cc")
        lib = os.path.join(tmp, "traj_harness" + sysconfig.get_config_var("EXT_SUFFIX"))
        open(src, "w").write(HARNESS)
        subprocess.check_call(["g++", "-std=c++2b", "-O1", "-fPIC", "-shared", "-I", os.path.join(reference, "cpp", "include"), "-I", os.path.join(ROOT, "include"),
                               "-I", pybind11.get_include(), "-I", sysconfig.get_paths()["include"], src, "-o", lib])
        sys.path.insert(0, tmp)
        import traj_harness
        got = {k: np.array(v) for k, v in traj_harness.run(recs.tobytes()).items()}
    assert got["mask"].min() >= -1 and got["mask"].max() < 3749
    np.savez_compressed(OUT, names=np.array(names), records=recs, action=got["action"], mask=got["mask"].astype(np.int16), policy=got["policy"],
                        value=got["value"], score=got["score"], start=got["start"], end=got["end"])
    print("wrote %s: %d records, %d bytes" % (OUT, len(names), os.path.getsize(OUT)))


if __name__ == "__main__":
    main(sys.argv[1])
