"""CPU: tests/train_ref.py -- the numpy restatement of a training row the GPU kernels are held to in tests/test_gpu_train_frames.py --
against tests/golden/train_goldens.npz, the reference's own dense encoders run on fixed states (tests/golden/make_train_goldens.py),
bit for bit; and the checks that the goldens can tell the dense rule from its neighbours."""
import os

import numpy as np

import train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "train_goldens.npz"))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_dense_rows_equal_the_reference_bit_for_bit():
    pokemon, active, hp = T.positions(G["battles"], G["durations"])
    assert G["battles"].shape[0] >= 64
    assert (_bits(pokemon) == _bits(G["pokemon"])).all()
    assert (_bits(active[:, :, 0]) == _bits(G["active_clear"][:, :, :229])).all()
    # a cleared buffer stays cleared behind the row
    assert (_bits(G["active_clear"][:, :, 229:]) == 0).all()
    # hp is 0 exactly where the reference wrote no row
    dead = ~G["pokemon"].any(axis=3)
    assert ((hp[..., 0] == 0) == dead).all() and dead.any() and (hp[..., 0][~dead] > 0).all()


def test_every_cell_the_active_writer_touches():
    """The sentinel-prefilled buffer: the cells the writer assigned inside the row are the restatement's, and the only cell it touches
    behind its move block that is not its own is the disabled move's zero at 209 + id -- 0 inside the row (where a cleared buffer
    holds 0 already, unless the duration writer put its 1 there afterwards) or behind it (not part of the row)."""
    _, active, _ = T.positions(G["battles"], G["durations"])
    marked, sentinel = G["active_marked"], G["sentinel"]
    touched = marked != sentinel
    names = list(G["names"])
    # (the marked run is not gated on hp: compare it where the active is alive)
    alive = G["active_clear"][:, :, :229].any(axis=2)
    inside = touched[:, :, :229] & alive[:, :, None]
    assert (_bits(marked[:, :, :229])[inside] == _bits(active[:, :, 0])[inside]).all()
    assert (active[:, :, 0][~touched[:, :, :229] & alive[:, :, None]] == 0).all()          # what it leaves alone is 0 in a cleared row
    assert (marked[:, :, 229:][touched[:, :, 229:]] == 0).all()                              # every changed cell behind the row holds 0
    behind = {names[i] for i in np.nonzero(touched[:, :, 229:].any(axis=(1, 2)))[0]}
    assert behind == {"disable_id_20", "disable_id_164"}, behind
    for name, cell in (("disable_id_20", 229), ("disable_id_164", 209 + 164)):
        i = names.index(name)
        assert list(np.nonzero(touched[i, 0, 229:])[0] + 229) == [cell]
    for name, cell, value in (("disable_id_below_20", 221, 0.0), ("disable_id_19", 228, 0.0), ("disable_id_below_20_duration_on_it", 219, 1.0)):
        i = names.index(name)
        assert touched[i, 0, cell] and marked[i, 0, cell] == value and active[i, 0, 0, cell] == value
    # the disabled move itself is NOT zeroed: its cell in the move block stays 1
    for name, mid in (("disable_id_below_20", 12), ("disable_id_20", 20), ("disable_id_164", 164)):
        assert active[names.index(name), 0, 0, 45 + mid - 1] == 1.0


def test_the_goldens_tell_the_last_slot_rule_from_the_sum_and_the_or_rule():
    b, d = G["battles"], G["durations"]
    dup = T.duplicated_move_sides(b).any(axis=(1, 2))
    assert dup.sum() >= 6
    ref = (G["pokemon"], G["active_clear"][:, :, None, :229])
    for rule in ("sum", "or"):
        pokemon, active, _ = T.positions(b, d, rule=rule)
        differs = (pokemon != ref[0]).any(axis=(1, 2, 3)) | (active != ref[1]).any(axis=(1, 2, 3))
        assert differs.any() and not differs[~dup].any(), rule
    names = list(G["names"])
    for where in (-1, 0, 2):                                                              # {30: pp 5, 30: pp 0} -> 0, {30: pp 0, 30: pp 5} -> 1
        for name, value in (("dup_last_pp0_at%d", 0.0), ("dup_first_pp0_at%d", 1.0), ("dup_both_pp_at%d", 1.0)):
            i = names.index(name % where)
            rows = [G["active_clear"][i, s, :229] if where < 0 else G["pokemon"][i, s, where] for s in range(2)]
            rows = [r for r in rows if r.any()]                                                  # (a fainted Pokemon has no row)
            assert rows and all(r[(45 if where < 0 else 5) + 30 - 1] == value for r in rows), name % where


def test_targets_equal_the_reference():
    assert (_bits(T.uncompress(G["probs_u16"])) == _bits(G["probs_f32"])).all()
    assert {0, 1, 65534, 65535} <= set(G["probs_u16"].tolist())
    assert list(G["scores"]) == [1.0, 0.0, 0.5] and int(G["policy_dim"][0]) == T.POLICY_DIM


def test_picks_of_a_played_game_and_the_draw_rule():
    """Corpus.expected / draws on a small corpus: statuses, the 315 fill, the filters of the draw rule."""
    import oracle_lib as O
    import replay_oracle as R
    b, _, _, _ = O.make_random_ou_batch(3, seed0=0x5EED0000)
    games = [R.play_random_game(b[i], seed=i) for i in range(3)]
    recs = [R.make_record(g[0], g[1], g[2]) for g in games]
    bad = bytearray(recs[1])
    bad[391 + 1] = 0xFF                                                                      # frame 0: c1 is no legal choice
    corpus = T.Corpus(recs + [bytes(bad), R.make_record(games[0][0], 0x50, games[0][2]), R.make_record(games[0][0], 1, [])])
    n0 = len(games[0][2])
    exp = corpus.expected([(0, 0), (0, n0 - 1), (0, n0), (9, 0), (3, 0), (3, 5), (4, 2), (5, 0)])
    assert list(exp["status"]) == [T.OK, T.OK, T.RANGE, T.RANGE, T.ILLEGAL, T.ILLEGAL, T.RESULT, T.RANGE]
    assert list(exp["where"]) == [0, n0 - 1, n0, 0, 0, 0, n0, 0]
    for name in T.FIELDS:
        if name not in ("status", "where"):
            assert not exp[name][2:].any(), name
    k = exp["k"][:2, :, 0]
    live = np.arange(9)[None, None, :] < k[:, :, None]
    assert (exp["choice_indices"][:2][~live] == T.POLICY_DIM).all() and (exp["choice_indices"][:2][live] < T.POLICY_DIM).all()
    assert (exp["score"][:2, 0] == {1: 1.0, 2: 0.0, 3: 0.5}[games[0][1] & 15]).all()
    picks = corpus.draws(64, seed=11, min_iterations=0, max_battle_length=max(len(g[2]) for g in games[1:]))
    longest = int(np.argmax([len(g[2]) for g in games]))
    assert ((picks[:, 0] < 4) | (picks[:, 0] == 4)).all() and 5 not in picks[:, 0]           # the empty record is never eligible
    if len(games[longest][2]) > max(len(g[2]) for g in games[1:]):
        assert longest not in picks[:, 0]
    assert (picks == corpus.draws(128, seed=11, min_iterations=0, max_battle_length=max(len(g[2]) for g in games[1:]))[:64]).all()
    assert (corpus.draws(8, seed=11, min_iterations=0, first=3) == corpus.draws(11, seed=11, min_iterations=0)[3:]).all()


def test_cpp_layer_of_the_loader_compiles_and_links(tmp_path):
    """OakGPU::FrameCorpus / EncodedFrames (include/oakgpu.hpp) compile as C++17 and link against liboakgpu.so."""
    import subprocess
    src = tmp_path / "train_frames.cc"
    src.write_text("""#include "oakgpu.hpp"
int main(int argc, char **) {
  if (argc < 100) return 0;  // (compiled and linked, not run: there is no GPU in this test)
  OakGPU::Context ctx;
  OakGPU::FrameCorpus corpus(ctx, std::vector<uint8_t>{});
  OakGPU::EncodedFrames frames(8);
  frames.picks[0] = 0;
  return static_cast<int>(corpus.encode(frames, 1) + corpus.sample(frames, 1, 0, 1) + corpus.info().records);
}
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", os.path.join(ROOT, "oak_amd"),
                           "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "train_frames")])
