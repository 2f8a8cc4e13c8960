// oak_amd/csrc/selfplay.hip -- `.battle.data` training frames and the self-play game loop over the GPU hot path (host code).
//
// the sink of the search results.  Two pieces of the reference are mirrored here:
//   * Train::Battle::CompressedFrames (cpp/include/train/battle/compressed-frame.h:37-223): the on-disk record of one
//     game -- u32 byte length, u16 frame count, the 384-byte battle after the opening update, the final result byte, then
//     per turn an Update {mn byte = (m-1) | (n-1) << 4, both chosen pkmn_choices, u32 iterations, u16 empirical value,
//     u16 nash value, m u16 empirical + m u16 nash probabilities of P1, n + n of P2}; probabilities and values are stored
//     as `x * 65535` truncated to u16 (compress_probs, :11-25).  oakgpu_frames_write / _read are its write() / read().
//   * the per-game loop of the data generator (cpp/src/generate.cc:238-322): PKMN::battle + opening update, then per turn
//     RuntimeSearch::run -> RuntimePolicy::process_and_sample for both sides (cpp/include/util/policy.h:22-106) ->
//     frame -> PKMN::update, until the result is terminal.  oakgpu_selfplay_game runs it with every battle operation on
//     the GPU: oakgpu_init_battles, oakgpu_search (batched leaves), oakgpu_update.
// The replay self-check of the reference (cpp/include/py/battle/frames.h:52-67: replaying the stored choices from the
// stored battle must reproduce the stored result) is tests/test_gpu_frames.py.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "../../include/oakgpu.h"
#include "oakgpu_internal.h"
#include "selfplay_pick.hpp"
#include "record_scan.hpp"

namespace {

using oak_pick::compress_prob;
using oak_pick::update_bytes;
using oak_pick::splitmix64;
using oak_pick::sample_pdf;

template <class T> void put(uint8_t *&p, T v) { memcpy(p, &v, sizeof v); p += sizeof v; }
template <class T> T get(const uint8_t *&p) { T v; memcpy(&v, p, sizeof v); p += sizeof v; return v; }

// RuntimePolicy::get_policy (util/policy.h:22-98) for the modes the search output can feed: words of the mode string are
// 'e' (empirical), 'n' (nash), 'x' (argmax of empirical), each optionally followed by a weight ("e0.9-x0.1"); then
// temperature, the minimum-probability cut and renormalisation.  'p' (prior, the contextual bandits' softmaxed logits) adds
// w * prior AND THEN w * empirical: the reference's `case Mode::prior` has no `break` and falls into the empirical case
// (policy.h:37-46), and a drop-in follows what the code does.  'b' (beta) throws in the reference (policy.h:59-60) and is
// refused here, like an unknown mode character.
// The string is parsed into words here; the arithmetic is selfplay_pick.hpp's, shared with the device game loop.
bool get_policy(const double *prior, const double *empirical, const double *nash, int k, const char *mode, double temp, double minp, double *policy) {
  oak_pick::PolicyMode words;
  if (oak_pick::parse_policy_mode(mode, 64, &words)) { for (int i = 0; i < 9; ++i) policy[i] = 0; return false; }
  return oak_pick::get_policy(prior, empirical, nash, k, words, temp, minp, policy);
}

// endless_battle_check (generate.cc:127-152): with ebc=false a battle of Ghosts that cannot hurt each other never ends before turn 1,000.
// Moves that cannot hit a Ghost: type Normal or Fighting, or base power 0 (the reference's own test) -- one bit per move id, from
// oak_amd/data/gen1_data.json (tests/test_frames.py recomputes the mask from that file).
const uint64_t CANT_HIT_GHOST[3] = {0x8047f8ffffb5fc7full, 0x03ffffdf9442e67cull, 0x0000003fd6dd5bfeull};
bool set_is_ghost(const uint8_t *set) { return set[0] == 92 || set[0] == 93 || set[0] == 94; } // Gastly, Haunter, Gengar
bool set_cant_hit_ghosts(const uint8_t *set) {
  for (int k = 1; k <= 4; ++k) { const uint32_t m = set[k]; if (m > 165 || !((CANT_HIT_GHOST[m >> 6] >> (m & 63)) & 1)) return false; }
  return true;
}

} // namespace

// The checks of CompressedFrames::read on one record at the head of `buffer` (shared by oakgpu_frames_read and oakgpu_replay_index, with
// oakgpu_frames_read's messages).  OAKGPU_RECORD_STOP: the length field cannot be trusted -- a header cut short, or a length below
// the fixed part or past the buffer's end -- so nothing behind this point can be found.  OAKGPU_RECORD_MALFORMED: the record is
// damaged inside its own length (an m or n nibble above 8, an update past the record's end, a frame count that disagrees with the
// header); *total is still where the next record starts.
// The rule itself is record_scan.hpp's, the text the replay window's device pass compiles too.
int oakgpu_record_scan_length(const uint8_t *buffer, size_t size, uint32_t *total, uint16_t *n_frames, const char **msg) {
  oak_scan::HostBytes rd{buffer};
  int why = 0;
  const int kind = oak_scan::scan_length(rd, size, total, n_frames, &why);
  if (kind) *msg = oak_scan::why_message(why);
  return kind;
}
int oakgpu_record_scan(const uint8_t *buffer, size_t size, uint32_t *total, uint16_t *n_frames, const char **msg) {
  oak_scan::HostBytes rd{buffer};
  int why = 0;
  const int kind = oak_scan::scan(rd, size, total, n_frames, &why);
  if (kind) *msg = oak_scan::why_message(why);
  return kind;
}
static_assert(OAKGPU_RECORD_OK == oak_scan::RECORD_OK && OAKGPU_RECORD_MALFORMED == oak_scan::RECORD_MALFORMED && OAKGPU_RECORD_STOP == oak_scan::RECORD_STOP,
              "one set of values");

extern "C" {

// 1 when EVERY pairing of the two teams is Ghost against Ghost with no move on either side that can hit a Ghost -- the match-ups the
// reference's generator rejects up front (generate.cc:127-152, 222-225): teams = 2 x 6 x {species, 4 moves}.
int oakgpu_endless_battle_check(const uint8_t *teams) {
  if (!teams) return 0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      const uint8_t *a = teams + 5 * i, *b = teams + 30 + 5 * j;
      if (!(set_is_ghost(a) && set_cant_hit_ghosts(b) && set_is_ghost(b) && set_cant_hit_ghosts(a))) return 0;
    }
  return 1;
}

size_t oakgpu_frames_size(const oakgpu_frame_update *updates, uint32_t count) { // CompressedFrames::n_bytes (:180-187)
  size_t n = 4 + 2 + 384 + 1;
  for (uint32_t i = 0; i < count; ++i) n += update_bytes(updates[i].m, updates[i].n);
  return n;
}

int oakgpu_frames_write(const uint8_t *battle, uint8_t result, const oakgpu_frame_update *updates, uint32_t count, uint8_t *buffer,
                        size_t capacity, size_t *written) {
  if (!battle || (!updates && count) || !buffer) return oakgpu_fail_msg("oakgpu_frames_write: null argument");
  if (count > 0xFFFF) return oakgpu_fail_msg("oakgpu_frames_write: more than 65535 frames in one game (FrameCount is u16)");
  for (uint32_t i = 0; i < count; ++i)
    if (updates[i].m < 1 || updates[i].m > 9 || updates[i].n < 1 || updates[i].n > 9) return oakgpu_fail_msg("oakgpu_frames_write: m, n must be in 1..9");
  const size_t total = oakgpu_frames_size(updates, count);
  if (total > capacity) return oakgpu_fail_msg("oakgpu_frames_write: buffer too small");
  uint8_t *p = buffer;
  put<uint32_t>(p, (uint32_t)total);          // Offset: byte length of this game's record (:190-191)
  put<uint16_t>(p, (uint16_t)count);          // FrameCount
  memcpy(p, battle, 384); p += 384;
  *p++ = result;
  for (uint32_t i = 0; i < count; ++i) {      // Update::write (:89-113)
    const oakgpu_frame_update &u = updates[i];
    *p++ = (uint8_t)((u.m - 1) | ((u.n - 1) << 4));
    *p++ = u.c1;
    *p++ = u.c2;
    put<uint32_t>(p, u.iterations);
    put<uint16_t>(p, compress_prob(u.empirical_value));
    put<uint16_t>(p, compress_prob(u.nash_value));
    for (int k = 0; k < u.m; ++k) put<uint16_t>(p, compress_prob(u.p1_empirical[k]));
    for (int k = 0; k < u.m; ++k) put<uint16_t>(p, compress_prob(u.p1_nash[k]));
    for (int k = 0; k < u.n; ++k) put<uint16_t>(p, compress_prob(u.p2_empirical[k]));
    for (int k = 0; k < u.n; ++k) put<uint16_t>(p, compress_prob(u.p2_nash[k]));
  }
  if (written) *written = total;
  return 0;
}

int oakgpu_frames_read(const uint8_t *buffer, size_t size, uint8_t *battle, uint8_t *result, oakgpu_frame_update *updates,
                       uint32_t capacity, uint32_t *count, size_t *consumed) {
  if (!buffer || !count) return oakgpu_fail_msg("oakgpu_frames_read: null argument");
  uint32_t total = 0;
  uint16_t frames = 0;
  const char *msg = nullptr;
  const int kind = oakgpu_record_scan(buffer, size, &total, &frames, &msg);
  if (kind == OAKGPU_RECORD_STOP) return oakgpu_fail_msg(msg);
  const uint8_t *p = buffer + 6;
  if (battle) memcpy(battle, p, 384);
  p += 384;
  if (result) *result = *p;
  ++p;
  if (kind == OAKGPU_RECORD_MALFORMED) return oakgpu_fail_msg(msg);
  uint32_t n_read = 0;
  while ((size_t)(p - buffer) < total) {      // CompressedFrames::read (:224-243); oakgpu_record_scan has checked every bound
    const uint8_t mn = *p;
    const uint32_t m = (mn & 15) + 1, n = (mn >> 4) + 1;
    ++p;
    oakgpu_frame_update u{};
    u.m = (uint8_t)m; u.n = (uint8_t)n;
    u.c1 = *p++; u.c2 = *p++;
    u.iterations = get<uint32_t>(p);
    u.empirical_value = get<uint16_t>(p) / 65535.0; // uncompress_probs (:27-35)
    u.nash_value = get<uint16_t>(p) / 65535.0;
    for (uint32_t k = 0; k < m; ++k) u.p1_empirical[k] = get<uint16_t>(p) / 65535.0;
    for (uint32_t k = 0; k < m; ++k) u.p1_nash[k] = get<uint16_t>(p) / 65535.0;
    for (uint32_t k = 0; k < n; ++k) u.p2_empirical[k] = get<uint16_t>(p) / 65535.0;
    for (uint32_t k = 0; k < n; ++k) u.p2_nash[k] = get<uint16_t>(p) / 65535.0;
    if (updates && n_read < capacity) updates[n_read] = u;
    ++n_read;
  }
  if (updates && n_read > capacity) return oakgpu_fail_msg("oakgpu_frames_read: more frames than the caller's capacity");
  *count = n_read;
  if (consumed) *consumed = total;
  return 0;
}

// Record boundaries + the per-frame validation of oakgpu_frames_read, for the replay check (oakgpu_replay_records).  Boundaries are
// found in one sequential walk over the length fields (a record's length is where the next one starts); the records' own frames are
// then checked on up to 16 host threads.
int oakgpu_replay_index(const uint8_t *buffer, size_t size, uint64_t *offsets, uint16_t *frames, uint8_t *malformed, uint32_t capacity,
                        uint32_t *n_records, size_t *stopped_at) {
  if ((!buffer && size) || !n_records) return oakgpu_fail_msg("oakgpu_replay_index: null argument");
  std::vector<uint64_t> offs;
  size_t pos = 0;
  while (pos < size) {
    uint32_t total = 0;
    uint16_t nf = 0;
    const char *msg = nullptr;
    if (oakgpu_record_scan_length(buffer + pos, size - pos, &total, &nf, &msg) != OAKGPU_RECORD_OK) break;
    if (offs.size() == 0xFFFFFFFFu) break;
    offs.push_back(pos);
    pos += total;
  }
  *n_records = (uint32_t)offs.size();
  if (stopped_at) *stopped_at = pos;
  if (!offsets && !frames && !malformed) return 0; // counting call
  if (!offsets || !frames || !malformed) return oakgpu_fail_msg("oakgpu_replay_index: offsets, frames and malformed go together");
  if (offs.size() > capacity) return oakgpu_fail_msg("oakgpu_replay_index: more records than the caller's capacity");
  const size_t n = offs.size();
  auto scan = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      uint32_t total = 0;
      uint16_t nf = 0;
      const char *msg = nullptr;
      const int kind = oakgpu_record_scan(buffer + offs[i], size - offs[i], &total, &nf, &msg);
      offsets[i] = offs[i];
      frames[i] = nf;
      malformed[i] = kind == OAKGPU_RECORD_MALFORMED ? 1 : 0;
    }
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t threads = std::min<size_t>({(size_t)16, hw ? (size_t)hw : 1, n / 4096 + 1}); // (a GPU job's 16 CPUs at most)
  if (threads <= 1) { scan(0, n); return 0; }
  std::vector<std::thread> pool;
  const size_t per = (n + threads - 1) / threads;
  for (size_t t = 0; t < threads; ++t) pool.emplace_back(scan, std::min(n, t * per), std::min(n, (t + 1) * per));
  for (auto &th : pool) th.join();
  return 0;
}

int oakgpu_selfplay_game(oakgpu_ctx *ctx, oakgpu_net *net, const uint8_t *teams, uint64_t battle_seed, oakgpu_selfplay_params *prm,
                         uint8_t *buffer, size_t capacity, size_t *written, uint32_t *n_frames, uint8_t *result_out) {
  if (!ctx || !teams || !prm || !buffer) return oakgpu_fail_msg("oakgpu_selfplay_game: null argument");
  // generate.cc:222-225: such a pair is not played (the reference prints "EBC check failed. Continuing." and draws other teams; the teams
  // are the caller's here, so the caller is told)
  if (oakgpu_endless_battle_check(teams)) return oakgpu_fail_msg("oakgpu_selfplay_game: EBC check failed (every match-up is Ghost against Ghost with no move that can hit a Ghost, generate.cc:127-152)");
  // PKMN::battle(p1, p2, seed) + the opening update(0, 0) (generate.cc:238-240), on the device
  uint8_t battle[384], durations[8] = {}, result = 0;
  if (int rc = oakgpu_init_battles(ctx, teams, &battle_seed, 1, 1, battle, durations, &result)) return rc;
  uint8_t first[384];
  memcpy(first, battle, 384); // CompressedFrames{battle_data.battle} (generate.cc:244)
  std::vector<oakgpu_frame_update> frames;
  uint64_t rng = prm->seed ^ 0x9FB21C651E98DF25ull;
  // 0 = no limit, the reference's default (--max-battle-length -1, generate.cc:49-52): the engine itself ends a game at turn 1,000,
  // and only the handful of forced-switch updates come on top of that (2,048 is a backstop against a bug, never a rule of the game)
  const uint32_t max_len = prm->max_battle_length ? prm->max_battle_length : 2048;
  oakgpu_search_params sp = prm->search;
  struct HeapOwner { oakgpu_heap *h = nullptr; ~HeapOwner() { oakgpu_heap_destroy(h); } } heap;
  if (prm->keep_node && oakgpu_heap_create(&heap.h)) return -1;
  prm->nodes_kept = 0;
  // fast searches (selfplay_pick.hpp's turn_prelude): "" = the same mode, 0 = the same budget
  if (!(prm->fast_search_prob >= 0.0 && prm->fast_search_prob <= 1.0)) return oakgpu_fail_msg("oakgpu_selfplay_game: fast_search_prob must be in [0, 1]");
  {
    oak_pick::PolicyMode words;
    if (oak_pick::parse_policy_mode(prm->fast_policy_mode, sizeof prm->fast_policy_mode, &words))
      return oakgpu_fail_msg("oakgpu_selfplay_game: fast_policy_mode must be built from e / n / x / p words, 8 at the most (util/policy.h:22-98)");
  }
  char fast_mode[17] = {};
  memcpy(fast_mode, prm->fast_policy_mode[0] ? prm->fast_policy_mode : prm->policy_mode, 16);
  char full_mode[17] = {};
  memcpy(full_mode, prm->policy_mode, 16);
  while ((result & 15) == 0) {
    if (frames.size() >= max_len) return oakgpu_fail_msg("oakgpu_selfplay_game: max battle length exceeded (generate.cc:268-271)");
    oakgpu_search_output out;
    const oak_pick::TurnPrelude turn = oak_pick::turn_prelude(rng, prm->fast_search_prob);
    sp.seed = turn.search_seed;
    if (turn.fast) sp.iterations = oak_pick::turn_budget(true, (uint32_t)prm->search.iterations, prm->fast_budget);
    else sp.iterations = prm->search.iterations;
    const char *mode = turn.fast ? fast_mode : full_mode;
    int src = oakgpu_search_heap(ctx, net, heap.h, battle, durations, result, &sp, nullptr, &out);
    if (src == OAKGPU_E_ROOT_MISMATCH && heap.h) {
      // --keep-node: the kept child was expanded by a playout whose RESAMPLED hidden variables (mcts.h:254-259) gave it other
      // legal choices than the position the game really reached (a thrash / bide counter that ran out in one and not in the
      // other).  Its statistics are about another decision: start this position's tree afresh, like an update that found no child.
      oakgpu_heap_clear(heap.h);
      if (prm->nodes_kept) --prm->nodes_kept;
      src = oakgpu_search_heap(ctx, net, heap.h, battle, durations, result, &sp, nullptr, &out);
    }
    if (src) return src;
    double pol1[9], pol2[9];
    if (!get_policy(out.p1_prior, out.p1_empirical, out.p1_nash, out.m, mode, prm->policy_temp > 0 ? prm->policy_temp : 1.0, prm->policy_min, pol1) ||
        !get_policy(out.p2_prior, out.p2_empirical, out.p2_nash, out.n, mode, prm->policy_temp > 0 ? prm->policy_temp : 1.0, prm->policy_min, pol2))
      return oakgpu_fail_msg("oakgpu_selfplay_game: policy mode must be built from e / n / x words and leave a non-zero policy (util/policy.h:22-98)");
    const int i = sample_pdf(pol1, out.m, rng), j = sample_pdf(pol2, out.n, rng);
    oakgpu_frame_update u{};
    u.m = out.m; u.n = out.n;
    u.c1 = out.p1_choices[i]; u.c2 = out.p2_choices[j];
    u.iterations = (uint32_t)out.iterations;
    u.empirical_value = out.empirical_value;
    u.nash_value = out.nash_value;
    for (int k = 0; k < 9; ++k) { u.p1_empirical[k] = out.p1_empirical[k]; u.p1_nash[k] = out.p1_nash[k]; u.p2_empirical[k] = out.p2_empirical[k]; u.p2_nash[k] = out.p2_nash[k]; }
    frames.push_back(u);
    // PKMN::update(battle, c1, c2, options); durations <- options (generate.cc:319-322)
    uint8_t obs[16];
    if (int rc = oakgpu_update(ctx, battle, &u.c1, &u.c2, durations, obs, nullptr, 1, &result)) return rc;
    if (heap.h) prm->nodes_kept += (uint32_t)oakgpu_heap_update(heap.h, (uint8_t)i, (uint8_t)j, obs); // generate.cc:324-329
  }
  if (result_out) *result_out = result;
  if (n_frames) *n_frames = (uint32_t)frames.size();
  return oakgpu_frames_write(first, result, frames.data(), (uint32_t)frames.size(), buffer, capacity, written);
}

// n self-play games at once on one GPU -- the generator's worker pool (generate.cc:527-536: N threads, one game each, never waiting
// for each other): game g runs oakgpu_selfplay_game on ctxs[g] (a context of its own each) with teams[g], battle_seeds[g], params[g],
// its record into buffers + g * capacity_each.  One game at a time leaves the card idle for most of every search (the tree walk is host
// work); n games keep n trees in flight.  Every game is the game it would be alone.  threads_per_game: host threads of each game's tree
// walks (1, 2, 4, 8); 0 = the usable cores shared evenly (OAKGPU_SEARCH_CORES overrides the affinity mask's count).
int oakgpu_selfplay_games(oakgpu_ctx *const *ctxs, oakgpu_net *net, const uint8_t *teams, const uint64_t *battle_seeds, oakgpu_selfplay_params *params,
                          uint32_t n, int threads_per_game, uint8_t *buffers, size_t capacity_each, size_t *written, uint32_t *n_frames, uint8_t *results) {
  if (n == 0) return 0;
  if (!ctxs || !teams || !battle_seeds || !params || !buffers || !written) return oakgpu_fail_msg("oakgpu_selfplay_games: null argument");
  for (uint32_t g = 0; g < n; ++g) {
    if (!ctxs[g]) return oakgpu_fail_msg("oakgpu_selfplay_games: null context");
    for (uint32_t k = 0; k < g; ++k) if (ctxs[k] == ctxs[g]) return oakgpu_fail_msg("oakgpu_selfplay_games: every game needs a context of its own");
  }
  int W = threads_per_game;
  if (W <= 0) W = (int)(oakgpu_usable_cores() / n);
  W = W >= 16 ? 16 : W >= 8 ? 8 : W >= 4 ? 4 : W >= 2 ? 2 : 1;
  std::vector<int> rc(n, 0);
  std::vector<std::string> err(n);
  std::vector<std::thread> th;
  th.reserve(n);
  for (uint32_t g = 0; g < n; ++g)
    th.emplace_back([&, g] {
      oakgpu_set_thread_search_threads(W);
      rc[g] = oakgpu_selfplay_game(ctxs[g], net, teams + (size_t)g * 60, battle_seeds[g], params + g, buffers + (size_t)g * capacity_each, capacity_each,
                                   written + g, n_frames ? n_frames + g : nullptr, results ? results + g : nullptr);
      if (rc[g]) err[g] = oakgpu_last_error();
    });
  for (auto &t : th) t.join();
  for (uint32_t g = 0; g < n; ++g)
    if (rc[g]) return oakgpu_fail_msg(("oakgpu_selfplay_games: game " + std::to_string(g) + ": " + err[g]).c_str());
  return 0;
}

// Diagnostic (no GPU involved): selfplay_pick.hpp's turn prelude on one stream
int oakgpu_selfplay_prelude_host(uint64_t *rng, double fast_search_prob, int32_t *use_fast, uint64_t *search_seed) {
  if (!rng || !use_fast || !search_seed) return oakgpu_fail_msg("oakgpu_selfplay_prelude_host: null argument");
  const oak_pick::TurnPrelude t = oak_pick::turn_prelude(*rng, fast_search_prob);
  *use_fast = t.fast ? 1 : 0;
  *search_seed = t.search_seed;
  return 0;
}

// Diagnostic (no GPU involved): one turn's pick from a root output, by selfplay_pick.hpp's rule -- the text the device game loop compiles.
int oakgpu_selfplay_pick_host(uint32_t m, uint32_t n, const uint64_t *visit_matrix, const double *value_matrix, uint64_t iterations, const double *p1_nash,
                              const double *p2_nash, double nash_value, const double *p1_prior, const double *p2_prior, const uint8_t *p1_choices,
                              const uint8_t *p2_choices, const char *policy_mode, double policy_temp, double policy_min, uint64_t *rng,
                              double *empirical_value, double *p1_empirical, double *p2_empirical, double *p1_policy, double *p2_policy, int32_t *i_out,
                              int32_t *j_out, uint8_t *update, uint32_t *update_len) {
  if (!visit_matrix || !value_matrix || !rng || !empirical_value || !p1_empirical || !p2_empirical || !p1_policy || !p2_policy || !i_out || !j_out)
    return oakgpu_fail_msg("oakgpu_selfplay_pick_host: null argument");
  if (m < 1 || m > 9 || n < 1 || n > 9) return oakgpu_fail_msg("oakgpu_selfplay_pick_host: m, n must be in 1..9");
  oak_pick::PolicyMode words;
  if (oak_pick::parse_policy_mode(policy_mode, 63, &words))
    return oakgpu_fail_msg("oakgpu_selfplay_pick_host: policy mode must be built from e / n / x / p words, 8 at the most (util/policy.h:22-98)");
  const double zero[9] = {};
  const double *n1 = p1_nash ? p1_nash : zero, *n2 = p2_nash ? p2_nash : zero, *r1 = p1_prior ? p1_prior : zero, *r2 = p2_prior ? p2_prior : zero;
  oak_pick::process_output(visit_matrix, value_matrix, (int)m, (int)n, iterations, empirical_value, p1_empirical, p2_empirical, nullptr);
  const double temp = policy_temp > 0 ? policy_temp : 1.0;
  if (!oak_pick::get_policy(r1, p1_empirical, n1, (int)m, words, temp, policy_min, p1_policy) ||
      !oak_pick::get_policy(r2, p2_empirical, n2, (int)n, words, temp, policy_min, p2_policy))
    return oakgpu_fail_msg("oakgpu_selfplay_pick_host: RuntimePolicy: zero policy (the minimum-probability cut left nothing)");
  const int i = sample_pdf(p1_policy, (int)m, *rng), j = sample_pdf(p2_policy, (int)n, *rng);
  *i_out = i; *j_out = j;
  if (update) {
    const uint32_t len = oak_pick::encode_update(update, m, n, p1_choices ? p1_choices[i] : (uint8_t)i, p2_choices ? p2_choices[j] : (uint8_t)j, (uint32_t)iterations,
                                                 *empirical_value, nash_value, p1_empirical, n1, p2_empirical, n2);
    if (update_len) *update_len = len;
  }
  return 0;
}

} // extern "C"
