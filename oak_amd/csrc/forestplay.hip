// oak_amd/csrc/forestplay.hip -- self-play over the forest search: a batch of games resident on one device, `.battle.data` out (the
// contract is in include/oakgpu.h; the per-game form is selfplay.hip's oakgpu_selfplay_game, generate.cc:238-322).
//
//   k_fsp_start    : row g is game g at frame 0: its stream, its counters
//   k_fsp_retire   : one lane per row: a finished, dropped or stopped row scatters result, frame count, status and record length by game
//                    index; how many rows of each block are still live
//   k_rows_offsets : (game_rows.hpp) one workgroup: the exclusive prefix sums of those per-block counts, and their total = the live count the
//                    host reads
//   k_fsp_compact  : the live rows, in order, into the other half of the double buffer -- and the turn prelude: the row's stream advances,
//                    its first draw is the seed of the row's tree
//   k_fsp_payoffs  : (forest_rows.hpp's solve_turn, solve_nash) the integer payoffs of process_output's exact Nash solve, for the host threads
//                    that solve them (1) or for oakgpu_nash_solve_dev (2: nashdev.hip, on the stream, the same bits)
//   k_fsp_pick     : one lane per live row: selfplay_pick.hpp's rule over the m x n live cells of the root matrices, the joint choice for the
//                    update, one fixed-size entry of the turn-major log
//   k_fsp_lengths  : (forest_rows.hpp, as the two below) one workgroup: the exclusive scan of the record lengths in game order = the record bases
//   k_fsp_pack_head: one wave per game: length, frame count, first battle, result byte
//   k_fsp_pack_log : 16 lanes per log entry: the update's bytes to base[game] + 391 + cursor
// keep_node (a kept forest, oakgpu_forest_create_kept): the pick leaves the played cell (i, j) in the row and the update its observation; the
// next turn's compaction carries them to the row's new place and lists each new row's source row, and ONE oakgpu_forest_advance_dev with
// that list re-roots every tree and moves it along with its row; the search is then oakgpu_forest_search_kept_dev.  A retired row has no
// successor.  The pick also keeps the row's nodes_kept count (selfplay.hip: + 1 per advance that kept, - 1 per root mismatch, never below 0).
// Fast searches (params->fast_search_prob > 0; the rule is selfplay_pick.hpp's turn_prelude, one text with the host loop): the prelude first
// draws the turn's flag from the game's stream, and the compaction becomes a stable partition into two classes, the rows of the larger
// budget first -- k_fsp_retire counts both classes per block (it looks at the flag on a copy of the stream), the ONE scan runs over both
// count arrays, so the second class's offsets follow the first's, and k_fsp_compact places each class by its own offsets and writes the
// row's budget.  The search is then oakgpu_forest_search_budgets(_kept)_dev with budgets that do not increase in row order: no launch of it
// covers a finished tree.  With keep_node the trees follow through src_row as before.  The pick takes fast_policy_mode for a fast row.  Two
// departures from generate.cc:292-299: the draw is the game's own (there: the worker thread's), and none is made at probability 0.
// Matchup values and skipped battles (the _build calls; the rule is selfplay_pick.hpp's game_is_skipped): k_fsp_start draws each game's skip
// byte from a stream of its own; the pick scatters every row's first empirical value by game index (the matchup), and a skipped row's
// pick does that and nothing else -- it flags the row OAKGPU_FSP_SKIPPED, and the next retire pass retires it with no record.  On turn 1
// the compaction writes a skipped row's budget (t1_budget), and the search is a budgets search when some row's budget differs.
// Every kernel is a plain grid over rows, games or entries (the two scans: one workgroup); none waits for another block.  Between
// compact and pick runs oakgpu_forest_search_dev over exactly the live rows (the forest refuses terminal roots), after pick
// oakgpu_update_dev.  Retire / offsets / compact run on game_rows.hpp's scan, place and move, as in policyplay.hip, with this loop's own
// row; the Nash solve, the log, the record bases, the pack and the records' copies are forest_rows.hpp's, shared with forestmatch.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/oakgpu.h"
#include "oakgpu_internal.h"
#include "selfplay_pick.hpp"
#include "forest_rows.hpp"

namespace oak {
namespace fsp {

// one half of the double buffer: a row is its battle, durations, result byte, the joint choice between pick and the update, the stop flag
// (OAKGPU_FSP_ZERO_POLICY), its game index, the game's stream, its frame count and the byte cursor within its record's updates
struct Rows {
  uint8_t *battles, *durations, *results, *c1, *c2, *flag;
  uint32_t *game, *frames, *cursor;
  uint64_t *rng;
  // keep_node: the played cell, the update's observation, and the game's counts so far (advances that kept, root mismatches, nodes carried in)
  uint8_t *pi, *pj, *obs;
  uint32_t *kept, *mism, *carry;
  // fast searches: this turn's flag (written by the compaction's prelude) and the game's fast frames so far
  uint8_t *fast;
  uint32_t *fastn;
};

// fast searches (fast_search_prob > 0; selfplay_pick.hpp's turn_prelude), as the retire and compact kernels need them.  The live rows of
// the class with the larger budget go first (`fast_first`: that is the fast class), so the turn's budgets are non-increasing in row order;
// partition == 0 (benchmarks) leaves every live row in the first class, in game order
struct FastArgs {
  double prob;
  uint32_t on, fast_first, partition, blocks; // blocks: the second class's live counts and offsets start there
  uint32_t budget_full, budget_fast;
};
__device__ __forceinline__ bool first_class(const FastArgs &f, bool fast) { return !f.partition || fast == (f.fast_first != 0); }

// matchup: by game index, NaN until the game's first search; skip (by game index) <- the skip rule, with `built` null: no game is skipped
__global__ __launch_bounds__(BLOCK) void k_fsp_start(Rows r, const uint64_t *seeds, uint32_t n, int keep, double *matchup, const uint8_t *built, double skip_prob,
                                                     uint8_t *skip) {
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  if (row >= n) return;
  matchup[row] = __longlong_as_double(0x7FF8000000000000ll);
  skip[row] = built && oak_pick::game_is_skipped(seeds[row], skip_prob, built[row]) ? 1 : 0;
  if (keep) { r.kept[row] = 0; r.mism[row] = 0; r.carry[row] = 0; }
  r.game[row] = row;
  r.frames[row] = 0;
  r.cursor[row] = 0;
  r.flag[row] = 0;
  r.fast[row] = 0;
  r.fastn[row] = 0;
  r.rng[row] = seeds[row] ^ oak_pick::GAME_STREAM_XOR;
}

struct RetireArgs {
  Rows r;
  uint8_t *results_out, *status_out; // by game index
  uint32_t *frames_out, *length_out;
  uint32_t *block_live;              // per block of BLOCK rows: rows still live after this pass
  uint32_t rows, max_len;
  uint32_t *kept_out, *mism_out, *carry_out; // keep_node, by game index; else null
  uint32_t *fast_out;                        // by game index: the game's fast frames
  FastArgs fast;
};

__global__ __launch_bounds__(BLOCK) void k_fsp_retire(RetireArgs a) {
  __shared__ uint32_t wave_live[BLOCK / 64], wave_live2[BLOCK / 64];
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  const bool in = row < a.rows;
  const uint32_t g = in ? a.r.game[row] : DEAD;
  bool live = false;
  if (g != DEAD) {
    const uint32_t res = a.r.results[row], frames = a.r.frames[row];
    // the host loop's order: a policy that was zeroed ends the game where it stood; a terminal result ends it; only then is another frame due
    const uint32_t stopped = a.r.flag[row]; // the pick's: OAKGPU_FSP_ZERO_POLICY, or OAKGPU_FSP_SKIPPED (no frame, result byte 0)
    const uint32_t status = stopped ? stopped : (res & 15) != 0 ? (uint32_t)OAKGPU_FSP_OK : frames >= a.max_len ? (uint32_t)OAKGPU_FSP_MAX_LENGTH : DEAD;
    if (status == DEAD) live = true;
    else {
      a.results_out[g] = status == OAKGPU_FSP_SKIPPED ? (uint8_t)0 : (uint8_t)res;
      a.frames_out[g] = frames;
      a.status_out[g] = (uint8_t)status;
      a.length_out[g] = status == OAKGPU_FSP_OK ? HEAD_BYTES + a.r.cursor[row] : 0u;
      a.fast_out[g] = a.r.fastn[row];
      if (a.kept_out) { a.kept_out[g] = a.r.kept[row]; a.mism_out[g] = a.r.mism[row]; a.carry_out[g] = a.r.carry[row]; }
      a.r.game[row] = DEAD;
    }
  }
  if (!a.fast.on) { game_rows::count_block_live(live, wave_live, a.block_live); return; }
  // two classes: the flag the compaction's prelude will draw, looked at here on a copy of the stream
  bool first = false;
  if (live) {
    uint64_t rng = a.r.rng[row];
    first = first_class(a.fast, oak_pick::turn_is_fast(rng, a.fast.prob));
  }
  game_rows::count_block_live(first, wave_live, a.block_live);
  game_rows::count_block_live(live && !first, wave_live2, a.block_live + a.fast.blocks);
}

struct CompactArgs {
  Rows from, to;
  const uint32_t *block_offset;
  uint64_t *tree_seed; // per compacted row: the seed of this turn's tree
  uint32_t rows;
  // keep_node from the second turn on (else null): per compacted row, what oakgpu_forest_advance_dev takes -- the row (= tree) it came from,
  // the cell played there, the observation
  uint32_t *src_row;
  uint8_t *adv_i, *adv_j, *adv_obs;
  int keep; // keep_node: the game's counts move with the row
  FastArgs fast;
  uint32_t *budget; // fast searches: per compacted row, the iterations of this turn's search
  // skipped battles, turn 1 only (else null): the games' skip bytes; a skipped row's budget is t1_budget, every other row's its own
  const uint8_t *skip;
  uint32_t t1_budget;
};

// Stable (game_rows.hpp: compact_place, compact_battles).  The turn prelude rides along (selfplay_pick.hpp's turn_prelude): with fast
// searches the turn's flag, then search seed = splitmix64(rng).  With fast searches the compaction is a stable partition into two classes,
// each placed by its own offsets (the second class's follow the first's in the one scan).
__global__ __launch_bounds__(BLOCK) void k_fsp_compact(CompactArgs a) {
  __shared__ uint32_t wave_total[BLOCK / 64], wave_total2[BLOCK / 64];
  __shared__ uint32_t place[BLOCK], place2[BLOCK];
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = row < a.rows && a.from.game[row] != DEAD;
  uint64_t rng = 0;
  oak_pick::TurnPrelude turn{0, false};
  if (live) {
    rng = a.from.rng[row];
    turn = oak_pick::turn_prelude(rng, a.fast.on ? a.fast.prob : 0.0);
  }
  uint32_t to;
  if (!a.fast.on) to = game_rows::compact_place(live, a.block_offset[blockIdx.x], wave_total, place);
  else {
    const bool first = live && first_class(a.fast, turn.fast);
    to = game_rows::compact_place(first, a.block_offset[blockIdx.x], wave_total, place);
    const uint32_t to2 = game_rows::compact_place(live && !first, a.block_offset[a.fast.blocks + blockIdx.x], wave_total2, place2);
    if (live && !first) { to = to2; place[threadIdx.x] = to2; } // (the lane's own entry; read after the barrier below)
  }
  if (live) {
    *((uint2 *)a.to.durations + to) = *((const uint2 *)a.from.durations + row);
    a.to.results[to] = a.from.results[row];
    a.to.flag[to] = 0;
    a.to.game[to] = a.from.game[row];
    a.to.frames[to] = a.from.frames[row];
    a.to.cursor[to] = a.from.cursor[row];
    a.tree_seed[to] = turn.search_seed;
    a.to.rng[to] = rng;
    a.to.fast[to] = turn.fast ? 1 : 0;
    a.to.fastn[to] = a.from.fastn[row];
    if (a.skip && a.skip[a.from.game[row]]) a.budget[to] = a.t1_budget;
    else if (a.fast.on || a.skip) a.budget[to] = turn.fast ? a.fast.budget_fast : a.fast.budget_full;
    if (a.src_row) {
      a.src_row[to] = row;
      a.adv_i[to] = a.from.pi[row]; a.adv_j[to] = a.from.pj[row];
      *((u32x4 *)a.adv_obs + to) = *((const u32x4 *)a.from.obs + row);
    }
    if (a.keep) { a.to.kept[to] = a.from.kept[row]; a.to.mism[to] = a.from.mism[row]; a.to.carry[to] = a.from.carry[row]; }
  }
  __syncthreads();
  game_rows::compact_battles(a.from.battles, a.to.battles, a.rows, place);
}

struct PickArgs {
  Rows r;
  oakgpu_forest_outputs out;                 // the search's outputs, row-major over the live rows
  const double *p1_nash, *p2_nash, *nash_value; // rows x 9, rows x 9, rows; null without solve_nash
  LogEntry *log;                             // this turn's entries, one per row
  oak_pick::PolicyMode mode, fast_mode;      // fast_mode: the pick of a fast turn (the row's flag)
  double temp, minp;
  uint32_t rows;
  // keep_node: the row keeps the played cell; from the second turn on (else null) the advance's results, the kept search's mismatch bytes and carried nodes
  int keep;
  const uint8_t *advanced, *mismatch;
  const uint32_t *carried;
  double *matchup;     // by game index: the first search's empirical value
  const uint8_t *skip; // by game index, turn 1 only (else null): a skipped row's pick writes its matchup and nothing else
};

__global__ __launch_bounds__(BLOCK) void k_fsp_pick(PickArgs a) {
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  if (row >= a.rows) return;
  const int m = a.out.m[row], n = a.out.n[row];
  double ev, e1[9], e2[9], n1[9], n2[9], r1[9], r2[9], pol1[9], pol2[9], nv = 0.0;
  const uint64_t iterations = a.out.iterations[row];
  oak_pick::process_output(a.out.visit_matrix + (size_t)row * 81, a.out.value_matrix + (size_t)row * 81, m, n, iterations, &ev, e1, e2, nullptr);
  for (int q = 0; q < 9; ++q) {
    n1[q] = a.p1_nash && q < m ? a.p1_nash[(size_t)row * 9 + q] : 0.0;
    n2[q] = a.p2_nash && q < n ? a.p2_nash[(size_t)row * 9 + q] : 0.0;
    r1[q] = q < m ? a.out.p1_prior[(size_t)row * 9 + q] : 0.0;
    r2[q] = q < n ? a.out.p2_prior[(size_t)row * 9 + q] : 0.0;
  }
  if (a.nash_value) nv = a.nash_value[row];
  LogEntry *entry = a.log + row;
  const uint32_t game = a.r.game[row];
  entry->game = game;
  entry->cursor = a.r.cursor[row];
  uint8_t c1 = a.out.p1_choices[(size_t)row * 9], c2 = a.out.p2_choices[(size_t)row * 9];
  if (a.r.frames[row] == 0) a.matchup[game] = ev; // generate.cc:303-305: the first search's value is the built seats' target
  if (a.skip && a.skip[game]) { // no policy, no draw, no frame: the row takes a legal step with the rest and is retired with no record
    a.r.flag[row] = (uint8_t)OAKGPU_FSP_SKIPPED;
    entry->length = 0;
    a.r.c1[row] = c1;
    a.r.c2[row] = c2;
    if (a.keep) { a.r.pi[row] = 0; a.r.pj[row] = 0; }
    return;
  }
  uint32_t len = 0;
  uint8_t pi = 0, pj = 0;
  const bool fast = a.r.fast[row] != 0;
  const oak_pick::PolicyMode &mode = fast ? a.fast_mode : a.mode;
  if (!oak_pick::get_policy(r1, e1, n1, m, mode, a.temp, a.minp, pol1) || !oak_pick::get_policy(r2, e2, n2, n, mode, a.temp, a.minp, pol2)) {
    a.r.flag[row] = (uint8_t)OAKGPU_FSP_ZERO_POLICY; // the game stops here: its row takes a legal step and is retired with no record
  } else {
    uint64_t rng = a.r.rng[row];
    const int i = oak_pick::sample_pdf(pol1, m, rng), j = oak_pick::sample_pdf(pol2, n, rng);
    a.r.rng[row] = rng;
    c1 = a.out.p1_choices[(size_t)row * 9 + i];
    c2 = a.out.p2_choices[(size_t)row * 9 + j];
    pi = (uint8_t)i; pj = (uint8_t)j;
    len = oak_pick::encode_update(entry->bytes, (uint32_t)m, (uint32_t)n, c1, c2, (uint32_t)iterations, ev, nv, e1, n1, e2, n2);
    a.r.frames[row] += 1;
    if (fast) a.r.fastn[row] += 1;
    a.r.cursor[row] += len;
  }
  entry->length = len;
  a.r.c1[row] = c1;
  a.r.c2[row] = c2;
  if (a.keep) {
    a.r.pi[row] = pi; a.r.pj[row] = pj;
    if (a.advanced) {
      uint32_t kept = a.r.kept[row] + a.advanced[row];
      if (a.mismatch[row]) { if (kept) --kept; a.r.mism[row] += 1; }
      a.r.kept[row] = kept;
      a.r.carry[row] += a.carried[row];
    }
  }
}

} // namespace fsp
} // namespace oak

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {

using namespace oak::fsp;

#define RC(x) do { int _r = (x); if (_r) return _r; } while (0)

// the loop's workspace, attached to the forest and freed with it: everything sized by the batch is grow-only, the log grows by doubling
// between turns, the stream is sized by the records
struct Workspace {
  DeviceArrays dev;
  uint32_t capacity = 0; // rows
  Rows half[2] = {};
  uint64_t *tree_seed = nullptr;
  uint8_t *out_block = nullptr; // the search's outputs
  int32_t *pay = nullptr;
  double *nash = nullptr;       // rows x 9, rows x 9, rows
  uint8_t *first = nullptr, *results_out = nullptr, *status_out = nullptr, *d_teams = nullptr;
  uint32_t *frames_out = nullptr, *length_out = nullptr, *block_live = nullptr, *block_offset = nullptr, *ctl = nullptr;
  uint64_t *d_seeds = nullptr; // the host-array call's staging: battle seeds, then seeds
  unsigned long long *offsets = nullptr;
  LogEntry *log = nullptr;
  size_t log_capacity = 0;
  uint8_t *stream = nullptr;
  size_t stream_capacity = 0, stream_bytes = 0;
  uint32_t last_n = 0;
  bool have = false;
  uint64_t stats[4] = {0, 0, 0, 0};
  // keep_node: the advance's inputs and results per compacted row, the per-game counts, and the last call's totals
  uint32_t *src_row = nullptr, *kept_out = nullptr, *mism_out = nullptr, *carry_out = nullptr;
  uint8_t *adv_i = nullptr, *adv_j = nullptr, *adv_obs = nullptr, *advanced = nullptr;
  bool kept_call = false;
  uint64_t keep_stats[4] = {0, 0, 0, 0};
  uint64_t loop_syncs = 0, loop_copies = 0; // the turn loop's stream synchronisations and host <-> device copies
  // fast searches: the turn's budgets per compacted row, the games' fast frames, the last call's tree-iterations launched and run
  uint32_t *budget = nullptr, *fast_out = nullptr;
  uint64_t rows_launched = 0, rows_run = 0;
  bool partition = true;
  // the build side, by game index: the first search's empirical value, the skip byte, the host-array call's staging of `built`
  double *matchup = nullptr;
  uint8_t *skip = nullptr, *d_built = nullptr;
  std::vector<int32_t> h_pay;
  std::vector<double> h_nash;
  void release() {
    dev.free_all();
    if (log) (void)hipFree(log);
    if (stream) (void)hipFree(stream);
    log = nullptr; stream = nullptr; log_capacity = stream_capacity = 0; capacity = 0;
  }
};

void workspace_free(void *p) {
  Workspace *w = (Workspace *)p;
  w->release();
  delete w;
}

int workspace_for(oakgpu_forest *f, uint32_t n, Workspace **out) {
  Workspace *w = (Workspace *)oakgpu_forest_attachment(f);
  if (!w) {
    w = new Workspace();
    oakgpu_forest_set_attachment(f, w, workspace_free);
  }
  *out = w;
  if (w->capacity >= n) return 0;
  HIPCHK(hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(oakgpu_forest_ctx(f))));
  DeviceArrays &d = w->dev;
  d.free_all();
  w->capacity = 0;
  w->have = false;
  const size_t T = n, blocks = (T + BLOCK - 1) / BLOCK;
  for (int h = 0; h < 2; ++h) {
    Rows &r = w->half[h];
    RC(d.get(r.battles, T * 384)); RC(d.get(r.durations, T * 8)); RC(d.get(r.results, T)); RC(d.get(r.c1, T)); RC(d.get(r.c2, T)); RC(d.get(r.flag, T));
    RC(d.get(r.game, T)); RC(d.get(r.frames, T)); RC(d.get(r.cursor, T)); RC(d.get(r.rng, T)); RC(d.get(r.fast, T)); RC(d.get(r.fastn, T));
    if (oakgpu_forest_is_kept(f)) { RC(d.get(r.pi, T)); RC(d.get(r.pj, T)); RC(d.get(r.obs, T * 16)); RC(d.get(r.kept, T)); RC(d.get(r.mism, T)); RC(d.get(r.carry, T)); }
  }
  if (oakgpu_forest_is_kept(f)) {
    RC(d.get(w->src_row, T)); RC(d.get(w->kept_out, T)); RC(d.get(w->mism_out, T)); RC(d.get(w->carry_out, T));
    RC(d.get(w->adv_i, T)); RC(d.get(w->adv_j, T)); RC(d.get(w->adv_obs, T * 16)); RC(d.get(w->advanced, T));
  }
  RC(d.get(w->tree_seed, T)); RC(d.get(w->out_block, OUT_BYTES * T + 16 * 16)); RC(d.get(w->pay, T * PAY_STRIDE)); RC(d.get(w->nash, T * 19));
  RC(d.get(w->first, T * 384)); RC(d.get(w->results_out, T)); RC(d.get(w->status_out, T)); RC(d.get(w->d_teams, T * 60));
  RC(d.get(w->frames_out, T)); RC(d.get(w->length_out, T)); RC(d.get(w->block_live, 2 * blocks)); RC(d.get(w->block_offset, 2 * blocks)); RC(d.get(w->ctl, 4));
  RC(d.get(w->budget, T)); RC(d.get(w->fast_out, T));
  RC(d.get(w->matchup, T)); RC(d.get(w->skip, T)); RC(d.get(w->d_built, T));
  RC(d.get(w->d_seeds, 2 * T)); RC(d.get(w->offsets, T + 1));
  w->capacity = n;
  return 0;
}

int fail_fmt(const char *fmt, unsigned a) {
  char msg[256];
  snprintf(msg, sizeof msg, fmt, a);
  return oakgpu_fail_msg(msg);
}

} // namespace

extern "C" {

int oakgpu_forest_selfplay_check(uint32_t max_trees, uint32_t max_iterations, int contextual, const oakgpu_selfplay_params *prm, int has_net, uint32_t n,
                                 const uint8_t *teams, int solve_nash) {
  if (!prm) return oakgpu_fail_msg("oakgpu_forest_selfplay: null argument");
  if (prm->keep_node != 0 && !(contextual & OAKGPU_FOREST_KEPT))
    return oakgpu_fail_msg("oakgpu_forest_selfplay: keep_node is not supported on this forest (every turn searches a fresh tree): oakgpu_forest_create_kept makes one that keeps its trees");
  contextual &= ~OAKGPU_FOREST_KEPT;
  const std::string refusal = policy_refusal(prm->policy_mode, sizeof prm->policy_mode, prm->policy_min, solve_nash);
  if (!refusal.empty()) return oakgpu_fail_msg(("oakgpu_forest_selfplay: " + refusal).c_str());
  if (!(prm->fast_search_prob >= 0.0 && prm->fast_search_prob <= 1.0)) return oakgpu_fail_msg("oakgpu_forest_selfplay: fast_search_prob must be in [0, 1]");
  if (prm->fast_budget > max_iterations) return oakgpu_fail_msg("oakgpu_forest_selfplay: fast_budget exceeds the forest's max_iterations");
  const std::string fast_refusal = policy_refusal(prm->fast_policy_mode, sizeof prm->fast_policy_mode, prm->policy_min, solve_nash);
  if (!fast_refusal.empty()) return oakgpu_fail_msg(("oakgpu_forest_selfplay: fast_policy_mode: " + fast_refusal).c_str());
  if (int rc = oakgpu_forest_check(max_trees, max_iterations, contextual, &prm->search, has_net, n, nullptr, 0, 0)) {
    std::string msg = oakgpu_last_error();
    const std::string from = "oakgpu_forest_search:";
    if (msg.compare(0, from.size(), from) == 0) msg = "oakgpu_forest_selfplay: the forest search refuses:" + msg.substr(from.size());
    oakgpu_fail_msg(msg.c_str());
    return rc;
  }
  if (teams)
    for (uint32_t g = 0; g < n; ++g)
      if (oakgpu_endless_battle_check(teams + (size_t)g * 60))
        return fail_fmt("oakgpu_forest_selfplay: game %u: EBC check failed (every match-up is Ghost against Ghost with no move that can hit a Ghost, generate.cc:127-152)", g);
  return 0;
}

int oakgpu_forest_selfplay_skip_check(uint32_t max_iterations, const oakgpu_selfplay_skip *skip) {
  if (!skip) return 0;
  if (!(skip->battle_skip_prob >= 0.0 && skip->battle_skip_prob <= 1.0)) return oakgpu_fail_msg("oakgpu_forest_selfplay: battle_skip_prob must be in [0, 1]");
  if (skip->t1_budget > max_iterations) return oakgpu_fail_msg("oakgpu_forest_selfplay: t1_budget exceeds the forest's max_iterations");
  return 0;
}

int oakgpu_forest_selfplay_build_dev(oakgpu_forest *f, oakgpu_net *net, const oakgpu_selfplay_params *prm, const oakgpu_selfplay_skip *skip_prm, const uint8_t *teams,
                                     const uint64_t *battle_seeds, const uint64_t *seeds, const uint8_t *built, uint32_t n, int solve_nash) {
  if (!f || !prm) return oakgpu_fail_msg("oakgpu_forest_selfplay: null argument");
  const oakgpu_selfplay_skip skp = skip_prm ? *skip_prm : oakgpu_selfplay_skip{0, 0.0};
  uint32_t max_trees = 0, max_iterations = 0;
  int contextual = 0;
  oakgpu_forest_limits(f, &max_trees, &max_iterations, &contextual);
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  if (n && (!teams || !battle_seeds || !seeds)) return oakgpu_fail_msg("oakgpu_forest_selfplay: null argument");
  std::vector<uint8_t> h_teams((size_t)n * 60);
  if (n) { // the endless battle check reads the teams on the host: one copy, before anything is launched
    HIPCHK(hipMemcpyAsync(h_teams.data(), teams, h_teams.size(), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  if (oakgpu_forest_is_kept(f)) contextual |= OAKGPU_FOREST_KEPT;
  RC(oakgpu_forest_selfplay_check(max_trees, max_iterations, contextual, prm, net != nullptr, n, n ? h_teams.data() : nullptr, solve_nash));
  RC(oakgpu_forest_selfplay_skip_check(max_iterations, &skp));
  const bool keep = prm->keep_node != 0;
  Workspace *w = nullptr;
  RC(workspace_for(f, std::max(n, 1u), &w));
  w->have = false;
  w->kept_call = keep;
  w->keep_stats[0] = w->keep_stats[1] = w->keep_stats[2] = w->keep_stats[3] = 0;
  const uint8_t *d_mismatch = nullptr;
  const uint32_t *d_carried = nullptr, *d_dropped = nullptr;
  uint32_t dropped_before = 0;
  if (keep) {
    oakgpu_forest_keep_arrays(f, &d_mismatch, &d_carried, &d_dropped);
    HIPCHK(hipMemcpyAsync(&dropped_before, d_dropped, 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  w->last_n = n;
  w->stream_bytes = 0;
  w->stats[0] = w->stats[1] = w->stats[2] = w->stats[3] = 0;
  w->loop_syncs = w->loop_copies = 0;
  if (n == 0) { w->have = true; return 0; }
  oak_pick::PolicyMode mode, fast_mode;
  (void)oak_pick::parse_policy_mode(prm->policy_mode, sizeof prm->policy_mode, &mode);
  fast_mode = mode;
  if (prm->fast_policy_mode[0]) (void)oak_pick::parse_policy_mode(prm->fast_policy_mode, sizeof prm->fast_policy_mode, &fast_mode);
  const uint32_t max_len = prm->max_battle_length ? prm->max_battle_length : 2048;
  oakgpu_search_params sp = prm->search;
  sp.batch = 1; sp.seed = 0;
  // fast searches: the two budgets of a turn; the budgets search is sized by the larger
  FastArgs fa{};
  fa.prob = prm->fast_search_prob; fa.on = prm->fast_search_prob > 0 ? 1u : 0u; fa.partition = w->partition ? 1u : 0u;
  w->partition = true; // (the benchmark's switch holds for one call)
  fa.budget_full = (uint32_t)sp.iterations; fa.budget_fast = oak_pick::turn_budget(true, fa.budget_full, prm->fast_budget);
  fa.fast_first = fa.budget_fast > fa.budget_full ? 1u : 0u;
  oakgpu_search_params sp_budgets = sp;
  sp_budgets.iterations = std::max(fa.budget_full, fa.budget_fast);
  w->rows_launched = w->rows_run = 0;
  // skipped battles: the games' skip bytes hold on turn 1 alone, where a skipped row is searched with t1_budget iterations
  const bool skipping = built && skp.battle_skip_prob > 0;
  const uint32_t t1_budget = skp.t1_budget ? skp.t1_budget : fa.budget_full;
  oakgpu_search_params sp_first = sp_budgets;
  sp_first.iterations = std::max((uint32_t)sp_budgets.iterations, t1_budget);
  auto grid = [](uint32_t rows) { return dim3((rows + BLOCK - 1) / BLOCK); };

  // the opening: PKMN::battle + update(0, 0); the battle after it is the record's stored one
  int cur = 0;
  uint32_t rows = n;
  {
    Rows &r = w->half[0];
    RC(oakgpu_init_battles_dev(ctx, teams, battle_seeds, n, 1, r.battles, r.durations, r.results));
    HIPCHK(hipMemcpyAsync(w->first, r.battles, (size_t)n * 384, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(k_fsp_start, grid(n), dim3(BLOCK), 0, stream, r, seeds, n, keep ? 1 : 0, w->matchup, skipping ? built : nullptr, skp.battle_skip_prob, w->skip);
    HIPCHK(hipGetLastError());
  }
  if (!w->log) {
    RC(dev_alloc(w->log, first_log_capacity(n)));
    w->log_capacity = first_log_capacity(n);
  }
  oakgpu_forest_outputs o;
  size_t entries = 0;
  for (uint64_t turn = 0;; ++turn) {
    // retire what ended, compact the rest: the rows handed to the search are exactly the live games
    const uint32_t blocks = (rows + BLOCK - 1) / BLOCK;
    fa.blocks = blocks;
    const RetireArgs ra{w->half[cur], w->results_out, w->status_out, w->frames_out, w->length_out, w->block_live, rows, max_len,
                        keep ? w->kept_out : nullptr, keep ? w->mism_out : nullptr, keep ? w->carry_out : nullptr, w->fast_out, fa};
    hipLaunchKernelGGL(k_fsp_retire, grid(rows), dim3(BLOCK), 0, stream, ra);
    hipLaunchKernelGGL(k_rows_offsets, dim3(1), dim3(1024), 0, stream, w->block_live, fa.on ? 2 * blocks : blocks, w->block_offset, w->ctl);
    const bool advance = keep && turn > 0; // the first turn's trees are new
    const bool first_skips = skipping && turn == 0;
    const CompactArgs ca{w->half[cur], w->half[cur ^ 1], w->block_offset, w->tree_seed, rows, advance ? w->src_row : nullptr, w->adv_i, w->adv_j, w->adv_obs, keep ? 1 : 0,
                         fa, w->budget, first_skips ? w->skip : nullptr, t1_budget};
    hipLaunchKernelGGL(k_fsp_compact, grid(rows), dim3(BLOCK), 0, stream, ca);
    HIPCHK(hipGetLastError());
    uint32_t live = 0;
    HIPCHK(hipMemcpyAsync(&live, w->ctl, 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    ++w->stats[3];
    ++w->stats[2];
    ++w->loop_syncs;
    ++w->loop_copies;
    cur ^= 1;
    if (live > rows) return oakgpu_fail_msg("oakgpu_forest_selfplay: the live count grew (internal error)");
    rows = live;
    if (rows == 0) break;
    if (turn > (uint64_t)max_len + 1) return oakgpu_fail_msg("oakgpu_forest_selfplay: a game outlived max_battle_length (internal error)");
    Rows &r = w->half[cur];
    ++w->stats[0];
    w->stats[1] += rows;
    if (entries + rows > w->log_capacity) { // the log follows the frames played: doubled between turns
      const size_t want = std::max(w->log_capacity * 2, entries + rows);
      RC(grow_log(w->log, entries, want, stream));
      w->log_capacity = want;
    }
    carve_outputs(w->out_block, rows, &o);
    if (advance) { // every live game's tree: re-rooted at the child it played into, and moved to the game's new row
      RC(oakgpu_forest_advance_dev(f, w->adv_i, w->adv_j, w->adv_obs, w->src_row, rows, w->advanced));
      if (fa.on) RC(oakgpu_forest_search_budgets_kept_dev(f, net, &sp_budgets, r.battles, r.durations, r.results, w->tree_seed, w->budget, rows, &o, nullptr, 0));
      else RC(oakgpu_forest_search_kept_dev(f, net, &sp, r.battles, r.durations, r.results, w->tree_seed, rows, &o, nullptr, 0));
    } else if (first_skips && (fa.on || t1_budget != fa.budget_full)) // (turn 1: a skipped row's budget differs; the first turn's trees are new)
      RC(oakgpu_forest_search_budgets_dev(f, net, &sp_first, r.battles, r.durations, r.results, w->tree_seed, w->budget, rows, &o, nullptr, 0));
    else if (fa.on) RC(oakgpu_forest_search_budgets_dev(f, net, &sp_budgets, r.battles, r.durations, r.results, w->tree_seed, w->budget, rows, &o, nullptr, 0));
    else RC(oakgpu_forest_search_dev(f, net, &sp, r.battles, r.durations, r.results, w->tree_seed, rows, &o, nullptr, 0));
    {
      uint64_t tree_iterations[2];
      RC(oakgpu_forest_last_rows(f, tree_iterations));
      w->rows_launched += tree_iterations[0]; w->rows_run += tree_iterations[1];
    }
    double *d_p1 = nullptr, *d_p2 = nullptr, *d_nv = nullptr;
    if (solve_nash) {
      RC(solve_turn(ctx, stream, solve_nash, o, rows, w->pay, w->nash, w->h_pay, w->h_nash));
      if (solve_nash == 1) { // the host solve: the download and the upload, its synchronisation and the one after the update
        w->loop_syncs += 2;
        w->loop_copies += 2;
      }
      d_p1 = w->nash; d_p2 = w->nash + (size_t)rows * 9; d_nv = w->nash + (size_t)rows * 18;
    }
    PickArgs pk{};
    pk.r = r; pk.out = o; pk.p1_nash = d_p1; pk.p2_nash = d_p2; pk.nash_value = d_nv; pk.log = w->log + entries; pk.mode = mode; pk.fast_mode = fast_mode;
    pk.temp = prm->policy_temp > 0 ? prm->policy_temp : 1.0; pk.minp = prm->policy_min; pk.rows = rows;
    pk.keep = keep ? 1 : 0;
    if (advance) { pk.advanced = w->advanced; pk.mismatch = d_mismatch; pk.carried = d_carried; }
    pk.matchup = w->matchup; pk.skip = first_skips ? w->skip : nullptr;
    hipLaunchKernelGGL(k_fsp_pick, grid(rows), dim3(BLOCK), 0, stream, pk);
    HIPCHK(hipGetLastError());
    entries += rows;
    // PKMN::update(battle, c1, c2, options); durations <- options (generate.cc:319-322)
    RC(oakgpu_update_dev(ctx, r.battles, r.c1, r.c2, r.durations, keep ? r.obs : nullptr, nullptr, rows, r.results));
    if (solve_nash == 1) HIPCHK(hipStreamSynchronize(stream)); // (the strategies' host copy is reused next turn)
  }

  // pack: record bases in game order, the headers, the log's updates
  size_t total = 0;
  RC(record_bases(stream, w->length_out, n, w->offsets, &w->stream, 1, &w->stream_capacity, &total));
  if (total) {
    if (entries > 0xFFFFFFFFull) return oakgpu_fail_msg("oakgpu_forest_selfplay: more than 2^32 frames in one call");
    RC(pack_records(stream, PackArgs{w->offsets, w->frames_out, w->length_out, w->results_out, w->status_out, w->first, w->log, w->stream, n, (uint32_t)entries}));
  }
  HIPCHK(hipStreamSynchronize(stream));
  if (keep) { // the per-game counts, read once: the call's totals
    std::vector<uint32_t> h((size_t)n * 3);
    uint32_t dropped_after = 0;
    HIPCHK(hipMemcpyAsync(h.data(), w->kept_out, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h.data() + n, w->mism_out, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h.data() + 2 * (size_t)n, w->carry_out, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&dropped_after, d_dropped, 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (uint32_t g = 0; g < n; ++g) { w->keep_stats[0] += h[g]; w->keep_stats[2] += h[n + g]; w->keep_stats[3] += h[2 * (size_t)n + g]; }
    w->keep_stats[1] = dropped_after - dropped_before;
  }
  w->stream_bytes = (size_t)total;
  w->have = true;
  return 0;
}

int oakgpu_forest_selfplay_dev(oakgpu_forest *f, oakgpu_net *net, const oakgpu_selfplay_params *prm, const uint8_t *teams, const uint64_t *battle_seeds,
                               const uint64_t *seeds, uint32_t n, int solve_nash) {
  return oakgpu_forest_selfplay_build_dev(f, net, prm, nullptr, teams, battle_seeds, seeds, nullptr, n, solve_nash);
}

int oakgpu_forest_selfplay_matchup(oakgpu_forest *f, double *out, int to_device) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_selfplay_matchup: null argument");
  Workspace *w = (Workspace *)oakgpu_forest_attachment(f);
  if (!w || !w->have) return oakgpu_fail_msg("oakgpu_forest_selfplay_matchup: the forest holds no finished self-play call");
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  if (w->last_n) HIPCHK(hipMemcpyAsync(out, w->matchup, (size_t)w->last_n * 8, to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_selfplay_skip_host(uint64_t seed, double prob, int built) { return oak_pick::game_is_skipped(seed, prob, built) ? 1 : 0; }

int oakgpu_forest_selfplay_nodes_kept(oakgpu_forest *f, uint32_t *nodes_kept, int to_device) {
  if (!f || !nodes_kept) return oakgpu_fail_msg("oakgpu_forest_selfplay_nodes_kept: null argument");
  Workspace *w = (Workspace *)oakgpu_forest_attachment(f);
  if (!w || !w->have) return oakgpu_fail_msg("oakgpu_forest_selfplay_nodes_kept: the forest holds no finished self-play call");
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  const size_t n = w->last_n;
  if (n) {
    if (w->kept_call) HIPCHK(hipMemcpyAsync(nodes_kept, w->kept_out, n * 4, to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    else if (to_device) HIPCHK(hipMemsetAsync(nodes_kept, 0, n * 4, stream));
    else memset(nodes_kept, 0, n * 4);
  }
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_forest_selfplay_fast_stats(oakgpu_forest *f, uint64_t out[4]) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_selfplay_fast_stats: null argument");
  Workspace *w = (Workspace *)oakgpu_forest_attachment(f);
  if (!w || !w->have) return oakgpu_fail_msg("oakgpu_forest_selfplay_fast_stats: the forest holds no finished self-play call");
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  const size_t n = w->last_n;
  std::vector<uint32_t> fast(n), frames(n);
  std::vector<uint8_t> status(n);
  if (n) { // the per-game counts, read when asked for
    HIPCHK(hipMemcpyAsync(fast.data(), w->fast_out, n * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(frames.data(), w->frames_out, n * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(status.data(), w->status_out, n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  out[0] = out[1] = 0;
  for (size_t g = 0; g < n; ++g)
    if (status[g] == OAKGPU_FSP_OK) { out[0] += fast[g]; out[1] += frames[g] - fast[g]; }
  out[2] = w->rows_launched; out[3] = w->rows_run;
  return 0;
}

int oakgpu_forest_selfplay_set_partition(oakgpu_forest *f, int on) {
  if (!f) return oakgpu_fail_msg("oakgpu_forest_selfplay_set_partition: null argument");
  Workspace *w = (Workspace *)oakgpu_forest_attachment(f);
  if (!w) {
    w = new Workspace();
    oakgpu_forest_set_attachment(f, w, workspace_free);
  }
  w->partition = on != 0;
  return 0;
}

int oakgpu_forest_selfplay_keep_stats(const oakgpu_forest *f, uint64_t out[4]) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_selfplay_keep_stats: null argument");
  const Workspace *w = (const Workspace *)oakgpu_forest_attachment(f);
  for (int q = 0; q < 4; ++q) out[q] = w ? w->keep_stats[q] : 0;
  return 0;
}

int oakgpu_forest_selfplay_records(oakgpu_forest *f, uint8_t *stream_out, size_t capacity, size_t *bytes, uint64_t *offsets, uint32_t *n_frames, uint8_t *results,
                                   uint8_t *status, int to_device) {
  if (!f) return oakgpu_fail_msg("oakgpu_forest_selfplay_records: null argument");
  Workspace *w = (Workspace *)oakgpu_forest_attachment(f);
  if (!w || !w->have) return oakgpu_fail_msg("oakgpu_forest_selfplay_records: the forest holds no finished self-play call");
  if (bytes) *bytes = w->stream_bytes;
  if (stream_out && capacity < w->stream_bytes) return oakgpu_fail_msg("oakgpu_forest_selfplay_records: buffer too small");
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  const Records held{w->stream, w->stream_bytes, w->offsets, w->frames_out, w->results_out, w->status_out, w->last_n};
  return copy_records((hipStream_t)oakgpu_ctx_stream(ctx), held, stream_out, offsets, n_frames, results, status, to_device);
}

int oakgpu_forest_selfplay_build(oakgpu_forest *f, oakgpu_net *net, const oakgpu_selfplay_params *prm, const oakgpu_selfplay_skip *skip_prm, const uint8_t *teams,
                                 const uint64_t *battle_seeds, const uint64_t *seeds, const uint8_t *built, uint32_t n, int solve_nash) {
  if (!f || !prm || (n && (!teams || !battle_seeds || !seeds))) return oakgpu_fail_msg("oakgpu_forest_selfplay: null argument");
  uint32_t max_trees = 0, max_iterations = 0;
  int contextual = 0;
  oakgpu_forest_limits(f, &max_trees, &max_iterations, &contextual);
  if (oakgpu_forest_is_kept(f)) contextual |= OAKGPU_FOREST_KEPT;
  RC(oakgpu_forest_selfplay_check(max_trees, max_iterations, contextual, prm, net != nullptr, n, teams, solve_nash));
  RC(oakgpu_forest_selfplay_skip_check(max_iterations, skip_prm));
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  Workspace *w = nullptr;
  RC(workspace_for(f, std::max(n, 1u), &w));
  if (n) {
    HIPCHK(hipMemcpyAsync(w->d_teams, teams, (size_t)n * 60, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(w->d_seeds, battle_seeds, (size_t)n * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(w->d_seeds + n, seeds, (size_t)n * 8, hipMemcpyHostToDevice, stream));
    if (built) HIPCHK(hipMemcpyAsync(w->d_built, built, n, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  return oakgpu_forest_selfplay_build_dev(f, net, prm, skip_prm, w->d_teams, w->d_seeds, w->d_seeds + n, built && n ? w->d_built : nullptr, n, solve_nash);
}

int oakgpu_forest_selfplay(oakgpu_forest *f, oakgpu_net *net, const oakgpu_selfplay_params *prm, const uint8_t *teams, const uint64_t *battle_seeds,
                           const uint64_t *seeds, uint32_t n, int solve_nash) {
  return oakgpu_forest_selfplay_build(f, net, prm, nullptr, teams, battle_seeds, seeds, nullptr, n, solve_nash);
}

int oakgpu_forest_selfplay_last_traffic(const oakgpu_forest *f, uint64_t out[2]) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_selfplay_last_traffic: null argument");
  const Workspace *w = (const Workspace *)oakgpu_forest_attachment(f);
  out[0] = w ? w->loop_syncs : 0;
  out[1] = w ? w->loop_copies : 0;
  return 0;
}

int oakgpu_forest_selfplay_last_stats(const oakgpu_forest *f, uint64_t out[4]) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_selfplay_last_stats: null argument");
  const Workspace *w = (const Workspace *)oakgpu_forest_attachment(f);
  for (int q = 0; q < 4; ++q) out[q] = w ? w->stats[q] : 0;
  return 0;
}

} // extern "C"
