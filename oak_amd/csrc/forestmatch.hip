// oak_amd/csrc/forestmatch.hip -- matches between two search agents over the forest search: a batch of games resident on one device, seat p1
// and seat p2 each with its own search, network and policy options (the contract is in include/oakgpu.h; the per-game form is vs.cc:230-345).
//
//   k_fm_start   : row g is game g at turn 0: its stream, its counter
//   k_fm_retire  : one lane per row: a finished, stopped or cut row scatters result, turn count and status by game index and counts itself;
//                  how many rows of each block are still live
//   k_rows_offsets: (game_rows.hpp) the exclusive prefix sums of those per-block counts, and their total = the live count
//   k_fm_compact : the live rows, in order, into the other half of the double buffer, each with its two choice counts and the first legal
//                  choice of either side (what an unsearched seat plays)
//   k_fm_prelude : one workgroup over the live rows: the streams advance, both seats' tree seeds, both seats' row lists by a stable prefix
//                  sum (game_rows.hpp's scan pass), and the 12-byte record the host reads: live rows, p1 rows, p2 rows
//   k_fm_gather  : 24 lanes per listed row: battle (16-byte pieces), durations, result byte into the seat's contiguous search input
//   k_fsp_payoffs: (forest_rows.hpp's solve_turn, solve_nash) the integer payoffs for the host threads that solve them (1) or for
//                  oakgpu_nash_solve_dev (2)
//   k_fm_pick    : one lane per listed row: selfplay_pick.hpp's rule for ONE side of the seat's own root output, the early-stop sign,
//                  scattered back by row list
//   k_fm_finish  : one lane per live row: the early stop, the turn's log record, the turn count
// Recording (oakgpu_forest_match_set_records; the <true> forms of pick and finish, the <false> forms are the loop without it): each seat has
// a turn-major log of forest_rows.hpp's LogEntry, one entry per live row per turn.  k_fm_pick<true> encodes the seat's own root output into
// the row's entry while that output is still in the workspace, with the choice bytes open; k_fm_finish<true>, which runs when both seats
// have picked, writes the joint choice into both entries, encodes an unsearched seat's entry whole, gives every entry its game, cursor and
// length (0 for a turn that makes no update) and moves the game's cursor.  Both seats' entries of a turn have the same length, so ONE
// cursor per game, kept by game index, serves both logs, and one scan of the record lengths serves both streams.
//   k_fm_record_lengths: one lane per game: the record's length (0 for a cut or zeroed game) and the byte the pack kernels keep a game by
//   k_fsp_lengths, k_fsp_pack_head, k_fsp_pack_log: (forest_rows.hpp) the record bases, then per seat the heads and the log's updates
// Every kernel is a plain grid over rows, games or entries (the scans: one workgroup); none waits for another block.  Between gather and pick runs
// oakgpu_forest_search_dev over exactly the seat's rows, after finish oakgpu_update_dev over the live rows.  Retire and compact run on
// game_rows.hpp's place, move and live count, with this loop's own row; the host's Nash solve, log growth, record bases, pack and records'
// copies are forest_rows.hpp's, shared with forestplay.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/oakgpu.h"
#include "oakgpu_internal.h"
#include "selfplay_pick.hpp"
#include "forest_rows.hpp"

namespace oak {
namespace fm {

using game_rows::BLOCK;
using game_rows::DEAD;
using game_rows::NO_ROW;
using game_rows::u32x4;
using fsp::HEAD_BYTES;
using fsp::LogEntry;
enum : uint8_t { FLAG_NONE = 0, FLAG_ZERO_POLICY = 2, FLAG_EARLY_WIN = 3, FLAG_EARLY_LOSE = 4 }; // a row's stop flag between pick and retire
static_assert(sizeof(oakgpu_match_turn) == 24, "one log record is 24 bytes");

// t = (log(ev) - log(1 - ev)) / early_stop, cut to its sign at +-1 (vs.cc:263,287,300): ev = 1 / 0 give +-inf
OAK_PICK_HD inline int early_stop_sign(double ev, double early_stop) {
#pragma clang fp contract(off)
  if (!(early_stop > 0)) return 0;
  const double t = (log(ev) - log(1.0 - ev)) / early_stop;
  return t >= 1.0 ? 1 : t <= -1.0 ? -1 : 0;
}

// One seat's pick from one root output (matrices of row stride 9): process_output, get_policy for `side`, sample_pdf.  false: the cut
// zeroed the policy (nothing is drawn).  e1 / e2 (9 entries each) receive process_output's empirical strategies of both sides.
OAK_PICK_HD inline bool seat_pick(int side, const uint64_t *visit_matrix, const double *value_matrix, int m, int n, uint64_t iterations, const double *nash,
                                  const double *prior, const oak_pick::PolicyMode &mode, double temp, double minp, uint64_t &rng, double *policy, int *index,
                                  double *ev, double *e1, double *e2) {
  double nn[9], pr[9];
  oak_pick::process_output(visit_matrix, value_matrix, m, n, iterations, ev, e1, e2, nullptr);
  const int k = side ? n : m;
  for (int q = 0; q < 9; ++q) {
    nn[q] = nash && q < k ? nash[q] : 0.0;
    pr[q] = prior && q < k ? prior[q] : 0.0;
  }
  if (!oak_pick::get_policy(pr, side ? e2 : e1, nn, k, mode, temp, minp, policy)) return false;
  *index = oak_pick::sample_pdf(policy, k, rng);
  return true;
}

// one half of the double buffer: a row is its battle, durations, result byte, the two choice counts, the joint choice for the update (the
// first legal choices until a searched seat picks), the stop flag, both seats' ev and early-stop sign, its game, the game's stream and turns
struct Rows {
  uint8_t *battles, *durations, *results, *m, *n, *c1, *c2, *flag;
  int8_t *s1, *s2;
  uint32_t *game, *turns;
  uint64_t *rng;
  double *ev1, *ev2;
};

__global__ __launch_bounds__(BLOCK) void k_fm_start(Rows r, const uint64_t *seeds, uint32_t n) {
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  if (row >= n) return;
  r.game[row] = row;
  r.turns[row] = 0;
  r.flag[row] = FLAG_NONE;
  r.rng[row] = seeds[row] ^ oak_pick::GAME_STREAM_XOR;
}

struct RetireArgs {
  Rows r;
  uint8_t *results_out, *status_out; // by game index
  uint32_t *turns_out;
  unsigned long long *counts;        // wins, ties, losses of seat p1, stopped at max_turns
  uint32_t *block_live;              // per block of BLOCK rows: rows still live after this pass
  uint32_t rows, max_turns;
};

__global__ __launch_bounds__(BLOCK) void k_fm_retire(RetireArgs a) {
  __shared__ uint32_t wave_live[BLOCK / 64];
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  const bool in = row < a.rows;
  const uint32_t g = in ? a.r.game[row] : DEAD;
  bool live = false;
  if (g != DEAD) {
    const uint32_t flag = a.r.flag[row], turns = a.r.turns[row];
    uint32_t res = a.r.results[row];
    // the loop's order: a zeroed policy or an early stop ended the game before its update (the row took a legal step since, which is
    // not the game's); a terminal result ends it; only then is another turn due
    uint32_t status = DEAD;
    if (flag == FLAG_ZERO_POLICY) { status = OAKGPU_FM_ZERO_POLICY; res = 0xFF; }
    else if (flag == FLAG_EARLY_WIN || flag == FLAG_EARLY_LOSE) { status = OAKGPU_FM_EARLY_STOP; res = flag == FLAG_EARLY_WIN ? 1u : 2u; }
    else if ((res & 15) != 0) status = OAKGPU_FM_OK;
    else if (turns >= a.max_turns) status = OAKGPU_FM_MAX_TURNS;
    if (status == DEAD) live = true;
    else {
      a.results_out[g] = (uint8_t)res;
      a.turns_out[g] = turns;
      a.status_out[g] = (uint8_t)status;
      a.r.game[row] = DEAD;
      if (status == OAKGPU_FM_MAX_TURNS) atomicAdd(a.counts + 3, 1ull);
      else if (status != OAKGPU_FM_ZERO_POLICY) {
        const uint32_t type = res & 15;
        if (type >= 1 && type <= 3) atomicAdd(a.counts + (type == 1 ? 0 : type == 3 ? 1 : 2), 1ull);
      }
    }
  }
  game_rows::count_block_live(live, wave_live, a.block_live);
}

struct CompactArgs {
  Rows from, to;
  const uint32_t *block_offset;
  const uint8_t *ch1, *cnt1, *ch2, *cnt2; // oakgpu_choices_dev over the rows of `from`: rows x 9, rows
  uint32_t rows;
};

// Stable (game_rows.hpp: compact_place, compact_battles).  The turn's choice counts and default choices ride along.
__global__ __launch_bounds__(BLOCK) void k_fm_compact(CompactArgs a) {
  __shared__ uint32_t wave_total[BLOCK / 64];
  __shared__ uint32_t place[BLOCK];
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = row < a.rows && a.from.game[row] != DEAD;
  const uint32_t to = game_rows::compact_place(live, a.block_offset[blockIdx.x], wave_total, place);
  if (live) {
    *((uint2 *)a.to.durations + to) = *((const uint2 *)a.from.durations + row);
    a.to.results[to] = a.from.results[row];
    a.to.m[to] = a.cnt1[row];
    a.to.n[to] = a.cnt2[row];
    a.to.c1[to] = a.ch1[(size_t)row * 9];
    a.to.c2[to] = a.ch2[(size_t)row * 9];
    a.to.flag[to] = FLAG_NONE;
    a.to.s1[to] = 0;
    a.to.s2[to] = 0;
    a.to.ev1[to] = 0.0;
    a.to.ev2[to] = 0.0;
    a.to.game[to] = a.from.game[row];
    a.to.turns[to] = a.from.turns[row];
    a.to.rng[to] = a.from.rng[row];
  }
  __syncthreads();
  game_rows::compact_battles(a.from.battles, a.to.battles, a.rows, place);
}

struct PreludeArgs {
  Rows r;
  uint32_t *ctl;                 // [0] = the live count (k_rows_offsets' total), [1], [2] = the seats' row counts: the host's 12 bytes
  uint32_t *list1, *list2;       // the live rows with m > 1 / n > 1, in row order
  uint64_t *seed1, *seed2;       // per list entry: the seed of that seat's tree
  uint32_t capacity;             // rows the buffers hold (a live count above it is never followed)
};

// The turn prelude, one workgroup of 1,024: per live row the stream advances -- seat p1's seed first, then seat p2's, each only where the
// seat has more than one choice -- and both row lists are built by one scan of the two flags packed into a dword (16 bits each: a pass
// holds 1,024 rows, so neither half overflows within game_rows.hpp's scan pass), with the carries of the two lists in registers.
__global__ __launch_bounds__(1024) void k_fm_prelude(PreludeArgs a) {
  __shared__ uint32_t wave_total[16];
  const uint32_t live = a.ctl[0] < a.capacity ? a.ctl[0] : a.capacity;
  uint32_t carry1 = 0, carry2 = 0;
  for (uint32_t base = 0; base < live; base += 1024) {
    const uint32_t row = base + threadIdx.x;
    const bool in = row < live;
    const bool f1 = in && a.r.m[row] > 1, f2 = in && a.r.n[row] > 1;
    const game_rows::ScanPass<uint32_t> s = game_rows::scan_pass((f1 ? 1u : 0u) | (f2 ? 0x10000u : 0u), wave_total);
    if (f1 || f2) {
      uint64_t rng = a.r.rng[row];
      if (f1) {
        const uint32_t k = carry1 + (s.before & 0xFFFFu);
        a.list1[k] = row;
        a.seed1[k] = oak_pick::splitmix64(rng);
      }
      if (f2) {
        const uint32_t k = carry2 + (s.before >> 16);
        a.list2[k] = row;
        a.seed2[k] = oak_pick::splitmix64(rng);
      }
      a.r.rng[row] = rng;
    }
    carry1 += s.total & 0xFFFFu;
    carry2 += s.total >> 16;
  }
  if (threadIdx.x == 0) { a.ctl[1] = carry1; a.ctl[2] = carry2; }
}

struct GatherArgs {
  Rows r;
  const uint32_t *list;
  uint8_t *battles, *durations, *results; // count x 384 (16-byte aligned), count x 8, count
  uint32_t count;
};

// 393 bytes per listed row: the battle as 24 pieces of 16 bytes, one lane each; the piece-0 lane also moves the durations and the result
__global__ __launch_bounds__(BLOCK) void k_fm_gather(GatherArgs a) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x, k = i / 24, w = i - k * 24;
  if (k >= a.count) return;
  const uint32_t row = a.list[k];
  ((u32x4 *)a.battles)[(size_t)k * 24 + w] = ((const u32x4 *)a.r.battles)[(size_t)row * 24 + w];
  if (w == 0) {
    *((uint2 *)a.durations + k) = *((const uint2 *)a.r.durations + row);
    a.results[k] = a.r.results[row];
  }
}

struct PickArgs {
  Rows r;
  const uint32_t *list;
  oakgpu_forest_outputs out;    // the seat's search outputs, one row per list entry
  const double *nash;           // the seat's own side's strategies, count x 9; null without solve_nash
  oak_pick::PolicyMode mode;
  double temp, minp, early_stop;
  uint32_t count;
  int side;                     // 0: seat p1, 1: seat p2
  // recording: this seat's log entries of the turn, one per live row, and the search's whole solve (count x 9 of p1, count x 9 of p2, count
  // values; null without solve_nash)
  LogEntry *rlog;
  const double *nash_all;
};

template <bool REC> __global__ __launch_bounds__(BLOCK) void k_fm_pick(PickArgs a) {
  const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= a.count) return;
  const uint32_t row = a.list[k];
  if (a.r.flag[row] != FLAG_NONE) return; // (seat p1's policy was zeroed: the game stopped there, seat p2 draws nothing)
  const int m = a.out.m[k], n = a.out.n[k];
  double policy[9], ev, e1[9], e2[9];
  int index = 0;
  uint64_t rng = a.r.rng[row];
  const double *prior = (a.side ? a.out.p2_prior : a.out.p1_prior) + (size_t)k * 9;
  if (!seat_pick(a.side, a.out.visit_matrix + (size_t)k * 81, a.out.value_matrix + (size_t)k * 81, m, n, a.out.iterations[k],
                 a.nash ? a.nash + (size_t)k * 9 : nullptr, prior, a.mode, a.temp, a.minp, rng, policy, &index, &ev, e1, e2)) {
    a.r.flag[row] = FLAG_ZERO_POLICY;
    return;
  }
  a.r.rng[row] = rng;
  const int8_t s = (int8_t)early_stop_sign(ev, a.early_stop);
  if (a.side == 0) {
    a.r.c1[row] = a.out.p1_choices[(size_t)k * 9 + index];
    a.r.ev1[row] = ev;
    a.r.s1[row] = s;
  } else {
    a.r.c2[row] = a.out.p2_choices[(size_t)k * 9 + index];
    a.r.ev2[row] = ev;
    a.r.s2[row] = s;
  }
  if (REC) { // the seat's own output as the turn's update, the joint choice left open until both seats have picked (k_fm_finish)
    double n1[9], n2[9], nv = 0.0;
    for (int q = 0; q < 9; ++q) {
      n1[q] = a.nash_all && q < m ? a.nash_all[(size_t)k * 9 + q] : 0.0;
      n2[q] = a.nash_all && q < n ? a.nash_all[((size_t)a.count + k) * 9 + q] : 0.0;
    }
    if (a.nash_all) nv = a.nash_all[(size_t)a.count * 18 + k];
    (void)oak_pick::encode_update(a.rlog[row].bytes, (uint32_t)m, (uint32_t)n, 0, 0, (uint32_t)a.out.iterations[k], ev, nv, e1, n1, e2, n2);
  }
}

struct FinishArgs {
  Rows r;
  oakgpu_match_turn *log; // n x log_turns, game-major; nullable
  uint32_t rows, log_turns;
  LogEntry *rlog1, *rlog2; // recording: the seats' log entries of this turn, one per live row
  uint32_t *cursor;        // recording: by game index, the bytes of updates in the game's records so far (the same for both seats)
};

template <bool REC> __global__ __launch_bounds__(BLOCK) void k_fm_finish(FinishArgs a) {
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  if (row >= a.rows) return;
  const bool zeroed = a.r.flag[row] != FLAG_NONE;
  const int s1 = a.r.s1[row], s2 = a.r.s2[row];
  const bool stop = s1 * s2 > 0;
  if (REC) {
    const uint32_t g = a.r.game[row], m = a.r.m[row], n = a.r.n[row];
    const bool made = !zeroed && !stop; // (a zeroed policy or an early stop: the update is not made, nothing is recorded)
    const uint32_t at = a.cursor[g], len = made ? (uint32_t)oak_pick::update_bytes(m, n) : 0u;
    LogEntry *e[2] = {a.rlog1 + row, a.rlog2 + row};
    for (int s = 0; s < 2; ++s) {
      e[s]->game = g;
      e[s]->cursor = at;
      e[s]->length = len;
      if (!made) continue;
      const uint8_t c1 = a.r.c1[row], c2 = a.r.c2[row];
      if ((s ? n : m) > 1) { e[s]->bytes[1] = c1; e[s]->bytes[2] = c2; }
      else { // an unsearched seat: the real m and n, the joint choice, iterations 0 and every value and strategy 0
        const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        (void)oak_pick::encode_update(e[s]->bytes, m, n, c1, c2, 0u, 0.0, 0.0, zero, zero, zero, zero);
      }
    }
    if (made) a.cursor[g] = at + len;
  }
  if (zeroed) return; // (a zeroed policy: no record, no turn)
  const uint32_t turn = a.r.turns[row];
  if (a.log && turn < a.log_turns) {
    oakgpu_match_turn t;
    t.c1 = stop ? 0 : a.r.c1[row];
    t.c2 = stop ? 0 : a.r.c2[row];
    t.m = a.r.m[row];
    t.n = a.r.n[row];
    t.zero = 0;
    t.ev_p1 = a.r.ev1[row];
    t.ev_p2 = a.r.ev2[row];
    a.log[(size_t)a.r.game[row] * a.log_turns + turn] = t;
  }
  if (stop) a.r.flag[row] = s1 > 0 ? FLAG_EARLY_WIN : FLAG_EARLY_LOSE;
  else a.r.turns[row] = turn + 1;
}

// recording, after the last turn: a finished or early-stopped game keeps a record (head + its updates; 0 frames when its input was
// terminal), a cut or zeroed game has none.  keep: 0 for a kept game -- what the pack kernels read as their status byte.
__global__ __launch_bounds__(BLOCK) void k_fm_record_lengths(const uint8_t *status, const uint32_t *cursor, uint32_t *length, uint8_t *keep, uint32_t n) {
  const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n) return;
  const bool kept = status[g] == OAKGPU_FM_OK || status[g] == OAKGPU_FM_EARLY_STOP;
  length[g] = kept ? HEAD_BYTES + cursor[g] : 0u;
  keep[g] = kept ? 0 : 1;
}

} // namespace fm
} // namespace oak

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {

using namespace oak::fm;
using oak::fsp::carve_outputs;
using oak::fsp::copy_records;
using oak::fsp::DeviceArrays;
using oak::fsp::first_log_capacity;
using oak::fsp::grow_log;
using oak::fsp::k_rows_offsets;
using oak::fsp::OUT_BYTES;
using oak::fsp::pack_records;
using oak::fsp::PackArgs;
using oak::fsp::PAY_STRIDE;
using oak::fsp::policy_refusal;
using oak::fsp::record_bases;
using oak::fsp::Records;
using oak::fsp::solve_turn;

#define RC(x) do { int _r = (x); if (_r) return _r; } while (0)

// the loop's workspace, attached to the forest and freed with it: grow-only, sized by the batch.  What recording needs is allocated by the
// first call that records: the per-game arrays sized by the batch, the two logs grown by doubling between turns as forestplay.hip's, the
// two streams sized by the records.
struct Workspace {
  DeviceArrays dev;
  uint32_t capacity = 0; // rows
  Rows half[2] = {};
  uint8_t *ch1 = nullptr, *cnt1 = nullptr, *ch2 = nullptr, *cnt2 = nullptr;
  uint32_t *list[2] = {nullptr, nullptr};
  uint64_t *seed[2] = {nullptr, nullptr};
  uint8_t *gb = nullptr, *gd = nullptr, *gr = nullptr; // a seat's gathered search input
  uint8_t *out_block[2] = {nullptr, nullptr};          // a seat's search outputs
  int32_t *pay = nullptr;
  double *nash[2] = {nullptr, nullptr};                // rows x 9, rows x 9, rows
  uint8_t *results_out = nullptr, *status_out = nullptr;
  uint32_t *turns_out = nullptr, *block_live = nullptr, *block_offset = nullptr, *ctl = nullptr;
  unsigned long long *counts = nullptr;
  uint8_t *in_b = nullptr, *in_d = nullptr, *in_r = nullptr; // the host-array call's staging
  uint64_t *in_seeds = nullptr;
  oakgpu_match_turn *log_stage = nullptr;
  size_t log_capacity = 0;
  uint64_t stats[4] = {0, 0, 0, 0};
  std::vector<int32_t> h_pay;
  std::vector<double> h_nash;
  // recording
  bool records_on = false, have_records = false;
  DeviceArrays rec_dev;
  uint32_t rec_capacity = 0, last_n = 0;               // games
  uint32_t *cursor = nullptr, *length = nullptr;       // by game index
  uint8_t *keep = nullptr;
  unsigned long long *offsets = nullptr;               // games + 1
  LogEntry *rlog[2] = {nullptr, nullptr};
  size_t rlog_capacity = 0;                            // entries of each log
  uint8_t *stream[2] = {nullptr, nullptr};
  size_t stream_capacity = 0, stream_bytes = 0;        // of each stream: the two are the same size
  void release_records() {
    rec_dev.free_all();
    for (int s = 0; s < 2; ++s) {
      if (rlog[s]) (void)hipFree(rlog[s]);
      if (stream[s]) (void)hipFree(stream[s]);
      rlog[s] = nullptr; stream[s] = nullptr;
    }
    rec_capacity = 0; rlog_capacity = 0; stream_capacity = 0; stream_bytes = 0; have_records = false;
  }
  void release() {
    dev.free_all();
    if (log_stage) (void)hipFree(log_stage);
    log_stage = nullptr; log_capacity = 0; capacity = 0;
    release_records();
  }
};

void workspace_free(void *p) {
  Workspace *w = (Workspace *)p;
  w->release();
  delete w;
}

Workspace *workspace_of(oakgpu_forest *f) {
  Workspace *w = (Workspace *)oakgpu_forest_match_attachment(f);
  if (!w) {
    w = new Workspace();
    oakgpu_forest_set_match_attachment(f, w, workspace_free);
  }
  return w;
}

// recording's per-game arrays for n games and the two logs' first size
int records_for(Workspace *w, hipStream_t stream, uint32_t n) {
  if (w->rec_capacity < n) {
    HIPCHK(hipStreamSynchronize(stream));
    DeviceArrays &d = w->rec_dev;
    d.free_all();
    w->rec_capacity = 0;
    RC(d.get(w->cursor, n)); RC(d.get(w->length, n)); RC(d.get(w->keep, n)); RC(d.get(w->offsets, (size_t)n + 1));
    w->rec_capacity = n;
  }
  if (!w->rlog[0]) {
    for (int s = 0; s < 2; ++s) RC(dev_alloc(w->rlog[s], first_log_capacity(n)));
    w->rlog_capacity = first_log_capacity(n);
  }
  return 0;
}

int workspace_for(oakgpu_forest *f, uint32_t n, Workspace **out) {
  Workspace *w = workspace_of(f);
  *out = w;
  if (w->capacity >= n) return 0;
  HIPCHK(hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(oakgpu_forest_ctx(f))));
  DeviceArrays &d = w->dev;
  d.free_all();
  w->capacity = 0;
  const size_t T = n, blocks = (T + BLOCK - 1) / BLOCK;
  for (int h = 0; h < 2; ++h) {
    Rows &r = w->half[h];
    RC(d.get(r.battles, T * 384)); RC(d.get(r.durations, T * 8)); RC(d.get(r.results, T)); RC(d.get(r.m, T)); RC(d.get(r.n, T)); RC(d.get(r.c1, T));
    RC(d.get(r.c2, T)); RC(d.get(r.flag, T)); RC(d.get(r.s1, T)); RC(d.get(r.s2, T)); RC(d.get(r.game, T)); RC(d.get(r.turns, T)); RC(d.get(r.rng, T));
    RC(d.get(r.ev1, T)); RC(d.get(r.ev2, T));
  }
  RC(d.get(w->ch1, T * 9)); RC(d.get(w->cnt1, T)); RC(d.get(w->ch2, T * 9)); RC(d.get(w->cnt2, T));
  for (int s = 0; s < 2; ++s) {
    RC(d.get(w->list[s], T)); RC(d.get(w->seed[s], T)); RC(d.get(w->out_block[s], OUT_BYTES * T + 16 * 16)); RC(d.get(w->nash[s], T * 19));
  }
  RC(d.get(w->gb, T * 384)); RC(d.get(w->gd, T * 8)); RC(d.get(w->gr, T)); RC(d.get(w->pay, T * PAY_STRIDE));
  RC(d.get(w->results_out, T)); RC(d.get(w->status_out, T)); RC(d.get(w->turns_out, T)); RC(d.get(w->block_live, blocks)); RC(d.get(w->block_offset, blocks));
  RC(d.get(w->ctl, 4)); RC(d.get(w->counts, 4));
  RC(d.get(w->in_b, T * 384)); RC(d.get(w->in_d, T * 8)); RC(d.get(w->in_r, T)); RC(d.get(w->in_seeds, T));
  w->capacity = n;
  return 0;
}

int fail_seat(const char *seat, const std::string &what) { return oakgpu_fail_msg((std::string("oakgpu_forest_match: seat ") + seat + ": " + what).c_str()); }

int check_seat(const char *name, const oakgpu_match_seat &s, uint32_t max_trees, uint32_t max_iterations, int contextual, uint32_t n, int solve_nash) {
  const std::string refusal = policy_refusal(s.policy_mode, sizeof s.policy_mode, s.policy_min, solve_nash);
  if (!refusal.empty()) return fail_seat(name, refusal);
  if (int rc = oakgpu_forest_check(max_trees, max_iterations, contextual, &s.search, s.net != nullptr, n, nullptr, 0, 0)) {
    std::string msg = oakgpu_last_error();
    const std::string from = "oakgpu_forest_search:";
    if (msg.compare(0, from.size(), from) == 0) msg = msg.substr(from.size());
    fail_seat(name, "the forest search refuses:" + msg);
    return rc;
  }
  return 0;
}

} // namespace

extern "C" {

int oakgpu_forest_match_check(uint32_t max_trees, uint32_t max_iterations, int contextual, const oakgpu_forest_match_params *prm, uint32_t n) {
  if (!prm) return oakgpu_fail_msg("oakgpu_forest_match: null argument");
  if (!(prm->early_stop >= 0.0)) return oakgpu_fail_msg("oakgpu_forest_match: early_stop must be >= 0 (0 = off; the reference's default is 10)");
  if (n > max_trees) return oakgpu_fail_msg("oakgpu_forest_match: n exceeds the forest's max_trees");
  RC(check_seat("p1", prm->p1, max_trees, max_iterations, contextual, n, prm->solve_nash));
  RC(check_seat("p2", prm->p2, max_trees, max_iterations, contextual, n, prm->solve_nash));
  return 0;
}

int oakgpu_forest_match_dev(oakgpu_forest *f, const oakgpu_forest_match_params *prm, const uint8_t *battles, const uint8_t *durations, const uint8_t *results_in,
                            const uint64_t *seeds, uint32_t n, uint8_t *results_out, uint32_t *turns_out, uint8_t *status_out, oakgpu_match_turn *turn_log,
                            uint64_t counts_out[4]) {
  if (!f || !prm) return oakgpu_fail_msg("oakgpu_forest_match: null argument");
  uint32_t max_trees = 0, max_iterations = 0;
  int contextual = 0;
  oakgpu_forest_limits(f, &max_trees, &max_iterations, &contextual);
  RC(oakgpu_forest_match_check(max_trees, max_iterations, contextual, prm, n));
  if (n && (!battles || !durations || !results_in || !seeds)) return oakgpu_fail_msg("oakgpu_forest_match: null argument");
  if (((uintptr_t)battles & 15) != 0) return oakgpu_fail_msg("oakgpu_forest_match: battles must be 16-byte aligned");
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  Workspace *w = nullptr;
  RC(workspace_for(f, std::max(n, 1u), &w));
  w->stats[0] = w->stats[1] = w->stats[2] = w->stats[3] = 0;
  if (counts_out) counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
  const bool recording = w->records_on;
  w->have_records = false;
  w->last_n = n;
  w->stream_bytes = 0;
  if (n == 0) { w->have_records = recording; return 0; }
  const oakgpu_match_seat *seat[2] = {&prm->p1, &prm->p2};
  oak_pick::PolicyMode mode[2];
  oakgpu_search_params sp[2];
  for (int s = 0; s < 2; ++s) {
    (void)oak_pick::parse_policy_mode(seat[s]->policy_mode, sizeof seat[s]->policy_mode, &mode[s]);
    sp[s] = seat[s]->search;
    sp[s].batch = 1; sp[s].seed = 0;
  }
  const uint32_t max_turns = prm->max_turns ? prm->max_turns : 1000;
  const uint32_t log_turns = turn_log ? prm->log_turns : 0;
  auto grid = [](size_t items) { return dim3((uint32_t)((items + BLOCK - 1) / BLOCK)); };

  int cur = 0;
  uint32_t rows = n;
  {
    Rows &r = w->half[0];
    HIPCHK(hipMemcpyAsync(r.battles, battles, (size_t)n * 384, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(r.durations, durations, (size_t)n * 8, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(r.results, results_in, n, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemsetAsync(w->counts, 0, 4 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(k_fm_start, grid(n), dim3(BLOCK), 0, stream, r, seeds, n);
    HIPCHK(hipGetLastError());
  }
  size_t entries = 0; // recording: entries in each seat's log
  if (recording) {
    RC(records_for(w, stream, n));
    HIPCHK(hipMemsetAsync(w->cursor, 0, (size_t)n * 4, stream));
  }
  for (uint64_t turn = 0;; ++turn) {
    // both sides' legal choices over the resident rows (finished ones included: their states are whole), retire what ended, compact the
    // rest, the prelude: the host's one read of the turn
    {
      Rows &r = w->half[cur];
      RC(oakgpu_choices_dev(ctx, r.battles, r.results, 0, w->ch1, w->cnt1, rows));
      RC(oakgpu_choices_dev(ctx, r.battles, r.results, 1, w->ch2, w->cnt2, rows));
    }
    const uint32_t blocks = (rows + BLOCK - 1) / BLOCK;
    const RetireArgs ra{w->half[cur], w->results_out, w->status_out, w->turns_out, w->counts, w->block_live, rows, max_turns};
    hipLaunchKernelGGL(k_fm_retire, grid(rows), dim3(BLOCK), 0, stream, ra);
    hipLaunchKernelGGL(k_rows_offsets, dim3(1), dim3(1024), 0, stream, w->block_live, blocks, w->block_offset, w->ctl);
    const CompactArgs ca{w->half[cur], w->half[cur ^ 1], w->block_offset, w->ch1, w->cnt1, w->ch2, w->cnt2, rows};
    hipLaunchKernelGGL(k_fm_compact, grid(rows), dim3(BLOCK), 0, stream, ca);
    cur ^= 1;
    Rows &r = w->half[cur];
    const PreludeArgs pa{r, w->ctl, w->list[0], w->list[1], w->seed[0], w->seed[1], rows};
    hipLaunchKernelGGL(k_fm_prelude, dim3(1), dim3(1024), 0, stream, pa);
    HIPCHK(hipGetLastError());
    uint32_t rec[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(rec, w->ctl, 12, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    ++w->stats[3];
    if (rec[0] > rows || rec[1] > rec[0] || rec[2] > rec[0]) return oakgpu_fail_msg("oakgpu_forest_match: the live count grew (internal error)");
    rows = rec[0];
    if (rows == 0) break;
    if (turn > (uint64_t)max_turns + 1) return oakgpu_fail_msg("oakgpu_forest_match: a game outlived max_turns (internal error)");
    ++w->stats[0];
    w->stats[1] += rec[1];
    w->stats[2] += rec[2];
    if (recording && entries + rows > w->rlog_capacity) { // the logs follow the turns played: doubled between turns
      const size_t want = std::max(w->rlog_capacity * 2, entries + rows);
      HIPCHK(hipStreamSynchronize(stream));
      for (int s = 0; s < 2; ++s) RC(grow_log(w->rlog[s], entries, want, stream));
      w->rlog_capacity = want;
    }
    for (int s = 0; s < 2; ++s) {
      const uint32_t count = rec[1 + s];
      if (count == 0) continue; // (no row of this seat has a choice to make: no search)
      const GatherArgs ga{r, w->list[s], w->gb, w->gd, w->gr, count};
      hipLaunchKernelGGL(k_fm_gather, grid((size_t)count * 24), dim3(BLOCK), 0, stream, ga);
      HIPCHK(hipGetLastError());
      oakgpu_forest_outputs o;
      carve_outputs(w->out_block[s], count, &o);
      RC(oakgpu_forest_search_dev(f, seat[s]->net, &sp[s], w->gb, w->gd, w->gr, w->seed[s], count, &o, nullptr, 0));
      const double *d_nash = nullptr;
      if (prm->solve_nash) {
        RC(solve_turn(ctx, stream, prm->solve_nash, o, count, w->pay, w->nash[s], w->h_pay, w->h_nash));
        if (prm->solve_nash == 1) HIPCHK(hipStreamSynchronize(stream)); // (the strategies' host copy is reused by the other seat)
        d_nash = w->nash[s] + (s ? (size_t)count * 9 : 0);
      }
      PickArgs pk{};
      pk.r = r; pk.list = w->list[s]; pk.out = o; pk.nash = d_nash; pk.mode = mode[s];
      pk.temp = seat[s]->policy_temp > 0 ? seat[s]->policy_temp : 1.0; pk.minp = seat[s]->policy_min; pk.early_stop = prm->early_stop;
      pk.count = count; pk.side = s;
      if (recording) {
        pk.rlog = w->rlog[s] + entries; pk.nash_all = prm->solve_nash ? w->nash[s] : nullptr;
        hipLaunchKernelGGL(k_fm_pick<true>, grid(count), dim3(BLOCK), 0, stream, pk);
      } else hipLaunchKernelGGL(k_fm_pick<false>, grid(count), dim3(BLOCK), 0, stream, pk);
      HIPCHK(hipGetLastError());
    }
    if (recording) {
      const FinishArgs fa{r, turn_log, rows, log_turns, w->rlog[0] + entries, w->rlog[1] + entries, w->cursor};
      hipLaunchKernelGGL(k_fm_finish<true>, grid(rows), dim3(BLOCK), 0, stream, fa);
      entries += rows;
    } else {
      const FinishArgs fa{r, turn_log, rows, log_turns, nullptr, nullptr, nullptr};
      hipLaunchKernelGGL(k_fm_finish<false>, grid(rows), dim3(BLOCK), 0, stream, fa);
    }
    HIPCHK(hipGetLastError());
    // PKMN::update(battle, c1, c2, options); durations <- options (vs.cc:312-318).  A row that stopped in this turn takes a legal step too
    // and is retired by its flag.
    RC(oakgpu_update_dev(ctx, r.battles, r.c1, r.c2, r.durations, nullptr, nullptr, rows, r.results));
  }
  if (results_out) HIPCHK(hipMemcpyAsync(results_out, w->results_out, n, hipMemcpyDeviceToDevice, stream));
  if (turns_out) HIPCHK(hipMemcpyAsync(turns_out, w->turns_out, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
  if (status_out) HIPCHK(hipMemcpyAsync(status_out, w->status_out, n, hipMemcpyDeviceToDevice, stream));
  unsigned long long counts[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(counts, w->counts, sizeof counts, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (counts_out) for (int q = 0; q < 4; ++q) counts_out[q] = counts[q];
  if (recording) { // pack: the record lengths and their bases in game order, then per seat the heads and the log's updates
    if (entries > 0xFFFFFFFFull) return oakgpu_fail_msg("oakgpu_forest_match: more than 2^32 turns in one call");
    hipLaunchKernelGGL(k_fm_record_lengths, grid(n), dim3(BLOCK), 0, stream, w->status_out, w->cursor, w->length, w->keep, n);
    size_t total = 0;
    RC(record_bases(stream, w->length, n, w->offsets, w->stream, 2, &w->stream_capacity, &total));
    if (total)
      for (int s = 0; s < 2; ++s) // the stored battle is the game's input battle
        RC(pack_records(stream, PackArgs{w->offsets, w->turns_out, w->length, w->results_out, w->keep, battles, w->rlog[s], w->stream[s], n, (uint32_t)entries}));
    HIPCHK(hipStreamSynchronize(stream));
    w->stream_bytes = total;
    w->have_records = true;
  }
  return 0;
}

int oakgpu_forest_match(oakgpu_forest *f, const oakgpu_forest_match_params *prm, const uint8_t *battles, const uint8_t *durations, const uint8_t *results_in,
                        const uint64_t *seeds, uint32_t n, uint8_t *results_out, uint32_t *turns_out, uint8_t *status_out, oakgpu_match_turn *turn_log,
                        uint64_t counts_out[4]) {
  if (!f || !prm || (n && (!battles || !durations || !results_in || !seeds))) return oakgpu_fail_msg("oakgpu_forest_match: null argument");
  uint32_t max_trees = 0, max_iterations = 0;
  int contextual = 0;
  oakgpu_forest_limits(f, &max_trees, &max_iterations, &contextual);
  RC(oakgpu_forest_match_check(max_trees, max_iterations, contextual, prm, n));
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  Workspace *w = nullptr;
  RC(workspace_for(f, std::max(n, 1u), &w));
  const size_t log_records = turn_log ? (size_t)n * prm->log_turns : 0;
  if (log_records > w->log_capacity) {
    HIPCHK(hipStreamSynchronize(stream));
    if (w->log_stage) (void)hipFree(w->log_stage);
    w->log_stage = nullptr; w->log_capacity = 0;
    RC(dev_alloc(w->log_stage, log_records));
    w->log_capacity = log_records;
  }
  if (n) {
    HIPCHK(hipMemcpyAsync(w->in_b, battles, (size_t)n * 384, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(w->in_d, durations, (size_t)n * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(w->in_r, results_in, n, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(w->in_seeds, seeds, (size_t)n * 8, hipMemcpyHostToDevice, stream));
    if (log_records) HIPCHK(hipMemcpyAsync(w->log_stage, turn_log, log_records * sizeof(oakgpu_match_turn), hipMemcpyHostToDevice, stream)); // (entries no game reaches stay the caller's)
    HIPCHK(hipStreamSynchronize(stream));
  }
  RC(oakgpu_forest_match_dev(f, prm, w->in_b, w->in_d, w->in_r, w->in_seeds, n, nullptr, nullptr, nullptr, log_records ? w->log_stage : nullptr, counts_out));
  if (n) {
    if (results_out) HIPCHK(hipMemcpyAsync(results_out, w->results_out, n, hipMemcpyDeviceToHost, stream));
    if (turns_out) HIPCHK(hipMemcpyAsync(turns_out, w->turns_out, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    if (status_out) HIPCHK(hipMemcpyAsync(status_out, w->status_out, n, hipMemcpyDeviceToHost, stream));
    if (log_records) HIPCHK(hipMemcpyAsync(turn_log, w->log_stage, log_records * sizeof(oakgpu_match_turn), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  return 0;
}

int oakgpu_forest_match_last_stats(const oakgpu_forest *f, uint64_t out[4]) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_match_last_stats: null argument");
  const Workspace *w = (const Workspace *)oakgpu_forest_match_attachment(f);
  for (int q = 0; q < 4; ++q) out[q] = w ? w->stats[q] : 0;
  return 0;
}

int oakgpu_forest_match_set_records(oakgpu_forest *f, int on) {
  if (!f) return oakgpu_fail_msg("oakgpu_forest_match_set_records: null argument");
  if (on != 0 && on != 1) return oakgpu_fail_msg("oakgpu_forest_match_set_records: on must be 0 or 1");
  workspace_of(f)->records_on = on != 0;
  return 0;
}

int oakgpu_forest_match_records(oakgpu_forest *f, int seat, uint8_t *stream_out, size_t capacity, size_t *bytes, uint64_t *offsets, uint32_t *n_frames,
                                uint8_t *results, uint8_t *status, int to_device) {
  if (!f) return oakgpu_fail_msg("oakgpu_forest_match_records: null argument");
  if (seat != 0 && seat != 1) return oakgpu_fail_msg("oakgpu_forest_match_records: seat must be 0 (p1) or 1 (p2)");
  Workspace *w = (Workspace *)oakgpu_forest_match_attachment(f);
  if (!w || !w->have_records)
    return oakgpu_fail_msg("oakgpu_forest_match_records: the forest holds no finished match call made with recording on (oakgpu_forest_match_set_records)");
  if (bytes) *bytes = w->stream_bytes;
  if (stream_out && capacity < w->stream_bytes) return oakgpu_fail_msg("oakgpu_forest_match_records: buffer too small");
  oakgpu_ctx *ctx = oakgpu_forest_ctx(f);
  RC(oakgpu_ctx_enter(ctx));
  const Records held{w->stream[seat], w->stream_bytes, w->offsets, w->turns_out, w->results_out, w->status_out, w->last_n};
  return copy_records((hipStream_t)oakgpu_ctx_stream(ctx), held, stream_out, offsets, n_frames, results, status, to_device);
}

int oakgpu_match_pick_host(int side, uint32_t m, uint32_t n, const uint64_t *visit_matrix, const double *value_matrix, uint64_t iterations, const double *nash,
                           const double *prior, const char *policy_mode, double policy_temp, double policy_min, double early_stop, uint64_t *rng, double *policy,
                           int32_t *index, double *empirical_value, int32_t *sign) {
  if (!visit_matrix || !value_matrix || !rng || !policy || !index || !empirical_value || !sign) return oakgpu_fail_msg("oakgpu_match_pick_host: null argument");
  if (side < 0 || side > 1 || m < 1 || m > 9 || n < 1 || n > 9) return oakgpu_fail_msg("oakgpu_match_pick_host: side must be 0 or 1, m and n in 1..9");
  if (!(early_stop >= 0.0)) return oakgpu_fail_msg("oakgpu_match_pick_host: early_stop must be >= 0");
  oak_pick::PolicyMode mode;
  if (oak_pick::parse_policy_mode(policy_mode, policy_mode ? strlen(policy_mode) : 0, &mode) != 0)
    return oakgpu_fail_msg("oakgpu_match_pick_host: policy mode must be built from e / n / x / p words, 8 at the most (util/policy.h:22-98)");
  uint64_t state = *rng;
  int idx = 0;
  double ev = 0, e1[9], e2[9];
  if (!seat_pick(side, visit_matrix, value_matrix, (int)m, (int)n, iterations, nash, prior, mode, policy_temp > 0 ? policy_temp : 1.0, policy_min, state, policy, &idx, &ev,
                 e1, e2))
    return oakgpu_fail_msg("oakgpu_match_pick_host: RuntimePolicy: zero policy (the minimum-probability cut left nothing)");
  *rng = state;
  *index = idx;
  *empirical_value = ev;
  *sign = early_stop_sign(ev, early_stop);
  return 0;
}

} // extern "C"
