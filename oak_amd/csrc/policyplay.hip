// oak_amd/csrc/policyplay.hip -- batches of whole games between two policies, resident on the device (the contract is in
// include/oakgpu.h; the reference's per-game form is `vs --budget=0 --bandit=pucb-1.0 --policy-mode=p`, cpp/src/vs.cc:107-408).
//
//   k_games_start   : row i is game i at turn 0; the control words
//   k_policy_pick   : one lane per row: the joint choice of this turn from the two seats' rules, the row's draws, the choice log
//   k_games_retire  : one lane per row: a finished row's outputs go to the caller's arrays by game index, the counters, the live count,
//                     and how many rows of each block are still live
//   k_rows_offsets  : (game_rows.hpp) one workgroup: the exclusive prefix sums of those per-block counts
//   k_games_compact : the live rows, in order, into the other half of the double buffer
// The scan, the place of a live row, the move of the battles and the count of a block's live rows are game_rows.hpp's, shared with the two
// loops over the forest search.  Every kernel is a plain grid over rows (k_rows_offsets: one workgroup); none waits for another block.
// The turn in between is oakgpu_tree_step_dev and oakgpu_leaf_eval_policy_dev over the resident rows.  A finished row is frozen -- pick
// draws nothing for it, the tree step leaves it alone -- so it can be retired at any later turn: the host retires and reads the live
// count every `poll` turns only.  There is no CPU fallback in this library.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>

#include "../../include/oakgpu.h"
#include "fast_prng.hpp"
#include "game_rows.hpp"
#include "oakgpu_internal.h"

namespace oak {
namespace pg {

using game_rows::BLOCK;
using game_rows::DEAD;
using game_rows::k_rows_offsets;
using game_rows::NO_ROW;
using game_rows::u32x4;
constexpr uint32_t FLAGGED = 0xFFu;      // result byte of a game whose policy was all zero
enum : uint32_t { T_WIN = 1, T_LOSE = 2 }; // pkmn_result types (gen1_device.hpp's R_WIN / R_LOSE)

// the control words: [0] live rows, [1] flagged games, [2] the lowest flagged game index; counters at byte 32
struct Control { uint32_t live, flagged, first_flagged, pad[5]; unsigned long long counts[4]; };

// one half of the double buffer (a row is its battle, durations, result byte, PRNG state, game index, turn count -- and, between pick and
// the tree step, its joint choice)
struct Rows {
  uint8_t *battles, *durations, *results, *prng, *c1, *c2;
  uint32_t *game, *turns;
};

__global__ __launch_bounds__(BLOCK) void k_games_start(uint32_t *game, uint32_t *turns, uint32_t n, Control *ctl) {
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  if (row == 0) {
    ctl->live = n; ctl->flagged = 0; ctl->first_flagged = DEAD;
    ctl->counts[0] = ctl->counts[1] = ctl->counts[2] = ctl->counts[3] = 0;
  }
  if (row >= n) return;
  game[row] = row;
  turns[row] = 0;
}

// ---- pick --------------------------------------------------------------------------------------------------------------------------
struct SeatDev { int32_t kind; double temp, min; };
struct PickArgs {
  Rows r;
  const uint8_t *ch1, *cnt1, *ch2, *cnt2; // rows x 9, rows: the legal choices of the state (oakgpu_choices_dev / the tree step)
  const float *l1, *l2;                   // rows x 9: seat p1's network's p1 logits, seat p2's network's p2 logits
  uint8_t *log;                           // nullable
  SeatDev s1, s2;
  uint32_t rows, max_turns, log_turns;
};

__device__ __forceinline__ uint32_t mod64(uint32_t hi, uint32_t lo, uint32_t m) { // (hi << 32 | lo) % m for m < 2^16, in 32-bit steps
  uint32_t r = hi % m;
  r = ((r << 16) | (lo >> 16)) % m;
  return ((r << 16) | (lo & 0xFFFFu)) % m;
}

// RuntimePolicy mode "p" at budget 0 (util/policy.h:22-106) over the k legal logits, then fast_prng::sample_pdf (util/random.h:123-132) of
// the draw u.  -1: every entry fell below `min`.
__device__ __forceinline__ int sample_policy(const float *logit, uint32_t k, double temp, double minp, double u) {
  float ex[OAKGPU_MAX_CHOICES], fsum = 0.0f; // softmax(prior, logits, k): search/util/softmax.h:5-15 -- expf, the sum in fp32 in index order ...
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) {
    ex[i] = i < k ? expf(logit[i]) : 0.0f;
    if (i < k) fsum = __fadd_rn(fsum, ex[i]);
  }
  double p[OAKGPU_MAX_CHOICES]; // ... and the quotient in the prior's own type, double
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) p[i] = i < k ? (double)ex[i] / (double)fsum : 0.0;
  if (temp != 1.0) {
    double sum = 0.0;
#pragma unroll
    for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) { p[i] = i < k ? pow(p[i], temp) : 0.0; sum += p[i]; }
#pragma unroll
    for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) p[i] /= sum;
  }
  double sum = 0.0;
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) { if (p[i] < minp) p[i] = 0.0; sum += p[i]; }
  if (sum == 0.0) return -1;
  int index = 0;
  bool found = false;
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) {
    u -= p[i] / sum;
    if (!found && i < k && u <= 0.0) { index = (int)i; found = true; }
  }
  return index;
}

// one seat's index into its k legal choices (k >= 1); both-RANDOM games do not come here
__device__ __forceinline__ int seat_index(const SeatDev &s, FastPrng &g, const float *logit, uint32_t k) {
  if (s.kind == OAKGPU_SEAT_RANDOM) {
    const uint32_t hi = g.next32(), lo = g.next32(); // uniform_64 = hi << 32 | lo
    return (int)mod64(hi, lo, k);
  }
  if (k == 1) return 0; // (vs.cc:258,273: no search output is sampled for a forced move)
  const uint32_t hi = g.next32(), lo = g.next32();
  const double u = (double)(((((unsigned long long)hi) << 32) | lo) >> 11) * (1.0 / 9007199254740992.0); // uniform(): random.h:109-112
  return sample_policy(logit, k, s.temp, s.min, u);
}

__global__ __launch_bounds__(BLOCK) void k_policy_pick(PickArgs a) {
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  if (row >= a.rows) return;
  const uint32_t res = a.r.results[row], turn = a.r.turns[row];
  uint32_t c1 = 0xFF, c2 = 0xFF;
  if ((res & 15) == 0 && turn < a.max_turns) { // (a finished, flagged or stopped row is frozen)
    uint32_t *ps = (uint32_t *)a.r.prng + 2 * (size_t)row;
    FastPrng g;
    g.s0 = ps[0];
    g.s1 = ps[1];
    const uint32_t k1 = max((uint32_t)a.cnt1[row], 1u), k2 = max((uint32_t)a.cnt2[row], 1u);
    int i1, i2;
    if (a.s1.kind == OAKGPU_SEAT_RANDOM && a.s2.kind == OAKGPU_SEAT_RANDOM) { // the rollout kernels' rule: one draw for both (mcts.h:448-496)
      const uint32_t hi = g.next32(), lo = g.next32();
      i1 = (int)mod64(hi, lo, k1);
      i2 = (int)(hi % k2);
    } else {
      i1 = seat_index(a.s1, g, a.l1 + (size_t)row * OAKGPU_MAX_CHOICES, k1);
      i2 = seat_index(a.s2, g, a.l2 + (size_t)row * OAKGPU_MAX_CHOICES, k2);
    }
    ps[0] = g.s0;
    ps[1] = g.s1;
    if (i1 < 0 || i2 < 0) a.r.results[row] = (uint8_t)FLAGGED;
    else {
      c1 = a.ch1[(size_t)row * OAKGPU_MAX_CHOICES + i1];
      c2 = a.ch2[(size_t)row * OAKGPU_MAX_CHOICES + i2];
      if (a.log && turn < a.log_turns) {
        uint8_t *at = a.log + ((size_t)a.r.game[row] * a.log_turns + turn) * 2;
        at[0] = (uint8_t)c1;
        at[1] = (uint8_t)c2;
      }
      a.r.turns[row] = turn + 1;
    }
  }
  a.r.c1[row] = (uint8_t)c1;
  a.r.c2[row] = (uint8_t)c2;
}

// ---- retire ------------------------------------------------------------------------------------------------------------------------
struct RetireArgs {
  Rows r;
  uint8_t *results_out, *prng_out, *battles_out, *durations_out; // by game index; battles_out / durations_out nullable
  uint32_t *turns_out;
  float *values_out;
  Control *ctl;
  uint32_t *block_live; // per block of BLOCK rows: rows still live after this pass
  uint32_t rows, final; // final: every row that is still live is stopped (the turn cap)
};

__global__ __launch_bounds__(BLOCK) void k_games_retire(RetireArgs a) {
  __shared__ uint32_t wave_live[BLOCK / 64];
  const uint32_t tid = threadIdx.x, row = blockIdx.x * BLOCK + tid, lane = tid & 63;
  const bool in = row < a.rows;
  const uint32_t g = in ? a.r.game[row] : DEAD;
  const uint32_t res = in ? a.r.results[row] : 0;
  const uint32_t type = res & 15;
  const bool done = g != DEAD && (type != 0 || a.final);
  const bool flagged = done && res == FLAGGED;
  if (done) {
    a.results_out[g] = (uint8_t)res;
    a.turns_out[g] = a.r.turns[row];
    a.values_out[g] = flagged ? __builtin_nanf("") : type == T_WIN ? 1.0f : type == T_LOSE ? 0.0f : 0.5f; // mcts.h:481-495
    const uint32_t *ps = (const uint32_t *)a.r.prng + 2 * (size_t)row;
    uint32_t *pd = (uint32_t *)a.prng_out + 2 * (size_t)g;
    pd[0] = ps[0];
    pd[1] = ps[1];
    if (a.durations_out) {
      const uint32_t *ds = (const uint32_t *)a.r.durations + 2 * (size_t)row;
      uint32_t *dd = (uint32_t *)a.durations_out + 2 * (size_t)g;
      dd[0] = ds[0];
      dd[1] = ds[1];
    }
    if (a.battles_out) { // (once per game: the lane copies its own 384 bytes)
      const u32x4 *src = (const u32x4 *)a.r.battles + (size_t)row * 24;
      u32x4 *dst = (u32x4 *)a.battles_out + (size_t)g * 24;
#pragma unroll 4
      for (int w = 0; w < 24; ++w) dst[w] = src[w];
    }
    a.r.game[row] = DEAD;
    if (flagged) atomicMin(&a.ctl->first_flagged, g);
  }
  // wins, ties, losses, stopped: one atomic per wave and counter (a flagged game counts in none)
  const uint32_t cat = flagged ? 4u : type == 0 ? 3u : type == T_WIN ? 0u : type == T_LOSE ? 2u : 1u;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const unsigned long long m = __ballot(done && cat == k);
    if (lane == 0 && m) atomicAdd(&a.ctl->counts[k], (unsigned long long)__popcll(m));
  }
  const unsigned long long md = __ballot(done), mf = __ballot(flagged);
  if (lane == 0) {
    if (md) atomicSub(&a.ctl->live, (uint32_t)__popcll(md));
    if (mf) atomicAdd(&a.ctl->flagged, (uint32_t)__popcll(mf));
  }
  game_rows::count_block_live(g != DEAD && !done, wave_live, a.block_live);
}

// ---- compaction --------------------------------------------------------------------------------------------------------------------
struct CompactArgs {
  Rows from, to;
  const uint32_t *block_offset;
  uint32_t rows;
};

// Stable (game_rows.hpp: compact_place, compact_battles); a live row's own fields go with it.
__global__ __launch_bounds__(BLOCK) void k_games_compact(CompactArgs a) {
  __shared__ uint32_t wave_total[BLOCK / 64];
  __shared__ uint32_t place[BLOCK];
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = row < a.rows && a.from.game[row] != DEAD;
  const uint32_t to = game_rows::compact_place(live, a.block_offset[blockIdx.x], wave_total, place);
  if (live) {
    *((uint2 *)a.to.durations + to) = *((const uint2 *)a.from.durations + row);
    *((uint2 *)a.to.prng + to) = *((const uint2 *)a.from.prng + row);
    a.to.results[to] = a.from.results[row];
    a.to.c1[to] = a.from.c1[row];
    a.to.c2[to] = a.from.c2[row];
    a.to.game[to] = a.from.game[row];
    a.to.turns[to] = a.from.turns[row];
  }
  __syncthreads();
  game_rows::compact_battles(a.from.battles, a.to.battles, a.rows, place);
}

} // namespace pg
} // namespace oak

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {

using namespace oak::pg;

thread_local uint64_t g_stats[4] = {0, 0, 0, 0}; // oakgpu_policy_games_last_stats

struct Workspace {
  Rows half[2];
  uint8_t *ch1, *cnt1, *ch2, *cnt2, *actions;
  float *values, *l1, *l2, *unused; // `unused`: the other side's logits of a network that plays one seat only
  uint32_t *block_live, *block_offset;
  Control *ctl;
};

// the context's block, carved into 256-byte aligned arrays for n rows
int carve(oakgpu_ctx *c, uint32_t n, Workspace *w) {
  const size_t rows = n, blocks = (rows + BLOCK - 1) / BLOCK;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 255) & ~(size_t)255; return here; };
  size_t o_half[2][8];
  for (int h = 0; h < 2; ++h) {
    o_half[h][0] = take(rows * 384); o_half[h][1] = take(rows * 8); o_half[h][2] = take(rows); o_half[h][3] = take(rows * 8);
    o_half[h][4] = take(rows); o_half[h][5] = take(rows); o_half[h][6] = take(rows * 4); o_half[h][7] = take(rows * 4);
  }
  const size_t o_ch1 = take(rows * 9), o_cnt1 = take(rows), o_ch2 = take(rows * 9), o_cnt2 = take(rows), o_act = take(rows * 16);
  const size_t o_val = take(rows * 4), o_l1 = take(rows * 36), o_l2 = take(rows * 36), o_un = take(rows * 36);
  const size_t o_bl = take(blocks * 4), o_bo = take(blocks * 4), o_ctl = take(sizeof(Control));
  uint8_t *p = (uint8_t *)oakgpu_ctx_games_workspace(c, at);
  if (!p) return -1;
  for (int h = 0; h < 2; ++h)
    w->half[h] = Rows{p + o_half[h][0], p + o_half[h][1], p + o_half[h][2], p + o_half[h][3], p + o_half[h][4], p + o_half[h][5],
                      (uint32_t *)(p + o_half[h][6]), (uint32_t *)(p + o_half[h][7])};
  w->ch1 = p + o_ch1; w->cnt1 = p + o_cnt1; w->ch2 = p + o_ch2; w->cnt2 = p + o_cnt2; w->actions = p + o_act;
  w->values = (float *)(p + o_val); w->l1 = (float *)(p + o_l1); w->l2 = (float *)(p + o_l2); w->unused = (float *)(p + o_un);
  w->block_live = (uint32_t *)(p + o_bl); w->block_offset = (uint32_t *)(p + o_bo); w->ctl = (Control *)(p + o_ctl);
  return 0;
}

// everything that can be refused before anything is launched
int check(const char *who, oakgpu_ctx *c, const oakgpu_policy_games_params *p) {
  static thread_local char msg[200];
  auto fail = [&](const char *what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return oakgpu_fail_msg(msg); };
  if (!c) return fail("null ctx");
  if (!p) return fail("null params");
  const oakgpu_seat *seats[2] = {&p->p1, &p->p2};
  for (int s = 0; s < 2; ++s) {
    const oakgpu_seat &seat = *seats[s];
    if (seat.kind != OAKGPU_SEAT_RANDOM && seat.kind != OAKGPU_SEAT_POLICY) return fail(s ? "seat p2: unknown kind" : "seat p1: unknown kind");
    if (seat.kind != OAKGPU_SEAT_POLICY) continue;
    if (!seat.net) return fail(s ? "seat p2: a POLICY seat needs a network" : "seat p1: a POLICY seat needs a network");
    if (!(seat.temp >= 0.0)) return fail(s ? "seat p2: temp must not be negative" : "seat p1: temp must not be negative");
    if (!(seat.min <= 1.0)) // (every policy would be zeroed: RuntimePolicy's failure, known before the first turn)
      return fail(s ? "seat p2: RuntimePolicy: zero policy, mode: p (min above 1 zeroes every policy)" : "seat p1: RuntimePolicy: zero policy, mode: p (min above 1 zeroes every policy)");
    if (oakgpu_net_device(seat.net) != oakgpu_ctx_device(c))
      return fail(s ? "seat p2: the network was loaded on another device than the context's" : "seat p1: the network was loaded on another device than the context's");
  }
  return 0;
}

SeatDev seat_dev(const oakgpu_seat &s) { return SeatDev{s.kind, s.temp == 0.0 ? 1.0 : s.temp, s.min}; }

} // namespace

extern "C" {

int oakgpu_policy_games_dev(oakgpu_ctx *c, const oakgpu_policy_games_params *params, const uint8_t *battles, const uint8_t *durations,
                            const uint8_t *results_in, uint8_t *prng_state, uint32_t n, uint8_t *results_out, uint32_t *turns_out, float *values_out,
                            uint8_t *battles_out, uint8_t *durations_out, uint8_t *choice_log, uint64_t counts_out[4]) {
  const char *who = "oakgpu_policy_games_dev";
  if (int rc = check(who, c, params)) return rc;
  if (counts_out) counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
  g_stats[0] = g_stats[1] = g_stats[2] = g_stats[3] = 0;
  if (n == 0) return 0;
  if (!battles || !durations || !results_in || !prng_state || !results_out || !turns_out || !values_out)
    return oakgpu_fail_msg("oakgpu_policy_games_dev: null required pointer");
  if (((uintptr_t)battles_out & 15) || ((uintptr_t)durations_out & 3) || ((uintptr_t)prng_state & 3) || ((uintptr_t)turns_out & 3) || ((uintptr_t)values_out & 3))
    return oakgpu_fail_msg("oakgpu_policy_games_dev: misaligned array (battles_out: 16 bytes; durations_out, prng_state, turns_out, values_out: 4)");
  const uint32_t max_turns = params->max_turns ? params->max_turns : 1000, poll = params->poll ? params->poll : 16;
  const float compact_below = params->compact_below == 0.0f ? 0.5f : params->compact_below;
  const uint32_t log_turns = choice_log ? params->log_turns : 0;
  const oakgpu_seat &s1 = params->p1, &s2 = params->p2;
  const bool pol1 = s1.kind == OAKGPU_SEAT_POLICY, pol2 = s2.kind == OAKGPU_SEAT_POLICY, one_call = pol1 && pol2 && s1.net == s2.net;
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  Workspace w;
  if (int rc = carve(c, n, &w)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  auto grid = [](uint32_t rows) { return dim3((rows + BLOCK - 1) / BLOCK); };

  // turn 0: the caller's states, their legal choices
  int cur = 0;
  uint32_t rows = n;
  {
    Rows &r = w.half[0];
    HIPCHK(hipMemcpyAsync(r.battles, battles, (size_t)n * 384, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(r.durations, durations, (size_t)n * 8, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(r.results, results_in, (size_t)n, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(r.prng, prng_state, (size_t)n * 8, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(k_games_start, grid(n), dim3(BLOCK), 0, stream, r.game, r.turns, n, w.ctl);
    if (int rc = oakgpu_choices_dev(c, r.battles, r.results, 0, w.ch1, w.cnt1, n)) return rc;
    if (int rc = oakgpu_choices_dev(c, r.battles, r.results, 1, w.ch2, w.cnt2, n)) return rc;
  }
  for (uint32_t turn = 0;; ++turn) {
    Rows &r = w.half[cur];
    const bool last = turn == max_turns;
    if (!last) {
      if (pol1)
        if (int rc = oakgpu_leaf_eval_policy_dev(c, s1.net, r.battles, r.durations, rows, w.ch1, w.cnt1, w.ch2, w.cnt2, w.values, w.l1, one_call ? w.l2 : w.unused)) return rc;
      if (pol2 && !one_call)
        if (int rc = oakgpu_leaf_eval_policy_dev(c, s2.net, r.battles, r.durations, rows, w.ch1, w.cnt1, w.ch2, w.cnt2, w.values, w.unused, w.l2)) return rc;
      g_stats[0] += rows;
      ++g_stats[1];
      const PickArgs pa{r, w.ch1, w.cnt1, w.ch2, w.cnt2, w.l1, w.l2, choice_log, seat_dev(s1), seat_dev(s2), rows, max_turns, log_turns};
      hipLaunchKernelGGL(k_policy_pick, grid(rows), dim3(BLOCK), 0, stream, pa);
    }
    if (last || (turn + 1) % poll == 0) {
      const RetireArgs ra{r, results_out, prng_state, battles_out, durations_out, turns_out, values_out, w.ctl, w.block_live, rows, last ? 1u : 0u};
      hipLaunchKernelGGL(k_games_retire, grid(rows), dim3(BLOCK), 0, stream, ra);
      HIPCHK(hipGetLastError());
      uint32_t live = 0;
      HIPCHK(hipMemcpyAsync(&live, &w.ctl->live, 4, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      ++g_stats[3];
      if (live == 0 || last) break;
      if (live < rows && compact_below >= 0.0f && (float)live / (float)rows < compact_below) {
        const uint32_t blocks = (rows + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL(k_rows_offsets, dim3(1), dim3(1024), 0, stream, w.block_live, blocks, w.block_offset, (uint32_t *)nullptr);
        const CompactArgs ca{r, w.half[cur ^ 1], w.block_offset, rows};
        hipLaunchKernelGGL(k_games_compact, grid(rows), dim3(BLOCK), 0, stream, ca);
        cur ^= 1;
        rows = live;
        ++g_stats[2];
      }
    }
    Rows &now = w.half[cur];
    if (int rc = oakgpu_tree_step_dev(c, now.battles, now.durations, now.results, now.c1, now.c2, rows, 39, w.actions, w.ch1, w.cnt1, w.ch2, w.cnt2)) return rc;
  }
  Control end{};
  HIPCHK(hipMemcpyAsync(&end, w.ctl, sizeof end, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (counts_out) for (int k = 0; k < 4; ++k) counts_out[k] = end.counts[k];
  if (end.flagged) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "RuntimePolicy: zero policy, mode: p (game %u; %u game%s in all: values_out NaN, results_out 0xFF)", end.first_flagged, end.flagged,
             end.flagged == 1 ? "" : "s");
    return oakgpu_fail_msg(msg);
  }
  return 0;
}

int oakgpu_policy_games(oakgpu_ctx *c, const oakgpu_policy_games_params *params, const uint8_t *battles, const uint8_t *durations, const uint8_t *results_in,
                        uint8_t *prng_state, uint32_t n, uint8_t *results_out, uint32_t *turns_out, float *values_out, uint8_t *battles_out,
                        uint8_t *durations_out, uint8_t *choice_log, uint64_t counts_out[4]) {
  if (int rc = check("oakgpu_policy_games", c, params)) return rc;
  if (counts_out) counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
  if (n == 0) return 0;
  if (!battles || !durations || !results_in || !prng_state || !results_out || !turns_out || !values_out)
    return oakgpu_fail_msg("oakgpu_policy_games: null required pointer");
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  OakHostCall hc(c);
  const size_t rows = n, log_bytes = choice_log ? rows * params->log_turns * 2 : 0;
  // in: battles, durations, results, prng (in / out), the log (entries no game reaches keep the caller's bytes); out: the rest
  const size_t bytes[10] = {rows * 384, rows * 8, rows, rows * 8, log_bytes, rows, rows * 4, rows * 4, battles_out ? rows * 384 : 0, durations_out ? rows * 8 : 0};
  const void *in[5] = {battles, durations, results_in, prng_state, choice_log};
  void *out[10] = {nullptr, nullptr, nullptr, prng_state, choice_log, results_out, turns_out, values_out, battles_out, durations_out};
  void *dev[10] = {};
  for (int t = 0; t < 10; ++t)
    if (bytes[t] && !(dev[t] = hc.get(std::max<size_t>(bytes[t], 16)))) return -1;
  for (int t = 0; t < 5; ++t)
    if (bytes[t]) HIPCHK(hipMemcpyAsync(dev[t], in[t], bytes[t], hipMemcpyHostToDevice, stream));
  const int rc = oakgpu_policy_games_dev(c, params, (const uint8_t *)dev[0], (const uint8_t *)dev[1], (const uint8_t *)dev[2], (uint8_t *)dev[3], n, (uint8_t *)dev[5],
                                         (uint32_t *)dev[6], (float *)dev[7], (uint8_t *)dev[8], (uint8_t *)dev[9], (uint8_t *)dev[4], counts_out);
  // (a call that failed for a zero policy has written every game's outputs all the same: they travel back with the flagged ones marked)
  const bool ran = rc == 0 || strstr(oakgpu_last_error(), "zero policy") != nullptr;
  if (ran) {
    std::string keep = oakgpu_last_error();
    for (int t = 3; t < 10; ++t)
      if (bytes[t] && out[t]) HIPCHK(hipMemcpyAsync(out[t], dev[t], bytes[t], hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (rc) oakgpu_fail_msg(keep.c_str());
  }
  return rc;
}

int oakgpu_policy_games_last_stats(uint64_t out[4]) {
  if (!out) return oakgpu_fail_msg("oakgpu_policy_games_last_stats: null pointer");
  for (int k = 0; k < 4; ++k) out[k] = g_stats[k];
  return 0;
}

} // extern "C"
