// oak_amd/csrc/oakgpu.hip -- HIP kernels (gfx950) + the C ABI of include/oakgpu.h.
//
// K1  k_rollout_* : batched random playouts (replaces cpp/include/search/mcts.h:448-496 and
//                   the per-iteration prep of mcts.h:250-263): one lane per playout on the
//                   register-resident engine (gen1_regs.hpp), party slots and tables in LDS,
//                   choice RNG (fast_prng) and durations in registers.
//     k_update    : batched pkmn_gen1_battle_update (+ chance durations / actions / calc).
//     k_choices   : batched pkmn_gen1_battle_choices.
//     k_init      : batched PKMN::battle (cpp/include/libpkmn/init.h:90-154) + opening update.
//     k_random_ou : SURVEY 8(d) config-2 input generator (teams drawn on device).
// There is no CPU fallback in this library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/oakgpu.h"
#include "gen1_device.hpp"
#include "gen1_regs.hpp"
#include "record_walk.hpp"
#include "oakgpu_internal.h"
#include "fast_prng.hpp"

namespace oak {
using namespace walk; // the queue constants, cold_ptr_at and STAGE_STRIDE are record_walk.hpp's

constexpr int STATE_WORDS = 96; // 384-byte battle
constexpr int TABLE_LDS_PAD = TABLE_PAD; // (record_walk.hpp; this file's older name for it)

// The engine's tables (moves, species, type chart, boosts, reciprocals, effect descriptors, bit lists: 3.5 KB) as ONE image in exactly
// their LDS layout, built once per device by k_build_table_image (oakgpu_create).  A kernel's prologue is then a straight
// copy with all of a thread's loads in flight at once -- built table by table it was a dozen load -> wait -> store round
// trips plus four integer divisions per thread in front of every launch (~10 us of the 61 us a one-turn launch takes).
constexpr int TABLE_IMAGE_WORDS = TABLE_LDS_PAD / 4;
__device__ uint32_t g_table_image[TABLE_IMAGE_WORDS];

__global__ __launch_bounds__(64) void k_build_table_image() {
  extern __shared__ __align__(16) uint8_t smem[];
  for (int i = threadIdx.x; i < TABLE_IMAGE_WORDS; i += 64) ((lds_u32 *)smem)[i] = 0;
  __syncthreads();
  (void)stage_tables<true>((lds_u8 *)smem, OAK_MOVE_WORDS, OAK_MOVE_MAXPP, OAK_SPECIES_W0, OAK_SPECIES_W1, OAK_TYPE_CHART, OAK_BOOSTS);
  __syncthreads();
  for (int i = threadIdx.x; i < TABLE_IMAGE_WORDS; i += 64) g_table_image[i] = ((lds_u32 *)smem)[i];
}

// call with all threads of the workgroup, then barrier (the table area is 16-byte aligned in every kernel's LDS layout)
__device__ __forceinline__ Tables stage_default_tables(lds_u8 *lds) {
  constexpr int N4 = TABLE_IMAGE_WORDS / 4;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef OAK_LDS u32x4 lds_u128;
  const u32x4 *src = (const u32x4 *)g_table_image;
  lds_u128 *dst = (lds_u128 *)lds;
  for (int base = threadIdx.x; base < N4; base += 4 * (int)blockDim.x) {
    u32x4 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int i = base + u * (int)blockDim.x; t[u] = src[i < N4 ? i : N4 - 1]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int i = base + u * (int)blockDim.x; if (i < N4) dst[i] = t[u]; }
  }
  return tables_at(lds);
}

// ---- K1: random playouts -------------------------------------------------------------------
struct RolloutArgs {
  const uint8_t *battles;
  const uint8_t *durations;
  const uint8_t *results_in;
  uint8_t *prng;
  uint32_t n, max_steps;
  int prep;
  uint8_t *results_out;
  uint32_t *steps_out;
  float *values_out;
  uint8_t *battles_out;
  uint8_t *durations_out;
};

// ---- K1, one lane per playout and no queue (oakgpu_rollout_dev's contract).  LDS holds only
// the party slots (24 dwords per lane) + one table image per workgroup, so 8 waves fit on a CU.
template <int BLK>
__global__ __launch_bounds__(BLK, 2) void k_rollout_regs(RolloutArgs a) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<BLK, false>;
  Tables T = stage_default_tables((lds_u8 *)smem + ER::PARTY_WORDS * BLK * 4);
  __syncthreads();
  const uint32_t tid = threadIdx.x, lane = blockIdx.x * BLK + tid;
  if (lane >= a.n) return;
  const uint32_t *dsrc = (const uint32_t *)a.durations + 2 * (size_t)lane;
  FastPrng g;
  const uint32_t *psrc = (const uint32_t *)a.prng + 2 * (size_t)lane;
  g.s0 = psrc[0];
  g.s1 = psrc[1];
  ER e;
  e.m = party + tid;
  e.T = T;
  e.load_battle_global(a.battles + (size_t)lane * 384, dsrc[0], dsrc[1]);
  if (a.prep) { // mcts.h:254-259
    const uint32_t hi = g.next32(), lo = g.next32();
    e.rng = ((uint64_t)hi << 32) | lo;
    e.randomize_hidden();
  }
  uint32_t result = a.results_in[lane];
  uint32_t steps = 0;
  while ((result & 15) == 0 && steps < a.max_steps) {
    const uint32_t hi = g.next32(), lo = g.next32(); // uniform_64 = hi << 32 | lo
    result = e.random_step(result, hi, lo);
    ++steps;
  }
  e.normalize();
  a.results_out[lane] = (uint8_t)result;
  a.steps_out[lane] = steps;
  const uint32_t t = result & 15;
  a.values_out[lane] = t == R_WIN ? 1.0f : t == R_LOSE ? 0.0f : 0.5f;
  uint32_t *pdst = (uint32_t *)a.prng + 2 * (size_t)lane;
  pdst[0] = g.s0;
  pdst[1] = g.s1;
  if (a.durations_out) {
    uint32_t *ddst = (uint32_t *)a.durations_out + 2 * (size_t)lane;
    ddst[0] = e.S.dur;
    ddst[1] = e.F.dur;
  }
  if (a.battles_out) e.store_battle_global(a.battles_out + (size_t)lane * 384);
}

// The same, for launches of a FEW turn-steps over a resident batch (BASELINE configs[2]: one turn-step, then a leaf
// evaluation, every turn).  There the launch is all load / decode / encode / store: a lane reading its own 384-byte
// battle touches a 16-byte piece of 64 different lines per instruction, and writes it back the same way (45 us for a
// launch with ZERO steps; the HBM traffic is worth 12).  Here the wave moves its 64 battles (24 KB, contiguous) between
// global memory and LDS with fully coalesced 1 KB accesses, and the engine reads / writes the LDS copy through `gin`
// (a generic pointer: the flat loads resolve to LDS).
constexpr int STAGED_COLD_BYTES = 128; // the kernel arguments, parked (below)
constexpr int STAGED_LDS_BYTES = 24 * 64 * 4 + TABLE_LDS_PAD + 64 * STAGE_STRIDE * 4 + STAGED_COLD_BYTES;
// The staged kernels' LDS, in order: the engine's party slots, the tables, the wave's 64 staged rows, the parked arguments.
__device__ __forceinline__ lds_u32 *staged_rows(uint8_t *smem) { return (lds_u32 *)((lds_u8 *)smem + 24 * 64 * 4 + TABLE_LDS_PAD); }
// Pointer arguments are parked in LDS across the turn loop, like k_rollout_queue's cold arguments (read back with cold_ptr_at): as
// kernel arguments they held ~20 SGPRs the loop's nested exec masks need (54 spilled SGPRs, a v_writelane / v_readlane pair each, in
// a kernel that runs ONE turn-step per launch in BASELINE configs[2])
template <class Args>
__device__ __forceinline__ lds_u32 *park_args(lds_u32 *stage, const Args &a) {
  static_assert(sizeof(Args) <= STAGED_COLD_BYTES, "parked arguments fit");
  lds_u32 *cold = stage + 64 * STAGE_STRIDE;
  if (threadIdx.x < sizeof(Args) / 4) cold[threadIdx.x] = ((const uint32_t *)&a)[threadIdx.x];
  return cold;
}
// The wave's `cnt` battles, from battle `base` on, between global memory and the staged rows, 24 pieces per lane and trip: piece i is
// piece i % P of battle i / P.  DWORDS = false moves 16-byte pieces in one trip (battles 16-byte aligned); DWORDS = true moves dwords in
// four (all 96 in flight at once spilled the update kernels), for the entry points that take battles at any 4-byte boundary.  A barrier
// belongs behind stage_in and in front of stage_out.
template <bool DWORDS>
struct StagePiece {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef std::conditional_t<DWORDS, uint32_t, u32x4> type;
  static constexpr uint32_t P = 384 / sizeof(type), WORDS = sizeof(type) / 4; // pieces per battle, words per piece
};
template <bool DWORDS = false>
__device__ __forceinline__ void stage_in(lds_u32 *stage, const uint8_t *battles, uint32_t base, uint32_t cnt) {
  using SP = StagePiece<DWORDS>;
  typedef typename SP::type piece;
  const piece *src = (const piece *)(battles + (size_t)base * 384);
  const uint32_t tid = threadIdx.x;
#pragma unroll 1
  for (uint32_t q = 0; q < SP::P; q += 24) {
    piece t[24];
#pragma unroll
    for (uint32_t k = 0; k < 24; ++k) { const uint32_t i = (q + k) * 64 + tid; t[k] = src[i < cnt * SP::P ? i : 0]; }
#pragma unroll
    for (uint32_t k = 0; k < 24; ++k) { const uint32_t i = (q + k) * 64 + tid, b = i / SP::P, w = i - b * SP::P; *(OAK_LDS piece *)(stage + b * STAGE_STRIDE + SP::WORDS * w) = t[k]; }
  }
}
template <bool DWORDS = false>
__device__ __forceinline__ void stage_out(const lds_u32 *stage, uint8_t *battles, uint32_t base, uint32_t cnt) {
  using SP = StagePiece<DWORDS>;
  typedef typename SP::type piece;
  piece *dst = (piece *)(battles + (size_t)base * 384);
  const uint32_t tid = threadIdx.x;
  // (opaque: the bounds tests here are the ones of stage_in, and the compiler kept their 24 lane masks -- 48 SGPRs -- alive across the
  // whole turn loop to reuse them: 44 of k_rollout_staged's 46 spilled SGPRs)
  uint32_t cnt_out = cnt;
  asm volatile("" : "+s"(cnt_out));
#pragma unroll 1
  for (uint32_t q = 0; q < SP::P; q += 24) {
#pragma unroll
    for (uint32_t k = 0; k < 24; ++k) {
      const uint32_t i = (q + k) * 64 + tid, b = i / SP::P, w = i - b * SP::P;
      if (i < cnt_out * SP::P) dst[i] = *(const OAK_LDS piece *)(stage + b * STAGE_STRIDE + SP::WORDS * w);
    }
  }
}

__global__ __launch_bounds__(64, 2) void k_rollout_staged(RolloutArgs a) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<64, false, true>;
  Tables T = stage_default_tables((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4);
  lds_u32 *stage = staged_rows(smem);
  lds_u32 *cold = park_args(stage, a);
#define SA_PTR(field, type) cold_ptr_at<type>(cold, offsetof(RolloutArgs, field))
  const uint32_t tid = threadIdx.x, base = blockIdx.x * 64, lane = base + tid;
  const uint32_t cnt = a.n - base < 64 ? a.n - base : 64; // battles of this wave
  stage_in(stage, a.battles, base, cnt);
  __syncthreads();
  uint32_t result = 0, steps = 0;
  FastPrng g;
  g.s0 = g.s1 = 0;
  ER e;
  e.m = party + tid;
  e.T = T;
  const uint32_t n_all = (uint32_t)__builtin_amdgcn_readfirstlane((int)cold[offsetof(RolloutArgs, n) / 4]);
  const uint32_t max_steps = (uint32_t)__builtin_amdgcn_readfirstlane((int)cold[offsetof(RolloutArgs, max_steps) / 4]);
  if (lane < n_all) {
    const uint32_t *dsrc = SA_PTR(durations, const uint32_t *) + 2 * (size_t)lane;
    const uint32_t *psrc = SA_PTR(prng, const uint32_t *) + 2 * (size_t)lane;
    g.s0 = psrc[0];
    g.s1 = psrc[1];
    e.load_battle_global((const uint8_t *)(stage + tid * STAGE_STRIDE), dsrc[0], dsrc[1]);   // (the address space comes back inside: gin_t)
    if (cold[offsetof(RolloutArgs, prep) / 4]) { // mcts.h:254-259
      const uint32_t hi = g.next32(), lo = g.next32();
      e.rng = ((uint64_t)hi << 32) | lo;
      e.randomize_hidden();
    }
    result = SA_PTR(results_in, const uint8_t *)[lane];
    while ((result & 15) == 0 && steps < max_steps) {
      const uint32_t hi = g.next32(), lo = g.next32(); // uniform_64 = hi << 32 | lo
      result = e.random_step(result, hi, lo);
      ++steps;
    }
    e.normalize();
    SA_PTR(results_out, uint8_t *)[lane] = (uint8_t)result;
    SA_PTR(steps_out, uint32_t *)[lane] = steps;
    const uint32_t t = result & 15;
    SA_PTR(values_out, float *)[lane] = t == R_WIN ? 1.0f : t == R_LOSE ? 0.0f : 0.5f;
    uint32_t *pdst = SA_PTR(prng, uint32_t *) + 2 * (size_t)lane;
    pdst[0] = g.s0;
    pdst[1] = g.s1;
    uint32_t *dout = SA_PTR(durations_out, uint32_t *);
    if (dout) {
      uint32_t *ddst = dout + 2 * (size_t)lane;
      ddst[0] = e.S.dur;
      ddst[1] = e.F.dur;
    }
    if (SA_PTR(battles_out, uint8_t *)) e.store_battle_global((uint8_t *)(stage + tid * STAGE_STRIDE));
  }
  uint8_t *bout = SA_PTR(battles_out, uint8_t *);
  if (!bout) return;
  __syncthreads();
  stage_out(stage, bout, base, cnt);
#undef SA_PTR
}

// ---- K1 driven by a caller-supplied DRAW STREAM instead of per-lane fast_prng: lane i consumes
// draws[offsets[i]], draws[offsets[i] + 1], ... -- one u64 per device.uniform_64() call of the reference loop (with
// prep the first goes to battle.rng, mcts.h:255-257, then one per turn-step, mcts.h:452).  This is how a SHARED
// sequential generator (benchmark.cc:24: one std::mt19937 for every playout) is replayed on the device: the host
// generates the generator's output once, and playout i starts where playout i-1 stopped (oakgpu_rollout_shared_device).
// stride 0 for battles / durations / results_in = every lane starts from the same root state.  A lane that would
// read past the end of the stream stops there and reports used = 0xFFFFFFFF.
struct DrawArgs {
  const uint8_t *battles, *durations, *results_in;
  uint32_t battle_stride, dur_stride, res_stride; // bytes (384 / 8 / 1) or 0
  const uint64_t *draws;
  uint32_t n_draws;
  const uint32_t *offsets; // nullable: lane i starts at draw i
  uint32_t n, max_steps;
  int prep;
  uint8_t *results_out;   // every output below is nullable
  uint32_t *steps_out;
  float *values_out;
  uint8_t *battles_out, *durations_out;
  uint32_t *used_out;     // draws consumed by lane i
};
template <int BLK>
__global__ __launch_bounds__(BLK, 2) void k_rollout_draws(DrawArgs a) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<BLK, false>;
  Tables T = stage_default_tables((lds_u8 *)smem + ER::PARTY_WORDS * BLK * 4);
  __syncthreads();
  const uint32_t tid = threadIdx.x, lane = blockIdx.x * BLK + tid;
  if (lane >= a.n) return;
  const uint32_t *dsrc = (const uint32_t *)(a.durations + (size_t)lane * a.dur_stride);
  ER e;
  e.m = party + tid;
  e.T = T;
  e.load_battle_global(a.battles + (size_t)lane * a.battle_stride, dsrc[0], dsrc[1]);
  uint32_t pos = a.offsets ? a.offsets[lane] : lane;
  const uint32_t first = pos;
  bool over = false;
  if (a.prep) { // mcts.h:254-259
    if (pos < a.n_draws) { e.rng = a.draws[pos++]; e.randomize_hidden(); }
    else over = true;
  }
  uint32_t result = a.results_in[(size_t)lane * a.res_stride];
  uint32_t steps = 0;
  while (!over && (result & 15) == 0 && steps < a.max_steps) {
    if (pos >= a.n_draws) { over = true; break; }
    const uint64_t dr = a.draws[pos++];
    result = e.random_step(result, (uint32_t)(dr >> 32), (uint32_t)dr);
    ++steps;
  }
  e.normalize();
  if (a.used_out) a.used_out[lane] = over ? 0xFFFFFFFFu : pos - first;
  if (a.results_out) a.results_out[lane] = (uint8_t)result;
  if (a.steps_out) a.steps_out[lane] = steps;
  const uint32_t t = result & 15;
  if (a.values_out) a.values_out[lane] = t == R_WIN ? 1.0f : t == R_LOSE ? 0.0f : 0.5f;
  if (a.durations_out) {
    uint32_t *ddst = (uint32_t *)a.durations_out + 2 * (size_t)lane;
    ddst[0] = e.S.dur;
    ddst[1] = e.F.dur;
  }
  if (a.battles_out) e.store_battle_global(a.battles_out + (size_t)lane * 384);
}

// ---- K1 with lane refill: a persistent grid of `gridDim.x * BLK` lanes pulls playouts from an atomic
// queue.  A lane that finishes its playout immediately starts the next unassigned one (wave ballot ->
// one atomicAdd per wave -> prefix rank), so waves stay full instead of idling on their longest lane.
// Results are indexed by playout, each playout owns its RNG streams: output is identical to k_rollout*.
//
// Regrouping rounds.  Playout lengths have a long tail (mean ~100 turn-steps, 0.1% reach the 1000-step cap),
// so once the queue is dry every wave decays towards a single live lane that still pays a whole wave's issue
// slots.  With `suspend_below` > 0 a wave whose queue is dry and that is down to fewer live lanes than that
// SUSPENDS them: the full state goes to a per-playout scratch slot (the 384-byte battle image, durations,
// PRNG, result, step count), the playout indices are appended to `list_out`, and the wave exits.  The next
// launch (`list_in` = that list) packs the survivors 64 to a wave again.  The last round runs with
// suspend_below = 0.  Serialisation is the engine's own bit-exact load/store, so results do not change.
struct RoundArgs {
  const uint32_t *list_in;  // nullptr: round 0, playout k of the group
  const uint32_t *n_in;     // device count of list_in
  uint32_t *list_out;       // suspended playouts of this round
  uint32_t *count_out;
  uint8_t *sb;              // scratch: total x 384 battle images
  uint8_t *sd;              // scratch: total x 8 durations
  uint8_t *sres;            // scratch: total results
  uint32_t suspend_below;
  uint32_t *queue;          // this round's queue heads: QUEUE_HEADS counters, QUEUE_HEAD_STRIDE words apart
  uint32_t lanes;           // lanes of a wave that take playouts (0 / 64: all); a tail round runs a few playouts per wave
  const uint32_t *order;    // round 0, nullable: queue position -> playout (k_queue_order: the likely-long playouts first)
  // long-playout migration (below): control words {tail, head, bulk waves exited, error}, one list entry per donation
  uint32_t *adopt_ctl;
  uint64_t *adopt_list;     // tickets {playout + 1, epoch << 32}: written for THIS launch when the high word is `epoch` (no per-launch clearing)
  uint32_t epoch;           // the context's count of migrating launches, never 0
  uint32_t n_adopters;      // 0 = off; waves [0, n_adopters) adopt
  uint32_t long_steps;      // bits 0-15: a bulk wave donates a playout that is still running after this many turn-steps;
                            // bits 16-24: ... or whose actives' {slot, hp} have not changed for this many turn-steps (256: never)
  uint32_t no_skip;         // 1: a proven inert standstill is played turn by turn like everything else (oakgpu_set_standstill_skip: A/B)
  uint32_t *stats;          // words 44-45 of the context's control block: {playouts fast-forwarded, turn-steps skipped}
  uint32_t move_carry;      // 0..64 (oakgpu_set_move_carry): a turn's second action waits for the wave's next action pass unless this many lanes want it now
  uint32_t move_carry_dry;  // 0..64 (oakgpu_set_move_carry_dry): a dry bulk wave goes on carrying while at least this many of its lanes play; 0 = a dry wave never carries
};

// One launch drains a GROUP of independent batches (oakgpu_rollout_group_dev): the queue hands out GLOBAL playout
// indices 0 .. total-1, batch b owns [start_b, start_b + n_b).  A 20-batch group has ONE tail instead of twenty.
struct BatchDesc {
  const uint8_t *battles, *durations, *results_in;
  uint8_t *prng;
  uint8_t *results_out;
  uint32_t *steps_out;
  float *values_out;
  uint8_t *battles_out, *durations_out;
  uint32_t start, n;
};
constexpr int MAX_GROUP = 64;
struct GroupArgs {
  const BatchDesc *table; // device memory, `count` entries
  uint32_t count, total, max_steps;
  int prep;
};

// The kernel's pointer arguments are needed only when a lane is (re)filled or retired, but as kernel arguments
// they would sit in ~40 SGPRs for the whole turn loop, whose nested divergent control flow needs those SGPRs
// for exec masks (the overflow is spilled to VGPR lanes: v_writelane / v_readlane in the hot path).  So the cold
// arguments are parked in LDS once (with the batches' start offsets) and the cold paths read them back.
struct ColdArgs {
  GroupArgs g;
  RoundArgs q;
  uint32_t starts[MAX_GROUP];
};
constexpr int COLD_LDS_BYTES = (sizeof(ColdArgs) + 15) & ~15;
template <class P>
__device__ __forceinline__ P cold_ptr(const lds_u32 *cold, size_t byte_off) {
  return (P)((uint64_t)cold[byte_off / 4] | ((uint64_t)cold[byte_off / 4 + 1] << 32));
}
#define COLD_Q(field, type) cold_ptr<type>(cold, offsetof(ColdArgs, q) + offsetof(RoundArgs, field))
// batch of global playout idx: largest b with starts[b] <= idx (binary search over the LDS copy)
__device__ __forceinline__ const BatchDesc *find_batch(const lds_u32 *cold, uint32_t idx) {
  const uint32_t count = cold[(offsetof(ColdArgs, g) + offsetof(GroupArgs, count)) / 4];
  const lds_u32 *starts = cold + offsetof(ColdArgs, starts) / 4;
  uint32_t lo = 0, hi = count; // invariant: starts[lo] <= idx < starts[hi] (starts[count] = +inf)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (starts[mid] <= idx) lo = mid; else hi = mid;
  }
  return cold_ptr<const BatchDesc *>(cold, offsetof(ColdArgs, g) + offsetof(GroupArgs, table)) + lo;
}

#ifdef OAKGPU_TIMELINE
// profile build only (tools/timeline.py): per wave of the queue kernel {start, first dry refill, exit} on the
// 100 MHz wall clock + turn-steps executed
static __device__ unsigned long long g_timeline[5 * 16384];
#define OAK_TL(slot, v) do { const unsigned long long tl_v = (v); if (wl == 0 && blockIdx.x < 16384) g_timeline[5 * blockIdx.x + (slot)] = tl_v; } while (0)
#else
#define OAK_TL(slot, v)
#endif

// Queue order of a group launch: LONGEST-EXPECTED FIRST.  The launch ends with its longest playout, and the longest are the
// 0.1% that run into the step cap: stalemates -- a Rage-locked or PP-less (Struggle) attacker whose Normal-type hits cannot
// touch a Ghost, a frozen Ghost nobody can hurt.  Measured on the CPU oracle (3 x 65,536 random OU playouts, 183 capped):
// 99.5% of the capped playouts have a Ghost-type Pokemon on one of the two teams, against 22% of all playouts; the rest had a
// Ditto (with Ghosts and Dittos: 183 of 183, 29% of all playouts).  A playout
// that starts when the queue runs dry still has its 1,000 dependent turn-steps in front of it; one that started in the first
// fifth of the launch has most of them behind it.  So the playouts with a Ghost on either team go to the front of the queue
// (order[] filled from the front), the others behind them (filled from the back).  Pure scheduling: results are indexed by
// playout and never depend on it.
// A group launch's control words are cleared by the launch's own first small kernel, on the context's stream (they were two fills
// in front of every launch): words 0-62 of the control block but the pair at `keep` (word 63 is the sticky migration error word:
// never cleared here), and every round's queue heads.
constexpr uint32_t QUEUE_MAX_ROUNDS = 16;
__device__ __forceinline__ void clear_launch_words(uint32_t *ctl, uint32_t *heads, uint32_t keep, uint32_t tid, uint32_t threads) {
  for (uint32_t i = tid; i < 63; i += threads) if ((i & ~1u) != keep) ctl[i] = 0;
  for (uint32_t i = tid; i < QUEUE_MAX_ROUNDS * QUEUE_HEADS; i += threads) heads[i * QUEUE_HEAD_STRIDE] = 0;
}
__global__ __launch_bounds__(256) void k_clear_launch_words(uint32_t *ctl, uint32_t *heads) { clear_launch_words(ctl, heads, 64, threadIdx.x, 256); }

// Blocks of 256 threads, 1,024 playouts each (four per thread).  The kernel runs in front of a launch whose stream neighbour
// saturates the device: a block is placed when ALL its waves fit on one compute unit, and sixteen-wave blocks waited for a whole
// drained SIMD set while four waves fit wherever a few slots are free.  Block 0 also clears the launch's control words (above);
// the two counters in use (control words `pair`, `pair` + 1) were cleared by the PREVIOUS launch's kernel, which used the other pair.
constexpr uint32_t ORDER_BLOCK = 256, ORDER_PER_BLOCK = 1024;
__global__ __launch_bounds__(ORDER_BLOCK) void k_queue_order(GroupArgs g, uint32_t *order, uint32_t *ctl, uint32_t *heads, uint32_t pair) {
  constexpr uint32_t PER = ORDER_PER_BLOCK / ORDER_BLOCK, GROUPS = ORDER_PER_BLOCK / 64;
  __shared__ uint32_t starts[MAX_GROUP + 1];
  __shared__ uint32_t wave_s[GROUPS], wave_o[GROUPS], base_s, base_o;
  if (blockIdx.x == 0) clear_launch_words(ctl, heads, pair, threadIdx.x, ORDER_BLOCK);
  for (uint32_t i = threadIdx.x; i < g.count; i += ORDER_BLOCK) starts[i] = g.table[i].start;
  if (threadIdx.x == 0) starts[g.count] = 0xFFFFFFFFu;
  __syncthreads();
  const uint32_t wl = threadIdx.x & 63, wib = threadIdx.x >> 6;
  uint64_t ms[PER], mo[PER];
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) { // playout j * 256 + thread of the block's 1,024: every wave instruction reads 64 consecutive playouts
    const uint32_t idx = blockIdx.x * ORDER_PER_BLOCK + j * ORDER_BLOCK + threadIdx.x;
    bool suspect = false;
    if (idx < g.total) {
      uint32_t lo = 0, hi = g.count;
      while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (starts[mid] <= idx) lo = mid; else hi = mid; }
      const BatchDesc &bd = g.table[lo];
      const uint32_t *b = (const uint32_t *)(bd.battles + (size_t)(idx - bd.start) * 384);
      uint32_t w[12]; // the dword {status, species, types, level} of each of the 12 Pokemon: all twelve loads in flight together
#pragma unroll
      for (int k = 0; k < 12; ++k) w[k] = b[((k / 6) * SIDE_SZ + (k % 6) * PK_SZ + P_STATUS) / 4];
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const uint32_t sp = (w[k] >> 8) & 0xFF, ty = (w[k] >> 16) & 0xFF;
        suspect |= sp != 0 && ((ty & 15) == T_Ghost || (ty >> 4) == T_Ghost || sp == 132 /* Ditto: Transform into a stalemate */);
      }
    }
    ms[j] = __ballot(suspect);
    mo[j] = __ballot(idx < g.total && !suspect);
    if (wl == 0) { wave_s[j * (ORDER_BLOCK / 64) + wib] = (uint32_t)__popcll(ms[j]); wave_o[j * (ORDER_BLOCK / 64) + wib] = (uint32_t)__popcll(mo[j]); }
  }
  // one pair of atomics per 1,024 playouts (a pair per wave: 41,000 atomics on two addresses took longer than the loads)
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t ts = 0, to = 0;
    for (uint32_t q = 0; q < GROUPS; ++q) { const uint32_t a = wave_s[q], c = wave_o[q]; wave_s[q] = ts; wave_o[q] = to; ts += a; to += c; }
    base_s = ts ? atomicAdd(ctl + pair, ts) : 0;
    base_o = to ? atomicAdd(ctl + pair + 1, to) : 0;
  }
  __syncthreads();
  const uint64_t below = (1ull << wl) - 1;
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    const uint32_t idx = blockIdx.x * ORDER_PER_BLOCK + j * ORDER_BLOCK + threadIdx.x, grp = j * (ORDER_BLOCK / 64) + wib;
    if ((ms[j] >> wl) & 1) order[base_s + wave_s[grp] + (uint32_t)__popcll(ms[j] & below)] = idx;
    else if ((mo[j] >> wl) & 1) order[g.total - 1 - (base_o + wave_o[grp] + (uint32_t)__popcll(mo[j] & below))] = idx;
  }
}

#ifndef OAK_LONG_STEPS
#define OAK_LONG_STEPS 200
#endif
constexpr uint32_t LONG_STEPS = OAK_LONG_STEPS;
#ifndef OAK_PRIO_STILL
#define OAK_PRIO_STILL 24
#endif
constexpr uint32_t PRIO_STILL = OAK_PRIO_STILL;
// (REFILL_EVERY / REFILL_LANES, with their OAK_REFILL_* overrides, and QUEUE_HEADS / QUEUE_HEAD_STRIDE: record_walk.hpp)
// KEEP_DUR = false, the LEAN instantiation (round 32): for a group none of whose batches takes durations back.  The engine keeps no
// durations word (EngineR's KEEP_DUR): a batch's durations are read for the prep of a fresh playout only, the scratch durations
// `sd` are neither written nor read when a playout is donated, parked or resumed, and no durations_out is written.  The schedule --
// queue order, refill batching, migration, adopters, standstill skip, both carries -- is the same code.
// PREP = false (lean launches with prep = 0, the headline's): the instantiation without the prep code -- randomize_hidden takes `%` by
// run-time divisors, ~1,000 static VALU of cold code that such a launch never reaches (7,645 -> 6,290 instructions; 194.7 against
// 195.8 wave cycles per turn-step, profiles/r32_lean_rollout.json).
template <int BLK, int WPS, bool KEEP_DUR = true, bool PREP = true>
__global__ __launch_bounds__(BLK, WPS) void k_rollout_queue(GroupArgs g_in, RoundArgs q_in) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<BLK, false, false, KEEP_DUR>;
  Tables T = stage_default_tables((lds_u8 *)smem + ER::PARTY_WORDS * BLK * 4);
  lds_u32 *cold = (lds_u32 *)((lds_u8 *)smem + ER::PARTY_WORDS * BLK * 4 + TABLE_LDS_PAD);
  if (threadIdx.x == 0) {
    struct { GroupArgs g; RoundArgs q; } c{g_in, q_in};
    const uint32_t *src = (const uint32_t *)&c;
#pragma unroll
    for (uint32_t i = 0; i < offsetof(ColdArgs, starts) / 4; ++i) cold[i] = src[i];
  }
  for (uint32_t i = threadIdx.x; i < g_in.count; i += BLK) cold[offsetof(ColdArgs, starts) / 4 + i] = g_in.table[i].start;
  __syncthreads();
  const uint32_t tid = threadIdx.x, wl = tid & 63;
  constexpr uint32_t NONE = 0xFFFFFFFFu, DONE = 0xFFFFFFFEu;
  // the few scalars the turn loop itself needs stay in SGPRs -- each read back from the LDS copy as a 32-bit value of its own:
  // taken straight from the kernel arguments they stay sub-registers of the 16-dword argument load, and the register
  // allocator then spills and restores that WHOLE tuple around the turn loop (round 3: 39 SGPR spills, 16 v_readlane per
  // wave iteration, after the migration arguments joined RoundArgs)
#define COLD_U32(off) ((uint32_t)__builtin_amdgcn_readfirstlane((int)cold[(off) / 4]))
#define COLD_QU(field) COLD_U32(offsetof(ColdArgs, q) + offsetof(RoundArgs, field))
#define COLD_GU(field) COLD_U32(offsetof(ColdArgs, g) + offsetof(GroupArgs, field))
  // (wave-uniform booleans live as BITS of one scalar word: as `bool`s each is a 64-bit lane mask, two SGPRs, and the turn loop
  // has none to spare)
  constexpr uint32_t U_RESUME = 1, U_PREP = 2, U_ADOPTER = 4, U_DRY = 8, U_ADOPTING = 16, U_ANY_PLAYING = 32, U_NO_SKIP = 64, U_CARRIED = 128, U_MIGRATE = 1u << 11;
  uint32_t ust = (COLD_QU(list_in) | COLD_U32(offsetof(ColdArgs, q) + offsetof(RoundArgs, list_in) + 4)) != 0 ? U_RESUME : 0u; // a later round: playouts come from the previous round's suspended list
#define IS_RESUME ((ust & U_RESUME) != 0)
#define IS_PREP ((ust & U_PREP) != 0)
  const uint32_t total = IS_RESUME ? (uint32_t)__builtin_amdgcn_readfirstlane((int)*COLD_Q(n_in, const uint32_t *)) : COLD_GU(total);
  const uint32_t max_steps = COLD_GU(max_steps), suspend_below = COLD_QU(suspend_below);
  if (!IS_RESUME && COLD_GU(prep) != 0) ust |= U_PREP;
  ust |= (blockIdx.x & 7u) << 8; // the queue head this wave starts at
  if (COLD_QU(no_skip) != 0) ust |= U_NO_SKIP;
  // bits 24-31: the move-carry threshold (below).  A resume or tail round and a launch spread over part of its lanes never carry.
  if (!IS_RESUME && COLD_QU(lanes) == 0) ust |= (COLD_QU(move_carry) & 0xFFu) << 24;
  ER e;
  e.m = party + tid;
  e.T = T;
  FastPrng g;
  g.s0 = g.s1 = 0;
  uint32_t idx = NONE, result = 0, steps = 0;
  { const uint32_t lanes = COLD_QU(lanes); if (lanes && wl >= lanes) idx = DONE; } // (tail round: this lane stays empty)
#define IS_DRY ((ust & U_DRY) != 0) // wave-uniform: the queue has handed out its last playout
  // ---- long-playout migration.  The launch ends with its longest playouts -- 1,000-step chains -- and while the device is
  // full such a playout advances at the pace of a full, divergent wave (31 us per turn-step).  So a BULK wave hands a playout
  // that is still running after `long_steps` turn-steps (99.5% end before 250) to the ADOPTER waves (the first n_adopters
  // waves, about one per CU): bit-exact state image to the scratch slot (the regrouping rounds' suspend image), agent-scope
  // release, a ticket in the adoption list.  An adopter stops taking playouts from the main queue once the first donation
  // exists, lets its own finish, and from then on holds only long playouts -- a dozen per wave, at the top priority of its
  // SIMD -- so the chains run at a sparse wave's pace (4-8 us per turn-step) from their 200th step on instead of from the
  // moment the device drains.  Every wait is bounded (a ticket reserved but not yet written; an adopter with nothing to
  // adopt while bulk waves still run): on overflow the error word is set and the wave leaves.  Results are indexed by
  // playout: they do not depend on who finishes a playout.
  // Round 4: a STANDSTILL counter donates earlier.  Measured on the oracle (2 x 65,536 playouts): the playouts that run into the cap
  // stop changing any hp at a median of turn-step 85 (p90 160) -- from then on they are the stalemates of k_queue_order's comment --
  // while an ordinary playout almost never goes 40 turn-steps without its actives' {slot, hp} changing.  `stale` = a 24-bit
  // signature of both actives (hp xor, slot sum: symmetric, the frame may be swapped) | the turn-steps it has stood still << 24.
  const uint32_t long_steps = COLD_QU(long_steps);
  uint32_t stale = 0;
  { const uint32_t n_adopt = COLD_QU(n_adopters); if (n_adopt != 0) ust |= blockIdx.x < n_adopt ? U_MIGRATE | U_ADOPTER : U_MIGRATE; } // (the count itself is read where an adopter needs it)
#define IS_ADOPTER ((ust & U_ADOPTER) != 0)
#define IS_ADOPTING ((ust & U_ADOPTING) != 0) // adopter: a donation has been seen, no more playouts from the main queue
#define ANY_PLAYING ((ust & U_ANY_PLAYING) != 0)
  uint32_t idle_polls = 0, poll_tick = 15;
  constexpr uint32_t SPIN_CAP = 1u << 22;
  constexpr int ERR_WORD = 23; // adopt_ctl + 23 = word 63 of the context's control block: STICKY (no launch clears it; oakgpu_synchronize reads and clears)
  OAK_PROF_ZERO();
  OAK_TL(0, wall_clock64());
#ifdef OAKGPU_TIMELINE
  bool tl_dry = false;
  unsigned long long tl_steps = 0;
#endif
  for (;;) {
    bool need = idx == NONE, load = false, from_scratch = IS_RESUME;
    uint64_t mask = __ballot(need);
    // (an adopter looks at the adoption list every 16th turn-step, or at once when it has nothing to play: 256 sparse waves
    // polling three words on every iteration saturate that L2 line's atomics and slow the whole launch down)
    if (mask && IS_ADOPTER && ((++poll_tick & 15u) == 0 || !ANY_PLAYING)) { // wave-uniform: an adopter's free lanes take donated playouts first
      uint32_t *ctl = COLD_Q(adopt_ctl, uint32_t *);
      uint32_t h = 0, k = 0, closed = 0;
      if (wl == 0) {
        for (int tries = 0; tries < 8; ++tries) {
          // HEAD first, then TAIL: the tail only grows and the head never passes it, so tail - head cannot underflow (read the
          // other way round, a head that moved in between claimed tickets beyond the list: a memory fault at full size)
          const uint32_t hh = __hip_atomic_load(ctl + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
          const uint32_t t = __hip_atomic_load(ctl + 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
          if (t) closed |= 2; // (bit 1: a donation exists)
          const uint32_t kk = t > hh ? min(t - hh, (uint32_t)__popcll(mask)) : 0u;
          if (!kk) {
            // every bulk wave has left (a wave's last donation is complete before it counts itself out) and nothing is waiting
            if (__hip_atomic_load(ctl + 2, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - COLD_QU(n_adopters) &&
                __hip_atomic_load(ctl + 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == hh &&
                __hip_atomic_load(ctl + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == hh) closed |= 1;
            break;
          }
          if (atomicCAS(ctl + 1, hh, hh + kk) == hh) { h = hh; k = kk; break; }
        }
      }
      h = (uint32_t)__builtin_amdgcn_readfirstlane((int)h); k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k); closed = (uint32_t)__builtin_amdgcn_readfirstlane((int)closed);
      if (closed & 2) ust |= U_ADOPTING;
      const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << wl) - 1));
      const bool take = need && rank < k;
      uint32_t got = 0;
      if (take && h + rank < COLD_GU(total)) { // (tickets live in [0, total): one per donation at most)
        // a ticket is one 64-bit word {playout + 1, this launch's epoch}: whatever an earlier launch left in the slot carries another
        // epoch and reads as "not written yet", so no launch clears the list (it was a pass over total x 4 bytes in front of every launch)
        const uint64_t *slot = COLD_Q(adopt_list, const uint64_t *) + h + rank;
        const uint32_t epoch = COLD_QU(epoch);
        uint32_t spins = 0;
        uint64_t tk;
        while ((uint32_t)((tk = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != epoch && ++spins < SPIN_CAP) __builtin_amdgcn_s_sleep(2);
        if ((uint32_t)(tk >> 32) == epoch) got = (uint32_t)tk;
        if (!got) atomicOr(ctl + ERR_WORD, 1u); // (a ticket that never arrived: reported, the playout is lost -- the tests would see it)
      }
      if (k) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); // the donors' images, step counts and PRNG states
      if (take && got) { idx = got - 1; load = true; from_scratch = true; }
      need = idx == NONE;
      if ((closed & 1) && need) idx = DONE;              // adoption is over
      mask = (IS_ADOPTING || (closed & 1)) ? 0 : __ballot(need); // once donations exist an adopter takes no more bulk work
      need = need && mask != 0;
    }
    if (IS_ADOPTING) { mask = 0; need = false; } // (an adopter between two looks at the list: no bulk work either)
    // (an adopter's free lanes stay NONE after the queue has run dry -- they wait for donations -- and must not keep asking the
    // dry queue: ~150 waves adding to one L2 word on every iteration, and in a long launch the 32-bit head could wrap and hand
    // playouts out twice; round-3 advice)
    // (refills in batches, OAK_REFILL_EVERY > 1: a refill is a wave-wide stall -- a returning atomic, then the dependent loads of the
    // queue order, the batch descriptor and the 384-byte battle -- for the sake of the one or two lanes that finished in this
    // iteration; free lanes cost no issue slots, so they wait for company: every 8th iteration, or at once when 16 lanes are free.
    // Measured, tools/refill_variants.sh: driver command 8.53-8.59 -> 8.91-8.96 G, 160 steps 9.24-9.30 -> 9.76-9.79 G; every 4th / 16th
    // iteration and thresholds of 8 / 64 lanes are within 2 % of it)
    ust = (ust & ~0xFF0000u) | ((ust + 0x10000u) & 0xFF0000u);
    if (mask && !IS_DRY && (REFILL_EVERY <= 1 || ((ust >> 16) & (REFILL_EVERY - 1)) == 0 || (uint32_t)__popcll(mask) >= REFILL_LANES || !ANY_PLAYING)) { // wave-uniform
      OAK_SCOPE(PS_REFILL);
      // The queue has EIGHT heads, each on a 256-byte line of its own (round 5): one device-scope counter saturates at ~88 returning
      // atomics per microsecond on this chip (MI355X_MICROARCH.md, "dequeue"), and 4,096 waves refilling 0.5 times per ~28 us
      // iteration ask for 70-90 -- the single head of rounds 1-4 ran at its limit.  Head s hands out the queue positions s, s + 8,
      // s + 16, ... (so every head's sequence starts with the likely-long playouts of k_queue_order); a wave starts at head
      // blockIdx % 8 (workgroups are dealt round-robin over the XCDs) and moves to the next head when its own is exhausted; the
      // queue is dry for a wave when it has seen all eight exhausted.  `ust` bits 8-10: the current head, bits 12-15: heads seen dry.
      uint64_t rem = mask;
      bool got = false;
      uint32_t my = 0;
      for (;;) {
        const uint32_t shard = (ust >> 8) & 7u, need_n = (uint32_t)__popcll(rem);
        const uint32_t lim = total > shard ? (total - shard + 7u) >> 3 : 0u; // positions of this head
        uint32_t base = 0;
        if (wl == 0) base = atomicAdd(COLD_Q(queue, uint32_t *) + shard * QUEUE_HEAD_STRIDE, need_n);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base); // (lane 0 is active: whole waves run this loop)
        const uint32_t avail = base < lim ? (lim - base < need_n ? lim - base : need_n) : 0u;
        const uint32_t rank = (uint32_t)__popcll(rem & ((1ull << wl) - 1));
        if (((rem >> wl) & 1) && rank < avail) { my = shard + ((base + rank) << 3); got = true; }
        if (avail == need_n) break;
        rem = __ballot(need && !got);
        ust = (ust & ~(7u << 8)) | (((shard + 1u) & 7u) << 8);
        ust += 1u << 12;
        if (((ust >> 12) & 15u) >= 8u) { ust |= U_DRY; break; }
      }
#ifdef OAKGPU_TIMELINE
      if (IS_DRY && !tl_dry) { tl_dry = true; OAK_TL(1, wall_clock64()); }
#endif
      if (need) {
        if (got) {
          const uint32_t *order = COLD_Q(order, const uint32_t *);
          idx = IS_RESUME ? COLD_Q(list_in, const uint32_t *)[my] : order ? order[my] : my;
          load = true;
        } else idx = IS_ADOPTER ? NONE : DONE; // (the queue is dry; an adopter's free lanes wait for donations until adoption is over)
      }
    } else if (mask && IS_DRY && !IS_ADOPTER) { // the queue is dry: a bulk wave's free lanes are done (an adopter's wait for donations)
      if (need) idx = DONE;
    }
    if (__ballot(load)) { // wave-uniform: (re)fill the lanes that got a playout -- from its batch, or from its parked image
      OAK_SCOPE(PS_REFILL);
      if (load) {
        const BatchDesc *bd = find_batch(cold, idx);
        const uint32_t k = idx - bd->start; // playout k of its batch
        if constexpr (KEEP_DUR) {
          const uint32_t *dsrc = from_scratch ? COLD_Q(sd, const uint32_t *) + 2 * (size_t)idx : (const uint32_t *)bd->durations + 2 * (size_t)k;
          const uint32_t *psrc = (const uint32_t *)bd->prng + 2 * (size_t)k;
          g.s0 = psrc[0];
          g.s1 = psrc[1];
          e.load_battle_global(from_scratch ? COLD_Q(sb, const uint8_t *) + (size_t)idx * 384 : bd->battles + (size_t)k * 384, dsrc[0], dsrc[1]);
          if (IS_PREP && !from_scratch) { // mcts.h:254-259
            const uint32_t hi = g.next32(), lo = g.next32();
            e.rng = ((uint64_t)hi << 32) | lo;
            e.randomize_hidden();
          }
        } else {
          const uint32_t *psrc = (const uint32_t *)bd->prng + 2 * (size_t)k;
          g.s0 = psrc[0];
          g.s1 = psrc[1];
          e.load_battle_global(from_scratch ? COLD_Q(sb, const uint8_t *) + (size_t)idx * 384 : bd->battles + (size_t)k * 384);
          if (PREP && IS_PREP && !from_scratch) { // the batch's durations serve the prep of a fresh playout and nothing after it
            const uint32_t *dsrc = (const uint32_t *)bd->durations + 2 * (size_t)k;
            const uint32_t hi = g.next32(), lo = g.next32();
            e.rng = ((uint64_t)hi << 32) | lo;
            e.randomize_hidden(dsrc[0], dsrc[1]);
          }
        }
        result = from_scratch ? COLD_Q(sres, const uint8_t *)[idx] : bd->results_in[k];
        steps = from_scratch ? bd->steps_out[k] : 0;
        stale = 0;
      }
    }
    if (__ballot(idx != DONE) == 0) break;
    // MOVE CARRY.  A turn is up to two actions, and the wave walks ONE copy of the action code once per action.  A switch goes before
    // a move, so the first walk holds the move pipeline for the move + move lanes alone and the second for them and the switch + move
    // lanes together: two trips through before_move / execute_selected / run_move per turn-step, each for well under half of the wave.
    // The lanes are independent playouts, so a lane's second action may as well wait for the wave's NEXT walk, where it runs beside
    // the other lanes' first actions.  Such a lane is in MID-TURN: T_PEND and its pending choice byte sit in the free bits of `result`
    // (whose low byte is 0 then: it reads as playing), it skips the turn's start in the next iteration, and its step count, `stale`
    // and everything that retires, parks or refills a lane wait for the turn's end.  Per lane the engine operations and draws are the
    // same sequence as ever.  The first trip through the move pipeline takes every pending move (a switch in front of a move has
    // run by then).  The second trip takes what is still pending -- if at least `carry_below` (ust bits
    // 24-31; 0 = always, the schedule without carrying) lanes want it, or if the wave FLUSHES: it is dry (and below its dry-carry threshold: U_CARRIED below) or an adopter that adopts
    // (resume, tail and spread launches have carry_below 0).  So a wave that can suspend, a wave that leaves and every lane that
    // is written out stands at a turn boundary: the drain, the adopters and the images are what they were.
    constexpr uint32_t T_PEND = 0x100u, T_DONE = 0x200u; // during the walks the low byte of `result` is the turn's result so far
    const bool mid = (result & T_PEND) != 0;
    bool playing = idx != DONE && idx != NONE && (result & 15) == 0 && steps < max_steps; // (NONE: an adopter's lane that waits)
    const bool start = playing && !mid;
#ifdef OAKGPU_TIMELINE
    tl_steps += (unsigned long long)__popcll(__ballot(start));
#endif
    // A standstill that can be PROVEN (EngineR::inert_standstill): each side is either FROZEN with no way out (gen 1 never thaws by
    // itself) or FORCED -- Rage-locked, or down to Struggle on its last Pokemon -- into a move the foe's types are immune to, and
    // nothing acts on a Pokemon that cannot act (no Leech Seed, no binding).  Such a turn-step executes no move beyond its type
    // check, spends no PP, and leaves every byte as it was except the turn counter, battle.rng -- by a CONSTANT number c of draws:
    // the speed tie of equal speeds and a paralysed side's full-paralysis roll, both outcomes of which are no-ops -- and the fields
    // the NEXT turn-step overwrites before anything reads them.  So all but the last of the remaining turn-steps are taken at
    // once: turn and step count advance, the choice stream advances by its two draws per turn-step, battle.rng jumps c draws per
    // turn-step ahead, and the last turn-step runs for real (it writes last selected / used move, last damage 0, the counterable
    // bits and, at turn 1,000, the tie).  These are the launch's stalemates -- Rage or Struggle against a Ghost, a frozen Ghost --
    // ~1,100 of 1.31 M playouts, each otherwise ~850 dependent turn-steps on an adopter.  Exact, not a heuristic:
    // tests/test_gpu_inert_standstill.py and tests/test_gpu_parity.py hold it to the oracle, which plays every turn.  The `stale`
    // gate keeps ordinary lanes from ever evaluating the predicate.
    if (start && stale >= (8u << 24) && !(ust & U_NO_SKIP)) {
      const int draws = e.inert_standstill(result);
      const uint32_t by_steps = max_steps - steps, by_turn = 1000u - e.turn;
      const uint32_t skip = (by_steps < by_turn ? by_steps : by_turn) - 1u; // (both >= 1 while playing)
      if (draws >= 0 && skip != 0) {
        for (uint32_t k = 0; k < skip; ++k) { (void)g.next32(); (void)g.next32(); }
        e.rng_jump((uint32_t)draws * skip);
        e.turn += skip;
        steps += skip;
        atomicAdd((unsigned long long *)COLD_Q(stats, uint32_t *), 1ull | ((unsigned long long)skip << 32)); // {playouts, turn-steps}: one atomic
      }
    }
    {
      OAK_SCOPE(PS_STEP);
      // (the pending choice byte lives in bits 16-23 of `result` and the one after it in bits 24-31, during the walks as between
      // iterations: a lane in mid-turn comes in with T_PEND, its last action and nothing behind it)
      if (start) { // the turn's start: two draws of the choice stream, both sides' choices, who acts first
        OAK_T0(t_ld);
        const uint32_t hi = g.next32(), lo = g.next32(); // uniform_64 = hi << 32 | lo
        uint32_t cS, cF, pc = 0, qc = 0;
        e.random_choices(result, hi, lo, cS, cF);
        OAK_T1(PS_LEGAL_DRAW, t_ld);
        const uint32_t r = e.turn_prologue(cS, cF, pc, qc);
        result = r ? (r | T_DONE) : (T_PEND | (pc << 16) | (qc << 24)); // (turn 0 sends both leads out and is over)
      }
      // ONE copy of the action code, walked up to three times.  A wave that carries walks it first for the lanes whose pending action
      // is cheap (a switch, a pass) -- so that a switch + move turn has its move ready for the next walk --, then for every pending
      // action: the one trip through the move pipeline that every iteration makes.  The third walk is the second trip, for what is
      // still pending (move + move turns): only if `carry_below` lanes want it.  A wave that does not carry (threshold 0, or a
      // flush) skips the first walk and always takes the third: the schedule of update_frame.
      // (wave-uniform, kept as a bit of `ust` like the other flags: U_CARRIED = this iteration carries and may leave lanes in mid-turn)
      if ((ust >> 24) != 0 && !(ust & (U_DRY | U_ADOPTING))) ust |= U_CARRIED; else ust &= ~U_CARRIED;
      // (round 18: a dry BULK wave goes on carrying while at least `move_carry_dry` of its lanes play -- the host makes that no fewer than
      // a regrouping or tail launch suspends at: a wave about to suspend flushes first.  The threshold is read where it is needed: a dry
      // wave's iterations)
      if ((ust >> 24) != 0 && IS_DRY && !IS_ADOPTER) {
        const uint32_t dry_below = COLD_QU(move_carry_dry);
        if (dry_below != 0 && (uint32_t)__popcll(__ballot(playing)) >= dry_below) ust |= U_CARRIED;
      }
#define CARRYING ((ust & U_CARRIED) != 0)
#pragma unroll 1
      for (uint32_t walk = CARRYING ? 0u : 1u;; ++walk) {
        const uint32_t c = (result >> 16) & 0xFFu;
        if ((result & T_PEND) && (walk != 0 || (c & 3) != C_MOVE)) {
          OAK_SET_K(e, walk ? walk - 1 : 0);
          const uint32_t r = e.act(c);
          e.next_actor();
          const uint32_t next = T_PEND | ((result >> 8) & 0xFF0000u); // the action behind it moves up; none: a pass
          result = (r != 0 || ((next >> 16) & 3) == C_PASS) ? (r | T_DONE) : next;
        }
        if (walk == 2) break;
        if (walk == 1) {
          const uint32_t want = (uint32_t)__popcll(__ballot((result & T_PEND) != 0));
          if (want == 0 || (CARRYING && want < (ust >> 24))) break;
        }
      }
      // (a lane that is still pending is carried as it stands: low byte 0, still playing)
      if (result & T_DONE) { // the turn's end, and what belongs to a turn boundary
        result = e.turn_finish(result & 0xFFu);
        ++steps;
        playing = (result & 15) == 0 && steps < max_steps;
        const uint32_t sg = ((e.S.p4 ^ e.F.p4) >> 16) | (((e.S.o0 + e.F.o0) & 0xFFu) << 16);
        stale = sg != (stale & 0xFFFFFFu) ? sg : stale + (stale < 0xFF000000u ? 0x01000000u : 0u);
      }
    }
    // a wave that holds a playout far beyond the usual length (99.5% end before 250 turn-steps) is on the launch's critical
    // path -- a 1000-step chain: it goes first on its SIMD (an adopter as soon as it adopts)
    // (round 4: ... or one whose actives have stood still for PRIO_STILL turn-steps -- the stalemates that run into the cap stop changing
    // at a median of turn-step 85, so their wave goes first ~90 turn-steps earlier; a false alarm costs nothing but a while of priority)
    if (IS_ADOPTING || __ballot(playing && (steps > LONG_STEPS || stale >= (PRIO_STILL << 24)))) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(0);
    if (__ballot(playing) != 0) ust |= U_ANY_PLAYING; else ust &= ~U_ANY_PLAYING;
    if (IS_ADOPTER && !ANY_PLAYING) { // nothing to play: wait for donations (bounded) without burning issue slots
      __builtin_amdgcn_s_sleep(100);
      if (++idle_polls > SPIN_CAP) { if (wl == 0) atomicOr(COLD_Q(adopt_ctl, uint32_t *) + ERR_WORD, 2u); break; }
    }
    // wave-uniform: the queue is dry and too few lanes are still playing -> hand them to the next round
    const uint64_t still = __ballot(playing);
    // (a lane in mid-turn -- a dry wave that carried in this iteration -- has no image to park: the wave flushes in its next iteration, then suspends)
    const bool suspend = IS_DRY && !(ust & U_CARRIED) && still != 0 && (uint32_t)__popcll(still) < suspend_below;
    const bool lng = (ust & U_MIGRATE) != 0 && !IS_ADOPTER && playing && !(result & T_PEND) && (steps >= (long_steps & 0xFFFFu) || (stale >> 24) >= (long_steps >> 16)); // a bulk wave's long (or standing-still) playout: to the adopters
    if (idx != DONE && idx != NONE && (!playing || suspend || lng)) { // retire the lane: publish a finished playout / park a suspended or donated one
      OAK_SCOPE(PS_PUBLISH);
      const bool fin = !playing;
      // the image is written from COPIES of the sides by player: normalising `e` in place (lane-masked) made the whole engine state a
      // value that differs between the two ways out of this branch, and the wave copied it to a second register set and back in
      // every iteration (round 18); the engine's own frame stays where the turn left it -- a parked or finished lane's is dead
      typename ER::SideR P1, P2;
      sides_by_player(ER::absp(e.S) != 0, e.S, e.F, P1, P2);
      const BatchDesc *bd = find_batch(cold, idx);
      const uint32_t k = idx - bd->start;
      if (fin) bd->results_out[k] = (uint8_t)result; else COLD_Q(sres, uint8_t *)[idx] = (uint8_t)result;
      bd->steps_out[k] = steps;
      const uint32_t t = result & 15;
      if (fin) bd->values_out[k] = t == R_WIN ? 1.0f : t == R_LOSE ? 0.0f : 0.5f;
      uint32_t *pdst = (uint32_t *)bd->prng + 2 * (size_t)k;
      pdst[0] = g.s0;
      pdst[1] = g.s1;
      if constexpr (KEEP_DUR) {
        uint32_t *ddst = fin ? (bd->durations_out ? (uint32_t *)bd->durations_out + 2 * (size_t)k : nullptr) : COLD_Q(sd, uint32_t *) + 2 * (size_t)idx;
        if (ddst) {
          ddst[0] = P1.dur;
          ddst[1] = P2.dur;
        }
      }
      uint8_t *bdst = fin ? (bd->battles_out ? bd->battles_out + (size_t)k * 384 : nullptr) : COLD_Q(sb, uint8_t *) + (size_t)idx * 384;
      if (bdst) e.store_battle_global(bdst, P1, P2);
      idx = fin ? NONE : idx;
    }
    const uint64_t dm = __ballot(lng);
    if (dm) { // wave-uniform, rare: release the images, take tickets, write them
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      uint32_t *ctl = COLD_Q(adopt_ctl, uint32_t *);
      const uint32_t leader = (uint32_t)__ffsll((unsigned long long)dm) - 1;
      uint32_t base = 0;
      if (wl == leader) base = atomicAdd(ctl + 0, (uint32_t)__popcll(dm));
      base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader);
      if (lng) {
        __hip_atomic_store(COLD_Q(adopt_list, uint64_t *) + base + (uint32_t)__popcll(dm & ((1ull << wl) - 1)), (uint64_t)(idx + 1) | ((uint64_t)COLD_QU(epoch) << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        idx = NONE; // the lane is free again
      }
    }
    if (suspend) {
      const uint32_t leader = (uint32_t)__ffsll((unsigned long long)still) - 1;
      uint32_t base = 0;
      if (wl == leader) base = atomicAdd(COLD_Q(count_out, uint32_t *), (uint32_t)__popcll(still));
      base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader);
      if (playing) COLD_Q(list_out, uint32_t *)[base + (uint32_t)__popcll(still & ((1ull << wl) - 1))] = idx;
      break;
    }
  }
  if ((ust & U_MIGRATE) != 0 && !IS_ADOPTER && wl == 0) atomicAdd(COLD_Q(adopt_ctl, uint32_t *) + 2, 1u); // a bulk wave has left: it donates no more
  OAK_TL(2, wall_clock64());
#ifdef OAKGPU_TIMELINE
  OAK_TL(4, tl_steps);
#endif
  OAK_PROF_FLUSH();
}
#undef COLD_Q
#undef COLD_U32
#undef COLD_QU
#undef COLD_GU
#undef IS_RESUME
#undef IS_PREP
#undef IS_DRY
#undef IS_ADOPTER
#undef IS_ADOPTING
#undef ANY_PLAYING
#undef CARRYING

// ---- root-parallel search steps in SLICES (BASELINE configs[3]: 256 roots x 4,096 playouts per search step) -----------------
// A search step of root-parallel MCTS hands every root `reps` fresh playouts (run_root_iteration's prep, mcts.h:250-263, then the
// rollout loop of mcts.h:448-496) and consumes one aggregate per root.  Run to terminal inside the step, a step lasts as long
// as its LONGEST playout -- 98 % of the 4,096-playout batches hold one that runs into the 1,000-step cap: a chain of 1,000 dependent
// turn-steps (6 ms) however little work the step holds, which is what bound a rank's share at 8 GPUs (round 4: 6.5 ms, 1.8x
// projected).  The reference's workers never wait for each other (generate.cc:527-536), and neither does a step here: a launch
// advances every playout in flight by at most `slice` turn-steps (a power of two).  A playout that ends inside its slice is
// CREDITED TO THE STEP WHOSE LAUNCH FINISHED IT -- step k + (len - 1) / slice for a playout of len turn-steps started in step k,
// a function of the playout's own length only, never of the schedule; one that does not is CARRIED: its bit-exact state image
// (the 384-byte battle, durations, result, step count, its own choice stream, its root) goes to the carry list and the NEXT
// step's launch resumes it beside that step's fresh playouts.  Values never change, only the step they are credited to.
// The per-root aggregate is folded into the retire path: one 64-bit atomic per finished playout, count | (2 x value) << 32
// -- integers, so a root's aggregate does not depend on the order its playouts finish in (byte-identical to the oracle's).
//   Streams: lane (root r, replica i) owns one fast_prng stream that advances by exactly ONE uniform_64 per step; that draw IS
// the 8-byte state of the step's fresh playout's own stream (an all-zero draw -- the generator's fixed point -- becomes s1 = 1),
// from which the playout takes battle.rng (prep) and its choices.  So a carried playout and the lane's next fresh one never
// share draws, and nothing depends on which launch, wave or rank runs a playout.
struct RootStepArgs {
  const uint8_t *root_battles, *root_durations, *root_results; // n_roots x {384, 8, 1}
  uint8_t *lane_prng;              // n_fresh x 8
  const uint4 *cin_state;          // carried playouts: ROOT_SHARDS segments of `seg` records of CARRY_VEC uint4 (below)
  const uint32_t *cin_count;       // ROOT_SHARDS counters, CTL_STRIDE words apart (one 256-byte line each)
  uint4 *cout_state;
  uint32_t *cout_count;
  unsigned long long *acc;         // ROOT_SHARDS x acc_stride: finished playouts credited to this step per root, count | (2 x value) << 32, one copy per
                                   // shard (a rank's 32 roots are ONE 256-byte line: 131,072 credits per 1.4 ms on it ran at the ~90 atomics/us a line takes)
  unsigned long long *turn_steps;  // += the turn-steps this launch executed
  uint32_t *queue;                 // ROOT_SHARDS queue heads (CTL_STRIDE words apart), zeroed before the launch
  uint32_t *err;                   // sticky: bit 0 = a carry segment overflowed (playouts lost)
  uint32_t n_fresh, reps, seg, slice_mask, max_steps, fper; // fper: fresh lanes per shard (the last shard takes what is left)
  uint32_t acc_stride, pad;        // u64 entries between two shards' accumulators
};
// The queue and the carry list are cut into 8 SHARDS, each with a head and a counter on a 256-byte line of its own: one device-scope
// counter saturates at ~88 returning atomics per microsecond on this chip (MI355X_MICROARCH.md, "dequeue"), and a step in slices
// of 64 turn-steps needs ~110 dequeues + ~60 carry tickets per microsecond -- with ONE head and ONE ticket counter the kernel ran at
// exactly that rate whatever else it did (256 roots: 20 ms per step at slice 64, 30 ms at 32, against 11 ms of turn-steps).  Shard
// s = {segment s of the carry list, fresh lanes [s * fper, (s + 1) * fper)}; a wave starts at shard blockIdx % 8 (the dispatcher
// deals workgroups round-robin over the XCDs) and moves on to the next shard when its own is exhausted, so every playout is taken
// whoever is left; it carries into its home shard's segment of the outgoing list.
#ifndef OAK_ROOT_REFILL_EVERY
#define OAK_ROOT_REFILL_EVERY 8
#endif
#ifndef OAK_ROOT_REFILL_LANES
#define OAK_ROOT_REFILL_LANES 16
#endif
constexpr uint32_t ROOT_REFILL_EVERY = OAK_ROOT_REFILL_EVERY, ROOT_REFILL_LANES = OAK_ROOT_REFILL_LANES;
constexpr int ROOT_SHARDS = 8;
constexpr int CTL_STRIDE = 64; // words between two counters
// A carried playout travels as the engine's own MUTABLE state, raw: both sides' register sets (2 x 18 dwords, in whatever frame the
// turn left them), the battle scalars, the 24 party dwords of its LDS column, its choice stream, step count, root and result --
// 72 dwords = 18 uint4, stored and loaded as whole vectors with no load in the store path.  (First form: the 384-byte battle
// image through store_battle_global / load_battle_global, whose stores each wait for a load of the immutable fields behind the
// previous store -- stores count in vmcnt on gfx950 -- ~37 us of wave time per carried playout: 256 roots in slices of 64 ran at
// 5.2 G turn-steps/s against 9.4 G without slices.)  The immutable party data is the ROOT's (`gin`), shared by the root's playouts.
// KEEP_DUR = false (round 32): the step returns aggregates only, so the engine keeps no durations word -- a fresh playout's serve its
// prep and nothing after, a carried playout's serve nothing.  The record stays CARRY_VEC = 18 vectors: the sides' 2 x 17 dwords packed
// at 0 .. 33, dwords 34 and 35 are padding and the scalars behind them keep their places (a pad dword behind EACH side's set cost the
// kernel 16 bytes of scratch).  Records of the two instantiations differ: a handle runs ONE of them for its whole life
// (oakgpu_root_steps_create).
constexpr int CARRY_VEC = 18;
constexpr int ROOT_STEP_COLD_BYTES = ((sizeof(RootStepArgs) + 15) & ~15) + ROOT_SHARDS * 4;
constexpr int ROOT_STEP_LDS_BYTES = 24 * 64 * 4 + TABLE_LDS_PAD + ROOT_STEP_COLD_BYTES;
template <int WPS, bool KEEP_DUR = true>
__global__ __launch_bounds__(64, WPS) void k_root_step(RootStepArgs a_in) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<64, false, false, KEEP_DUR>;
  Tables T = stage_default_tables((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4);
  // the cold arguments are parked in LDS, like k_rollout_queue's: as kernel arguments they would hold ~34 SGPRs across the turn loop
  lds_u32 *cold = (lds_u32 *)((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4 + TABLE_LDS_PAD);
  if (threadIdx.x == 0) {
    const uint32_t *src = (const uint32_t *)&a_in;
#pragma unroll
    for (uint32_t i = 0; i < sizeof(RootStepArgs) / 4; ++i) cold[i] = src[i];
  }
  lds_u32 *sh_carry = cold + ((sizeof(RootStepArgs) + 15) & ~15) / 4; // carried playouts per shard (clamped to the segment size)
  if (threadIdx.x < ROOT_SHARDS) {
    const uint32_t c = a_in.cin_count[threadIdx.x * CTL_STRIDE];
    sh_carry[threadIdx.x] = c < a_in.seg ? c : a_in.seg; // (an overflowing launch lost the playouts beyond the segment and said so in *err)
  }
  __syncthreads();
#define RS_PTR(field, type) cold_ptr<type>(cold, offsetof(RootStepArgs, field))
#define RS_U32(field) ((uint32_t)__builtin_amdgcn_readfirstlane((int)cold[offsetof(RootStepArgs, field) / 4]))
  const uint32_t wl = threadIdx.x;
  constexpr uint32_t NONE = 0xFFFFFFFFu, DONE = 0xFFFFFFFEu;
  const uint32_t seg = RS_U32(seg), max_steps = RS_U32(max_steps), slice_mask = RS_U32(slice_mask);
  const uint32_t home = blockIdx.x & (ROOT_SHARDS - 1);
  uint32_t shard = home, exhausted = 0, iter = 0xFFFFFFFFu;
  bool any_playing = false;
  ER e;
  e.m = party + wl;
  e.T = T;
  FastPrng g;
  g.s0 = g.s1 = 0;
  uint32_t root = NONE, result = 0, steps = 0, executed = 0;
  bool dry = false;
  for (;;) {
    bool load = false;
    uint32_t my = 0, my_carry = 0, my_shard = 0;
    const uint64_t mask = __ballot(root == NONE);
    ++iter;
    if (mask && !dry && (ROOT_REFILL_EVERY <= 1 || (iter & (ROOT_REFILL_EVERY - 1)) == 0 || (uint32_t)__popcll(mask) >= ROOT_REFILL_LANES || !any_playing)) { // wave-uniform: free lanes take the next playouts of the wave's current shard -- its carried ones first (the oldest)
      uint64_t rem = mask;
      while (rem) {
        const uint32_t need = (uint32_t)__popcll(rem);
        const uint32_t carry_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh_carry[shard]);
        const uint32_t n_fresh = RS_U32(n_fresh), fper = RS_U32(fper), flo = shard * fper;
        const uint32_t fresh_s = flo < n_fresh ? (n_fresh - flo < fper ? n_fresh - flo : fper) : 0u;
        const uint32_t tot = carry_s + fresh_s;
        uint32_t base = 0;
        if (wl == 0) base = atomicAdd(RS_PTR(queue, uint32_t *) + shard * CTL_STRIDE, need);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        const uint32_t avail = base < tot ? (tot - base < need ? tot - base : need) : 0u;
        const uint32_t rank = (uint32_t)__popcll(rem & ((1ull << wl) - 1));
        if (((rem >> wl) & 1) && rank < avail) { my = base + rank; my_carry = carry_s; my_shard = shard; load = true; }
        if (avail == need) break;
        rem = __ballot(root == NONE && !load);           // the shard is exhausted: the lanes it could not serve try the next one
        shard = (shard + 1) & (ROOT_SHARDS - 1);
        if (++exhausted >= (uint32_t)ROOT_SHARDS) { dry = true; break; }
      }
    }
    if (dry && root == NONE && !load) root = DONE;
    if (__ballot(load)) {
      if (load && my < my_carry) { // resume a carried playout from its record
        const uint4 *rec = RS_PTR(cin_state, const uint4 *) + (size_t)CARRY_VEC * ((size_t)my_shard * seg + my);
        uint4 v[CARRY_VEC];
#pragma unroll
        for (int q = 0; q < CARRY_VEC; ++q) v[q] = rec[q];
        // (component i of the record by CONSTANT index: no pointer into the register array, which would put it in scratch)
        auto w = [&](int i) -> uint32_t { const uint4 &q = v[i >> 2]; return (i & 3) == 0 ? q.x : (i & 3) == 1 ? q.y : (i & 3) == 2 ? q.z : q.w; };
        int o = 0;
        if constexpr (KEEP_DUR) {
#define X(f) e.S.f = w(o++);
          OAK_FOR_SIDE_FIELDS(X)
#undef X
#define X(f) e.F.f = w(o++);
          OAK_FOR_SIDE_FIELDS(X)
#undef X
        } else {
#define X(f) e.S.f = w(o++);
          OAK_FOR_SIDE_FIELDS_LEAN(X)
#undef X
#define X(f) e.F.f = w(o++);
          OAK_FOR_SIDE_FIELDS_LEAN(X)
#undef X
        }
        e.rng = (uint64_t)w(36) | ((uint64_t)w(37) << 32);
        e.turn = w(38) & 0xFFFF; e.last_damage = w(38) >> 16; e.lm = w(39);
#pragma unroll
        for (int q = 0; q < 24; ++q) e.m[q * 64] = w(40 + q);
        g.s0 = w(64); g.s1 = w(65); steps = w(66); root = w(67); result = w(68);
        e.actS = e.actF = 0;
        e.gin = (const uint32_t *)(RS_PTR(root_battles, const uint8_t *) + (size_t)root * 384);
      } else if (load) {          // a fresh playout of lane `ln` = (root, replica): mcts.h:250-263
        const uint32_t ln = my_shard * RS_U32(fper) + (my - my_carry);
        root = ln / RS_U32(reps);
        uint32_t *ps = (uint32_t *)RS_PTR(lane_prng, uint8_t *) + 2 * (size_t)ln;
        FastPrng lane;
        lane.s0 = ps[0]; lane.s1 = ps[1];
        const uint32_t hi = lane.next32(), lo = lane.next32(); // the lane's uniform_64 of this step = the playout's own stream
        ps[0] = lane.s0; ps[1] = lane.s1;
        g.s0 = hi; g.s1 = (hi | lo) ? lo : 1u;
        const uint32_t *dsrc = (const uint32_t *)RS_PTR(root_durations, const uint8_t *) + 2 * (size_t)root;
        if constexpr (KEEP_DUR) {
          e.load_battle_global(RS_PTR(root_battles, const uint8_t *) + (size_t)root * 384, dsrc[0], dsrc[1]);
          const uint32_t bh = g.next32(), bl = g.next32();
          e.rng = ((uint64_t)bh << 32) | bl;
          e.randomize_hidden();
        } else { // the root's durations serve the prep and are dropped
          e.load_battle_global(RS_PTR(root_battles, const uint8_t *) + (size_t)root * 384);
          const uint32_t bh = g.next32(), bl = g.next32();
          e.rng = ((uint64_t)bh << 32) | bl;
          e.randomize_hidden(dsrc[0], dsrc[1]);
        }
        result = RS_PTR(root_results, const uint8_t *)[root];
        steps = 0;
      }
    }
    if (__ballot(root != DONE) == 0) break;
    bool playing = root < DONE && (result & 15) == 0 && steps < max_steps;
    bool sliced = false;
    executed += (uint32_t)__popcll(__ballot(playing));
    if (playing) {
      const uint32_t hi = g.next32(), lo = g.next32(); // uniform_64 = hi << 32 | lo
      result = e.random_step(result, hi, lo);
      ++steps;
      playing = (result & 15) == 0 && steps < max_steps;
      sliced = playing && (steps & slice_mask) == 0; // the slice is over: the playout is carried
    }
    any_playing = __ballot(playing && !sliced) != 0;
    // (retiring in batches as well -- finished and sliced lanes waiting for the iteration in front of a refill -- was measured and
    // dropped: nothing at 256 roots, 1.53 -> 1.60 ms for a rank's 32 roots; same for the queue kernel's publishing)
    const uint64_t cm = __ballot(sliced);
    uint32_t slot = 0;
    if (cm) { // wave-uniform: one ticket range per wave for the playouts whose slice is over
      const uint32_t leader = (uint32_t)__ffsll((unsigned long long)cm) - 1;
      uint32_t base = 0;
      if (wl == leader) base = atomicAdd(RS_PTR(cout_count, uint32_t *) + home * CTL_STRIDE, (uint32_t)__popcll(cm));
      slot = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader) + (uint32_t)__popcll(cm & ((1ull << wl) - 1));
    }
    if (root < DONE && (!playing || sliced)) { // retire the lane: credit a finished playout to this step / carry an unfinished one
      if (!sliced) {
        const uint32_t t = result & 15;
        const unsigned long long v2 = t == R_WIN ? 2ull : t == R_LOSE ? 0ull : 1ull; // 2 x {1, 0, 0.5}: mcts.h:481-495
        atomicAdd(RS_PTR(acc, unsigned long long *) + (size_t)home * RS_U32(acc_stride) + root, 1ull | (v2 << 32));
      } else if (slot < seg) {
        uint32_t w[CARRY_VEC * 4];
        int o = 0;
        if constexpr (KEEP_DUR) {
#define X(f) w[o++] = e.S.f;
          OAK_FOR_SIDE_FIELDS(X)
#undef X
#define X(f) w[o++] = e.F.f;
          OAK_FOR_SIDE_FIELDS(X)
#undef X
        } else {
#define X(f) w[o++] = e.S.f;
          OAK_FOR_SIDE_FIELDS_LEAN(X)
#undef X
#define X(f) w[o++] = e.F.f;
          OAK_FOR_SIDE_FIELDS_LEAN(X)
#undef X
          w[34] = w[35] = 0;
        }
        w[36] = (uint32_t)e.rng; w[37] = (uint32_t)(e.rng >> 32); w[38] = e.turn | (e.last_damage << 16); w[39] = e.lm;
#pragma unroll
        for (int q = 0; q < 24; ++q) w[40 + q] = e.m[q * 64];
        w[64] = g.s0; w[65] = g.s1; w[66] = steps; w[67] = root; w[68] = result; w[69] = w[70] = w[71] = 0;
        uint4 *rec = RS_PTR(cout_state, uint4 *) + (size_t)CARRY_VEC * ((size_t)home * seg + slot);
#pragma unroll
        for (int q = 0; q < CARRY_VEC; ++q) rec[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
      } else atomicOr(RS_PTR(err, uint32_t *), 1u);
      root = NONE;
    }
  }
  if (wl == 0 && executed) atomicAdd(RS_PTR(turn_steps, unsigned long long *), (unsigned long long)executed);
#undef RS_PTR
#undef RS_U32
}
// The launch's report: report[r] = the shards' accumulators of root r added up; report[n_roots + 1] = playouts carried into the next
// step (sum over the shards, each clamped to its segment) | error word << 32.  (report[n_roots], the turn-steps, is written by the waves.)
__global__ __launch_bounds__(256) void k_root_step_report(const unsigned long long *acc, uint32_t acc_stride, uint32_t n_roots, const uint32_t *cout_count,
                                                          const uint32_t *err, uint32_t seg, unsigned long long *report) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r < n_roots) {
    unsigned long long a = 0;
#pragma unroll
    for (int s = 0; s < ROOT_SHARDS; ++s) a += acc[(size_t)s * acc_stride + r];
    report[r] = a;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    uint32_t c = threadIdx.x < ROOT_SHARDS ? cout_count[threadIdx.x * CTL_STRIDE] : 0u;
    if (c > seg) c = seg;
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) c += __shfl_down(c, o);
    if (threadIdx.x == 0) report[n_roots + 1] = (unsigned long long)c | ((unsigned long long)*err << 32);
  }
}

// ---- the libpkmn boundary: k_update, k_choices, k_init, k_random_ou ---------------------------------------------------------------
// One wave per workgroup on the register engine, its battles staged like k_rollout_staged's (STAGED_LDS_BYTES); DWORDS as stage_in's.
// This is one wave's LDS and its share of the batch.
struct BoundaryWave {
  using ER = EngineR<64, true, true>;
  lds_u32 *party, *stage;
  Tables T;
  uint32_t tid, base, lane, cnt;
  __device__ __forceinline__ BoundaryWave(uint8_t *smem, uint32_t n, bool tables = true) {
    party = (lds_u32 *)smem;
    stage = staged_rows(smem);
    T = tables ? stage_default_tables((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4) : Tables{};
    tid = threadIdx.x, base = blockIdx.x * 64, lane = base + tid;
    cnt = n - base < 64 ? n - base : 64;
  }
  __device__ __forceinline__ uint8_t *row() const { return (uint8_t *)(stage + tid * STAGE_STRIDE); } // (EngineR takes the address space back: gin_t)
  __device__ __forceinline__ ER engine() const { ER e; e.m = party + tid; e.T = T; return e; }
};

// batched pkmn_gen1_battle_update: k_tree_step_staged's update half, with the caller's override bytes
template <bool DWORDS>
__global__ __launch_bounds__(64, 2) void k_update(uint8_t *battles, const uint8_t *c1, const uint8_t *c2, uint8_t *durations, uint8_t *actions,
                                                  const uint8_t *overrides, uint32_t n, uint8_t *results) {
  extern __shared__ __align__(16) uint8_t smem[];
  const BoundaryWave w(smem, n);
  // the lane's small inputs are asked for in front of the staging: their round trip runs beside it (a batch of one is all latency)
  const bool live = w.tid < w.cnt;
  uint32_t *d = (uint32_t *)durations + 2 * (size_t)w.lane;
  uint32_t d0 = 0, d1 = 0, pc1 = 0, pc2 = 0, over1 = 0, over2 = 0;
  if (live) {
    d0 = d[0], d1 = d[1], pc1 = c1[w.lane], pc2 = c2[w.lane];
    if (overrides) over1 = overrides[(size_t)w.lane * 16], over2 = overrides[(size_t)w.lane * 16 + 8];
  }
  stage_in<DWORDS>(w.stage, battles, w.base, w.cnt);
  __syncthreads();
  if (live) {
    auto e = w.engine();
    e.load_battle_global(w.row(), d0, d1);
    e.S.misc |= over1 << 16;
    e.F.misc |= over2 << 16;
    results[w.lane] = (uint8_t)e.update(pc1, pc2);
    d[0] = e.S.dur;
    d[1] = e.F.dur;
    if (actions) {
      uint64_t *ad = (uint64_t *)actions + 2 * (size_t)w.lane;
      ad[0] = e.actS;
      ad[1] = e.actF;
    }
    e.store_battle_global(w.row());
  }
  __syncthreads();
  stage_out<DWORDS>(w.stage, battles, w.base, w.cnt);
}

template <bool DWORDS>
__global__ __launch_bounds__(64, 2) void k_choices(const uint8_t *battles, const uint8_t *results, int player, uint8_t *out, uint8_t *counts, uint32_t n) {
  extern __shared__ __align__(16) uint8_t smem[];
  const BoundaryWave w(smem, n, false); // (choices reads no table)
  const uint32_t r = w.tid < w.cnt ? results[w.lane] : 0u; // (in front of the staging, as in k_update)
  stage_in<DWORDS>(w.stage, battles, w.base, w.cnt);
  __syncthreads();
  if (w.tid < w.cnt) {
    auto e = w.engine();
    e.load_battle_global(w.row(), 0, 0); // (nor a duration)
    const auto c = e.choices(player ? e.F : e.S, player == 0 ? (r >> 4) & 3 : (r >> 6) & 3);
    counts[w.lane] = (uint8_t)c.n;
    for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) out[(size_t)w.lane * OAKGPU_MAX_CHOICES + i] = i < c.n ? (uint8_t)c.get(i) : 0;
  }
}

// ---- one level of a batch of tree descents (MCTS::Search::run_iteration, mcts.h:304-389, per lane) --------
// Applies the joint action the host-side bandits selected, reports the result, the 16-byte observation key
// (pkmn_gen1_battle_options_chance_actions: the tree edge key, mcts.h:93-98,359) and the legal choices of BOTH
// players in the new state, so that one device round trip per tree level is enough.  c1 == 0xFF: the lane's
// descent has already ended (leaf or terminal) -- its state is left untouched.  `rolls` != 39 clamps the damage
// rolls like battle_options_set (mcts.h:569-604): override bytes from the last two bytes of battle.rng.
__device__ __forceinline__ uint32_t roll_byte(uint32_t rolls, uint32_t seed) {
  if (rolls == 1) return 236;
  return 217 + (38 / (rolls - 1)) * (seed % rolls);
}
// Staged like k_rollout_staged: one wave per workgroup, its 64 battles moved between global memory and LDS with coalesced 1-KB
// accesses, 35 KB of LDS (four workgroups per CU).  A search level is a launch of 4-32 k lanes that does not fill the device: its
// time is the latency of ONE wave's turn-step (6.4 us for a dense lone wave).  Chance actions (EngineR<.., TRACK_ACTIONS>) and the
// damage-roll clamp (the override byte in SideR::misc) are the register engine's own.  DWORDS as stage_in's.
struct TreeStepArgs {
  uint8_t *battles, *durations, *results;
  const uint8_t *c1, *c2;
  uint8_t *actions, *ch1, *cnt1, *ch2, *cnt2;
  uint32_t n, rolls;
};
template <bool DWORDS>
__global__ __launch_bounds__(64, 2) void k_tree_step_staged(TreeStepArgs a) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<64, true, true>;
  Tables T = stage_default_tables((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4);
  lds_u32 *stage = staged_rows(smem);
  lds_u32 *cold = park_args(stage, a); // (k_rollout_staged: the SGPRs the pointers would hold across the turn-step are needed for exec masks)
#define TS_PTR(field, type) cold_ptr_at<type>(cold, offsetof(TreeStepArgs, field))
  const uint32_t tid = threadIdx.x, base = blockIdx.x * 64, lane = base + tid;
  const uint32_t cnt = a.n - base < 64 ? a.n - base : 64; // battles of this wave
  stage_in<DWORDS>(stage, a.battles, base, cnt);
  __syncthreads();
  const uint32_t n_all = (uint32_t)__builtin_amdgcn_readfirstlane((int)cold[offsetof(TreeStepArgs, n) / 4]);
  const uint32_t rolls = (uint32_t)__builtin_amdgcn_readfirstlane((int)cold[offsetof(TreeStepArgs, rolls) / 4]);
  const uint32_t pc1 = lane < n_all ? TS_PTR(c1, const uint8_t *)[lane] : 0xFFu;
  if (pc1 != 0xFF) {
    ER e;
    e.m = party + tid;
    e.T = T;
    uint32_t *d = TS_PTR(durations, uint32_t *) + 2 * (size_t)lane;
    e.load_battle_global((const uint8_t *)(stage + tid * STAGE_STRIDE), d[0], d[1]);
    if (rolls != 39) { // battle_options_set's clamp (mcts.h:569-604): override bytes from the last two bytes of battle.rng
      const uint32_t hi = (uint32_t)(e.rng >> 32);
      e.S.misc |= roll_byte(rolls, (hi >> 16) & 0xFF) << 16;
      e.F.misc |= roll_byte(rolls, hi >> 24) << 16;
    }
    e.actS = e.actF = 0;
    const uint32_t r = e.update(pc1, TS_PTR(c2, const uint8_t *)[lane]);
    TS_PTR(results, uint8_t *)[lane] = (uint8_t)r;
    d[0] = e.S.dur;
    d[1] = e.F.dur;
    uint64_t *ad = TS_PTR(actions, uint64_t *) + 2 * (size_t)lane;
    ad[0] = e.actS;
    ad[1] = e.actF;
#pragma unroll 1
    for (int pl = 0; pl < 2; ++pl) {
      const auto c = e.choices(pl ? e.F : e.S, pl == 0 ? (r >> 4) & 3 : (r >> 6) & 3);
      uint8_t *out = (pl ? TS_PTR(ch2, uint8_t *) : TS_PTR(ch1, uint8_t *)) + (size_t)lane * OAKGPU_MAX_CHOICES;
      (pl ? TS_PTR(cnt2, uint8_t *) : TS_PTR(cnt1, uint8_t *))[lane] = (r & 15) ? 0 : (uint8_t)c.n;
      for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) out[i] = i < c.n ? (uint8_t)c.get(i) : 0;
    }
    e.store_battle_global((uint8_t *)(stage + tid * STAGE_STRIDE));
  }
  __syncthreads();
  stage_out<DWORDS>(stage, TS_PTR(battles, uint8_t *), base, cnt);
#undef TS_PTR
}

// ---- Replay check of `.battle.data` records (oakgpu_replay_records_dev; the contract is in include/oakgpu.h) ------------------
// A replay turn is a rollout turn-step whose choices are read from the record instead of drawn, so the kernel is the queue kernel's
// shape on the register engine: persistent lanes, one game each, refilled from eight queue heads when their game ends (the queue and
// the per-frame check are record_walk.hpp's), the queue ordered longest game first by the host.  Records stay in their on-disk
// layout; a battle can start at any byte, so k_replay_gather
// first copies every stored battle to a 16-byte aligned slot (the engine's dword loads and its immutable-data pointer `gin` read
// it there) and derives the first request from it.
struct ReplayArgs {
  const uint8_t *records;   // the file bytes, unchanged
  const uint64_t *offsets;  // n: byte offset of each record
  const uint16_t *frames;   // n: frame count of each record
  const uint32_t *order;    // n_live: queue position -> record (longest first; MALFORMED records are not queued)
  const uint8_t *aligned;   // n x 384: the stored battles, aligned (k_replay_gather)
  const uint8_t *first;     // n: the first request, PKMN::result(battle)
  uint32_t *reports;        // n x 2 dwords (oakgpu_replay_report)
  uint8_t *battles_out;     // nullable, n x 384
  uint8_t *durations_out;   // nullable, n x 8
  uint32_t *heads;          // QUEUE_HEADS counters, QUEUE_HEAD_STRIDE words apart (zeroed before every launch)
  uint32_t n_live;
};
constexpr int REPLAY_COLD_BYTES = (sizeof(ReplayArgs) + 15) & ~15;
constexpr int REPLAY_LDS_BYTES = 24 * 64 * 4 + TABLE_LDS_PAD + REPLAY_COLD_BYTES;

__device__ __forceinline__ void replay_report(uint32_t *reports, uint32_t idx, uint32_t frame, uint32_t status, uint32_t player,
                                              uint32_t expected, uint32_t got) {
  *(uint2 *)(reports + 2 * (size_t)idx) = make_uint2(frame, status | (player << 8) | (expected << 16) | (got << 24)); // one 8-byte vector store
}

// One wave per record: the stored battle (byte-aligned in the record) -> its aligned slot, the first request; a MALFORMED record gets
// its report here (and zero states), it is not replayed.
__global__ __launch_bounds__(256) void k_replay_gather(ReplayArgs a, const uint8_t *malformed, uint32_t n) {
  const uint32_t rec = blockIdx.x * 4 + (threadIdx.x >> 6), wl = threadIdx.x & 63;
  if (rec >= n) return;
  if (malformed[rec]) {
    if (wl == 0) replay_report(a.reports, rec, 0, OAKGPU_REPLAY_MALFORMED, 0, 0, 0);
    if (a.battles_out) for (uint32_t j = wl; j < 96; j += 64) ((uint32_t *)(a.battles_out + (size_t)rec * 384))[j] = 0;
    if (a.durations_out && wl < 2) ((uint32_t *)(a.durations_out + (size_t)rec * 8))[wl] = 0;
    return;
  }
  const uint8_t *src = a.records + a.offsets[rec] + 6; // u32 length, u16 frame count, then the battle
  uint32_t *dst = (uint32_t *)(a.aligned + (size_t)rec * 384);
  for (uint32_t j = wl; j < 96; j += 64) dst[j] = load_u32(src + 4 * j);
  if (wl == 0) { // PKMN::result(battle) (pkmn.h:235-272)
    bool alive[2] = {false, false}, fainted[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < 6; ++i) alive[s] |= (src[184 * s + 24 * i + 18] | src[184 * s + 24 * i + 19]) != 0;
      const uint32_t o = src[184 * s + 176], i = o ? (o <= 6 ? o - 1 : 5) : 0; // (order bytes outside 1..6 do not occur in a battle)
      fainted[s] = (src[184 * s + 24 * i + 18] | src[184 * s + 24 * i + 19]) == 0;
    }
    uint32_t r;
    if (!alive[0]) r = mk_result(alive[1] ? R_LOSE : R_TIE, 0, 0);
    else if (!alive[1]) r = mk_result(R_WIN, 0, 0);
    else if (fainted[0]) r = mk_result(0, C_SWITCH, fainted[1] ? C_SWITCH : C_PASS);
    else if (fainted[1]) r = mk_result(0, C_PASS, C_SWITCH);
    else r = mk_result(0, C_MOVE, C_MOVE);
    ((uint8_t *)a.first)[rec] = (uint8_t)r;
  }
}

template <int WPS>
__global__ __launch_bounds__(64, WPS) void k_replay_records(ReplayArgs a_in) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<64, false>;
  Tables T = stage_default_tables((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4);
  lds_u32 *cold = (lds_u32 *)((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4 + TABLE_LDS_PAD); // the arguments, parked (cold_ptr_at)
  if (threadIdx.x < sizeof(ReplayArgs) / 4) cold[threadIdx.x] = ((const uint32_t *)&a_in)[threadIdx.x];
  __syncthreads();
#define RA_PTR(field, type) cold_ptr_at<type>(cold, offsetof(ReplayArgs, field))
  const uint32_t wl = threadIdx.x & 63;
  const uint32_t n_live = (uint32_t)__builtin_amdgcn_readfirstlane((int)cold[offsetof(ReplayArgs, n_live) / 4]);
  ER e;
  e.m = party + threadIdx.x;
  e.T = T;
  uint32_t idx = LANE_NONE, r = 0, k = 0, nf = 0, mn = 0, c1 = 0, c2 = 0;
  const uint8_t *fp = nullptr; // the next frame of this lane's record
  uint32_t ust = queue_state(blockIdx.x);
  for (;;) {
    const bool need = idx == LANE_NONE;
    const uint64_t mask = __ballot(need);
    bool load = false;
    if (refill_due(ust, mask, __ballot(idx < LANE_DONE) != 0)) {
      uint32_t my = 0;
      const bool got = queue_take(ust, cold, offsetof(ReplayArgs, heads), n_live, need, mask, wl, my);
      if (need) {
        if (got) { idx = RA_PTR(order, const uint32_t *)[my]; load = true; }
        else idx = LANE_DONE;
      }
    } else if (need && queue_dry(ust)) idx = LANE_DONE;
    if (__ballot(load)) {
      if (load) {
        e.load_battle_global(RA_PTR(aligned, const uint8_t *) + (size_t)idx * 384, 0, 0); // zero durations (frames.h:57-59)
        r = RA_PTR(first, const uint8_t *)[idx];
        nf = RA_PTR(frames, const uint16_t *)[idx];
        fp = RA_PTR(records, const uint8_t *) + RA_PTR(offsets, const uint64_t *)[idx] + 391;
        k = 0;
        if (nf) { mn = fp[0]; c1 = fp[1]; c2 = fp[2]; }
      }
    }
    if (__ballot(idx != LANE_DONE) == 0) break;
    if (idx < LANE_DONE) {
      Verdict v{STATUS_PENDING, 0, 0, 0};
      if (k == nf) { // after the last frame
        v.expected = RA_PTR(records, const uint8_t *)[RA_PTR(offsets, const uint64_t *)[idx] + 390];
        v.status = r == v.expected ? OAKGPU_REPLAY_OK : OAKGPU_REPLAY_RESULT;
        v.got = r;
      } else if (r & 15) {
        v.expected = RA_PTR(records, const uint8_t *)[RA_PTR(offsets, const uint64_t *)[idx] + 390];
        v.status = OAKGPU_REPLAY_EARLY_END;
        v.got = r;
      } else {
        typename ER::Choices l1, l2;
        v = frame_check(e, r, mn, c1, c2, l1, l2);
        if (v.status == STATUS_PENDING) {
          r = play_frame(e, fp, mn, c1, c2, k + 1 < nf);
          ++k;
        }
      }
      if (v.status != STATUS_PENDING) { // the verdict: report, state at the verdict, lane free
        replay_report(RA_PTR(reports, uint32_t *), idx, k, v.status, v.player, v.expected, v.got);
        uint8_t *bout = RA_PTR(battles_out, uint8_t *);
        if (bout) e.store_battle_global(bout + (size_t)idx * 384);
        uint32_t *dout = RA_PTR(durations_out, uint32_t *);
        if (dout) *(uint2 *)(dout + 2 * (size_t)idx) = make_uint2(e.S.dur, e.F.dur);
        idx = LANE_NONE;
      }
    }
  }
#undef RA_PTR
}

// ---- PokeEngine::Eval (cpp/include/search/poke-engine-evaluate.h:9-204): the hand-written fp32 position score the
// reference uses as its default data-generation evaluator.  One lane per battle, straight from the AoS bytes.
__device__ __forceinline__ float pe_boost(uint32_t nib) { // get_boost_multiplier (:52-85) of a 4-bit two's-complement stage
  const int st = (int)((nib ^ 8) - 8);
  const int a = st < 0 ? -st : st;
  const float m = a == 0 ? 0.0f : a == 1 ? 1.0f : a == 2 ? 2.0f : a == 3 ? 2.5f : a == 4 ? 3.0f : a == 5 ? 3.15f : 3.3f;
  return st < 0 ? -m : m;
}
__device__ __forceinline__ float pe_pokemon(const uint8_t *pk) { // evaluate_pokemon (:131-140), pk = 24 stored bytes
  const uint32_t hp = pk[18] | (pk[19] << 8);
  if (hp == 0) return 0.0f;
  const uint32_t maxhp = pk[0] | (pk[1] << 8), status = pk[20];
  float score = (100.0f * (float)hp) / (float)maxhp;
  float st = 0.0f; // evaluate_status (:106-129)
  if (status == ST_BRN) { // evaluate_burned (:87-104)
    float mult = 0.0f;
    for (int m = 0; m < 4; ++m) {
      const uint32_t w = OAK_MOVE_WORDS[pk[10 + 2 * m]];
      if (((w >> 8) & 0xFF) > 0 && ((w >> 16) & 0xFF) < 8) mult += 1.0f;
    }
    const uint32_t atk = pk[2] | (pk[3] << 8), spc = pk[8] | (pk[9] << 8);
    if (spc > atk) mult *= 0.5f;
    st = mult * -25.0f;
  } else if (status == ST_FRZ) st = -40.0f;
  else if (status == ST_PAR) st = -25.0f;
  else if (status == ST_TOX) st = -30.0f;
  else if (status == ST_PSN) st = -10.0f;
  else if (status & 7) st = -25.0f;
  score += st;
  score = fmaxf(score, 0.0f);
  return score + 30.0f;
}
__device__ __forceinline__ float pe_side(const uint8_t *side) { // evaluate_side / evaluate_active (:142-184)
  float score = 0.0f;
  const uint32_t aid = side[176];
  const uint8_t *stored = side + 24 * (aid ? aid - 1 : 0); // Side::stored(): pokemon[order[0] - 1]
  const uint32_t shp = aid ? (stored[18] | (stored[19] << 8)) : 0;
  if (shp) {
    score += pe_pokemon(stored);
    const uint8_t *ac = side + 144;
    const uint32_t vlo = ac[16] | (ac[17] << 8) | (ac[18] << 16);
    if (vlo & V_LEECHSEED) score += -30.0f;
    if (vlo & V_SUBSTITUTE) score += 40.0f;
    if (vlo & V_CONFUSION) score += -20.0f;
    if (vlo & V_REFLECT) score += 20.0f;
    if (vlo & V_LIGHTSCREEN) score += 20.0f;
    score += 30.0f * pe_boost(ac[12] & 15);   // atk
    score += 15.0f * pe_boost(ac[12] >> 4);   // def
    score += 30.0f * pe_boost(ac[13] >> 4);   // spc
    score += 30.0f * pe_boost(ac[13] & 15);   // spe
  }
  for (int slot = 2; slot <= 6; ++slot) {
    const uint32_t id = side[176 + slot - 1];
    if (id != 0) score += pe_pokemon(side + 24 * (id - 1));
  }
  return score;
}
__global__ void k_poke_engine(const uint8_t *battles, uint32_t n, float root_score, float *values, float *scores) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t *b = battles + (size_t)i * 384;
  const float score = pe_side(b) - pe_side(b + 184);
  if (scores) scores[i] = score;
  if (values) values[i] = 1.0f / (1.0f + expf(-0.0125f * (score - root_score))); // scaled_sigmoid (:11-13), Eval::evaluate (:195-201)
}

// ---- PKMN::battle / Init::init_side (cpp/include/libpkmn/init.h:35-40,90-154) ---------------
template <class E>
__device__ void init_from_teams(E &e, const uint8_t *teams /* 60 B, this lane */, uint32_t seed_lo, uint32_t seed_hi) {
  for (int w = 0; w < STATE_WORDS; ++w) e.w32(4 * w, 0);
  for (int s = 0; s < 2; ++s) {
    const int so = s * SIDE_SZ;
    for (int i = 0; i < 6; ++i) {
      const uint8_t *set = teams + (s * 6 + i) * 5;
      const int pk = so + PK_SZ * i;
      const uint32_t sp = set[0];
      e.w8(pk + P_SPECIES, sp);
      if (sp == 0) { if (i == 0) e.w8(so + O_ORDER, 1); continue; }
      const uint32_t w0 = e.T.sp0[sp], w1 = e.T.sp1[sp];
      const uint32_t level = 100;
      auto stat = [&](uint32_t base, bool hp) { return (2 * (base + 15) + 63) * level / 100 + (hp ? level + 10 : 5); };
      const uint32_t hp = stat(w0 & 0xFF, true);
      e.w16(pk + P_HP_MAX, hp);
      e.w16(pk + P_ATK, stat((w0 >> 8) & 0xFF, false));
      e.w16(pk + P_DEF, stat((w0 >> 16) & 0xFF, false));
      e.w16(pk + P_SPE, stat(w0 >> 24, false));
      e.w16(pk + P_SPC, stat(w1 & 0xFF, false));
      for (int mi = 0; mi < 4; ++mi) {
        const uint32_t id = set[1 + mi];
        e.w8(pk + P_MOVES + 2 * mi, id);
        e.w8(pk + P_MOVES + 2 * mi + 1, id ? e.T.maxpp[id] : 0);
      }
      e.w16(pk + P_HP, hp);
      e.w8(pk + P_TYPES, ((w1 >> 8) & 0xFF) | (((w1 >> 16) & 0xFF) << 4));
      e.w8(pk + P_LEVEL, level);
      e.w8(so + O_ORDER + i, i + 1);
    }
  }
  e.w32(B_RNG, seed_lo);
  e.w32(B_RNG + 4, seed_hi);
}
// what init_from_teams writes through: this lane's staged row (bytes and dwords only: the engine reads the row as dwords)
struct RowWriter {
  lds_u8 *row;
  Tables T;
  __device__ __forceinline__ void w8(int off, uint32_t v) { row[off] = (uint8_t)v; }
  __device__ __forceinline__ void w16(int off, uint32_t v) { w8(off, v); w8(off + 1, v >> 8); }
  __device__ __forceinline__ void w32(int off, uint32_t v) { *(lds_u32 *)(row + off) = v; }
};
// A lane's new battle from its teams into its staged row, the opening update if asked for, and the outputs (both nullable).  The
// row is the lane's own: its LDS writes and the engine's reads stay in order without a barrier.
__device__ __forceinline__ void open_battle(const BoundaryWave &w, const uint8_t *teams, uint32_t seed_lo, uint32_t seed_hi, bool first_update,
                                            uint8_t *durations, uint8_t *results) {
  RowWriter rw{(lds_u8 *)(w.stage + w.tid * STAGE_STRIDE), w.T};
  init_from_teams(rw, teams, seed_lo, seed_hi);
  uint32_t r = mk_result(0, C_MOVE, C_MOVE), d0 = 0, d1 = 0;
  if (first_update) {
    auto e = w.engine();
    e.load_battle_global(w.row(), 0, 0);
    r = e.update(0, 0);
    e.store_battle_global(w.row());
    d0 = e.S.dur;
    d1 = e.F.dur;
  }
  if (results) results[w.lane] = (uint8_t)r;
  if (durations) {
    uint32_t *d = (uint32_t *)durations + 2 * (size_t)w.lane;
    d[0] = d0;
    d[1] = d1;
  }
}

template <bool DWORDS>
__global__ __launch_bounds__(64, 2) void k_init(const uint8_t *teams, const uint64_t *seeds, uint32_t n, int first_update, uint8_t *battles,
                                                uint8_t *durations, uint8_t *results) {
  extern __shared__ __align__(16) uint8_t smem[];
  // the lane's seed and teams are asked for in front of the table copy: their round trip runs beside it (a batch of one is all latency)
  const uint32_t lane = blockIdx.x * 64 + threadIdx.x;
  uint64_t sd = 0;
  uint8_t mine[OAKGPU_TEAMS_SIZE];
  if (lane < n) {
    sd = seeds[lane];
#pragma unroll
    for (int i = 0; i < OAKGPU_TEAMS_SIZE; ++i) mine[i] = teams[(size_t)lane * OAKGPU_TEAMS_SIZE + i];
  }
  const BoundaryWave w(smem, n);
  __syncthreads();
  if (w.tid < w.cnt) open_battle(w, mine, (uint32_t)sd, (uint32_t)(sd >> 32), first_update != 0, durations, results);
  __syncthreads();
  stage_out<DWORDS>(w.stage, battles, w.base, w.cnt);
}

template <bool DWORDS>
__global__ __launch_bounds__(64, 2) void k_random_ou(uint64_t seed0, uint32_t n, const uint8_t *legal, int n_legal, const uint8_t *pools,
                                                     const uint8_t *sizes, uint8_t *battles, uint8_t *durations, uint8_t *prng, uint8_t *results) {
  extern __shared__ __align__(16) uint8_t smem[];
  const BoundaryWave w(smem, n);
  __syncthreads();
  if (w.tid < w.cnt) {
    FastPrng g;
    g.seed(seed0 + w.lane);
    uint8_t teams[OAKGPU_TEAMS_SIZE];
    for (int i = 0; i < OAKGPU_TEAMS_SIZE; ++i) teams[i] = 0;
    for (int s = 0; s < 2; ++s)
      for (int k = 0; k < 6; ++k) {
        uint32_t sp;
        for (;;) {
          sp = legal[g.next32() % (uint32_t)n_legal];
          bool dup = false;
          for (int j = 0; j < k; ++j) dup |= teams[(s * 6 + j) * 5] == sp;
          if (!dup) break;
        }
        uint8_t *set = teams + (s * 6 + k) * 5;
        set[0] = (uint8_t)sp;
        const uint32_t psz = sizes[sp];
        const uint32_t want = psz < 4 ? psz : 4;
        for (uint32_t mi = 0; mi < want; ++mi) {
          for (;;) {
            uint32_t mvid = pools[sp * 48 + g.next32() % psz];
            bool dup = false;
            for (uint32_t j = 0; j < mi; ++j) dup |= set[1 + j] == mvid;
            if (!dup) { set[1 + mi] = (uint8_t)mvid; break; }
          }
        }
      }
    const uint32_t hi = g.next32(), lo = g.next32();
    open_battle(w, teams, lo, hi, true, durations, results);
    uint32_t *pd = (uint32_t *)prng + 2 * (size_t)w.lane;
    pd[0] = g.s0;
    pd[1] = g.s1;
  }
  __syncthreads();
  stage_out<DWORDS>(w.stage, battles, w.base, w.cnt);
}

} // namespace oak

// =================================== C ABI ==================================================
struct oakgpu_ctx {
  int device;
  hipStream_t stream;
  bool own_stream;
  uint8_t *d_legal, *d_pools, *d_sizes;
  int n_legal;
  int playouts_per_lane; // > 1: persistent grid of n / this lanes with queue refill (k_rollout_queue)
  uint32_t *d_queue;      // 64 counters: suspended-playout counts of the regrouping rounds, queue-order counters, migration control block
  uint32_t *d_heads;      // the queue kernel's heads: MAX_ROUNDS rounds x 8 heads, each on a 256-byte line of its own
  int rounds;             // regrouping rounds of the queue kernel (1 = none)
  int suspend_below;      // a dry wave with fewer live lanes than this hands them to the next round
  int round_shrink;       // each round launches 1/round_shrink of the previous round's waves
  uint8_t *d_scratch;     // suspended playout state: n x (384 + 8 + 1) bytes + two n-entry index lists
  size_t scratch_n;
  int rounds_auto;        // 1 (default): every launch is one dispatch; 0 after oakgpu_set_regroup: the rounds it asked for
  int concurrent_hint;    // set by callers that keep several contexts busy at once (the tree search): small launches run in rounds
  int search_party_table; // oakgpu_set_search_party_table: the tree search's network evaluations look bench slots up in a per-search table
  uint64_t search_table_fills = 0, search_table_evals = 0; // oakgpu_search_party_table_stats
  const void *ws2_owner = nullptr; // the party table whose eval wrote workspace 2's counters last (null: someone else did)
  int tail_below;         // > 0: a SATURATED launch parks the lanes of dry waves with fewer live lanes than this and ONE follow-up
  int tail_waves;         //      dispatch of this many waves (0 = one per CU) finishes them, a few to a wave (the tail)
  int tail_lanes;         //      lanes per wave of that dispatch that take playouts (0 = all 64)
  int migrate;            // long-playout migration (k_rollout_queue): 0 off, 1 (default) for launches that saturate the device, 2 always
  int migrate_steps;      //   a bulk wave donates a playout still running after this many turn-steps (default 300)
  int migrate_adopters;   //   adopter waves (0 = one per four CUs)
  int migrate_window;     //   ... or whose actives' {slot, hp} stood still for this many turn-steps (0 = off, at most 255)
  int migrate_used;       //   the last queue launch ran with migration: oakgpu_synchronize reports its error word
  int spread_lanes;       // launches that do not fill the device: lanes per wave that take playouts (-1 automatic, 0 / 64 = all)
  int queue_order;        // 1 (default): a saturated launch hands its playouts out likely-longest first (k_queue_order)
  int standstill_skip;    // 1 (default): the queue kernel takes a PROVEN inert standstill to its last turn-step in one go (exact); 0: plays every turn
  int move_carry;         // 0..64 (oakgpu_set_move_carry): the queue kernel's move carry, 0 = a turn's two actions in one wave iteration
  int move_carry_dry;     // 0..64 (oakgpu_set_move_carry_dry): a dry bulk wave carries while at least this many lanes play, 0 = never
  int lean_rollout;       // 1 (default, oakgpu_set_lean_rollout): a group launch none of whose batches takes durations back runs the queue kernel that keeps none
  int last_launch_lean;   // the last group launch ran that kernel (oakgpu_last_launch_lean)
  // The yielding schedule (oakgpu_set_yield_schedule): a context that alternates saturating group launches with
  // another context of its device launches R waves FEWER than the device holds, its dry waves park their last lanes and leave, and ONE
  // follow-up dispatch of at most R waves finishes the parked playouts in the slots the other context's launch leaves free.  Migration
  // is off in it: no wave ever waits for another, so it is correct whatever part of a grid is resident.
  int yield_mode;         // 0 off, 1 automatic (below), 2 every group launch of two waves or more (tests reach it at small sizes)
  int yield_below;        //   a dry wave with fewer playing lanes than this parks them
  int yield_waves;        //   R (0 = one per CU)
  int yield_lanes;        //   lanes per follow-up wave that take playouts (0 = all 64)
  int yield_min_waves;    //   automatic: a launch of this many waves counts as saturating (0 = the device's resident waves; tests lower it)
  uint64_t sat_seq = 0;   //   the registry's sequence number of this context's last saturating group launch (0: none yet)
  int last_launch_yield;  // the last group launch took the yielding schedule (oakgpu_last_launch_yield)
  int last_launch_rounds; // dispatches of the last group launch: with more than one, control word 1 is its parked count
  uint32_t *d_order;      // total entries
  size_t order_n;
  uint32_t order_pair = 0;      // k_queue_order's two counters: control words 32-33 and 34-35 in turn (each launch clears the next one's)
  uint32_t ticket_epoch = 0;    // migrating launches of this context: tags the adoption tickets (RoundArgs::epoch)
  bool tickets_dirty = true;    // the ticket list holds something else (fresh scratch, a regrouping round's lists): ONE clearing, then epochs again
  int n_cu;               // compute units of the device
  static constexpr int TABLE_SLOTS = 8;
  void *h_table, *d_table; // batch tables of the group launches: pinned host ring -> device ring
  hipEvent_t table_ev[TABLE_SLOTS];
  uint64_t table_next;
  struct Block { void *p; size_t cap; };
  std::vector<Block> stage; // staging buffers of the host-pointer entry points (oakgpu_internal.h)
  size_t stage_cursor;
  Block ws[3];              // leaf-evaluator workspaces: embeddings, policy activations, party work list
  int timing;               // oakgpu_set_kernel_timing
  hipEvent_t tev[4];
  bool tev_valid;
  Block replay_ws{nullptr, 0};             // oakgpu_replay_records_dev: queue heads, queue order, first requests, aligned battles
  Block games_ws{nullptr, 0};              // oakgpu_policy_games_dev (policyplay.hip): the resident rows, both halves, and the per-turn arrays
  void *attachment = nullptr;              // oakgpu_internal.h: the tree search's cached batch slots
  void (*attachment_dtor)(void *) = nullptr;
};

// Saturating group launches, per process: which context of a device issued one last (host side only -- no device query, no
// synchronisation).  Automatic yielding applies to a context whose previous saturating launch has been followed by another live
// context's on the same device: the two alternate, so each one's tail runs beside the other one's bulk phase.
static std::mutex g_yield_mu;
static std::vector<oakgpu_ctx *> g_live_ctx;
static uint64_t g_sat_seq = 0;
static void yield_registry_add(oakgpu_ctx *c) { std::lock_guard<std::mutex> lock(g_yield_mu); g_live_ctx.push_back(c); }
static void yield_registry_remove(oakgpu_ctx *c) {
  std::lock_guard<std::mutex> lock(g_yield_mu);
  for (size_t i = 0; i < g_live_ctx.size(); ++i) if (g_live_ctx[i] == c) { g_live_ctx[i] = g_live_ctx.back(); g_live_ctx.pop_back(); break; }
}
// notes a saturating group launch of `c`; true when another live context of its device has issued one since c's previous one
static bool yield_registry_launch(oakgpu_ctx *c) {
  std::lock_guard<std::mutex> lock(g_yield_mu);
  bool other = false;
  if (c->sat_seq) for (const oakgpu_ctx *o : g_live_ctx) other |= o != c && o->device == c->device && o->sat_seq > c->sat_seq;
  c->sat_seq = ++g_sat_seq;
  return other;
}

static thread_local std::string g_err;
static int fail(hipError_t e, const char *what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return (int)e;
}
static int bad(const char *what) {
  g_err = what;
  return -1;
}
int oakgpu_fail_hip(int e, const char *what) { return fail((hipError_t)e, what); }
int oakgpu_fail_msg(const char *what) { return bad(what); }
int oakgpu_ctx_device(const oakgpu_ctx *c) { return c->device; }
int oakgpu_ctx_enter(oakgpu_ctx *c) {
  hipError_t e = hipSetDevice(c->device);
  return e == hipSuccess ? 0 : fail(e, "hipSetDevice");
}
static void *grow_block(oakgpu_ctx *c, oakgpu_ctx::Block &b, size_t bytes) {
  if (b.cap >= bytes && b.p) return b.p;
  if (b.p) { // a launch on this context's stream may still use the old block
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
  }
  const size_t cap = (bytes + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
  hipError_t e = hipMalloc(&b.p, cap);
  if (e != hipSuccess) { b.p = nullptr; fail(e, "hipMalloc(context buffer)"); return nullptr; }
  b.cap = cap;
  return b.p;
}
void **oakgpu_ctx_timing_events(oakgpu_ctx *c) { return c->timing && c->tev_valid ? (void **)c->tev : nullptr; }
void *oakgpu_ctx_workspace(oakgpu_ctx *c, int slot, size_t bytes) {
  if (slot % 3 == 2) c->ws2_owner = nullptr; // (whoever asks for the work-list block is about to write its head)
  return grow_block(c, c->ws[slot % 3], bytes ? bytes : 1);
}
void *oakgpu_ctx_games_workspace(oakgpu_ctx *c, size_t bytes) { return grow_block(c, c->games_ws, bytes ? bytes : 1); }
void oakgpu_ctx_set_ws2_owner(oakgpu_ctx *c, const void *table) { c->ws2_owner = table; }
const void *oakgpu_ctx_ws2_owner(const oakgpu_ctx *c) { return c->ws2_owner; }
void oakgpu_ctx_count_search_table(oakgpu_ctx *c, uint64_t fills, uint64_t evals) { c->search_table_fills += fills; c->search_table_evals += evals; }
void oakgpu_stage_begin(oakgpu_ctx *c) { c->stage_cursor = 0; }
void oakgpu_stage_end(oakgpu_ctx *c) { (void)hipStreamSynchronize(c->stream); }
void *oakgpu_stage_get(oakgpu_ctx *c, size_t bytes) {
  if (c->stage_cursor >= c->stage.size()) c->stage.push_back(oakgpu_ctx::Block{nullptr, 0});
  return grow_block(c, c->stage[c->stage_cursor++], bytes ? bytes : 1);
}
void *oakgpu_ctx_stream(const oakgpu_ctx *c) { return (void *)c->stream; }
int oakgpu_ctx_set_concurrent_hint(oakgpu_ctx *c, int on) { const int old = c->concurrent_hint; c->concurrent_hint = on; return old; }
int oakgpu_ctx_search_party_table(const oakgpu_ctx *c) { return c->search_party_table; }
void *oakgpu_ctx_attachment(const oakgpu_ctx *c) { return c->attachment; }
void oakgpu_ctx_set_attachment(oakgpu_ctx *c, void *p, void (*dtor)(void *)) {
  if (c->attachment && c->attachment_dtor) c->attachment_dtor(c->attachment);
  c->attachment = p;
  c->attachment_dtor = dtor;
}
#undef HIPCHK // (oakgpu_internal.h's form: this file's errors go through its own fail())
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(_e, #x); } while (0)

// ---- host-buffer conveniences (PCIe-inclusive; never the benchmarked path) ------------------
namespace {
struct DevBuf { // one staging buffer of the current host call (owned by the context's grow-only cache)
  void *p = nullptr;
  size_t bytes = 0;
  hipError_t alloc(size_t b, oakgpu_ctx *c) { bytes = b; p = oakgpu_stage_get(c, b); return p ? hipSuccess : hipErrorOutOfMemory; }
};
} // namespace

extern "C" {

const char *oakgpu_last_error(void) { return g_err.c_str(); }

int oakgpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// the queue kernel runs four one-wave workgroups per SIMD: sixteen of them must fit in a CU's 160 KiB of LDS
static_assert(24 * 64 * 4 + oak::TABLE_LDS_PAD + oak::COLD_LDS_BYTES <= 160 * 1024 / 16, "k_rollout_queue<64, 4>: sixteen workgroups no longer fit in a CU's LDS");
static int set_lds_limits() {
  HIPCHK(hipFuncSetAttribute((const void *)oak::k_rollout_regs<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 24 * 64 * 4 + oak::TABLE_LDS_PAD));
  HIPCHK(hipFuncSetAttribute((const void *)oak::k_rollout_staged, hipFuncAttributeMaxDynamicSharedMemorySize, oak::STAGED_LDS_BYTES));
  HIPCHK(hipFuncSetAttribute((const void *)oak::k_rollout_draws<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 24 * 64 * 4 + oak::TABLE_LDS_PAD));
  HIPCHK(hipFuncSetAttribute((const void *)oak::k_rollout_queue<64, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, 24 * 64 * 4 + oak::TABLE_LDS_PAD + oak::COLD_LDS_BYTES));
  HIPCHK(hipFuncSetAttribute((const void *)oak::k_rollout_queue<64, 4, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 24 * 64 * 4 + oak::TABLE_LDS_PAD + oak::COLD_LDS_BYTES));
  HIPCHK(hipFuncSetAttribute((const void *)oak::k_rollout_queue<64, 4, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 24 * 64 * 4 + oak::TABLE_LDS_PAD + oak::COLD_LDS_BYTES));
#define STAGED_LIMIT(kernel)                                                                                                           \
  HIPCHK(hipFuncSetAttribute((const void *)oak::kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, oak::STAGED_LDS_BYTES)); \
  HIPCHK(hipFuncSetAttribute((const void *)oak::kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, oak::STAGED_LDS_BYTES))
  STAGED_LIMIT(k_update);
  STAGED_LIMIT(k_choices);
  STAGED_LIMIT(k_tree_step_staged);
  STAGED_LIMIT(k_init);
  STAGED_LIMIT(k_random_ou);
#undef STAGED_LIMIT
  return 0;
}

// A staged kernel over n battles, one wave per 64: its 16-byte form, or its dword form when `battles` sits on a 4-byte boundary only.
#define LAUNCH_STAGED(kernel, battles, n, ...)                                                                                          \
  do {                                                                                                                                  \
    if (((uintptr_t)(battles) & 15) == 0) hipLaunchKernelGGL(oak::kernel<false>, dim3(((n) + 63) / 64), dim3(64), oak::STAGED_LDS_BYTES, c->stream, __VA_ARGS__); \
    else hipLaunchKernelGGL(oak::kernel<true>, dim3(((n) + 63) / 64), dim3(64), oak::STAGED_LDS_BYTES, c->stream, __VA_ARGS__);             \
    HIPCHK(hipGetLastError());                                                                                                          \
  } while (0)

int oakgpu_create(oakgpu_ctx **out, int device) {
  if (!out) return bad("oakgpu_create: null out");
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (n <= 0) return bad("oakgpu_create: no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= n) return bad("oakgpu_create: device index out of range");
  HIPCHK(hipSetDevice(device));
  {
    // per-DEVICE initialisation, once per process and device (round-2 advice: every context repeated it, on the NULL stream):
    // kernel attributes, and the engine's table image built on a non-blocking stream of its own -- it neither serialises
    // with the caller's blocking streams nor rewrites the image under another context's running kernels
    static std::mutex init_mu;
    static bool init_done[64] = {};
    std::lock_guard<std::mutex> lock(init_mu);
    if (device >= 64 || !init_done[device]) {
      if (int r = set_lds_limits()) return r;
      if (int r = oakgpu_leaf_set_lds_limits()) return r;
      hipStream_t s0;
      HIPCHK(hipStreamCreateWithFlags(&s0, hipStreamNonBlocking));
      hipLaunchKernelGGL(oak::k_build_table_image, dim3(1), dim3(64), oak::TABLE_LDS_PAD, s0);
      hipError_t le = hipGetLastError();
      hipError_t se = hipStreamSynchronize(s0);
      (void)hipStreamDestroy(s0);
      if (le != hipSuccess) return fail(le, "k_build_table_image launch");
      if (se != hipSuccess) return fail(se, "k_build_table_image");
      if (device < 64) init_done[device] = true;
    }
  }
  oakgpu_ctx *c = new oakgpu_ctx();
  c->device = device;
  c->own_stream = true;
  c->d_legal = c->d_pools = c->d_sizes = nullptr;
  c->n_legal = 0;
  c->playouts_per_lane = 2;
  if (const char *env = getenv("OAKGPU_PLAYOUTS_PER_LANE")) c->playouts_per_lane = atoi(env) > 0 ? atoi(env) : 1;
  c->d_queue = nullptr;
  c->d_heads = nullptr;
  c->d_scratch = nullptr;
  c->scratch_n = 0;
  c->h_table = c->d_table = nullptr;
  c->table_next = 0;
  c->stage_cursor = 0;
  c->ws[0] = c->ws[1] = c->ws[2] = oakgpu_ctx::Block{nullptr, 0};
  c->timing = 0;
  c->tev_valid = false;
  c->rounds_auto = 1;
  c->concurrent_hint = 0;
  c->search_party_table = 0;
  if (const char *env = getenv("OAKGPU_PARTY_TABLE")) c->search_party_table = atoi(env) != 0;
  if (const char *env = getenv("OAKGPU_ROUNDS_AUTO")) c->rounds_auto = atoi(env) != 0;
  {
    hipDeviceProp_t prop;
    hipError_t pe = hipGetDeviceProperties(&prop, device);
    if (pe != hipSuccess) { delete c; return fail(pe, "hipGetDeviceProperties"); }
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  c->rounds = 4;
  c->suspend_below = 32;
  c->round_shrink = 3;
  c->tail_below = 0;
  c->tail_waves = 0;
  if (const char *env = getenv("OAKGPU_TAIL_BELOW")) c->tail_below = atoi(env) < 0 ? 0 : atoi(env) > 64 ? 64 : atoi(env);
  if (const char *env = getenv("OAKGPU_TAIL_WAVES")) c->tail_waves = atoi(env) < 0 ? 0 : atoi(env);
  c->spread_lanes = -1; // automatic
  if (const char *env = getenv("OAKGPU_SPREAD_LANES")) c->spread_lanes = atoi(env) < -1 ? -1 : atoi(env) > 64 ? 64 : atoi(env);
  c->queue_order = 1;
  if (const char *env = getenv("OAKGPU_QUEUE_ORDER")) c->queue_order = atoi(env) != 0;
  c->standstill_skip = 1;
  if (const char *env = getenv("OAKGPU_STANDSTILL_SKIP")) c->standstill_skip = atoi(env) != 0;
  c->move_carry = OAKGPU_MOVE_CARRY_DEFAULT;
  if (const char *env = getenv("OAKGPU_MOVE_CARRY")) c->move_carry = atoi(env) < 0 ? 0 : atoi(env) > 64 ? 64 : atoi(env);
  c->move_carry_dry = OAKGPU_MOVE_CARRY_DRY_DEFAULT;
  if (const char *env = getenv("OAKGPU_MOVE_CARRY_DRY")) c->move_carry_dry = atoi(env) < 0 ? 0 : atoi(env) > 64 ? 64 : atoi(env);
  c->lean_rollout = OAKGPU_LEAN_ROLLOUT_DEFAULT;
  if (const char *env = getenv("OAKGPU_LEAN_ROLLOUT")) c->lean_rollout = atoi(env) != 0;
  c->last_launch_lean = 0;
  c->yield_mode = OAKGPU_YIELD_SCHEDULE_DEFAULT;
  c->yield_below = OAKGPU_YIELD_BELOW_DEFAULT;
  c->yield_waves = OAKGPU_YIELD_WAVES_DEFAULT;
  c->yield_lanes = OAKGPU_YIELD_LANES_DEFAULT;
  c->yield_min_waves = 0;
  c->last_launch_yield = c->last_launch_rounds = 0;
  if (const char *env = getenv("OAKGPU_YIELD_SCHEDULE")) c->yield_mode = atoi(env) < 0 ? 0 : atoi(env) > 2 ? 2 : atoi(env);
  if (const char *env = getenv("OAKGPU_YIELD_BELOW")) c->yield_below = atoi(env) < 1 ? 1 : atoi(env) > 64 ? 64 : atoi(env);
  if (const char *env = getenv("OAKGPU_YIELD_WAVES")) c->yield_waves = atoi(env) < 0 ? 0 : atoi(env);
  if (const char *env = getenv("OAKGPU_YIELD_LANES")) c->yield_lanes = atoi(env) < 0 ? 0 : atoi(env) > 64 ? 64 : atoi(env);
  c->migrate = 1;
  c->migrate_steps = 300;
  c->migrate_adopters = 0;
  c->migrate_window = 48;
  c->migrate_used = 0;
  if (const char *env = getenv("OAKGPU_MIGRATE")) c->migrate = atoi(env) < 0 ? 0 : atoi(env) > 2 ? 2 : atoi(env);
  if (const char *env = getenv("OAKGPU_MIGRATE_STEPS")) c->migrate_steps = atoi(env) < 1 ? 1 : atoi(env);
  if (const char *env = getenv("OAKGPU_MIGRATE_ADOPTERS")) c->migrate_adopters = atoi(env) < 0 ? 0 : atoi(env);
  if (const char *env = getenv("OAKGPU_MIGRATE_WINDOW")) c->migrate_window = atoi(env) < 0 ? 0 : atoi(env) > 255 ? 255 : atoi(env);
  c->d_order = nullptr;
  c->order_n = 0;
  c->tail_lanes = 0;
  if (const char *env = getenv("OAKGPU_TAIL_LANES")) c->tail_lanes = atoi(env) < 0 ? 0 : atoi(env) > 64 ? 64 : atoi(env);
  if (const char *env = getenv("OAKGPU_ROUNDS")) c->rounds = atoi(env) < 1 ? 1 : atoi(env) > 8 ? 8 : atoi(env);
  if (const char *env = getenv("OAKGPU_SUSPEND_BELOW")) c->suspend_below = atoi(env) < 0 ? 0 : atoi(env) > 64 ? 64 : atoi(env);
  if (const char *env = getenv("OAKGPU_ROUND_SHRINK")) c->round_shrink = atoi(env) < 1 ? 1 : atoi(env);
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return fail(e, "hipStreamCreate"); }
  yield_registry_add(c);
  *out = c;
  return 0;
}

void oakgpu_destroy(oakgpu_ctx *c) {
  if (!c) return;
  yield_registry_remove(c);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->attachment && c->attachment_dtor) { c->attachment_dtor(c->attachment); c->attachment = nullptr; }
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  if (c->d_legal) (void)hipFree(c->d_legal);
  if (c->d_pools) (void)hipFree(c->d_pools);
  if (c->d_sizes) (void)hipFree(c->d_sizes);
  if (c->d_queue) (void)hipFree(c->d_queue);
  if (c->d_heads) (void)hipFree(c->d_heads);
  if (c->d_scratch) (void)hipFree(c->d_scratch);
  if (c->d_order) (void)hipFree(c->d_order);
  for (auto &b : c->stage) if (b.p) (void)hipFree(b.p);
  for (auto &b : c->ws) if (b.p) (void)hipFree(b.p);
  if (c->replay_ws.p) (void)hipFree(c->replay_ws.p);
  if (c->games_ws.p) (void)hipFree(c->games_ws.p);
  if (c->tev_valid) for (auto &e : c->tev) (void)hipEventDestroy(e);
  if (c->h_table) {
    (void)hipHostFree(c->h_table);
    (void)hipFree(c->d_table);
    for (int i = 0; i < oakgpu_ctx::TABLE_SLOTS; ++i) (void)hipEventDestroy(c->table_ev[i]);
  }
  delete c;
}

int oakgpu_set_stream(oakgpu_ctx *c, void *hip_stream) {
  if (!c) return bad("null ctx");
  if (c->own_stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
  c->stream = (hipStream_t)hip_stream;
  c->own_stream = false;
  return 0;
}

int oakgpu_set_playouts_per_lane(oakgpu_ctx *c, int k) {
  if (!c || k < 1) return bad("oakgpu_set_playouts_per_lane: bad argument");
  c->playouts_per_lane = k;
  return 0;
}

int oakgpu_set_regroup(oakgpu_ctx *c, int rounds, int suspend_below, int shrink) {
  if (!c || rounds < 1 || rounds > 8 || suspend_below < 0 || suspend_below > 64 || shrink < 1)
    return bad("oakgpu_set_regroup: bad argument");
  c->rounds = rounds;
  c->suspend_below = suspend_below;
  c->round_shrink = shrink;
  c->rounds_auto = 0; // an explicit setting applies to every launch, saturating or not
  return 0;
}

int oakgpu_set_migration(oakgpu_ctx *c, int mode, int long_steps, int adopters) {
  if (!c || mode < 0 || mode > 2 || long_steps < 1 || adopters < 0) return bad("oakgpu_set_migration: bad argument");
  c->migrate = mode;
  c->migrate_steps = long_steps;
  c->migrate_adopters = adopters;
  return 0;
}

int oakgpu_set_migration_window(oakgpu_ctx *c, int window) {
  if (!c || window < 0 || window > 255) return bad("oakgpu_set_migration_window: window must be 0 (off) .. 255 turn-steps");
  c->migrate_window = window;
  return 0;
}

int oakgpu_get_queue_counters(oakgpu_ctx *c, uint32_t *out64) { // diagnostic: synchronises the stream
  if (!c || !out64) return bad("oakgpu_get_queue_counters: null argument");
  if (!c->d_queue) { memset(out64, 0, 256); return 0; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out64, c->d_queue, 256, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int oakgpu_set_spread(oakgpu_ctx *c, int lanes) {
  if (!c || lanes < -1 || lanes > 64) return bad("oakgpu_set_spread: lanes must be -1 (automatic) or 0..64");
  c->spread_lanes = lanes;
  return 0;
}

int oakgpu_set_standstill_skip(oakgpu_ctx *c, int on) {
  if (!c) return bad("null ctx");
  c->standstill_skip = on != 0;
  return 0;
}

int oakgpu_set_move_carry(oakgpu_ctx *c, int below) {
  if (!c || below < 0 || below > 64) return bad("oakgpu_set_move_carry: below must be 0 (off) .. 64 lanes");
  c->move_carry = below;
  return 0;
}

int oakgpu_set_move_carry_dry(oakgpu_ctx *c, int below) {
  if (!c || below < 0 || below > 64) return bad("oakgpu_set_move_carry_dry: below must be 0 (off) .. 64 lanes");
  c->move_carry_dry = below;
  return 0;
}

int oakgpu_set_lean_rollout(oakgpu_ctx *c, int on) {
  if (!c) return bad("null ctx");
  c->lean_rollout = on != 0;
  return 0;
}

int oakgpu_last_launch_lean(oakgpu_ctx *c) { return c ? c->last_launch_lean : 0; }

int oakgpu_set_search_party_table(oakgpu_ctx *c, int on) {
  if (!c) return bad("null ctx");
  const int old = c->search_party_table;
  c->search_party_table = on != 0;
  return old;
}

int oakgpu_search_party_table_stats(oakgpu_ctx *c, uint64_t *fills, uint64_t *evals) {
  if (!c) return bad("null ctx");
  if (fills) *fills = c->search_table_fills;
  if (evals) *evals = c->search_table_evals;
  return 0;
}

int oakgpu_set_queue_order(oakgpu_ctx *c, int on) {
  if (!c) return bad("null ctx");
  c->queue_order = on != 0;
  return 0;
}

int oakgpu_set_tail_pack(oakgpu_ctx *c, int below, int waves, int lanes) {
  if (!c || below < 0 || below > 64 || waves < 0 || lanes < 0 || lanes > 64) return bad("oakgpu_set_tail_pack: bad argument");
  c->tail_below = below;
  c->tail_waves = waves;
  c->tail_lanes = lanes;
  return 0;
}

int oakgpu_set_yield_schedule(oakgpu_ctx *c, int mode, int below, int waves, int lanes) {
  if (!c || mode < 0 || mode > 2 || below < 1 || below > 64 || waves < 0 || lanes < 0 || lanes > 64) return bad("oakgpu_set_yield_schedule: bad argument");
  c->yield_mode = mode;
  c->yield_below = below;
  c->yield_waves = waves;
  c->yield_lanes = lanes;
  return 0;
}

int oakgpu_set_yield_saturation(oakgpu_ctx *c, int waves) {
  if (!c || waves < 0) return bad("oakgpu_set_yield_saturation: bad argument");
  c->yield_min_waves = waves;
  return 0;
}

int oakgpu_last_launch_yield(oakgpu_ctx *c) { return c ? c->last_launch_yield : 0; }

int oakgpu_last_launch_parked(oakgpu_ctx *c, uint32_t *parked) { // diagnostic: synchronises the stream
  if (!c || !parked) return bad("oakgpu_last_launch_parked: null argument");
  *parked = 0;
  if (!c->d_queue || c->last_launch_rounds < 2) return 0;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(parked, c->d_queue + 1, 4, hipMemcpyDeviceToHost, c->stream)); // round 0's count_out
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

void *oakgpu_get_stream(oakgpu_ctx *c) { return c ? (void *)c->stream : nullptr; }

int oakgpu_set_kernel_timing(oakgpu_ctx *c, int on) {
  if (!c) return bad("null ctx");
  HIPCHK(hipSetDevice(c->device));
  if (on && !c->tev_valid) {
    for (auto &e : c->tev) HIPCHK(hipEventCreate(&e));
    c->tev_valid = true;
  }
  c->timing = on != 0;
  return 0;
}

int oakgpu_get_leaf_kernel_ms(oakgpu_ctx *c, float ms[3]) {
  if (!c || !ms) return bad("oakgpu_get_leaf_kernel_ms: null argument");
  if (!c->timing || !c->tev_valid) return bad("oakgpu_get_leaf_kernel_ms: kernel timing is off (oakgpu_set_kernel_timing)");
  HIPCHK(hipEventSynchronize(c->tev[3]));
  for (int i = 0; i < 3; ++i) HIPCHK(hipEventElapsedTime(&ms[i], c->tev[i], c->tev[i + 1]));
  return 0;
}

int oakgpu_synchronize(oakgpu_ctx *c) {
  if (!c) return bad("null ctx");
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->d_queue && c->migrate_used) { // a queue launch since the last check migrated playouts: did a bounded wait run out?
    uint32_t err = 0;
    HIPCHK(hipMemcpy(&err, c->d_queue + 63, 4, hipMemcpyDeviceToHost));
    c->migrate_used = 0;
    if (err) { HIPCHK(hipMemsetAsync(c->d_queue + 63, 0, 4, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); }
    if (err) return bad("rollout: a bounded wait of the long-playout migration ran out (playouts were lost) -- oakgpu_set_migration(ctx, 0, ...) turns it off");
  }
  return 0;
}

#ifdef OAKGPU_SITE_PROFILE
// profile build only (tools/site_profile.sh): read-and-reset the region counters of gen1_regs.hpp
extern "C" int oakgpu_site_profile(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(oak::g_site_prof), sizeof(unsigned long long) * 32 * 4) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[32 * 4] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(oak::g_site_prof), z, sizeof z) != hipSuccess) return 1;
  }
  return 0;
}
#endif

#ifdef OAKGPU_TIMELINE
extern "C" int oakgpu_timeline(unsigned long long *out, int waves) { // profile build only (tools/timeline.py)
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(oak::g_timeline), sizeof(unsigned long long) * 5 * (size_t)waves) != hipSuccess;
}
#endif

// ---- group launch of the queue kernel --------------------------------------------------------------------------
// The batch table travels through a small ring of pinned host slots -> device slots (async copy on the context's
// stream; a slot is reused only after the event behind its previous copy has completed).
// The control block, the queue heads and the batch-table ring of the group launches; the batch table of this launch on its way to
// the device (async copy on the context's stream; a slot is reused only after the event behind its previous copy has completed).
static int stage_group_table(oakgpu_ctx *c, const oak::BatchDesc *descs, uint32_t count, oak::BatchDesc **dt_out) {
  // (the first clearing covers the sticky word too, ON THE CONTEXT'S STREAM: a hipMemset on the NULL stream is not ordered with a
  // non-blocking stream and could land in the middle of the first launch -- queue heads zeroed under a running kernel)
  if (!c->d_queue) { HIPCHK(hipMalloc((void **)&c->d_queue, 256)); HIPCHK(hipMemsetAsync(c->d_queue, 0, 256, c->stream)); }
  constexpr size_t HEADS_BYTES = (size_t)oak::QUEUE_MAX_ROUNDS * oak::QUEUE_HEADS * oak::QUEUE_HEAD_STRIDE * 4;
  if (!c->d_heads) HIPCHK(hipMalloc((void **)&c->d_heads, HEADS_BYTES));
  if (!c->h_table) {
    HIPCHK(hipHostMalloc((void **)&c->h_table, sizeof(oak::BatchDesc) * oak::MAX_GROUP * oakgpu_ctx::TABLE_SLOTS, hipHostMallocDefault));
    HIPCHK(hipMalloc((void **)&c->d_table, sizeof(oak::BatchDesc) * oak::MAX_GROUP * oakgpu_ctx::TABLE_SLOTS));
    for (int i = 0; i < oakgpu_ctx::TABLE_SLOTS; ++i) HIPCHK(hipEventCreateWithFlags(&c->table_ev[i], hipEventDisableTiming));
  }
  const int slot = (int)(c->table_next++ % oakgpu_ctx::TABLE_SLOTS);
  HIPCHK(hipEventSynchronize(c->table_ev[slot])); // never-recorded events are complete
  oak::BatchDesc *ht = (oak::BatchDesc *)c->h_table + (size_t)slot * oak::MAX_GROUP, *dt = (oak::BatchDesc *)c->d_table + (size_t)slot * oak::MAX_GROUP;
  memcpy(ht, descs, sizeof(oak::BatchDesc) * count);
  HIPCHK(hipMemcpyAsync(dt, ht, sizeof(oak::BatchDesc) * count, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->table_ev[slot], c->stream));
  *dt_out = dt;
  return 0;
}

// k_queue_order on the context's stream (it clears the launch's control words on its way); the order goes to c->d_order
static int launch_queue_order(oakgpu_ctx *c, const oak::GroupArgs &g) {
  if (c->order_n < g.total) {
    if (c->d_order) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->d_order)); c->d_order = nullptr; }
    HIPCHK(hipMalloc((void **)&c->d_order, (size_t)g.total * 4));
    c->order_n = g.total;
  }
  const uint32_t pair = 32u + 2u * c->order_pair;
  c->order_pair ^= 1u;
  hipLaunchKernelGGL(oak::k_queue_order, dim3((g.total + oak::ORDER_PER_BLOCK - 1) / oak::ORDER_PER_BLOCK), dim3(oak::ORDER_BLOCK), 0, c->stream, g, c->d_order,
                     c->d_queue, c->d_heads, pair);
  return 0;
}

static int launch_group(oakgpu_ctx *c, const oak::BatchDesc *descs, uint32_t count, uint32_t total, uint32_t max_steps, int prep) {
  HIPCHK(hipSetDevice(c->device));
  oak::BatchDesc *dt = nullptr;
  if (int r = stage_group_table(c, descs, count, &dt)) return r;
  // grid: at least `playouts_per_lane` playouts per lane, and never more waves than the device keeps resident
  const uint32_t n64 = (total + 63) / 64;
  uint32_t waves = (n64 + c->playouts_per_lane - 1) / c->playouts_per_lane;
  if (waves < 1) waves = 1;
  const uint32_t resident = (uint32_t)c->n_cu * 4u * 4u; // four waves per SIMD (k_rollout_queue<64, 4>: 128 VGPRs, measured best; 2 and 3 were removed in round 5)
  bool saturated = waves >= resident;
  if (saturated) waves = resident;
  // A launch that leaves wave slots empty uses them: the same playouts in flight on MORE waves, each taking only a few at a
  // time -- a wave of 8 lanes executes the union of 8 playouts' paths instead of 64's, and the device had the issue slots free
  // (round 3, tools/small_launch_sweep.py ... spread: 65,536 playouts 8.5 -> 7.7 ms at 8 lanes per wave, 16,384 playouts 7.8 ->
  // 6.2 ms at 4, a rank's share of configs[3] 9.3 -> 8.3 ms at 16).  Automatic: as few lanes per wave as fill the resident
  // waves, at least 4.  Not for callers that keep several contexts busy (the other context needs the slots).
  // the yielding schedule (oakgpu_set_yield_schedule): automatic for a saturating launch of full-length playouts when another context
  // of the device has issued one since this context's previous one -- a context on its own keeps the single dispatch with migration
  bool yield = false;
  uint32_t yield_r = 0;
  {
    const bool ysat = max_steps >= 500 && (saturated || (c->yield_min_waves > 0 && waves >= (uint32_t)c->yield_min_waves));
    const bool alternating = ysat && yield_registry_launch(c);
    yield = waves >= 2 && (c->yield_mode == 2 || (c->yield_mode == 1 && alternating));
    if (yield) { // R slots stay free for the other context's follow-up dispatch, and this launch's own takes at most R
      yield_r = (uint32_t)(c->yield_waves > 0 ? c->yield_waves : c->n_cu);
      if (yield_r * 2 > waves) yield_r = waves / 4 ? waves / 4 : 1; // (a small launch: a quarter of its waves)
      waves -= yield_r;
    }
  }
  c->last_launch_yield = yield;
  uint32_t spread = 0;
  if (!yield && !saturated && c->spread_lanes != 0 && !c->concurrent_hint && max_steps > 64) {
    const uint64_t slots = ((uint64_t)total + c->playouts_per_lane - 1) / c->playouts_per_lane; // lanes in flight
    uint32_t lanes = c->spread_lanes > 0 ? (uint32_t)c->spread_lanes : (uint32_t)((slots + resident - 1) / resident);
    if (lanes < 4) lanes = 4;
    if (lanes < 64) {
      uint32_t w = (uint32_t)((slots + lanes - 1) / lanes);
      if (w > resident) w = resident;
      if (w > waves) { waves = w; spread = lanes; }
    }
  }
  // regrouping rounds pay off while the launch leaves SIMDs idle in its tail; a launch that saturates the device
  // for most of its life (a group of batches) runs as a single dispatch (measured: DESIGN.md 3)
  // ... and so does a launch capped at a few steps (stepping a resident batch turn by turn): there is no tail to regroup
  const bool tail_pack = yield || (saturated && c->tail_below > 0 && max_steps > 64);
  const int tail_below = yield ? c->yield_below : c->tail_below, tail_lanes = yield ? c->yield_lanes : c->tail_lanes;
  const uint32_t tail_waves = yield ? yield_r : (uint32_t)(c->tail_waves > 0 ? c->tail_waves : c->n_cu);
  // (one per FOUR CUs since the stalemate chains are fast-forwarded instead of played: the adopters hold ~700 live long playouts per
  // 1.31 M instead of ~1,800, and every adopter is a wave that takes no bulk work once donations exist.  Measured on the driver
  // command, profiles/r13_drain.json: 16 / 32 / 64 / 96 / 128 adopters 8.42 / 8.89 / 9.00 / 8.84 / 8.90 G at the median of four runs)
  const uint32_t adopters = (uint32_t)(c->migrate_adopters > 0 ? c->migrate_adopters : (c->n_cu + 3) / 4);
  // long-playout migration (k_rollout_queue) replaces the regrouping rounds where it applies: a single dispatch
  const bool migrate = !tail_pack && max_steps > (uint32_t)c->migrate_steps && waves > adopters &&
                       (c->migrate == 2 || (c->migrate == 1 && saturated && max_steps >= 500));
  // Regrouping rounds only on request (oakgpu_set_regroup).  They were the default for launches that do not fill the device while
  // twenty such launches ran side by side on twenty streams (round 1: a parked wave's slots went to another batch); since group
  // launches replaced that, a lone launch is measured FASTER as one dispatch at every size (round 3, tools/small_launch_sweep.py:
  // 16,384 / 65,536 / 131,072 / 262,144 playouts: 10.3 / 11.7 / 11.9 / 12.5 ms with rounds 4 / 32 / 3 against 8.0 / 8.6 / 9.5 / 9.5 ms
  // as a single dispatch with the queue order below)
  // (the tree search keeps two batches in flight on two contexts and asks for the rounds -- oakgpu_ctx_set_concurrent_hint --:
  // behind a single 8 ms dispatch the other context's small per-level kernels queued up: 11 -> 69 ms of waiting per search)
  const int rounds = tail_pack ? 2 : migrate ? 1 : ((!c->rounds_auto || (c->concurrent_hint && !saturated && max_steps > 64)) && c->suspend_below > 0 && waves >= 8) ? c->rounds : 1;
  c->last_launch_rounds = rounds;
  if ((rounds > 1 || migrate) && c->scratch_n < total) {
    if (c->d_scratch) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->d_scratch)); c->d_scratch = nullptr; }
    HIPCHK(hipMalloc((void **)&c->d_scratch, (size_t)total * (384 + 8 + 4 + 4) + (((size_t)total + 15) & ~(size_t)15)));
    c->scratch_n = total;
    c->tickets_dirty = true;
  }
  const size_t lq = 24 * 64 * 4 + oak::TABLE_LDS_PAD + oak::COLD_LDS_BYTES;
  uint8_t *sb = c->d_scratch, *sd = sb ? sb + (size_t)c->scratch_n * 384 : nullptr;
  uint32_t *lists[2] = {sd ? (uint32_t *)(sd + (size_t)c->scratch_n * 8) : nullptr, nullptr};
  lists[1] = lists[0] ? lists[0] + c->scratch_n : nullptr;
  uint8_t *sres = lists[1] ? (uint8_t *)(lists[1] + c->scratch_n) : nullptr;
  const oak::GroupArgs g{dt, count, total, max_steps, prep};
  // no batch takes durations back: the kernel that keeps none (any prep, any battles_out), in every round of the launch
  bool lean = c->lean_rollout != 0;
  for (uint32_t i = 0; i < count; ++i) lean = lean && !descs[i].durations_out;
  c->last_launch_lean = lean;
  const uint32_t *order = nullptr;
  if (c->queue_order && max_steps > 250 && total >= 8192) { // (a few thousand playouts have no queue to speak of: they all start at once)
    if (int r = launch_queue_order(c, g)) return r;
    order = c->d_order;
  } else {
    hipLaunchKernelGGL(oak::k_clear_launch_words, dim3(1), dim3(256), 0, c->stream, c->d_queue, c->d_heads);
  }
  // the adoption tickets (one per donation at most) are tagged with the launch's epoch, so a launch clears nothing -- but for the
  // first use of the list, a regrouping launch's lists in the same memory, and the epoch's wrap to 0 after 2^32 launches
  if (migrate) {
    if (++c->ticket_epoch == 0 || c->tickets_dirty) {
      HIPCHK(hipMemsetAsync(lists[0], 0, (size_t)c->scratch_n * 8, c->stream));
      if (c->ticket_epoch == 0) c->ticket_epoch = 1;
      c->tickets_dirty = false;
    }
    c->migrate_used = 1; // (sticky, like the device word: back-to-back launches keep an earlier launch's error)
  } else if (rounds > 1) c->tickets_dirty = true;
  for (int r = 0; r < rounds; ++r) {
    oak::RoundArgs q{};
    q.order = r == 0 ? order : nullptr;
    q.long_steps = (uint32_t)(c->migrate_steps > 0xFFFF ? 0xFFFF : c->migrate_steps) | (uint32_t)(c->migrate_window > 0 ? c->migrate_window : 256) << 16;
    q.no_skip = c->standstill_skip ? 0u : 1u;
    q.move_carry = (uint32_t)c->move_carry;
    q.stats = c->d_queue + OAKGPU_CTL_FAST_FORWARDED;
    if (migrate) { q.adopt_ctl = c->d_queue + 40; q.adopt_list = (uint64_t *)lists[0]; q.epoch = c->ticket_epoch; q.n_adopters = adopters; } // (one round: both lists' memory)
    q.list_in = r ? lists[(r - 1) & 1] : nullptr;
    q.n_in = r ? c->d_queue + 2 * r - 1 : nullptr; // = count_out of round r - 1
    q.list_out = lists[r & 1];
    q.count_out = c->d_queue + 2 * r + 1;
    q.sb = sb; q.sd = sd; q.sres = sres;
    q.suspend_below = r + 1 < rounds ? (uint32_t)(tail_pack ? tail_below : c->suspend_below) : 0u;
    q.move_carry_dry = c->move_carry_dry > 0 ? std::max((uint32_t)c->move_carry_dry, q.suspend_below) : 0u; // (a wave that could suspend does not carry)
    q.queue = c->d_heads + (size_t)r * oak::QUEUE_HEADS * oak::QUEUE_HEAD_STRIDE;
    q.lanes = (tail_pack && r > 0) ? (uint32_t)tail_lanes : (r == 0 ? spread : 0u);
    if (lean && !prep) hipLaunchKernelGGL((oak::k_rollout_queue<64, 4, false, false>), dim3(waves), dim3(64), lq, c->stream, g, q); // (no prep code either)
    else if (lean) hipLaunchKernelGGL((oak::k_rollout_queue<64, 4, false>), dim3(waves), dim3(64), lq, c->stream, g, q);
    else hipLaunchKernelGGL((oak::k_rollout_queue<64, 4>), dim3(waves), dim3(64), lq, c->stream, g, q);
    waves = tail_pack ? tail_waves : (waves + c->round_shrink - 1) / c->round_shrink;
    if (waves < 1) waves = 1;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// Diagnostic (tests): k_queue_order alone, at ANY total, on host battles -- the order a group launch of these batches would hand its
// playouts out in, and how many of them it put in front.  Synchronises; clears the control words like a launch.
int oakgpu_queue_order(oakgpu_ctx *c, const oakgpu_rollout_batch *batches, uint32_t count, uint32_t *order_out, uint32_t *suspects_out) {
  if (!c || !batches || !order_out || count == 0 || count > (uint32_t)oak::MAX_GROUP) return bad("oakgpu_queue_order: bad argument");
  HIPCHK(hipSetDevice(c->device));
  uint64_t total = 0;
  for (uint32_t i = 0; i < count; ++i) { if (!batches[i].battles || batches[i].n == 0) return bad("oakgpu_queue_order: empty batch"); total += batches[i].n; }
  if (total >= 0xFFFFFFF0ull) return bad("oakgpu_queue_order: more than 2^32 playouts");
  uint8_t *d_battles = nullptr;
  HIPCHK(hipMalloc((void **)&d_battles, (size_t)total * 384));
  oak::BatchDesc descs[oak::MAX_GROUP] = {};
  uint32_t start = 0;
  int rc = 0;
  for (uint32_t i = 0; i < count && !rc; ++i) {
    descs[i].battles = d_battles + (size_t)start * 384;
    descs[i].start = start;
    descs[i].n = batches[i].n;
    if (hipMemcpyAsync(d_battles + (size_t)start * 384, batches[i].battles, (size_t)batches[i].n * 384, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = bad("oakgpu_queue_order: copy");
    start += batches[i].n;
  }
  oak::BatchDesc *dt = nullptr;
  if (!rc) rc = stage_group_table(c, descs, count, &dt);
  uint32_t pair = 32u + 2u * c->order_pair; // (the pair launch_queue_order is about to use)
  if (!rc) rc = launch_queue_order(c, oak::GroupArgs{dt, count, (uint32_t)total, 1000u, 0});
  if (!rc && hipGetLastError() != hipSuccess) rc = bad("oakgpu_queue_order: launch");
  if (!rc && hipMemcpyAsync(order_out, c->d_order, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = bad("oakgpu_queue_order: copy back");
  uint32_t suspects = 0;
  if (!rc && hipMemcpyAsync(&suspects, c->d_queue + pair, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = bad("oakgpu_queue_order: copy back");
  hipError_t se = hipStreamSynchronize(c->stream);
  (void)hipFree(d_battles);
  if (!rc && se != hipSuccess) return fail(se, "oakgpu_queue_order");
  if (suspects_out) *suspects_out = suspects;
  return rc;
}

static int launch_single(oakgpu_ctx *c, const oak::RolloutArgs &a) { // one lane per playout, no queue
  const uint32_t n = a.n;
  static const bool no_staged = getenv("OAKGPU_NO_STAGED") != nullptr; // (A/B)
  if (a.max_steps <= 16 && !no_staged && ((uintptr_t)a.battles & 15) == 0 && (!a.battles_out || ((uintptr_t)a.battles_out & 15) == 0))
    hipLaunchKernelGGL(oak::k_rollout_staged, dim3((n + 63) / 64), dim3(64), oak::STAGED_LDS_BYTES, c->stream, a);
  else
    hipLaunchKernelGGL(oak::k_rollout_regs<64>, dim3((n + 63) / 64), dim3(64), 24 * 64 * 4 + oak::TABLE_LDS_PAD, c->stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int oakgpu_rollout_group_dev(oakgpu_ctx *c, const oakgpu_rollout_batch *batches, uint32_t count, uint32_t max_steps, int prep) {
  if (!c) return bad("null ctx");
  if (count == 0) return 0;
  if (!batches) return bad("oakgpu_rollout_group_dev: null batches");
  if (count > (uint32_t)oak::MAX_GROUP) return bad("oakgpu_rollout_group_dev: more than 64 batches in one group");
  oak::BatchDesc descs[oak::MAX_GROUP];
  uint32_t used = 0;
  uint64_t total = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const oakgpu_rollout_batch &b = batches[i];
    if (b.n == 0) continue;
    if (!b.battles || !b.durations || !b.results_in || !b.prng_state || !b.results_out || !b.steps_out || !b.values_out)
      return bad("oakgpu_rollout_group_dev: null required pointer");
    descs[used++] = oak::BatchDesc{b.battles, b.durations, b.results_in, b.prng_state, b.results_out, b.steps_out, b.values_out,
                                   b.battles_out, b.durations_out, (uint32_t)total, b.n};
    total += b.n;
  }
  if (used == 0) return 0;
  if (total >= 0xFFFFFFF0ull) return bad("oakgpu_rollout_group_dev: more than 2^32 playouts in one group");
  // no queue: one launch per batch -- also for launches capped at a few turn-steps (stepping a resident batch turn by turn,
  // BASELINE configs[2]): there is no tail for a queue to fill, and twice the waves hide twice the latency (measured, one
  // turn-step of 65,536 battles: 61 us against 99 us; tools/onestep_latency.py)
  if (c->playouts_per_lane <= 1 || max_steps <= 16) {
    HIPCHK(hipSetDevice(c->device));
    for (uint32_t i = 0; i < used; ++i) {
      const oak::BatchDesc &d = descs[i];
      if (int r = launch_single(c, oak::RolloutArgs{d.battles, d.durations, d.results_in, d.prng, d.n, max_steps, prep, d.results_out,
                                                    d.steps_out, d.values_out, d.battles_out, d.durations_out})) return r;
    }
    return 0;
  }
  return launch_group(c, descs, used, (uint32_t)total, max_steps, prep);
}

int oakgpu_rollout_dev(oakgpu_ctx *c, const uint8_t *battles, const uint8_t *durations, const uint8_t *results_in,
                       uint8_t *prng_state, uint32_t n, uint32_t max_steps, int prep, uint8_t *results_out,
                       uint32_t *steps_out, float *values_out, uint8_t *battles_out, uint8_t *durations_out) {
  const oakgpu_rollout_batch b{battles, durations, results_in, prng_state, n, results_out, steps_out, values_out, battles_out, durations_out};
  return oakgpu_rollout_group_dev(c, &b, 1, max_steps, prep);
}

// ---- root-parallel search steps in slices (k_root_step; include/oakgpu.h) -----------------------------------------------------
struct oakgpu_root_steps {
  oakgpu_ctx *ctx;
  uint32_t n_roots, reps, slice, max_steps, cap;
  uint4 *state[2];     // carry lists, ping-pong: cap records of oak::CARRY_VEC uint4
  unsigned long long *acc; // ROOT_SHARDS x acc_stride per-root accumulators of the launch in flight
  uint32_t acc_stride;
  uint32_t *ctl;       // counters on 256-byte lines of their own: lines [0, 8) / [8, 16) the two lists' per-shard counts, [16, 24) the queue heads, 24 the sticky error word
  int cur;             // the list the NEXT launch reads
  bool lean;           // the context's oakgpu_set_lean_rollout when the handle was made: k_root_step<4, false>, for the handle's whole life (the carry records are the instantiation's own)
};

int oakgpu_root_steps_create(oakgpu_ctx *c, uint32_t n_roots, uint32_t reps, uint32_t slice, uint32_t max_steps, oakgpu_root_steps **out) {
  if (!c || !out) return bad("oakgpu_root_steps_create: null argument");
  if (n_roots == 0 || reps == 0 || max_steps == 0) return bad("oakgpu_root_steps_create: roots, replicas and max_steps must be positive");
  if (slice & (slice - 1)) return bad("oakgpu_root_steps_create: slice must be a power of two (0 = playouts run to terminal inside their step)");
  if ((uint64_t)n_roots * reps >= 0x40000000ull) return bad("oakgpu_root_steps_create: more than 2^30 playouts per step");
  HIPCHK(hipSetDevice(c->device));
  oakgpu_root_steps *rs = new oakgpu_root_steps{};
  rs->ctx = c; rs->n_roots = n_roots; rs->reps = reps; rs->slice = slice; rs->max_steps = max_steps;
  rs->lean = c->lean_rollout != 0;
  // every playout in flight is in at most one list: a step adds n_roots * reps and a playout lives ceil(max_steps / slice) launches
  const uint64_t lives = slice ? (max_steps + slice - 1) / slice : 1;
  const uint64_t worst = (uint64_t)n_roots * reps * (lives > 1 ? lives - 1 : 0);
  // ... but the length distribution decays fast (random OU playouts: mean ~100 turn-steps, 99.5 % end before 250): the steady population
  // is ~(mean length / slice - 0.4) steps' worth (measured: 0.17 / 1.14 / 2.66 steps' worth at slice 128 / 64 / 32); 1 + 256 / slice steps'
  // worth leaves 3-4x of that, shard imbalance included; an overflow is reported (sticky error), never silent
  const uint64_t want = (uint64_t)n_roots * reps * (1 + (slice ? 256 / slice : 0));
  rs->cap = (uint32_t)(worst < want ? worst : want);
  rs->cap = (rs->cap + oak::ROOT_SHARDS - 1) / oak::ROOT_SHARDS * oak::ROOT_SHARDS; // (segments of cap / 8 records)
  if (rs->cap == 0) rs->cap = oak::ROOT_SHARDS;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipMalloc((void **)&rs->state[k], (size_t)rs->cap * oak::CARRY_VEC * 16);
  rs->acc_stride = (n_roots + 31u) & ~31u; // (whole 256-byte lines per shard)
  if (e == hipSuccess) e = hipMalloc((void **)&rs->acc, (size_t)oak::ROOT_SHARDS * rs->acc_stride * 8);
  constexpr size_t CTL_BYTES = (size_t)25 * oak::CTL_STRIDE * 4;
  if (e == hipSuccess) e = hipMalloc((void **)&rs->ctl, CTL_BYTES);
  if (e == hipSuccess) e = hipMemsetAsync(rs->ctl, 0, CTL_BYTES, c->stream);
  if (e != hipSuccess) { oakgpu_root_steps_destroy(rs); return fail(e, "oakgpu_root_steps_create"); }
  *out = rs;
  return 0;
}

void oakgpu_root_steps_destroy(oakgpu_root_steps *rs) {
  if (!rs) return;
  (void)hipSetDevice(rs->ctx->device);
  (void)hipStreamSynchronize(rs->ctx->stream);
  for (int k = 0; k < 2; ++k) if (rs->state[k]) (void)hipFree(rs->state[k]);
  if (rs->ctl) (void)hipFree(rs->ctl);
  if (rs->acc) (void)hipFree(rs->acc);
  delete rs;
}

// Grow the carry lists to hold at least `playouts` carried playouts (never shrinks).  Synchronises the context's stream; the playouts
// in flight keep their places (each shard's segment is copied to its new base).  The default capacity (1 + 256 / slice steps' worth)
// is 3-4x what random OU roots need; roots whose playouts mostly run into the step cap (stalemates) need up to
// ceil(max_steps / slice) - 1 steps' worth -- a caller that sees `carried` approach the capacity reserves more BEFORE the next launch.
int oakgpu_root_steps_reserve(oakgpu_root_steps *rs, uint64_t playouts) {
  if (!rs) return bad("oakgpu_root_steps_reserve: null argument");
  oakgpu_ctx *c = rs->ctx;
  HIPCHK(hipSetDevice(c->device));
  uint64_t want = (playouts + oak::ROOT_SHARDS - 1) / oak::ROOT_SHARDS * oak::ROOT_SHARDS;
  if (want <= rs->cap) return 0;
  if (want >= 0xFFFFFFF0ull) return bad("oakgpu_root_steps_reserve: more than 2^32 carried playouts");
  HIPCHK(hipStreamSynchronize(c->stream));
  constexpr size_t LINES8 = (size_t)oak::ROOT_SHARDS * oak::CTL_STRIDE;
  uint32_t counts[oak::ROOT_SHARDS];
  for (int sh = 0; sh < oak::ROOT_SHARDS; ++sh) HIPCHK(hipMemcpy(&counts[sh], rs->ctl + rs->cur * LINES8 + (size_t)sh * oak::CTL_STRIDE, 4, hipMemcpyDeviceToHost));
  const size_t old_seg = rs->cap / oak::ROOT_SHARDS, new_seg = want / oak::ROOT_SHARDS, rec = (size_t)oak::CARRY_VEC * 16;
  uint4 *fresh[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) {
    hipError_t e = hipMalloc((void **)&fresh[k], (size_t)want * rec);
    if (e != hipSuccess) { if (fresh[0]) (void)hipFree(fresh[0]); return fail(e, "oakgpu_root_steps_reserve"); }
  }
  for (int sh = 0; sh < oak::ROOT_SHARDS; ++sh) { // the list the next launch reads; the other one is scratch
    const size_t n = counts[sh] < old_seg ? counts[sh] : old_seg;
    if (n) HIPCHK(hipMemcpy((uint8_t *)fresh[rs->cur] + (size_t)sh * new_seg * rec, (const uint8_t *)rs->state[rs->cur] + (size_t)sh * old_seg * rec, n * rec, hipMemcpyDeviceToDevice));
  }
  for (int k = 0; k < 2; ++k) { (void)hipFree(rs->state[k]); rs->state[k] = fresh[k]; }
  rs->cap = (uint32_t)want;
  return 0;
}
int oakgpu_root_steps_capacity(const oakgpu_root_steps *rs, uint32_t *capacity) {
  if (!rs || !capacity) return bad("oakgpu_root_steps_capacity: null argument");
  *capacity = rs->cap;
  return 0;
}

int oakgpu_root_steps_launch_dev(oakgpu_root_steps *rs, const uint8_t *root_battles, const uint8_t *root_durations,
                                 const uint8_t *root_results, uint8_t *lane_prng, int fresh, unsigned long long *report) {
  if (!rs || !report) return bad("oakgpu_root_steps_launch_dev: null argument");
  // (root_battles also in a drain step: a carried playout reads its Pokemon's immutable data -- stats, move ids, species, types -- from its ROOT's battle)
  if (!root_battles) return bad("oakgpu_root_steps_launch_dev: null root_battles (carried playouts read their root's immutable data: drain steps need it too)");
  if (fresh && (!root_durations || !root_results || !lane_prng)) return bad("oakgpu_root_steps_launch_dev: null root / stream pointer");
  oakgpu_ctx *c = rs->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int in = rs->cur, outl = in ^ 1;
  HIPCHK(hipMemsetAsync(report, 0, ((size_t)rs->n_roots + 2) * 8, c->stream));
  HIPCHK(hipMemsetAsync(rs->acc, 0, (size_t)oak::ROOT_SHARDS * rs->acc_stride * 8, c->stream));
  constexpr size_t LINES8 = (size_t)oak::ROOT_SHARDS * oak::CTL_STRIDE; // words of eight counters
  uint32_t *cnt_in = rs->ctl + in * LINES8, *cnt_out = rs->ctl + outl * LINES8, *heads = rs->ctl + 2 * LINES8, *errw = rs->ctl + 3 * LINES8;
  HIPCHK(hipMemsetAsync(cnt_out, 0, LINES8 * 4, c->stream)); // the list this launch fills
  HIPCHK(hipMemsetAsync(heads, 0, LINES8 * 4, c->stream));   // queue heads
  oak::RootStepArgs a{};
  a.root_battles = root_battles; a.root_durations = root_durations; a.root_results = root_results; a.lane_prng = lane_prng;
  a.cin_state = rs->state[in]; a.cin_count = cnt_in;
  a.cout_state = rs->state[outl]; a.cout_count = cnt_out;
  a.acc = rs->acc; a.acc_stride = rs->acc_stride; a.turn_steps = report + rs->n_roots; a.queue = heads; a.err = errw;
  a.n_fresh = fresh ? rs->n_roots * rs->reps : 0u; a.reps = rs->reps; a.seg = rs->cap / oak::ROOT_SHARDS;
  a.fper = (a.n_fresh + oak::ROOT_SHARDS - 1) / oak::ROOT_SHARDS;
  a.slice_mask = rs->slice ? rs->slice - 1 : 0xFFFFFFFFu; // (0xFFFFFFFF: steps & mask is never 0 after a step -- no slicing)
  a.max_steps = rs->max_steps;
  // a persistent grid of the resident waves: the number of carried playouts is only known on the device
  const uint64_t upper = (uint64_t)a.n_fresh + rs->cap;
  const uint32_t resident = (uint32_t)c->n_cu * 4u * 4u;
  const uint32_t waves = (uint32_t)std::min<uint64_t>(resident, (upper + 63) / 64);
  if (rs->lean) hipLaunchKernelGGL((oak::k_root_step<4, false>), dim3(waves), dim3(64), oak::ROOT_STEP_LDS_BYTES, c->stream, a);
  else hipLaunchKernelGGL((oak::k_root_step<4>), dim3(waves), dim3(64), oak::ROOT_STEP_LDS_BYTES, c->stream, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(oak::k_root_step_report, dim3((rs->n_roots + 255) / 256), dim3(256), 0, c->stream, rs->acc, rs->acc_stride, rs->n_roots, cnt_out, errw,
                     a.seg, report);
  HIPCHK(hipGetLastError());
  rs->cur = outl;
  return 0;
}

int oakgpu_rollout_draws_dev(oakgpu_ctx *c, const uint8_t *battles, uint32_t battle_stride, const uint8_t *durations,
                             uint32_t durations_stride, const uint8_t *results_in, uint32_t results_stride, const uint64_t *draws,
                             uint32_t n_draws, const uint32_t *offsets, uint32_t n, uint32_t max_steps, int prep,
                             uint8_t *results_out, uint32_t *steps_out, float *values_out, uint8_t *battles_out,
                             uint8_t *durations_out, uint32_t *used_out) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!battles || !durations || !results_in || !draws) return bad("oakgpu_rollout_draws_dev: null required pointer");
  if ((battle_stride != 0 && battle_stride != 384) || (durations_stride != 0 && durations_stride != 8) || results_stride > 1)
    return bad("oakgpu_rollout_draws_dev: strides must be 0 (one shared root) or the element size");
  HIPCHK(hipSetDevice(c->device));
  const oak::DrawArgs a{battles, durations, results_in, battle_stride, durations_stride, results_stride, draws, n_draws, offsets, n,
                        max_steps, prep, results_out, steps_out, values_out, battles_out, durations_out, used_out};
  hipLaunchKernelGGL(oak::k_rollout_draws<64>, dim3((n + 63) / 64), dim3(64), 24 * 64 * 4 + oak::TABLE_LDS_PAD, c->stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// std::mt19937 + the reference's uniform_64 (util/random.h:37: std::uniform_int_distribution<uint64_t> over the full
// range = two 32-bit outputs, high word first -- pinned by tests/golden/rng_known_answers.json)
int oakgpu_mt19937_fill(uint32_t seed, uint64_t skip, uint64_t *out, size_t count) {
  if (!out && count) return bad("oakgpu_mt19937_fill: null out");
  std::mt19937 g{seed};
  g.discard(2 * skip);
  for (size_t i = 0; i < count; ++i) {
    const uint64_t hi = g(), lo = g();
    out[i] = (hi << 32) | lo;
  }
  return 0;
}

// n playouts from ONE root driven by ONE sequential device generator (benchmark.cc:23-31 + mcts.h:250-263,448-496):
// playout i consumes the generator's output right where playout i-1 stopped, so its start offset depends on every
// earlier playout's length.  Resolved on the device without serialising the playouts: pass 1 plays a playout from
// EVERY possible start offset (one lane per draw of the stream; only the number of draws it consumes is kept), the host
// then follows the chain offset[i+1] = offset[i] + used[offset[i]], and pass 2 plays the n real playouts from their
// resolved offsets with full outputs.
int oakgpu_rollout_shared_device(oakgpu_ctx *c, const uint8_t *battle, const uint8_t *durations, uint8_t result,
                                 const uint64_t *draws, uint32_t n_draws, uint32_t n, uint32_t max_steps, int prep,
                                 uint8_t *results_out, uint32_t *steps_out, float *values_out, uint8_t *battles_out,
                                 uint8_t *durations_out, uint32_t *offsets_out, uint64_t *draws_consumed) {
  if (!c) return bad("null ctx");
  if (!battle || !durations || (!draws && n_draws)) return bad("oakgpu_rollout_shared_device: null required pointer");
  if (draws_consumed) *draws_consumed = 0;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  OakHostCall hc(c);
  DevBuf root, dr, used, off, ro, st, va, bo, dd;
  hipError_t e = hipSuccess;
  int rc = 0;
  std::vector<uint32_t> h_used(n_draws), h_off(n);
  uint8_t h_root[384 + 8 + 8] = {};
  memcpy(h_root, battle, 384);
  memcpy(h_root + 384, durations, 8);
  h_root[392] = result;
  auto ok = [&]() { return e == hipSuccess && rc == 0; };
  e = root.alloc(sizeof h_root, c);
  if (ok()) e = hipMemcpyAsync(root.p, h_root, sizeof h_root, hipMemcpyHostToDevice, c->stream);
  if (ok()) e = dr.alloc((size_t)n_draws * 8 + 8, c);
  if (ok() && n_draws) e = hipMemcpyAsync(dr.p, draws, (size_t)n_draws * 8, hipMemcpyHostToDevice, c->stream);
  if (ok()) e = used.alloc((size_t)n_draws * 4 + 4, c);
  const uint8_t *rb = (const uint8_t *)root.p;
  // pass 1: draws consumed by a playout started at every offset
  if (ok() && n_draws)
    rc = oakgpu_rollout_draws_dev(c, rb, 0, rb + 384, 0, rb + 392, 0, (const uint64_t *)dr.p, n_draws, nullptr, n_draws, max_steps, prep,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, (uint32_t *)used.p);
  if (ok() && n_draws) e = hipMemcpyAsync(h_used.data(), used.p, (size_t)n_draws * 4, hipMemcpyDeviceToHost, c->stream);
  if (ok()) e = hipStreamSynchronize(c->stream);
  bool short_stream = false;
  if (ok()) { // the chain
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (pos >= n_draws || h_used[pos] == 0xFFFFFFFFu) { short_stream = true; break; }
      h_off[i] = (uint32_t)pos;
      pos += h_used[pos];
    }
    if (!short_stream && draws_consumed) *draws_consumed = pos;
  }
  // pass 2: the n playouts themselves
  if (ok() && !short_stream) {
    e = off.alloc((size_t)n * 4, c);
    if (ok()) e = hipMemcpyAsync(off.p, h_off.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
    if (ok()) e = ro.alloc(n, c);
    if (ok()) e = st.alloc((size_t)n * 4, c);
    if (ok()) e = va.alloc((size_t)n * 4, c);
    if (ok() && battles_out) e = bo.alloc((size_t)n * 384, c);
    if (ok() && durations_out) e = dd.alloc((size_t)n * 8, c);
    if (ok())
      rc = oakgpu_rollout_draws_dev(c, rb, 0, rb + 384, 0, rb + 392, 0, (const uint64_t *)dr.p, n_draws, (const uint32_t *)off.p, n, max_steps,
                                    prep, (uint8_t *)ro.p, (uint32_t *)st.p, (float *)va.p, (uint8_t *)bo.p, (uint8_t *)dd.p, nullptr);
    auto down = [&](void *host, DevBuf &buf) {
      if (ok() && host && buf.p) e = hipMemcpyAsync(host, buf.p, buf.bytes, hipMemcpyDeviceToHost, c->stream);
    };
    down(results_out, ro); down(steps_out, st); down(values_out, va); down(battles_out, bo); down(durations_out, dd);
    if (ok() && offsets_out) memcpy(offsets_out, h_off.data(), (size_t)n * 4);
  }
  const hipError_t se = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(e, "oakgpu_rollout_shared_device");
  if (rc) return rc;
  if (se != hipSuccess) return fail(se, "hipStreamSynchronize");
  if (short_stream) return bad("oakgpu_rollout_shared_device: the draw stream is too short for n playouts");
  return 0;
}

int oakgpu_update_dev(oakgpu_ctx *c, uint8_t *battles, const uint8_t *c1, const uint8_t *c2, uint8_t *durations,
                      uint8_t *actions, const uint8_t *overrides, uint32_t n, uint8_t *results) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!battles || !c1 || !c2 || !durations || !results) return bad("oakgpu_update_dev: null required pointer");
  HIPCHK(hipSetDevice(c->device));
  LAUNCH_STAGED(k_update, battles, n, battles, c1, c2, durations, actions, overrides, n, results);
  return 0;
}

int oakgpu_choices_dev(oakgpu_ctx *c, const uint8_t *battles, const uint8_t *results, int player, uint8_t *out,
                       uint8_t *counts, uint32_t n) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!battles || !results || !out || !counts || player < 0 || player > 1) return bad("oakgpu_choices_dev: bad argument");
  HIPCHK(hipSetDevice(c->device));
  LAUNCH_STAGED(k_choices, battles, n, battles, results, player, out, counts, n);
  return 0;
}

int oakgpu_tree_step_dev(oakgpu_ctx *c, uint8_t *battles, uint8_t *durations, uint8_t *results, const uint8_t *c1,
                         const uint8_t *c2, uint32_t n, uint32_t rolls, uint8_t *actions, uint8_t *p1_choices,
                         uint8_t *p1_counts, uint8_t *p2_choices, uint8_t *p2_counts) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!battles || !durations || !results || !c1 || !c2 || !actions || !p1_choices || !p1_counts || !p2_choices || !p2_counts)
    return bad("oakgpu_tree_step_dev: null required pointer");
  if (!(rolls == 1 || rolls == 2 || rolls == 3 || rolls == 20 || rolls == 39)) return bad("oakgpu_tree_step_dev: rolls must be 1, 2, 3, 20 or 39");
  HIPCHK(hipSetDevice(c->device));
  const oak::TreeStepArgs ta{battles, durations, results, c1, c2, actions, p1_choices, p1_counts, p2_choices, p2_counts, n, rolls};
  LAUNCH_STAGED(k_tree_step_staged, battles, n, ta);
  return 0;
}

int oakgpu_poke_engine_eval_dev(oakgpu_ctx *c, const uint8_t *battles, uint32_t n, float root_score, float *values, float *scores) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!battles || (!values && !scores)) return bad("oakgpu_poke_engine_eval_dev: null required pointer");
  HIPCHK(hipSetDevice(c->device));
  hipLaunchKernelGGL(oak::k_poke_engine, dim3((n + 255) / 256), dim3(256), 0, c->stream, battles, n, root_score, values, scores);
  HIPCHK(hipGetLastError());
  return 0;
}

int oakgpu_poke_engine_eval(oakgpu_ctx *c, const uint8_t *battles, uint32_t n, float root_score, float *values, float *scores) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!battles || (!values && !scores)) return bad("oakgpu_poke_engine_eval: null required pointer");
  HIPCHK(hipSetDevice(c->device));
  OakHostCall hc(c);
  DevBuf db, dv;
  HIPCHK(db.alloc((size_t)n * 384, c));
  HIPCHK(dv.alloc((size_t)n * 8, c));
  float *fv = (float *)dv.p, *fs = fv + n;
  HIPCHK(hipMemcpyAsync(db.p, battles, (size_t)n * 384, hipMemcpyHostToDevice, c->stream));
  if (int rc = oakgpu_poke_engine_eval_dev(c, (const uint8_t *)db.p, n, root_score, fv, fs)) return rc;
  if (values) HIPCHK(hipMemcpyAsync(values, fv, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (scores) HIPCHK(hipMemcpyAsync(scores, fs, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int oakgpu_init_battles_dev(oakgpu_ctx *c, const uint8_t *teams, const uint64_t *seeds, uint32_t n, int first_update,
                            uint8_t *battles, uint8_t *durations, uint8_t *results) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!teams || !seeds || !battles) return bad("oakgpu_init_battles_dev: null required pointer");
  HIPCHK(hipSetDevice(c->device));
  LAUNCH_STAGED(k_init, battles, n, teams, seeds, n, first_update, battles, durations, results);
  return 0;
}

int oakgpu_set_ou_pools(oakgpu_ctx *c, const uint8_t *legal, int n_legal, const uint8_t *pools, const uint8_t *sizes) {
  if (!c || !legal || !pools || !sizes || n_legal > 152) return bad("oakgpu_set_ou_pools: bad argument");
  // k_random_ou draws 6 DISTINCT species per side and min(4, pool) distinct moves per species by rejection: with fewer
  // than 6 distinct legal species, or a pool holding repeated / too few move ids, its loops would never terminate
  if (n_legal < 6) return bad("oakgpu_set_ou_pools: at least 6 legal species are required");
  {
    bool seen[256] = {};
    for (int i = 0; i < n_legal; ++i) {
      const uint8_t sp = legal[i];
      if (sp == 0 || sp >= 152 || seen[sp]) return bad("oakgpu_set_ou_pools: legal species must be distinct ids in 1..151");
      seen[sp] = true;
      const uint32_t psz = sizes[sp];
      if (psz == 0 || psz > 48) return bad("oakgpu_set_ou_pools: every legal species needs a move pool of 1..48 moves");
      bool mseen[256] = {};
      for (uint32_t k = 0; k < psz; ++k) {
        const uint8_t mv = pools[(size_t)sp * 48 + k];
        if (mv == 0 || mv > 165 || mseen[mv]) return bad("oakgpu_set_ou_pools: move pools must hold distinct move ids in 1..165");
        mseen[mv] = true;
      }
    }
  }
  HIPCHK(hipSetDevice(c->device));
  if (!c->d_legal) {
    HIPCHK(hipMalloc((void **)&c->d_legal, 152));
    HIPCHK(hipMalloc((void **)&c->d_pools, 152 * 48));
    HIPCHK(hipMalloc((void **)&c->d_sizes, 152));
  }
  HIPCHK(hipMemcpy(c->d_legal, legal, (size_t)n_legal, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->d_pools, pools, 152 * 48, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->d_sizes, sizes, 152, hipMemcpyHostToDevice));
  c->n_legal = n_legal;
  return 0;
}

int oakgpu_random_ou_battles_dev(oakgpu_ctx *c, uint64_t seed0, uint32_t n, uint8_t *battles, uint8_t *durations,
                                 uint8_t *prng_state, uint8_t *results) {
  if (!c) return bad("null ctx");
  if (!c->d_legal) return bad("oakgpu_random_ou_battles_dev: call oakgpu_set_ou_pools first");
  if (n == 0) return 0;
  if (!battles || !durations || !prng_state || !results) return bad("oakgpu_random_ou_battles_dev: null pointer");
  HIPCHK(hipSetDevice(c->device));
  LAUNCH_STAGED(k_random_ou, battles, n, seed0, n, c->d_legal, c->n_legal, c->d_pools, c->d_sizes, battles, durations, prng_state, results);
  return 0;
}

// ---- host-buffer conveniences (PCIe-inclusive; never the benchmarked path) ------------------
#define UP(buf, host, nbytes) do { HIPCHK((buf).alloc(nbytes, c)); if (host) HIPCHK(hipMemcpyAsync((buf).p, host, nbytes, hipMemcpyHostToDevice, c->stream)); } while (0)
#define DOWN(host, buf) do { if (host) HIPCHK(hipMemcpyAsync(host, (buf).p, (buf).bytes, hipMemcpyDeviceToHost, c->stream)); } while (0)

int oakgpu_rollout_group(oakgpu_ctx *c, const oakgpu_rollout_batch *batches, uint32_t count, uint32_t max_steps, int prep) {
  if (!c) return bad("null ctx");
  if (count == 0) return 0;
  if (!batches) return bad("oakgpu_rollout_group: null batches");
  if (count > (uint32_t)oak::MAX_GROUP) return bad("oakgpu_rollout_group: more than 64 batches in one group");
  for (uint32_t i = 0; i < count; ++i) {
    const oakgpu_rollout_batch &h = batches[i];
    if (h.n && (!h.battles || !h.durations || !h.results_in || !h.prng_state || !h.results_out || !h.steps_out || !h.values_out))
      return bad("oakgpu_rollout_group: null required pointer");
  }
  HIPCHK(hipSetDevice(c->device));
  OakHostCall hc(c);
  struct Bufs { DevBuf b, d, ri, pr, ro, st, va, bo, dd; };
  std::vector<Bufs> bufs(count);
  std::vector<oakgpu_rollout_batch> dev(count);
  int rc = 0;
  hipError_t e = hipSuccess;
  auto up = [&](DevBuf &buf, const void *host, size_t nbytes) {
    if (e != hipSuccess) return;
    e = buf.alloc(nbytes, c);
    if (e == hipSuccess && host) e = hipMemcpyAsync(buf.p, host, nbytes, hipMemcpyHostToDevice, c->stream);
  };
  auto down = [&](void *host, DevBuf &buf) {
    if (e == hipSuccess && host && buf.p) e = hipMemcpyAsync(host, buf.p, buf.bytes, hipMemcpyDeviceToHost, c->stream);
  };
  for (uint32_t i = 0; i < count; ++i) {
    const oakgpu_rollout_batch &h = batches[i];
    Bufs &B = bufs[i];
    const size_t n = h.n;
    dev[i] = oakgpu_rollout_batch{};
    if (n == 0) continue;
    up(B.b, h.battles, n * 384); up(B.d, h.durations, n * 8); up(B.ri, h.results_in, n); up(B.pr, h.prng_state, n * 8);
    up(B.ro, nullptr, n); up(B.st, nullptr, n * 4); up(B.va, nullptr, n * 4);
    if (h.battles_out) up(B.bo, nullptr, n * 384);
    if (h.durations_out) up(B.dd, nullptr, n * 8);
    dev[i] = oakgpu_rollout_batch{(uint8_t *)B.b.p, (uint8_t *)B.d.p, (uint8_t *)B.ri.p, (uint8_t *)B.pr.p, h.n, (uint8_t *)B.ro.p,
                                  (uint32_t *)B.st.p, (float *)B.va.p, (uint8_t *)B.bo.p, (uint8_t *)B.dd.p};
  }
  if (e == hipSuccess) rc = oakgpu_rollout_group_dev(c, dev.data(), count, max_steps, prep);
  if (e == hipSuccess && !rc)
    for (uint32_t i = 0; i < count; ++i) {
      const oakgpu_rollout_batch &h = batches[i];
      Bufs &B = bufs[i];
      down(h.results_out, B.ro); down(h.steps_out, B.st); down(h.values_out, B.va); down(h.prng_state, B.pr);
      down(h.battles_out, B.bo); down(h.durations_out, B.dd);
    }
  const hipError_t se = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(e, "oakgpu_rollout_group");
  if (rc) return rc;
  if (se != hipSuccess) return fail(se, "hipStreamSynchronize");
  return oakgpu_synchronize(c); // (reports a migration wait that ran out)
}

int oakgpu_rollout(oakgpu_ctx *c, const uint8_t *battles, const uint8_t *durations, const uint8_t *results_in,
                   uint8_t *prng_state, uint32_t n, uint32_t max_steps, int prep, uint8_t *results_out, uint32_t *steps_out,
                   float *values_out, uint8_t *battles_out, uint8_t *durations_out) {
  const oakgpu_rollout_batch b{battles, durations, results_in, prng_state, n, results_out, steps_out, values_out, battles_out, durations_out};
  return oakgpu_rollout_group(c, &b, 1, max_steps, prep);
}

int oakgpu_update(oakgpu_ctx *c, uint8_t *battles, const uint8_t *c1, const uint8_t *c2, uint8_t *durations, uint8_t *actions,
                  const uint8_t *overrides, uint32_t n, uint8_t *results) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!battles || !c1 || !c2 || !durations || !results) return bad("oakgpu_update: null required pointer");
  HIPCHK(hipSetDevice(c->device));
  OakHostCall hc(c);
  DevBuf b, a1, a2, d, ac, ov, rs;
  UP(b, battles, (size_t)n * 384);
  UP(a1, c1, n);
  UP(a2, c2, n);
  UP(d, durations, (size_t)n * 8);
  if (actions) UP(ac, (const void *)nullptr, (size_t)n * 16);
  if (overrides) UP(ov, overrides, (size_t)n * 16);
  UP(rs, (const void *)nullptr, n);
  int r = oakgpu_update_dev(c, (uint8_t *)b.p, (uint8_t *)a1.p, (uint8_t *)a2.p, (uint8_t *)d.p, (uint8_t *)ac.p,
                            (uint8_t *)ov.p, n, (uint8_t *)rs.p);
  if (r) return r;
  DOWN(battles, b);
  DOWN(durations, d);
  DOWN(actions, ac);
  DOWN(results, rs);
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int oakgpu_choices(oakgpu_ctx *c, const uint8_t *battles, const uint8_t *results, int player, uint8_t *out, uint8_t *counts,
                   uint32_t n) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!battles || !results || !out || !counts) return bad("oakgpu_choices: null required pointer");
  HIPCHK(hipSetDevice(c->device));
  OakHostCall hc(c);
  DevBuf b, rs, o, cn;
  UP(b, battles, (size_t)n * 384);
  UP(rs, results, n);
  UP(o, (const void *)nullptr, (size_t)n * 9);
  UP(cn, (const void *)nullptr, n);
  int r = oakgpu_choices_dev(c, (uint8_t *)b.p, (uint8_t *)rs.p, player, (uint8_t *)o.p, (uint8_t *)cn.p, n);
  if (r) return r;
  DOWN(out, o);
  DOWN(counts, cn);
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int oakgpu_init_battles(oakgpu_ctx *c, const uint8_t *teams, const uint64_t *seeds, uint32_t n, int first_update,
                        uint8_t *battles, uint8_t *durations, uint8_t *results) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!teams || !seeds || !battles) return bad("oakgpu_init_battles: null required pointer");
  HIPCHK(hipSetDevice(c->device));
  OakHostCall hc(c);
  DevBuf t, s, b, d, rs;
  UP(t, teams, (size_t)n * 60);
  UP(s, seeds, (size_t)n * 8);
  UP(b, (const void *)nullptr, (size_t)n * 384);
  UP(d, (const void *)nullptr, (size_t)n * 8);
  UP(rs, (const void *)nullptr, n);
  int r = oakgpu_init_battles_dev(c, (uint8_t *)t.p, (uint64_t *)s.p, n, first_update, (uint8_t *)b.p, (uint8_t *)d.p,
                                  (uint8_t *)rs.p);
  if (r) return r;
  DOWN(battles, b);
  DOWN(durations, d);
  DOWN(results, rs);
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- replay check (include/oakgpu.h): the queue order is built on the host from the frame counts -- longest game first, so the
// launch ends on short games instead of a lone 1,000-turn chain -- then k_replay_gather and the persistent k_replay_records.
static int replay_launch(oakgpu_ctx *c, const uint8_t *records, const uint64_t *offsets, const uint16_t *frames, const uint8_t *malformed,
                         const uint16_t *h_frames, const uint8_t *h_malformed, uint32_t n, oakgpu_replay_report *reports, uint8_t *battles,
                         uint8_t *durations) {
  std::vector<uint32_t> start(65537, 0), order;
  for (uint32_t i = 0; i < n; ++i) if (!h_malformed[i]) ++start[65535 - h_frames[i] + 1]; // counting sort, frame counts descending
  for (int b = 1; b <= 65536; ++b) start[b] += start[b - 1];
  const uint32_t n_live = start[65536];
  order.resize(n_live ? n_live : 1);
  for (uint32_t i = 0; i < n; ++i) if (!h_malformed[i]) order[start[65535 - h_frames[i]]++] = i;
  constexpr size_t HEADS_BYTES = oak::QUEUE_HEADS * oak::QUEUE_HEAD_STRIDE * 4;
  const size_t order_bytes = ((size_t)n * 4 + 15) & ~(size_t)15, first_bytes = ((size_t)n + 15) & ~(size_t)15;
  uint8_t *ws = (uint8_t *)grow_block(c, c->replay_ws, HEADS_BYTES + order_bytes + first_bytes + (size_t)n * 384);
  if (!ws) return -1;
  uint32_t *heads = (uint32_t *)ws, *d_order = (uint32_t *)(ws + HEADS_BYTES);
  uint8_t *first = ws + HEADS_BYTES + order_bytes, *aligned = first + first_bytes;
  HIPCHK(hipMemsetAsync(heads, 0, HEADS_BYTES, c->stream));
  if (n_live) HIPCHK(hipMemcpyAsync(d_order, order.data(), (size_t)n_live * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream)); // (`order` is pageable host memory that dies with this call)
  const oak::ReplayArgs a{records, offsets, frames, d_order, aligned, first, (uint32_t *)reports, battles, durations, heads, n_live};
  hipLaunchKernelGGL(oak::k_replay_gather, dim3((n + 3) / 4), dim3(256), 0, c->stream, a, malformed, n);
  if (n_live) {
    const uint32_t waves = std::min((n_live + 63) / 64, oak::walk::resident_walk_waves(c->n_cu));
    hipLaunchKernelGGL((oak::k_replay_records<4>), dim3(waves), dim3(64), oak::REPLAY_LDS_BYTES, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// k_replay_gather alone, for the training-frame corpus (trainframes.hip): aligned battles + first requests of n indexed records, in the
// context's stream.  `reports` (n x 2 dwords, scratch) takes the MALFORMED reports the kernel writes.
int oakgpu_replay_gather_dev(oakgpu_ctx *c, const uint8_t *records, const uint64_t *offsets, const uint8_t *malformed, uint32_t n,
                             uint8_t *aligned, uint8_t *first, uint32_t *reports) {
  if (n == 0) return 0;
  const oak::ReplayArgs a{records, offsets, nullptr, nullptr, aligned, first, reports, nullptr, nullptr, nullptr, 0};
  hipLaunchKernelGGL(oak::k_replay_gather, dim3((n + 3) / 4), dim3(256), 0, c->stream, a, malformed, n);
  HIPCHK(hipGetLastError());
  return 0;
}

int oakgpu_replay_records_dev(oakgpu_ctx *c, const uint8_t *records, const uint64_t *offsets, const uint16_t *frames, const uint8_t *malformed,
                              uint32_t n, oakgpu_replay_report *reports, uint8_t *battles, uint8_t *durations) {
  if (!c) return bad("null ctx");
  if (n == 0) return 0;
  if (!records || !offsets || !frames || !malformed || !reports) return bad("oakgpu_replay_records_dev: null required pointer");
  if (((uintptr_t)offsets & 7) || ((uintptr_t)frames & 1) || ((uintptr_t)reports & 7) || ((uintptr_t)battles & 15) || ((uintptr_t)durations & 7))
    return bad("oakgpu_replay_records_dev: misaligned array (offsets, reports, durations: 8 bytes; frames: 2; battles: 16)");
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint16_t> h_frames(n);
  std::vector<uint8_t> h_malformed(n);
  HIPCHK(hipMemcpyAsync(h_frames.data(), frames, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(h_malformed.data(), malformed, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return replay_launch(c, records, offsets, frames, malformed, h_frames.data(), h_malformed.data(), n, reports, battles, durations);
}

int oakgpu_replay_records(oakgpu_ctx *c, const uint8_t *buffer, size_t size, oakgpu_replay_report *reports, uint32_t capacity,
                          uint32_t *n_records, size_t *stopped_at, uint8_t *battles, uint8_t *durations) {
  if (!c) return bad("null ctx");
  if ((!buffer && size) || !n_records) return bad("oakgpu_replay_records: null argument");
  uint32_t n = 0;
  size_t stop = 0;
  if (int rc = oakgpu_replay_index(buffer, size, nullptr, nullptr, nullptr, 0, &n, &stop)) return rc;
  *n_records = n;
  if (stopped_at) *stopped_at = stop;
  if (n == 0) return 0;
  if (!reports) return bad("oakgpu_replay_records: null reports");
  if (n > capacity) return bad("oakgpu_replay_records: more records than the caller's capacity");
  std::vector<uint64_t> offs(n);
  std::vector<uint16_t> fr(n);
  std::vector<uint8_t> mal(n);
  if (int rc = oakgpu_replay_index(buffer, stop, offs.data(), fr.data(), mal.data(), n, &n, nullptr)) return rc;
  HIPCHK(hipSetDevice(c->device));
  OakHostCall hc(c);
  DevBuf rb, ob, fb, mb, rp, bb, db;
  UP(rb, buffer, stop);
  UP(ob, offs.data(), (size_t)n * 8);
  UP(fb, fr.data(), (size_t)n * 2);
  UP(mb, mal.data(), n);
  UP(rp, (const void *)nullptr, (size_t)n * 8);
  if (battles) UP(bb, (const void *)nullptr, (size_t)n * 384);
  if (durations) UP(db, (const void *)nullptr, (size_t)n * 8);
  if (int rc = replay_launch(c, (const uint8_t *)rb.p, (const uint64_t *)ob.p, (const uint16_t *)fb.p, (const uint8_t *)mb.p, fr.data(), mal.data(), n,
                             (oakgpu_replay_report *)rp.p, (uint8_t *)bb.p, (uint8_t *)db.p))
    return rc;
  DOWN(reports, rp);
  DOWN(battles, bb);
  DOWN(durations, db);
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int oakgpu_engine_switches(int out[4]) { // the unit's own compile-time switches (tools/engine_variants.sh builds this file with others)
  if (!out) return bad("oakgpu_engine_switches: null argument");
  out[0] = OAK_MULTIHIT_ROLL_FIRST;
  out[1] = OAK_PSYWAVE_SHOWDOWN;
  out[2] = OAK_COUNTER_SHOWDOWN;
  out[3] = OAK_ACCURACY_LAST;
  return 0;
}

} // extern "C"
