// oak_amd/csrc/record_walk.hpp -- what the kernels that walk `.battle.data` records on the register engine share: k_replay_records
// (oakgpu.hip), k_frames_pick (trainframes.hip), k_frames_expand (corpuseval.hip).  Include after gen1_regs.hpp.
//
// The replay check of one frame (cpp/include/py/battle/frames.h:52-67; the contract is in include/oakgpu.h), stated here once.  Frame
// k of a record holds the byte mn = (m - 1) | (n - 1) << 4 and the stored choices c1, c2; the engine holds its result byte `res` in
// front of the frame (zero durations at the stored battle, frames.h:57-59; the frame is normalised: S = P1, F = P2).  In this order,
// the first failing check is the verdict:
//   1. res is terminal                                   -> EARLY_END
//   2. P1's legal-choice count != m, then P2's != n      -> COUNT   (player 1 before player 2)
//   3. c1 not among P1's legal choices, then c2 not P2's -> ILLEGAL (membership: the record does not fix the list's order)
//   else the frame is playable: update(c1, c2).
// frame_check() is that order; what a walker does with a playable frame, and where its verdict goes, is the walker's own.
//
// A walker with persistent lanes (the first two) feeds them from eight queue heads.  Its wave-uniform state is one word, `ust`, whose
// layout is stated here and nowhere else: bit 0 every head has been seen dry, bits 8-10 the wave's current head, 12-15 the heads
// seen dry, 16-23 an iteration counter.  Only the functions below read or write it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oakgpu.h"
#include "gen1_regs.hpp"

namespace oak {
namespace walk {

constexpr int TABLE_PAD = (TABLE_LDS_BYTES + 15) & ~15; // the engine's tables in LDS, padded to 16 bytes
constexpr int STAGE_STRIDE = 100; // words per battle staged in LDS: 96 + 4 (16-byte aligned rows that spread over the banks)
constexpr uint32_t STATUS_PENDING = 0xFF; // no verdict yet (not an OAKGPU_REPLAY_* value)
constexpr uint32_t LANE_NONE = 0xFFFFFFFFu, LANE_DONE = 0xFFFFFFFEu; // a persistent lane's item: none yet / the queue is dry
#ifndef OAK_REFILL_EVERY
#define OAK_REFILL_EVERY 8
#endif
#ifndef OAK_REFILL_LANES
#define OAK_REFILL_LANES 16
#endif
constexpr uint32_t REFILL_EVERY = OAK_REFILL_EVERY, REFILL_LANES = OAK_REFILL_LANES; // free lanes refill every n-th iteration (a power of two), or at once when this many are free
constexpr uint32_t QUEUE_HEADS = 8, QUEUE_HEAD_STRIDE = 64; // eight queue heads, 64 words (one 256-byte line) apart

__device__ __forceinline__ uint32_t load_u32(const uint8_t *p) { // (frames sit at any byte of the file)
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ uint32_t load_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t frame_bytes(uint32_t mn) { return 11 + 4 * ((mn & 15) + 1 + (mn >> 4) + 1); }

// A 64-bit pointer parked in LDS.  The walkers park their kernel arguments there and read them back where they are used: as kernel
// arguments they would hold SGPRs the turn-step's exec masks need.
template <class P>
__device__ __forceinline__ P cold_ptr_at(const lds_u32 *cold, size_t byte_off) {
  return (P)((uint64_t)cold[byte_off / 4] | ((uint64_t)cold[byte_off / 4 + 1] << 32));
}

__device__ __forceinline__ bool member(uint32_t n, uint64_t lo, uint32_t hi, uint32_t c) { // c among the n choice bytes
  bool in = false;
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) in |= i < n && (i < 8 ? (uint32_t)(lo >> (8 * i)) & 0xFF : hi) == c;
  return in;
}

// ---- the queue of a persistent-lane walker ----------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t queue_state(uint32_t block) { return (block & 7u) << 8; } // a wave starts at head block % 8
__device__ __forceinline__ bool queue_dry(uint32_t ust) { return ust & 1u; }

// Once per loop turn: counts the turn, and says (wave-uniform) whether the lanes of `mask`, the free ones, take from the queue now.
// Refills come in batches -- every REFILL_EVERY-th turn, or at once when REFILL_LANES lanes are free or no lane is playing -- because
// a refill is a returning atomic and dependent loads for the whole wave.
__device__ __forceinline__ bool refill_due(uint32_t &ust, uint64_t mask, bool any_playing) {
  ust = (ust & ~0xFF0000u) | ((ust + 0x10000u) & 0xFF0000u);
  return mask && !queue_dry(ust) && (((ust >> 16) & (REFILL_EVERY - 1)) == 0 || (uint32_t)__popcll(mask) >= REFILL_LANES || !any_playing);
}

// The lanes with `need` (mask = their ballot, wl = the lane) take one queue position each out of `total`: head s hands out the
// positions s, s + 8, s + 16, ... from a counter at heads[s * QUEUE_HEAD_STRIDE], and a wave that finds its head dry moves to the
// next one for good, so after at most eight turns every lane has a position or the queue is dry (queue_dry).  Returns whether this
// lane got one (my < total).  The heads pointer is parked at cold[heads_byte_off / 4] and read by the one lane that needs it.
__device__ __forceinline__ bool queue_take(uint32_t &ust, const lds_u32 *cold, size_t heads_byte_off, uint32_t total, bool need, uint64_t mask, uint32_t wl,
                                           uint32_t &my) {
  uint64_t rem = mask;
  bool got = false;
  for (;;) {
    const uint32_t shard = (ust >> 8) & 7u, need_n = (uint32_t)__popcll(rem);
    const uint32_t lim = total > shard ? (total - shard + 7u) >> 3 : 0u;
    uint32_t base = 0;
    if (wl == 0) base = atomicAdd(cold_ptr_at<uint32_t *>(cold, heads_byte_off) + shard * QUEUE_HEAD_STRIDE, need_n);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    const uint32_t avail = base < lim ? (lim - base < need_n ? lim - base : need_n) : 0u;
    const uint32_t rank = (uint32_t)__popcll(rem & ((1ull << wl) - 1));
    if (((rem >> wl) & 1) && rank < avail) { my = shard + ((base + rank) << 3); got = true; }
    if (avail == need_n) break;
    rem = __ballot(need && !got);
    ust = (ust & ~(7u << 8)) | (((shard + 1u) & 7u) << 8);
    ust += 1u << 12;
    if (((ust >> 12) & 15u) >= 8u) { ust |= 1u; break; }
  }
  return got;
}

// ---- one frame -------------------------------------------------------------------------------------------------------------------
// The report's fields (include/oakgpu.h): expected = the record's byte, got = the engine's.  EARLY_END's expected byte is the stored
// result, which the walker that reports it reads.
struct Verdict { uint32_t status, player, expected, got; };

// The check in the order of this file's head; status == STATUS_PENDING: playable.  l1, l2: the engine's legal choices, set unless
// the game has ended.
template <class ER>
__device__ __forceinline__ Verdict frame_check(ER &e, uint32_t res, uint32_t mn, uint32_t c1, uint32_t c2, typename ER::Choices &l1, typename ER::Choices &l2) {
  if (res & 15) return {OAKGPU_REPLAY_EARLY_END, 0, 0, res};
  const uint32_t m = (mn & 15) + 1, n = (mn >> 4) + 1;
  l1 = e.choices(e.S, (res >> 4) & 3);
  l2 = e.choices(e.F, (res >> 6) & 3);
  if (l1.n != m) return {OAKGPU_REPLAY_COUNT, 1, m, l1.n};
  if (l2.n != n) return {OAKGPU_REPLAY_COUNT, 2, n, l2.n};
  if (!member(l1.n, l1.lo, l1.hi, c1)) return {OAKGPU_REPLAY_ILLEGAL, 1, c1, l1.n};
  if (!member(l2.n, l2.lo, l2.hi, c2)) return {OAKGPU_REPLAY_ILLEGAL, 2, c2, l2.n};
  return {STATUS_PENDING, 0, 0, 0};
}

// Plays the checked frame at fp and returns the engine's result.  The next frame's three bytes are loaded before the update: the
// dependent load overlaps the turn-step (`more`: there is a next frame).
template <class ER>
__device__ __forceinline__ uint32_t play_frame(ER &e, const uint8_t *&fp, uint32_t &mn, uint32_t &c1, uint32_t &c2, bool more) {
  const uint32_t a1 = c1, a2 = c2;
  fp += frame_bytes(mn);
  if (more) { mn = fp[0]; c1 = fp[1]; c2 = fp[2]; }
  return e.update(a1, a2);
}

// ---- lane order ------------------------------------------------------------------------------------------------------------------
// order[] = the items 0 .. n - 1 by length(i) descending, so that the 64 games a wave walks are of similar length.  One workgroup of
// 1,024 threads, a counting sort; lengths past 1,023 share a bucket (the engine ends a game at turn 1,000).
template <class Length>
__device__ __forceinline__ void order_desc(uint32_t n, uint32_t *order, Length length) {
  __shared__ uint32_t hist[1024];
  const uint32_t tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  for (uint32_t i = tid; i < n; i += 1024) atomicAdd(&hist[1023u - min(length(i), 1023u)], 1u);
  __syncthreads();
  const uint32_t own = hist[tid];
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint32_t v = tid >= off ? hist[tid - off] : 0;
    __syncthreads();
    hist[tid] += v;
    __syncthreads();
  }
  const uint32_t start = hist[tid] - own;
  __syncthreads();
  hist[tid] = start;
  __syncthreads();
  for (uint32_t i = tid; i < n; i += 1024) order[atomicAdd(&hist[1023u - min(length(i), 1023u)], 1u)] = i;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// What the device holds of a walker compiled for four waves per SIMD (128 VGPRs): the grid of a persistent-lane launch is the work's
// waves up to this.
constexpr uint32_t resident_walk_waves(int cus) { return (uint32_t)(cus > 0 ? cus : 1) * 4u * 4u; }

} // namespace walk
} // namespace oak
