// oak_amd/csrc/game_rows.hpp -- what the loops that keep a batch of whole games resident on the device share (policyplay.hip: two policies;
// forestplay.hip: self-play over the forest; forestmatch.hip: two search agents): the constants of a row, one pass of the 1,024-lane
// exclusive scan with the kernel that scans the per-block live counts on it, the two halves of the stable compaction (a live row's place,
// then the move of the 384-byte battles) and the tail of a retire kernel.  What a row carries besides its battle, and when it retires, is each
// loop's own.  The kernels are `static` so that each translation unit that includes the header holds its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oak {
namespace game_rows {

constexpr uint32_t DEAD = 0xFFFFFFFFu; // game index of a retired row
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
constexpr int BLOCK = 256;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One pass of an exclusive scan over a workgroup of 1,024 lanes (a wave scans its 64 by shuffles, the 16 wave totals are scanned by every
// lane): `before` = the sum of the lanes in front of this one, `total` = the sum of all 1,024.  wave_total: 16 entries of LDS, the same for
// every pass of a kernel: the first barrier keeps a pass from writing them while a lane still reads the pass before.  A scan over more
// items runs pass after pass, and the caller adds its own carry.
template <class T> struct ScanPass { T before, total; };

template <class T> __device__ __forceinline__ ScanPass<T> scan_pass(T own, T *wave_total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = own;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(incl, d);
    if ((int)lane >= d) incl += up;
  }
  __syncthreads(); // (every lane has read the pass before this one's totals)
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll 4 // (four totals in flight, not sixteen: unrolled in full, the kernels on this pass take 12 to 22 more VGPRs)
  for (uint32_t w = 0; w < 16; ++w) { const T t = wave_total[w]; if (w < wave) before += t; all += t; }
  return ScanPass<T>{before + incl - own, all};
}

// one workgroup: exclusive prefix sums of `count` dwords (the per-block live counts), 1,024 at a time; out_total (nullable) receives the sum
static __global__ __launch_bounds__(1024) void k_rows_offsets(const uint32_t *in, uint32_t count, uint32_t *out, uint32_t *out_total) {
  __shared__ uint32_t wave_total[16];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < count; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const ScanPass<uint32_t> s = scan_pass(i < count ? in[i] : 0u, wave_total);
    if (i < count) out[i] = carry + s.before;
    carry += s.total;
  }
  if (threadIdx.x == 0 && out_total) *out_total = carry;
}

// The tail of a retire kernel (one lane per row, BLOCK lanes): how many rows of this block are still live.  wave_live: BLOCK / 64 entries.
__device__ __forceinline__ void count_block_live(bool live, uint32_t *wave_live, uint32_t *block_live) {
  const unsigned long long ml = __ballot(live);
  if ((threadIdx.x & 63) == 0) wave_live[threadIdx.x >> 6] = (uint32_t)__popcll(ml);
  __syncthreads();
  if (threadIdx.x == 0) block_live[blockIdx.x] = wave_live[0] + wave_live[1] + wave_live[2] + wave_live[3];
}

// The stable compaction of a block of BLOCK rows, first half: a live row's place is its block's offset + the live rows in front of it in the
// block (a ballot and a lane prefix within the wave, the wave totals across the block); NO_ROW for a dead lane.  place[tid] holds the same
// for compact_battles, after the caller's barrier.  wave_total: BLOCK / 64 entries, place: BLOCK.
__device__ __forceinline__ uint32_t compact_place(bool live, uint32_t block_offset, uint32_t *wave_total, uint32_t *place) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long m = __ballot(live);
  const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (lane == 0) wave_total[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (uint32_t w = 0; w < BLOCK / 64; ++w) if (w < wave) before += wave_total[w];
  const uint32_t to = live ? block_offset + before + prefix : NO_ROW;
  place[tid] = to;
  return to;
}

// second half: the block's 384-byte battles move as whole rows to their places, 24 lanes x 16 bytes each
__device__ __forceinline__ void compact_battles(const uint8_t *from, uint8_t *to, uint32_t rows, const uint32_t *place) {
  const uint32_t tid = threadIdx.x, base = blockIdx.x * BLOCK;
  const u32x4 *src = (const u32x4 *)from + (size_t)base * 24;
  u32x4 *dst = (u32x4 *)to;
  const uint32_t in_block = rows - base < (uint32_t)BLOCK ? rows - base : (uint32_t)BLOCK;
#pragma unroll 4
  for (int q = 0; q < 24; ++q) {
    const uint32_t i = q * BLOCK + tid, b = i / 24, w = i - b * 24;
    if (b >= in_block) continue; // (rows past the end are not read)
    const uint32_t t = place[b];
    if (t != NO_ROW) dst[(size_t)t * 24 + w] = src[i];
  }
}

} // namespace game_rows
} // namespace oak
