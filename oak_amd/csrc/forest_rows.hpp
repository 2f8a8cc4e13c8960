// oak_amd/csrc/forest_rows.hpp -- what the game loops over the forest search share (forestplay.hip: self-play; forestmatch.hip: two search
// agents against each other): the scan behind a stable compaction, the integer payoffs of process_output's exact Nash solve with the host
// threads that solve them, the carving of one block of device memory into the forest search's output arrays, and the way from a turn-major
// log of encoded updates to one contiguous `.battle.data` stream (the log entry, the scan of the record lengths, the head and log pack).
// The text is forestplay.hip's, moved here unchanged; the kernels are `static` so that each translation unit that includes the header
// holds its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/oakgpu.h"
#include "oakgpu_internal.h"
#include "nash.hpp"
#include "selfplay_pick.hpp"

namespace oak {
namespace fsp {

constexpr uint32_t DEAD = 0xFFFFFFFFu; // game index of a retired row
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
constexpr int BLOCK = 256;
constexpr uint32_t PAY_STRIDE = 82;              // 81 payoffs + (m | n << 8)

// exclusive prefix sums of `count` dwords, 1,024 at a time (a wave scans its 64 by shuffles, the 16 wave totals are scanned by every lane);
// out_total (nullable) receives the sum.  policyplay.hip's k_games_offsets with a total.
static __global__ __launch_bounds__(1024) void k_fsp_offsets(const uint32_t *in, uint32_t count, uint32_t *out, uint32_t *out_total) {
  __shared__ uint32_t wave_total[16];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < count; base += 1024) {
    const uint32_t i = base + tid, own = i < count ? in[i] : 0;
    uint32_t incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if ((int)lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) { const uint32_t t = wave_total[w]; if (w < wave) before += t; all += t; }
    if (i < count) out[i] = carry + before + incl - own;
    carry += all;
    __syncthreads();
  }
  if (tid == 0 && out_total) *out_total = carry;
}

struct PayoffArgs {
  const uint8_t *m, *n;
  const uint64_t *visit_matrix;
  const double *value_matrix;
  int32_t *pay; // rows x PAY_STRIDE
  uint32_t rows;
};

static __global__ __launch_bounds__(BLOCK) void k_fsp_payoffs(PayoffArgs a) {
#pragma clang fp contract(off)
  const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
  if (row >= a.rows) return;
  const uint32_t m = a.m[row], n = a.n[row];
  const uint64_t *vis = a.visit_matrix + (size_t)row * 81;
  const double *val = a.value_matrix + (size_t)row * 81;
  int32_t *M = a.pay + (size_t)row * PAY_STRIDE;
  for (uint32_t i = 0; i < m; ++i)
    for (uint32_t j = 0; j < n; ++j) {
      uint64_t v = vis[i * 9 + j];
      v += !v;
      M[i * n + j] = (int32_t)(val[i * 9 + j] / (double)v * 256.0);
    }
  M[81] = (int32_t)(m | n << 8);
}

// bytes of one tree's outputs (forest.hip's staging block has the same arrays), every array 16-byte aligned for any n
inline void carve_outputs(uint8_t *p, size_t n, oakgpu_forest_outputs *o) {
  auto take = [&](size_t bytes_per) { uint8_t *q = p; p += ((bytes_per * n + 15) / 16) * 16; return q; };
  o->visit_matrix = (uint64_t *)take(81 * 8); o->value_matrix = (double *)take(81 * 8);
  o->iterations = (uint64_t *)take(8); o->nodes = (uint64_t *)take(8); o->total_depth = (uint64_t *)take(8);
  o->initial_value = (double *)take(8);
  o->p1_logit = (double *)take(72); o->p2_logit = (double *)take(72); o->p1_prior = (double *)take(72); o->p2_prior = (double *)take(72);
  o->stream = (uint64_t *)take(8);
  o->p1_choices = take(9); o->p2_choices = take(9); o->m = take(1); o->n = take(1);
}
constexpr size_t OUT_BYTES = 81 * 8 * 2 + 8 * 4 + 72 * 4 + 8 + 9 * 2 + 2;

// the turn's payoffs on the host's threads, min(16, usable cores): p1 / p2 strategies and the value / 256; a matrix the solver refuses
// keeps zeros, as oakgpu_forest_search leaves them
inline void solve_rows(const int32_t *pay, uint32_t rows, double *nash) {
  double *p1 = nash, *p2 = nash + (size_t)rows * 9, *nv = nash + (size_t)rows * 18;
  auto work = [&](uint32_t lo, uint32_t hi) {
    for (uint32_t r = lo; r < hi; ++r) {
      const int32_t *M = pay + (size_t)r * PAY_STRIDE;
      const int m = M[81] & 0xFF, n = (M[81] >> 8) & 0xFF;
      double x[9] = {}, y[9] = {}, v = 0;
      const bool ok = m >= 1 && m <= 9 && n >= 1 && n <= 9 && oak_nash::solve(M, m, n, x, y, &v);
      for (int q = 0; q < 9; ++q) { p1[(size_t)r * 9 + q] = ok ? x[q] : 0.0; p2[(size_t)r * 9 + q] = ok ? y[q] : 0.0; }
      nv[r] = ok ? v / 256.0 : 0.0;
    }
  };
  const uint32_t threads = std::min<uint32_t>({16u, std::max(1u, oakgpu_usable_cores()), rows / 32 + 1});
  if (threads <= 1) { work(0, rows); return; }
  std::vector<std::thread> pool;
  const uint32_t per = (rows + threads - 1) / threads;
  for (uint32_t t = 0; t < threads; ++t) pool.emplace_back(work, std::min(rows, t * per), std::min(rows, (t + 1) * per));
  for (auto &th : pool) th.join();
}

// ---- records: a game's CompressedFrames record is packed from the log at the end of the call.  `status` is 0 (OAKGPU_FSP_OK) for a game
// whose record is kept; forestmatch.hip hands in a byte of its own making that is 0 for the games it keeps.
constexpr uint32_t HEAD_BYTES = 4 + 2 + 384 + 1; // a record in front of its updates

// one entry of the turn-major log: which game, where in its record, how long, the encoded update
struct LogEntry { uint32_t game, cursor, length; uint8_t bytes[84]; };
static_assert(sizeof(LogEntry) == 96 && oak_pick::MAX_UPDATE_BYTES <= 84, "one log entry is 96 bytes");

// k_fsp_offsets' scan in 64 bits, over the record lengths in game order: offsets[g] = where game g's record starts, offsets[n] = the stream's size
static __global__ __launch_bounds__(1024) void k_fsp_lengths(const uint32_t *length, uint32_t n, unsigned long long *offsets) {
  __shared__ unsigned long long wave_total[16];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t i = base + tid;
    const unsigned long long own = i < n ? length[i] : 0;
    unsigned long long incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long up = __shfl_up(incl, d);
      if ((int)lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) { const unsigned long long t = wave_total[w]; if (w < wave) before += t; all += t; }
    if (i < n) offsets[i] = carry + before + incl - own;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) offsets[n] = carry;
}

struct PackArgs {
  const unsigned long long *offsets;
  const uint32_t *frames, *length;
  const uint8_t *results, *status, *first; // first: n x 384, the battles after the opening update
  const LogEntry *log;
  uint8_t *stream;
  uint32_t n, entries;
};

// the fixed part of every kept record: u32 byte length, u16 frame count, the 384-byte battle, the result byte.  One wave per game; the
// record starts at any byte, so the bytes go out one by one.
static __global__ __launch_bounds__(BLOCK) void k_fsp_pack_head(PackArgs a) {
  const uint32_t g = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= a.n || a.status[g] != OAKGPU_FSP_OK) return;
  uint8_t *dst = a.stream + a.offsets[g];
  const uint32_t total = a.length[g], frames = a.frames[g];
  const uint8_t *battle = a.first + (size_t)g * 384;
  for (uint32_t i = lane; i < HEAD_BYTES; i += 64) {
    uint8_t v;
    if (i < 4) v = (uint8_t)(total >> (8 * i));
    else if (i < 6) v = (uint8_t)(frames >> (8 * (i - 4)));
    else if (i < 6 + 384) v = battle[i - 6];
    else v = a.results[g];
    dst[i] = v;
  }
}

static __global__ __launch_bounds__(BLOCK) void k_fsp_pack_log(PackArgs a) {
  const uint32_t e = blockIdx.x * (BLOCK / 16) + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (e >= a.entries) return;
  const LogEntry &entry = a.log[e];
  const uint32_t g = entry.game, len = entry.length;
  if (g >= a.n || len == 0 || len > oak_pick::MAX_UPDATE_BYTES || a.status[g] != OAKGPU_FSP_OK) return; // (a dropped game's entries stay behind)
  const uint32_t at = HEAD_BYTES + entry.cursor;
  if (at + len > a.length[g]) return;
  uint8_t *dst = a.stream + a.offsets[g] + at;
  for (uint32_t i = lane; i < len; i += 16) dst[i] = entry.bytes[i];
}

} // namespace fsp
} // namespace oak
