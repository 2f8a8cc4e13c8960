// oak_amd/csrc/forest_rows.hpp -- what the game loops over the forest search share (forestplay.hip: self-play; forestmatch.hip: two search
// agents against each other): the scan behind a stable compaction, the integer payoffs of process_output's exact Nash solve with the host
// threads that solve them, and the carving of one block of device memory into the forest search's output arrays.  The text is
// forestplay.hip's, moved here unchanged; the kernels are `static` so that each translation unit that includes the header holds its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/oakgpu.h"
#include "oakgpu_internal.h"
#include "nash.hpp"

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

} // namespace fsp
} // namespace oak
