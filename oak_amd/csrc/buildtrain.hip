// oak_amd/csrc/buildtrain.hip -- the optimiser step of the team-building network on the device: the forward of both nets on the valid rows
// of a chunk of trajectories, build.py's loss (src/oak/build.py:153-251) with GAE, its exact gradient (through the GAE recursion: the
// reference does not detach it), gradient accumulation over chunks, torch.optim.Adam and the rolling average.  The contract is in
// include/oakgpu.h, "Training the build network"; the two 31-step recursions are build_loss.hpp's, one text for host and device.
//
// What the dense form (3,749-wide products on 0/1 states with at most 31 ones, 3,749 logits of which at most 339 are read) does not need:
//   k_state_keys    one lane per (row, slot): the state's cell, NONE for padding, a cell outside the table or one an earlier slot holds
//   k_layer1        a1 = b1 + the columns of W1 at the state's cells in slot order (W1 is kept transposed: a column is `h` contiguous
//                   floats), relu and its 0/1 derivative factor; once per net
//   k_gemm          (train_kernels.hpp) the dense middle layers and the value head: forward, dX, dW|db with k_reduce
//   k_l3_forward    one wave per row: the n_legal logits, four entries of the list a pass, 16 lanes per row of W3 (lane s sums k = s, s + 16,
//                   ... ascending with fmaf, a butterfly of four steps joins them, b3 last); then S = sum exp(z) with no maximum taken off,
//                   the probability and the log-probability of entry 0, and the value's sigmoid
//   k_keep_mark / k_select   game_rows.hpp's scan: a row is selected when it is kept and fewer than n_cap kept rows stand in front of it
//   k_traj          one lane per trajectory: value_full, build_loss.hpp's GAE forward, the clipped force and the loss terms of each valid
//                   row, G, build_loss.hpp's GAE backward, du
//   k_l3_backward   one wave per row: dz over the list, and dh2 = sum_j dz_j W3[L_j, :] (j ascending, chains of 32 terms, 16 chains a
//                   middle sum) times the derivative factor
//   the transposed sparse products G[c, :] = sum over the entries with cell c of w_e D[row_e, :] (dW1 of both nets over the states'
//   cells; dW3 and db3 over the selected rows' lists) through an inverted index: k_hist (per-block counts in LDS, integer atomics: a count
//   does not depend on their order), an exclusive scan over [cell][block] in two levels (k_cell_totals, game_rows.hpp's k_rows_offsets over
//   the cells, k_cell_offsets), k_place (stable: inside a cell's segment the entries ascend), k_seg_partial (a segment in pieces of OAKGPU_BUILD_TRAINER_SEGMENT entries, each summed in entry order in chains of 32)
//   and k_seg_combine (a cell's pieces pairwise in a fixed order).
//   k_accumulate, k_zero, k_average: elementwise over the block.
// No float atomics anywhere: every sum runs in a fixed order that depends on the entries alone, not on the grid (the same bits from call to
// call of one build; a compiler is still free to fuse a product and a sum outside build_loss.hpp, k_traj and k_l3_backward).  No workspace is allocated
// inside a call.  There is no CPU fallback.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/oakgpu.h"
#include "build_loss.hpp"
#include "game_rows.hpp"
#include "oakgpu_internal.h"
#include "train_kernels.hpp"

using namespace oak::tr;
namespace bl = oak_build_loss;
namespace gr = oak::game_rows;

namespace {
#define RC(x) do { int _r = (x); if (_r) return _r; } while (0)

constexpr uint32_t N_DIM = OAKGPU_BUILD_N_DIM, MAXA = OAKGPU_BUILD_MAX_ACTIONS, STEPS = OAKGPU_BUILD_MAX_STEPS, SEG = OAKGPU_BUILD_TRAINER_SEGMENT;
constexpr uint32_t NONE = 0xFFFFFFFFu, MAX_WIDTH = 256, MAX_TRAJ = OAKGPU_BUILD_TRAINER_MAX_TRAJ, HIST_BLOCKS = 512, HIST_SLOTS = 8192;
static_assert(STEPS == bl::STEPS, "include/oakgpu.h and build_loss.hpp disagree");
static_assert(SEG % CHAIN == 0 && SEG / CHAIN <= MID, "a piece is at most one middle sum of whole chains");

int fail(const char *fn, const std::string &what) { return oakgpu_fail_msg((std::string(fn) + ": " + what).c_str()); }

struct Report {   // device side
  uint32_t rows, kept, n_cap, pad;
  double policy_loss, value_loss, entropy, loss;
};

struct NetLayout {   // offsets into a parameter block, in floats (the working layout)
  uint32_t h1 = 0, h2 = 0, out = 0;
  size_t w1t = 0, b1 = 0, w2 = 0, b2 = 0, w3 = 0, b3 = 0;   // w1t [3749][h1], w2 [h2][h1], w3 [out][h2]
};

// ---- the rows ------------------------------------------------------------------------------------------------------------------------------
struct Chunk {   // oakgpu_build_chunk on the device side, with the trainer's buffers
  const void *mask;
  int32_t mask_dtype;
  const uint16_t *n_legal;
  const uint8_t *valid;
  const float *rewards;
  const uint32_t *rows;
  const uint16_t *state_cells;
  const uint8_t *state_n;
  const uint8_t *keep;
  uint32_t n, V, total, remaining;
  float gamma, gamma_lam, pw, vw, ew;
};

__device__ __forceinline__ bool row_at(const Chunk &c, uint32_t i, uint32_t &b, uint32_t &t) {
  b = c.rows[2 * (size_t)i], t = c.rows[2 * (size_t)i + 1];
  return b < c.n && t < STEPS;
}
__device__ __forceinline__ uint32_t legal_count(const Chunk &c, uint32_t b, uint32_t t) { return min((uint32_t)c.n_legal[(size_t)b * STEPS + t], MAXA); }
// entry j of the list of step (b, t): its cell, NONE when it is outside the table
__device__ __forceinline__ uint32_t legal_cell(const Chunk &c, uint32_t b, uint32_t t, uint32_t j) {
  const size_t at = ((size_t)b * STEPS + t) * MAXA + j;
  const int64_t v = c.mask_dtype == OAKGPU_BUILD_MASK_INT16 ? (int64_t)((const int16_t *)c.mask)[at] : ((const int64_t *)c.mask)[at];
  return (v >= 0 && v < (int64_t)N_DIM) ? (uint32_t)v : NONE;
}

__global__ __launch_bounds__(256) void k_row_index(Chunk c, int32_t *row_index) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c.V) return;
  uint32_t b, t;
  if (row_at(c, i, b, t)) row_index[(size_t)b * STEPS + t] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_state_keys(Chunk c, uint16_t *keys) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)c.V * STEPS) return;
  const uint32_t i = (uint32_t)(e / STEPS), k = (uint32_t)(e % STEPS);
  const uint16_t *cells = c.state_cells + (size_t)i * STEPS;
  uint16_t key = 0xFFFFu;
  if (k < min((uint32_t)c.state_n[i], STEPS) && cells[k] < N_DIM) {
    key = cells[k];
    for (uint32_t q = 0; q < k; ++q) if (cells[q] == key) key = 0xFFFFu;   // the dense state holds a cell once
  }
  keys[e] = key;
}

__global__ __launch_bounds__(256) void k_layer1(const uint16_t *keys, uint32_t V, const float *w1t, const float *b1, uint32_t h, float *y, float *d) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)V * h) return;
  const uint32_t i = (uint32_t)(idx / h), col = (uint32_t)(idx % h);
  float a = b1[col];
  for (uint32_t k = 0; k < STEPS; ++k) {
    const uint32_t key = keys[(size_t)i * STEPS + k];
    if (key < N_DIM) a += w1t[(size_t)key * h + col];
  }
  y[idx] = fmaxf(a, 0.0f);
  d[idx] = a > 0.0f ? 1.0f : 0.0f;   // torch.relu: no gradient at 0
}

struct RowBuffers {
  const float *y2p, *d2p;   // the policy net's second hidden layer [V][h] and its derivative factor
  const float *w3, *b3;     // [3749][h], [3749]
  uint32_t h;
  const float *zv;          // [V] the value net's output before the sigmoid
  float *z, *dz;            // [V][339]
  float *S, *lp, *q0, *val, *gae, *ret, *cf, *forced, *du, *terms, *dz2p;
  uint8_t *sel;
  const int32_t *row_index;
  uint32_t *block_live, *block_offset;
  Report *report;
};

__global__ __launch_bounds__(64) void k_l3_forward(Chunk c, RowBuffers r) {
  __shared__ float s_z[MAXA + 1];
  const uint32_t i = blockIdx.x, lane = threadIdx.x, sub = lane & 15, slot = lane >> 4;
  uint32_t b, t;
  const uint32_t nl = row_at(c, i, b, t) ? legal_count(c, b, t) : 0;
  const float *x = r.y2p + (size_t)i * r.h;
  for (uint32_t base = 0; base < nl; base += 4) {   // (nl is the wave's: every lane runs every pass)
    const uint32_t j = base + slot;
    const uint32_t cell = j < nl ? legal_cell(c, b, t, j) : NONE;
    float acc = 0.0f;
    if (cell != NONE) {
      const float *w = r.w3 + (size_t)cell * r.h;
      for (uint32_t k = sub; k < r.h; k += 16) acc = fmaf(x[k], w[k], acc);
    }
    acc += __shfl_xor(acc, 8);
    acc += __shfl_xor(acc, 4);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 1);
    if (sub == 0 && j < nl) {
      const float z = cell != NONE ? acc + r.b3[cell] : -INFINITY;
      s_z[j] = z;
      r.z[(size_t)i * MAXA + j] = z;
    }
  }
  __syncthreads();
  float part = 0.0f;
  for (uint32_t j = lane; j < nl; j += 64) part += expf(s_z[j]);   // torch.exp, no maximum subtracted
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
  if (lane == 0) {
    if (nl == 0) r.z[(size_t)i * MAXA] = -INFINITY;   // (a caller-made row with an empty list: nothing is read from an earlier call)
    const float den = fmaxf(part, 1e-12f);   // normalize(p=1)'s eps
    const float q0 = nl ? expf(s_z[0]) / den : 0.0f;
    r.S[i] = part;
    r.q0[i] = q0;
    r.lp[i] = logf(q0);
    r.val[i] = 1.0f / (1.0f + expf(-r.zv[i]));
  }
}

__global__ __launch_bounds__(256) void k_keep_mark(Chunk c, RowBuffers r) {
  __shared__ uint32_t wave_live[gr::BLOCK / 64];
  const uint32_t i = blockIdx.x * gr::BLOCK + threadIdx.x;
  const bool kept = i < c.V && (c.keep ? c.keep[i] != 0 : true);
  gr::count_block_live(kept, wave_live, r.block_live);
}

// block_offset[blocks] holds k, the number of kept rows
__global__ __launch_bounds__(256) void k_select(Chunk c, RowBuffers r, uint32_t blocks) {
  __shared__ uint32_t wave_total[gr::BLOCK / 64], place[gr::BLOCK];
  const uint32_t i = blockIdx.x * gr::BLOCK + threadIdx.x;
  const bool kept = i < c.V && (c.keep ? c.keep[i] != 0 : true);
  const uint32_t to = gr::compact_place(kept, r.block_offset[blockIdx.x], wave_total, place);
  const uint32_t k = r.block_offset[blocks], n_cap = min(k, c.remaining);
  if (i < c.V) r.sel[i] = (kept && to < n_cap) ? 1 : 0;
  if (i == 0) r.report->rows = c.V, r.report->kept = k, r.report->n_cap = n_cap;
}

__global__ __launch_bounds__(64) void k_traj(Chunk c, RowBuffers r) {
#pragma clang fp contract(off)
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= c.n) return;
  float vf[STEPS], rew[STEPS], gae[STEPS], ret[STEPS], G[STEPS], dvf[STEPS];
  uint8_t ok[STEPS];
  int32_t at[STEPS];
  for (uint32_t t = 0; t < STEPS; ++t) {
    const size_t s = (size_t)b * STEPS + t;
    at[t] = r.row_index[s];
    ok[t] = (c.valid[s] != 0 && at[t] >= 0) ? 1 : 0;
    vf[t] = ok[t] ? r.val[at[t]] : 0.0f;
    rew[t] = c.rewards[s];
  }
  bl::gae_forward(vf, rew, ok, c.gamma, c.gamma_lam, gae, ret);
  const float scale = 1.0f / (float)c.total;
  for (uint32_t t = 0; t < STEPS; ++t) {
    G[t] = 0.0f;
    if (!ok[t]) continue;
    const uint32_t i = (uint32_t)at[t];
    const bool sel = r.sel[i] != 0;
    const float z0 = r.z[(size_t)i * MAXA], lp = r.lp[i];
    const float resid = ret[t] - vf[t];
    const float cf = bl::clipped_force(z0, gae[t]), forced = z0 * cf;
    r.gae[i] = gae[t], r.ret[i] = ret[t], r.cf[i] = cf, r.forced[i] = forced;
    r.terms[(size_t)i * 3 + 0] = sel ? forced : 0.0f;
    r.terms[(size_t)i * 3 + 1] = sel ? resid * resid : 0.0f;
    r.terms[(size_t)i * 3 + 2] = sel ? lp * expf(lp) : 0.0f;
    if (sel) G[t] = ((2.0f * scale) * c.vw) * resid;
  }
  bl::gae_backward(G, ok, c.gamma, c.gamma_lam, dvf);
  for (uint32_t t = 0; t < STEPS; ++t)
    if (ok[t]) r.du[at[t]] = dvf[t] * (vf[t] * (1.0f - vf[t]));
}

__global__ __launch_bounds__(64) void k_l3_backward(Chunk c, RowBuffers r) {
#pragma clang fp contract(off)   // (dz is the contract's written order; the sums below are explicit fmaf)
  __shared__ float s_dz[MAXA + 1];
  __shared__ uint32_t s_cell[MAXA + 1];
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  uint32_t b, t;
  const bool sel = r.sel[i] != 0;
  const uint32_t nl = (row_at(c, i, b, t) && sel) ? legal_count(c, b, t) : 0;
  const float scale = 1.0f / (float)c.total, S = r.S[i], q0 = r.q0[i], lp = r.lp[i];
  const float den = fmaxf(S, 1e-12f), ent = (scale * c.ew) * (q0 * (1.0f + lp)), force = (scale * c.pw) * r.cf[i];
  const bool clamped = S < 1e-12f;   // the denominator is the constant eps: the log-probability depends on z_0 alone
  for (uint32_t j = lane; j < nl; j += 64) {
    const uint32_t cell = legal_cell(c, b, t, j);
    float dz = 0.0f;
    if (cell != NONE) {
      const float q = clamped ? 0.0f : expf(r.z[(size_t)i * MAXA + j]) / den;
      dz = ent * ((j == 0 ? 1.0f : 0.0f) - q);
      if (j == 0) dz -= force;
    }
    s_dz[j] = dz, s_cell[j] = cell;
    r.dz[(size_t)i * MAXA + j] = dz;
  }
  __syncthreads();
  for (uint32_t col = lane; col < r.h; col += 64) {
    float total = 0.0f, mid = 0.0f, acc = 0.0f;
    uint32_t terms = 0, chains = 0;
    for (uint32_t j = 0; j < nl; ++j) {
      if (s_cell[j] == NONE) continue;
      acc = fmaf(s_dz[j], r.w3[(size_t)s_cell[j] * r.h + col], acc);
      if (++terms == CHAIN) {
        mid += acc, acc = 0.0f, terms = 0;
        if (++chains == MID) total += mid, mid = 0.0f, chains = 0;
      }
    }
    total += mid + acc;
    r.dz2p[(size_t)i * r.h + col] = total * r.d2p[(size_t)i * r.h + col];
  }
}

// The report in two levels, both in a fixed order: float64 sums of the terms of REPORT_ROWS rows per workgroup (thread t adding rows t,
// t + 256, ... of the slice, the 256 sums combined pairwise), then the slices' sums the same way in one workgroup.
constexpr uint32_t REPORT_ROWS = 4096;
__device__ __forceinline__ void report_sum(const double s[3], double part[3][256]) {
  for (int q = 0; q < 3; ++q) part[q][threadIdx.x] = s[q];
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (threadIdx.x < w)
      for (int q = 0; q < 3; ++q) part[q][threadIdx.x] += part[q][threadIdx.x + w];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_report_slices(const float *terms, uint32_t V, double *slices) {
  __shared__ double part[3][256];
  const uint32_t lo = blockIdx.x * REPORT_ROWS, hi = min(V, lo + REPORT_ROWS);
  double s[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256)
    for (int q = 0; q < 3; ++q) s[q] += (double)terms[(size_t)i * 3 + q];
  report_sum(s, part);
  if (threadIdx.x < 3) slices[(size_t)blockIdx.x * 3 + threadIdx.x] = part[threadIdx.x][0];
}
__global__ __launch_bounds__(256) void k_build_report(const double *slices, uint32_t count, Chunk c, Report *report) {
  __shared__ double part[3][256];
  double s[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = threadIdx.x; i < count; i += 256)
    for (int q = 0; q < 3; ++q) s[q] += slices[(size_t)i * 3 + q];
  report_sum(s, part);
  if (threadIdx.x == 0) {
    const double n = (double)report->n_cap, inv = n > 0.0 ? 1.0 / n : 0.0;
    report->policy_loss = -part[0][0] * inv;
    report->value_loss = part[1][0] * inv;
    report->entropy = -part[2][0] * inv;
    report->loss = (n / (double)c.total) * ((double)c.pw * report->policy_loss + (double)c.vw * report->value_loss - (double)c.ew * report->entropy);
  }
}

__global__ __launch_bounds__(256) void k_export_logits(Chunk c, const float *z, float *out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)c.V * MAXA) return;
  const uint32_t i = (uint32_t)(e / MAXA), j = (uint32_t)(e % MAXA);
  uint32_t b, t;
  const uint32_t nl = row_at(c, i, b, t) ? legal_count(c, b, t) : 0;
  out[e] = j < nl ? z[e] : __builtin_nanf("");
}

// ---- the inverted index ----------------------------------------------------------------------------------------------------------------------
struct StateKeys {   // entry e = row * 31 + slot
  const uint16_t *keys;
  __device__ uint32_t operator()(uint32_t e) const { const uint32_t k = keys[e]; return k < N_DIM ? k : NONE; }
};
struct ListKeys {    // entry e = row * 339 + position, of the selected rows
  Chunk c;
  const uint8_t *sel;
  __device__ uint32_t operator()(uint32_t e) const {
    const uint32_t i = e / MAXA, j = e - i * MAXA;
    uint32_t b, t;
    if (!sel[i] || !row_at(c, i, b, t) || j >= legal_count(c, b, t)) return NONE;
    return legal_cell(c, b, t, j);
  }
};

// hist[cell * blocks + block]: the entries of the block's range with that cell
template <class Keys> __global__ __launch_bounds__(256) void k_hist(Keys keys, uint32_t entries, uint32_t per_block, uint32_t blocks, uint32_t *hist) {
  __shared__ uint32_t count[N_DIM];
  for (uint32_t cell = threadIdx.x; cell < N_DIM; cell += 256) count[cell] = 0;
  __syncthreads();
  const uint32_t lo = min(entries, blockIdx.x * per_block), hi = min(entries, lo + per_block);
  for (uint32_t e = lo + threadIdx.x; e < hi; e += 256) {
    const uint32_t cell = keys(e);
    if (cell != NONE) atomicAdd(&count[cell], 1u);
  }
  __syncthreads();
  for (uint32_t cell = threadIdx.x; cell < N_DIM; cell += 256) hist[(size_t)cell * blocks + blockIdx.x] = count[cell];
}

// The exclusive scan of hist [cell][block] in two levels: a cell's total, game_rows.hpp's scan over the 3,749 totals, then each cell's blocks in
// order.  Integer sums: exact in any order.  offset[N_DIM * blocks] receives the number of entries.
__global__ __launch_bounds__(256) void k_cell_totals(const uint32_t *hist, uint32_t blocks, uint32_t *cell_total) {
  const uint32_t cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= N_DIM) return;
  uint32_t sum = 0;
  for (uint32_t b = 0; b < blocks; ++b) sum += hist[(size_t)cell * blocks + b];
  cell_total[cell] = sum;
}
__global__ __launch_bounds__(256) void k_cell_offsets(const uint32_t *hist, uint32_t blocks, const uint32_t *cell_offset, uint32_t *offset) {
  const uint32_t cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= N_DIM) return;
  uint32_t run = cell_offset[cell];
  for (uint32_t b = 0; b < blocks; ++b) {
    const uint32_t count = hist[(size_t)cell * blocks + b];
    offset[(size_t)cell * blocks + b] = run;
    run += count;
  }
  if (cell == N_DIM - 1) offset[(size_t)N_DIM * blocks] = run;
}

// One wave per block of the range, 64 entries a pass.  A pass whose cells are all different (the entries of one row's list are) takes its
// places at once: every lane owns next[cell].  Otherwise the lanes that hold the first remaining lane's cell take the places next[cell] ..
// in lane order, then the next cell, until the pass is placed.  Stable either way, and no place depends on the order of an atomic.
template <class Keys> __global__ __launch_bounds__(64) void k_place(Keys keys, uint32_t entries, uint32_t per_block, uint32_t blocks, const uint32_t *offset, uint32_t *sorted) {
  __shared__ uint32_t next[N_DIM];
  __shared__ uint8_t owner[N_DIM];
  const uint32_t lane = threadIdx.x;
  for (uint32_t cell = lane; cell < N_DIM; cell += 64) next[cell] = offset[(size_t)cell * blocks + blockIdx.x];
  __syncthreads();
  const uint32_t lo = min(entries, blockIdx.x * per_block), hi = min(entries, lo + per_block);
  for (uint32_t base = lo; base < hi; base += 64) {
    const uint32_t e = base + lane;
    const uint32_t cell = e < hi ? keys(e) : NONE;
    bool waiting = cell != NONE;
    unsigned long long left = __ballot(waiting);
    if (!left) continue;
    if (waiting) owner[cell] = (uint8_t)lane;
    __syncthreads();   // (a workgroup of one wave)
    const bool shared_cell = waiting && owner[cell] != (uint8_t)lane;   // of two lanes with one cell, one reads the other's id
    if (!__ballot(shared_cell)) {
      if (waiting) {
        const uint32_t first = next[cell];
        sorted[first] = e;
        next[cell] = first + 1;
      }
      __syncthreads();
      continue;
    }
    while (left) {
      const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1;
      const uint32_t its = (uint32_t)__shfl((int)cell, (int)leader);
      const bool same = waiting && cell == its;
      const unsigned long long m = __ballot(same);
      const uint32_t first = next[its];
      __syncthreads();   // every lane has read `first`
      if (same) {
        sorted[first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = e;
        waiting = false;
      }
      if (lane == leader) next[its] = first + (uint32_t)__popcll(m);
      __syncthreads();
      left &= ~m;
    }
  }
}

// pieces[cell] = the pieces of SEG entries its segment is cut into; offset[(size_t)N_DIM * blocks] holds the number of entries
__global__ __launch_bounds__(256) void k_seg_pieces(const uint32_t *offset, uint32_t blocks, uint32_t *pieces) {
  const uint32_t cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= N_DIM) return;
  const uint32_t len = offset[(size_t)(cell + 1) * blocks] - offset[(size_t)cell * blocks];
  pieces[cell] = (len + SEG - 1) / SEG;
}

struct SegArgs {
  const uint32_t *sorted, *offset, *piece_offset;   // piece_offset [N_DIM + 1]
  uint32_t blocks;
  const float *D;         // [rows][width]
  uint32_t width, per;    // row of entry e = e / per
  const float *weights;   // nullable (1): per entry
  uint32_t ones;          // column `width` reads as 1 (the bias)
  float *part;            // [pieces][width + ones]
  float *out_w, *out_b;   // [N_DIM][width], [N_DIM]
};

__global__ __launch_bounds__(256) void k_seg_partial(SegArgs a) {
  const uint32_t piece = blockIdx.x;
  if (piece >= a.piece_offset[N_DIM]) return;
  uint32_t lo = 0, hi = N_DIM;   // the last cell whose first piece is not behind this one: it has pieces, since piece < the total
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (a.piece_offset[mid] <= piece) lo = mid; else hi = mid;
  }
  const uint32_t cell = lo;
  const uint32_t begin = a.offset[(size_t)cell * a.blocks] + (piece - a.piece_offset[cell]) * SEG;
  const uint32_t end = min(a.offset[(size_t)(cell + 1) * a.blocks], begin + SEG);
  const uint32_t cols = a.width + a.ones;
  for (uint32_t col = threadIdx.x; col < cols; col += 256) {
    float mid = 0.0f, acc = 0.0f;
    uint32_t terms = 0;
    for (uint32_t q = begin; q < end; ++q) {
      const uint32_t e = a.sorted[q], row = e / a.per;
      const float w = a.weights ? a.weights[e] : 1.0f;
      const float x = col < a.width ? a.D[(size_t)row * a.width + col] : 1.0f;
      acc = fmaf(w, x, acc);
      if (++terms == CHAIN) mid += acc, acc = 0.0f, terms = 0;
    }
    a.part[(size_t)piece * cols + col] = mid + acc;
  }
}

// a cell's pieces pairwise in a fixed order (in place), as k_reduce combines the K ranges of a dense product
__global__ __launch_bounds__(256) void k_seg_combine(SegArgs a) {
  const uint32_t cols = a.width + a.ones;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)N_DIM * cols) return;
  const uint32_t cell = (uint32_t)(idx / cols), col = (uint32_t)(idx % cols);
  const uint32_t first = a.piece_offset[cell], count = a.piece_offset[cell + 1] - first;
  if (count == 0) return;   // no entry reaches this cell: its gradient is left as it is
  float *v = a.part + (size_t)first * cols + col;
  for (uint32_t stride = 1; stride < count; stride *= 2)
    for (uint32_t i = 0; i + stride < count; i += 2 * stride) v[(size_t)i * cols] += v[(size_t)(i + stride) * cols];
  if (col < a.width) a.out_w[(size_t)cell * a.width + col] = v[0]; else a.out_b[cell] = v[0];
}

// ---- elementwise over the block --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_accumulate(float *grad, const float *chunk, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) grad[i] = grad[i] + chunk[i];
}
__global__ __launch_bounds__(256) void k_zero(float *x, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) x[i] = 0.0f;
}
// avg.mul_(g).add_(p, alpha = 1 - g): two products and one sum, each rounded
__global__ __launch_bounds__(256) void k_average(float *avg, const float *p, float g, float omg, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) avg[i] = __fadd_rn(__fmul_rn(avg[i], g), __fmul_rn(omg, p[i]));
}

uint32_t grid_of(size_t items) { return (uint32_t)((items + 255) / 256); }

// ---- the file ----------------------------------------------------------------------------------------------------------------------------------
struct FileLayer { uint32_t in, out; size_t bias, weight; };   // byte offsets into the file

int parse_file(const char *fn, const uint8_t *net, size_t size, FileLayer L[6]) {
  RC(oakgpu_build_net_check(net, size));
  size_t pos = 0;
  for (int k = 0; k < 6; ++k) {
    uint32_t dims[2];
    memcpy(dims, net + pos, 8);
    L[k] = FileLayer{dims[0], dims[1], pos + 8, pos + 8 + 4 * (size_t)dims[1]};
    pos += 8 + 4 * (size_t)dims[1] * ((size_t)dims[0] + 1);
  }
  if (L[3].out > MAX_WIDTH || L[4].out > MAX_WIDTH) return fail(fn, "value hidden width above 256");
  return 0;
}
} // namespace

struct oakgpu_build_trainer {
  oakgpu_ctx *ctx = nullptr;
  NetLayout net[2];
  uint32_t dims[12] = {};
  size_t count = 0;
  uint32_t max_traj = 0, max_rows = 0;
  float *block = nullptr;   // parameters | gradients | m | v | average | the chunk's own gradient, each `count` floats
  uint8_t *kind = nullptr;  // k_adam's groups: one, no clamp
  float *work = nullptr;
  uint32_t *iwork = nullptr;
  Report *report = nullptr;
  double *report_slices = nullptr;   // [rows / REPORT_ROWS][3]
  uint64_t steps = 0;
  // workspaces
  float *y1[2] = {}, *d1[2] = {}, *y2[2] = {}, *d2[2] = {}, *dz2[2] = {}, *da1[2] = {};
  float *zv = nullptr, *z = nullptr, *dz = nullptr, *S = nullptr, *lp = nullptr, *q0 = nullptr, *val = nullptr, *gae = nullptr, *ret = nullptr, *cf = nullptr,
        *forced = nullptr, *du = nullptr, *terms = nullptr, *partials = nullptr, *seg_part = nullptr;
  uint32_t *row_index = nullptr, *block_live = nullptr, *block_offset = nullptr, *hist = nullptr, *hist_offset = nullptr, *pieces = nullptr, *piece_offset = nullptr,
           *sorted_state = nullptr, *sorted_list = nullptr;
  uint16_t *keys = nullptr;
  uint8_t *sel = nullptr;
  float *part(int which) const { return block + (size_t)which * count; }
  float *chunk_grad() const { return block + 5 * count; }
};

namespace {
uint32_t hist_blocks(size_t entries) { return (uint32_t)std::min<size_t>(std::max<size_t>((entries + HIST_SLOTS - 1) / HIST_SLOTS, 1), HIST_BLOCKS); }
uint32_t splits_of(uint32_t rows) { return std::min<uint32_t>((rows + SPAN - 1) / SPAN, MAX_SPLITS); }

View plain(const float *p, uint32_t rows, uint32_t cols) {
  View v{};
  v.p = p, v.rows = rows, v.cols = cols, v.ld = cols, v.mode = V_PLAIN;
  return v;
}
int launch_gemm(hipStream_t stream, const GemmArgs &g, uint32_t splits) {
  dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, splits);
  hipLaunchKernelGGL(k_gemm, grid, dim3(256), 0, stream, g);
  HIPCHK(hipGetLastError());
  return 0;
}
// Y = act(X W^T + b): X [V][in], W [out][in]
int dense_forward(hipStream_t stream, const float *x, uint32_t V, uint32_t in, uint32_t out, const float *w, const float *b, uint32_t act, float *y, float *deriv) {
  GemmArgs g{};
  g.a = plain(x, V, in), g.b = plain(w, out, in);
  g.ta = 0, g.tb = 1, g.M = V, g.N = out, g.K = in, g.klen = in, g.epi = EPI_FWD;
  g.bias = b, g.act = act, g.deriv = deriv, g.out = y, g.ldo = out;
  return launch_gemm(stream, g, 1);
}
// dX = dZ W (times a factor): dZ [V][out], W [out][in]
int dense_input_grad(hipStream_t stream, const float *dz, uint32_t V, uint32_t in, uint32_t out, const float *w, const float *mask, float *dx) {
  GemmArgs g{};
  g.a = plain(dz, V, out), g.b = plain(w, out, in);
  g.M = V, g.N = in, g.K = out, g.klen = out, g.epi = EPI_DX, g.out = dx, g.ldo = in, g.mask = mask;
  return launch_gemm(stream, g, 1);
}
// dW|db = dZ^T [X|1] into gw [out][in], gb [out]; in == 0: the bias alone
int dense_weight_grad(hipStream_t stream, oakgpu_build_trainer *t, const float *dz, const float *x, uint32_t V, uint32_t in, uint32_t out, float *gw, float *gb) {
  const uint32_t splits = splits_of(V);
  GemmArgs g{};
  g.a = plain(dz, V, out), g.b = plain(x, V, in);
  g.b.ones = 1;
  g.ta = 1, g.tb = 0, g.M = out, g.N = in + 1, g.K = V;
  g.klen = ((V + splits - 1) / splits + SPAN - 1) / SPAN * SPAN;
  g.epi = EPI_DW, g.out = t->partials;
  RC(launch_gemm(stream, g, splits));
  hipLaunchKernelGGL(k_reduce, dim3(grid_of((size_t)g.M * g.N)), dim3(256), 0, stream, t->partials, splits, out, in, gb, gw);
  HIPCHK(hipGetLastError());
  return 0;
}

// the inverted index of `entries` keyed entries into `sorted`; its offsets stay in t->hist_offset, its pieces in t->piece_offset
template <class Keys> int build_index(hipStream_t stream, oakgpu_build_trainer *t, const Keys &keys, size_t entries, uint32_t *sorted, uint32_t &blocks) {
  blocks = hist_blocks(entries);
  const uint32_t per_block = (uint32_t)((entries + blocks - 1) / blocks);
  hipLaunchKernelGGL(k_hist<Keys>, dim3(blocks), dim3(256), 0, stream, keys, (uint32_t)entries, per_block, blocks, t->hist);
  hipLaunchKernelGGL(k_cell_totals, dim3(grid_of(N_DIM)), dim3(256), 0, stream, t->hist, blocks, t->pieces);
  hipLaunchKernelGGL(gr::k_rows_offsets, dim3(1), dim3(1024), 0, stream, t->pieces, N_DIM, t->piece_offset, t->piece_offset + N_DIM);
  hipLaunchKernelGGL(k_cell_offsets, dim3(grid_of(N_DIM)), dim3(256), 0, stream, t->hist, blocks, t->piece_offset, t->hist_offset);
  hipLaunchKernelGGL(k_place<Keys>, dim3(blocks), dim3(64), 0, stream, keys, (uint32_t)entries, per_block, blocks, t->hist_offset, sorted);
  hipLaunchKernelGGL(k_seg_pieces, dim3(grid_of(N_DIM)), dim3(256), 0, stream, t->hist_offset, blocks, t->pieces);
  hipLaunchKernelGGL(gr::k_rows_offsets, dim3(1), dim3(1024), 0, stream, t->pieces, N_DIM, t->piece_offset, t->piece_offset + N_DIM);
  HIPCHK(hipGetLastError());
  return 0;
}
int segment_sums(hipStream_t stream, oakgpu_build_trainer *t, const uint32_t *sorted, uint32_t blocks, size_t entries, const float *D, uint32_t width, uint32_t per,
                 const float *weights, float *out_w, float *out_b) {
  SegArgs a{sorted, t->hist_offset, t->piece_offset, blocks, D, width, per, weights, out_b ? 1u : 0u, t->seg_part, out_w, out_b};
  const uint32_t most = (uint32_t)(entries / SEG) + N_DIM;   // every cell ends on at most one short piece
  hipLaunchKernelGGL(k_seg_partial, dim3(most), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(k_seg_combine, dim3(grid_of((size_t)N_DIM * (width + a.ones))), dim3(256), 0, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int check_chunk(const char *fn, oakgpu_ctx *ctx, oakgpu_build_trainer *t, const oakgpu_build_chunk *c) {
  if (!ctx || !t || !c) return fail(fn, "null argument");
  if (t->ctx != ctx) return fail(fn, "the trainer belongs to another context");
  if (c->n == 0) return fail(fn, "n == 0");
  if (c->n > t->max_traj) return fail(fn, "n = " + std::to_string(c->n) + " trajectories exceed max_traj = " + std::to_string(t->max_traj));
  if (c->n_valid > c->n * STEPS) return fail(fn, "n_valid exceeds n x 31");
  if (c->mask_dtype != OAKGPU_BUILD_MASK_INT64 && c->mask_dtype != OAKGPU_BUILD_MASK_INT16) return fail(fn, "mask_dtype outside {int64, int16}");
  if (!c->mask || !c->n_legal || !c->valid || !c->rewards || !c->rows || !c->state_cells || !c->state_n) return fail(fn, "the chunk lacks an array the trainer reads");
  if (c->total == 0) return fail(fn, "total == 0");
  if (!(c->gamma == c->gamma) || !(c->gamma_lam == c->gamma_lam)) return fail(fn, "gamma or gamma_lam is NaN");
  return oakgpu_ctx_enter(ctx);
}

Chunk chunk_of(const oakgpu_build_chunk *c) {
  return Chunk{c->mask, c->mask_dtype, c->n_legal, c->valid, c->rewards, c->rows, c->state_cells, c->state_n, c->keep, c->n, c->n_valid, c->total, c->remaining,
               (float)c->gamma, (float)c->gamma_lam, c->policy_loss_weight, c->value_loss_weight, c->entropy_loss_weight};
}

RowBuffers row_buffers(oakgpu_build_trainer *t) {
  RowBuffers r{};
  const NetLayout &p = t->net[0];
  r.y2p = t->y2[0], r.d2p = t->d2[0], r.w3 = t->part(0) + p.w3, r.b3 = t->part(0) + p.b3, r.h = p.h2, r.zv = t->zv, r.z = t->z, r.dz = t->dz;
  r.S = t->S, r.lp = t->lp, r.q0 = t->q0, r.val = t->val, r.gae = t->gae, r.ret = t->ret, r.cf = t->cf, r.forced = t->forced, r.du = t->du, r.terms = t->terms;
  r.dz2p = t->dz2[0], r.sel = t->sel, r.row_index = (const int32_t *)t->row_index, r.block_live = t->block_live, r.block_offset = t->block_offset, r.report = t->report;
  return r;
}

// the forward of both nets, the selection, the per-trajectory pass and the report (V >= 1)
int run_forward(oakgpu_build_trainer *t, const Chunk &c) {
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(t->ctx);
  const uint32_t V = c.V;
  const float *P = t->part(0);
  HIPCHK(hipMemsetAsync(t->row_index, 0xFF, (size_t)c.n * STEPS * 4, stream));
  hipLaunchKernelGGL(k_row_index, dim3(grid_of(V)), dim3(256), 0, stream, c, (int32_t *)t->row_index);
  hipLaunchKernelGGL(k_state_keys, dim3(grid_of((size_t)V * STEPS)), dim3(256), 0, stream, c, t->keys);
  for (int k = 0; k < 2; ++k) {
    const NetLayout &L = t->net[k];
    hipLaunchKernelGGL(k_layer1, dim3(grid_of((size_t)V * L.h1)), dim3(256), 0, stream, t->keys, V, P + L.w1t, P + L.b1, L.h1, t->y1[k], t->d1[k]);
    HIPCHK(hipGetLastError());
    RC(dense_forward(stream, t->y1[k], V, L.h1, L.h2, P + L.w2, P + L.b2, 1, t->y2[k], t->d2[k]));
  }
  const NetLayout &Lv = t->net[1];
  RC(dense_forward(stream, t->y2[1], V, Lv.h2, 1, P + Lv.w3, P + Lv.b3, 0, t->zv, nullptr));
  const RowBuffers r = row_buffers(t);
  const uint32_t blocks = (V + gr::BLOCK - 1) / gr::BLOCK;
  hipLaunchKernelGGL(k_l3_forward, dim3(V), dim3(64), 0, stream, c, r);
  hipLaunchKernelGGL(k_keep_mark, dim3(blocks), dim3(gr::BLOCK), 0, stream, c, r);
  hipLaunchKernelGGL(gr::k_rows_offsets, dim3(1), dim3(1024), 0, stream, t->block_live, blocks, t->block_offset, t->block_offset + blocks);
  hipLaunchKernelGGL(k_select, dim3(blocks), dim3(gr::BLOCK), 0, stream, c, r, blocks);
  HIPCHK(hipMemsetAsync(t->terms, 0, (size_t)V * 3 * 4, stream));
  HIPCHK(hipMemsetAsync(t->du, 0, (size_t)V * 4, stream));
  hipLaunchKernelGGL(k_traj, dim3((c.n + 63) / 64), dim3(64), 0, stream, c, r);
  const uint32_t slices = (V + REPORT_ROWS - 1) / REPORT_ROWS;
  hipLaunchKernelGGL(k_report_slices, dim3(slices), dim3(256), 0, stream, t->terms, V, t->report_slices);
  hipLaunchKernelGGL(k_build_report, dim3(1), dim3(256), 0, stream, t->report_slices, slices, c, t->report);
  HIPCHK(hipGetLastError());
  return 0;
}

int run_backward(oakgpu_build_trainer *t, const Chunk &c) {
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(t->ctx);
  const uint32_t V = c.V;
  const float *P = t->part(0);
  float *G = t->chunk_grad();
  const RowBuffers r = row_buffers(t);
  const NetLayout &Lp = t->net[0], &Lv = t->net[1];
  HIPCHK(hipMemsetAsync(G, 0, t->count * 4, stream));
  // layer 3: the policy's list, the value's one row
  hipLaunchKernelGGL(k_l3_backward, dim3(V), dim3(64), 0, stream, c, r);
  HIPCHK(hipGetLastError());
  RC(dense_weight_grad(stream, t, t->du, t->y2[1], V, Lv.h2, 1, G + Lv.w3, G + Lv.b3));
  RC(dense_input_grad(stream, t->du, V, Lv.h2, 1, P + Lv.w3, t->d2[1], t->dz2[1]));
  uint32_t blocks = 0;
  const size_t list_entries = (size_t)V * MAXA, state_entries = (size_t)V * STEPS;
  RC(build_index(stream, t, ListKeys{c, t->sel}, list_entries, t->sorted_list, blocks));
  RC(segment_sums(stream, t, t->sorted_list, blocks, list_entries, t->y2[0], Lp.h2, MAXA, t->dz, G + Lp.w3, G + Lp.b3));
  // layers 2 and 1, both nets
  for (int k = 0; k < 2; ++k) {
    const NetLayout &L = t->net[k];
    RC(dense_weight_grad(stream, t, t->dz2[k], t->y1[k], V, L.h1, L.h2, G + L.w2, G + L.b2));
    RC(dense_input_grad(stream, t->dz2[k], V, L.h1, L.h2, P + L.w2, t->d1[k], t->da1[k]));
    RC(dense_weight_grad(stream, t, t->da1[k], nullptr, V, 0, L.h1, nullptr, G + L.b1));
  }
  RC(build_index(stream, t, StateKeys{t->keys}, state_entries, t->sorted_state, blocks));
  for (int k = 0; k < 2; ++k)
    RC(segment_sums(stream, t, t->sorted_state, blocks, state_entries, t->da1[k], t->net[k].h1, STEPS, nullptr, G + t->net[k].w1t, nullptr));
  hipLaunchKernelGGL(k_accumulate, dim3(grid_of(t->count)), dim3(256), 0, stream, t->part(OAKGPU_BUILD_TRAIN_GRADIENTS), G, t->count);
  HIPCHK(hipGetLastError());
  return 0;
}

int empty_report(oakgpu_build_trainer *t) {
  HIPCHK(hipMemsetAsync(t->report, 0, sizeof(Report), (hipStream_t)oakgpu_ctx_stream(t->ctx)));
  return 0;
}

// working layout <-> file order ([out][in] per layer, bias in front of the weights); w1 is the one tensor that differs
void to_file(const oakgpu_build_trainer *t, const float *work, float *file) {
  size_t at = 0;
  for (int k = 0; k < 2; ++k) {
    const NetLayout &L = t->net[k];
    memcpy(file + at, work + L.b1, 4 * (size_t)L.h1), at += L.h1;
    for (uint32_t j = 0; j < L.h1; ++j)
      for (uint32_t c = 0; c < N_DIM; ++c) file[at + (size_t)j * N_DIM + c] = work[L.w1t + (size_t)c * L.h1 + j];
    at += (size_t)L.h1 * N_DIM;
    memcpy(file + at, work + L.b2, 4 * (size_t)L.h2), at += L.h2;
    memcpy(file + at, work + L.w2, 4 * (size_t)L.h2 * L.h1), at += (size_t)L.h2 * L.h1;
    memcpy(file + at, work + L.b3, 4 * (size_t)L.out), at += L.out;
    memcpy(file + at, work + L.w3, 4 * (size_t)L.out * L.h2), at += (size_t)L.out * L.h2;
  }
}
void from_file(const oakgpu_build_trainer *t, const float *file, float *work) {
  size_t at = 0;
  for (int k = 0; k < 2; ++k) {
    const NetLayout &L = t->net[k];
    memcpy(work + L.b1, file + at, 4 * (size_t)L.h1), at += L.h1;
    for (uint32_t j = 0; j < L.h1; ++j)
      for (uint32_t c = 0; c < N_DIM; ++c) work[L.w1t + (size_t)c * L.h1 + j] = file[at + (size_t)j * N_DIM + c];
    at += (size_t)L.h1 * N_DIM;
    memcpy(work + L.b2, file + at, 4 * (size_t)L.h2), at += L.h2;
    memcpy(work + L.w2, file + at, 4 * (size_t)L.h2 * L.h1), at += (size_t)L.h2 * L.h1;
    memcpy(work + L.b3, file + at, 4 * (size_t)L.out), at += L.out;
    memcpy(work + L.w3, file + at, 4 * (size_t)L.out * L.h2), at += (size_t)L.out * L.h2;
  }
}
int check_handle(const char *fn, oakgpu_ctx *ctx, oakgpu_build_trainer *t) {
  if (!ctx || !t) return fail(fn, "null argument");
  if (t->ctx != ctx) return fail(fn, "the trainer belongs to another context");
  return oakgpu_ctx_enter(ctx);
}
} // namespace

extern "C" {

int oakgpu_build_trainer_check(const uint8_t *net, size_t size, uint32_t max_traj) {
  const char *fn = "oakgpu_build_trainer_check";
  FileLayer L[6];
  RC(parse_file(fn, net, size, L));
  if (max_traj == 0 || max_traj > MAX_TRAJ) return fail(fn, "max_traj must be in 1 .. " + std::to_string(MAX_TRAJ));
  return 0;
}

void oakgpu_build_trainer_destroy(oakgpu_build_trainer *t) {
  if (!t) return;
  if (t->ctx && oakgpu_ctx_enter(t->ctx) == 0) (void)hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(t->ctx));
  (void)hipFree(t->block);
  (void)hipFree(t->kind);
  (void)hipFree(t->work);
  (void)hipFree(t->iwork);
  (void)hipFree(t->report);
  (void)hipFree(t->report_slices);
  delete t;
}

int oakgpu_build_trainer_create(oakgpu_ctx *ctx, const uint8_t *net, size_t size, uint32_t max_traj, oakgpu_build_trainer **out) {
  const char *fn = "oakgpu_build_trainer_create";
  if (!ctx || !out) return fail(fn, "null argument");
  *out = nullptr;
  FileLayer F[6];
  RC(parse_file(fn, net, size, F));
  if (max_traj == 0 || max_traj > MAX_TRAJ) return fail(fn, "max_traj must be in 1 .. " + std::to_string(MAX_TRAJ));
  RC(oakgpu_ctx_enter(ctx));
  oakgpu_build_trainer *t = new oakgpu_build_trainer;
  t->ctx = ctx, t->max_traj = max_traj, t->max_rows = max_traj * STEPS;
  size_t count = 0;
  for (int k = 0; k < 2; ++k) {
    NetLayout &L = t->net[k];
    L.h1 = F[3 * k].out, L.h2 = F[3 * k + 1].out, L.out = F[3 * k + 2].out;
    L.w1t = count, count += (size_t)N_DIM * L.h1;
    L.b1 = count, count += L.h1;
    L.w2 = count, count += (size_t)L.h2 * L.h1;
    L.b2 = count, count += L.h2;
    L.w3 = count, count += (size_t)L.out * L.h2;
    L.b3 = count, count += L.out;
    for (int q = 0; q < 3; ++q) t->dims[6 * k + 2 * q] = F[3 * k + q].in, t->dims[6 * k + 2 * q + 1] = F[3 * k + q].out;
  }
  t->count = count;
  std::vector<float> file(count), work(count);
  {
    size_t at = 0;
    for (int k = 0; k < 6; ++k) {
      const size_t floats = (size_t)F[k].out * (F[k].in + 1);
      memcpy(file.data() + at, net + F[k].bias, 4 * floats);   // (the weights follow the biases in the file)
      at += floats;
    }
  }
  from_file(t, file.data(), work.data());
  // workspaces
  const size_t R = t->max_rows;
  size_t total = 0, itotal = 0;
  std::vector<std::pair<float **, size_t>> carve;
  std::vector<std::pair<uint32_t **, size_t>> icarve;
  auto want = [&](float *&p, size_t floats) { carve.push_back({&p, total}); total += (floats + 3) & ~(size_t)3; };
  auto iwant = [&](uint32_t *&p, size_t words) { icarve.push_back({&p, itotal}); itotal += (words + 3) & ~(size_t)3; };
  size_t partial = 0;
  uint32_t widest = 0;
  for (int k = 0; k < 2; ++k) {
    const NetLayout &L = t->net[k];
    want(t->y1[k], R * L.h1), want(t->d1[k], R * L.h1), want(t->da1[k], R * L.h1);
    want(t->y2[k], R * L.h2), want(t->d2[k], R * L.h2), want(t->dz2[k], R * L.h2);
    partial = std::max(partial, (size_t)MAX_SPLITS * L.h2 * (L.h1 + 1));
    widest = std::max(widest, L.h1);
  }
  partial = std::max(partial, (size_t)MAX_SPLITS * (t->net[1].h2 + 1));
  want(t->zv, R), want(t->S, R), want(t->lp, R), want(t->q0, R), want(t->val, R), want(t->gae, R), want(t->ret, R), want(t->cf, R), want(t->forced, R), want(t->du, R);
  want(t->terms, R * 3), want(t->z, R * MAXA), want(t->dz, R * MAXA), want(t->partials, partial);
  const size_t list_pieces = R * MAXA / SEG + N_DIM, state_pieces = R * STEPS / SEG + N_DIM;
  want(t->seg_part, std::max(list_pieces * (t->net[0].h2 + 1), state_pieces * (size_t)widest));
  const size_t cells = (size_t)N_DIM * HIST_BLOCKS, row_blocks = (R + gr::BLOCK - 1) / gr::BLOCK;
  iwant(t->row_index, R), iwant(t->block_live, row_blocks), iwant(t->block_offset, row_blocks + 1), iwant(t->hist, cells), iwant(t->hist_offset, cells + 1);
  iwant(t->pieces, N_DIM), iwant(t->piece_offset, N_DIM + 1), iwant(t->sorted_state, R * STEPS), iwant(t->sorted_list, R * MAXA);
  uint32_t *keys = nullptr, *sel = nullptr;
  iwant(keys, (R * STEPS + 1) / 2), iwant(sel, (R + 3) / 4);
  auto failed = [&](int rc) { oakgpu_build_trainer_destroy(t); return rc; };
  if (int rc = dev_alloc(t->block, 6 * count)) return failed(rc);
  if (int rc = dev_alloc(t->kind, count)) return failed(rc);
  if (int rc = dev_alloc(t->work, total)) return failed(rc);
  if (int rc = dev_alloc(t->iwork, itotal)) return failed(rc);
  if (int rc = dev_alloc(t->report, 1)) return failed(rc);
  if (int rc = dev_alloc(t->report_slices, 3 * ((R + REPORT_ROWS - 1) / REPORT_ROWS))) return failed(rc);
  for (auto &c : carve) *c.first = t->work + c.second;
  for (auto &c : icarve) *c.first = t->iwork + c.second;
  t->keys = (uint16_t *)keys, t->sel = (uint8_t *)sel;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  hipError_t e = hipMemsetAsync(t->block, 0, 6 * count * sizeof(float), stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->kind, 0, count, stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->report, 0, sizeof(Report), stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->part(OAKGPU_BUILD_TRAIN_PARAMETERS), work.data(), count * 4, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->part(OAKGPU_BUILD_TRAIN_AVERAGE), work.data(), count * 4, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (the host vectors go away)
  if (e != hipSuccess) return failed(oakgpu_fail_hip((int)e, "oakgpu_build_trainer_create: upload"));
  *out = t;
  return 0;
}

int oakgpu_build_trainer_shape(const oakgpu_build_trainer *t, uint32_t dims[12], size_t *count, uint32_t *max_traj) {
  if (!t) return fail("oakgpu_build_trainer_shape", "null trainer");
  if (dims) memcpy(dims, t->dims, sizeof t->dims);
  if (count) *count = t->count;
  if (max_traj) *max_traj = t->max_traj;
  return 0;
}

int oakgpu_build_trainer_forward_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t, const oakgpu_build_chunk *chunk, const oakgpu_build_train_outputs *out) {
  const char *fn = "oakgpu_build_trainer_forward_dev";
  RC(check_chunk(fn, ctx, t, chunk));
  if (chunk->n_valid == 0) return empty_report(t);
  const Chunk c = chunk_of(chunk);
  RC(run_forward(t, c));
  if (!out) return 0;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  const size_t V = c.V;
  if (out->logits) hipLaunchKernelGGL(k_export_logits, dim3(grid_of(V * MAXA)), dim3(256), 0, stream, c, t->z, out->logits);
  HIPCHK(hipGetLastError());
  auto copy = [&](void *dst, const void *src, size_t bytes) -> hipError_t { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream) : hipSuccess; };
  HIPCHK(copy(out->value, t->val, V * 4));
  HIPCHK(copy(out->logp, t->lp, V * 4));
  HIPCHK(copy(out->gae, t->gae, V * 4));
  HIPCHK(copy(out->returns, t->ret, V * 4));
  HIPCHK(copy(out->forced, t->forced, V * 4));
  HIPCHK(copy(out->selected, t->sel, V));
  HIPCHK(copy(out->du, t->du, V * 4));
  return 0;
}

int oakgpu_build_trainer_accumulate_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t, const oakgpu_build_chunk *chunk) {
  const char *fn = "oakgpu_build_trainer_accumulate_dev";
  RC(check_chunk(fn, ctx, t, chunk));
  if (chunk->n_valid == 0) return empty_report(t);
  const Chunk c = chunk_of(chunk);
  RC(run_forward(t, c));
  return run_backward(t, c);
}

int oakgpu_build_trainer_zero_gradients_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t) {
  RC(check_handle("oakgpu_build_trainer_zero_gradients_dev", ctx, t));
  hipLaunchKernelGGL(k_zero, dim3(grid_of(t->count)), dim3(256), 0, (hipStream_t)oakgpu_ctx_stream(ctx), t->part(OAKGPU_BUILD_TRAIN_GRADIENTS), t->count);
  HIPCHK(hipGetLastError());
  return 0;
}

int oakgpu_build_trainer_adam_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t, float lr) {
  const char *fn = "oakgpu_build_trainer_adam_dev";
  RC(check_handle(fn, ctx, t));
  if (!(lr >= 0.0f)) return fail(fn, "lr must be a number >= 0");
  AdamArgs a{};
  a.p = t->part(OAKGPU_BUILD_TRAIN_PARAMETERS), a.g = t->part(OAKGPU_BUILD_TRAIN_GRADIENTS), a.m = t->part(OAKGPU_BUILD_TRAIN_M), a.v = t->part(OAKGPU_BUILD_TRAIN_V);
  a.kind = t->kind, a.count = t->count;
  const double b1 = 0.9, b2 = 0.999, step = (double)++t->steps;
  a.b1 = (float)b1, a.omb1 = (float)(1.0 - b1), a.b2 = (float)b2, a.omb2 = (float)(1.0 - b2), a.eps = 1e-8f;
  a.step_size[0] = (float)((double)lr / (1.0 - pow(b1, step)));
  a.bc2_sqrt[0] = (float)sqrt(1.0 - pow(b2, step));
  a.groups = 1;
  hipLaunchKernelGGL(k_adam, dim3(grid_of(a.count)), dim3(256), 0, (hipStream_t)oakgpu_ctx_stream(ctx), a);
  HIPCHK(hipGetLastError());
  return 0;
}

int oakgpu_build_trainer_average_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t, double g) {
  const char *fn = "oakgpu_build_trainer_average_dev";
  RC(check_handle(fn, ctx, t));
  if (!(g >= 0.0 && g <= 1.0)) return fail(fn, "the average's gamma must be in 0 .. 1");
  hipLaunchKernelGGL(k_average, dim3(grid_of(t->count)), dim3(256), 0, (hipStream_t)oakgpu_ctx_stream(ctx), t->part(OAKGPU_BUILD_TRAIN_AVERAGE),
                     t->part(OAKGPU_BUILD_TRAIN_PARAMETERS), (float)g, (float)(1.0 - g), t->count);
  HIPCHK(hipGetLastError());
  return 0;
}

int oakgpu_build_trainer_report(oakgpu_ctx *ctx, oakgpu_build_trainer *t, oakgpu_build_train_report *out) {
  const char *fn = "oakgpu_build_trainer_report";
  RC(check_handle(fn, ctx, t));
  if (!out) return fail(fn, "null argument");
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  Report r;
  HIPCHK(hipMemcpyAsync(&r, t->report, sizeof r, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  out->rows = r.rows, out->kept = r.kept, out->n_cap = r.n_cap;
  out->policy_loss = r.policy_loss, out->value_loss = r.value_loss, out->entropy = r.entropy, out->loss = r.loss;
  out->steps = t->steps;
  return 0;
}

int oakgpu_build_trainer_read(oakgpu_ctx *ctx, oakgpu_build_trainer *t, int which, float *host, size_t count) {
  const char *fn = "oakgpu_build_trainer_read";
  RC(check_handle(fn, ctx, t));
  if (!host) return fail(fn, "null argument");
  if (which < 0 || which > OAKGPU_BUILD_TRAIN_AVERAGE) return fail(fn, "which must be OAKGPU_BUILD_TRAIN_PARAMETERS, _GRADIENTS, _M, _V or _AVERAGE");
  if (count != t->count) return fail(fn, "count is not the trainer's parameter count");
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  std::vector<float> work(count);
  HIPCHK(hipMemcpyAsync(work.data(), t->part(which), count * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  to_file(t, work.data(), host);
  return 0;
}

int oakgpu_build_trainer_set_gradients(oakgpu_ctx *ctx, oakgpu_build_trainer *t, const float *host, size_t count) {
  const char *fn = "oakgpu_build_trainer_set_gradients";
  RC(check_handle(fn, ctx, t));
  if (!host) return fail(fn, "null argument");
  if (count != t->count) return fail(fn, "count is not the trainer's parameter count");
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  std::vector<float> work(count);
  from_file(t, host, work.data());
  HIPCHK(hipMemcpyAsync(t->part(OAKGPU_BUILD_TRAIN_GRADIENTS), work.data(), count * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_build_trainer_net_bytes(oakgpu_ctx *ctx, oakgpu_build_trainer *t, int which, uint8_t *out, size_t capacity, size_t *size) {
  const char *fn = "oakgpu_build_trainer_net_bytes";
  if (!ctx || !t || !size) return fail(fn, "null argument");
  if (which != OAKGPU_BUILD_TRAIN_PARAMETERS && which != OAKGPU_BUILD_TRAIN_AVERAGE) return fail(fn, "which must be OAKGPU_BUILD_TRAIN_PARAMETERS or _AVERAGE");
  *size = 8 * 6 + 4 * t->count;
  if (!out) return 0;
  if (capacity < *size) return fail(fn, "the buffer is too small");
  std::vector<float> file(t->count);
  RC(oakgpu_build_trainer_read(ctx, t, which, file.data(), t->count));
  size_t pos = 0, at = 0;
  for (int k = 0; k < 6; ++k) {
    const uint32_t dims[2] = {t->dims[2 * k], t->dims[2 * k + 1]};
    const size_t floats = (size_t)dims[1] * (dims[0] + 1);
    memcpy(out + pos, dims, 8);
    memcpy(out + pos + 8, file.data() + at, 4 * floats);
    pos += 8 + 4 * floats, at += floats;
  }
  return 0;
}

} // extern "C"
