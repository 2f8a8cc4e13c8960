// oak_amd/csrc/forest_rows.hpp -- what the two game loops over the forest search share beyond game_rows.hpp (forestplay.hip: self-play;
// forestmatch.hip: two search agents against each other).  On the device: the integer payoffs of process_output's exact Nash solve, and
// the way from a turn-major log of encoded updates to one contiguous `.battle.data` stream (the log entry, the scan of the record lengths,
// the head and log pack).  On the host: the owner of a workspace's device arrays, the carving of one block of device memory into the forest
// search's output arrays, the turn's Nash solve (on the device, or by the host threads here), the doubling of a log, the record bases with
// their stream buffers, the pack launches, the copies behind a `_records` getter and the refusals of a seat's policy options.  Each loop
// keeps its own row, retire rule, pick kernel, synchronisation points and error prefixes.  The kernels are `static` so that each
// translation unit that includes the header holds its own, and so are the host functions that launch them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../include/oakgpu.h"
#include "game_rows.hpp"
#include "oakgpu_internal.h"
#include "nash.hpp"
#include "selfplay_pick.hpp"

namespace oak {
namespace fsp {

using game_rows::BLOCK;
using game_rows::DEAD;
using game_rows::k_rows_offsets;
using game_rows::NO_ROW;
using game_rows::u32x4;
using oak_nash::PAY_STRIDE;

// the device arrays of one workspace, freed together: a workspace is grow-only, a larger batch frees every array and allocates them again
struct DeviceArrays {
  std::vector<void *> held;
  template <class T> int get(T *&p, size_t count) {
    if (int rc = dev_alloc(p, count)) return rc;
    held.push_back(p);
    return 0;
  }
  void free_all() {
    for (void *p : held) (void)hipFree(p);
    held.clear();
  }
};

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

// The turn's Nash solve of `rows` root outputs into nash (rows x 9 of p1, rows x 9 of p2, rows values): the payoff kernel, then
// oakgpu_nash_solve_dev on the stream (solve_nash 2: nothing leaves the device) or download, solve_rows, upload (1).  h_pay / h_nash are
// the caller's, kept between turns; the upload reads h_nash until the stream is synchronised, which each loop does where it suits it.
static inline int solve_turn(oakgpu_ctx *ctx, hipStream_t stream, int solve_nash, const oakgpu_forest_outputs &o, uint32_t rows, int32_t *pay, double *nash,
                             std::vector<int32_t> &h_pay, std::vector<double> &h_nash) {
  const PayoffArgs pa{o.m, o.n, o.visit_matrix, o.value_matrix, pay, rows};
  hipLaunchKernelGGL(k_fsp_payoffs, dim3((rows + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, pa);
  HIPCHK(hipGetLastError());
  if (solve_nash == 2) return oakgpu_nash_solve_dev(ctx, pay, rows, nash);
  h_pay.resize((size_t)rows * PAY_STRIDE);
  h_nash.resize((size_t)rows * 19);
  HIPCHK(hipMemcpyAsync(h_pay.data(), pay, h_pay.size() * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  solve_rows(h_pay.data(), rows, h_nash.data());
  HIPCHK(hipMemcpyAsync(nash, h_nash.data(), h_nash.size() * 8, hipMemcpyHostToDevice, stream));
  return 0;
}

// Why a seat's policy options are refused, without the caller's prefix; empty when they pass.
inline std::string policy_refusal(const char *policy_mode, size_t size, double policy_min, int solve_nash) {
  oak_pick::PolicyMode mode;
  const int bad = oak_pick::parse_policy_mode(policy_mode, size, &mode);
  if (bad == 'b') return "policy mode 'b' (beta) is not supported (util/policy.h:59-60 throws)";
  if (bad > 0) return std::string("unknown policy mode letter '") + (char)bad + "' (words are e / n / x / p with optional weights, util/policy.h:22-98)";
  if (bad < 0) return "more than 8 policy mode words";
  if (!(policy_min <= 1.0)) return "RuntimePolicy: zero policy (policy_min above 1 zeroes every policy)";
  if (!solve_nash)
    for (uint32_t q = 0; q < mode.count; ++q)
      if (mode.word[q].kind == oak_pick::W_NASH) return "policy mode word 'n' needs solve_nash (the nash strategies are not computed)";
  return std::string();
}

// ---- records: a game's CompressedFrames record is packed from the log at the end of the call.  `status` is 0 (OAKGPU_FSP_OK) for a game
// whose record is kept; forestmatch.hip hands in a byte of its own making that is 0 for the games it keeps.
constexpr uint32_t HEAD_BYTES = 4 + 2 + 384 + 1; // a record in front of its updates

// one entry of the turn-major log: which game, where in its record, how long, the encoded update
struct LogEntry { uint32_t game, cursor, length; uint8_t bytes[84]; };
static_assert(sizeof(LogEntry) == 96 && oak_pick::MAX_UPDATE_BYTES <= 84, "one log entry is 96 bytes");

// one workgroup: game_rows.hpp's scan in 64 bits over the record lengths in game order: offsets[g] = where game g's record starts,
// offsets[n] = the stream's size
static __global__ __launch_bounds__(1024) void k_fsp_lengths(const uint32_t *length, uint32_t n, unsigned long long *offsets) {
  __shared__ unsigned long long wave_total[16];
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const game_rows::ScanPass<unsigned long long> s = game_rows::scan_pass<unsigned long long>(i < n ? length[i] : 0, wave_total);
    if (i < n) offsets[i] = carry + s.before;
    carry += s.total;
  }
  if (threadIdx.x == 0) offsets[n] = carry;
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

inline size_t first_log_capacity(uint32_t n) { return std::max<size_t>((size_t)n * 16, 4096); } // entries of a log before it has grown

// a log follows the turns played, doubled between turns: room for `want` entries, the first `entries` carried over
inline int grow_log(LogEntry *&log, size_t entries, size_t want, hipStream_t stream) {
  LogEntry *bigger = nullptr;
  if (int rc = dev_alloc(bigger, want)) return rc;
  HIPCHK(hipMemcpyAsync(bigger, log, entries * sizeof(LogEntry), hipMemcpyDeviceToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
  (void)hipFree(log);
  log = bigger;
  return 0;
}

// The record bases of n games in game order (k_fsp_lengths), the host's 8-byte read of their total = *bytes, and `count` stream buffers of
// one capacity that hold it: grow-only, freed and allocated again.
static inline int record_bases(hipStream_t stream, const uint32_t *length, uint32_t n, unsigned long long *offsets, uint8_t **streams, int count, size_t *capacity,
                               size_t *bytes) {
  hipLaunchKernelGGL(k_fsp_lengths, dim3(1), dim3(1024), 0, stream, length, n, offsets);
  HIPCHK(hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, offsets + n, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (total > *capacity) {
    for (int s = 0; s < count; ++s) {
      if (streams[s]) (void)hipFree(streams[s]);
      streams[s] = nullptr;
    }
    *capacity = 0;
    for (int s = 0; s < count; ++s)
      if (int rc = dev_alloc(streams[s], (size_t)total)) return rc;
    *capacity = (size_t)total;
  }
  *bytes = (size_t)total;
  return 0;
}

// one stream's records: the heads, then the log's updates
static inline int pack_records(hipStream_t stream, const PackArgs &pa) {
  hipLaunchKernelGGL(k_fsp_pack_head, dim3((pa.n + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, stream, pa);
  if (pa.entries) hipLaunchKernelGGL(k_fsp_pack_log, dim3((uint32_t)(((size_t)pa.entries + BLOCK / 16 - 1) / (BLOCK / 16))), dim3(BLOCK), 0, stream, pa);
  HIPCHK(hipGetLastError());
  return 0;
}

// What a finished call holds for its `_records` getter, and the getter's copies (to host or device arrays, each nullable) with the
// synchronisation after them.  The getter has checked the capacity of stream_out.
struct Records {
  const uint8_t *stream;
  size_t bytes;
  const unsigned long long *offsets; // n + 1
  const uint32_t *frames;
  const uint8_t *results, *status;
  size_t n;
};

inline int copy_records(hipStream_t stream, const Records &r, uint8_t *stream_out, uint64_t *offsets, uint32_t *n_frames, uint8_t *results, uint8_t *status,
                        int to_device) {
  const hipMemcpyKind kind = to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (stream_out && r.bytes) HIPCHK(hipMemcpyAsync(stream_out, r.stream, r.bytes, kind, stream));
  if (offsets) {
    if (r.n) HIPCHK(hipMemcpyAsync(offsets, r.offsets, (r.n + 1) * 8, kind, stream));
    else if (to_device) HIPCHK(hipMemsetAsync(offsets, 0, 8, stream));
    else offsets[0] = 0;
  }
  if (n_frames && r.n) HIPCHK(hipMemcpyAsync(n_frames, r.frames, r.n * 4, kind, stream));
  if (results && r.n) HIPCHK(hipMemcpyAsync(results, r.results, r.n, kind, stream));
  if (status && r.n) HIPCHK(hipMemcpyAsync(status, r.status, r.n, kind, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

} // namespace fsp
} // namespace oak
