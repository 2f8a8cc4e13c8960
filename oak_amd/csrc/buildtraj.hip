// oak_amd/csrc/buildtraj.hip -- `.build.data` records into training tensors on the device: the reference's read_build_trajectories
// (cpp/src/pyoak.cc:247-329) with Py::Build::Trajectories::write (cpp/include/py/build/trajectories.h:145-233), and the network-free half of
// build.py's process_targets (src/oak/build.py:119-129, 157-195).  The rule is build_traj.hpp's; the contract is in include/oakgpu.h.
//
//   k_traj_scan     one lane per record: its status (build_traj.hpp's walk with one thread), counted per status with integer atomics
//   k_traj_draw     one lane per draw: the reference's two-stage rule (a file, then a record of it) with a fast_prng stream per draw
//   k_build_traj    one wave per trajectory (a workgroup of one wave, so its barriers are the wave's own).  The record, the helper and one
//                   row of the list live in LDS (1 KiB).  The 31 steps are sequential: lane 0 applies each action; every lane writes its
//                   entries of a step's list to their places (a count of the flags in front of each, no entry waits for another), lane 0
//                   exchanges the taken action with entry 0, then the row leaves LDS for the mask with 16 bytes per lane wherever the address
//                   allows it (a trajectory's block is only 8-byte aligned for odd rows: the head and the tail of a range go out one
//                   entry per lane).  The rows before start and from end on are two fills of -1.  The mask is the whole cost: 84,072 bytes
//                   per trajectory as int64.
//   k_targets_mark  one lane per (row, step): valid, the reward, the live count per block -- game_rows.hpp's one scan path
//   k_targets_rows  the stable compaction of the valid steps: (b, t), the state's cells in step order, the logarithm of the old policy
//   k_state_dense   one workgroup per valid row: the 0/1 state of 3,749 floats from a bit mask in LDS
// No float atomics; a row's bits depend on its record alone, and two calls give the same bits.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "oakgpu_internal.h"
#include "build_corpus.hpp"
#include "build_traj.hpp"
#include "fast_prng.hpp"
#include "game_rows.hpp"

namespace bt = oak_build_traj;

namespace {
#define RC(x) do { int _r = (x); if (_r) return _r; } while (0)

constexpr uint32_t STEPS = bt::STEPS, MAX_ACTIONS = bt::MAX_ACTIONS, N_DIM = bt::N_DIM, RECORD_BYTES = bt::RECORD_BYTES, WAVE = 64;
constexpr uint32_t MASK_ENTRIES = STEPS * MAX_ACTIONS; // of one trajectory
constexpr uint8_t BAD_PICK = OAKGPU_BUILD_TRAJ_BAD_PICK;
static_assert(STEPS == OAKGPU_BUILD_MAX_STEPS && MAX_ACTIONS == OAKGPU_BUILD_MAX_ACTIONS && N_DIM == OAKGPU_BUILD_N_DIM, "include/oakgpu.h and build_tables.inc disagree");
static_assert(bt::OK == OAKGPU_BUILD_TRAJ_OK && bt::BAD_ACTION == OAKGPU_BUILD_TRAJ_BAD_ACTION && bt::NO_SPECIES == OAKGPU_BUILD_TRAJ_NO_SPECIES &&
                  bt::TEAM_FULL == OAKGPU_BUILD_TRAJ_TEAM_FULL && bt::NOT_LEGAL == OAKGPU_BUILD_TRAJ_NOT_LEGAL &&
                  bt::LIST_OVERFLOW == OAKGPU_BUILD_TRAJ_LIST_OVERFLOW && bt::N_STATUS == OAKGPU_BUILD_TRAJ_N_STATUS,
              "include/oakgpu.h and build_traj.hpp disagree");

int fail(const char *fn, const std::string &what) { return oakgpu_fail_msg((std::string(fn) + ": " + what).c_str()); }

// ---- the scan and the draw ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_traj_scan(const uint8_t *records, uint32_t n, uint8_t *status, uint32_t *counts) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  uint32_t words[RECORD_BYTES / 4];
  const uint32_t *src = (const uint32_t *)records + (size_t)r * (RECORD_BYTES / 4);
#pragma unroll
  for (uint32_t k = 0; k < RECORD_BYTES / 4; ++k) words[k] = src[k];
  const uint8_t s = bt::record_status((const uint8_t *)words);
  status[r] = s;
  atomicAdd(&counts[s], 1u);
}

// draw i: fast_prng seeded with seed + i; file = uniform_64 % n_files; record = uniform_64 % records(file)
__global__ __launch_bounds__(256) void k_traj_draw(const uint32_t *file_first, uint32_t n_files, uint64_t seed, uint32_t n, uint32_t *picks) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  oak::FastPrng g;
  g.seed(seed + i);
  const uint32_t h0 = g.next32(), l0 = g.next32(), h1 = g.next32(), l1 = g.next32(); // uniform_64 = hi << 32 | lo
  const uint32_t file = (uint32_t)((((uint64_t)h0 << 32) | l0) % n_files);
  const uint32_t first = file_first[file], count = file_first[file + 1] - first; // (no file is empty)
  picks[i] = first + (uint32_t)((((uint64_t)h1 << 32) | l1) % count);
}

// ---- the decode --------------------------------------------------------------------------------------------------------------------------
struct TrajArgs {
  const uint8_t *records;
  uint32_t n_records;
  const uint32_t *picks; // nullable: row b reads record b
  int no_score;
  int64_t *action;
  void *mask;
  uint16_t *n_legal;
  float *policy, *value, *score;
  int64_t *start, *end;
  uint8_t *status;
  uint32_t *t_max;
};

template <class T> struct Vec16;
template <> struct Vec16<int64_t> {
  typedef long long type __attribute__((ext_vector_type(2)));
  static constexpr uint32_t E = 2;
};
template <> struct Vec16<int16_t> {
  typedef short type __attribute__((ext_vector_type(8)));
  static constexpr uint32_t E = 8;
};

// Entries [g0, g1) of a trajectory's mask block, by the whole wave: entry g0 + k is row[k] for k < length and -1 from there on (row null:
// all -1).  16 bytes per lane from the first 16-byte boundary in the range to the last; the entries in front and behind go out one per lane.
template <class T> __device__ __forceinline__ void store_range(T *block, uint32_t g0, uint32_t g1, const int16_t *row, uint32_t length, uint32_t lane) {
  typedef typename Vec16<T>::type V;
  constexpr uint32_t E = Vec16<T>::E;
  if (g0 >= g1) return;
  T *p = block + g0;
  const uint32_t total = g1 - g0;
  const uint32_t past = (uint32_t)(((uintptr_t)p & 15) / sizeof(T)); // entries past a 16-byte boundary (the block is aligned to its entries)
  uint32_t head = past ? E - past : 0;
  if (head > total) head = total;
  const uint32_t vectors = (total - head) / E, tail_at = head + vectors * E, tail = total - tail_at;
  auto value = [&](uint32_t k) -> T { return (row && k < length) ? (T)row[k] : (T)-1; };
  if (lane < head) p[lane] = value(lane);
  for (uint32_t v = lane; v < vectors; v += WAVE) {
    const uint32_t k = head + v * E;
    V out;
#pragma unroll
    for (uint32_t e = 0; e < E; ++e) out[e] = value(k + e);
    *(V *)(p + k) = out;
  }
  if (lane < tail) p[tail_at + lane] = value(tail_at + lane);
}

template <class T> struct WaveVisitor {
  uint32_t lane;
  int16_t *lds;   // one row of the list
  T *mask;        // this trajectory's block; nullable
  uint32_t my_n;  // lane i: the length of step i's list
  __device__ bool leader() const { return lane == 0; }
  __device__ void sync() const { __syncthreads(); }
  __device__ void row(int32_t i, const bt::Bounds &b, const bt::Helper &h, uint32_t length, uint32_t place, uint32_t action) {
    if (lane == (uint32_t)i) my_n = length;
    if (!mask) return;
    bt::list_write(h, i, b, lane, WAVE, lds);
    __syncthreads();
    if (lane == 0) { // the taken action is exchanged with entry 0
      lds[place] = lds[0];
      lds[0] = (int16_t)action;
    }
    __syncthreads();
    store_range(mask, (uint32_t)i * MAX_ACTIONS, (uint32_t)(i + 1) * MAX_ACTIONS, lds, length, lane);
    __syncthreads(); // (the next step writes the row again)
  }
};

template <class T> __global__ __launch_bounds__(64) void k_build_traj(TrajArgs a) {
  __shared__ uint32_t s_rec[RECORD_BYTES / 4];
  __shared__ bt::Helper s_helper;
  __shared__ int16_t s_row[MAX_ACTIONS + 1];
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  const uint32_t pick = a.picks ? a.picks[b] : b;
  const bool in = pick < a.n_records; // (a pick outside the corpus reads nothing)
  if (lane < RECORD_BYTES / 4) s_rec[lane] = in ? ((const uint32_t *)a.records)[(size_t)pick * (RECORD_BYTES / 4) + lane] : 0u;
  __syncthreads();
  const uint8_t *r = (const uint8_t *)s_rec;
  const bt::Bounds bd = bt::bounds_of(r);
  T *mask = a.mask ? (T *)a.mask + (size_t)b * MASK_ENTRIES : nullptr;
  if (mask) { // the rows before start and from end on
    store_range<T>(mask, 0, (uint32_t)bd.start * MAX_ACTIONS, nullptr, 0, lane);
    store_range<T>(mask, (uint32_t)bd.end * MAX_ACTIONS, MASK_ENTRIES, nullptr, 0, lane);
  }
  WaveVisitor<T> v{lane, s_row, mask, 0};
  const uint8_t status = in ? bt::walk(r, bd, s_helper, v) : BAD_PICK;
  const bool ok = status == bt::OK;
  if (!ok && mask) { // a record that is not OK is an ended trajectory: the rows written so far go back to -1, after them
    __threadfence();
    store_range<T>(mask, (uint32_t)bd.start * MAX_ACTIONS, (uint32_t)bd.end * MAX_ACTIONS, nullptr, 0, lane);
  }
  if (lane < STEPS) {
    const bool read = ok && (int32_t)lane >= bd.start && (int32_t)lane < bd.end;
    const size_t at = (size_t)b * STEPS + lane;
    if (a.action) a.action[at] = read ? (int64_t)bt::rec_action(r, lane) : (int64_t)-1;
    if (a.policy) a.policy[at] = read ? bt::probability_of(bt::rec_probability(r, lane)) : 0.0f;
    if (a.n_legal) a.n_legal[at] = read ? (uint16_t)v.my_n : (uint16_t)0;
  }
  if (lane == 0) {
    if (a.value) a.value[b] = bt::rec_value(r);
    if (a.score) a.score[b] = bt::rec_score(r, a.no_score);
    if (a.start) a.start[b] = ok ? bd.start : 0;
    if (a.end) a.end[b] = ok ? bd.end : 0;
    a.status[b] = status;
    if (a.t_max && ok) atomicMax(a.t_max, (uint32_t)bd.end);
  }
}

// ---- the targets -------------------------------------------------------------------------------------------------------------------------
struct TargetArgs {
  const int64_t *action, *start, *end;
  const float *policy, *value, *score;
  uint32_t n;
  float value_weight, score_weight;
  uint8_t *valid;
  uint32_t *rows;
  uint16_t *state_cells;
  uint8_t *state_n;
  float *old_logp, *rewards;
  uint32_t *block_live, *block_offset;
};

__device__ __forceinline__ bool step_valid(const TargetArgs &a, uint32_t item, uint32_t total) {
  return item < total && a.action[item] != -1 && a.policy[item] > 0.0f;
}

__global__ __launch_bounds__(256) void k_targets_mark(TargetArgs a) {
  __shared__ uint32_t wave_live[oak::game_rows::BLOCK / 64];
  const uint32_t total = a.n * STEPS, item = blockIdx.x * oak::game_rows::BLOCK + threadIdx.x;
  const bool valid = step_valid(a, item, total);
  if (item < total) {
    const uint32_t b = item / STEPS, t = item - b * STEPS;
    if (a.valid) a.valid[item] = valid ? 1 : 0;
    if (a.rewards) { // value_weight * value + score_weight * score at end - 1, each product and the sum rounded to float (no fma)
      const int64_t end = a.end[b];
      a.rewards[item] = (end > 0 && (int64_t)t == end - 1) ? __fadd_rn(__fmul_rn(a.value_weight, a.value[b]), __fmul_rn(a.score_weight, a.score[b])) : 0.0f;
    }
  }
  oak::game_rows::count_block_live(valid, wave_live, a.block_live);
}

__global__ __launch_bounds__(256) void k_targets_rows(TargetArgs a) {
  __shared__ uint32_t wave_total[oak::game_rows::BLOCK / 64], place[oak::game_rows::BLOCK];
  const uint32_t total = a.n * STEPS, item = blockIdx.x * oak::game_rows::BLOCK + threadIdx.x;
  const bool valid = step_valid(a, item, total);
  const uint32_t to = oak::game_rows::compact_place(valid, a.block_offset[blockIdx.x], wave_total, place);
  if (!valid) return;
  const uint32_t b = item / STEPS, t = item - b * STEPS;
  if (a.rows) { a.rows[2 * (size_t)to] = b; a.rows[2 * (size_t)to + 1] = t; }
  // the logarithm in double, rounded to float once: the device library's double log is within 3 ulp of double (OpenCL's bound), so the float is
  // within 0.5 + 3 x 2^-29 of its own ulp of the exact logarithm -- a bound that float logf (3 ulp by the same table) does not give
  if (a.old_logp) a.old_logp[to] = (float)log((double)a.policy[item]);
  uint32_t count = 0; // get_state: the actions of the steps in front of t, pre-start steps (-1) dropped
  for (uint32_t s = 0; s < t; ++s) {
    const int64_t c = a.action[(size_t)b * STEPS + s];
    if (c < 0) continue;
    if (a.state_cells) a.state_cells[(size_t)to * STEPS + count] = (uint16_t)c;
    ++count;
  }
  if (a.state_cells)
    for (uint32_t k = count; k < STEPS; ++k) a.state_cells[(size_t)to * STEPS + k] = 0xFFFFu;
  if (a.state_n) a.state_n[to] = (uint8_t)count;
}

constexpr uint32_t STATE_WORDS = (N_DIM + 31) / 32;
__global__ __launch_bounds__(256) void k_state_dense(const uint16_t *state_cells, const uint8_t *state_n, uint32_t lo, float *out) {
  __shared__ uint32_t bits[STATE_WORDS];
  const uint32_t row = lo + blockIdx.x, tid = threadIdx.x;
  if (tid < STATE_WORDS) bits[tid] = 0;
  __syncthreads();
  if (tid < STEPS && tid < state_n[row]) {
    const uint32_t c = state_cells[(size_t)row * STEPS + tid];
    if (c < N_DIM) atomicOr(&bits[c >> 5], 1u << (c & 31));
  }
  __syncthreads();
  float *dst = out + (size_t)blockIdx.x * N_DIM;
  for (uint32_t c = tid; c < N_DIM; c += 256) dst[c] = ((bits[c >> 5] >> (c & 31)) & 1) ? 1.0f : 0.0f;
}

int check_params(const char *fn, const oakgpu_build_traj_params *prm) {
  if (!prm) return fail(fn, "null params");
  if (prm->mask_dtype != OAKGPU_BUILD_MASK_INT64 && prm->mask_dtype != OAKGPU_BUILD_MASK_INT16) return fail(fn, "mask_dtype outside {int64, int16}");
  if (prm->no_score != 0 && prm->no_score != 1) return fail(fn, "no_score outside {0, 1}");
  return 0;
}

int launch_traj(oakgpu_ctx *ctx, const oakgpu_build_corpus *corpus, const uint32_t *picks, uint32_t n, const oakgpu_build_traj_params *prm,
                const oakgpu_build_trajectories *out) {
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  const TrajArgs a{corpus->records, corpus->n_records, picks, prm->no_score, out->action, out->mask, out->n_legal, out->policy, out->value, out->score,
                   out->start, out->end, out->status, out->t_max};
  if (out->t_max) HIPCHK(hipMemsetAsync(out->t_max, 0, 4, stream));
  if (prm->mask_dtype == OAKGPU_BUILD_MASK_INT16) hipLaunchKernelGGL(k_build_traj<int16_t>, dim3(n), dim3(WAVE), 0, stream, a);
  else hipLaunchKernelGGL(k_build_traj<int64_t>, dim3(n), dim3(WAVE), 0, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int check_traj_call(const char *fn, oakgpu_ctx *ctx, const oakgpu_build_corpus *corpus, uint32_t n, const oakgpu_build_traj_params *prm,
                    const oakgpu_build_trajectories *out) {
  if (!ctx || !corpus || !out) return fail(fn, "null argument");
  if (n == 0) return fail(fn, "n == 0");
  RC(check_params(fn, prm));
  if (!out->status) return fail(fn, "status is null");
  if (corpus->ctx != ctx) return fail(fn, "the corpus belongs to another context");
  if (corpus->n_records == 0) return fail(fn, "the corpus holds no record (an empty window)");
  if ((uintptr_t)out->mask & (prm->mask_dtype == OAKGPU_BUILD_MASK_INT16 ? 1 : 7)) return fail(fn, "mask is not aligned to its entries");
  return 0;
}

int scan(oakgpu_ctx *ctx, oakgpu_build_corpus *corpus) {
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  HIPCHK(hipMemsetAsync(corpus->counts, 0, sizeof(uint32_t) * bt::N_STATUS, stream));
  if (corpus->n_records == 0) return 0; // (an empty window)
  hipLaunchKernelGGL(k_traj_scan, dim3((corpus->n_records + 255) / 256), dim3(256), 0, stream, corpus->records, corpus->n_records, corpus->status, corpus->counts);
  HIPCHK(hipGetLastError());
  return 0;
}

// the files of a buffer: what oakgpu_build_corpus_create refuses, by name; first[f] = the first record of file f
int check_files(const char *fn, const uint8_t *buffer, size_t size, const size_t *file_sizes, uint32_t n_files, std::vector<uint32_t> &first) {
  if (!buffer || !file_sizes || n_files == 0 || size == 0) return fail(fn, "an empty corpus");
  size_t at = 0;
  first.assign(1, 0u);
  for (uint32_t f = 0; f < n_files; ++f) {
    const size_t bytes = file_sizes[f];
    if (bytes == 0) return fail(fn, "file " + std::to_string(f) + ": an empty file");
    if (bytes % RECORD_BYTES) return fail(fn, "file " + std::to_string(f) + ": " + std::to_string(bytes) + " bytes is not a multiple of 128");
    if (bytes > size - at) return fail(fn, "file " + std::to_string(f) + ": the file sizes add up to more than the buffer");
    for (size_t r = 0; r < bytes / RECORD_BYTES; ++r)
      if (buffer[at + r * RECORD_BYTES] != 0)
        return fail(fn, "file " + std::to_string(f) + ", record " + std::to_string(r) + ": format byte " + std::to_string(buffer[at + r * RECORD_BYTES]) +
                            " (only NoTeam records, format 0, are read)");
    at += bytes;
    if (at / RECORD_BYTES > 0xFFFFFFFEull) return fail(fn, "more than 2^32 - 2 records");
    first.push_back((uint32_t)(at / RECORD_BYTES));
  }
  if (at != size) return fail(fn, "the file sizes add up to less than the buffer");
  return 0;
}
} // namespace

extern "C" {

int oakgpu_build_traj_check(const uint8_t *bytes, size_t len, uint8_t *status_out) {
  const char *fn = "oakgpu_build_traj_check";
  if (!bytes || len == 0) return fail(fn, "no records");
  if (!status_out) return fail(fn, "null status_out");
  if (len % RECORD_BYTES) return fail(fn, std::to_string(len) + " bytes is not a multiple of 128");
  for (size_t r = 0; r < len / RECORD_BYTES; ++r) {
    if (bytes[r * RECORD_BYTES] != 0)
      return fail(fn, "record " + std::to_string(r) + ": format byte " + std::to_string(bytes[r * RECORD_BYTES]) + " (only NoTeam records, format 0, are read)");
    status_out[r] = bt::record_status(bytes + r * RECORD_BYTES);
  }
  return 0;
}

int oakgpu_build_corpus_create(oakgpu_ctx *ctx, const uint8_t *buffer, size_t size, const size_t *file_sizes, uint32_t n_files, oakgpu_build_corpus **out) {
  const char *fn = "oakgpu_build_corpus_create";
  std::vector<uint32_t> first;
  RC(check_files(fn, buffer, size, file_sizes, n_files, first));
  if (!ctx || !out) return fail(fn, "null argument");
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  oakgpu_build_corpus *c = new oakgpu_build_corpus;
  c->ctx = ctx;
  c->n_records = first.back();
  c->n_files = n_files;
  int rc = dev_alloc(c->records, size);
  if (!rc) rc = dev_alloc(c->file_first, first.size());
  if (!rc) rc = dev_alloc(c->status, (size_t)c->n_records);
  if (!rc) rc = dev_alloc(c->counts, (size_t)bt::N_STATUS);
  if (!rc && hipMemcpyAsync(c->records, buffer, size, hipMemcpyHostToDevice, stream) != hipSuccess) rc = fail(fn, "the copy of the records failed");
  if (!rc && hipMemcpyAsync(c->file_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, stream) != hipSuccess) rc = fail(fn, "the copy of the file table failed");
  if (hipStreamSynchronize(stream) != hipSuccess && !rc) rc = fail(fn, "the copy of the records failed"); // (`first` and the caller's buffer are pageable)
  if (rc) {
    oakgpu_build_corpus_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void oakgpu_build_corpus_destroy(oakgpu_build_corpus *corpus) {
  if (!corpus) return;
  if (corpus->ctx && oakgpu_ctx_enter(corpus->ctx) == 0) (void)hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(corpus->ctx));
  (void)hipFree(corpus->records);
  (void)hipFree(corpus->file_first);
  (void)hipFree(corpus->status);
  (void)hipFree(corpus->counts);
  (void)hipFree(corpus->picks);
  delete corpus;
}

int oakgpu_build_corpus_scan_dev(oakgpu_ctx *ctx, oakgpu_build_corpus *corpus) {
  const char *fn = "oakgpu_build_corpus_scan_dev";
  if (!ctx || !corpus) return fail(fn, "null argument");
  if (corpus->ctx != ctx) return fail(fn, "the corpus belongs to another context");
  RC(oakgpu_ctx_enter(ctx));
  RC(scan(ctx, corpus));
  corpus->scan_launched = true;
  corpus->scanned = false;
  return 0;
}

int oakgpu_build_corpus_info(oakgpu_build_corpus *corpus, oakgpu_build_corpus_stats *info) {
  const char *fn = "oakgpu_build_corpus_info";
  if (!corpus || !info) return fail(fn, "null argument");
  if (!corpus->scanned) {
    RC(oakgpu_ctx_enter(corpus->ctx));
    hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(corpus->ctx);
    if (!corpus->scan_launched) RC(scan(corpus->ctx, corpus));
    corpus->scan_launched = true;
    HIPCHK(hipMemcpyAsync(corpus->h_counts, corpus->counts, sizeof(corpus->h_counts), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    corpus->scanned = true;
  }
  info->records = corpus->n_records;
  info->files = corpus->n_files;
  for (uint32_t s = 0; s < bt::N_STATUS; ++s) info->status_count[s] = corpus->h_counts[s];
  return 0;
}

int oakgpu_build_traj_dev(oakgpu_ctx *ctx, const oakgpu_build_corpus *corpus, const uint32_t *picks, uint32_t n, const oakgpu_build_traj_params *prm,
                          const oakgpu_build_trajectories *out) {
  const char *fn = "oakgpu_build_traj_dev";
  RC(check_traj_call(fn, ctx, corpus, n, prm, out));
  if (!picks) return fail(fn, "null picks");
  RC(oakgpu_ctx_enter(ctx));
  return launch_traj(ctx, corpus, picks, n, prm, out);
}

int oakgpu_build_traj_sample_dev(oakgpu_ctx *ctx, oakgpu_build_corpus *corpus, uint32_t n, uint64_t seed, const oakgpu_build_traj_params *prm, uint32_t *picks_out,
                                 const oakgpu_build_trajectories *out) {
  const char *fn = "oakgpu_build_traj_sample_dev";
  RC(check_traj_call(fn, ctx, corpus, n, prm, out));
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  uint32_t *picks = picks_out;
  if (!picks) {
    if (corpus->capacity < n) { // (a launch on the stream may still read the old picks)
      HIPCHK(hipStreamSynchronize(stream));
      (void)hipFree(corpus->picks);
      corpus->picks = nullptr;
      corpus->capacity = 0;
      RC(dev_alloc(corpus->picks, (size_t)n));
      corpus->capacity = n;
    }
    picks = corpus->picks;
  }
  hipLaunchKernelGGL(k_traj_draw, dim3((n + 255) / 256), dim3(256), 0, stream, corpus->file_first, corpus->n_files, seed, n, picks);
  HIPCHK(hipGetLastError());
  return launch_traj(ctx, corpus, picks, n, prm, out);
}

int oakgpu_build_targets_dev(oakgpu_ctx *ctx, const oakgpu_build_trajectories *traj, uint32_t n, double value_weight, const oakgpu_build_target_outputs *out) {
  const char *fn = "oakgpu_build_targets_dev";
  if (!ctx || !traj || !out) return fail(fn, "null argument");
  if (n == 0) return fail(fn, "n == 0");
  if (n > 0xFFFFFFFFu / STEPS) return fail(fn, "n x 31 steps do not fit 32 bits");
  if (!traj->action || !traj->policy) return fail(fn, "action and policy are required");
  if (out->rewards && (!traj->value || !traj->score || !traj->end)) return fail(fn, "rewards need value, score and end");
  if (!out->n_valid) return fail(fn, "n_valid is null");
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  const uint32_t blocks = (n * STEPS + oak::game_rows::BLOCK - 1) / oak::game_rows::BLOCK;
  uint32_t *ws = (uint32_t *)oakgpu_ctx_workspace(ctx, 1, (size_t)blocks * 8);
  if (!ws) return -1;
  const double score_weight = 1.0 - value_weight; // build.py's order: the difference in double, then each weight to float at its product
  const TargetArgs a{traj->action, traj->start, traj->end, traj->policy, traj->value, traj->score, n, (float)value_weight, (float)score_weight,
                     out->valid, out->rows, out->state_cells, out->state_n, out->old_logp, out->rewards, ws, ws + blocks};
  hipLaunchKernelGGL(k_targets_mark, dim3(blocks), dim3(oak::game_rows::BLOCK), 0, stream, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(oak::game_rows::k_rows_offsets, dim3(1), dim3(1024), 0, stream, ws, blocks, ws + blocks, out->n_valid);
  HIPCHK(hipGetLastError());
  if (out->rows || out->state_cells || out->state_n || out->old_logp) {
    hipLaunchKernelGGL(k_targets_rows, dim3(blocks), dim3(oak::game_rows::BLOCK), 0, stream, a);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

int oakgpu_build_state_dense_dev(oakgpu_ctx *ctx, const uint16_t *state_cells, const uint8_t *state_n, uint32_t lo, uint32_t hi, float *out) {
  const char *fn = "oakgpu_build_state_dense_dev";
  if (!ctx || !state_cells || !state_n || !out) return fail(fn, "null argument");
  if (hi <= lo) return fail(fn, "an empty range of rows");
  RC(oakgpu_ctx_enter(ctx));
  hipLaunchKernelGGL(k_state_dense, dim3(hi - lo), dim3(256), 0, (hipStream_t)oakgpu_ctx_stream(ctx), state_cells, state_n, lo, out);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- host-pointer forms: staged in, staged out, complete on return -----------------------------------------------------------------------
namespace {
struct StagedTraj {
  oakgpu_build_trajectories dev{};
  size_t mask_bytes = 0;
};
int stage_traj(OakHostCall &call, uint32_t n, const oakgpu_build_traj_params *prm, const oakgpu_build_trajectories *host, StagedTraj &s) {
  const size_t steps = (size_t)n * STEPS;
  s.mask_bytes = steps * MAX_ACTIONS * (prm->mask_dtype == OAKGPU_BUILD_MASK_INT16 ? 2 : 8);
  auto get = [&](const void *wanted, size_t bytes, void **p) { *p = wanted ? call.get(bytes) : nullptr; return wanted && !*p ? -1 : 0; };
  RC(get(host->action, steps * 8, (void **)&s.dev.action));
  RC(get(host->mask, s.mask_bytes, &s.dev.mask));
  RC(get(host->n_legal, steps * 2, (void **)&s.dev.n_legal));
  RC(get(host->policy, steps * 4, (void **)&s.dev.policy));
  RC(get(host->value, (size_t)n * 4, (void **)&s.dev.value));
  RC(get(host->score, (size_t)n * 4, (void **)&s.dev.score));
  RC(get(host->start, (size_t)n * 8, (void **)&s.dev.start));
  RC(get(host->end, (size_t)n * 8, (void **)&s.dev.end));
  RC(get(host->status, n, (void **)&s.dev.status));
  RC(get(host->t_max, 4, (void **)&s.dev.t_max));
  return 0;
}
int fetch_traj(hipStream_t stream, uint32_t n, const StagedTraj &s, const oakgpu_build_trajectories *host) {
  const size_t steps = (size_t)n * STEPS;
  auto back = [&](void *h, const void *d, size_t bytes) -> hipError_t { return h ? hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream) : hipSuccess; };
  HIPCHK(back(host->action, s.dev.action, steps * 8));
  HIPCHK(back(host->mask, s.dev.mask, s.mask_bytes));
  HIPCHK(back(host->n_legal, s.dev.n_legal, steps * 2));
  HIPCHK(back(host->policy, s.dev.policy, steps * 4));
  HIPCHK(back(host->value, s.dev.value, (size_t)n * 4));
  HIPCHK(back(host->score, s.dev.score, (size_t)n * 4));
  HIPCHK(back(host->start, s.dev.start, (size_t)n * 8));
  HIPCHK(back(host->end, s.dev.end, (size_t)n * 8));
  HIPCHK(back(host->status, s.dev.status, n));
  HIPCHK(back(host->t_max, s.dev.t_max, 4));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}
} // namespace

int oakgpu_build_traj(oakgpu_ctx *ctx, const oakgpu_build_corpus *corpus, const uint32_t *picks, uint32_t n, const oakgpu_build_traj_params *prm,
                      const oakgpu_build_trajectories *out) {
  const char *fn = "oakgpu_build_traj";
  RC(check_traj_call(fn, ctx, corpus, n, prm, out));
  if (!picks) return fail(fn, "null picks");
  for (uint32_t i = 0; i < n; ++i)
    if (picks[i] >= corpus->n_records) return fail(fn, "pick " + std::to_string(i) + ": record " + std::to_string(picks[i]) + " of " + std::to_string(corpus->n_records));
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall call(ctx);
  StagedTraj s;
  RC(stage_traj(call, n, prm, out, s));
  uint32_t *d_picks = (uint32_t *)call.get((size_t)n * 4);
  if (!d_picks) return -1;
  HIPCHK(hipMemcpyAsync(d_picks, picks, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  RC(oakgpu_build_traj_dev(ctx, corpus, d_picks, n, prm, &s.dev));
  return fetch_traj(stream, n, s, out);
}

int oakgpu_build_traj_sample(oakgpu_ctx *ctx, oakgpu_build_corpus *corpus, uint32_t n, uint64_t seed, const oakgpu_build_traj_params *prm, uint32_t *picks_out,
                             const oakgpu_build_trajectories *out) {
  const char *fn = "oakgpu_build_traj_sample";
  RC(check_traj_call(fn, ctx, corpus, n, prm, out));
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall call(ctx);
  StagedTraj s;
  RC(stage_traj(call, n, prm, out, s));
  uint32_t *d_picks = (uint32_t *)call.get((size_t)n * 4);
  if (!d_picks) return -1;
  RC(oakgpu_build_traj_sample_dev(ctx, corpus, n, seed, prm, d_picks, &s.dev));
  if (picks_out) HIPCHK(hipMemcpyAsync(picks_out, d_picks, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  return fetch_traj(stream, n, s, out);
}

int oakgpu_build_targets(oakgpu_ctx *ctx, const oakgpu_build_trajectories *traj, uint32_t n, double value_weight, const oakgpu_build_target_outputs *out) {
  const char *fn = "oakgpu_build_targets";
  if (!ctx || !traj || !out) return fail(fn, "null argument");
  if (n == 0) return fail(fn, "n == 0");
  if (!traj->action || !traj->policy || !traj->value || !traj->score || !traj->end) return fail(fn, "action, policy, value, score and end are required");
  if (!out->n_valid) return fail(fn, "n_valid is null");
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall call(ctx);
  const size_t steps = (size_t)n * STEPS;
  oakgpu_build_trajectories t{};
  t.action = (int64_t *)call.get(steps * 8);
  t.policy = (float *)call.get(steps * 4);
  t.value = (float *)call.get((size_t)n * 4);
  t.score = (float *)call.get((size_t)n * 4);
  t.end = (int64_t *)call.get((size_t)n * 8);
  oakgpu_build_target_outputs d{};
  d.valid = (uint8_t *)call.get(steps);
  d.n_valid = (uint32_t *)call.get(4);
  d.rows = (uint32_t *)call.get(steps * 8);
  d.state_cells = (uint16_t *)call.get(steps * STEPS * 2);
  d.state_n = (uint8_t *)call.get(steps);
  d.old_logp = (float *)call.get(steps * 4);
  d.rewards = (float *)call.get(steps * 4);
  if (!t.action || !t.policy || !t.value || !t.score || !t.end || !d.valid || !d.n_valid || !d.rows || !d.state_cells || !d.state_n || !d.old_logp || !d.rewards) return -1;
  HIPCHK(hipMemcpyAsync(t.action, traj->action, steps * 8, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(t.policy, traj->policy, steps * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(t.value, traj->value, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(t.score, traj->score, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(t.end, traj->end, (size_t)n * 8, hipMemcpyHostToDevice, stream));
  RC(oakgpu_build_targets_dev(ctx, &t, n, value_weight, &d));
  HIPCHK(hipMemcpyAsync(out->n_valid, d.n_valid, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  const size_t v = *out->n_valid;
  auto back = [&](void *h, const void *dev, size_t bytes) -> hipError_t { return (h && bytes) ? hipMemcpyAsync(h, dev, bytes, hipMemcpyDeviceToHost, stream) : hipSuccess; };
  HIPCHK(back(out->valid, d.valid, steps));
  HIPCHK(back(out->rewards, d.rewards, steps * 4));
  HIPCHK(back(out->rows, d.rows, v * 8));
  HIPCHK(back(out->state_cells, d.state_cells, v * STEPS * 2));
  HIPCHK(back(out->state_n, d.state_n, v));
  HIPCHK(back(out->old_logp, d.old_logp, v * 4));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_build_state_dense(oakgpu_ctx *ctx, const uint16_t *state_cells, const uint8_t *state_n, uint32_t lo, uint32_t hi, float *out) {
  const char *fn = "oakgpu_build_state_dense";
  if (!ctx || !state_cells || !state_n || !out) return fail(fn, "null argument");
  if (hi <= lo) return fail(fn, "an empty range of rows");
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall call(ctx);
  const size_t k = hi - lo;
  uint16_t *d_cells = (uint16_t *)call.get(k * STEPS * 2);
  uint8_t *d_n = (uint8_t *)call.get(k);
  float *d_out = (float *)call.get(k * N_DIM * 4);
  if (!d_cells || !d_n || !d_out) return -1;
  HIPCHK(hipMemcpyAsync(d_cells, state_cells + (size_t)lo * STEPS, k * STEPS * 2, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_n, state_n + lo, k, hipMemcpyHostToDevice, stream));
  RC(oakgpu_build_state_dense_dev(ctx, d_cells, d_n, 0, (uint32_t)k, d_out));
  HIPCHK(hipMemcpyAsync(out, d_out, k * N_DIM * 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

} // extern "C"
