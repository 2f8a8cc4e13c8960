// oak_amd/csrc/corpuseval.hip -- a network evaluated on every frame of a resident `.battle.data` corpus (the contract is in
// include/oakgpu.h; the reference's per-record form is pyoak.cpp_inference, cpp/src/pyoak.cc:331-392).
//
//   k_chunk_order        : the records of a chunk -> lane order, longest first (one workgroup, counting sort by frame count)
//   k_frames_expand      : one lane per record, the replay check's walk on the register engine (record_walk.hpp) with EVERY frame
//                          written: the state in front of frame f goes to row base[r] - base[first] + f of the chunk.  The 384-byte battles are staged in
//                          LDS and the wave writes whole rows (24 lanes x 16 B each) instead of one lane writing 16-byte pieces
//                          384 bytes apart.
//   k_corpus_terms       : one lane per row: softmax policies, the squared value error and both sides' cross-entropy terms of
//                          battle.py's loss against the frame's stored targets
//   k_corpus_record_sums : one lane per record: float64 sums of its included rows' terms, in frame order
// The evaluation in between is oakgpu_leaf_eval_policy_dev over the chunk's rows.  There is no CPU fallback in this library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/oakgpu.h"
#include "gen1_device.hpp"
#include "gen1_regs.hpp"
#include "record_walk.hpp"
#include "oakgpu_internal.h"

namespace oak {
namespace ce {

using namespace walk;

constexpr uint32_t ROW_NONE = 0xFFFFFFFFu;

// ---- lane order of a chunk: frame count descending, longest game first (a malformed record has no frames)
__global__ __launch_bounds__(1024) void k_chunk_order(const uint16_t *frames, const uint8_t *malformed, uint32_t n, uint32_t *order) {
  order_desc(n, order, [&](uint32_t i) { return malformed[i] ? 0u : (uint32_t)frames[i]; });
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------
struct ExpandArgs {
  const uint8_t *records;   // the corpus: file bytes, unchanged
  const uint64_t *offsets;  // the corpus' records
  const uint16_t *frames;
  const uint8_t *malformed;
  const uint8_t *aligned;   // records x 384 (k_replay_gather)
  const uint8_t *first;     // records: the first request
  const uint64_t *bases;    // records + 1: prefix sums of the frame counts (0 for a malformed record)
  const uint32_t *order;    // n: lane -> record of the chunk (relative to first_record)
  uint8_t *battles;         // rows x 384
  uint8_t *durations;       // rows x 8
  uint8_t *results;         // rows
  uint8_t *ch1, *cnt1, *ch2, *cnt2; // rows x 9, rows
  uint8_t *status;          // rows
  uint32_t *where;          // rows
  uint32_t *rowrec;         // rows x 2: the frame's byte offset inside its record, the record
  uint32_t first_record, n;
};
constexpr int EXPAND_COLD_BYTES = (sizeof(ExpandArgs) + 15) & ~15;
constexpr int EXPAND_LDS_BYTES = 24 * 64 * 4 + TABLE_PAD + 64 * STAGE_STRIDE * 4 + 64 * 4 + EXPAND_COLD_BYTES;

__device__ __forceinline__ void store_choices(uint8_t *dst, uint64_t lo, uint32_t hi) { // 9 bytes at any address
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) dst[i] = (uint8_t)(lo >> (8 * i));
  dst[8] = (uint8_t)hi;
}

// One wave per workgroup, one record per lane; every loop turn each lane that still has a frame settles its row: the replay check
// (frame_check) fails -- from the first failing frame on every row of the record carries that verdict and zeros -- else the state goes to the lane's LDS slot and its
// small fields straight to their arrays, the wave copies the 64 slots out as whole rows, and the lane plays update(c1, c2).
template <int WPS>
__global__ __launch_bounds__(64, WPS) void k_frames_expand(ExpandArgs a_in) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<64, false>;
  Tables T = stage_tables((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4, OAK_MOVE_WORDS, OAK_MOVE_MAXPP, OAK_SPECIES_W0, OAK_SPECIES_W1, OAK_TYPE_CHART, OAK_BOOSTS);
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef OAK_LDS u32x4 lds_u128;
  lds_u32 *stage = (lds_u32 *)((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4 + TABLE_PAD);
  lds_u32 *srow = stage + 64 * STAGE_STRIDE; // the row each lane's slot goes to this turn
  lds_u32 *cold = srow + 64; // the arguments, parked (cold_ptr_at)
  if (threadIdx.x < sizeof(ExpandArgs) / 4) cold[threadIdx.x] = ((const uint32_t *)&a_in)[threadIdx.x];
  __syncthreads();
#define EA_PTR(field, type) cold_ptr_at<type>(cold, offsetof(ExpandArgs, field))
  const uint32_t tid = threadIdx.x, gid = blockIdx.x * 64 + tid;
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)cold[offsetof(ExpandArgs, n) / 4]);
  ER e;
  e.m = party + tid;
  e.T = T;
  uint32_t r = 0, nf = 0, k = 0, row0 = 0, res = 0, mn = 0, c1 = 0, c2 = 0, verdict = STATUS_PENDING, vwhere = 0;
  const uint8_t *fp = nullptr, *rec = nullptr; // frame k of this lane's record; the record
  if (gid < n) {
    const uint32_t first_record = cold[offsetof(ExpandArgs, first_record) / 4];
    r = first_record + EA_PTR(order, const uint32_t *)[gid];
    if (!EA_PTR(malformed, const uint8_t *)[r]) { // (a malformed record has no rows)
      nf = EA_PTR(frames, const uint16_t *)[r];
      const uint64_t *bases = EA_PTR(bases, const uint64_t *);
      row0 = (uint32_t)(bases[r] - bases[first_record]);
      rec = EA_PTR(records, const uint8_t *) + EA_PTR(offsets, const uint64_t *)[r];
      const uint32_t stored = rec[390] & 15;
      if (stored < R_WIN || stored > R_TIE) { verdict = OAKGPU_REPLAY_RESULT; vwhere = nf; } // (there is no score)
      else if (nf) {
        e.load_battle_global(EA_PTR(aligned, const uint8_t *) + (size_t)r * 384, 0, 0); // zero durations (frames.h:57-59)
        res = EA_PTR(first, const uint8_t *)[r];
        fp = rec + 391;
        mn = fp[0]; c1 = fp[1]; c2 = fp[2];
      }
    }
  }
  for (;;) {
    const bool live = k < nf;
    if (__ballot(live) == 0) break;
    uint32_t row = ROW_NONE;
    bool play = false;
    if (live) {
      row = row0 + k;
      typename ER::Choices l1{0, 0, 0}, l2{0, 0, 0};
      if (verdict == STATUS_PENDING) {
        verdict = frame_check(e, res, mn, c1, c2, l1, l2).status;
        if (verdict != STATUS_PENDING) vwhere = k;
      }
      const bool ok = verdict == STATUS_PENDING;
      if (ok) e.store_battle_global((uint8_t *)(stage + tid * STAGE_STRIDE));
      else {
#pragma unroll
        for (int w = 0; w < 24; ++w) *(lds_u128 *)(stage + tid * STAGE_STRIDE + 4 * w) = u32x4{0, 0, 0, 0};
        l1 = l2 = typename ER::Choices{0, 0, 0};
      }
      *(uint2 *)(EA_PTR(durations, uint8_t *) + 8 * (size_t)row) = ok ? make_uint2(e.S.dur, e.F.dur) : make_uint2(0, 0);
      EA_PTR(results, uint8_t *)[row] = ok ? (uint8_t)res : 0;
      store_choices(EA_PTR(ch1, uint8_t *) + (size_t)row * OAKGPU_MAX_CHOICES, l1.lo, l1.hi);
      store_choices(EA_PTR(ch2, uint8_t *) + (size_t)row * OAKGPU_MAX_CHOICES, l2.lo, l2.hi);
      EA_PTR(cnt1, uint8_t *)[row] = (uint8_t)l1.n;
      EA_PTR(cnt2, uint8_t *)[row] = (uint8_t)l2.n;
      EA_PTR(status, uint8_t *)[row] = ok ? (uint8_t)OAKGPU_REPLAY_OK : (uint8_t)verdict;
      EA_PTR(where, uint32_t *)[row] = ok ? k : vwhere;
      *(uint2 *)(EA_PTR(rowrec, uint32_t *) + 2 * (size_t)row) = make_uint2(ok ? (uint32_t)(fp - rec) : 0u, r);
      play = ok && k + 1 < nf; // (the state behind the last frame is nobody's row)
    }
    srow[tid] = row;
    __syncthreads();
    {
      u32x4 *dst = (u32x4 *)EA_PTR(battles, uint8_t *);
#pragma unroll 4
      for (int q = 0; q < 24; ++q) {
        const uint32_t i = q * 64 + tid, b = i / 24, w = i - b * 24, to = srow[b];
        if (to != ROW_NONE) dst[(size_t)to * 24 + w] = *(const lds_u128 *)(stage + b * STAGE_STRIDE + 4 * w);
      }
    }
    __syncthreads();
    if (play) res = play_frame(e, fp, mn, c1, c2, true);
    ++k;
  }
#undef EA_PTR
}

// ---- the terms -------------------------------------------------------------------------------------------------------------------
struct TermArgs {
  const float *value_in, *l1, *l2;          // the evaluator's outputs over the chunk's rows
  const uint8_t *cnt1, *cnt2, *ch1, *ch2, *status;
  const uint32_t *rowrec;
  const uint8_t *records;
  const uint64_t *offsets;
  oakgpu_corpus_eval out;                    // each nullable
  oakgpu_corpus_terms terms;                 // sq_err, ce, excluded nullable together (`loss` says whether they are wanted)
  oakgpu_loss_params p;
  uint32_t rows, loss;
};

// softmax over the first k logits (shifted by their maximum), and the log-softmax the cross entropy reads
__device__ __forceinline__ void side_terms(const float *logit, uint32_t k, const uint8_t *emp16, const uint8_t *nash16, float pn, bool loss,
                                           float (&policy)[OAKGPU_MAX_CHOICES], float &ce) {
  float mx = -INFINITY, ex[OAKGPU_MAX_CHOICES], sum = 0.0f;
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) if (i < k) mx = fmaxf(mx, logit[i]);
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) {
    ex[i] = i < k ? expf(__fsub_rn(logit[i], mx)) : 0.0f;
    sum = __fadd_rn(sum, ex[i]);
  }
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) policy[i] = i < k ? __fdiv_rn(ex[i], sum) : 0.0f;
  ce = 0.0f;
  if (!loss) return;
  const float lse = logf(sum), we = __fsub_rn(1.0f, pn);
  float acc = 0.0f;
  uint32_t support = 0;
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) {
    if (i < k) { // Update::write_to_tensor: u16 / 65535.0f; battle.py:238-245: (1 - pn) * empirical + pn * nash
      const float emp = __fdiv_rn((float)load_u16(emp16 + 2 * i), 65535.0f), nash = __fdiv_rn((float)load_u16(nash16 + 2 * i), 65535.0f);
      const float t = __fadd_rn(__fmul_rn(we, emp), __fmul_rn(pn, nash));
      const float logp = __fsub_rn(__fsub_rn(logit[i], mx), lse);
      support += t != 0.0f;
      acc = __fadd_rn(acc, __fmul_rn(-t, logp));
    }
  }
  ce = __fdiv_rn(acc, (float)max(support, 1u));
}

__global__ __launch_bounds__(256) void k_corpus_terms(TermArgs a) {
  const uint32_t row = blockIdx.x * 256 + threadIdx.x;
  if (row >= a.rows) return;
  const uint32_t status = a.status[row];
  const bool ok = status == OAKGPU_REPLAY_OK;
  const uint32_t k1 = ok ? a.cnt1[row] : 0, k2 = ok ? a.cnt2[row] : 0;
  float lg[2][OAKGPU_MAX_CHOICES], policy[2][OAKGPU_MAX_CHOICES], ce[2] = {0.0f, 0.0f};
#pragma unroll
  for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) {
    lg[0][i] = i < k1 ? a.l1[(size_t)row * OAKGPU_MAX_CHOICES + i] : 0.0f;
    lg[1][i] = i < k2 ? a.l2[(size_t)row * OAKGPU_MAX_CHOICES + i] : 0.0f;
  }
  const float value = ok ? a.value_in[row] : 0.0f; // (a row that is not OK was evaluated as a zero state: its output is dropped)
  const uint8_t *fr = ok ? a.records + a.offsets[a.rowrec[2 * (size_t)row + 1]] + a.rowrec[2 * (size_t)row] : nullptr;
  bool counted = false;
  if (a.loss && ok) counted = load_u32(fr + 3) >= a.p.min_iterations;
  const uint8_t *t1 = ok ? fr + 11 : nullptr, *t2 = ok ? fr + 11 + 4 * k1 : nullptr; // (k1 = the frame's m: the row is OK)
  if (ok) {
    side_terms(lg[0], k1, t1, t1 + 2 * k1, a.p.pn, counted, policy[0], ce[0]);
    side_terms(lg[1], k2, t2, t2 + 2 * k2, a.p.pn, counted, policy[1], ce[1]);
  } else {
#pragma unroll
    for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) policy[0][i] = policy[1][i] = 0.0f;
  }
  if (a.out.value) a.out.value[row] = value;
#pragma unroll
  for (uint32_t s = 0; s < 2; ++s)
#pragma unroll
    for (uint32_t i = 0; i < OAKGPU_MAX_CHOICES; ++i) {
      const size_t at = ((size_t)row * 2 + s) * OAKGPU_MAX_CHOICES + i;
      if (a.out.policy_logit) a.out.policy_logit[at] = lg[s][i];
      if (a.out.policy) a.out.policy[at] = policy[s][i];
      if (a.out.choices) a.out.choices[at] = (s ? a.ch2 : a.ch1)[(size_t)row * OAKGPU_MAX_CHOICES + i];
    }
  if (a.out.k) { a.out.k[2 * (size_t)row] = (uint8_t)k1; a.out.k[2 * (size_t)row + 1] = (uint8_t)k2; }
  if (a.out.status && a.out.status != a.status) a.out.status[row] = (uint8_t)status;
  if (a.loss) {
    float sq = 0.0f;
    if (counted) { // battle.py:227-231: (wn * nash + we * empirical) + ws * score, fp32
      const float emp = __fdiv_rn((float)load_u16(fr + 7), 65535.0f), nash = __fdiv_rn((float)load_u16(fr + 9), 65535.0f);
      const uint32_t type = (a.records + a.offsets[a.rowrec[2 * (size_t)row + 1]])[390] & 15;
      const float score = type == R_WIN ? 1.0f : type == R_LOSE ? 0.0f : 0.5f; // PKMN::score (libpkmn/pkmn.h:174-190)
      const float vt = __fadd_rn(__fadd_rn(__fmul_rn(a.p.wn, nash), __fmul_rn(a.p.we, emp)), __fmul_rn(a.p.ws, score));
      const float d = __fsub_rn(value, vt);
      sq = __fmul_rn(d, d);
    }
    a.terms.sq_err[row] = sq;
    a.terms.ce[2 * (size_t)row] = ce[0];
    a.terms.ce[2 * (size_t)row + 1] = ce[1];
    a.terms.excluded[row] = !ok ? 2 : counted ? 0 : 1;
  }
}

// One lane per record of the chunk: its rows in frame order.  sums: n x 3 doubles (sq_err, ce p1, ce p2); counts: n x 3 (rows included,
// excluded for their iterations, not OK).
__global__ __launch_bounds__(64) void k_corpus_record_sums(const float *sq_err, const float *ce, const uint8_t *excluded, const uint64_t *bases,
                                                           uint32_t first_record, uint32_t n, double *sums, uint32_t *counts) {
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  const uint32_t lo = (uint32_t)(bases[first_record + j] - bases[first_record]), hi = (uint32_t)(bases[first_record + j + 1] - bases[first_record]);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  uint32_t c[3] = {0, 0, 0};
  for (uint32_t row = lo; row < hi; ++row) {
    const uint32_t x = excluded[row];
    c[0] += x == 0; c[1] += x == 1; c[2] += x == 2;
    if (x == 0) { s0 += (double)sq_err[row]; s1 += (double)ce[2 * (size_t)row]; s2 += (double)ce[2 * (size_t)row + 1]; }
  }
  sums[3 * (size_t)j] = s0; sums[3 * (size_t)j + 1] = s1; sums[3 * (size_t)j + 2] = s2;
  counts[3 * (size_t)j] = c[0]; counts[3 * (size_t)j + 1] = c[1]; counts[3 * (size_t)j + 2] = c[2];
}

} // namespace ce
} // namespace oak

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t DEFAULT_CHUNK_ROWS = 65536;

// the corpus' workspace of a chunk: the prefix sums (once), the lane order, and -- for the calls that evaluate -- the states
struct EvalWs {
  uint64_t *bases = nullptr;
  std::vector<uint64_t> h_bases;
  uint32_t *order = nullptr, order_cap = 0;
  uint32_t *rowrec = nullptr, rowrec_cap = 0;
  uint32_t rows_cap = 0;
  uint8_t *battles = nullptr, *durations = nullptr, *results = nullptr, *ch1 = nullptr, *cnt1 = nullptr, *ch2 = nullptr, *cnt2 = nullptr, *status = nullptr;
  uint32_t *where = nullptr;
  float *value = nullptr, *l1 = nullptr, *l2 = nullptr;
};

void ws_free(void *p) { // (the stream is idle: corpus_free's callers have waited for it)
  EvalWs *w = (EvalWs *)p;
  for (void *q : {(void *)w->bases, (void *)w->order, (void *)w->rowrec, (void *)w->battles, (void *)w->durations, (void *)w->results, (void *)w->ch1, (void *)w->cnt1,
                  (void *)w->ch2, (void *)w->cnt2, (void *)w->status, (void *)w->where, (void *)w->value, (void *)w->l1, (void *)w->l2})
    if (q) (void)hipFree(q);
  delete w;
}

template <class T>
int dev_grow(oakgpu_corpus *k, T *&p, uint32_t &cap, size_t per, uint32_t want) { // grow-only; an earlier chunk may still read the old block
  if (want <= cap && p) return 0;
  HIPCHK(hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(k->ctx)));
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  if (dev_alloc(p, per * std::max(want, 1u))) return -1;
  cap = std::max(want, 1u);
  return 0;
}

int workspace(oakgpu_corpus *k, EvalWs **out) { // the prefix sums are uploaded once (the call waits for the stream then)
  if (!k->eval) {
    EvalWs *w = new EvalWs;
    w->h_bases.assign((size_t)k->n + 1, 0);
    for (uint32_t r = 0; r < k->n; ++r) w->h_bases[r + 1] = w->h_bases[r] + (k->h_malformed[r] ? 0u : k->h_frames[r]);
    hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(k->ctx);
    int rc = dev_alloc(w->bases, (size_t)k->n + 1);
    if (!rc) {
      hipError_t e = hipMemcpyAsync(w->bases, w->h_bases.data(), ((size_t)k->n + 1) * 8, hipMemcpyHostToDevice, stream);
      const hipError_t done = hipStreamSynchronize(stream);
      if (e == hipSuccess) e = done;
      if (e != hipSuccess) rc = oakgpu_fail_hip((int)e, "corpus evaluation: prefix sums");
    }
    if (rc) { ws_free(w); return rc; }
    k->eval = w;
    k->eval_free = ws_free;
  }
  *out = (EvalWs *)k->eval;
  return 0;
}

int reserve_rows(oakgpu_corpus *k, EvalWs *w, uint32_t rows) { // the states and evaluator outputs of a chunk
  if (rows <= w->rows_cap) return 0;
  HIPCHK(hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(k->ctx)));
  for (void **q : {(void **)&w->battles, (void **)&w->durations, (void **)&w->results, (void **)&w->ch1, (void **)&w->cnt1, (void **)&w->ch2, (void **)&w->cnt2,
                   (void **)&w->status, (void **)&w->where, (void **)&w->value, (void **)&w->l1, (void **)&w->l2}) {
    if (*q) (void)hipFree(*q);
    *q = nullptr;
  }
  w->rows_cap = 0;
  const size_t n = rows;
  if (dev_alloc(w->battles, n * 384) || dev_alloc(w->durations, n * 8) || dev_alloc(w->results, n) || dev_alloc(w->ch1, n * 9) || dev_alloc(w->cnt1, n) ||
      dev_alloc(w->ch2, n * 9) || dev_alloc(w->cnt2, n) || dev_alloc(w->status, n) || dev_alloc(w->where, n) || dev_alloc(w->value, n) || dev_alloc(w->l1, n * 9) ||
      dev_alloc(w->l2, n * 9))
    return -1;
  w->rows_cap = rows;
  return 0;
}

// the range's rows, checked against the caller's capacity; *rows = 0 is a chunk without work
int chunk_rows_of(const char *who, oakgpu_ctx *c, oakgpu_corpus *k, uint32_t first_record, uint32_t n_records, uint32_t rows_capacity, EvalWs **w, uint32_t *rows) {
  static char msg[200];
  if (!c || !k || k->ctx != c) { snprintf(msg, sizeof msg, "%s: the corpus does not belong to this context", who); return oakgpu_fail_msg(msg); }
  if ((uint64_t)first_record + n_records > k->n) { snprintf(msg, sizeof msg, "%s: records %u .. %llu are not all in the corpus (%u records)", who, first_record, (unsigned long long)first_record + n_records, k->n); return oakgpu_fail_msg(msg); }
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  if (int rc = workspace(k, w)) return rc;
  const uint64_t total = (*w)->h_bases[first_record + n_records] - (*w)->h_bases[first_record];
  if (total > rows_capacity) {
    snprintf(msg, sizeof msg, "%s: records %u .. %u hold %llu frames, more than rows_capacity %u", who, first_record, first_record + n_records - 1, (unsigned long long)total, rows_capacity);
    return oakgpu_fail_msg(msg);
  }
  *rows = (uint32_t)total;
  return 0;
}

int expand(oakgpu_ctx *c, oakgpu_corpus *k, EvalWs *w, uint32_t first_record, uint32_t n_records, uint32_t rows, uint8_t *battles, uint8_t *durations,
           uint8_t *results, uint8_t *ch1, uint8_t *cnt1, uint8_t *ch2, uint8_t *cnt2, uint8_t *status, uint32_t *where) {
  using namespace oak::ce;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  if (dev_grow(k, w->order, w->order_cap, 1, n_records) || dev_grow(k, w->rowrec, w->rowrec_cap, 2, rows)) return -1;
  hipLaunchKernelGGL(k_chunk_order, dim3(1), dim3(1024), 0, stream, k->frames + first_record, k->malformed + first_record, n_records, w->order);
  const ExpandArgs ea{k->records, k->offsets, k->frames, k->malformed, k->aligned, k->first, w->bases, w->order, battles, durations, results,
                      ch1, cnt1, ch2, cnt2, status, where, w->rowrec, first_record, n_records};
  hipLaunchKernelGGL((k_frames_expand<4>), dim3((n_records + 63) / 64), dim3(64), EXPAND_LDS_BYTES, stream, ea);
  HIPCHK(hipGetLastError());
  return 0;
}

int check_params(const oakgpu_loss_params *p, const char *who) {
  static char msg[120];
  if (!p) { snprintf(msg, sizeof msg, "%s: null loss parameters", who); return oakgpu_fail_msg(msg); }
  return 0;
}

// expander -> evaluator -> terms (-> record sums) over one chunk, on the context's stream
int eval_chunk(const char *who, oakgpu_ctx *c, oakgpu_net *net, oakgpu_corpus *k, uint32_t first_record, uint32_t n_records, uint32_t rows_capacity,
               const oakgpu_corpus_eval *out, const oakgpu_loss_params *p, const oakgpu_corpus_terms *terms) {
  using namespace oak::ce;
  static char msg[160];
  EvalWs *w = nullptr;
  uint32_t rows = 0;
  if (!net) { snprintf(msg, sizeof msg, "%s: null network", who); return oakgpu_fail_msg(msg); }
  if (terms && (!terms->sq_err || !terms->ce || !terms->excluded || !terms->record_sums || !terms->record_counts)) {
    snprintf(msg, sizeof msg, "%s: null term array", who);
    return oakgpu_fail_msg(msg);
  }
  if ((out && (((uintptr_t)out->value & 3) || ((uintptr_t)out->policy_logit & 3) || ((uintptr_t)out->policy & 3) || ((uintptr_t)out->where & 3))) ||
      (terms && (((uintptr_t)terms->sq_err & 3) || ((uintptr_t)terms->ce & 3) || ((uintptr_t)terms->record_sums & 7) || ((uintptr_t)terms->record_counts & 3)))) {
    snprintf(msg, sizeof msg, "%s: misaligned array (record_sums: 8 bytes; the other 4-byte types: 4)", who);
    return oakgpu_fail_msg(msg);
  }
  if (int rc = chunk_rows_of(who, c, k, first_record, n_records, rows_capacity, &w, &rows)) return rc;
  if (n_records == 0) return 0;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  if (rows) {
    if (int rc = reserve_rows(k, w, rows)) return rc;
    uint32_t *where = out && out->where ? out->where : w->where;
    if (int rc = expand(c, k, w, first_record, n_records, rows, w->battles, w->durations, w->results, w->ch1, w->cnt1, w->ch2, w->cnt2, w->status, where)) return rc;
    if (int rc = oakgpu_leaf_eval_policy_dev(c, net, w->battles, w->durations, rows, w->ch1, w->cnt1, w->ch2, w->cnt2, w->value, w->l1, w->l2)) return rc;
    TermArgs ta{};
    ta.value_in = w->value; ta.l1 = w->l1; ta.l2 = w->l2;
    ta.cnt1 = w->cnt1; ta.cnt2 = w->cnt2; ta.ch1 = w->ch1; ta.ch2 = w->ch2; ta.status = w->status;
    ta.rowrec = w->rowrec; ta.records = k->records; ta.offsets = k->offsets;
    if (out) ta.out = *out;
    if (terms) { ta.terms = *terms; ta.p = *p; ta.loss = 1; }
    ta.rows = rows;
    hipLaunchKernelGGL(k_corpus_terms, dim3((rows + 255) / 256), dim3(256), 0, stream, ta);
  }
  if (terms)
    hipLaunchKernelGGL(k_corpus_record_sums, dim3((n_records + 63) / 64), dim3(64), 0, stream, terms->sq_err, terms->ce, terms->excluded, w->bases, first_record,
                       n_records, terms->record_sums, terms->record_counts);
  HIPCHK(hipGetLastError());
  return 0;
}

void finish(oakgpu_corpus_losses *l) {
  const double d = l->rows ? (double)l->rows : 1.0;
  l->mse = l->sq_err / d;
  l->ce_p1 = l->ce1 / d;
  l->ce_p2 = l->ce2 / d;
}

} // namespace

extern "C" {

int oakgpu_corpus_frame_bases(const oakgpu_corpus *k, uint64_t *bases) {
  if (!k || !bases) return oakgpu_fail_msg("oakgpu_corpus_frame_bases: null argument");
  bases[0] = 0;
  for (uint32_t r = 0; r < k->n; ++r) bases[r + 1] = bases[r] + (k->h_malformed[r] ? 0u : k->h_frames[r]);
  return 0;
}

int oakgpu_corpus_chunks(const uint16_t *frames, const uint8_t *malformed, uint32_t n, uint32_t chunk_rows, uint32_t *first_record, uint32_t capacity,
                         uint32_t *n_chunks) {
  static char msg[160];
  if (!n_chunks || (n && !frames)) return oakgpu_fail_msg("oakgpu_corpus_chunks: null argument");
  if (chunk_rows == 0) chunk_rows = DEFAULT_CHUNK_ROWS;
  uint32_t chunks = 0, rows = 0;
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t f = malformed && malformed[r] ? 0u : frames[r];
    if (f > chunk_rows) {
      snprintf(msg, sizeof msg, "oakgpu_corpus_chunks: record %u has %u frames, more than chunk_rows %u", r, f, chunk_rows);
      return oakgpu_fail_msg(msg);
    }
    if (r == 0 || rows + f > chunk_rows) { // a new chunk starts at r
      if (first_record && chunks < capacity) first_record[chunks] = r;
      ++chunks;
      rows = 0;
    }
    rows += f;
  }
  *n_chunks = chunks;
  if (first_record) {
    if (chunks + 1 > capacity) return oakgpu_fail_msg("oakgpu_corpus_chunks: capacity is below the chunk count + 1");
    first_record[chunks] = n;
  }
  return 0;
}

int oakgpu_corpus_states_dev(oakgpu_ctx *c, oakgpu_corpus *k, uint32_t first_record, uint32_t n_records, uint32_t rows_capacity, uint8_t *battles,
                             uint8_t *durations, uint8_t *results, uint8_t *p1_choices, uint8_t *p1_counts, uint8_t *p2_choices, uint8_t *p2_counts, uint8_t *status,
                             uint32_t *where) {
  EvalWs *w = nullptr;
  uint32_t rows = 0;
  if (!battles || !durations || !results || !p1_choices || !p1_counts || !p2_choices || !p2_counts || !status || !where)
    return oakgpu_fail_msg("oakgpu_corpus_states_dev: null pointer");
  if (((uintptr_t)battles & 15) || ((uintptr_t)durations & 7) || ((uintptr_t)where & 3))
    return oakgpu_fail_msg("oakgpu_corpus_states_dev: misaligned array (battles: 16 bytes; durations: 8; where: 4)");
  if (int rc = chunk_rows_of("oakgpu_corpus_states_dev", c, k, first_record, n_records, rows_capacity, &w, &rows)) return rc;
  if (rows == 0) return 0;
  return expand(c, k, w, first_record, n_records, rows, battles, durations, results, p1_choices, p1_counts, p2_choices, p2_counts, status, where);
}

int oakgpu_corpus_inference_dev(oakgpu_ctx *c, oakgpu_net *net, oakgpu_corpus *k, uint32_t first_record, uint32_t n_records, uint32_t rows_capacity,
                                const oakgpu_corpus_eval *out) {
  if (!out) return oakgpu_fail_msg("oakgpu_corpus_inference_dev: null outputs");
  return eval_chunk("oakgpu_corpus_inference_dev", c, net, k, first_record, n_records, rows_capacity, out, nullptr, nullptr);
}

int oakgpu_corpus_loss_dev(oakgpu_ctx *c, oakgpu_net *net, oakgpu_corpus *k, uint32_t first_record, uint32_t n_records, uint32_t rows_capacity,
                           const oakgpu_loss_params *p, const oakgpu_corpus_eval *out, const oakgpu_corpus_terms *terms) {
  if (int rc = check_params(p, "oakgpu_corpus_loss_dev")) return rc;
  if (!terms) return oakgpu_fail_msg("oakgpu_corpus_loss_dev: null terms");
  return eval_chunk("oakgpu_corpus_loss_dev", c, net, k, first_record, n_records, rows_capacity, out, p, terms);
}

// the chunks of records first .. first + n - 1 (host list, first_record[n_chunks] = first + n)
static int chunk_list(oakgpu_corpus *k, uint32_t first, uint32_t n, uint32_t chunk_rows, std::vector<uint32_t> &firsts) {
  uint32_t count = 0;
  if (int rc = oakgpu_corpus_chunks(k->h_frames.data() + first, k->h_malformed.data() + first, n, chunk_rows, nullptr, 0, &count)) return rc;
  firsts.assign((size_t)count + 1, 0);
  if (int rc = oakgpu_corpus_chunks(k->h_frames.data() + first, k->h_malformed.data() + first, n, chunk_rows, firsts.data(), count + 1, &count)) return rc;
  for (uint32_t &f : firsts) f += first;
  return 0;
}

int oakgpu_corpus_states(oakgpu_ctx *c, oakgpu_corpus *k, uint32_t first_record, uint32_t n_records, uint32_t rows_capacity, uint8_t *battles, uint8_t *durations,
                         uint8_t *results, uint8_t *p1_choices, uint8_t *p1_counts, uint8_t *p2_choices, uint8_t *p2_counts, uint8_t *status, uint32_t *where) {
  if (!c || !k || k->ctx != c) return oakgpu_fail_msg("oakgpu_corpus_states: the corpus does not belong to this context");
  if (!battles || !durations || !results || !p1_choices || !p1_counts || !p2_choices || !p2_counts || !status || !where)
    return oakgpu_fail_msg("oakgpu_corpus_states: null pointer");
  EvalWs *w = nullptr;
  uint32_t rows = 0;
  if (int rc = chunk_rows_of("oakgpu_corpus_states", c, k, first_record, n_records, rows_capacity, &w, &rows)) return rc;
  if (rows == 0) return 0;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  OakHostCall hc(c);
  static const size_t per[9] = {384, 8, 1, 9, 1, 9, 1, 1, 4};
  void *host[9] = {battles, durations, results, p1_choices, p1_counts, p2_choices, p2_counts, status, where}, *dev[9];
  for (int t = 0; t < 9; ++t) if (!(dev[t] = hc.get(std::max<size_t>(per[t] * rows, 16)))) return -1;
  if (int rc = oakgpu_corpus_states_dev(c, k, first_record, n_records, rows, (uint8_t *)dev[0], (uint8_t *)dev[1], (uint8_t *)dev[2], (uint8_t *)dev[3], (uint8_t *)dev[4],
                                        (uint8_t *)dev[5], (uint8_t *)dev[6], (uint8_t *)dev[7], (uint32_t *)dev[8]))
    return rc;
  for (int t = 0; t < 9; ++t) HIPCHK(hipMemcpyAsync(host[t], dev[t], per[t] * rows, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

// host arrays of every row of records first .. first + n - 1, chunk by chunk through one set of staged device arrays
int oakgpu_corpus_inference(oakgpu_ctx *c, oakgpu_net *net, oakgpu_corpus *k, uint32_t first_record, uint32_t n_records, uint32_t chunk_rows,
                            const oakgpu_corpus_eval *out) {
  if (!c || !k || k->ctx != c) return oakgpu_fail_msg("oakgpu_corpus_inference: the corpus does not belong to this context");
  if (!out) return oakgpu_fail_msg("oakgpu_corpus_inference: null outputs");
  if ((uint64_t)first_record + n_records > k->n) return oakgpu_fail_msg("oakgpu_corpus_inference: the records are not all in the corpus");
  if (chunk_rows == 0) chunk_rows = DEFAULT_CHUNK_ROWS;
  std::vector<uint32_t> firsts;
  if (int rc = chunk_list(k, first_record, n_records, chunk_rows, firsts)) return rc;
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  EvalWs *w = nullptr;
  if (int rc = workspace(k, &w)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  OakHostCall hc(c);
  static const size_t per[7] = {4, 72, 72, 2, 18, 1, 4};
  static_assert(sizeof(oakgpu_corpus_eval) == 7 * sizeof(void *), "a struct of 7 pointers");
  void *const *host = (void *const *)out;
  oakgpu_corpus_eval dev{};
  void **devp = (void **)&dev;
  uint32_t biggest = 0;
  for (size_t i = 0; i + 1 < firsts.size(); ++i) biggest = std::max(biggest, (uint32_t)(w->h_bases[firsts[i + 1]] - w->h_bases[firsts[i]]));
  for (int t = 0; t < 7; ++t)
    if (host[t] && !(devp[t] = hc.get(std::max<size_t>(per[t] * biggest, 16)))) return -1;
  for (size_t i = 0; i + 1 < firsts.size(); ++i) {
    const uint64_t row0 = w->h_bases[firsts[i]] - w->h_bases[first_record];
    const uint32_t rows = (uint32_t)(w->h_bases[firsts[i + 1]] - w->h_bases[firsts[i]]);
    if (rows == 0) continue;
    if (int rc = oakgpu_corpus_inference_dev(c, net, k, firsts[i], firsts[i + 1] - firsts[i], rows, &dev)) return rc;
    for (int t = 0; t < 7; ++t)
      if (host[t]) HIPCHK(hipMemcpyAsync((uint8_t *)host[t] + per[t] * row0, devp[t], per[t] * rows, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream)); // (the next chunk writes the same staged arrays)
  }
  return 0;
}

int oakgpu_corpus_evaluate(oakgpu_ctx *c, oakgpu_net *net, oakgpu_corpus *k, const oakgpu_loss_params *p, uint32_t chunk_rows, oakgpu_corpus_losses *total,
                           oakgpu_corpus_losses *per_record) {
  if (!c || !k || k->ctx != c) return oakgpu_fail_msg("oakgpu_corpus_evaluate: the corpus does not belong to this context");
  if (int rc = check_params(p, "oakgpu_corpus_evaluate")) return rc;
  if (!total) return oakgpu_fail_msg("oakgpu_corpus_evaluate: null totals");
  if (chunk_rows == 0) chunk_rows = DEFAULT_CHUNK_ROWS;
  std::vector<uint32_t> firsts;
  if (int rc = chunk_list(k, 0, k->n, chunk_rows, firsts)) return rc;
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  EvalWs *w = nullptr;
  if (int rc = workspace(k, &w)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  OakHostCall hc(c);
  uint32_t biggest = 0, most = 0;
  for (size_t i = 0; i + 1 < firsts.size(); ++i) {
    biggest = std::max(biggest, (uint32_t)(w->h_bases[firsts[i + 1]] - w->h_bases[firsts[i]]));
    most = std::max(most, firsts[i + 1] - firsts[i]);
  }
  oakgpu_corpus_terms terms{};
  terms.sq_err = (float *)hc.get(std::max<size_t>(4 * (size_t)biggest, 16));
  terms.ce = (float *)hc.get(std::max<size_t>(8 * (size_t)biggest, 16));
  terms.excluded = (uint8_t *)hc.get(std::max<size_t>(biggest, 16));
  terms.record_sums = (double *)hc.get(std::max<size_t>(24 * (size_t)most, 16));
  terms.record_counts = (uint32_t *)hc.get(std::max<size_t>(12 * (size_t)most, 16));
  if (!terms.sq_err || !terms.ce || !terms.excluded || !terms.record_sums || !terms.record_counts) return -1;
  std::vector<double> sums(3 * (size_t)std::max(most, 1u));
  std::vector<uint32_t> counts(3 * (size_t)std::max(most, 1u));
  *total = oakgpu_corpus_losses{};
  for (size_t i = 0; i + 1 < firsts.size(); ++i) {
    const uint32_t n = firsts[i + 1] - firsts[i], rows = (uint32_t)(w->h_bases[firsts[i + 1]] - w->h_bases[firsts[i]]);
    if (int rc = oakgpu_corpus_loss_dev(c, net, k, firsts[i], n, rows, p, nullptr, &terms)) return rc;
    HIPCHK(hipMemcpyAsync(sums.data(), terms.record_sums, 24 * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(counts.data(), terms.record_counts, 12 * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (uint32_t j = 0; j < n; ++j) { // record order: the totals do not depend on the chunking
      oakgpu_corpus_losses one{};
      one.sq_err = sums[3 * (size_t)j]; one.ce1 = sums[3 * (size_t)j + 1]; one.ce2 = sums[3 * (size_t)j + 2];
      one.rows = counts[3 * (size_t)j]; one.excluded = counts[3 * (size_t)j + 1]; one.failed = counts[3 * (size_t)j + 2];
      total->sq_err += one.sq_err; total->ce1 += one.ce1; total->ce2 += one.ce2;
      total->rows += one.rows; total->excluded += one.excluded; total->failed += one.failed;
      if (per_record) { finish(&one); per_record[firsts[i] + j] = one; }
    }
  }
  finish(total);
  return 0;
}

} // extern "C"
