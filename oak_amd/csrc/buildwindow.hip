// oak_amd/csrc/buildwindow.hip -- the newest `.build.data` records, resident on the device: a corpus of ONE file that self-play appends to
// (the contract is in include/oakgpu.h; the battle side's counterpart is the replay window of corpus.hip).
//
//   k_window_mark : one workgroup over the incoming batch: a record whose format byte is 0 is accepted; each accepted record's index among
//                   the accepted (an inclusive scan per pass of 256, the base carried from pass to pass), and the two totals the host reads
//   k_window_move : 8 lanes x 16 bytes per record: the surviving records of the window, oldest first, then the accepted records of the
//                   batch, into the buffer the window holds next; one lane writes the file table {0, records held}
// The window owns two record buffers of max_records x 128 bytes.  An append that fits goes behind the held records in place; one that
// evicts compacts survivors and newcomers into the other buffer, and the two swap.  The host waits for the stream once per append, for the
// two totals: what it then knows -- the records held -- is all the corpus calls need.  The status scan is redone when next asked for.
#include <string>

#include "oakgpu_internal.h"
#include "build_corpus.hpp"

namespace bt = oak_build_traj;

struct oakgpu_build_window {
  oakgpu_build_corpus corpus; // what every corpus call is handed; its `records` is the buffer in use
  uint32_t max_records = 0;
  uint8_t *buffer[2] = {nullptr, nullptr};
  int cur = 0;
  uint32_t *slot = nullptr;     // per incoming record: its index among the accepted, or NONE
  uint32_t slot_capacity = 0;
  uint32_t *totals = nullptr;   // accepted, rejected
  uint8_t *staging = nullptr;   // the host form's upload: the records, then the count word
  size_t staging_capacity = 0;
  uint64_t appended = 0, evicted = 0, rejected = 0;
};

namespace {
#define RC(x) do { int _r = (x); if (_r) return _r; } while (0)

constexpr uint32_t RECORD_BYTES = bt::RECORD_BYTES, MARK_BLOCK = 256, NONE = 0xFFFFFFFFu;
static_assert(RECORD_BYTES == 128 && RECORD_BYTES == OAKGPU_BUILD_RECORD_BYTES, "a record is eight 16-byte words");
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

int fail(const char *fn, const std::string &what) { return oakgpu_fail_msg((std::string(fn) + ": " + what).c_str()); }

__global__ __launch_bounds__(MARK_BLOCK) void k_window_mark(const uint8_t *records, const uint32_t *count, uint32_t max_count, uint32_t *slot, uint32_t *totals) {
  __shared__ uint32_t s_scan[MARK_BLOCK];
  __shared__ uint32_t s_base;
  const uint32_t tid = threadIdx.x;
  const uint32_t n = *count < max_count ? *count : max_count; // (a count word beyond the buffer is cut to the buffer)
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (uint32_t first = 0; first < n; first += MARK_BLOCK) {
    const uint32_t i = first + tid;
    const bool ok = i < n && records[(size_t)i * RECORD_BYTES] == 0;
    s_scan[tid] = ok;
    __syncthreads();
    for (uint32_t d = 1; d < MARK_BLOCK; d <<= 1) { // inclusive scan
      const uint32_t v = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    const uint32_t base = s_base;
    if (i < n) slot[i] = ok ? base + s_scan[tid] - 1 : NONE;
    __syncthreads();
    if (tid == MARK_BLOCK - 1) s_base = base + s_scan[tid];
    __syncthreads();
  }
  if (tid == 0) { totals[0] = s_base; totals[1] = n - s_base; }
}

struct MoveArgs {
  const uint8_t *from; // the buffer in use: its records [first_kept, first_kept + kept) survive (kept = 0: none is moved)
  uint8_t *to;         // the buffer in use next (the same one for an append in place)
  uint32_t first_kept, kept;
  const uint8_t *incoming;
  const uint32_t *slot;
  uint32_t batch;      // incoming records looked at
  uint32_t first_taken; // accepted records with a lower index are older than the window
  uint32_t base;       // where the accepted record `first_taken` goes
  uint32_t *file_first;
  uint32_t held;       // records held after the append
};

__global__ __launch_bounds__(256) void k_window_move(MoveArgs a) {
  const uint32_t item = blockIdx.x * 32 + (threadIdx.x >> 3), word = threadIdx.x & 7;
  if (blockIdx.x == 0 && threadIdx.x == 0) { a.file_first[0] = 0; a.file_first[1] = a.held; }
  if (item < a.kept) {
    ((u32x4 *)a.to)[(size_t)item * 8 + word] = ((const u32x4 *)a.from)[(size_t)(a.first_kept + item) * 8 + word];
  } else if (item - a.kept < a.batch) {
    const uint32_t i = item - a.kept, s = a.slot[i];
    if (s == NONE || s < a.first_taken) return;
    ((u32x4 *)a.to)[(size_t)(a.base + s - a.first_taken) * 8 + word] = ((const u32x4 *)a.incoming)[(size_t)i * 8 + word];
  }
}
} // namespace

extern "C" {

int oakgpu_build_window_create(oakgpu_ctx *ctx, uint32_t max_records, oakgpu_build_window **out) {
  const char *fn = "oakgpu_build_window_create";
  if (max_records == 0) return fail(fn, "max_records == 0");
  if (max_records > 0x7FFFFFFFu) return fail(fn, "max_records above 2^31 - 1");
  if (!ctx || !out) return fail(fn, "null argument");
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  oakgpu_build_window *w = new oakgpu_build_window;
  w->max_records = max_records;
  oakgpu_build_corpus &c = w->corpus;
  c.ctx = ctx;
  c.n_files = 1;
  int rc = dev_alloc(w->buffer[0], (size_t)max_records * RECORD_BYTES);
  if (!rc) rc = dev_alloc(w->buffer[1], (size_t)max_records * RECORD_BYTES);
  if (!rc) rc = dev_alloc(c.file_first, 2);
  if (!rc) rc = dev_alloc(c.status, (size_t)max_records);
  if (!rc) rc = dev_alloc(c.counts, (size_t)bt::N_STATUS);
  if (!rc) rc = dev_alloc(w->totals, 2);
  if (!rc && hipMemsetAsync(c.file_first, 0, 8, stream) != hipSuccess) rc = fail(fn, "clearing the file table failed");
  if (rc) {
    oakgpu_build_window_destroy(w);
    return rc;
  }
  c.records = w->buffer[0];
  *out = w;
  return 0;
}

void oakgpu_build_window_destroy(oakgpu_build_window *w) {
  if (!w) return;
  oakgpu_build_corpus &c = w->corpus;
  if (c.ctx && oakgpu_ctx_enter(c.ctx) == 0) (void)hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(c.ctx));
  (void)hipFree(w->buffer[0]);
  (void)hipFree(w->buffer[1]);
  (void)hipFree(c.file_first);
  (void)hipFree(c.status);
  (void)hipFree(c.counts);
  (void)hipFree(c.picks);
  (void)hipFree(w->slot);
  (void)hipFree(w->totals);
  (void)hipFree(w->staging);
  delete w;
}

int oakgpu_build_window_append_dev(oakgpu_ctx *ctx, oakgpu_build_window *w, const uint8_t *records, const uint32_t *count, uint32_t max_count) {
  const char *fn = "oakgpu_build_window_append_dev";
  if (!ctx || !w || !records || !count) return fail(fn, "null argument");
  if (w->corpus.ctx != ctx) return fail(fn, "the window belongs to another context");
  if ((uintptr_t)records & 15) return fail(fn, "records must be 16-byte aligned");
  if (max_count == 0) return 0;
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  if (w->slot_capacity < max_count) { // (a launch on the stream may still read the old map)
    HIPCHK(hipStreamSynchronize(stream));
    (void)hipFree(w->slot);
    w->slot = nullptr;
    w->slot_capacity = 0;
    RC(dev_alloc(w->slot, (size_t)max_count));
    w->slot_capacity = max_count;
  }
  hipLaunchKernelGGL(k_window_mark, dim3(1), dim3(MARK_BLOCK), 0, stream, records, count, max_count, w->slot, w->totals);
  HIPCHK(hipGetLastError());
  uint32_t totals[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(totals, w->totals, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream)); // the append's one wait: the records held from here on are the host's to know
  const uint32_t accepted = totals[0], batch = totals[0] + totals[1];
  w->rejected += totals[1];
  if (batch > max_count) return fail(fn, "the batch's totals exceed max_count (internal error)");
  if (accepted == 0) return 0;
  oakgpu_build_corpus &c = w->corpus;
  const uint32_t M = w->max_records, held = c.n_records;
  const uint32_t taken = accepted < M ? accepted : M;                 // a batch larger than the window keeps its newest
  const uint32_t kept = held < M - taken ? held : M - taken;          // the oldest records leave first
  const bool in_place = kept == held;
  MoveArgs a{};
  a.from = w->buffer[w->cur];
  a.to = in_place ? w->buffer[w->cur] : w->buffer[w->cur ^ 1];
  a.first_kept = held - kept;
  a.kept = in_place ? 0 : kept;
  a.incoming = records; a.slot = w->slot; a.batch = batch;
  a.first_taken = accepted - taken;
  a.base = kept;
  a.file_first = c.file_first;
  a.held = kept + taken;
  const uint32_t items = a.kept + batch;
  hipLaunchKernelGGL(k_window_move, dim3((items + 31) / 32), dim3(256), 0, stream, a);
  HIPCHK(hipGetLastError());
  if (!in_place) w->cur ^= 1;
  c.records = w->buffer[w->cur];
  c.n_records = kept + taken;
  c.scan_launched = c.scanned = false;
  w->appended += accepted;
  w->evicted += (uint64_t)(held - kept) + (accepted - taken);
  return 0;
}

int oakgpu_build_window_append(oakgpu_ctx *ctx, oakgpu_build_window *w, const uint8_t *bytes, size_t len) {
  const char *fn = "oakgpu_build_window_append";
  if (!ctx || !w || (!bytes && len)) return fail(fn, "null argument");
  if (w->corpus.ctx != ctx) return fail(fn, "the window belongs to another context");
  if (len % RECORD_BYTES) return fail(fn, std::to_string(len) + " bytes is not a multiple of 128");
  if (len / RECORD_BYTES > 0x7FFFFFFFull) return fail(fn, "more than 2^31 - 1 records");
  if (len == 0) return 0;
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  if (w->staging_capacity < len + 16) {
    HIPCHK(hipStreamSynchronize(stream));
    (void)hipFree(w->staging);
    w->staging = nullptr;
    w->staging_capacity = 0;
    RC(dev_alloc(w->staging, len + 16));
    w->staging_capacity = len + 16;
  }
  const uint32_t n = (uint32_t)(len / RECORD_BYTES);
  HIPCHK(hipMemcpyAsync(w->staging, bytes, len, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(w->staging + len, &n, 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream)); // (`n` and the caller's bytes are pageable)
  return oakgpu_build_window_append_dev(ctx, w, w->staging, (const uint32_t *)(w->staging + len), n);
}

oakgpu_build_corpus *oakgpu_build_window_corpus(oakgpu_build_window *w) { return w ? &w->corpus : nullptr; }

int oakgpu_build_window_records(oakgpu_build_window *w, uint8_t *out, size_t capacity, size_t *bytes) {
  const char *fn = "oakgpu_build_window_records";
  if (!w) return fail(fn, "null argument");
  const size_t size = (size_t)w->corpus.n_records * RECORD_BYTES;
  if (bytes) *bytes = size;
  if (!out) return 0; // (the size query)
  if (capacity < size) return fail(fn, "buffer too small");
  RC(oakgpu_ctx_enter(w->corpus.ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(w->corpus.ctx);
  if (size) HIPCHK(hipMemcpyAsync(out, w->corpus.records, size, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_build_window_stats(const oakgpu_build_window *w, uint64_t out[4]) {
  if (!w || !out) return fail("oakgpu_build_window_stats", "null argument");
  out[0] = w->corpus.n_records; out[1] = w->appended; out[2] = w->evicted; out[3] = w->rejected;
  return 0;
}

} // extern "C"
