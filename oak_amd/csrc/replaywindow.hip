// oak_amd/csrc/replaywindow.hip -- a corpus that self-play appends to on the device (the contract is in include/oakgpu.h).
//
// The window is a double buffer: an append classes the batch's slices, cuts the oldest records, and moves the survivors and the new
// records into the other buffer, each record at a 16-byte aligned offset; then the buffers change places.  Nothing of the window is read
// by the host: one summary and the batch's own frame counts and classes come back per append.
//   k_window_scan : one wave per slice of the batch: record_scan.hpp's rule through a 256-byte register window -> class, frames, bytes
//   k_window_cut  : one workgroup: newest first, game_rows.hpp's scan over records and bytes -> each record's rank from the end and the
//                   bytes behind it, and the summary (what survives, under both caps)
//   k_window_move : one wave per surviving record: its bytes to its aligned place in 16-byte stores, its row of the index arrays, and for
//                   a record the window already held its aligned battle and first request
//   (k_replay_gather over the new rows alone fills theirs)
//   k_window_pack : one wave per record: the records back to back, as a `.battle.data` file holds them
// There is no CPU fallback in this library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/oakgpu.h"
#include "oakgpu_internal.h"
#include "game_rows.hpp"
#include "record_scan.hpp"

namespace oak {
namespace rw {
using game_rows::scan_pass;
using game_rows::ScanPass;
using game_rows::NO_ROW;
using oak_scan::AppendSummary;

// byte i of a slice for a whole wave: 256 bytes at a time sit in the wave's registers, a dword per lane, and a byte is one shuffle.
// Every lane asks for the same i (the walk is wave-uniform), so the reload is uniform too.
struct WaveBytes {
  const uint8_t *p;
  uint64_t size, base;
  uint32_t word;
  __device__ __forceinline__ uint32_t operator()(size_t i) {
    if (i < base || i >= base + 256) {
      base = i & ~(uint64_t)255;
      const uint64_t at = base + 4 * (threadIdx.x & 63);
      word = 0;
      if (at + 4 <= size) __builtin_memcpy(&word, p + at, 4); // (a slice starts at any byte of the stream)
      else for (uint32_t b = 0; at + b < size; ++b) word |= (uint32_t)p[at + b] << (8 * b);
    }
    const uint32_t rel = (uint32_t)(i - base);
    return (__shfl(word, rel >> 2) >> (8 * (rel & 3))) & 0xFF;
  }
};

__global__ __launch_bounds__(256) void k_window_scan(const uint8_t *stream, const uint64_t *offsets, uint32_t n, uint8_t *kinds, uint16_t *frames, uint32_t *sizes) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const uint64_t lo = offsets[i], hi = offsets[i + 1];
  int kind = oak_scan::SLICE_REJECTED;
  uint16_t nf = 0;
  if (hi >= lo) {
    WaveBytes rd{stream + lo, hi - lo, ~(uint64_t)0, 0};
    kind = oak_scan::scan_slice(rd, hi - lo, &nf);
  }
  if ((threadIdx.x & 63) == 0) {
    kinds[i] = (uint8_t)kind;
    frames[i] = nf;
    sizes[i] = kind == oak_scan::SLICE_OK || kind == oak_scan::SLICE_MALFORMED ? (uint32_t)(hi - lo) : 0u;
  }
}

// What the cut leaves per source item (the batch's slices 0 .. n-1, then the window's records 0 .. n_old-1): its rank from the newest
// surviving record (NO_ROW: not in the new window), and the bytes of it and everything newer, packed and placed.
struct CutArrays {
  uint32_t *rank;
  uint64_t *bytes_incl, *placed_incl;
};

__global__ __launch_bounds__(1024) void k_window_cut(const uint8_t *kinds, const uint32_t *sizes, uint32_t n, const uint8_t *old_records, const uint64_t *old_offsets,
                                                     uint32_t n_old, uint32_t max_records, uint64_t max_bytes, CutArrays out, AppendSummary *summary) {
  __shared__ uint32_t wt32[16];
  __shared__ uint64_t wt64a[16], wt64b[16];
  __shared__ uint64_t last[2];
  if (threadIdx.x == 0) last[0] = last[1] = 0;
  uint32_t c_count = 0, accepted = 0, rejected = 0, kept = 0;
  uint64_t c_bytes = 0, c_placed = 0;
  bool stopped = false; // (uniform) an accepted record did not fit: nothing older does
  const uint32_t items = n + n_old;
  for (uint32_t part = 0; part < 2; ++part) { // the batch, newest first, then the window's own records, newest first
    const uint32_t count = part ? n_old : n;
    for (uint32_t base = 0; base < count; base += 1024) {
      const uint32_t j = base + threadIdx.x;
      const bool in = j < count;
      const uint32_t src = part ? n + (n_old - 1 - j) : n - 1 - j; // (read only when `in`)
      if (stopped) {
        if (in) out.rank[src] = NO_ROW;
        if (!part) {
          const uint32_t kind = in ? kinds[src] : 0;
          rejected += __syncthreads_count(kind == oak_scan::SLICE_REJECTED);
          accepted += __syncthreads_count(kind == oak_scan::SLICE_OK || kind == oak_scan::SLICE_MALFORMED);
        }
        continue;
      }
      uint32_t size = 0, kind = 0;
      if (in) {
        if (part) size = *(const uint32_t *)(old_records + old_offsets[n_old - 1 - j]); // (a placed record's length field is aligned)
        else { size = sizes[src]; kind = kinds[src]; }
      }
      const bool acc = size != 0;
      if (!part) rejected += __syncthreads_count(kind == oak_scan::SLICE_REJECTED);
      const ScanPass<uint32_t> sc = scan_pass<uint32_t>(acc ? 1u : 0u, wt32);
      const ScanPass<uint64_t> sb = scan_pass<uint64_t>((uint64_t)size, wt64a);
      const ScanPass<uint64_t> sp = scan_pass<uint64_t>(((uint64_t)size + 15) & ~(uint64_t)15, wt64b);
      const uint32_t rank = c_count + sc.before;
      const uint64_t bytes_incl = c_bytes + sb.before + size, placed_incl = c_placed + sp.before + ((size + 15ull) & ~15ull);
      const bool keep = acc && rank < max_records && bytes_incl <= max_bytes;
      const uint32_t kept_here = __syncthreads_count(keep);
      if (in) {
        out.rank[src] = keep ? rank : NO_ROW;
        out.bytes_incl[src] = bytes_incl;
        out.placed_incl[src] = placed_incl;
      }
      if (keep && sc.before == kept_here - 1) { last[0] = bytes_incl; last[1] = placed_incl; } // (the kept ones are the pass' first accepted ones)
      if (!part) accepted += sc.total;
      kept += kept_here;
      stopped = kept_here != sc.total;
      c_count += sc.total;
      c_bytes += sb.total;
      c_placed += sp.total;
    }
  }
  (void)items;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t kept_new = kept < accepted ? kept : accepted;
    *summary = AppendSummary{kept, kept - kept_new, accepted, kept_new, rejected, 0u, last[0], last[1]};
  }
}

struct MoveArgs {
  const uint8_t *stream;       // the batch
  const uint64_t *offsets;     // n + 1
  const uint8_t *kinds;        // n
  const uint16_t *b_frames;    // n
  uint32_t n;
  const uint8_t *old_records;  // the window as it was
  const uint64_t *old_offsets;
  const uint16_t *old_frames;
  const uint8_t *old_malformed, *old_aligned, *old_first;
  uint32_t n_old;
  CutArrays cut;
  const AppendSummary *summary;
  uint8_t *records;            // the window to be
  uint64_t *offsets_out, *packed_out;
  uint16_t *frames_out;
  uint8_t *malformed_out, *aligned_out, *first_out;
};

__global__ __launch_bounds__(256) void k_window_move(MoveArgs a) {
  const uint32_t item = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (item >= a.n + a.n_old) return;
  const uint32_t rank = a.cut.rank[item];
  if (rank == NO_ROW) return;
  const AppendSummary s = *a.summary;
  const uint32_t to = s.records - 1 - rank;
  const uint64_t at = s.placed - a.cut.placed_incl[item];
  const bool old = item >= a.n;
  const uint32_t r = old ? item - a.n : item;
  const uint8_t *src = old ? a.old_records + a.old_offsets[r] : a.stream + a.offsets[r];
  const uint32_t size = old ? *(const uint32_t *)src : (uint32_t)(a.offsets[r + 1] - a.offsets[r]);
  uint4 *dst = (uint4 *)(a.records + at);
  for (uint32_t c = lane; c < (size + 15) / 16; c += 64) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (16 * c + 16 <= size) {
      if (old) v = ((const uint4 *)src)[c];
      else __builtin_memcpy(&v, src + 16 * (size_t)c, 16);
    } else { // the record's last bytes, zeros behind them
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t b = 16 * c; b < size; ++b) w[(b >> 2) & 3] |= (uint32_t)src[b] << (8 * (b & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    dst[c] = v;
  }
  if (old && lane < 24) ((uint4 *)(a.aligned_out + (size_t)to * 384))[lane] = ((const uint4 *)(a.old_aligned + (size_t)r * 384))[lane];
  if (lane == 0) {
    a.offsets_out[to] = at;
    a.packed_out[to] = s.bytes - a.cut.bytes_incl[item];
    a.frames_out[to] = old ? a.old_frames[r] : a.b_frames[r];
    a.malformed_out[to] = old ? a.old_malformed[r] : (uint8_t)(a.kinds[r] == oak_scan::SLICE_MALFORMED);
    if (old) a.first_out[to] = a.old_first[r];
  }
}

__global__ __launch_bounds__(256) void k_window_pack(const uint8_t *records, const uint64_t *offsets, const uint64_t *packed, uint32_t n, uint8_t *out) {
  const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= n) return;
  const uint8_t *src = records + offsets[r];
  const uint32_t size = *(const uint32_t *)src;
  uint8_t *dst = out + packed[r];
  const uint32_t head = std::min(size, (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3)), words = (size - head) / 4, tail = head + 4 * words;
  if (lane < head) dst[lane] = src[lane];
  for (uint32_t w = lane; w < words; w += 64) {
    uint32_t v;
    __builtin_memcpy(&v, src + head + 4 * (size_t)w, 4);
    *(uint32_t *)(dst + head + 4 * (size_t)w) = v;
  }
  if (tail + lane < size) dst[tail + lane] = src[tail + lane];
}

} // namespace rw
} // namespace oak

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {

struct Window {
  uint32_t max_records = 0;
  uint64_t max_bytes = 0;
  oak_scan::WindowBook book;
  // the front buffers are the corpus' own arrays (+ packed); these are the other half
  uint8_t *records = nullptr, *malformed = nullptr, *aligned = nullptr, *first = nullptr;
  uint64_t *offsets = nullptr, *packed = nullptr, *front_packed = nullptr;
  uint16_t *frames = nullptr;
  uint64_t rec_cap = 0, front_rec_cap = 0;
  uint32_t idx_cap = 0, front_idx_cap = 0;
  uint8_t *tmp = nullptr, *stage = nullptr, *pack = nullptr; // grow-only: the append's arrays, a host batch on the device, records() for the host
  size_t tmp_cap = 0, stage_cap = 0, pack_cap = 0;
};

void window_free(void *p) { // (the stream is idle)
  Window *w = (Window *)p;
  for (void *q : {(void *)w->records, (void *)w->malformed, (void *)w->aligned, (void *)w->first, (void *)w->offsets, (void *)w->packed, (void *)w->front_packed,
                  (void *)w->frames, (void *)w->tmp, (void *)w->stage, (void *)w->pack})
    if (q) (void)hipFree(q);
  delete w;
}

int grow_bytes(oakgpu_ctx *c, uint8_t *&p, size_t &cap, size_t want) { // grow-only; an earlier call's kernels may still read the old block
  if (want <= cap && p) return 0;
  HIPCHK(hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(c)));
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  want = std::max<size_t>(want + want / 2, 256);
  if (dev_alloc(p, want)) return -1;
  cap = want;
  return 0;
}

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// the other half, large enough for `records` records in `placed` bytes (the stream is idle: the append has just waited for it)
int reserve_back(Window *w, uint32_t records, uint64_t placed) {
  if (placed > w->rec_cap || !w->records) {
    if (w->records) (void)hipFree(w->records);
    w->records = nullptr;
    w->rec_cap = 0;
    const uint64_t limit = up16(w->max_bytes) + 16ull * w->max_records; // what a full window can take
    const uint64_t want = std::max<uint64_t>(std::min<uint64_t>(placed + placed / 2, limit), std::max<uint64_t>(placed, 256));
    if (dev_alloc(w->records, want)) return -1;
    w->rec_cap = want;
  }
  if (records > w->idx_cap || !w->offsets) {
    for (void **q : {(void **)&w->malformed, (void **)&w->aligned, (void **)&w->first, (void **)&w->offsets, (void **)&w->packed, (void **)&w->frames}) {
      if (*q) (void)hipFree(*q);
      *q = nullptr;
    }
    w->idx_cap = 0;
    const uint32_t want = std::max<uint32_t>((uint32_t)std::min<uint64_t>((uint64_t)records + records / 2, w->max_records), std::max(records, 16u));
    if (dev_alloc(w->malformed, want) || dev_alloc(w->aligned, (size_t)want * 384) || dev_alloc(w->first, want) || dev_alloc(w->offsets, want) ||
        dev_alloc(w->packed, want) || dev_alloc(w->frames, want))
      return -1;
    w->idx_cap = want;
  }
  return 0;
}

Window *window_of(const oakgpu_corpus *k) { return k && k->window_free == window_free ? (Window *)k->window : nullptr; }

int append_dev(oakgpu_ctx *c, oakgpu_corpus *k, Window *w, const uint8_t *stream, const uint64_t *offsets, uint32_t n) {
  using namespace oak::rw;
  hipStream_t st = (hipStream_t)oakgpu_ctx_stream(c);
  const uint32_t n_old = k->n;
  const size_t items = (size_t)n + n_old;
  // the append's arrays in one block: kinds, frames, sizes of the batch; rank, bytes, placed per item; the summary; the gather's scratch
  const size_t o_kinds = 0, o_frames = up16(n), o_sizes = o_frames + up16((size_t)n * 2), o_rank = o_sizes + up16((size_t)n * 4), o_bytes = o_rank + up16(items * 4),
               o_placed = o_bytes + up16(items * 8), o_summary = o_placed + up16(items * 8), o_scratch = o_summary + up16(sizeof(AppendSummary)),
               total = o_scratch + up16((size_t)n * 8);
  if (int rc = grow_bytes(c, w->tmp, w->tmp_cap, total)) return rc;
  uint8_t *kinds = w->tmp + o_kinds;
  uint16_t *b_frames = (uint16_t *)(w->tmp + o_frames);
  uint32_t *sizes = (uint32_t *)(w->tmp + o_sizes);
  const CutArrays cut{(uint32_t *)(w->tmp + o_rank), (uint64_t *)(w->tmp + o_bytes), (uint64_t *)(w->tmp + o_placed)};
  AppendSummary *d_summary = (AppendSummary *)(w->tmp + o_summary);
  hipLaunchKernelGGL(k_window_scan, dim3((n + 3) / 4), dim3(256), 0, st, stream, offsets, n, kinds, b_frames, sizes);
  hipLaunchKernelGGL(k_window_cut, dim3(1), dim3(1024), 0, st, kinds, sizes, n, k->records, k->offsets, n_old, w->max_records, w->max_bytes, cut, d_summary);
  HIPCHK(hipGetLastError());
  // the append's one wait: the summary and the batch's own frames and classes
  AppendSummary s{};
  std::vector<uint8_t> h_kinds(n);
  std::vector<uint16_t> h_frames(n);
  HIPCHK(hipMemcpyAsync(&s, d_summary, sizeof s, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_kinds.data(), kinds, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_frames.data(), b_frames, (size_t)n * 2, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (s.accepted == 0) { // nothing joins, so nothing leaves: the caps held before
    if (!w->book.apply(s, h_kinds.data(), h_frames.data(), n)) return oakgpu_fail_msg("oakgpu_corpus_append: the device's summary does not fit the window (internal)");
    return 0;
  }
  if (s.placed > up16(w->max_bytes) + 16ull * w->max_records || s.records > w->max_records || s.bytes > w->max_bytes)
    return oakgpu_fail_msg("oakgpu_corpus_append: the device's summary exceeds the window (internal)");
  oak_scan::WindowBook next = w->book;
  if (!next.apply(s, h_kinds.data(), h_frames.data(), n)) return oakgpu_fail_msg("oakgpu_corpus_append: the device's summary does not fit the window (internal)");
  if (int rc = reserve_back(w, s.records, s.placed)) return rc;
  oakgpu_corpus_drop_caches(k); // (the stream is idle) the sampler's lists and the evaluation's prefix sums are the old window's
  const MoveArgs ma{stream, offsets, kinds, b_frames, n, k->records, k->offsets, k->frames, k->malformed, k->aligned, k->first, n_old, cut, d_summary,
                    w->records, w->offsets, w->packed, w->frames, w->malformed, w->aligned, w->first};
  hipLaunchKernelGGL(k_window_move, dim3((uint32_t)((items + 3) / 4)), dim3(256), 0, st, ma);
  HIPCHK(hipGetLastError());
  if (s.kept_new)
    if (int rc = oakgpu_replay_gather_dev(c, w->records, w->offsets + s.kept_old, w->malformed + s.kept_old, s.kept_new, w->aligned + (size_t)s.kept_old * 384,
                                          w->first + s.kept_old, (uint32_t *)(w->tmp + o_scratch)))
      return rc;
  // the halves change places
  std::swap(k->records, w->records);
  std::swap(k->offsets, w->offsets);
  std::swap(k->frames, w->frames);
  std::swap(k->malformed, w->malformed);
  std::swap(k->aligned, w->aligned);
  std::swap(k->first, w->first);
  std::swap(w->front_packed, w->packed);
  std::swap(w->front_rec_cap, w->rec_cap);
  std::swap(w->front_idx_cap, w->idx_cap);
  w->book = std::move(next);
  k->n = s.records;
  k->h_frames = w->book.frames;
  k->h_malformed = w->book.malformed;
  k->info.records = s.records;
  k->info.malformed = w->book.n_malformed;
  k->info.frames = w->book.n_frames;
  k->info.stopped_at = (size_t)s.bytes;
  return 0;
}

int check_window(const char *who, oakgpu_ctx *c, const oakgpu_corpus *k, Window **w) {
  static char msg[160];
  if (!c || !k) { snprintf(msg, sizeof msg, "%s: null ctx or corpus", who); return oakgpu_fail_msg(msg); }
  if (!(*w = window_of(k))) { snprintf(msg, sizeof msg, "%s: corpus was not made by oakgpu_corpus_create_window", who); return oakgpu_fail_msg(msg); }
  if (k->ctx != c) { snprintf(msg, sizeof msg, "%s: corpus belongs to another ctx", who); return oakgpu_fail_msg(msg); }
  return 0;
}

} // namespace

extern "C" {

int oakgpu_corpus_window_check(uint32_t max_records, size_t max_bytes) {
  if (max_records == 0) return oakgpu_fail_msg("oakgpu_corpus_create_window: max_records must be at least 1");
  if (max_bytes < oak_scan::FIXED_BYTES) return oakgpu_fail_msg("oakgpu_corpus_create_window: max_bytes is below one minimal record (391 bytes)");
  return 0;
}

int oakgpu_corpus_create_window(oakgpu_ctx *c, uint32_t max_records, size_t max_bytes, oakgpu_corpus **out) {
  if (!c || !out) return oakgpu_fail_msg("oakgpu_corpus_create_window: null ctx or out");
  *out = nullptr;
  if (int rc = oakgpu_corpus_window_check(max_records, max_bytes)) return rc;
  oakgpu_corpus *k = nullptr;
  if (int rc = oakgpu_corpus_create(c, nullptr, 0, &k)) return rc; // the empty corpus: its workspace and the device's wave count
  Window *w = new Window;
  w->max_records = max_records;
  w->max_bytes = max_bytes;
  k->window = w;
  k->window_free = window_free;
  *out = k;
  return 0;
}

int oakgpu_corpus_append_dev(oakgpu_ctx *c, oakgpu_corpus *k, const uint8_t *stream, const uint64_t *offsets, uint32_t n) {
  Window *w = nullptr;
  if (int rc = check_window("oakgpu_corpus_append_dev", c, k, &w)) return rc;
  if (n == 0) { ++w->book.appends; return 0; }
  if (!offsets || ((uintptr_t)offsets & 7)) return oakgpu_fail_msg("oakgpu_corpus_append_dev: offsets must be an 8-byte aligned device array of n + 1 entries");
  if (!stream) return oakgpu_fail_msg("oakgpu_corpus_append_dev: null stream");
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  return append_dev(c, k, w, stream, offsets, n);
}

int oakgpu_corpus_append(oakgpu_ctx *c, oakgpu_corpus *k, const uint8_t *buffer, size_t size) {
  Window *w = nullptr;
  if (int rc = check_window("oakgpu_corpus_append", c, k, &w)) return rc;
  if (!buffer && size) return oakgpu_fail_msg("oakgpu_corpus_append: null buffer");
  std::vector<uint64_t> offs{0};
  size_t pos = 0;
  while (pos < size && offs.size() <= 0xFFFFFFFFull) { // the length walk of oakgpu_replay_index: bytes behind an untrusted length are left out
    uint32_t total = 0;
    uint16_t nf = 0;
    const char *msg = nullptr;
    if (oakgpu_record_scan_length(buffer + pos, size - pos, &total, &nf, &msg) != OAKGPU_RECORD_OK) break;
    pos += total;
    offs.push_back(pos);
  }
  const uint32_t n = (uint32_t)(offs.size() - 1);
  if (n == 0) { ++w->book.appends; return 0; }
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  hipStream_t st = (hipStream_t)oakgpu_ctx_stream(c);
  const size_t o_offs = up16(pos);
  if (int rc = grow_bytes(c, w->stage, w->stage_cap, o_offs + offs.size() * 8)) return rc;
  HIPCHK(hipMemcpyAsync(w->stage, buffer, pos, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(w->stage + o_offs, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, st));
  const int rc = append_dev(c, k, w, w->stage, (const uint64_t *)(w->stage + o_offs), n);
  if (rc) (void)hipStreamSynchronize(st); // (a failure in front of the append's wait: the uploads may still read the caller's bytes)
  return rc;
}

int oakgpu_corpus_window_stats(const oakgpu_corpus *k, uint64_t out[6]) {
  const Window *w = window_of(k);
  if (!k || !out) return oakgpu_fail_msg("oakgpu_corpus_window_stats: null corpus or out");
  if (!w) return oakgpu_fail_msg("oakgpu_corpus_window_stats: corpus was not made by oakgpu_corpus_create_window");
  out[0] = k->n; out[1] = w->book.bytes; out[2] = w->book.appended; out[3] = w->book.evicted; out[4] = w->book.rejected; out[5] = w->book.appends;
  return 0;
}

int oakgpu_corpus_records(oakgpu_ctx *c, oakgpu_corpus *k, uint8_t *out, size_t capacity, size_t *bytes, int to_device) {
  Window *w = nullptr;
  if (int rc = check_window("oakgpu_corpus_records", c, k, &w)) return rc;
  const size_t total = (size_t)w->book.bytes;
  if (bytes) *bytes = total;
  if (!out) return 0; // the size alone
  if (capacity < total) return oakgpu_fail_msg("oakgpu_corpus_records: capacity is below the window's bytes");
  if (total == 0) return 0;
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  hipStream_t st = (hipStream_t)oakgpu_ctx_stream(c);
  uint8_t *dst = out;
  if (!to_device) {
    if (int rc = grow_bytes(c, w->pack, w->pack_cap, total)) return rc;
    dst = w->pack;
  }
  hipLaunchKernelGGL(oak::rw::k_window_pack, dim3((k->n + 3) / 4), dim3(256), 0, st, k->records, k->offsets, w->front_packed, k->n, dst);
  HIPCHK(hipGetLastError());
  if (!to_device) {
    HIPCHK(hipMemcpyAsync(out, dst, total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return 0;
}

// Diagnostic (no GPU involved): record_scan.hpp's slice rule on host bytes, the text k_window_scan compiles.
int oakgpu_window_scan_host(const uint8_t *stream, const uint64_t *offsets, uint32_t n, uint8_t *kinds, uint16_t *frames) {
  if ((!stream && n) || !offsets || !kinds || !frames) return oakgpu_fail_msg("oakgpu_window_scan_host: null argument");
  for (uint32_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) { kinds[i] = oak_scan::SLICE_REJECTED; frames[i] = 0; continue; }
    oak_scan::HostBytes rd{stream + offsets[i]};
    kinds[i] = (uint8_t)oak_scan::scan_slice(rd, offsets[i + 1] - offsets[i], &frames[i]);
  }
  return 0;
}

} // extern "C"
