// oak_amd/csrc/record_scan.hpp -- the checks of CompressedFrames::read (train/battle/compressed-frame.h:224-243) on one `.battle.data`
// record, one text for the host (selfplay.hip: oakgpu_frames_read, oakgpu_replay_index) and the device (replaywindow.hip: a wave per
// appended record), and the host bookkeeping of a replay window.  The record is read through `rd(i)`, byte i of the buffer: a plain
// pointer on the host, a wave's 256-byte register window on the device.  No HIP header is needed to compile the host form.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define OAK_SCAN_HD __host__ __device__ __forceinline__
#else
#define OAK_SCAN_HD inline
#endif

namespace oak_scan {

enum Kind { RECORD_OK = 0, RECORD_MALFORMED = 1, RECORD_STOP = 2 }; // (oakgpu_internal.h's OAKGPU_RECORD_* carry the same values)
enum Why { WHY_NONE = 0, WHY_TRUNCATED_RECORD, WHY_LENGTH_RANGE, WHY_TRUNCATED_UPDATE, WHY_MALFORMED_UPDATE, WHY_FRAME_COUNT };
constexpr uint32_t FIXED_BYTES = 4 + 2 + 384 + 1; // u32 length, u16 frame count, the battle, the result byte

OAK_SCAN_HD const char *why_message(int why) { // oakgpu_frames_read's messages
  switch (why) {
    case WHY_TRUNCATED_RECORD: return "oakgpu_frames_read: truncated record";
    case WHY_LENGTH_RANGE: return "oakgpu_frames_read: record length out of range";
    case WHY_TRUNCATED_UPDATE: return "oakgpu_frames_read: truncated update";
    case WHY_MALFORMED_UPDATE: return "oakgpu_frames_read: malformed update";
    case WHY_FRAME_COUNT: return "oakgpu_frames_read: frame count does not match the record";
    default: return "";
  }
}

struct HostBytes {
  const uint8_t *p;
  OAK_SCAN_HD uint32_t operator()(size_t i) const { return p[i]; }
};

OAK_SCAN_HD uint32_t update_bytes(uint32_t m, uint32_t n) { return 1 + 2 + 4 + 2 + 2 + 4 * (m + n); } // (selfplay_pick.hpp's, without its includes)

// The header alone.  RECORD_STOP: the length field cannot be trusted -- a header cut short, or a length below the fixed part or past
// `size` -- so nothing behind this point can be found.
template <class Read>
OAK_SCAN_HD int scan_length(Read &rd, size_t size, uint32_t *total, uint16_t *n_frames, int *why) {
  if (size < FIXED_BYTES) { *why = WHY_TRUNCATED_RECORD; return RECORD_STOP; }
  *total = rd(0) | (rd(1) << 8) | (rd(2) << 16) | (rd(3) << 24);
  *n_frames = (uint16_t)(rd(4) | (rd(5) << 8));
  if (*total > size || *total < FIXED_BYTES) { *why = WHY_LENGTH_RANGE; return RECORD_STOP; }
  *why = WHY_NONE;
  return RECORD_OK;
}

// The updates of a record whose header passed scan_length.  RECORD_MALFORMED: damaged inside its own length (an m or n nibble above
// 8, an update past the record's end, a frame count that disagrees with the header).
template <class Read>
OAK_SCAN_HD int scan_updates(Read &rd, uint32_t total, uint16_t n_frames, int *why) {
  uint32_t p = FIXED_BYTES, n_read = 0;
  while (p < total) {
    if (total - p < 3) { *why = WHY_TRUNCATED_UPDATE; return RECORD_MALFORMED; }
    const uint32_t mn = rd(p), m = (mn & 15) + 1, n = (mn >> 4) + 1;
    if (m > 9 || n > 9 || total - p < update_bytes(m, n)) { *why = WHY_MALFORMED_UPDATE; return RECORD_MALFORMED; }
    p += update_bytes(m, n);
    ++n_read;
  }
  if (n_read != n_frames) { *why = WHY_FRAME_COUNT; return RECORD_MALFORMED; }
  *why = WHY_NONE;
  return RECORD_OK;
}

template <class Read>
OAK_SCAN_HD int scan(Read &rd, size_t size, uint32_t *total, uint16_t *n_frames, int *why) {
  if (const int kind = scan_length(rd, size, total, n_frames, why)) return kind;
  return scan_updates(rd, *total, *n_frames, why);
}

// One slice of an appended batch, bytes 0 .. size-1 of `rd`.  DROPPED: zero bytes (a dropped game).  REJECTED: the length field is not
// the slice (where the host's walk would stop, or would find another boundary than the caller's).  Else the record joins the window,
// MALFORMED when it is damaged inside its own length.
enum Slice { SLICE_DROPPED = 0, SLICE_OK = 1, SLICE_MALFORMED = 2, SLICE_REJECTED = 3 };
template <class Read>
OAK_SCAN_HD int scan_slice(Read &rd, uint64_t size, uint16_t *n_frames) {
  *n_frames = 0;
  if (size == 0) return SLICE_DROPPED;
  uint32_t total = 0;
  int why = 0;
  if (size > 0xFFFFFFFFull || scan_length(rd, (size_t)size, &total, n_frames, &why) != RECORD_OK || total != size) { *n_frames = 0; return SLICE_REJECTED; }
  return scan_updates(rd, total, *n_frames, &why) == RECORD_OK ? SLICE_OK : SLICE_MALFORMED;
}

// ---- the host's side of a replay window: the surviving records' frame counts and malformed flags in arrival order, the corpus
// totals and the lifetime counters, advanced by what one append's device pass reports.
struct AppendSummary { // written by k_window_cut, read once per append
  uint32_t records;    // the window after the append
  uint32_t kept_old;   // how many of the records it held before are still in it (the newest ones)
  uint32_t accepted;   // slices of the batch that are records (OK or MALFORMED)
  uint32_t kept_new;   // how many of those are in the window (the newest ones)
  uint32_t rejected;   // slices refused for their length field
  uint32_t pad;
  uint64_t bytes;      // the surviving records' bytes
  uint64_t placed;     // the same, each record rounded up to 16 bytes
};

struct WindowBook {
  std::vector<uint16_t> frames;
  std::vector<uint8_t> malformed;
  uint32_t n_malformed = 0;
  uint64_t n_frames = 0, bytes = 0;
  uint64_t appended = 0, evicted = 0, rejected = 0, appends = 0;

  // kinds / batch_frames: the batch's n slices as scan_slice classed them.  false when the summary cannot belong to this book and batch
  // (nothing is changed then).
  bool apply(const AppendSummary &s, const uint8_t *kinds, const uint16_t *batch_frames, uint32_t n) {
    uint32_t accepted = 0, rejected = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (kinds[i] > SLICE_REJECTED) return false;
      accepted += kinds[i] == SLICE_OK || kinds[i] == SLICE_MALFORMED;
      rejected += kinds[i] == SLICE_REJECTED;
    }
    if (s.accepted != accepted || s.rejected != rejected || s.kept_old > frames.size() || s.kept_new > accepted ||
        (uint64_t)s.kept_old + s.kept_new != s.records || (s.kept_new < accepted && s.kept_old != 0))
      return false;
    const size_t drop = frames.size() - s.kept_old;
    for (size_t r = 0; r < drop; ++r) {
      if (malformed[r]) --n_malformed;
      else n_frames -= frames[r];
    }
    frames.erase(frames.begin(), frames.begin() + drop);
    malformed.erase(malformed.begin(), malformed.begin() + drop);
    uint32_t skip = accepted - s.kept_new;
    for (uint32_t i = 0; i < n; ++i) {
      if (kinds[i] != SLICE_OK && kinds[i] != SLICE_MALFORMED) continue;
      if (skip) { --skip; continue; }
      const bool bad = kinds[i] == SLICE_MALFORMED;
      frames.push_back(batch_frames[i]);
      malformed.push_back(bad ? 1 : 0);
      if (bad) ++n_malformed;
      else n_frames += batch_frames[i];
    }
    bytes = s.bytes;
    appended += accepted;
    evicted += drop + (accepted - s.kept_new);
    this->rejected += rejected;
    ++appends;
    return true;
  }
};

} // namespace oak_scan
