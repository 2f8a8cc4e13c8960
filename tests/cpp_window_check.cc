// tests/cpp_window_check.cc -- the host form of oak_amd/csrc/record_scan.hpp, stand-alone (no GPU, no library): the slice rule of a replay
// window's append and the window's host bookkeeping, on a file of slices that tests/test_replay_window_ref.py writes (cut and damaged
// records among them).  Built plain and under -fsanitize=address,undefined.
//   usage: cpp_window_check FILE MAX_RECORDS MAX_BYTES BATCH
//   FILE : u32 n, u64 offsets[n + 1], then the stream bytes.  Every slice is copied to a heap block of exactly its size before it is
//          scanned, so a read past a slice's end is a sanitizer report.
//   out  : one line "kind frames" per slice; then, after appending the slices BATCH at a time to a window of the two caps,
//          "records malformed frames bytes appended evicted rejected appends"; then "refused K" for K summaries the book must refuse.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <vector>

#include "../oak_amd/csrc/record_scan.hpp"

int main(int argc, char **argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s FILE MAX_RECORDS MAX_BYTES BATCH\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  std::vector<uint64_t> offsets((size_t)n + 1);
  if (fread(offsets.data(), 8, offsets.size(), f) != offsets.size()) return 2;
  std::vector<uint8_t> stream((size_t)offsets[n]);
  if (!stream.empty() && fread(stream.data(), 1, stream.size(), f) != stream.size()) return 2;
  fclose(f);
  const uint32_t max_records = (uint32_t)strtoul(argv[2], nullptr, 10), batch = (uint32_t)strtoul(argv[4], nullptr, 10);
  const uint64_t max_bytes = strtoull(argv[3], nullptr, 10);

  std::vector<uint8_t> kinds(n);
  std::vector<uint16_t> frames(n);
  std::vector<uint32_t> sizes(n);
  for (uint32_t i = 0; i < n; ++i) {
    const size_t size = (size_t)(offsets[i + 1] - offsets[i]);
    uint8_t *exact = (uint8_t *)malloc(size ? size : 1);
    if (size) memcpy(exact, stream.data() + offsets[i], size);
    oak_scan::HostBytes rd{exact};
    kinds[i] = (uint8_t)oak_scan::scan_slice(rd, size, &frames[i]);
    // the two scans a record goes through on the host agree with the slice rule
    uint32_t total = 0;
    uint16_t nf = 0;
    int why = 0;
    const int whole = oak_scan::scan(rd, size, &total, &nf, &why);
    if (kinds[i] == oak_scan::SLICE_OK && (whole != oak_scan::RECORD_OK || total != size || nf != frames[i])) return 3;
    if (kinds[i] == oak_scan::SLICE_MALFORMED && (whole != oak_scan::RECORD_MALFORMED || !oak_scan::why_message(why)[0])) return 3;
    if (size && size < oak_scan::FIXED_BYTES && (whole != oak_scan::RECORD_STOP || kinds[i] != oak_scan::SLICE_REJECTED)) return 3;
    free(exact);
    sizes[i] = kinds[i] == oak_scan::SLICE_OK || kinds[i] == oak_scan::SLICE_MALFORMED ? (uint32_t)size : 0u;
    printf("%u %u\n", (unsigned)kinds[i], (unsigned)frames[i]);
  }

  // the window: the cut is made here item by item (the device makes it with a scan), the book follows the summaries
  oak_scan::WindowBook book;
  std::deque<uint32_t> held; // sizes of the records in the window
  uint32_t refused = 0;
  for (uint32_t lo = 0; lo < n || lo == 0; lo += batch ? batch : 1) {
    const uint32_t hi = lo + batch < n ? lo + batch : n, count = hi - lo;
    oak_scan::AppendSummary s{};
    std::deque<uint32_t> joined = held;
    for (uint32_t i = lo; i < hi; ++i) {
      if (sizes[i]) { joined.push_back(sizes[i]); ++s.accepted; }
      s.rejected += kinds[i] == oak_scan::SLICE_REJECTED;
    }
    uint32_t keep = 0;
    uint64_t bytes = 0, placed = 0;
    for (auto it = joined.rbegin(); it != joined.rend(); ++it) {
      if (keep + 1 > max_records || bytes + *it > max_bytes) break;
      ++keep;
      bytes += *it;
      placed += (*it + 15ull) & ~15ull;
    }
    s.records = keep;
    s.kept_new = keep < s.accepted ? keep : s.accepted;
    s.kept_old = keep - s.kept_new;
    s.bytes = bytes;
    s.placed = placed;
    // summaries that cannot belong to this book and batch leave it as it is
    const oak_scan::WindowBook before = book;
    oak_scan::AppendSummary bad = s;
    bad.kept_old = (uint32_t)held.size() + 1;
    bad.records = bad.kept_old + bad.kept_new;
    refused += !book.apply(bad, kinds.data() + lo, frames.data() + lo, count);
    bad = s;
    bad.accepted += 1;
    refused += !book.apply(bad, kinds.data() + lo, frames.data() + lo, count);
    if (book.frames != before.frames || book.appends != before.appends) return 4;
    if (!book.apply(s, kinds.data() + lo, frames.data() + lo, count)) return 5;
    while (joined.size() > keep) joined.pop_front();
    held.swap(joined);
    if (book.frames.size() != held.size() || book.bytes != bytes) return 6;
    if (n == 0) break;
  }
  printf("%zu %u %llu %llu %llu %llu %llu %llu\n", book.frames.size(), book.n_malformed, (unsigned long long)book.n_frames, (unsigned long long)book.bytes,
         (unsigned long long)book.appended, (unsigned long long)book.evicted, (unsigned long long)book.rejected, (unsigned long long)book.appends);
  printf("refused %u\n", refused);
  return 0;
}
