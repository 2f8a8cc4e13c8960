// tests/cpp_build_traj_check.cc -- the host form of oak_amd/csrc/build_traj.hpp in a stand-alone program (tests/test_build_traj_ref.py builds
// it once plain and once under the address and undefined-behaviour sanitizers and compares what it prints with the referee):
//   cpp_build_traj_check RECORDS      one line per 128-byte record of the file: status, the sum of the lists' lengths, a digest of the lists
// The walk runs with one thread and a visitor that writes every list into a row of exactly 339 entries on the heap, so a write past a row
// is the sanitizer's to see.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../oak_amd/csrc/build_traj.hpp"

namespace bt = oak_build_traj;

struct ListVisitor {
  uint32_t lengths = 0, digest = 0;
  bool leader() const { return true; }
  void sync() const {}
  void row(int32_t i, const bt::Bounds &b, const bt::Helper &h, uint32_t length, uint32_t place, uint32_t action) {
    std::vector<int16_t> cells(bt::MAX_ACTIONS, (int16_t)-1);
    bt::list_write(h, i, b, 0, 1, cells.data());
    cells[place] = cells[0];
    cells[0] = (int16_t)action;
    lengths += length;
    for (uint32_t k = 0; k < bt::MAX_ACTIONS; ++k) digest += (uint32_t)(i + 1) * (k + 1) * (uint32_t)(cells[k] + 1);
  }
};

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<uint8_t> record(bt::RECORD_BYTES);
  while (fread(record.data(), 1, bt::RECORD_BYTES, in) == bt::RECORD_BYTES) {
    const bt::Bounds b = bt::bounds_of(record.data());
    bt::Helper h;
    ListVisitor v;
    const uint8_t status = bt::walk(record.data(), b, h, v);
    if (status != bt::record_status(record.data())) return 3;
    if (status != bt::OK) v = ListVisitor{};
    printf("%u %u %u\n", (unsigned)status, v.lengths, v.digest);
  }
  fclose(in);
  return 0;
}
