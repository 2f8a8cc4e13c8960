// oak_amd/csrc/build_corpus.hpp -- the `.build.data` corpus as its two owners see it: buildtraj.hip (oakgpu_build_corpus_create: records
// fixed at creation, one or more files) and buildwindow.hip (oakgpu_build_window: ONE file whose records come and go with self-play).
// Every corpus call reads the records through this struct alone, so a window's corpus serves them unchanged.
#pragma once
#include <stdint.h>

#include "../../include/oakgpu.h"
#include "build_traj.hpp"

struct oakgpu_build_corpus {
  oakgpu_ctx *ctx = nullptr;
  uint32_t n_records = 0, n_files = 0;
  uint8_t *records = nullptr;     // n_records x 128 bytes
  uint32_t *file_first = nullptr; // n_files + 1: the first record of each file
  uint8_t *status = nullptr;      // n_records, filled by the scan
  uint32_t *counts = nullptr;     // N_STATUS words, filled by the scan
  bool scan_launched = false, scanned = false;
  uint32_t h_counts[oak_build_traj::N_STATUS] = {};
  uint32_t capacity = 0; // picks of a sample call: grow-only
  uint32_t *picks = nullptr;
};
