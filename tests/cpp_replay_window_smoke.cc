// OakGPU::ReplayWindow (include/oakgpu.hpp): two appends of host bytes to a window of four records, a sample from it and from a FrameCorpus
// made of its records, and a saved file; the outputs go to a file that tests/test_gpu_replay_window_cpp.py compares with oak_amd.train's.
// usage: cpp_replay_window_smoke FIRST SECOND OUT SAVED.  Without a GPU it only links.
#include <cstdio>
#include <cstdlib>
#include <oakgpu.hpp>

static std::vector<uint8_t> slurp(const char *path) {
  std::vector<uint8_t> out;
  if (FILE *f = std::fopen(path, "rb")) {
    uint8_t buf[4096];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + k);
    std::fclose(f);
  }
  return out;
}
template <class T> static void dump(FILE *f, const std::vector<T> &v) { std::fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv) {
  if (oakgpu_device_count() == 0 || argc < 5) { std::puts("no gpu: link check only"); return 0; }
  OakGPU::Context ctx{0};
  OakGPU::ReplayWindow window{ctx, 4, size_t{1} << 30};
  window.append(slurp(argv[1]));
  const OakGPU::ReplayWindow::Stats st = window.append(slurp(argv[2]));
  const std::vector<uint8_t> records = window.records();
  OakGPU::FrameCorpus corpus{ctx, records};
  OakGPU::EncodedFrames a{33}, b{33};
  if (window.sample(a, 77) != corpus.sample(b, 77)) return 3;
  if (a.picks != b.picks || a.pokemon != b.pokemon || a.active != b.active || a.nash_policies != b.nash_policies || a.score != b.score) return 4;
  const oakgpu_corpus_stats info = window.info(), want = corpus.info();
  if (info.records != want.records || info.frames != want.frames || info.malformed != want.malformed || info.stopped_at != records.size()) return 5;
  window.save(argv[4]);
  FILE *f = std::fopen(argv[3], "wb");
  if (!f) return 2;
  const std::vector<uint64_t> stats{st.records, st.bytes, st.appended, st.evicted, st.rejected, st.appends};
  dump(f, stats); dump(f, a.picks); dump(f, a.pokemon); dump(f, a.empirical_policies); dump(f, a.score);
  std::fclose(f);
  std::printf("%llu records, %llu evicted\nok\n", (unsigned long long)st.records, (unsigned long long)st.evicted);
  return 0;
}
