// OakGPU::BuildTrajectories (include/oakgpu.hpp): the statuses on the host, then a corpus, a decode of every record, a sample and the targets
// on the files the test hands over; the outputs go to a file that tests/test_gpu_build_traj_cpp.py compares with oak_amd.build's.
// usage: cpp_build_traj_smoke RECORDS OUT.  Without a GPU it only links.
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
  if (oakgpu_device_count() == 0 || argc < 3) { std::puts("no gpu: link check only"); return 0; }
  const std::vector<uint8_t> bytes = slurp(argv[1]);
  const std::vector<uint8_t> status = OakGPU::BuildTrajectories::check_records(bytes);
  OakGPU::Context ctx{0};
  const size_t half = status.size() / 2 * OAKGPU_BUILD_RECORD_BYTES;
  OakGPU::BuildTrajectories corpus{ctx, {std::vector<uint8_t>(bytes.begin(), bytes.begin() + half), std::vector<uint8_t>(bytes.begin() + half, bytes.end())}};
  std::vector<uint32_t> picks(status.size());
  for (size_t i = 0; i < picks.size(); ++i) picks[i] = static_cast<uint32_t>(i);
  OakGPU::BuildTrajectories::Rows all = corpus.decode(picks);
  if (all.status != status) return 3;
  const OakGPU::BuildTrajectories::Rows drawn = corpus.sample(33, 77, false, true);
  const OakGPU::BuildTrajectories::Targets t = corpus.targets(all, 0.25);
  const oakgpu_build_corpus_stats st = corpus.info();
  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  dump(f, all.action); dump(f, all.mask); dump(f, all.policy); dump(f, all.status);
  dump(f, drawn.picks); dump(f, drawn.score);
  dump(f, t.rows); dump(f, t.state_cells); dump(f, t.old_logp); dump(f, t.rewards);
  std::fclose(f);
  std::printf("%u records in %u files, %u valid steps, t_max %u\nok\n", st.records, st.files, t.n_valid, all.t_max);
  return 0;
}
