// OakGPU::BuildNet (include/oakgpu.hpp): provide, rollout and records on the files the test hands over; the outputs go to a file that
// tests/test_gpu_build_selfplay.py compares with oak_amd.build's.  usage: cpp_build_smoke NET POOL OUT.  Without a GPU it only links.
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
  if (oakgpu_device_count() == 0 || argc < 4) { std::puts("no gpu: link check only"); return 0; }
  const std::vector<uint8_t> net_bytes = slurp(argv[1]), pool = slurp(argv[2]);
  OakGPU::BuildNet::check_net(net_bytes);
  OakGPU::Context ctx{0};
  OakGPU::BuildNet net{ctx, net_bytes};
  const uint32_t n = 40;
  std::vector<uint64_t> seeds(n);
  for (uint32_t g = 0; g < n; ++g) seeds[g] = 1000 + 17 * g;
  const oakgpu_build_provider prm{5, 0, 0.3, 0.3, 0.7};
  const OakGPU::BuildNet::Trajectories t = net.provide(pool, seeds, prm);
  std::vector<float> value(n, 0.5f), score(n);
  for (uint32_t g = 0; g < n; ++g) score[g] = g % 3 == 2 ? -1.0f : 0.5f * (g % 3);
  const std::vector<uint8_t> records = net.records(t, value, score);
  const OakGPU::BuildNet::Trajectories again = net.rollout(t.teams_init, seeds, t.sizes, 1);
  FILE *f = std::fopen(argv[3], "wb");
  if (!f) return 2;
  dump(f, t.teams_out); dump(f, t.n_updates); dump(f, t.teams_init); dump(f, t.sizes); dump(f, t.team_index); dump(f, t.action); dump(f, t.prob);
  dump(f, again.teams_out); dump(f, again.n_updates);
  dump(f, records);
  std::fclose(f);
  std::printf("%u rows, %zu records\nok\n", n, records.size() / OAKGPU_BUILD_RECORD_BYTES);
  return 0;
}
