// OakGPU::ForestMatch::play(..., records = true) (include/oakgpu.hpp) over games handed in by tests/test_gpu_forest_match_records.py, which
// compares the two streams written here with search_games'.  usage: <in> <out prefix>; in = u32 n, n x 384 battles, n x 8 durations, n results,
// n x u64 seeds; out: <prefix>.p1 / <prefix>.p2 = the streams, then the offsets (n + 1 x u64) and the frame counts (n x u32).  Seat p1:
// PokeEngine, seat p2: Monte-Carlo, 8 iterations each, UCB c = 2, mode e, the Nash solve, no early stop.  Without a GPU it only links.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <oakgpu.hpp>

int main(int argc, char **argv) {
  if (oakgpu_device_count() == 0) { std::puts("no gpu: link check only"); return 0; }
  if (argc != 3) { std::puts("usage: <in> <out prefix>"); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  uint32_t n = 0;
  if (!in || std::fread(&n, 4, 1, in) != 1 || n == 0 || n > 4096) { std::puts("bad input"); return 2; }
  std::vector<uint8_t> b((size_t)n * 384), d((size_t)n * 8), r(n);
  std::vector<uint64_t> seeds(n);
  if (std::fread(b.data(), 384, n, in) != n || std::fread(d.data(), 8, n, in) != n || std::fread(r.data(), 1, n, in) != n || std::fread(seeds.data(), 8, n, in) != n) {
    std::puts("short input");
    return 2;
  }
  std::fclose(in);
  std::vector<OakGPU::Leaf> starts(n);
  for (uint32_t g = 0; g < n; ++g) { std::memcpy(starts[g].battle, &b[(size_t)g * 384], 384); std::memcpy(starts[g].durations, &d[(size_t)g * 8], 8); starts[g].result = r[g]; }
  oakgpu_forest_match_params p{};
  p.p1.search = OakGPU::TreeSearch::default_params();
  p.p1.search.iterations = 8; p.p1.search.batch = 1; p.p1.search.ucb_c = 2.0f; p.p1.search.bandit = 0; p.p1.search.eval = 2;
  p.p2.search = p.p1.search;
  p.p2.search.eval = 0;
  std::strcpy(p.p1.policy_mode, "e");
  std::strcpy(p.p2.policy_mode, "e");
  p.p1.policy_temp = p.p2.policy_temp = 1.0;
  p.solve_nash = 1;
  OakGPU::Context ctx{0};
  OakGPU::SearchForest forest{ctx, n, 8};
  OakGPU::ForestMatch match{forest};
  const OakGPU::ForestMatch::Result off = match.play(p, starts, seeds);
  if (!off.records[0].stream.empty() || !off.records[0].offsets.empty()) { std::puts("records without the switch"); return 1; }
  size_t bytes = 0; // after a call made with recording off the accessor fails by name
  if (oakgpu_forest_match_records(forest.get(), 0, nullptr, 0, &bytes, nullptr, nullptr, nullptr, nullptr, 0) == 0 ||
      std::string{oakgpu_last_error()}.find("oakgpu_forest_match_records: ") != 0) {
    std::puts("the accessor accepted a call made with recording off");
    return 1;
  }
  const OakGPU::ForestMatch::Result got = match.play(p, starts, seeds, true);
  if (got.results != off.results || got.turns != off.turns || got.status != off.status) { std::puts("recording changed the games"); return 1; }
  for (int seat = 0; seat < 2; ++seat) {
    const OakGPU::ForestMatch::Records &rec = got.records[seat];
    if (rec.offsets.size() != (size_t)n + 1 || rec.offsets[n] != rec.stream.size() || rec.n_frames != got.turns) { std::puts("bad record bookkeeping"); return 1; }
    FILE *out = std::fopen((std::string{argv[2]} + (seat ? ".p2" : ".p1")).c_str(), "wb");
    if (!out) { std::puts("cannot write"); return 2; }
    std::fwrite(rec.stream.data(), 1, rec.stream.size(), out);
    std::fwrite(rec.offsets.data(), 8, rec.offsets.size(), out);
    std::fwrite(rec.n_frames.data(), 4, rec.n_frames.size(), out);
    std::fclose(out);
  }
  std::puts("ok");
  return 0;
}
