// OakGPU::ForestSelfplay (include/oakgpu.hpp) with fast searches against the C calls it wraps and against oakgpu_selfplay_game with batch = 1
// and the same fast fields (tests/test_gpu_forest_fast_selfplay.py).  Without a GPU it only links.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <oakgpu.hpp>
#include <pkmn.h>

int main() {
  if (oakgpu_device_count() == 0) { std::puts("no gpu: link check only"); return 0; }
  OakGPU::Context ctx{0};
  const uint32_t N = 6;
  static const uint8_t sets[12][5] = {{124, 59, 142, 94, 156}, {65, 94, 86, 105, 69}, {103, 79, 94, 153, 95}, {143, 34, 156, 89, 63}, {128, 34, 89, 63, 126}, {121, 59, 94, 85, 105},
                                      {113, 135, 86, 58, 85}, {94, 95, 101, 85, 153}, {112, 89, 157, 34, 63}, {145, 65, 85, 86, 97}, {80, 133, 94, 57, 156}, {91, 59, 153, 128, 62}};
  std::vector<uint8_t> teams(N * 60);
  std::vector<uint64_t> battle_seeds(N), seeds(N);
  for (uint32_t g = 0; g < N; ++g) { std::memcpy(&teams[g * 60], sets, 60); battle_seeds[g] = 0x9E3779B97F4A7C15ull * (g + 1); seeds[g] = 500 + 3 * g; }
  oakgpu_selfplay_params p{};
  p.search = OakGPU::TreeSearch::default_params();
  p.search.iterations = 12; p.search.batch = 1; p.search.ucb_c = 2.0f; p.search.bandit = 0; p.search.eval = 2;
  std::strcpy(p.policy_mode, "e0.9-x0.1");
  p.policy_temp = 1.0; p.policy_min = 0.0;
  p.fast_budget = 3; p.fast_search_prob = 0.5;
  std::strcpy(p.fast_policy_mode, "x");
  OakGPU::SearchForest forest{ctx, 8, 16};
  OakGPU::ForestSelfplay play{forest};
  const OakGPU::ForestSelfplay::Result got = play.play(p, teams, battle_seeds, seeds);
  // the C calls
  OakGPU::check(oakgpu_forest_selfplay(forest.get(), nullptr, &p, teams.data(), battle_seeds.data(), seeds.data(), N, 1));
  size_t bytes = 0;
  OakGPU::check(oakgpu_forest_selfplay_records(forest.get(), nullptr, 0, &bytes, nullptr, nullptr, nullptr, nullptr, 0));
  std::vector<uint8_t> raw(bytes + 1);
  std::vector<uint64_t> offsets(N + 1);
  OakGPU::check(oakgpu_forest_selfplay_records(forest.get(), raw.data(), bytes, &bytes, offsets.data(), nullptr, nullptr, nullptr, 0));
  raw.resize(bytes);
  if (raw != got.stream || offsets != got.offsets) { std::puts("ForestSelfplay differs from the C call"); return 1; }
  uint64_t frames_written = 0;
  for (uint32_t g = 0; g < N; ++g) frames_written += got.n_frames[g];
  if (got.fast_stats[0] == 0 || got.fast_stats[1] == 0 || got.fast_stats[0] + got.fast_stats[1] != frames_written || got.fast_stats[2] != got.fast_stats[3] ||
      got.fast_stats[3] != 3 * got.fast_stats[0] + 12 * got.fast_stats[1]) {
    std::puts("bad fast-search counters");
    return 1;
  }
  // the host loop, game by game
  std::vector<uint8_t> one(391 + 83 * 2048);
  for (uint32_t g = 0; g < N; ++g) {
    oakgpu_selfplay_params q = p;
    q.seed = seeds[g];
    size_t written = 0;
    uint32_t frames = 0;
    uint8_t result = 0;
    OakGPU::check(oakgpu_selfplay_game(ctx.get(), nullptr, &teams[g * 60], battle_seeds[g], &q, one.data(), one.size(), &written, &frames, &result));
    const size_t at = got.offsets[g], len = got.offsets[g + 1] - at;
    if (got.status[g] != OAKGPU_FSP_OK || len != written || std::memcmp(&got.stream[at], one.data(), len) != 0 || frames != got.n_frames[g] || result != got.results[g]) {
      std::printf("game %u differs from oakgpu_selfplay_game with batch 1\n", g);
      return 1;
    }
  }
  bool threw = false; // a refusal surfaces as std::runtime_error with the library's text
  p.fast_budget = 17;
  try { (void)play.play(p, teams, battle_seeds, seeds); } catch (const std::runtime_error &e) { threw = std::string{e.what()}.find("fast_budget") != std::string::npos; }
  if (!threw) { std::puts("a fast_budget above max_iterations accepted"); return 1; }
  std::puts("forest selfplay with fast searches == c call == host loop");
  std::puts("ok");
  return 0;
}
