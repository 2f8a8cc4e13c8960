// OakGPU::ForestMatch (include/oakgpu.hpp) against the C call it wraps (tests/test_gpu_forest_match.py).  Without a GPU it only links.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <oakgpu.hpp>
#include <pkmn.h>

int main() {
  if (oakgpu_device_count() == 0) { std::puts("no gpu: link check only"); return 0; }
  OakGPU::Context ctx{0};
  const uint32_t N = 6, LOG = 400;
  static const uint8_t sets[12][5] = {{124, 59, 142, 94, 156}, {65, 94, 86, 105, 69}, {103, 79, 94, 153, 95}, {143, 34, 156, 89, 63}, {128, 34, 89, 63, 126}, {121, 59, 94, 85, 105},
                                      {113, 135, 86, 58, 85}, {94, 95, 101, 85, 153}, {112, 89, 157, 34, 63}, {145, 65, 85, 86, 97}, {80, 133, 94, 57, 156}, {91, 59, 153, 128, 62}};
  std::vector<uint8_t> teams(N * 60), b(N * 384), d(N * 8), r(N);
  std::vector<uint64_t> battle_seeds(N), seeds(N);
  for (uint32_t g = 0; g < N; ++g) { std::memcpy(&teams[g * 60], sets, 60); battle_seeds[g] = 0x9E3779B97F4A7C15ull * (g + 1); seeds[g] = 700 + 3 * g; }
  OakGPU::check(oakgpu_init_battles(ctx.get(), teams.data(), battle_seeds.data(), N, 1, b.data(), d.data(), r.data()));
  std::vector<OakGPU::Leaf> starts(N);
  for (uint32_t g = 0; g < N; ++g) { std::memcpy(starts[g].battle, &b[g * 384], 384); std::memcpy(starts[g].durations, &d[g * 8], 8); starts[g].result = r[g]; }
  oakgpu_forest_match_params p{};
  p.p1.search = OakGPU::TreeSearch::default_params();
  p.p1.search.iterations = 12; p.p1.search.batch = 1; p.p1.search.ucb_c = 2.0f; p.p1.search.bandit = 0; p.p1.search.eval = 2;
  p.p2.search = p.p1.search;
  p.p2.search.iterations = 6; p.p2.search.eval = 0;
  std::strcpy(p.p1.policy_mode, "e0.9-x0.1");
  std::strcpy(p.p2.policy_mode, "e");
  p.p1.policy_temp = p.p2.policy_temp = 1.0;
  p.early_stop = 10.0; p.log_turns = LOG; p.solve_nash = 1;
  OakGPU::SearchForest forest{ctx, 8, 16};
  OakGPU::ForestMatch match{forest};
  const OakGPU::ForestMatch::Result got = match.play(p, starts, seeds);
  // the C call
  std::vector<uint8_t> results(N), status(N);
  std::vector<uint32_t> turns(N);
  std::vector<oakgpu_match_turn> log((size_t)N * LOG);
  std::memset(log.data(), 0xFF, log.size() * sizeof(oakgpu_match_turn));
  uint64_t counts[4];
  OakGPU::check(oakgpu_forest_match(forest.get(), &p, b.data(), d.data(), r.data(), seeds.data(), N, results.data(), turns.data(), status.data(), log.data(), counts));
  if (results != got.results || status != got.status || turns != got.turns || std::memcmp(log.data(), got.log.data(), log.size() * sizeof(oakgpu_match_turn)) != 0 ||
      std::memcmp(counts, got.counts.data(), sizeof counts) != 0) {
    std::puts("ForestMatch differs from the C call");
    return 1;
  }
  uint64_t sum = 0, longest = 0;
  for (uint32_t g = 0; g < N; ++g) {
    sum += turns[g];
    longest = turns[g] > longest ? turns[g] : longest;
    std::printf("game %u: %u turns, result %u, status %u\n", g, turns[g], (unsigned)results[g], (unsigned)status[g]);
    if (status[g] != OAKGPU_FM_OK && status[g] != OAKGPU_FM_EARLY_STOP) { std::puts("unexpected status"); return 1; }
  }
  if (counts[0] + counts[1] + counts[2] != N || counts[3] != 0 || got.stats[3] != got.stats[0] + 1 || got.stats[1] + got.stats[2] >= 2 * sum || got.stats[0] < longest) {
    std::puts("bad bookkeeping");
    return 1;
  }
  bool threw = false; // a refusal surfaces as std::runtime_error with the library's text
  p.p2.search.duration_us = 1000;
  try { (void)match.play(p, starts, seeds); } catch (const std::runtime_error &e) { threw = std::string{e.what()}.find("seat p2") != std::string::npos; }
  if (!threw) { std::puts("a time budget was accepted"); return 1; }
  std::puts("forest match == c call");
  std::puts("ok");
  return 0;
}
