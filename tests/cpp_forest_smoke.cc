// OakGPU::SearchForest (include/oakgpu.hpp) against the C call it wraps and against OakGPU::TreeSearch with batch = 1
// (tests/test_gpu_search_forest.py).  Without a GPU it only links.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <oakgpu.hpp>
#include <pkmn.h>

static bool same(oakgpu_search_output a, oakgpu_search_output b) { // every field but the duration
  a.duration_us = b.duration_us = 0;
  const size_t head = offsetof(oakgpu_search_output, p2_choices) + 9, body = offsetof(oakgpu_search_output, visit_matrix); // (padding between them)
  return std::memcmp(&a, &b, head) == 0 && std::memcmp((const char *)&a + body, (const char *)&b + body, sizeof a - body) == 0;
}

int main() {
  if (oakgpu_device_count() == 0) { std::puts("no gpu: link check only"); return 0; }
  OakGPU::Context ctx{0};
  const int N = 8;
  uint8_t teams[N][60];
  uint64_t battle_seeds[N];
  static const uint8_t sets[12][5] = {{124, 59, 142, 94, 156}, {65, 94, 86, 105, 69}, {103, 79, 94, 153, 95}, {143, 34, 156, 89, 63}, {128, 34, 89, 63, 126}, {121, 59, 94, 85, 105},
                                      {113, 135, 86, 58, 85}, {94, 95, 101, 85, 153}, {112, 89, 157, 34, 63}, {145, 65, 85, 86, 97}, {80, 133, 94, 57, 156}, {91, 59, 153, 128, 62}};
  for (int i = 0; i < N; ++i) { std::memcpy(teams[i], sets, 60); battle_seeds[i] = 0x9E3779B97F4A7C15ull * (i + 1); }
  std::vector<uint8_t> b(N * 384), d(N * 8), r(N);
  OakGPU::check(oakgpu_init_battles(ctx.get(), &teams[0][0], battle_seeds, N, 1, b.data(), d.data(), r.data()));
  std::vector<OakGPU::Leaf> roots(N);
  std::vector<uint64_t> seeds(N);
  for (int i = 0; i < N; ++i) {
    std::memcpy(roots[i].battle, &b[i * 384], 384);
    std::memcpy(roots[i].durations, &d[i * 8], 8);
    roots[i].result = r[i];
    seeds[i] = 1000 + 7 * i;
  }
  oakgpu_search_params p = OakGPU::TreeSearch::default_params();
  p.iterations = 16; p.batch = 1; p.ucb_c = 1.0f; p.bandit = 0; p.eval = 0;
  OakGPU::SearchForest forest{ctx, 16, 32};
  std::vector<uint64_t> streams;
  const std::vector<oakgpu_search_output> out = forest.search(p, roots, seeds, nullptr, true, &streams);
  std::vector<oakgpu_search_output> raw(N);
  std::vector<uint64_t> raw_streams(N);
  OakGPU::check(oakgpu_forest_search(forest.get(), nullptr, &p, b.data(), d.data(), r.data(), seeds.data(), N, raw.data(), 1, raw_streams.data(), nullptr, 0));
  OakGPU::TreeSearch search{ctx};
  for (int i = 0; i < N; ++i) {
    if (!same(out[i], raw[i]) || streams[i] != raw_streams[i]) { std::printf("SearchForest differs from the C call (tree %d)\n", i); return 1; }
    oakgpu_search_params q = p;
    q.seed = seeds[i];
    const oakgpu_search_output one = search.run(roots[i], q);
    if (!same(out[i], one)) { std::printf("SearchForest differs from TreeSearch with batch 1 (tree %d)\n", i); return 1; }
    if (out[i].iterations != 16 || out[i].nodes != forest.nodes(i, 0, (uint32_t)out[i].nodes).size()) { std::printf("bad bookkeeping (tree %d)\n", i); return 1; }
    std::printf("tree %d: nodes %llu value %.17g stream %llu\n", i, (unsigned long long)out[i].nodes, out[i].empirical_value, (unsigned long long)streams[i]);
  }
  bool threw = false; // a refusal surfaces as std::runtime_error with the library's text
  p.iterations = 33;
  try { (void)forest.search(p, roots, seeds); } catch (const std::runtime_error &e) { threw = std::string{e.what()}.find("max_iterations") != std::string::npos; }
  if (!threw) { std::puts("iterations above max_iterations accepted"); return 1; }
  std::puts("forest == c call == tree search");
  std::puts("ok");
  return 0;
}
