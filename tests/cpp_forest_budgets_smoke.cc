// OakGPU::SearchForest::search with budgets (include/oakgpu.hpp) against the C call it wraps and against the same face without budgets at
// each tree's own iteration count (tests/test_gpu_forest_budgets.py).  Without a GPU it only links.
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
  const std::vector<uint32_t> budgets = {16, 3, 1, 16, 9, 3, 1, 9};
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
  const std::vector<oakgpu_search_output> out = forest.search(p, roots, seeds, nullptr, true, &streams, false, budgets);
  const std::array<uint64_t, 2> rows = forest.last_rows();
  if (rows[1] != 16 + 3 + 1 + 16 + 9 + 3 + 1 + 9 || rows[0] < rows[1]) { std::printf("bad accounting: %llu launched, %llu run\n", (unsigned long long)rows[0], (unsigned long long)rows[1]); return 1; }
  std::vector<oakgpu_search_output> raw(N);
  std::vector<uint64_t> raw_streams(N);
  OakGPU::check(oakgpu_forest_search_budgets(forest.get(), nullptr, &p, b.data(), d.data(), r.data(), seeds.data(), budgets.data(), N, raw.data(), 1, raw_streams.data(), nullptr, 0));
  for (int i = 0; i < N; ++i)
    if (!same(out[i], raw[i]) || streams[i] != raw_streams[i]) { std::printf("SearchForest differs from the C call (tree %d)\n", i); return 1; }
  for (uint32_t k : {1u, 3u, 9u, 16u}) { // the same face without budgets, at each budget
    oakgpu_search_params q = p;
    q.iterations = k;
    std::vector<uint64_t> uniform_streams;
    const std::vector<oakgpu_search_output> uniform = forest.search(q, roots, seeds, nullptr, true, &uniform_streams);
    for (int i = 0; i < N; ++i) {
      if (budgets[i] != k) continue;
      if (!same(out[i], uniform[i]) || streams[i] != uniform_streams[i] || out[i].iterations != k) { std::printf("tree %d differs from the search with %u iterations\n", i, k); return 1; }
    }
  }
  bool threw = false; // a refusal surfaces as std::runtime_error with the library's text
  std::vector<uint32_t> bad = budgets;
  bad[2] = 17;
  try { (void)forest.search(p, roots, seeds, nullptr, true, nullptr, false, bad); } catch (const std::runtime_error &e) { threw = std::string{e.what()}.find("the budget of tree 2") != std::string::npos; }
  if (!threw) { std::puts("a budget above params->iterations accepted"); return 1; }
  std::puts("forest with budgets == c call == uniform searches");
  std::puts("ok");
  return 0;
}
