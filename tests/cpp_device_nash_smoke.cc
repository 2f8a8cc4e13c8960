// OakGPU::solve_matrices (include/oakgpu.hpp) against a loop of OakGPU::solve_matrix, and SearchForest::search with NASH_DEVICE against
// NASH_HOST, bit for bit (tests/test_gpu_device_nash.py).  Without a GPU it only links.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <oakgpu.hpp>
#include <pkmn.h>

static uint64_t g_state = 42;
static uint64_t next_u64() { // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

int main() {
  if (oakgpu_device_count() == 0) { std::puts("no gpu: link check only"); return 0; }
  OakGPU::Context ctx{0};
  std::vector<std::vector<int32_t>> payoffs;
  std::vector<int> m, n;
  for (int k = 0; k < 200; ++k) {
    const int mm = 1 + (int)(next_u64() % 9), nn = 1 + (int)(next_u64() % 9);
    std::vector<int32_t> M((size_t)mm * nn);
    for (auto &x : M) x = k % 3 == 0 ? (int32_t)(next_u64() % ((1u << 21) + 1)) - (1 << 20) : k % 3 == 1 ? (int32_t)(next_u64() % 257) : (int32_t)(next_u64() % 3);
    payoffs.push_back(M); m.push_back(mm); n.push_back(nn);
  }
  for (int factor : {256, 1, 7}) {
    const auto got = OakGPU::solve_matrices(ctx, payoffs, m, n, factor);
    if (got.size() != payoffs.size()) { std::puts("solve_matrices: wrong count"); return 1; }
    for (size_t k = 0; k < payoffs.size(); ++k) {
      const auto want = OakGPU::solve_matrix(payoffs[k], m[k], n[k], factor);
      const double gv = std::get<2>(got[k]), wv = std::get<2>(want);
      if (!same(std::get<0>(got[k]), std::get<0>(want)) || !same(std::get<1>(got[k]), std::get<1>(want)) || std::memcmp(&gv, &wv, 8)) {
        std::printf("solve_matrices: matrix %zu (%d x %d, factor %d) differs from solve_matrix\n", k, m[k], n[k], factor);
        return 1;
      }
    }
  }
  if (!OakGPU::solve_matrices(ctx, {}, {}, {}).empty()) { std::puts("solve_matrices: an empty batch is not empty"); return 1; }
  bool refused = false;
  try { OakGPU::solve_matrices(ctx, {{0, (1 << 20) + 1}}, {1}, {2}); } catch (const std::exception &) { refused = true; }
  if (!refused) { std::puts("solve_matrices: a payoff beyond 2^20 was not refused"); return 1; }
  std::puts("solve_matrices == solve_matrix");

  const int N = 6;
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
    seeds[i] = 500 + 3 * i;
  }
  oakgpu_search_params p = OakGPU::TreeSearch::default_params();
  p.iterations = 16; p.batch = 1; p.ucb_c = 1.0f; p.bandit = 0; p.eval = 2;
  OakGPU::SearchForest forest{ctx, 8, 16};
  const std::vector<oakgpu_search_output> host = forest.search(p, roots, seeds, nullptr, OakGPU::NASH_HOST);
  const std::vector<oakgpu_search_output> dev = forest.search(p, roots, seeds, nullptr, OakGPU::NASH_DEVICE);
  for (int i = 0; i < N; ++i)
    if (std::memcmp(host[i].p1_nash, dev[i].p1_nash, 72) || std::memcmp(host[i].p2_nash, dev[i].p2_nash, 72) || std::memcmp(&host[i].nash_value, &dev[i].nash_value, 8) ||
        std::memcmp(host[i].visit_matrix, dev[i].visit_matrix, sizeof host[i].visit_matrix)) {
      std::printf("forest search: tree %d differs between NASH_HOST and NASH_DEVICE\n", i);
      return 1;
    }
  double sum = 0;
  for (int q = 0; q < 9; ++q) sum += host[0].p1_nash[q];
  if (!(sum > 0.999 && sum < 1.001)) { std::puts("forest search: no strategy was solved"); return 1; }
  std::puts("ok");
  return 0;
}
