// tests/cpp_nash_soft_check.cc -- stand-alone check of oak_amd/csrc/nash.hpp for a sanitizer build (tests/test_nash_soft.py builds it with
// g++ -fsanitize=address,undefined and runs it): solve_soft at both widths against solve (the x87 long double path) over directed
// families of matrices, and the rounding restatement against real long double arithmetic.  Exit status 0 and "ok" when all agree.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define OAK_NASH_WORDS_ONLY 1 // the product in 32-bit words: the text the device compiles
#include "../oak_amd/csrc/nash.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() { // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
int below(int k) { return (int)(next_u64() % (uint64_t)k); }

long g_checked = 0, g_failed = 0;

bool same_bits(const double *a, const double *b, int k) { return memcmp(a, b, sizeof(double) * k) == 0; }

void check_matrix(const std::vector<int32_t> &M, int m, int n, const char *family) {
  double p1[9] = {}, p2[9] = {}, v = 0, q1[9] = {}, q2[9] = {}, u = 0;
  const bool ok = oak_nash::solve(M.data(), m, n, p1, p2, &v);
  int limbs = 0;
  const bool known = oak_nash::width_of(M.data(), m, n, &limbs);
  if (ok != known) { ++g_failed; printf("%s %dx%d: width_of and solve disagree on the refusal\n", family, m, n); return; }
  for (int width = 4; width <= 8; width += 4) {
    if (known && width < limbs) continue; // the narrow width only where the selector allows it
    memset(q1, 0, sizeof q1); memset(q2, 0, sizeof q2); u = 0;
    const bool got = width == 4 ? oak_nash::solve_soft<4>(M.data(), m, n, q1, q2, &u) : oak_nash::solve_soft<8>(M.data(), m, n, q1, q2, &u);
    ++g_checked;
    if (got != ok || (ok && !(same_bits(p1, q1, m) && same_bits(p2, q2, n) && same_bits(&v, &u, 1)))) {
      ++g_failed;
      printf("%s %dx%d at %d limbs differs from solve\n", family, m, n, width);
    }
  }
}

void matrices() {
  for (int m = 1; m <= 9; ++m)
    for (int n = 1; n <= 9; ++n)
      for (int rep = 0; rep < 2; ++rep) {
        std::vector<int32_t> M((size_t)m * n);
        for (auto &x : M) x = below(257);
        check_matrix(M, m, n, "0...256");
        for (auto &x : M) x = below((1 << 21) + 1) - (1 << 20);
        check_matrix(M, m, n, "+-2^20");
        for (auto &x : M) x = 77;
        check_matrix(M, m, n, "all equal");
        for (auto &x : M) x = below(257);
        if (m > 1) for (int j = 0; j < n; ++j) M[(size_t)(m - 1) * n + j] = M[j];
        check_matrix(M, m, n, "duplicated row");
        for (auto &x : M) x = below(257);
        if (n > 1) for (int i = 0; i < m; ++i) M[(size_t)i * n + n - 1] = M[(size_t)i * n];
        check_matrix(M, m, n, "duplicated column");
        for (auto &x : M) x = 1 + below(200);
        if (m > 1) for (int j = 0; j < n; ++j) M[(size_t)(m - 1) * n + j] = M[j] - 1;
        check_matrix(M, m, n, "dominated row");
        for (auto &x : M) x = below(100);
        { const int si = below(m), sj = below(n);
          for (int j = 0; j < n; ++j) M[(size_t)si * n + j] = 150 + below(50);
          for (int i = 0; i < m; ++i) M[(size_t)i * n + sj] = 100 + below(50);
          M[(size_t)si * n + sj] = 150; }
        check_matrix(M, m, n, "saddle point");
      }
  std::vector<int32_t> rps(81, 128); // rock-paper-scissors padded to 9 x 9
  for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) rps[i * 9 + j] = (i % 3 == j % 3) ? 128 : ((i % 3 + 2) % 3 == j % 3 ? 256 : 0);
  check_matrix(rps, 9, 9, "rock-paper-scissors");
  std::vector<int32_t> beyond(4, 0);
  beyond[3] = (1 << 20) + 1;
  check_matrix(beyond, 2, 2, "refused");
  std::vector<int32_t> edge(4, 0); // one step past the narrow width's bound: routed to 8 limbs
  edge[3] = (int32_t)oak_nash::WIDTH4_MAX_ENTRY;
  int limbs = 0;
  if (!oak_nash::width_of(edge.data(), 2, 2, &limbs) || limbs != 8) { ++g_failed; printf("the bound's successor is not routed to 8 limbs\n"); }
  edge[3] = (int32_t)oak_nash::WIDTH4_MAX_ENTRY - 1;
  if (!oak_nash::width_of(edge.data(), 2, 2, &limbs) || limbs != 4) { ++g_failed; printf("the bound itself is not routed to 4 limbs\n"); }
  check_matrix(edge, 2, 2, "at the bound");
}

void check_ratio(const oak_nash::Wide &a, const oak_nash::Wide &b, int64_t shift) {
  const double hard = (double)(a.to_ld() / b.to_ld() - (long double)shift);
  const double soft = oak_nash::x87_to_double(oak_nash::x87_subtract_int(oak_nash::x87_divide(oak_nash::x87_from_wide(a), oak_nash::x87_from_wide(b)), shift));
  ++g_checked;
  if (memcmp(&hard, &soft, 8)) { ++g_failed; printf("ratio differs: hard %a soft %a shift %lld\n", hard, soft, (long long)shift); }
}

oak_nash::Wide random_wide(int limbs) {
  oak_nash::Wide v;
  for (int i = 0; i < limbs; ++i) { const uint64_t x = next_u64() >> (i == limbs - 1 ? 1 + below(62) : 0); v.w[2 * i] = (uint32_t)x; v.w[2 * i + 1] = (uint32_t)(x >> 32); }
  if (v.zero()) v.w[0] = 1;
  return v;
}

void ratios() {
  const int64_t shifts[] = {0, 1, 2, -3, 257, (1 << 20) + 1, -(1 << 20)};
  for (int rep = 0; rep < 4000; ++rep) {
    const oak_nash::Wide a = random_wide(1 + below(7)), b = random_wide(1 + below(7));
    check_ratio(a, b, shifts[rep % 7]);
    check_ratio(-a, b, shifts[rep % 7]);
    check_ratio(a, a, shifts[rep % 7]);
  }
  for (int rep = 0; rep < 500; ++rep) { // 65 significant bits with a tie, or nearly one, at the accumulate step
    oak_nash::Wide a, b(1);
    const uint64_t low = next_u64() | 1;
    a.w[0] = (uint32_t)low; a.w[1] = (uint32_t)(low >> 32); a.w[2] = 1;
    check_ratio(a, b, 0);
    oak_nash::Wide c; // a third limb of 2^63 below it
    c.w[1] = 0x80000000u; c.w[2] = (uint32_t)low; c.w[3] = (uint32_t)(low >> 32); c.w[4] = 1;
    check_ratio(c, b, 0);
    check_ratio(c, a, 1);
    // quotients on a 53-bit midpoint: (2^53 + odd) * 2^10 + 2^10 over 2^k
    oak_nash::Wide mid(0);
    const uint64_t mant = (1ull << 63) | (next_u64() >> 12 << 11) | (1ull << 10);
    mid.w[0] = (uint32_t)mant; mid.w[1] = (uint32_t)(mant >> 32);
    check_ratio(mid, oak_nash::Wide(1 << below(20)), 0);
    oak_nash::Wide above = mid; // 65 bits whose 64-bit rounding lands on the 53-bit midpoint: double rounding
    above = above + above + oak_nash::Wide(1);
    check_ratio(above, oak_nash::Wide(3), 0);
    check_ratio(above, oak_nash::Wide(1), rep);
  }
}

} // namespace

int main() {
  matrices();
  ratios();
  printf("%ld checks, %ld failed\n", g_checked, g_failed);
  if (g_failed) return 1;
  printf("ok\n");
  return 0;
}
