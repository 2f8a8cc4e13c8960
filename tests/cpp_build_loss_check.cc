// tests/cpp_build_loss_check.cc -- oak_amd/csrc/build_loss.hpp on the host, without a GPU: `check FILE` reads
//   u32 n, f32 gamma, f32 gamma_lam, then value_full f32 [n][31], rewards f32 [n][31], valid u8 [n][31], G f32 [n][31], z0 f32 [n][31]
// and prints per trajectory 31 lines of four words in hex: gae, returns, d_value_full, clipped_force(z0, gae).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../oak_amd/csrc/build_loss.hpp"

namespace bl = oak_build_loss;

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

int main(int argc, char **argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s FILE\n", argv[0]), 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  uint32_t n = 0;
  float gamma = 0, gamma_lam = 0;
  if (fread(&n, 4, 1, f) != 1 || fread(&gamma, 4, 1, f) != 1 || fread(&gamma_lam, 4, 1, f) != 1) return fprintf(stderr, "short header\n"), 2;
  const size_t steps = (size_t)n * bl::STEPS;
  std::vector<float> vf(steps), rew(steps), G(steps), z0(steps);
  std::vector<uint8_t> valid(steps);
  if (fread(vf.data(), 4, steps, f) != steps || fread(rew.data(), 4, steps, f) != steps || fread(valid.data(), 1, steps, f) != steps ||
      fread(G.data(), 4, steps, f) != steps || fread(z0.data(), 4, steps, f) != steps)
    return fprintf(stderr, "short body\n"), 2;
  fclose(f);
  for (uint32_t b = 0; b < n; ++b) {
    float gae[bl::STEPS], ret[bl::STEPS], dvf[bl::STEPS];
    const size_t at = (size_t)b * bl::STEPS;
    bl::gae_forward(vf.data() + at, rew.data() + at, valid.data() + at, gamma, gamma_lam, gae, ret);
    bl::gae_backward(G.data() + at, valid.data() + at, gamma, gamma_lam, dvf);
    for (int t = 0; t < bl::STEPS; ++t) printf("%08x %08x %08x %08x\n", bits(gae[t]), bits(ret[t]), bits(dvf[t]), bits(bl::clipped_force(z0[at + t], gae[t])));
  }
  return 0;
}
