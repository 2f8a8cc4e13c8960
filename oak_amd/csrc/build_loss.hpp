// oak_amd/csrc/build_loss.hpp -- the two 31-step recursions of the build trainer's loss (src/oak/build.py:196-213 and their adjoint), one
// text for the host and the device (buildtrain.hip's k_traj; tests/cpp_build_loss_check.cc runs it without a GPU).  Plain float in the
// order torch evaluates build.py's lines; every function switches contraction off, so a * b + c is two roundings on the device as it is
// on the host.  The contract is in include/oakgpu.h, "Training the build network".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OAK_BUILD_LOSS_HD __host__ __device__
#else
#define OAK_BUILD_LOSS_HD
#endif

namespace oak_build_loss {

constexpr int STEPS = 31;

// value_full [31] (the value at valid steps, 0 elsewhere), rewards [31], valid [31] -> gae [31], returns [31].
//   delta[t] = rewards[t] + gamma * value_full[t + 1] - value_full[t]          (value_full[31] = 0)
//   gae[t]   = delta[t] * valid[t] + gamma_lam * gae[t + 1]                    (t descending, gae[31] = 0)
//   ret[t]   = gae[t] + value_full[t]
OAK_BUILD_LOSS_HD inline void gae_forward(const float *value_full, const float *rewards, const uint8_t *valid, float gamma, float gamma_lam, float *gae, float *ret) {
#pragma clang fp contract(off)
  float adv = 0.0f;
  for (int t = STEPS - 1; t >= 0; --t) {
    const float next = t + 1 < STEPS ? value_full[t + 1] : 0.0f;
    const float scaled = gamma * next;
    const float target = rewards[t] + scaled;
    const float delta = target - value_full[t];
    const float kept = delta * (valid[t] ? 1.0f : 0.0f);
    const float carried = gamma_lam * adv;
    adv = kept + carried;
    gae[t] = adv;
    ret[t] = adv + value_full[t];
  }
}

// The adjoint: G [31] = dL/dgae (0 where the step is not valid or not selected) -> d_value_full [31].
//   A[t] = G[t] + gamma_lam * A[t - 1]                                         (t ascending, A[-1] = 0)
//   D[t] = valid[t] * A[t]
//   d_value_full[t] = -D[t] + gamma * D[t - 1]
// (gae is not detached inside returns, and the direct paths of value_full through returns - values cancel.)
OAK_BUILD_LOSS_HD inline void gae_backward(const float *G, const uint8_t *valid, float gamma, float gamma_lam, float *d_value_full) {
#pragma clang fp contract(off)
  float A = 0.0f, D_before = 0.0f;
  for (int t = 0; t < STEPS; ++t) {
    const float carried = gamma_lam * A;
    A = G[t] + carried;
    const float D = valid[t] ? A : 0.0f;
    const float from_before = gamma * D_before;
    d_value_full[t] = from_before - D;
    D_before = D;
  }
}

// cf = [z0 > -2] * min(gae, 0) + [z0 < 2] * max(gae, 0): apply_force_with_threshold's clipped force (threshold 2, centre 0)
OAK_BUILD_LOSS_HD inline float clipped_force(float z0, float gae) {
#pragma clang fp contract(off)
  const float neg = gae < 0.0f ? gae : 0.0f, pos = gae > 0.0f ? gae : 0.0f;
  const float a = (z0 > -2.0f ? 1.0f : 0.0f) * neg;
  const float b = (z0 < 2.0f ? 1.0f : 0.0f) * pos;
  return a + b;
}

} // namespace oak_build_loss
