// oak_amd/csrc/fast_prng.hpp -- the reference's fast_prng on the device, shared by the rollout kernels (oakgpu.hip) and the
// training-frame sampler (trainframes.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oak {

// ---- fast_prng (cpp/include/util/random.h:67-133): 2 x u32 of state per lane ---------------
struct FastPrng {
  uint32_t s0, s1;
  __device__ __forceinline__ static uint32_t rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
  __device__ __forceinline__ uint32_t next32() {
    uint32_t result = rotl(s0 + s1, 9) + s0;
    s1 ^= s0;
    s0 = rotl(s0, 13) ^ s1 ^ (s1 << 5);
    s1 = rotl(s1, 28);
    return result;
  }
  // std::seed_seq{lo32, hi32}.generate(2 words), random.h:99-105
  __device__ void seed(uint64_t seed) {
    const uint32_t v[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t b0 = 0x8b8b8b8bu, b1 = 0x8b8b8b8bu;
    // n = 2, s = 2, t = 0, p = q = 1, m = 3; indices alternate between the two words
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      uint32_t &bk = (k & 1) ? b1 : b0, &bo = (k & 1) ? b0 : b1; // bk = b[k%2], bo = b[(k+1)%2] = b[(k-1)%2]
      uint32_t arg = bk ^ bo ^ bo;
      uint32_t r1 = 1664525u * (arg ^ (arg >> 27));
      uint32_t r2 = r1 + (k == 0 ? 2u : (k & 1) + v[k - 1 < 2 ? k - 1 : 0]);
      bo += r1;
      bo += r2;
      bk = r2;
    }
#pragma unroll
    for (uint32_t k = 3; k < 5; ++k) {
      uint32_t &bk = (k & 1) ? b1 : b0, &bo = (k & 1) ? b0 : b1;
      uint32_t arg = bk + bo + bo;
      uint32_t r3 = 1566083941u * (arg ^ (arg >> 27));
      uint32_t r4 = r3 - (k & 1);
      bo ^= r3;
      bo ^= r4;
      bk = r4;
    }
    s0 = b0;
    s1 = b1;
  }
};

} // namespace oak
