// oak_amd/csrc/encode_index.hpp -- the two index rules both encoders share: the leaf evaluator's sparse form (leafnet.hip) and the
// training rows' dense form (trainframes.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oak {

__host__ __device__ __forceinline__ uint32_t status_index(uint32_t status, uint32_t sleeps) { // battle.h:103-123
  if (!(status & 7)) return (uint32_t)__builtin_ctz(status) - 3;
  if (!(status & 0x80)) return 3 + sleeps;
  return 14 - (status & 7);
}

// Encode::Battle::Policy::get_index (encode/battle/policy.h:29-58) from the 184 bytes of a side
__device__ __forceinline__ uint32_t policy_index(const uint8_t *side, uint32_t choice) {
  const uint32_t kind = choice & 3, data = choice >> 2;
  if (kind == 1) {
    if (data == 0) return 0; // Struggle / forced continue: only ever a sole option (policy.h:11-19)
    const uint32_t sid = side[176] - 1u;
    const uint32_t mid = side[24 * sid + 10 + 2 * (data - 1)]; // side.stored().moves[data - 1].id
    return mid == 0 ? 0 : mid - 1;
  }
  if (kind == 2) {
    const uint32_t pid = side[176 + data - 1];
    return 164 + side[24 * (pid - 1) + 21] - 1u;
  }
  return 0;
}

} // namespace oak
