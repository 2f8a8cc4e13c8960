// oak_amd/csrc/party_key.hpp -- the bench-slot embedding table's key, its 240-variant enumeration and the stored identity of a
// Pokemon, on the 6 dwords of a stored Pokemon (stats 5 x u16 | 4 x {move id, pp} | hp u16 | status | species | types | level).
// One set of inline functions for the table's kernels (leafnet.hip) and for the host (oakgpu_party_key / oakgpu_party_variant).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode_index.hpp"

namespace oak {

constexpr uint32_t PARTY_KEYS = 240;      // NN::Battle::PokemonCache::n_embeddings (nn/battle/cache.h:21-28): 15 status x 16 has-PP
constexpr uint32_t PARTY_IDENT_WORDS = 6; // = TAG_WORDS of k_party_tags

// Encode::Battle::pokemon_key (encode/battle/key.h:22-30, 65-71): bit i = move slot i has PP; bits 4..7 = status index + 1, or 0
__host__ __device__ __forceinline__ uint32_t party_key(const uint32_t (&pk)[6], uint32_t sleep) {
  uint32_t key = ((pk[2] >> 24) ? 1u : 0u) | (((pk[3] >> 8) & 0xFF) ? 2u : 0u) | ((pk[3] >> 24) ? 4u : 0u) | (((pk[4] >> 8) & 0xFF) ? 8u : 0u);
  const uint32_t st = pk[5] & 0xFF;
  if (st) key |= (status_index(st, sleep) + 1) << 4;
  return key;
}

// The variant of `base` that PokemonCache::fill stores under `key` (cache.h:81-126): PP of move slot i = key & (1 << i); status
// None / PSN / BRN / FRZ / PAR with sleep 0, Sleep1 with public sleep turns 1..7 (status indices 4..10), Rest3 / Rest2 / Rest1
// (indices 11..13).  Only the four PP bytes and the status byte differ from the base.  False for key >= 240.
__host__ __device__ __forceinline__ bool party_variant(const uint32_t (&base)[6], uint32_t key, uint32_t (&out)[6], uint32_t &sleep) {
  const uint32_t m = key & 15, s = key >> 4;
  sleep = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = base[k];
  if (key >= PARTY_KEYS) return false;
  out[2] = (base[2] & 0x00FFFFFFu) | ((m & 1u) << 24);
  out[3] = (base[3] & 0x00FF00FFu) | ((m & 2u) << 8) | ((m & 4u) << 24);
  out[4] = (base[4] & 0xFFFF00FFu) | ((m & 8u) << 8);
  uint32_t st = 0;
  if (s >= 1 && s <= 4) st = 4u << s;                  // PSN 0x08, BRN 0x10, FRZ 0x20, PAR 0x40
  else if (s >= 5 && s <= 11) { st = 1; sleep = s - 4; } // Status::Sleep1, the public sleep turns carry the index
  else if (s >= 12) st = 0x80u | (15 - s);             // Rest3, Rest2, Rest1
  out[5] = (base[5] & 0xFFFFFF00u) | st;
  return true;
}

// What a stored Pokemon's 240 embeddings depend on and no variant changes: k_party_tags' tag words with the has-PP bits and the
// status field cleared (stats, move ids, species, types, level).  Word 2 of any Pokemon has a zero top byte, so the table marks an
// empty team slot (species 0) with PARTY_IDENT_EMPTY in every word: an identity no slot of a leaf can have.
constexpr uint32_t PARTY_IDENT_EMPTY = 0xFFFFFFFFu;
__host__ __device__ __forceinline__ void party_identity(const uint32_t (&pk)[6], uint32_t (&c)[6]) {
  c[0] = pk[0];
  c[1] = pk[1];
  c[2] = pk[2] & 0x00FFFFFFu;
  c[3] = pk[3] & 0x00FF00FFu;
  c[4] = pk[4] & 0x000000FFu;
  c[5] = pk[5] & 0xFFFFFF00u;
}

} // namespace oak
