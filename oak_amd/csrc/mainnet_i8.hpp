// oak_amd/csrc/mainnet_i8.hpp -- the quantized ("discrete") main net on the i8 matrix pipe (included by leafnet.hip).
//
// Replaces NN::Battle::Quantized::MainNet<768, H, VH, PH> (nn/battle/quantized/main-net.h:98-150): the battle embedding as
// bytes (static_cast<uint8_t>(127 f), network.h:131-175 / cache.h:62-126), fc0 -> crelu -> fc1 -> crelu -> value_fc2 -> crelu
// -> value_fc3 in int32, sigmoid(acc / 8128).  Integer arithmetic throughout, so the result is the reference's bit for bit:
//   k_mainnet_i8<H>  one wave owns 32 leaves; the three dense layers on v_mfma_i32_32x32x32_i8 with the WEIGHTS as the A
//                    operand (rows = output features) and the leaves' bytes as the B operand, so every layer's result has the
//                    leaf on the lane and its features in the 16 accumulator registers of each 32-wide block -- crelu'd and
//                    packed four to a register they are the next layer's B operand as they stand (k-step = block, byte j of
//                    lane half h = feature (j & 3) + 8 (j >> 2) + 4 h; the weight fragments are laid out in the same order).
//                    The weights of the three layers live in LDS (at most 128 KB), staged once per workgroup.
//   k_policy_i8      the policy heads (main-net.h:127-143): fc2 + crelu per head, then the <= 9 legal rows of fc3, on v_dot4.
//
// fc0's input bytes are UNSIGNED (0..255) and _mm256_maddubs_epi16 saturates each pair u[2k] w[2k] + u[2k+1] w[2k+1] to int16
// (simd.h:31-38); the matrix pipe multiplies signed bytes and never saturates.  So a byte is split u = (u & 127) + 128 (u >> 7):
// the low parts go through one MFMA, and where any byte of a k-step is above 127 (wave-uniform test) the high bits go through two
// more as 64 (u >> 7) each.  That is the exact unsaturated dot product; then every pair that CAN saturate (|w| <= 127, so
// u[2k] + u[2k+1] >= 259) gets its exact correction sat16(p) - p added per output on the vector ALU, the weights read back from
// LDS.  Inputs of fc1 / value_fc2 / value_fc3 are crelu outputs (<= 127): 2 x 127 x 127 < 32767, those never saturate.
#pragma once
#include "net_layout.hpp" // QI_IN, QI_T0, qi_lds_bytes

namespace oak {

constexpr int QI_BLOCK = 256;       // four waves, 32 leaves each
constexpr int QI_ROWS = 315;        // policy rows (policy.h); fc3 is padded to 320 (main-net.h:53-66)
typedef __attribute__((ext_vector_type(4))) int qi32x4;
typedef __attribute__((ext_vector_type(16))) int qi32x16;

struct QNetDev {
  const uint8_t *img;               // fc0 | fc1 | value_fc2 in k_mainnet_i8's fragment order (qnet_image), img_bytes long
  const int32_t *b0, *b1, *b2;      // biases: H, H, VH
  const int8_t *w3;                 // value_fc3's VH weights
  int32_t b3;
  const int8_t *pw2[2];             // policy fc2 of each head, [PH][H] row-major
  const int32_t *pb2[2];
  const int8_t *pw3[2];             // policy fc3 of each head, [320][PH] row-major (rows 315..319 zero)
  const int32_t *pb3[2];
  int H, VH, PH, img_bytes;
};
struct QMainArgs {
  QNetDev q;
  const float *emb;   // n x 768 fp32 battle embeddings (the embedding passes' output)
  uint32_t n;
  float *values;      // nullable
  uint8_t *h1;        // nullable: n x H crelu'd fc1 bytes, the policy heads' input
  uint8_t *q_emb;     // nullable: n x 768 embedding bytes (diagnostic)
  int32_t *value_acc; // nullable: value_fc3's int32 (diagnostic)
};

// static_cast<uint8_t>(127 * f) as the reference's g++ builds compile it (vcvttps2dq, then the low byte): values outside int32 --
// and NaN -- become 0x80000000, i.e. 0.  (C++ leaves every result >= 256 undefined)
__device__ __forceinline__ uint32_t quant_byte(float f) {
  const float v = 127.0f * f;
  const int32_t i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : INT32_MIN;
  return (uint32_t)i & 0xFFu;
}
// expf as glibc's (the reference's std::exp on a float): rounded from a double evaluation, so the sigmoid below is the reference's
// 1 / (1 + expf(-x)) to the last bit instead of within the few ulp two single-precision expf implementations may differ by
__device__ __forceinline__ float exp_f32(float x) { return (float)exp((double)x); }
__device__ __forceinline__ uint32_t crelu_i8(int32_t x) { return (uint32_t)min(max(x >> 6, 0), 127); } // clipped_relu.h:54-98

template <int H>
__global__ __launch_bounds__(QI_BLOCK) void k_mainnet_i8(QMainArgs a) {
  constexpr int NB = H / 32;
  extern __shared__ __align__(16) uint8_t lds_q[];
  const QNetDev &Q = a.q;
  for (int i = threadIdx.x; i < Q.img_bytes / 16; i += QI_BLOCK) ((uint4 *)lds_q)[i] = ((const uint4 *)Q.img)[i];
  __syncthreads();
  const qi32x4 *W0 = (const qi32x4 *)lds_q;
  const qi32x4 *W1 = W0 + QI_T0 * NB * 64;
  const qi32x4 *W2 = W1 + NB * NB * 64;
  const int NBv = Q.VH / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const uint32_t ntiles = (a.n + 31) / 32;
  for (uint32_t wt = blockIdx.x * (QI_BLOCK / 64) + wave; wt < ntiles; wt += gridDim.x * (QI_BLOCK / 64)) {
    const uint32_t row0 = wt * 32, n_rows = min(32u, a.n - row0);
    const bool valid = (uint32_t)r < n_rows;
    const uint32_t leaf = row0 + (valid ? (uint32_t)r : n_rows - 1); // rows past the batch repeat the last one, dropped below
    const float4 *erow = (const float4 *)(a.emb + (size_t)leaf * QI_IN) + 4 * h;
    qi32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = qi32x16{};
    // ---- fc0: lane (r, h) supplies bytes k = 32 t + 16 h + j of leaf r (the weight fragments use the same k per (h, j))
#pragma unroll 2
    for (int t = 0; t < QI_T0; ++t) {
      uint32_t U[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 f = erow[8 * t + i];
        U[i] = quant_byte(f.x) | quant_byte(f.y) << 8 | quant_byte(f.z) << 16 | quant_byte(f.w) << 24;
      }
      if (a.q_emb && valid) *(uint4 *)(a.q_emb + (size_t)leaf * QI_IN + 32 * t + 16 * h) = make_uint4(U[0], U[1], U[2], U[3]);
      const qi32x4 lo = {(int)(U[0] & 0x7F7F7F7Fu), (int)(U[1] & 0x7F7F7F7Fu), (int)(U[2] & 0x7F7F7F7Fu), (int)(U[3] & 0x7F7F7F7Fu)};
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(W0[(t * NB + b) * 64 + lane], lo, acc[b], 0, 0, 0);
      if (__ballot(((U[0] | U[1] | U[2] | U[3]) & 0x80808080u) != 0) == 0) continue;
      // bytes above 127: + 128 (u >> 7) as two MFMAs of 64 (u >> 7)
      const qi32x4 hi = {(int)(((U[0] >> 7) & 0x01010101u) * 0x40u), (int)(((U[1] >> 7) & 0x01010101u) * 0x40u),
                         (int)(((U[2] >> 7) & 0x01010101u) * 0x40u), (int)(((U[3] >> 7) & 0x01010101u) * 0x40u)};
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(W0[(t * NB + b) * 64 + lane], hi, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(W0[(t * NB + b) * 64 + lane], hi, acc[b], 0, 0, 0);
      }
      // pairs that can saturate: this lane's accumulators hold leaf r's outputs (j & 3) + 8 (j >> 2) + 4 h of every block, for
      // which the pairs of BOTH halves of the k-step matter -- the partner lane (r, 1 - h) supplies the other 16 bytes
      uint32_t F[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t P = (uint32_t)__shfl_xor((int)U[i], 32, 64);
        F[i] = h ? P : U[i];
        F[4 + i] = h ? U[i] : P;
      }
      uint32_t mask = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const uint32_t w2 = F[q >> 1] >> (16 * (q & 1));
        mask |= ((w2 & 0xFF) + ((w2 >> 8) & 0xFF) >= 259u ? 1u : 0u) << q;
      }
      while (__ballot(mask != 0) != 0) {
        if (mask) {
          const int q = __builtin_ctz(mask);
          mask &= mask - 1;
          const uint32_t w2 = F[q >> 1] >> (16 * (q & 1));
          const int u0 = (int)(w2 & 0xFF), u1 = (int)((w2 >> 8) & 0xFF);
          const int hk = q >> 3, jj = (2 * q) & 15; // the pair's lane half and byte in the fragments
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
              const int m = (j & 3) + 8 * (j >> 2) + 4 * h;
              const uint16_t wv = *(const uint16_t *)(lds_q + ((size_t)((t * NB + b) * 64 + m + 32 * hk) * 16 + jj));
              const int p = u0 * (int)(int8_t)(wv & 0xFF) + u1 * (int)(int8_t)(wv >> 8);
              acc[b][j] += min(max(p, -32768), 32767) - p;
            }
        }
      }
    }
    // ---- bias + crelu, packed as the next layer's B operand: block b = k-step b, byte 4 g + e = feature 32 b + 8 g + 4 h + e
    qi32x4 X[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int4 bv = *(const int4 *)(Q.b0 + 32 * b + 8 * g + 4 * h);
        X[b][g] = (int)(crelu_i8(acc[b][4 * g] + bv.x) | crelu_i8(acc[b][4 * g + 1] + bv.y) << 8 | crelu_i8(acc[b][4 * g + 2] + bv.z) << 16 |
                        crelu_i8(acc[b][4 * g + 3] + bv.w) << 24);
      }
    // ---- fc1
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      acc[b] = qi32x16{};
#pragma unroll
      for (int s = 0; s < NB; ++s) acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(W1[(s * NB + b) * 64 + lane], X[s], acc[b], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int4 bv = *(const int4 *)(Q.b1 + 32 * b + 8 * g + 4 * h);
        X[b][g] = (int)(crelu_i8(acc[b][4 * g] + bv.x) | crelu_i8(acc[b][4 * g + 1] + bv.y) << 8 | crelu_i8(acc[b][4 * g + 2] + bv.z) << 16 |
                        crelu_i8(acc[b][4 * g + 3] + bv.w) << 24);
        if (a.h1 && valid) *(uint32_t *)(a.h1 + (size_t)leaf * H + 32 * b + 8 * g + 4 * h) = (uint32_t)X[b][g];
      }
    // ---- value_fc2 (VH <= H outputs), crelu, value_fc3 on v_dot4 (the lane's half of the features, then its partner's)
    int part = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b >= NBv) break;
      qi32x16 v = qi32x16{};
#pragma unroll
      for (int s = 0; s < NB; ++s) v = __builtin_amdgcn_mfma_i32_32x32x32_i8(W2[(s * NBv + b) * 64 + lane], X[s], v, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int4 bv = *(const int4 *)(Q.b2 + 32 * b + 8 * g + 4 * h);
        const uint32_t y = crelu_i8(v[4 * g] + bv.x) | crelu_i8(v[4 * g + 1] + bv.y) << 8 | crelu_i8(v[4 * g + 2] + bv.z) << 16 |
                           crelu_i8(v[4 * g + 3] + bv.w) << 24;
        part = __builtin_amdgcn_sdot4(*(const int *)(Q.w3 + 32 * b + 8 * g + 4 * h), (int)y, part, false);
      }
    }
    part += __shfl_xor(part, 32, 64);
    const int32_t vacc = part + Q.b3;
    if (valid && h == 0) {
      if (a.value_acc) a.value_acc[leaf] = vacc;
      if (a.values) a.values[leaf] = 1.0f / (1.0f + exp_f32(-((float)vacc / 8128.0f)));
    }
  }
}

struct QPolicyArgs {
  QNetDev q;
  const uint8_t *h1; // n x H
  const uint8_t *battles;
  const uint8_t *choices[2]; // n x 9 each
  const uint8_t *counts[2];  // n each
  float *logits[2];          // n x 9 each
  uint32_t n;
};
// One wave per leaf and head: fc2 with lane c owning features c and c + 64, the crelu'd bytes through the wave's LDS row, then
// lane j < 9 the legal choice j's fc3 row (propagate_single, affine.h:173-184) / 8128.
__global__ __launch_bounds__(QI_BLOCK) void k_policy_i8(QPolicyArgs a) {
  __shared__ __align__(16) uint8_t h2s[QI_BLOCK / 64][128];
  const QNetDev &Q = a.q;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = Q.H, PH = Q.PH;
  for (uint32_t base = blockIdx.x * (QI_BLOCK / 64); base < a.n; base += gridDim.x * (QI_BLOCK / 64)) {
    const uint32_t leaf = base + wave;
    const bool live_leaf = leaf < a.n;
    const uint32_t lf = live_leaf ? leaf : a.n - 1;
    const int *hrow = (const int *)(a.h1 + (size_t)lf * H);
    for (int head = 0; head < 2; ++head) {
      for (int c = lane; c < PH; c += 64) {
        const int *wr = (const int *)(Q.pw2[head] + (size_t)c * H);
        int acc = Q.pb2[head][c];
        for (int k = 0; k < H / 4; ++k) acc = __builtin_amdgcn_sdot4(wr[k], hrow[k], acc, false);
        h2s[wave][c] = (uint8_t)crelu_i8(acc);
      }
      __syncthreads();
      if (lane < OAKGPU_MAX_CHOICES && live_leaf) {
        const uint32_t cnt = a.counts[head][lf];
        const bool live = (uint32_t)lane < cnt;
        uint32_t idx = live ? policy_index(a.battles + (size_t)lf * 384 + head * 184, a.choices[head][(size_t)lf * OAKGPU_MAX_CHOICES + lane]) : 0u;
        idx = idx < (uint32_t)QI_ROWS ? idx : 0u;
        const int *wr = (const int *)(Q.pw3[head] + (size_t)idx * PH);
        const int *hv = (const int *)h2s[wave];
        int acc = Q.pb3[head][idx];
        for (int k = 0; k < PH / 4; ++k) acc = __builtin_amdgcn_sdot4(wr[k], hv[k], acc, false);
        a.logits[head][(size_t)lf * OAKGPU_MAX_CHOICES + lane] = live ? (float)acc / 8128.0f : 0.0f;
      }
      __syncthreads();
    }
  }
}

} // namespace oak
