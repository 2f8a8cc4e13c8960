// oak_amd/csrc/train_kernels.hpp -- the kernels the two trainers share (trainer.hip: the battle network; buildtrain.hip: the team-building
// network): the tiled fp32 GEMM in its three forms with the operand views it reads, the pairwise reduction of its dW|db partials and the
// elementwise Adam update.  What they compute, and in which order every sum runs, is described at the head of trainer.hip.  The kernels are
// `static` so that each translation unit that includes the header holds its own (as in game_rows.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/oakgpu.h"

namespace oak {
namespace tr {

constexpr uint32_t POKEMON_IN = 198, ACTIVE_IN = 229;
constexpr uint32_t CHAIN = 32;       // terms per accumulation chain (k_gemm: one K step)
constexpr uint32_t MID = 16;         // chains per middle sum
constexpr uint32_t SPAN = 256;       // K ranges of a dW|db GEMM are multiples of this
constexpr uint32_t MAX_SPLITS = 32;  // K ranges of a dW|db GEMM

// ---- a matrix as a GEMM operand reads it ---------------------------------------------------------------------------------------------
enum { V_PLAIN = 0, V_PARTY = 1, V_ACTIVE = 2 };
struct View {
  const float *p;         // PLAIN: rows x ld;  PARTY, ACTIVE: the batch's `pokemon`
  const float *p2;        // ACTIVE: the batch's `active`
  const uint8_t *status;  // nullable (PARTY, ACTIVE): a row reads as zeros when its batch row's status is not OK
  uint32_t rows, cols, ld, mode;
  uint32_t ones;          // column `cols` reads as 1 (the bias' column of dW|db)
};
// (the data load does not wait for the status byte: both are issued, then one is chosen -- every address of an in-range cell is valid)
__device__ __forceinline__ float view_at(const View &v, uint32_t r, uint32_t c) {
  if (r >= v.rows) return 0.0f;
  if (c >= v.cols) return (v.ones && c == v.cols) ? 1.0f : 0.0f;
  const float *src;
  uint32_t item = r;                                                                       // the batch row whose status counts
  if (v.mode == V_PARTY) src = v.p + ((size_t)(r / 5) * 6 + 1 + r % 5) * POKEMON_IN + c, item = r / 10;   // pokemon[:, :, 1:6]
  else if (v.mode == V_ACTIVE) src = c < ACTIVE_IN ? v.p2 + (size_t)r * ACTIVE_IN + c : v.p + (size_t)r * 6 * POKEMON_IN + (c - ACTIVE_IN), item = r / 2;
  else src = v.p + (size_t)r * v.ld + c;
  const float x = *src;
  const uint8_t st = v.status ? v.status[item] : (uint8_t)OAKGPU_REPLAY_OK;
  return st == OAKGPU_REPLAY_OK ? x : 0.0f;
}

enum { EPI_FWD = 0, EPI_DX = 1, EPI_DW = 2 };
enum { OUT_PLAIN = 0, OUT_PARTY = 1, OUT_ACTIVE = 2 };
struct GemmArgs {
  View a, b;
  uint32_t ta, tb;     // A(m, k) = ta ? a(k, m) : a(m, k);  B(k, n) = tb ? b(n, k) : b(k, n)
  uint32_t M, N, K;
  uint32_t epi;
  uint32_t klen;       // EPI_DW: K rows per blockIdx.z (a multiple of SPAN); otherwise K
  float *out;          // FWD: Y;  DX: dX;  DW: partials [splits][M][N]
  uint32_t ldo;
  // FWD
  const float *bias;
  uint32_t act;        // 0 none, 1 relu, 2 clamp[0, 1]
  float *deriv;        // nullable: M x N, the factor dZ = dY * deriv (activation derivative times hp mask)
  uint32_t place;      // OUT_PARTY / OUT_ACTIVE: Y goes into the battle embedding, times hp != 0
  uint32_t side, aod, pod;
  const float *hp;
  const uint8_t *status;
  // DX
  uint32_t accum;      // add to what `out` holds
  const float *mask;   // nullable: M x N factor
};

constexpr int BM = 64, BN = 64, BK = 32, PAD = 1;

static __global__ __launch_bounds__(256) void k_gemm(GemmArgs g) {
  __shared__ float As[BK][BM + PAD], Bs[BK][BN + PAD];
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const uint32_t wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const uint32_t kbeg = blockIdx.z * g.klen, kend = min(g.K, kbeg + g.klen);
  static_assert(BK == CHAIN, "one K step is one chain");
  f32x16 total, mid, acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) total[i] = 0.0f, mid[i] = 0.0f, acc[i] = 0.0f;
  uint32_t chains = 0;
  for (uint32_t kb = kbeg; kb < kend; kb += BK) {
    // A tile: the view's column index is the contiguous one, so neighbouring threads walk it
    for (uint32_t i = tid; i < BM * BK; i += 256) {
      uint32_t m, k;
      if (g.ta) m = i % BM, k = i / BM; else k = i % BK, m = i / BK;
      const uint32_t kk = kb + k;
      As[k][m] = kk < kend ? (g.ta ? view_at(g.a, kk, m0 + m) : view_at(g.a, m0 + m, kk)) : 0.0f;
    }
    for (uint32_t i = tid; i < BN * BK; i += 256) {
      uint32_t n, k;
      if (g.tb) k = i % BK, n = i / BK; else n = i % BN, k = i / BN;
      const uint32_t kk = kb + k;
      Bs[k][n] = kk < kend ? (g.tb ? view_at(g.b, n0 + n, kk) : view_at(g.b, kk, n0 + n)) : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < BK / 2; ++s) {
      const float av = As[2 * s + (lane >> 5)][wm + (lane & 31)];
      const float bv = Bs[2 * s + (lane >> 5)][wn + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
    // the chain ends: its sum joins the middle sum, and that one the total after MID chains
#pragma unroll
    for (int i = 0; i < 16; ++i) mid[i] += acc[i], acc[i] = 0.0f;
    if (++chains == MID) {
#pragma unroll
      for (int i = 0; i < 16; ++i) total[i] += mid[i], mid[i] = 0.0f;
      chains = 0;
    }
  }
  if (chains) {
#pragma unroll
    for (int i = 0; i < 16; ++i) total[i] += mid[i];
  }
  const uint32_t col = n0 + wn + (lane & 31);
  if (col >= g.N) return;
#pragma unroll
  for (uint32_t r = 0; r < 16; ++r) {
    const uint32_t row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row >= g.M) continue;
    float x = total[r];
    if (g.epi == EPI_DW) {
      g.out[((size_t)blockIdx.z * g.M + row) * g.N + col] = x;
    } else if (g.epi == EPI_DX) {
      const size_t o = (size_t)row * g.ldo + col;
      if (g.accum) x = g.out[o] + x;
      if (g.mask) x *= g.mask[(size_t)row * g.N + col];
      g.out[o] = x;
    } else {
      const float z = x + g.bias[col];
      float y = z, d = 1.0f;
      if (g.act == 1) y = fmaxf(z, 0.0f), d = z > 0.0f ? 1.0f : 0.0f;                       // torch.relu: no gradient at 0
      else if (g.act == 2) y = fminf(fmaxf(z, 0.0f), 1.0f), d = (z >= 0.0f && z <= 1.0f) ? 1.0f : 0.0f;  // torch.clamp: gradient at both ends
      size_t o = (size_t)row * g.ldo + col;
      if (g.place != OUT_PLAIN) {
        const uint32_t bs = g.place == OUT_PARTY ? row / 5 : row, slot = g.place == OUT_PARTY ? 1 + row % 5 : 0;
        const bool ok = g.status[bs / 2] == OAKGPU_REPLAY_OK;
        const float keep = (ok && g.hp[(size_t)bs * 6 + slot] != 0.0f) ? 1.0f : 0.0f;
        y = keep != 0.0f ? y : 0.0f;
        d *= keep;
        o = (size_t)bs * g.side + (g.place == OUT_PARTY ? (1 + g.aod) + (slot - 1) * (1 + g.pod) + 1 : 1) + col;
      }
      g.out[o] = y;
      if (g.deriv) g.deriv[(size_t)row * g.N + col] = d;
    }
  }
}

// partials [splits][count] -> grad: element e = m * (in + 1) + i is weight (m, i), or bias m at i == in.  Pairwise, fixed order.
static __global__ __launch_bounds__(256) void k_reduce(const float *partials, uint32_t splits, uint32_t out_dim, uint32_t in_dim, float *gb, float *gw) {
  const size_t count = (size_t)out_dim * (in_dim + 1);
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float v[MAX_SPLITS];
#pragma unroll
  for (uint32_t s = 0; s < MAX_SPLITS; ++s) v[s] = s < splits ? partials[s * count + e] : 0.0f;
#pragma unroll
  for (uint32_t stride = 1; stride < MAX_SPLITS; stride *= 2)
#pragma unroll
    for (uint32_t i = 0; i + stride < MAX_SPLITS; i += 2 * stride) v[i] += v[i + stride];
  const uint32_t m = (uint32_t)(e / (in_dim + 1)), i = (uint32_t)(e % (in_dim + 1));
  if (i == in_dim) gb[m] = v[0]; else gw[(size_t)m * in_dim + i] = v[0];
}

struct AdamArgs {
  float *p, *m, *v;
  const float *g;
  const uint8_t *kind;   // per parameter: group | 4 for a weight
  size_t count;
  float b1, omb1, b2, omb2, eps;
  float step_size[3], bc2_sqrt[3];   // lr / (1 - b1^t), sqrt(1 - b2^t) per group
  uint32_t groups;       // bit g: group g is updated
  uint32_t clamp;
  const oakgpu_train_report *gate;  // nullable: nothing moves when gate->rows == 0, and `skipped` counts the call per group
  uint32_t *skipped;
};
static __global__ __launch_bounds__(256) void k_adam(AdamArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (a.gate && a.gate->rows == 0) {
    if (i == 0)
      for (uint32_t g = 0; g < 3; ++g) if (a.groups >> g & 1) a.skipped[g] += 1;
    return;
  }
  if (i >= a.count) return;
  const uint32_t kind = a.kind[i], grp = kind & 3;
  if (!(a.groups >> grp & 1)) return;
  const float g = a.g[i];
  const float m = fmaf(a.b1, a.m[i], a.omb1 * g);
  const float v = fmaf(a.b2, a.v[i], (a.omb2 * g) * g);
  const float denom = sqrtf(v) / a.bc2_sqrt[grp] + a.eps;
  float p = a.p[i] - a.step_size[grp] * (m / denom);
  if (a.clamp && (kind & 4)) p = fminf(fmaxf(p, -2.0f), 2.0f);
  a.m[i] = m;
  a.v[i] = v;
  a.p[i] = p;
}

}  // namespace tr
}  // namespace oak
