// oak_amd/csrc/trainer.hip -- the optimiser step of the battle network on the device: forward on training rows, battle.py's loss,
// its exact gradient and torch.optim.Adam's update (the contract is in include/oakgpu.h, "Training the battle network").
//
// (k_gemm, k_reduce and k_adam live in train_kernels.hpp, which buildtrain.hip includes too.)
//   k_gemm        : one tiled fp32 GEMM on v_mfma_f32_32x32x2_f32 (64 x 64 tile per workgroup, four waves of 32 x 32, K in steps of 32
//                   through LDS) in three forms: Y = act(X W^T + b) with the bias / activation / hp-mask epilogue and the derivative's
//                   0/1 factor kept next to Y; dX = dY W with the optional sum into dX and the derivative factor; dW|db = dY^T [X|1] as
//                   partial sums per K range.  Every accumulation chain is cut after 32 terms (one K step): the chain's sum joins a middle
//                   sum, which after 16 chains joins the running total, and both start at zero again -- a 256-term chain alone already
//                   spends the 2e-7 S of the gradient bound on a bias.
//   k_reduce      : the partials of dW|db combined pairwise in a fixed order into the gradient block
//   k_side_hp     : the hp cells of the battle embedding;  k_embed_grad: the embedding cells of its gradient times the kept factor
//   k_logits      : the <= 9 legal logits per side (the rows of fc3 that choice_indices names)
//   k_count_rows, k_loss, k_report : OK rows; value / softmax / loss terms and their gradients per row; the report
//   k_adam        : one elementwise launch over the whole parameter block with the group rule
//   k_symmetries  : battle.py's permute_sides / permute_pokemon on the encoded rows in place, one workgroup per row, a fast_prng stream per row
// No float atomics anywhere: every sum runs in a fixed order, so a call's bits depend on its inputs alone.  There is no CPU fallback.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/oakgpu.h"
#include "fast_prng.hpp"
#include "oakgpu_internal.h"
#include "train_kernels.hpp"   // k_gemm, k_reduce, k_adam and the operand views: shared with buildtrain.hip

namespace oak {
namespace tr {

constexpr uint32_t ACTIVE_POKEMON_IN = 427, POLICY_OUT = 315, MAXC = 9;
constexpr int N_LAYERS = 12;
enum { L_P0, L_P1, L_A0, L_A1, L_FC0, L_FC1, L_V2, L_V3, L_Q1A, L_Q1B, L_Q2A, L_Q2B };
enum { G_TRUNK = 0, G_VALUE = 1, G_POLICY = 2 };

// the hp cells of the battle embedding [n][2][side]: slot 0 in front of the active's embedding, slots 1..5 in front of each party embedding
__global__ __launch_bounds__(256) void k_side_hp(const float *hp, const uint8_t *status, uint32_t n, uint32_t side, uint32_t aod, uint32_t pod, float *E) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * 12) return;
  const uint32_t bs = i / 6, slot = i % 6;
  const float x = status[bs / 2] == OAKGPU_REPLAY_OK ? hp[i] : 0.0f;
  E[(size_t)bs * side + (slot == 0 ? 0 : (1 + aod) + (slot - 1) * (1 + pod))] = x;
}

// dZ of an embedding net's second layer: the battle embedding's gradient cell times the kept factor
__global__ __launch_bounds__(256) void k_embed_grad(const float *dE, const float *deriv, uint32_t rows, uint32_t width, uint32_t party, uint32_t side, uint32_t aod,
                                                    uint32_t pod, float *dZ) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * width) return;
  const uint32_t r = (uint32_t)(i / width), c = (uint32_t)(i % width);
  const uint32_t bs = party ? r / 5 : r;
  const size_t o = (size_t)bs * side + (party ? (1 + aod) + (r % 5) * (1 + pod) + 1 : 1) + c;
  dZ[i] = dE[o] * deriv[i];
}

struct RowArgs {
  oakgpu_encoded_frames f;
  oakgpu_train_loss loss;
  oakgpu_train_outputs out;
  uint32_t n, ph, want_grads;
  const float *yq[2];     // each head's hidden layer [n][ph]
  const float *wq[2];     // fc3 weights [315][ph]
  const float *bq[2];
  const float *zv;        // [n] value pre-sigmoid
  float *logits;          // [n][2][9]
  float *terms;           // [n][3]: sq_err, ce1, ce2
  float *dzv;             // [n]
  float *dl[2];           // [n][315] each, zeroed before the launch
  oakgpu_train_report *report;
};

__device__ __forceinline__ uint32_t legal_count(const RowArgs &a, uint32_t row, uint32_t s) { return min((uint32_t)a.f.k[row * 2 + s], MAXC); }
__device__ __forceinline__ bool legal_index(int64_t idx) { return idx >= 0 && idx < (int64_t)POLICY_OUT; }

__global__ __launch_bounds__(256) void k_logits(RowArgs a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n * 2 * MAXC) return;
  const uint32_t row = i / (2 * MAXC), s = (i / MAXC) & 1, j = i % MAXC;
  float l = 0.0f;
  if (a.f.status[row] == OAKGPU_REPLAY_OK && j < legal_count(a, row, s)) {
    const int64_t idx = a.f.choice_indices[i];
    if (legal_index(idx)) {
      const float *w = a.wq[s] + (size_t)idx * a.ph, *y = a.yq[s] + (size_t)row * a.ph;
      float tot = 0.0f, acc = 0.0f;
      for (uint32_t c = 0; c < a.ph; ++c) {
        acc = fmaf(y[c], w[c], acc);
        if ((c + 1) % CHAIN == 0) tot += acc, acc = 0.0f;
      }
      l = (tot + acc) + a.bq[s][idx];
    }
  }
  a.logits[i] = l;
}

__global__ __launch_bounds__(256) void k_count_rows(const uint8_t *status, uint32_t n, oakgpu_train_report *report) {
  __shared__ uint32_t part[256];
  uint32_t c = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 256) c += status[i] == OAKGPU_REPLAY_OK;
  part[threadIdx.x] = c;
  __syncthreads();
  for (uint32_t s = 128; s; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) report->rows = part[0];
}

__global__ __launch_bounds__(256) void k_loss(RowArgs a) {
  const uint32_t row = blockIdx.x * 256 + threadIdx.x;
  if (row >= a.n) return;
  const bool ok = a.f.status[row] == OAKGPU_REPLAY_OK;
  float value = 0.0f, sq = 0.0f, ce[2] = {0.0f, 0.0f}, dzv = 0.0f;
  float lg[2][MAXC];
#pragma unroll
  for (uint32_t s = 0; s < 2; ++s)
#pragma unroll
    for (uint32_t j = 0; j < MAXC; ++j) lg[s][j] = a.logits[(size_t)row * 2 * MAXC + s * MAXC + j];
  if (ok) {
    const float inv_rows = 1.0f / (float)a.report->rows;   // (rows >= 1: this row is OK)
    value = 1.0f / (1.0f + expf(-a.zv[row]));
    const float vt = (a.loss.wn * a.f.nash_value[row] + a.loss.we * a.f.empirical_value[row]) + a.loss.ws * a.f.score[row];
    const float d = value - vt;
    sq = d * d;
    dzv = ((a.loss.value_weight * 2.0f) * d * inv_rows) * (value * (1.0f - value));
#pragma unroll
    for (uint32_t s = 0; s < 2; ++s) {
      const uint32_t k = legal_count(a, row, s);
      float mx = -INFINITY;
#pragma unroll
      for (uint32_t j = 0; j < MAXC; ++j) if (j < k) mx = fmaxf(mx, lg[s][j]);
      float ex[MAXC], t[MAXC], sum = 0.0f, tsum = 0.0f, dot = 0.0f;
      uint32_t support = 0;
#pragma unroll
      for (uint32_t j = 0; j < MAXC; ++j) {
        ex[j] = j < k ? expf(lg[s][j] - mx) : 0.0f;
        sum += ex[j];
        const size_t o = (size_t)row * 2 * MAXC + s * MAXC + j;
        t[j] = j < k ? (1.0f - a.loss.pn) * a.f.empirical_policies[o] + a.loss.pn * a.f.nash_policies[o] : 0.0f;
        support += t[j] != 0.0f;
        tsum += t[j];
      }
      const float lsum = logf(sum), fsup = (float)max(support, 1u);
#pragma unroll
      for (uint32_t j = 0; j < MAXC; ++j) if (j < k) dot += -t[j] * ((lg[s][j] - mx) - lsum);
      ce[s] = dot / fsup;
      if (a.want_grads && a.loss.policy_weight != 0.0f) {
        const float scale = (a.loss.policy_weight * inv_rows) / fsup;
#pragma unroll
        for (uint32_t j = 0; j < MAXC; ++j) {
          if (j >= k) continue;
          const int64_t idx = a.f.choice_indices[(size_t)row * 2 * MAXC + s * MAXC + j];
          if (legal_index(idx)) a.dl[s][(size_t)row * POLICY_OUT + idx] += scale * ((ex[j] / sum) * tsum - t[j]);
        }
      }
    }
  }
  a.terms[(size_t)row * 3 + 0] = sq;
  a.terms[(size_t)row * 3 + 1] = ce[0];
  a.terms[(size_t)row * 3 + 2] = ce[1];
  if (a.want_grads) a.dzv[row] = dzv;
  if (a.out.value) a.out.value[row] = value;
  if (a.out.sq_err) a.out.sq_err[row] = sq;
  if (a.out.ce) a.out.ce[row * 2] = ce[0], a.out.ce[row * 2 + 1] = ce[1];
  if (a.out.logits)
#pragma unroll
    for (uint32_t j = 0; j < 2 * MAXC; ++j) a.out.logits[(size_t)row * 2 * MAXC + j] = ok ? lg[j / MAXC][j % MAXC] : 0.0f;
}

// the report: float64 sums of the rows' terms, thread t adding rows t, t + 256, ... and the 256 sums combined pairwise
__global__ __launch_bounds__(256) void k_report(const float *terms, uint32_t n, oakgpu_train_loss loss, oakgpu_train_report *report) {
  __shared__ double part[3][256];
  double s[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = threadIdx.x; i < n; i += 256)
    for (int c = 0; c < 3; ++c) s[c] += (double)terms[(size_t)i * 3 + c];
  for (int c = 0; c < 3; ++c) part[c][threadIdx.x] = s[c];
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (threadIdx.x < w)
      for (int c = 0; c < 3; ++c) part[c][threadIdx.x] += part[c][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double rows = (double)report->rows, inv = rows > 0.0 ? 1.0 / rows : 0.0;
    report->mse = part[0][0] * inv;
    report->ce_p1 = part[1][0] * inv;
    report->ce_p2 = part[2][0] * inv;
    report->loss = (double)loss.value_weight * report->mse + (double)loss.policy_weight * (report->ce_p1 + report->ce_p2);
  }
}

// ---- the symmetries: row i draws from fast_prng seeded seed + i: one uniform_64 whose lowest bit flips the sides, then four more for a
// Fisher-Yates permutation of the bench slots (q = 4 .. 1: slot q <-> slot draw % (q + 1)), the same on both sides.  new[s][slot] =
// old[s ^ flip][source(slot)]; hp moves with its Pokemon.  A row that is not OK is left as it is.
struct SymArgs {
  oakgpu_encoded_frames f;
  uint32_t n, flip_sides, permute_bench;
  uint64_t seed;
};
__global__ __launch_bounds__(64) void k_symmetries(SymArgs a) {
  __shared__ float buf[2 * 6 * POKEMON_IN];
  const uint32_t row = blockIdx.x, tid = threadIdx.x;
  if (a.f.status[row] != OAKGPU_REPLAY_OK) return;
  FastPrng g;
  g.seed(a.seed + row);
  uint32_t draws[5];
#pragma unroll
  for (uint32_t i = 0; i < 5; ++i) {
    const uint32_t hi = g.next32(), lo = g.next32();
    draws[i] = (uint32_t)((((uint64_t)hi << 32) | lo) % (i == 0 ? 2u : 6u - i));   // i = 1 .. 4: q + 1 = 5 .. 2
  }
  const uint32_t flip = a.flip_sides ? draws[0] : 0;
  uint32_t src[6] = {0, 1, 2, 3, 4, 5};                                             // src[slot]: where the slot's new content comes from
  if (a.permute_bench)
#pragma unroll
    for (uint32_t q = 4; q >= 1; --q) {
      const uint32_t j = draws[5 - q], t = src[1 + q];
      src[1 + q] = src[1 + j];
      src[1 + j] = t;
    }
  // pokemon [2][6][198] and hp [2][6] through LDS
  float *pk = a.f.pokemon + (size_t)row * 2 * 6 * POKEMON_IN;
  for (uint32_t i = tid; i < 2 * 6 * POKEMON_IN; i += 64) buf[i] = pk[i];
  __syncthreads();
  for (uint32_t i = tid; i < 2 * 6 * POKEMON_IN; i += 64) {
    const uint32_t s = i / (6 * POKEMON_IN), slot = (i / POKEMON_IN) % 6, c = i % POKEMON_IN;
    pk[i] = buf[((s ^ flip) * 6 + src[slot]) * POKEMON_IN + c];
  }
  __syncthreads();
  float *hp = a.f.hp + (size_t)row * 12;
  if (tid < 12) buf[tid] = hp[tid];
  __syncthreads();
  if (tid < 12) hp[tid] = buf[((tid / 6) ^ flip) * 6 + src[tid % 6]];
  if (!flip) return;
  // the side axis alone: active [2][229], choice_indices / policies [2][9], k [2]; the value targets become 1 - x
  float *act = a.f.active + (size_t)row * 2 * ACTIVE_IN;
  for (uint32_t i = tid; i < ACTIVE_IN; i += 64) {
    const float t = act[i];
    act[i] = act[ACTIVE_IN + i];
    act[ACTIVE_IN + i] = t;
  }
  if (tid < MAXC) {
    const size_t o = (size_t)row * 2 * MAXC + tid;
    const int64_t ci = a.f.choice_indices[o];
    a.f.choice_indices[o] = a.f.choice_indices[o + MAXC];
    a.f.choice_indices[o + MAXC] = ci;
    float t = a.f.empirical_policies[o];
    a.f.empirical_policies[o] = a.f.empirical_policies[o + MAXC];
    a.f.empirical_policies[o + MAXC] = t;
    t = a.f.nash_policies[o];
    a.f.nash_policies[o] = a.f.nash_policies[o + MAXC];
    a.f.nash_policies[o + MAXC] = t;
  }
  if (tid == 0) {
    const uint8_t k0 = a.f.k[row * 2];
    a.f.k[row * 2] = a.f.k[row * 2 + 1];
    a.f.k[row * 2 + 1] = k0;
    a.f.empirical_value[row] = 1.0f - a.f.empirical_value[row];
    a.f.nash_value[row] = 1.0f - a.f.nash_value[row];
    a.f.score[row] = 1.0f - a.f.score[row];
  }
}

}  // namespace tr
}  // namespace oak

using namespace oak::tr;

// ---- the trainer -----------------------------------------------------------------------------------------------------------------------
struct TrainLayer { uint32_t in = 0, out = 0; size_t b = 0, w = 0; };   // offsets into the parameter block, in floats
struct NetShape {
  uint8_t header[8];
  uint32_t act = 0;   // 1 relu, 2 clamp
  TrainLayer L[N_LAYERS];
  size_t count = 0;
  uint32_t ph, pod, ah, aod, side, H, VH, PH;
};

struct oakgpu_trainer {
  oakgpu_ctx *ctx = nullptr;
  NetShape s;
  uint32_t max_rows = 0;
  float *block = nullptr;   // params | grads | m | v, each s.count floats
  uint8_t *kind = nullptr;
  float *work = nullptr;    // every workspace, carved below
  oakgpu_train_report *report = nullptr;
  uint32_t *skipped = nullptr;
  uint64_t t[3] = {0, 0, 0};
  uint32_t last_groups = 0;
  // workspaces (floats)
  float *y[N_LAYERS] = {}, *d[N_LAYERS] = {}, *dz[N_LAYERS] = {};
  float *E = nullptr, *dE = nullptr, *logits = nullptr, *terms = nullptr, *dl[2] = {}, *partials = nullptr, *dy1 = nullptr;
  float *params() const { return block; }
  float *grads() const { return block + s.count; }
  float *m() const { return block + 2 * s.count; }
  float *v() const { return block + 3 * s.count; }
};

static const char *const LAYER_NAMES[N_LAYERS] = {"pokemon_net.fc0", "pokemon_net.fc1", "active_net.fc0", "active_net.fc1", "main_net.fc0", "main_net.fc1",
                                                  "value_fc2", "value_fc3", "p1_policy_fc2", "p1_policy_fc3", "p2_policy_fc2", "p2_policy_fc3"};

static int parse_shape(const uint8_t *bytes, size_t size, NetShape &s) {
  if (!bytes) return oakgpu_fail_msg("trainer: null network bytes");
  if (size < 8) return oakgpu_fail_msg("trainer: network file: truncated header");
  memcpy(s.header, bytes, 8);
  s.act = (uint32_t)bytes[0] + 1;
  if (s.act != 1 && s.act != 2) return oakgpu_fail_msg("trainer: network file: unknown activation byte");
  size_t p = 8, count = 0;
  for (int i = 0; i < N_LAYERS; ++i) {
    if (size - p < 8) return oakgpu_fail_msg((std::string("trainer: network file: truncated in front of ") + LAYER_NAMES[i]).c_str());
    uint32_t dims[2];
    memcpy(dims, bytes + p, 8);
    p += 8;
    if (dims[0] == 0 || dims[1] == 0 || dims[0] > 4096 || dims[1] > 4096)
      return oakgpu_fail_msg((std::string("trainer: network file: implausible dims of ") + LAYER_NAMES[i]).c_str());
    const size_t floats = (size_t)dims[1] * (dims[0] + 1);
    if ((size - p) / 4 < floats) return oakgpu_fail_msg((std::string("trainer: network file: truncated inside ") + LAYER_NAMES[i]).c_str());
    s.L[i].in = dims[0], s.L[i].out = dims[1];
    s.L[i].b = count, s.L[i].w = count + dims[1];
    count += floats;
    p += 4 * floats;
  }
  if (p != size) return oakgpu_fail_msg("trainer: network file: trailing bytes");
  s.count = count;
  const TrainLayer *L = s.L;
  if (L[L_P0].in != POKEMON_IN || L[L_A0].in != ACTIVE_POKEMON_IN) return oakgpu_fail_msg("trainer: embedding input dims must be 198 / 427");
  if (L[L_P0].out > 128 || L[L_P1].out > 128 || L[L_A0].out > 128 || L[L_A1].out > 128) return oakgpu_fail_msg("trainer: embedding widths above 128 unsupported");
  s.ph = L[L_P0].out, s.pod = L[L_P1].out, s.ah = L[L_A0].out, s.aod = L[L_A1].out;
  s.side = (1 + s.aod) + 5 * (1 + s.pod);
  s.H = L[L_FC0].out, s.VH = L[L_V2].out, s.PH = L[L_Q1A].out;
  if (L[L_P1].in != s.ph || L[L_A1].in != s.ah || L[L_FC1].in != s.H || L[L_V2].in != s.H || L[L_V3].in != s.VH || L[L_Q1A].in != s.H || L[L_Q2A].in != s.H ||
      L[L_Q1B].in != s.PH || L[L_Q2B].in != L[L_Q2A].out)
    return oakgpu_fail_msg("trainer: network file: inconsistent layer dims");
  if (L[L_FC0].in != 2 * s.side) return oakgpu_fail_msg("trainer: network file: fc0 input != 2 * side embedding");
  if (L[L_FC1].out != s.H) return oakgpu_fail_msg("trainer: network file: fc0/fc1 widths differ");
  if (s.H > 256 || s.VH > 256) return oakgpu_fail_msg("trainer: main-net widths above 256 unsupported");
  if (L[L_FC0].in % 4) return oakgpu_fail_msg("trainer: embedding dim must be a multiple of 4");
  if (L[L_V3].out != 1 || L[L_Q1B].out != POLICY_OUT || L[L_Q2B].out != POLICY_OUT || L[L_Q2A].out != s.PH)
    return oakgpu_fail_msg("trainer: network file: inconsistent value / policy-head dims");
  if (s.PH > 256) return oakgpu_fail_msg("trainer: policy hidden width above 256 unsupported");
  return 0;
}

static int check_loss(const oakgpu_train_loss *loss) {
  if (!loss) return oakgpu_fail_msg("trainer: null loss parameters");
  if (loss->value_weight == 0.0f && loss->policy_weight == 0.0f) return oakgpu_fail_msg("trainer: value_weight and policy_weight are both zero");
  return 0;
}

extern "C" int oakgpu_trainer_check(const uint8_t *net, size_t size, uint32_t max_rows, uint32_t n, const oakgpu_train_loss *loss) {
  NetShape s;
  if (int rc = parse_shape(net, size, s)) return rc;
  if (max_rows == 0 || max_rows > (1u << 20)) return oakgpu_fail_msg("trainer: max_rows must be in 1 .. 1,048,576");
  if (n > max_rows) return oakgpu_fail_msg(("trainer: n = " + std::to_string(n) + " rows exceed max_rows = " + std::to_string(max_rows)).c_str());
  if (loss) return check_loss(loss);
  return 0;
}

static uint32_t splits_of(uint32_t rows) { return std::min<uint32_t>((rows + SPAN - 1) / SPAN, MAX_SPLITS); }
static uint32_t rows_of(int layer, uint32_t n) { return layer <= L_P1 ? 10 * n : layer <= L_A1 ? 2 * n : n; }
static int group_of(int layer) { return layer <= L_FC1 ? G_TRUNK : layer <= L_V3 ? G_VALUE : G_POLICY; }

extern "C" void oakgpu_trainer_destroy(oakgpu_trainer *t) {
  if (!t) return;
  if (t->ctx) {
    oakgpu_ctx_enter(t->ctx);
    (void)hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(t->ctx));
  }
  (void)hipFree(t->block);
  (void)hipFree(t->kind);
  (void)hipFree(t->work);
  (void)hipFree(t->report);
  (void)hipFree(t->skipped);
  delete t;
}

extern "C" int oakgpu_trainer_create(oakgpu_ctx *ctx, const uint8_t *net, size_t size, uint32_t max_rows, oakgpu_trainer **out) {
  if (!ctx || !out) return oakgpu_fail_msg("oakgpu_trainer_create: null argument");
  if (int rc = oakgpu_trainer_check(net, size, max_rows, 0, nullptr)) return rc;
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  oakgpu_trainer *t = new oakgpu_trainer;
  t->ctx = ctx, t->max_rows = max_rows;
  parse_shape(net, size, t->s);
  const NetShape &s = t->s;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  auto fail = [&](int rc) { oakgpu_trainer_destroy(t); return rc; };
  if (int rc = dev_alloc(t->block, 4 * s.count)) return fail(rc);
  if (int rc = dev_alloc(t->kind, s.count)) return fail(rc);
  if (int rc = dev_alloc(t->report, 1)) return fail(rc);
  if (int rc = dev_alloc(t->skipped, 4)) return fail(rc);
  std::vector<float> params(s.count);
  std::vector<uint8_t> kind(s.count);
  size_t p = 8;
  for (int i = 0; i < N_LAYERS; ++i) {
    const size_t floats = (size_t)s.L[i].out * (s.L[i].in + 1);
    memcpy(params.data() + s.L[i].b, net + p + 8, 4 * floats);
    p += 8 + 4 * floats;
    for (size_t e = 0; e < floats; ++e) kind[s.L[i].b + e] = (uint8_t)(group_of(i) | (e >= s.L[i].out ? 4 : 0));
  }
  // workspaces
  const size_t N = max_rows;
  size_t total = 0;
  std::vector<std::pair<float **, size_t>> carve;
  auto want = [&](float *&ptr, size_t floats) { carve.push_back({&ptr, total}); total += (floats + 3) & ~(size_t)3; };
  size_t partial = 0;
  for (int i = 0; i < N_LAYERS; ++i) {
    const size_t cells = (size_t)rows_of(i, max_rows) * s.L[i].out;
    const bool own_y = i != L_P1 && i != L_A1 && i != L_Q1B && i != L_Q2B;   // those go into the battle embedding / are never dense
    if (own_y) want(t->y[i], cells);
    if (i != L_V3 && i != L_Q1B && i != L_Q2B) want(t->d[i], cells);
    if (i != L_Q1B && i != L_Q2B) want(t->dz[i], cells);
    partial = std::max(partial, (size_t)splits_of(rows_of(i, max_rows)) * s.L[i].out * (s.L[i].in + 1));
  }
  want(t->E, N * 2 * s.side);
  want(t->dE, N * 2 * s.side);
  want(t->dy1, N * s.H);
  want(t->logits, N * 2 * MAXC);
  want(t->terms, N * 3);
  want(t->dl[0], N * POLICY_OUT);
  want(t->dl[1], N * POLICY_OUT);
  want(t->partials, partial);
  if (int rc = dev_alloc(t->work, total)) return fail(rc);
  for (auto &c : carve) *c.first = t->work + c.second;
  t->dz[L_Q1B] = t->dl[0], t->dz[L_Q2B] = t->dl[1];
  hipError_t e = hipMemsetAsync(t->block, 0, 4 * s.count * sizeof(float), stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->work, 0, total * sizeof(float), stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->report, 0, sizeof(oakgpu_train_report), stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->skipped, 0, 16, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->block, params.data(), s.count * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->kind, kind.data(), s.count, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (the host vectors go away)
  if (e != hipSuccess) return fail(oakgpu_fail_hip((int)e, "oakgpu_trainer_create: upload"));
  *out = t;
  return 0;
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
static View plain(const float *p, uint32_t rows, uint32_t cols) {
  View v{};
  v.p = p, v.rows = rows, v.cols = cols, v.ld = cols, v.mode = V_PLAIN;
  return v;
}
// what layer `i` reads as its input X [rows_of(i)][in]
static View input_view(const oakgpu_trainer *t, const oakgpu_encoded_frames *f, int i, uint32_t n) {
  const NetShape &s = t->s;
  View v{};
  v.rows = rows_of(i, n), v.cols = s.L[i].in, v.ld = s.L[i].in;
  switch (i) {
    case L_P0: v.p = f->pokemon, v.mode = V_PARTY, v.status = f->status; break;
    case L_A0: v.p = f->pokemon, v.p2 = f->active, v.mode = V_ACTIVE, v.status = f->status; break;
    case L_P1: v.p = t->y[L_P0]; break;
    case L_A1: v.p = t->y[L_A0]; break;
    case L_FC0: v.p = t->E; break;
    case L_FC1: v.p = t->y[L_FC0]; break;
    case L_V2: case L_Q1A: case L_Q2A: v.p = t->y[L_FC1]; break;
    case L_V3: v.p = t->y[L_V2]; break;
    case L_Q1B: v.p = t->y[L_Q1A]; break;
    default: v.p = t->y[L_Q2A]; break;
  }
  return v;
}

static int launch_gemm(hipStream_t stream, const GemmArgs &g, uint32_t splits) {
  dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, splits);
  hipLaunchKernelGGL(k_gemm, grid, dim3(256), 0, stream, g);
  HIPCHK(hipGetLastError());
  return 0;
}

static int forward_layer(oakgpu_trainer *t, hipStream_t stream, const oakgpu_encoded_frames *f, int i, uint32_t n) {
  const NetShape &s = t->s;
  GemmArgs g{};
  g.a = input_view(t, f, i, n);
  g.b = plain(t->params() + s.L[i].w, s.L[i].out, s.L[i].in);
  g.ta = 0, g.tb = 1;
  g.M = g.a.rows, g.N = s.L[i].out, g.K = s.L[i].in, g.klen = g.K;
  g.epi = EPI_FWD;
  g.bias = t->params() + s.L[i].b;
  g.act = i == L_V3 ? 0 : s.act;
  g.deriv = t->d[i];
  g.out = t->y[i], g.ldo = g.N;
  if (i == L_P1 || i == L_A1) {
    g.place = i == L_P1 ? OUT_PARTY : OUT_ACTIVE;
    g.out = t->E, g.side = s.side, g.aod = s.aod, g.pod = s.pod, g.hp = f->hp, g.status = f->status;
  }
  return launch_gemm(stream, g, 1);
}

static RowArgs row_args(oakgpu_trainer *t, const oakgpu_encoded_frames *f, uint32_t n, const oakgpu_train_loss *loss, const oakgpu_train_outputs *out, bool grads) {
  const NetShape &s = t->s;
  RowArgs a{};
  a.f = *f, a.loss = *loss, a.n = n, a.ph = s.PH, a.want_grads = grads;
  if (out) a.out = *out;
  a.yq[0] = t->y[L_Q1A], a.yq[1] = t->y[L_Q2A];
  a.wq[0] = t->params() + s.L[L_Q1B].w, a.wq[1] = t->params() + s.L[L_Q2B].w;
  a.bq[0] = t->params() + s.L[L_Q1B].b, a.bq[1] = t->params() + s.L[L_Q2B].b;
  a.zv = t->y[L_V3], a.logits = t->logits, a.terms = t->terms, a.dzv = t->dz[L_V3], a.dl[0] = t->dl[0], a.dl[1] = t->dl[1];
  a.report = t->report;
  return a;
}

static int check_call(const char *who, oakgpu_ctx *ctx, oakgpu_trainer *t, const oakgpu_encoded_frames *f, uint32_t n, const oakgpu_train_loss *loss) {
  if (!ctx || !t || !f) return oakgpu_fail_msg((std::string(who) + ": null argument").c_str());
  if (t->ctx != ctx) return oakgpu_fail_msg((std::string(who) + ": the trainer belongs to another context").c_str());
  if (n > t->max_rows) return oakgpu_fail_msg((std::string(who) + ": n = " + std::to_string(n) + " rows exceed max_rows = " + std::to_string(t->max_rows)).c_str());
  if (int rc = check_loss(loss)) return rc;
  if (!f->pokemon || !f->active || !f->hp || !f->choice_indices || !f->k || !f->empirical_policies || !f->nash_policies || !f->empirical_value ||
      !f->nash_value || !f->score || !f->status)
    return oakgpu_fail_msg((std::string(who) + ": the rows lack a tensor the trainer reads").c_str());
  return oakgpu_ctx_enter(ctx);
}

// forward + loss terms (+ the gradients of the heads' outputs); the report is written at the end
static int run_forward(oakgpu_trainer *t, const oakgpu_encoded_frames *f, uint32_t n, const oakgpu_train_loss *loss, const oakgpu_train_outputs *out, bool grads) {
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(t->ctx);
  const NetShape &s = t->s;
  if (n) {
    hipLaunchKernelGGL(k_side_hp, dim3((n * 12 + 255) / 256), dim3(256), 0, stream, f->hp, f->status, n, s.side, s.aod, s.pod, t->E);
    for (int i : {L_P0, L_P1, L_A0, L_A1, L_FC0, L_FC1, L_V2, L_V3, L_Q1A, L_Q2A})
      if (int rc = forward_layer(t, stream, f, i, n)) return rc;
  }
  RowArgs a = row_args(t, f, n, loss, out, grads);
  hipLaunchKernelGGL(k_count_rows, dim3(1), dim3(256), 0, stream, f->status, n, t->report);
  if (n) {
    hipLaunchKernelGGL(k_logits, dim3((n * 2 * MAXC + 255) / 256), dim3(256), 0, stream, a);
    if (grads && loss->policy_weight != 0.0f) {
      HIPCHK(hipMemsetAsync(t->dl[0], 0, (size_t)n * POLICY_OUT * sizeof(float), stream));
      HIPCHK(hipMemsetAsync(t->dl[1], 0, (size_t)n * POLICY_OUT * sizeof(float), stream));
    }
    hipLaunchKernelGGL(k_loss, dim3((n + 255) / 256), dim3(256), 0, stream, a);
  }
  hipLaunchKernelGGL(k_report, dim3(1), dim3(256), 0, stream, t->terms, n, *loss, t->report);
  HIPCHK(hipGetLastError());
  return 0;
}

// dW|db of layer i from dz[i] and the layer's input
static int weight_grad(oakgpu_trainer *t, hipStream_t stream, const oakgpu_encoded_frames *f, int i, uint32_t n) {
  const NetShape &s = t->s;
  const uint32_t rows = rows_of(i, n), splits = splits_of(rows);
  GemmArgs g{};
  g.a = plain(t->dz[i], rows, s.L[i].out);
  g.b = input_view(t, f, i, n);
  g.b.ones = 1;
  g.ta = 1, g.tb = 0;
  g.M = s.L[i].out, g.N = s.L[i].in + 1, g.K = rows;
  g.klen = ((rows + splits - 1) / splits + SPAN - 1) / SPAN * SPAN;
  g.epi = EPI_DW, g.out = t->partials;
  if (int rc = launch_gemm(stream, g, splits)) return rc;
  const size_t count = (size_t)g.M * g.N;
  hipLaunchKernelGGL(k_reduce, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, stream, t->partials, splits, s.L[i].out, s.L[i].in, t->grads() + s.L[i].b,
                     t->grads() + s.L[i].w);
  HIPCHK(hipGetLastError());
  return 0;
}

// dX = dz[i] W_i into `out` (n rows of in_i), optionally added to it, optionally times a factor
static int input_grad(oakgpu_trainer *t, hipStream_t stream, int i, uint32_t n, float *out, bool accum, const float *mask) {
  const NetShape &s = t->s;
  GemmArgs g{};
  g.a = plain(t->dz[i], rows_of(i, n), s.L[i].out);
  g.b = plain(t->params() + s.L[i].w, s.L[i].out, s.L[i].in);
  g.M = g.a.rows, g.N = s.L[i].in, g.K = s.L[i].out, g.klen = g.K;
  g.epi = EPI_DX, g.out = out, g.ldo = g.N, g.accum = accum, g.mask = mask;
  return launch_gemm(stream, g, 1);
}

static int run_backward(oakgpu_trainer *t, const oakgpu_encoded_frames *f, uint32_t n, const oakgpu_train_loss *loss) {
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(t->ctx);
  const NetShape &s = t->s;
  const bool value = loss->value_weight != 0.0f, policy = loss->policy_weight != 0.0f;
  bool have = false;   // dy1 holds a sum already
  if (value) {
    if (int rc = weight_grad(t, stream, f, L_V3, n)) return rc;
    if (int rc = input_grad(t, stream, L_V3, n, t->dz[L_V2], false, t->d[L_V2])) return rc;
    if (int rc = weight_grad(t, stream, f, L_V2, n)) return rc;
    if (int rc = input_grad(t, stream, L_V2, n, t->dy1, false, policy ? nullptr : t->d[L_FC1])) return rc;
    have = true;
  }
  if (policy) {
    const int heads[2][2] = {{L_Q1A, L_Q1B}, {L_Q2A, L_Q2B}};
    for (int h = 0; h < 2; ++h) {
      const int a = heads[h][0], b = heads[h][1];
      if (int rc = weight_grad(t, stream, f, b, n)) return rc;
      if (int rc = input_grad(t, stream, b, n, t->dz[a], false, t->d[a])) return rc;
      if (int rc = weight_grad(t, stream, f, a, n)) return rc;
      if (int rc = input_grad(t, stream, a, n, t->dy1, have, h == 1 ? t->d[L_FC1] : nullptr)) return rc;
      have = true;
    }
  }
  // dy1 now holds dZ of fc1
  t->dz[L_FC1] = t->dy1;
  if (int rc = weight_grad(t, stream, f, L_FC1, n)) return rc;
  if (int rc = input_grad(t, stream, L_FC1, n, t->dz[L_FC0], false, t->d[L_FC0])) return rc;
  if (int rc = weight_grad(t, stream, f, L_FC0, n)) return rc;
  if (int rc = input_grad(t, stream, L_FC0, n, t->dE, false, nullptr)) return rc;
  const size_t pc = (size_t)10 * n * s.pod, ac = (size_t)2 * n * s.aod;
  hipLaunchKernelGGL(k_embed_grad, dim3((uint32_t)((pc + 255) / 256)), dim3(256), 0, stream, t->dE, t->d[L_P1], 10 * n, s.pod, 1u, s.side, s.aod, s.pod, t->dz[L_P1]);
  hipLaunchKernelGGL(k_embed_grad, dim3((uint32_t)((ac + 255) / 256)), dim3(256), 0, stream, t->dE, t->d[L_A1], 2 * n, s.aod, 0u, s.side, s.aod, s.pod, t->dz[L_A1]);
  HIPCHK(hipGetLastError());
  for (int e = 0; e < 2; ++e) {
    const int l0 = e ? L_A0 : L_P0, l1 = e ? L_A1 : L_P1;
    if (int rc = weight_grad(t, stream, f, l1, n)) return rc;
    if (int rc = input_grad(t, stream, l1, n, t->dz[l0], false, t->d[l0])) return rc;
    if (int rc = weight_grad(t, stream, f, l0, n)) return rc;
  }
  return 0;
}

static uint32_t groups_of(const oakgpu_train_loss *loss) {
  return 1u | (loss->value_weight != 0.0f ? 2u : 0u) | (loss->policy_weight != 0.0f ? 4u : 0u);
}

extern "C" int oakgpu_trainer_forward_dev(oakgpu_ctx *ctx, oakgpu_trainer *t, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss,
                                          const oakgpu_train_outputs *out) {
  if (int rc = check_call("oakgpu_trainer_forward_dev", ctx, t, rows, n, loss)) return rc;
  return run_forward(t, rows, n, loss, out, false);
}

// The gradient block of a group with a zero weight is left as it is (the group receives no gradient); with no OK row every dZ is zero
// and so is the block of the groups that do.
extern "C" int oakgpu_trainer_gradients_dev(oakgpu_ctx *ctx, oakgpu_trainer *t, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss) {
  if (int rc = check_call("oakgpu_trainer_gradients_dev", ctx, t, rows, n, loss)) return rc;
  if (int rc = run_forward(t, rows, n, loss, nullptr, true)) return rc;
  t->last_groups = groups_of(loss);
  if (n == 0) {   // nothing to launch over: the groups' gradients are zero
    hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
    for (int i = 0; i < N_LAYERS; ++i)
      if (t->last_groups >> group_of(i) & 1) HIPCHK(hipMemsetAsync(t->grads() + t->s.L[i].b, 0, (size_t)t->s.L[i].out * (t->s.L[i].in + 1) * sizeof(float), stream));
    return 0;
  }
  return run_backward(t, rows, n, loss);
}

static int run_adam(oakgpu_trainer *t, float lr, int clamp, uint32_t groups, bool gated) {
  if (!(lr >= 0.0f)) return oakgpu_fail_msg("trainer: lr must be a number >= 0");
  groups &= 7u;
  if (!groups) return oakgpu_fail_msg("trainer: no parameter group named");
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(t->ctx);
  AdamArgs a{};
  a.p = t->params(), a.g = t->grads(), a.m = t->m(), a.v = t->v(), a.kind = t->kind, a.count = t->s.count;
  const double b1 = 0.9, b2 = 0.999;
  a.b1 = (float)b1, a.omb1 = (float)(1.0 - b1), a.b2 = (float)b2, a.omb2 = (float)(1.0 - b2), a.eps = 1e-8f;
  for (int g = 0; g < 3; ++g) {
    if (!(groups >> g & 1)) continue;
    const double step = (double)++t->t[g];
    a.step_size[g] = (float)((double)lr / (1.0 - pow(b1, step)));
    a.bc2_sqrt[g] = (float)sqrt(1.0 - pow(b2, step));
  }
  a.groups = groups, a.clamp = clamp ? 1 : 0;
  a.gate = gated ? t->report : nullptr, a.skipped = t->skipped;
  hipLaunchKernelGGL(k_adam, dim3((uint32_t)((a.count + 255) / 256)), dim3(256), 0, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int oakgpu_trainer_adam_dev(oakgpu_ctx *ctx, oakgpu_trainer *t, float lr, int clamp_weights, uint32_t groups) {
  if (!ctx || !t) return oakgpu_fail_msg("oakgpu_trainer_adam_dev: null argument");
  if (t->ctx != ctx) return oakgpu_fail_msg("oakgpu_trainer_adam_dev: the trainer belongs to another context");
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  return run_adam(t, lr, clamp_weights, groups, false);
}

extern "C" int oakgpu_trainer_step_dev(oakgpu_ctx *ctx, oakgpu_trainer *t, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss, float lr,
                                       int clamp_weights) {
  if (int rc = oakgpu_trainer_gradients_dev(ctx, t, rows, n, loss)) return rc;
  return run_adam(t, lr, clamp_weights, groups_of(loss), true);
}

// the step counts as the device settled them: a gated update that found no OK row did not happen
static int settle(oakgpu_trainer *t) {
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(t->ctx);
  uint32_t skipped[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(skipped, t->skipped, 16, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (skipped[0] | skipped[1] | skipped[2]) {
    for (int g = 0; g < 3; ++g) t->t[g] -= std::min<uint64_t>(t->t[g], skipped[g]);
    HIPCHK(hipMemsetAsync(t->skipped, 0, 16, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  return 0;
}

extern "C" int oakgpu_trainer_report(oakgpu_ctx *ctx, oakgpu_trainer *t, oakgpu_train_report *out, uint64_t steps[3]) {
  if (!ctx || !t) return oakgpu_fail_msg("oakgpu_trainer_report: null argument");
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  if (out) HIPCHK(hipMemcpyAsync(out, t->report, sizeof *out, hipMemcpyDeviceToHost, stream));
  if (int rc = settle(t)) return rc;
  if (steps) memcpy(steps, t->t, sizeof t->t);
  return 0;
}

extern "C" int oakgpu_trainer_shape(const oakgpu_trainer *t, uint32_t dims[24], size_t *count, uint32_t *max_rows) {
  if (!t) return oakgpu_fail_msg("oakgpu_trainer_shape: null trainer");
  if (dims)
    for (int i = 0; i < N_LAYERS; ++i) dims[2 * i] = t->s.L[i].in, dims[2 * i + 1] = t->s.L[i].out;
  if (count) *count = t->s.count;
  if (max_rows) *max_rows = t->max_rows;
  return 0;
}

extern "C" int oakgpu_trainer_read(oakgpu_ctx *ctx, oakgpu_trainer *t, int which, float *host, size_t count) {
  if (!ctx || !t || !host) return oakgpu_fail_msg("oakgpu_trainer_read: null argument");
  if (which < 0 || which > 3) return oakgpu_fail_msg("oakgpu_trainer_read: which must be OAKGPU_TRAIN_PARAMETERS, _GRADIENTS, _M or _V");
  if (count != t->s.count) return oakgpu_fail_msg("oakgpu_trainer_read: count is not the trainer's parameter count");
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  HIPCHK(hipMemcpyAsync(host, t->block + (size_t)which * t->s.count, count * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

extern "C" int oakgpu_trainer_set_gradients(oakgpu_ctx *ctx, oakgpu_trainer *t, const float *host, size_t count) {
  if (!ctx || !t || !host) return oakgpu_fail_msg("oakgpu_trainer_set_gradients: null argument");
  if (count != t->s.count) return oakgpu_fail_msg("oakgpu_trainer_set_gradients: count is not the trainer's parameter count");
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  HIPCHK(hipMemcpyAsync(t->grads(), host, count * sizeof(float), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

extern "C" int oakgpu_trainer_net_bytes(oakgpu_ctx *ctx, oakgpu_trainer *t, uint8_t *out, size_t capacity, size_t *size) {
  if (!ctx || !t || !size) return oakgpu_fail_msg("oakgpu_trainer_net_bytes: null argument");
  const NetShape &s = t->s;
  *size = 8 + 8 * N_LAYERS + 4 * s.count;
  if (!out) return 0;
  if (capacity < *size) return oakgpu_fail_msg("oakgpu_trainer_net_bytes: the buffer is too small");
  std::vector<float> params(s.count);
  if (int rc = oakgpu_trainer_read(ctx, t, OAKGPU_TRAIN_PARAMETERS, params.data(), s.count)) return rc;
  memcpy(out, s.header, 8);
  size_t p = 8;
  for (int i = 0; i < N_LAYERS; ++i) {
    const uint32_t dims[2] = {s.L[i].in, s.L[i].out};
    const size_t floats = (size_t)s.L[i].out * (s.L[i].in + 1);
    memcpy(out + p, dims, 8);
    memcpy(out + p + 8, params.data() + s.L[i].b, 4 * floats);
    p += 8 + 4 * floats;
  }
  return 0;
}

extern "C" int oakgpu_frames_symmetries_dev(oakgpu_ctx *ctx, const oakgpu_encoded_frames *rows, uint32_t n, uint64_t seed, int flip_sides, int permute_bench) {
  if (!ctx || !rows) return oakgpu_fail_msg("oakgpu_frames_symmetries_dev: null argument");
  const oakgpu_encoded_frames *f = rows;
  if (!f->pokemon || !f->active || !f->hp || !f->choice_indices || !f->k || !f->empirical_policies || !f->nash_policies || !f->empirical_value ||
      !f->nash_value || !f->score || !f->status)
    return oakgpu_fail_msg("oakgpu_frames_symmetries_dev: the rows lack a tensor the symmetries move");
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  if (n == 0) return 0;
  SymArgs a{};
  a.f = *rows, a.n = n, a.seed = seed, a.flip_sides = flip_sides ? 1 : 0, a.permute_bench = permute_bench ? 1 : 0;
  hipLaunchKernelGGL(k_symmetries, dim3(n), dim3(64), 0, (hipStream_t)oakgpu_ctx_stream(ctx), a);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- host rows: staged, the calls wait for the stream --------------------------------------------------------------------------------
static int stage_rows(OakHostCall &hc, hipStream_t stream, const oakgpu_encoded_frames *h, uint32_t n, oakgpu_encoded_frames *d) {
  const size_t rows = std::max<uint32_t>(n, 1);
  struct Field { const void *src; void **dst; size_t bytes; };
  const Field fields[] = {
      {h->pokemon, (void **)&d->pokemon, rows * 12 * POKEMON_IN * 4}, {h->active, (void **)&d->active, rows * 2 * ACTIVE_IN * 4}, {h->hp, (void **)&d->hp, rows * 12 * 4},
      {h->choice_indices, (void **)&d->choice_indices, rows * 18 * 8}, {h->k, (void **)&d->k, rows * 2},
      {h->empirical_policies, (void **)&d->empirical_policies, rows * 18 * 4}, {h->nash_policies, (void **)&d->nash_policies, rows * 18 * 4},
      {h->empirical_value, (void **)&d->empirical_value, rows * 4}, {h->nash_value, (void **)&d->nash_value, rows * 4}, {h->score, (void **)&d->score, rows * 4},
      {h->status, (void **)&d->status, rows}};
  memset(d, 0, sizeof *d);
  for (const Field &f : fields) {
    if (!f.src) return oakgpu_fail_msg("trainer: the rows lack a tensor the trainer reads");
    void *p = hc.get(f.bytes);
    if (!p) return -1;
    *f.dst = p;
    if (n) HIPCHK(hipMemcpyAsync(p, f.src, f.bytes / rows * n, hipMemcpyHostToDevice, stream));
  }
  return 0;
}

extern "C" int oakgpu_trainer_forward(oakgpu_ctx *ctx, oakgpu_trainer *t, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss,
                                      const oakgpu_train_outputs *out) {
  if (!ctx || !t || !rows) return oakgpu_fail_msg("oakgpu_trainer_forward: null argument");
  if (n > t->max_rows) return oakgpu_fail_msg(("oakgpu_trainer_forward: n = " + std::to_string(n) + " rows exceed max_rows = " + std::to_string(t->max_rows)).c_str());
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall hc(ctx);
  oakgpu_encoded_frames d;
  if (int rc = stage_rows(hc, stream, rows, n, &d)) return rc;
  oakgpu_train_outputs o{};
  const size_t r = std::max<uint32_t>(n, 1);
  if (out) {
    if (out->value && !(o.value = (float *)hc.get(r * 4))) return -1;
    if (out->logits && !(o.logits = (float *)hc.get(r * 18 * 4))) return -1;
    if (out->sq_err && !(o.sq_err = (float *)hc.get(r * 4))) return -1;
    if (out->ce && !(o.ce = (float *)hc.get(r * 2 * 4))) return -1;
  }
  if (int rc = oakgpu_trainer_forward_dev(ctx, t, &d, n, loss, &o)) return rc;
  if (out && n) {
    if (out->value) HIPCHK(hipMemcpyAsync(out->value, o.value, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    if (out->logits) HIPCHK(hipMemcpyAsync(out->logits, o.logits, (size_t)n * 18 * 4, hipMemcpyDeviceToHost, stream));
    if (out->sq_err) HIPCHK(hipMemcpyAsync(out->sq_err, o.sq_err, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    if (out->ce) HIPCHK(hipMemcpyAsync(out->ce, o.ce, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, stream));
  }
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

extern "C" int oakgpu_trainer_gradients(oakgpu_ctx *ctx, oakgpu_trainer *t, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss) {
  if (!ctx || !t || !rows) return oakgpu_fail_msg("oakgpu_trainer_gradients: null argument");
  if (n > t->max_rows) return oakgpu_fail_msg(("oakgpu_trainer_gradients: n = " + std::to_string(n) + " rows exceed max_rows = " + std::to_string(t->max_rows)).c_str());
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall hc(ctx);
  oakgpu_encoded_frames d;
  if (int rc = stage_rows(hc, stream, rows, n, &d)) return rc;
  if (int rc = oakgpu_trainer_gradients_dev(ctx, t, &d, n, loss)) return rc;
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

extern "C" int oakgpu_trainer_step(oakgpu_ctx *ctx, oakgpu_trainer *t, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss, float lr,
                                   int clamp_weights) {
  if (!ctx || !t || !rows) return oakgpu_fail_msg("oakgpu_trainer_step: null argument");
  if (n > t->max_rows) return oakgpu_fail_msg(("oakgpu_trainer_step: n = " + std::to_string(n) + " rows exceed max_rows = " + std::to_string(t->max_rows)).c_str());
  if (int rc = oakgpu_ctx_enter(ctx)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall hc(ctx);
  oakgpu_encoded_frames d;
  if (int rc = stage_rows(hc, stream, rows, n, &d)) return rc;
  if (int rc = oakgpu_trainer_step_dev(ctx, t, &d, n, loss, lr, clamp_weights)) return rc;
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}
