// oak_amd/csrc/nashdev.hip -- the exact Nash solve of nash.hpp on the device: oakgpu_nash_solve_dev (what the forest loops call between
// k_fsp_payoffs and their pick kernels), oakgpu_solve_matrices (a batch of oakgpu_solve_matrix calls through it) and the host-only
// diagnostics behind tests/test_nash_soft.py.
//
//   k_nash_solve<L>: one workgroup of 256 lanes per matrix.  Lane t < 190 holds ONE cell of the tableau in registers -- row t / 19 (0 ... 8 the
//     constraint rows, 9 the objective), column t % 19 -- as a WideT<L>.  A pivot is five barriers: the objective lanes with a negative
//     reduced cost take the minimum of their columns (Bland); the entering column and the right-hand side go to LDS; 81 lanes compare the
//     ratios of every pair of candidate rows by cross products, and the one row no other beats under (ratio, basis[]) leaves -- the order is
//     total, so this is the row nash.hpp's scan keeps; the pivot row goes to LDS; every other cell becomes (cell * piv - f * row[c]) / D.
//     The division is exact, so it is a shift and a product with the inverse of D's odd part modulo 2^(64 L), which one lane of the
//     fourth wave (it holds no cell) works out for the NEXT pivot while the cells update.  The strategies and the value are rounded by
//     nash.hpp's X87 restatement in the lanes that hold their numerators.
//     Every loop is bounded: pivots by oak_nash::MAX_PIVOTS, Newton's rounds by the limb count; no workgroup waits for another.
//   Two launches cover a batch, L = 4 and L = 8: a workgroup leaves at once when oak_nash::limbs_for picks the other width for its
//     matrix, and the L = 4 launch writes the zeros of a matrix the solver refuses.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/oakgpu.h"
#include "oakgpu_internal.h"
#include "nash.hpp"

#define RC(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

namespace {

using oak_nash::WideT;
using oak_nash::X87;
using oak_nash::PAY_STRIDE;
constexpr int NASH_BLOCK = 256;
constexpr int NO_COLUMN = 255;

struct NashArgs {
  const int32_t *pay; // rows x PAY_STRIDE
  double *p1, *p2, *value; // rows x 9, rows x 9, rows
  double divisor;     // the value is stored divided by this
  uint32_t rows;
};

__device__ inline void store_zeros(const NashArgs &a, uint32_t mat, uint32_t tid) {
  if (tid < 9) a.p1[(size_t)mat * 9 + tid] = 0.0;
  else if (tid < 18) a.p2[(size_t)mat * 9 + tid - 9] = 0.0;
  else if (tid == 18) a.value[mat] = 0.0;
}

// a WideT in LDS (a __shared__ variable takes no constructor)
template <int L> struct Raw {
  uint32_t w[2 * L];
  __device__ void operator=(const WideT<L> &v) {
#pragma unroll
    for (int i = 0; i < 2 * L; ++i) w[i] = v.w[i];
  }
  __device__ WideT<L> get() const {
    WideT<L> v;
#pragma unroll
    for (int i = 0; i < 2 * L; ++i) v.w[i] = w[i];
    return v;
  }
};

template <int L> __global__ __launch_bounds__(NASH_BLOCK) void k_nash_solve(NashArgs a) {
  typedef WideT<L> Wd;
  __shared__ Raw<L> s_row[19], s_col[10], s_rhs[9], s_inverse[2], s_D, s_tot;
  __shared__ int32_t s_pay[PAY_STRIDE];
  __shared__ int s_tz[2], s_basis[9];
  __shared__ unsigned s_sel, s_cand, s_lose;
  __shared__ double s_out[19];
  const uint32_t mat = blockIdx.x, tid = threadIdx.x;
  if (mat >= a.rows) return;
  if (tid < PAY_STRIDE) s_pay[tid] = a.pay[(size_t)mat * PAY_STRIDE + tid];
  __syncthreads();
  const int m = s_pay[81] & 0xFF, n = (s_pay[81] >> 8) & 0xFF;
  bool ok = m >= 1 && m <= 9 && n >= 1 && n <= 9;
  int64_t lo = 0, hi = 0;
  if (ok) {
    lo = hi = s_pay[0];
    for (int i = 0; i < m * n; ++i) {
      const int64_t v = s_pay[i];
      if (v > oak_nash::MAX_PAYOFF || v < -oak_nash::MAX_PAYOFF) ok = false;
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
  }
  if (!ok) { // the solver refuses: zeros, from the launch of the narrow width alone
    if (L == 4) store_zeros(a, mat, tid);
    return;
  }
  if (oak_nash::limbs_for(hi - lo + 1) != L) return;
  const int64_t shift = 1 - lo;
  const int W = n + m + 1;
  const int r = tid / 19, c = tid % 19;
  const bool constraint = r < m, objective = r == 9;
  const bool active = tid < 190 && c < W && (constraint || objective);
  Wd cell;
  if (active) {
    if (constraint) cell = c < n ? Wd(s_pay[r * n + c] + shift) : Wd(c == W - 1 || c - n == r ? 1 : 0);
    else cell = Wd(c < n ? -1 : 0);
  }
  if (tid < 9) s_basis[tid] = n + tid;
  if (tid == 0) { s_inverse[0] = Wd(1); s_tz[0] = 0; s_D = Wd(1); }
  int cur = 0;
  bool unbounded = false;
  for (int iter = 0; iter < oak_nash::MAX_PIVOTS; ++iter) {
    if (tid == 0) { s_sel = NO_COLUMN; s_cand = 0; s_lose = 0; }
    __syncthreads();
    if (active && objective && c < n + m && cell.neg()) atomicMin(&s_sel, (unsigned)c); // Bland: lowest index with negative reduced cost
    __syncthreads();
    const int col = (int)s_sel;
    if (col == NO_COLUMN) break;
    if (active && c == col) {
      s_col[r] = cell;
      if (constraint && !cell.neg() && !cell.zero()) atomicOr(&s_cand, 1u << r);
    }
    if (active && constraint && c == W - 1) s_rhs[r] = cell;
    __syncthreads();
    const unsigned cand = s_cand;
    if (!cand) { unbounded = true; break; } // impossible for entries >= 1
    if (tid < 81) {
      const int i = tid / 9, k = tid % 9;
      if (i != k && (cand >> i & 1) && (cand >> k & 1)) {
        // ratio_i < ratio_k  <=>  rhs[i] * col[k] < rhs[k] * col[i]   (both pivots positive)
        const int cmp = Wd::cmp(s_rhs[i].get() * s_col[k].get(), s_rhs[k].get() * s_col[i].get());
        if (!(cmp < 0 || (cmp == 0 && s_basis[i] < s_basis[k]))) atomicOr(&s_lose, 1u << i);
      }
    }
    __syncthreads();
    const unsigned winners = cand & ~s_lose;
    if (!winners) { unbounded = true; break; } // (the order is total: one row is beaten by none)
    const int row = __ffs(winners) - 1;
    if (active && r == row) s_row[c] = cell;
    __syncthreads();
    if (active && r != row) {
      const Wd piv = s_col[row].get(), f = s_col[r].get();
      cell = Wd::divexact(cell * piv - f * s_row[c].get(), s_inverse[cur].get(), s_tz[cur]);
    }
    if (tid == 192) { // the next pivot's divisor
      const Wd piv = s_col[row].get();
      const int tz = piv.ctz();
      s_inverse[cur ^ 1] = Wd::inverse_odd(piv.sar(tz));
      s_tz[cur ^ 1] = tz;
      s_D = piv;
    }
    if (tid == 0) s_basis[row] = col;
    cur ^= 1;
  }
  // (both ways out of the loop are taken by every lane together, after a barrier)
  if (tid < 19) s_out[tid] = 0.0;
  if (active && objective && c == W - 1) s_tot = cell;
  __syncthreads();
  const Wd total = s_tot.get();
  const bool solved = !unbounded && !total.neg() && !total.zero(); // sum z = tot / D  (> 0)
  if (solved) {
    const bool p2_lane = active && constraint && c == W - 1 && s_basis[r] < n, p1_lane = active && objective && c >= n && c < n + m;
    if (p2_lane || p1_lane || tid == 192) {
      const X87 tot = oak_nash::x87_from_wide(total);
      if (tid == 192) {
        const Wd D = s_D.get();
        s_out[18] = oak_nash::x87_to_double(oak_nash::x87_subtract_int(oak_nash::x87_divide(oak_nash::x87_from_wide(D), tot), shift)) / a.divisor;
      } else {
        const double p = oak_nash::x87_to_double(oak_nash::x87_divide(oak_nash::x87_from_wide(cell), tot));
        s_out[p2_lane ? 9 + s_basis[r] : c - n] = p;
      }
    }
  }
  __syncthreads();
  if (tid < 9) a.p1[(size_t)mat * 9 + tid] = s_out[tid];
  else if (tid < 18) a.p2[(size_t)mat * 9 + tid - 9] = s_out[tid];
  else if (tid == 18) a.value[mat] = s_out[18];
}

int launch(hipStream_t stream, const int32_t *pay, uint32_t rows, double *nash, double divisor) {
  if (!rows) return 0;
  const NashArgs a{pay, nash, nash + (size_t)rows * 9, nash + (size_t)rows * 18, divisor, rows};
  hipLaunchKernelGGL(k_nash_solve<4>, dim3(rows), dim3(NASH_BLOCK), 0, stream, a);
  hipLaunchKernelGGL(k_nash_solve<8>, dim3(rows), dim3(NASH_BLOCK), 0, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int fail_at(const char *what, uint32_t k) {
  const std::string msg = "oakgpu_solve_matrices: matrix " + std::to_string(k) + ": " + what;
  return oakgpu_fail_msg(msg.c_str());
}

oak_nash::Wide wide_from_limbs(const uint64_t *limbs) {
  oak_nash::Wide v;
  for (int i = 0; i < 8; ++i) { v.w[2 * i] = (uint32_t)limbs[i]; v.w[2 * i + 1] = (uint32_t)(limbs[i] >> 32); }
  return v;
}

} // namespace

extern "C" {

int oakgpu_nash_solve_dev(oakgpu_ctx *ctx, const int32_t *pay, uint32_t rows, double *nash) {
  if (!ctx || (rows && (!pay || !nash))) return oakgpu_fail_msg("oakgpu_nash_solve_dev: null argument");
  RC(oakgpu_ctx_enter(ctx));
  return launch((hipStream_t)oakgpu_ctx_stream(ctx), pay, rows, nash, 256.0);
}

int oakgpu_solve_matrices(oakgpu_ctx *ctx, const int32_t *payoffs, const int32_t *m, const int32_t *n, uint32_t count, int discretize_factor,
                          double *p1, double *p2, double *value) {
  if (count && (!payoffs || !m || !n || !p1 || !p2 || !value)) return oakgpu_fail_msg("oakgpu_solve_matrices: null argument");
  if (discretize_factor < 1) return oakgpu_fail_msg("oakgpu_solve_matrices: discretize_factor must be positive");
  if (!count) return 0;
  std::vector<int32_t> pay((size_t)count * PAY_STRIDE, 0);
  for (uint32_t k = 0; k < count; ++k) { // oakgpu_solve_matrix's refusals, before anything is launched
    if (m[k] < 1 || n[k] < 1 || m[k] > 9 || n[k] > 9) return fail_at("payoff matrix must be between 1x1 and 9x9", k);
    const int32_t *src = payoffs + (size_t)k * 81;
    int32_t *dst = pay.data() + (size_t)k * PAY_STRIDE;
    for (int i = 0; i < m[k] * n[k]; ++i) {
      if (src[i] > oak_nash::MAX_PAYOFF || src[i] < -oak_nash::MAX_PAYOFF) return fail_at("payoffs out of range (|payoff| <= 2^20)", k);
      dst[i] = src[i];
    }
    dst[81] = m[k] | n[k] << 8;
  }
  if (!ctx) return oakgpu_fail_msg("oakgpu_solve_matrices: null context"); // (after the refusals: they need no device)
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall call(ctx);
  int32_t *d_pay = (int32_t *)call.get(pay.size() * 4);
  double *d_nash = (double *)call.get((size_t)count * 19 * 8);
  if (!d_pay || !d_nash) return -1;
  std::vector<double> nash((size_t)count * 19);
  HIPCHK(hipMemcpyAsync(d_pay, pay.data(), pay.size() * 4, hipMemcpyHostToDevice, stream));
  RC(launch(stream, d_pay, count, d_nash, (double)discretize_factor));
  HIPCHK(hipMemcpyAsync(nash.data(), d_nash, nash.size() * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  memcpy(p1, nash.data(), (size_t)count * 72);
  memcpy(p2, nash.data() + (size_t)count * 9, (size_t)count * 72);
  memcpy(value, nash.data() + (size_t)count * 18, (size_t)count * 8);
  return 0;
}

// ---- host-only diagnostics (no GPU): the device's solver text and its rounding, run on the host
int oakgpu_nash_width4_max_entry(void) { return (int)oak_nash::WIDTH4_MAX_ENTRY; }

int oakgpu_nash_soft_host(const int32_t *payoffs, const int32_t *m, const int32_t *n, uint32_t count, int limbs, double *p1, double *p2, double *value,
                          uint8_t *width) {
  if (count && (!payoffs || !m || !n || !p1 || !p2 || !value || !width)) return oakgpu_fail_msg("oakgpu_nash_soft_host: null argument");
  if (limbs != 0 && limbs != 4 && limbs != 8) return oakgpu_fail_msg("oakgpu_nash_soft_host: limbs is 0 (the selector's), 4 or 8");
  for (uint32_t k = 0; k < count; ++k) {
    const int32_t *M = payoffs + (size_t)k * 81;
    double x[9] = {}, y[9] = {}, v = 0;
    int chosen = 0;
    bool ok = oak_nash::width_of(M, m[k], n[k], &chosen);
    const int use = limbs ? limbs : chosen;
    if (ok) ok = use == 4 ? oak_nash::solve_soft<4>(M, m[k], n[k], x, y, &v) : oak_nash::solve_soft<8>(M, m[k], n[k], x, y, &v);
    for (int q = 0; q < 9; ++q) { p1[(size_t)k * 9 + q] = ok ? x[q] : 0.0; p2[(size_t)k * 9 + q] = ok ? y[q] : 0.0; }
    value[k] = ok ? v : 0.0;
    width[k] = ok ? (uint8_t)chosen : 0; // what the selector picks, whichever width ran; 0: refused
  }
  return 0;
}

int oakgpu_nash_round_host(const uint64_t *num, const uint64_t *den, const int64_t *shift, uint32_t count, double *hard, double *soft) {
  if (count && (!num || !den || !shift || !hard || !soft)) return oakgpu_fail_msg("oakgpu_nash_round_host: null argument");
  for (uint32_t k = 0; k < count; ++k) {
    const oak_nash::Wide a = wide_from_limbs(num + (size_t)k * 8), b = wide_from_limbs(den + (size_t)k * 8);
    if (b.zero()) return oakgpu_fail_msg("oakgpu_nash_round_host: zero denominator");
    hard[k] = (double)(a.to_ld() / b.to_ld() - (long double)shift[k]);
    soft[k] = oak_nash::x87_to_double(oak_nash::x87_subtract_int(oak_nash::x87_divide(oak_nash::x87_from_wide(a), oak_nash::x87_from_wide(b)), shift[k]));
  }
  return 0;
}

} // extern "C"
