// oak_amd/csrc/nash.hpp -- exact Nash equilibrium of a <= 9 x 9 zero-sum matrix game with integer payoffs (host and device code).
//
// Replaces LRSNash::solve_fast (lab-oak/lrsnash over GMP: absent from the reference checkout) at its three call sites:
// MCTS::Search::process_output (cpp/include/search/mcts.h:620-659), the MatrixUCB root solve (mcts.h:532-543) and
// pyoak's solve_matrix (cpp/src/pyoak.cc:394-426).  Like the reference's, the solve uses NO floating point: it is the
// simplex method with Bland's rule in integer ("fraction-free") pivoting -- the tableau holds integers over one common
// denominator, every division is exact -- on wide two's complement integers of L 64-bit limbs, kept as 2 L 32-bit words so
// that the host and the device compiler take the same text (a 32 x 32 product plus two 32-bit addends fits 64 bits).
// Only the final strategies / value are rounded to double: `solve` rounds them through x87 long double (host only, the
// results every host caller has always had), `solve_soft<L>` through a restatement of exactly those long double operations in
// integer arithmetic (X87 below), which both sides compile and which returns the same bits.
//
// Width.  Every tableau entry is, up to sign, a minor of [B | I | 1] bordered by the objective row: order <= 10, entries
// bounded by E = the largest shifted payoff.  Hadamard: |entry| <= (sqrt(10) E)^10.
//   E <= 2^21 + 1 (|payoff| <= 2^20):  (3.1623 * 2^21.000001)^10 < 2^227, a product of two < 2^454, their difference < 2^455: 8 limbs.
//   E <= WIDTH4_MAX_ENTRY = 2048:      (3.1623 * 2048)^10 < 2^127, products < 2^254, differences < 2^255: 4 limbs.
// (k_fsp_payoffs' entries are 1 ... 257 after the shift: 4 limbs.)  The integers are the same at either width, so is the result.
// The reference holds no test for its solver; this one is checked by LP optimality (zero best-response gap in exact
// arithmetic, tests/test_search_host.py).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define OAK_NASH_HD __host__ __device__
#else
#define OAK_NASH_HD
#endif

// The product below has two texts for the same integer: 32-bit words (what the device compiles, and any host build that defines
// OAK_NASH_WORDS_ONLY, as the stand-alone check does) and, on a host compiler with a 128-bit integer, 64-bit limbs.
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__SIZEOF_INT128__) && !defined(OAK_NASH_WORDS_ONLY)
#define OAK_NASH_MUL128 1
#else
#define OAK_NASH_MUL128 0
#endif

namespace oak_nash {

constexpr int MAX_PIVOTS = 100000;
constexpr int64_t MAX_PAYOFF = 1 << 20;      // |payoff| beyond this is refused
constexpr int64_t WIDTH4_MAX_ENTRY = 2048;   // largest shifted entry the 4-limb width takes (bound above)
constexpr uint32_t PAY_STRIDE = 82;          // int32 words of one matrix as oakgpu_nash_solve_dev takes it: 81 payoffs + (m | n << 8)

OAK_NASH_HD inline int limbs_for(int64_t max_shifted_entry) { return max_shifted_entry <= WIDTH4_MAX_ENTRY ? 4 : 8; }

template <int L> struct WideT { // 64 L-bit two's complement
  static constexpr int N = 2 * L;
  uint32_t w[N];
  OAK_NASH_HD WideT() {
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = 0;
  }
  OAK_NASH_HD WideT(int64_t v) {
    w[0] = (uint32_t)(uint64_t)v; w[1] = (uint32_t)((uint64_t)v >> 32);
#pragma unroll
    for (int i = 2; i < N; ++i) w[i] = v < 0 ? ~0u : 0u;
  }
  OAK_NASH_HD bool neg() const { return (w[N - 1] >> 31) != 0; }
  OAK_NASH_HD bool zero() const {
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) any |= w[i];
    return any == 0;
  }
  OAK_NASH_HD uint64_t limb(int i) const { return (uint64_t)w[2 * i] | (uint64_t)w[2 * i + 1] << 32; }
  OAK_NASH_HD WideT operator-() const {
    WideT r;
    uint64_t c = 1;
#pragma unroll
    for (int i = 0; i < N; ++i) { c += (uint32_t)~w[i]; r.w[i] = (uint32_t)c; c >>= 32; }
    return r;
  }
  OAK_NASH_HD WideT operator+(const WideT &o) const {
    WideT r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) { c += (uint64_t)w[i] + o.w[i]; r.w[i] = (uint32_t)c; c >>= 32; }
    return r;
  }
  OAK_NASH_HD WideT operator-(const WideT &o) const {
    WideT r;
    uint64_t c = 1;
#pragma unroll
    for (int i = 0; i < N; ++i) { c += (uint64_t)w[i] + (uint32_t)~o.w[i]; r.w[i] = (uint32_t)c; c >>= 32; }
    return r;
  }
  OAK_NASH_HD WideT operator*(const WideT &o) const { // modulo 2^(32 N): exact for every signed product that fits
    WideT r;
#if OAK_NASH_MUL128 // the host's compilers have a 64 x 64 -> 128 product: the same integer from a quarter of the multiplications
    uint64_t acc[L] = {};
    for (int i = 0; i < L; ++i) {
      unsigned __int128 c = 0;
      const uint64_t a = limb(i);
      for (int j = 0; j < L - i; ++j) {
        c += (unsigned __int128)a * o.limb(j) + acc[i + j];
        acc[i + j] = (uint64_t)c;
        c >>= 64;
      }
    }
    for (int i = 0; i < L; ++i) { r.w[2 * i] = (uint32_t)acc[i]; r.w[2 * i + 1] = (uint32_t)(acc[i] >> 32); }
#else
#pragma unroll
    for (int i = 0; i < N; ++i) {
      uint64_t c = 0;
#pragma unroll
      for (int j = 0; j < N - i; ++j) {
        c += (uint64_t)w[i] * o.w[j] + r.w[i + j];
        r.w[i + j] = (uint32_t)c;
        c >>= 32;
      }
    }
#endif
    return r;
  }
  OAK_NASH_HD static int cmp(const WideT &a, const WideT &b) { // signed
    if (a.neg() != b.neg()) return a.neg() ? -1 : 1;
    int r = 0; // same sign: two's complement orders like unsigned; the highest differing word decides
#pragma unroll
    for (int i = 0; i < N; ++i) if (a.w[i] != b.w[i]) r = a.w[i] < b.w[i] ? -1 : 1;
    return r;
  }
  OAK_NASH_HD int ctz() const { // trailing zero bits of a non-zero value
    int r = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (!found) { if (w[i]) { r += __builtin_ctz(w[i]); found = true; } else r += 32; }
    return r;
  }
  // arithmetic shift right by k bits, 0 <= k < 32 N (no indexing by a variable: the words stay in registers on the device)
  OAK_NASH_HD WideT sar(int k) const {
    WideT r = *this;
    const uint32_t fill = neg() ? ~0u : 0u;
    const int bs = k & 31;
    if (bs) {
#pragma unroll
      for (int i = 0; i < N; ++i) r.w[i] = (r.w[i] >> bs) | ((i + 1 < N ? r.w[i + 1] : fill) << (32 - bs));
    }
#pragma unroll
    for (int step = 1; step < N; step <<= 1)
      if ((k >> 5) & step) {
#pragma unroll
        for (int i = 0; i < N; ++i) r.w[i] = i + step < N ? r.w[i + step] : fill;
      }
    return r;
  }
  // the inverse of an odd value modulo 2^(32 N): Newton's x <- x (2 - d x) doubles the correct low bits each round
  OAK_NASH_HD static WideT inverse_odd(const WideT &d) {
    uint32_t x = (3u * d.w[0]) ^ 2u; // 5 bits
#pragma unroll
    for (int i = 0; i < 3; ++i) x *= 2u - d.w[0] * x; // 10, 20, 40
    WideT r;
    r.w[0] = x;
    const WideT two(2);
    for (int bits = 32; bits < 32 * N; bits <<= 1) r = r * (two - d * r);
    return r;
  }
  // Exact division by d > 0 that is known to divide: d = odd * 2^tz, so a / d = (a >> tz) * odd^-1 modulo 2^(32 N), and the quotient
  // fits.  The caller keeps tz and the inverse of d >> tz, which serve every cell of one pivot.
  OAK_NASH_HD static WideT divexact(const WideT &a, const WideT &odd_inverse, int tz) { return a.sar(tz) * odd_inverse; }
  long double to_ld() const { // host only.  x87 extended: every step rounds to 64 mantissa bits
    const WideT u = neg() ? -*this : *this;
    long double r = 0;
    for (int i = L - 1; i >= 0; --i) r = r * 18446744073709551616.0L + (long double)u.limb(i);
    return neg() ? -r : r;
  }
};
using Wide = WideT<8>;

// ---- the tableau and the pivoting rule
template <int L> struct Tableau {
  WideT<L> T[9][19], z[19], D;
  int basis[9];
  int m, n, W;
  int64_t shift;
};

// Runs the simplex for the zero-sum game in which the ROW player maximises payoffs[i * n + j].  False: bad arguments.
template <int L> OAK_NASH_HD inline bool simplex(const int32_t *payoffs, int m, int n, Tableau<L> &t) {
  typedef WideT<L> Wd;
  if (!payoffs || m < 1 || n < 1 || m > 9 || n > 9) return false;
  int64_t lo = payoffs[0];
  for (int i = 0; i < m * n; ++i) {
    if (payoffs[i] > MAX_PAYOFF || payoffs[i] < -MAX_PAYOFF) return false;
    lo = payoffs[i] < lo ? payoffs[i] : lo;
  }
  const int64_t shift = 1 - lo; // every entry >= 1
  // column player: maximise sum z  s.t.  B z <= 1, z >= 0;  p2 = z / sum z, value + shift = 1 / sum z; the duals
  // (reduced costs of the slacks) give p1.  Tableau [B | I | 1] and objective row over the common denominator D.
  const int W = n + m + 1;
  t.m = m; t.n = n; t.W = W; t.shift = shift;
  Wd(&T)[9][19] = t.T;
  Wd(&z)[19] = t.z;
  int(&basis)[9] = t.basis;
  Wd D(1), D_inverse(1); // D_inverse: of D >> D_tz
  int D_tz = 0;
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < n; ++j) T[i][j] = Wd(payoffs[i * n + j] + shift);
    for (int k = 0; k < m; ++k) T[i][n + k] = Wd(i == k ? 1 : 0);
    T[i][W - 1] = Wd(1);
    basis[i] = n + i;
  }
  for (int j = 0; j < W; ++j) z[j] = Wd(j < n ? -1 : 0);
  for (int iter = 0; iter < MAX_PIVOTS; ++iter) {
    int col = -1;
    for (int j = 0; j < n + m; ++j) if (z[j].neg()) { col = j; break; } // Bland: lowest index with negative reduced cost
    if (col < 0) break;
    int row = -1;
    for (int i = 0; i < m; ++i) {
      if (T[i][col].neg() || T[i][col].zero()) continue;
      if (row < 0) { row = i; continue; }
      // ratio_i < ratio_row  <=>  T[i][rhs] * T[row][col] < T[row][rhs] * T[i][col]   (both pivots positive)
      const int c = Wd::cmp(T[i][W - 1] * T[row][col], T[row][W - 1] * T[i][col]);
      if (c < 0 || (c == 0 && basis[i] < basis[row])) row = i;
    }
    if (row < 0) return false; // unbounded: impossible for entries >= 1
    const Wd piv = T[row][col];
    for (int i = 0; i < m; ++i) {
      if (i == row) continue;
      const Wd f = T[i][col];
      for (int j = 0; j < W; ++j) T[i][j] = Wd::divexact(T[i][j] * piv - f * T[row][j], D_inverse, D_tz);
    }
    const Wd f = z[col];
    for (int j = 0; j < W; ++j) z[j] = Wd::divexact(z[j] * piv - f * T[row][j], D_inverse, D_tz);
    D = piv;
    D_tz = D.ctz();
    D_inverse = Wd::inverse_odd(D.sar(D_tz));
    basis[row] = col;
  }
  t.D = D;
  return true;
}

// ---- x87 extended precision restated in integers: the operations `solve` applies to its long doubles, bit for bit, under the x87
// default (64 mantissa bits, round to nearest even).  A value is (-1)^neg * m * 2^e with m == 0 or m's top bit set.
struct X87 { uint64_t m; int32_t e; bool neg; };

// x <- x >> s on 192 bits, 0 <= s < 192; the bits shifted out are or-ed into sticky
OAK_NASH_HD inline void shr192(uint64_t &x2, uint64_t &x1, uint64_t &x0, int s, uint64_t &sticky) {
  if (s >= 128) { sticky |= x0 | x1; x0 = x2; x1 = 0; x2 = 0; s -= 128; }
  else if (s >= 64) { sticky |= x0; x0 = x1; x1 = x2; x2 = 0; s -= 64; }
  if (s) {
    sticky |= x0 << (64 - s);
    x0 = x0 >> s | x1 << (64 - s);
    x1 = x1 >> s | x2 << (64 - s);
    x2 >>= s;
  }
}

// (x2 : x1 : x0) * 2^e rounded to 64 mantissa bits, nearest even
OAK_NASH_HD inline X87 x87_round(uint64_t x2, uint64_t x1, uint64_t x0, int32_t e, bool neg) {
  X87 r{0, 0, false};
  if (!(x2 | x1 | x0)) return r; // +0
  const int top = x2 ? 191 - __builtin_clzll(x2) : x1 ? 127 - __builtin_clzll(x1) : 63 - __builtin_clzll(x0);
  r.neg = neg;
  if (top <= 63) { r.m = x0 << (63 - top); r.e = e - (63 - top); return r; }
  const int s = top - 63;
  uint64_t sticky = 0;
  shr192(x2, x1, x0, s - 1, sticky);
  const bool guard = x0 & 1;
  uint64_t m = x0 >> 1 | x1 << 63;
  e += s;
  if (guard && (sticky || (m & 1))) { if (++m == 0) { m = 1ull << 63; ++e; } }
  r.m = m; r.e = e;
  return r;
}

// r * 2^64 + limb: one step of to_ld()
OAK_NASH_HD inline X87 x87_accumulate(const X87 &r, uint64_t limb) {
  if (!r.m) return x87_round(0, 0, limb, 0, false);
  const int E = r.e + 64; // >= 1: r is an integer >= 1
  if (E >= 128) return X87{r.m, E, false}; // the limb is below half a unit
  uint64_t x2 = 0, x1 = 0, x0 = 0;
  if (E >= 64) { x1 = r.m << (E - 64); x2 = E > 64 ? r.m >> (128 - E) : 0; }
  else { x0 = r.m << E; x1 = r.m >> (64 - E); }
  const uint64_t s0 = x0 + limb;
  if (s0 < x0) { if (++x1 == 0) ++x2; }
  return x87_round(x2, x1, s0, 0, false);
}

template <int L> OAK_NASH_HD inline X87 x87_from_wide(const WideT<L> &v) {
  const WideT<L> u = v.neg() ? -v : v;
  X87 r{0, 0, false};
#pragma unroll
  for (int i = L - 1; i >= 0; --i) r = x87_accumulate(r, u.limb(i));
  if (r.m) r.neg = v.neg();
  return r;
}

// floor((hi : lo) / d) for hi < d, and the remainder: 64 shift-subtract steps
OAK_NASH_HD inline uint64_t div128(uint64_t hi, uint64_t lo, uint64_t d, uint64_t *rem) {
  uint64_t q = 0;
  for (int i = 63; i >= 0; --i) {
    const bool over = hi >> 63;
    hi = hi << 1 | ((lo >> i) & 1);
    q <<= 1;
    if (over || hi >= d) { hi -= d; q |= 1; }
  }
  *rem = hi;
  return q;
}

OAK_NASH_HD inline X87 x87_divide(const X87 &a, const X87 &b) { // b != 0
  X87 r{0, 0, false};
  if (!a.m) return r;
  uint64_t rem, q;
  int32_t e;
  if (a.m >= b.m) { q = div128(a.m >> 1, a.m << 63, b.m, &rem); e = a.e - b.e - 63; }
  else { q = div128(a.m, 0, b.m, &rem); e = a.e - b.e - 64; }
  // nearest even on the remainder: 2 rem against b.m (rem < b.m, so compare rem with b.m - rem)
  const uint64_t other = b.m - rem;
  if (rem > other || (rem == other && (q & 1))) { if (++q == 0) { q = 1ull << 63; ++e; } }
  r.m = q; r.e = e; r.neg = a.neg != b.neg;
  return r;
}

OAK_NASH_HD inline X87 x87_from_int(int64_t v) {
  return x87_round(0, 0, v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v, 0, v < 0);
}

OAK_NASH_HD inline X87 x87_add(X87 a, X87 b) {
  if (!b.m) return a;
  if (!a.m) return b;
  if (a.e < b.e) { const X87 t = a; a = b; b = t; }
  const int d = a.e - b.e;
  if (d >= 66) return a; // |b| < 2^(b.e + 64) <= a quarter of a's unit: under half the spacing even just below a power of two
  uint64_t x2 = 0, x1 = 0, x0 = a.m;
  if (d >= 64) { x1 = a.m << (d - 64); x2 = d > 64 ? a.m >> (128 - d) : 0; x0 = 0; }
  else if (d) { x0 = a.m << d; x1 = a.m >> (64 - d); }
  bool neg = a.neg;
  if (a.neg == b.neg) {
    const uint64_t s0 = x0 + b.m;
    if (s0 < x0) { if (++x1 == 0) ++x2; }
    x0 = s0;
  } else if (x2 | x1 || x0 >= b.m) {
    const uint64_t s0 = x0 - b.m;
    if (s0 > x0) { if (x1-- == 0) --x2; }
    x0 = s0;
  } else { x0 = b.m - x0; neg = b.neg; }
  return x87_round(x2, x1, x0, b.e, neg); // an exact zero comes back as +0, as under round to nearest
}

OAK_NASH_HD inline X87 x87_subtract_int(const X87 &a, int64_t v) {
  X87 b = x87_from_int(v);
  b.neg = !b.neg;
  return x87_add(a, b);
}

// (double)x: a second rounding, 64 -> 53 bits, nearest even.  Every value here lies far inside double's normal range (strategies in
// [0, 1] with denominators below 2^512, values within +-2^22); an exponent outside it saturates to infinity or flushes to zero.
OAK_NASH_HD inline double x87_to_double(const X87 &x) {
  uint64_t bits = (uint64_t)x.neg << 63;
  if (x.m) {
    int E = x.e + 63;
    uint64_t mant = x.m >> 11;
    const bool guard = (x.m >> 10) & 1, sticky = (x.m & 0x3FF) != 0;
    if (guard && (sticky || (mant & 1))) { if (++mant == (1ull << 53)) { mant >>= 1; ++E; } }
    if (E > 1023) bits |= 0x7FFull << 52;
    else if (E >= -1022) bits |= (uint64_t)(E + 1023) << 52 | (mant & ((1ull << 52) - 1));
  }
  double d;
  memcpy(&d, &bits, 8);
  return d;
}

// ---- the solvers
// Equilibrium of the zero-sum game in which the ROW player maximises payoffs[i * n + j] (integers, |.| <= 2^20).
// p1[m], p2[n]: equilibrium strategies; *value: the game value in payoff units.  Returns false on bad arguments.
inline bool solve(const int32_t *payoffs, int m, int n, double *p1, double *p2, double *value) {
  Tableau<8> t;
  if (!simplex<8>(payoffs, m, n, t)) return false;
  const int W = t.W;
  const long double tot = t.z[W - 1].to_ld(); // sum z = tot / D  (> 0)
  if (!(tot > 0)) return false;
  for (int j = 0; j < n; ++j) p2[j] = 0.0;
  for (int i = 0; i < m; ++i) if (t.basis[i] < n) p2[t.basis[i]] = (double)(t.T[i][W - 1].to_ld() / tot);
  for (int i = 0; i < m; ++i) p1[i] = (double)(t.z[n + i].to_ld() / tot);
  *value = (double)(t.D.to_ld() / tot - (long double)t.shift);
  return true;
}

// `solve` with the rounding restated (X87) on L-limb integers: the same bits wherever the tableau fits L limbs (limbs_for).
template <int L> OAK_NASH_HD inline bool solve_soft(const int32_t *payoffs, int m, int n, double *p1, double *p2, double *value) {
  Tableau<L> t;
  if (!simplex<L>(payoffs, m, n, t)) return false;
  const int W = t.W;
  const X87 tot = x87_from_wide(t.z[W - 1]);
  if (!tot.m || tot.neg) return false;
  for (int j = 0; j < n; ++j) p2[j] = 0.0;
  for (int i = 0; i < m; ++i) if (t.basis[i] < n) p2[t.basis[i]] = x87_to_double(x87_divide(x87_from_wide(t.T[i][W - 1]), tot));
  for (int i = 0; i < m; ++i) p1[i] = x87_to_double(x87_divide(x87_from_wide(t.z[n + i]), tot));
  *value = x87_to_double(x87_subtract_int(x87_divide(x87_from_wide(t.D), tot), t.shift));
  return true;
}

// the width a matrix takes: from its largest entry after the shift (false: the solver refuses it)
OAK_NASH_HD inline bool width_of(const int32_t *payoffs, int m, int n, int *limbs) {
  if (!payoffs || m < 1 || n < 1 || m > 9 || n > 9) return false;
  int64_t lo = payoffs[0], hi = payoffs[0];
  for (int i = 0; i < m * n; ++i) {
    if (payoffs[i] > MAX_PAYOFF || payoffs[i] < -MAX_PAYOFF) return false;
    lo = payoffs[i] < lo ? payoffs[i] : lo;
    hi = payoffs[i] > hi ? payoffs[i] : hi;
  }
  *limbs = limbs_for(hi - lo + 1);
  return true;
}

} // namespace oak_nash
