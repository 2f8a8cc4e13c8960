// oak_amd/csrc/net_pack.hpp -- the host half of the battle-net loader: a .battle.net file's bytes -> the checked, rearranged
// images that leafnet.hip uploads, one per NetDev / QNetDev field.  Plain C++17 with no HIP in it and a pure function of the
// file's bytes and the `discrete` flag: leafnet.hip includes it for oakgpu_net_load*, tests/cpp_net_pack_check.cc includes it
// stand-alone (tests/test_net_pack.py holds every image to a recorded digest, on the CPU and under sanitizers).
//
// Parameter file reader: nn/affine.h:35-70, network.h:52-70, main-net.h:36-55, search.cc:127-131.  Every image matches an LDS or
// MFMA-fragment layout of a kernel byte for byte; the constants both sides use are in net_layout.hpp.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <string>
#include <vector>

#include "net_layout.hpp"

namespace oak {
namespace pack {
namespace { // internal linkage, as the loader's functions always had: one translation unit per binary includes this, and the library exports its C ABI only

// ---- the file ----
struct HostAffine { uint32_t in, out; std::vector<float> b, w; };

bool read_affine(const uint8_t *&p, const uint8_t *end, HostAffine &a) {
  if (end - p < 8) return false;
  memcpy(&a.in, p, 4);
  memcpy(&a.out, p + 4, 4);
  p += 8;
  if (a.in == 0 || a.out == 0 || a.in > (1u << 16) || a.out > (1u << 16)) return false;
  const size_t nb = (size_t)a.out * 4, nw = (size_t)a.out * a.in * 4;
  if ((size_t)(end - p) < nb + nw) return false;
  a.b.resize(a.out);
  a.w.resize((size_t)a.out * a.in);
  memcpy(a.b.data(), p, nb);
  p += nb;
  memcpy(a.w.data(), p, nw);
  p += nw;
  return true;
}

// ---- the result ----
struct Image { // one device buffer, for the NetDev field `name` ("q." + the QNetDev field for the int8 net)
  const char *name;
  std::vector<float> f32; std::vector<uint16_t> u16; std::vector<uint8_t> u8; std::vector<int8_t> i8; std::vector<int32_t> i32; // the ONE the packer built, kept as it is (no copy)
  Image(const char *n, std::vector<float> v) : name(n), f32(std::move(v)) {}
  Image(const char *n, std::vector<uint16_t> v) : name(n), u16(std::move(v)) {}
  Image(const char *n, std::vector<uint8_t> v) : name(n), u8(std::move(v)) {}
  Image(const char *n, std::vector<int8_t> v) : name(n), i8(std::move(v)) {}
  Image(const char *n, std::vector<int32_t> v) : name(n), i32(std::move(v)) {}
  const void *data() const { return !f32.empty() ? (const void *)f32.data() : !u16.empty() ? (const void *)u16.data() : !u8.empty() ? (const void *)u8.data() : !i8.empty() ? (const void *)i8.data() : (const void *)i32.data(); }
  size_t bytes() const { return f32.size() * 4 + u16.size() * 2 + u8.size() + i8.size() + i32.size() * 4; }
};

template <class T>
void append(std::vector<uint8_t> &to, const std::vector<T> &v) {
  const uint8_t *p = (const uint8_t *)v.data();
  to.insert(to.end(), p, p + v.size() * sizeof(T));
}

struct PackedNet {
  int activation;                                    // 1 relu, 2 clamp
  int in_dim, hidden, value_hidden, policy_hidden;   // unpadded, as in the file
  int p_hidden, p_out, a_hidden, a_out, side_dim;    // the embedding nets' widths; one side's embedding
  int H, VH, PH;                                     // padded: H, VH to 32, PH to 32 PB
  int T0, NB, PB;                                    // the weight streams' fc0 k-steps and block count; the policy heads' block count
  float b3;
  bool split_safe, embed_safe, pair_safe, policy_safe; // which number forms the weights allow (pack_net)
  bool discrete;
  int q_H, q_VH, q_PH, q_img_bytes;                  // the int8 net's scalars (discrete only)
  int32_t q_b3;
  // In upload order.  Absent: q1b_img / q2b_img when PH > 64 (the rows do not fit the CU's LDS), q1a_t / q2a_t when !policy_safe,
  // every q.* unless discrete.
  std::vector<Image> images;

  template <class T>
  void add(const char *name, std::vector<T> v) { images.emplace_back(name, std::move(v)); }
};

// ---- plain fp32 layouts ----
uint32_t up32(uint32_t x) { return (x + 31) & ~31u; }
std::vector<float> pad_vec(const std::vector<float> &v, uint32_t n) {
  std::vector<float> t(n, 0.0f);
  for (size_t i = 0; i < v.size(); ++i) t[i] = v[i];
  return t;
}
std::vector<float> transpose(const HostAffine &a) { // W[out][in] -> Wt[in][out]
  std::vector<float> t((size_t)a.in * a.out);
  for (uint32_t o = 0; o < a.out; ++o)
    for (uint32_t i = 0; i < a.in; ++i) t[(size_t)i * a.out + o] = a.w[(size_t)o * a.in + i];
  return t;
}
// pad rows (out) to a multiple of 32 and columns (in) to `in_pad` with zeros
std::vector<float> pad_rows(const HostAffine &a, uint32_t out_pad, uint32_t in_pad) {
  std::vector<float> t((size_t)out_pad * in_pad, 0.0f);
  for (uint32_t o = 0; o < a.out; ++o)
    for (uint32_t i = 0; i < a.in; ++i) t[(size_t)o * in_pad + i] = a.w[(size_t)o * a.in + i];
  return t;
}
// k_mainnet_wave's MFMA-fragment order of a weight matrix: the 2 float4 x NB n-blocks of one SUB-chunk (8 k-steps) are contiguous:
// float4 (((c*4 + u)*NB + nb)*2 + qq)*64 + lane -> W[nb*32 + r][c*64 + h*32 + 8u + 4qq .. +3], so the 16 loads of a sub-chunk
// are one scalar base + the lane's offset + small constants (no per-block vector address arithmetic).  NB is rounded up to
// the kernel's template width (1, 2, 4, 8) with all-zero blocks, so that every block index is a compile-time constant.
std::vector<float> frag_order_wave(const HostAffine &a, uint32_t out_pad) {
  const uint32_t nch = (a.in + 63) / 64, nb_real = out_pad / 32;
  const uint32_t NB = nb_real > 4 ? 8 : nb_real > 2 ? 4 : nb_real; // the kernel's block count (wave_layer_nb): absent blocks are zeros
  std::vector<float> f((size_t)nch * NB * 8 * 64 * 4, 0.0f);
  for (uint32_t c = 0; c < nch; ++c)
    for (uint32_t u = 0; u < 4; ++u)
      for (uint32_t nb = 0; nb < NB; ++nb)
        for (uint32_t qq = 0; qq < 2; ++qq)
          for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t e = 0; e < 4; ++e) {
              const uint32_t row = nb * 32 + (lane & 31), col = c * 64 + (lane >> 5) * 32 + 8 * u + 4 * qq + e;
              if (row < a.out && col < a.in) f[(((((size_t)c * 4 + u) * NB + nb) * 2 + qq) * 64 + lane) * 4 + e] = a.w[(size_t)row * a.in + col];
            }
  return f;
}

// ---- the two 16-bit number forms ----
uint16_t f32_to_bf16(float f) { // round to nearest even (weights are finite; a NaN stays a NaN)
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
float bf16_to_f32(uint16_t b) { const uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
// the bf16 triple (h, m, l) of x: each part the rounded remainder of the ones before it
std::array<uint16_t, 3> bf16_triple(float x) {
  const uint16_t hh = f32_to_bf16(x);
  const float r1 = x - bf16_to_f32(hh);
  const uint16_t mm = f32_to_bf16(r1);
  return {hh, mm, f32_to_bf16(r1 - bf16_to_f32(mm))};
}
// the fp16 pair (h, l) of x, a weight already multiplied by its row's scale
struct F16Pair {
  _Float16 hi, lo;
  std::array<uint16_t, 2> bits() const { std::array<uint16_t, 2> b; memcpy(&b[0], &hi, 2); memcpy(&b[1], &lo, 2); return b; }
};
F16Pair f16_pair(float x) {
  const _Float16 hi = (_Float16)x;
  return {hi, (_Float16)(x - (float)hi)};
}
// scale = the power of two that takes the largest |w| of a weight's ROW (= output feature) into [2^14, 2^15) (1 for an all-zero row)
float pair_scale_of(float m) { // the power of two that takes m into [2^14, 2^15); 1 for m = 0
  if (!(m > 0.0f) || !std::isfinite(m)) return 1.0f;
  int e;
  std::frexp(m, &e); // m = f x 2^e, f in [0.5, 1): m in [2^(e-1), 2^e)
  e = 15 - e;        // (kept inside 2^+-100: the scale, its inverse and their products with a batch row's scale stay normal fp32 numbers;
  return std::ldexp(1.0f, e > 100 ? 100 : e < -100 ? -100 : e); // a row beyond that fails pair_layer_ok or saturates like fp32 does)
}
float row_pair_scale(const HostAffine &a, uint32_t n) {
  float m = 0.0f;
  for (uint32_t k = 0; k < a.in; ++k) m = std::fmax(m, std::fabs(a.w[(size_t)n * a.in + k]));
  return pair_scale_of(m);
}
std::vector<float> row_pair_scales(const HostAffine &a) {
  std::vector<float> s(a.out);
  for (uint32_t n = 0; n < a.out; ++n) s[n] = row_pair_scale(a, n);
  return s;
}
std::vector<float> scale_inverses(const std::vector<float> &scales, uint32_t padded) { // 1 / scale of every output row (padded rows: 0)
  std::vector<float> v(padded, 0.0f);
  for (size_t o = 0; o < scales.size(); ++o) v[o] = 1.0f / scales[o];
  return v;
}
// May this layer run as pairs?  Two checks on its weights:
//   rows    -- every row (= output feature) carries its own scale, so a row of small weights next to rows of large ones loses nothing.
//              Within a row the pair of x = w x scale misses x by at most 2^-23 |x| while its low part is a normal fp16 number (h is
//              within 2^-11 |x| of x, and l = fp16(x - h) within 2^-12 of that) and by up to 2^-25 / scale (= 2^-39 x the row's largest
//              weight) when it is a subnormal; the row passes when the sum of what its pairs miss stays within 2^-23 of the sum of
//              its magnitudes -- the normwise error of ONE fp32 rounding per weight;
//   columns -- a column whose largest weight is more than 2^16 below the layer's largest is carried with fewer bits, which is
//              harmless while its input is no larger than the others' and wrong when the network compensates small weights with
//              large inputs (an embedding net scaled up by 2^60 in front of fc0 columns scaled down by 2^60 is the same function in
//              fp32).  The loader cannot see the inputs, so every non-zero column must reach 2^-18 of the layer's largest weight: a column
//              that small matters only through inputs 2^18 times the others', and is then still carried to 2^-21 (the bound a
//              nearly dead input unit of a trained network passes, a rescaled one does not).
// With both, the weights a kernel multiplies are those of the file to ~2^-23 normwise.  The kernels' products h.h + h.l + l.h drop
// the l.l term on top of that: at most 2^-22 of a product in the worst case (|l| <= 2^-11 of its value on both sides), ~2^-27
// typically -- about four fp32 roundoffs per product at worst, not a strict fp32 bound; that a layer's outputs stay at the fp32
// multiply-add's own normwise error (~2^-23 of (the batch row's largest input) x (the weight row's magnitudes), for any input whose
// values of consequence lie within 2^15 of the row's largest) is what the GPU suites measure against float64.  A network that
// fails stays on the bf16 triples, which have fp32's exponent range.
bool pair_layer_ok(const HostAffine &a) {
  float layer_max = 0.0f;
  std::vector<float> col_max(a.in, 0.0f);
  for (uint32_t n = 0; n < a.out; ++n) {
    const float scale = row_pair_scale(a, n);
    double miss = 0.0, mag = 0.0;
    for (uint32_t k = 0; k < a.in; ++k) {
      const float wv = a.w[(size_t)n * a.in + k], x = wv * scale;
      const F16Pair p = f16_pair(x);
      miss += std::fabs((double)x - ((double)(float)p.hi + (double)(float)p.lo));
      mag += std::fabs((double)x);
      col_max[k] = std::fmax(col_max[k], std::fabs(wv));
      layer_max = std::fmax(layer_max, std::fabs(wv));
    }
    if (miss > mag * 0x1p-23 || !std::isfinite(mag)) return false;
  }
  for (uint32_t k = 0; k < a.in; ++k)
    if (col_max[k] != 0.0f && col_max[k] < layer_max * 0x1p-18f) return false;
  return true;
}
bool within_2p20(std::initializer_list<const HostAffine *> layers) { // no weight above 2^20 in magnitude
  bool ok = true;
  for (const HostAffine *a : layers)
    for (float v : a->w) ok = ok && std::fabs(v) <= 0x1p20f;
  return ok;
}

// ---- the main net's weight stream (k_mainnet_split: P = 3, bf16 triples; k_mainnet_pair: P = 2, scaled fp16 pairs) ----
// fc0, fc1, value_fc2 back to back, every weight as its P parts = parts(layer 0..2, row, weight), in the order the kernel's LDS
// ring is read: byte (((t * NB + nb) * P + part) * 64 + lane) * 16 + 2 j = part of W[32 nb + (lane & 31)][k],
// k = 16 t + 8 h + j for fc0 (h = lane >> 5) and 32 (t >> 1) + (reg & 3) + 8 (reg >> 2) + 4 h, reg = 8 (t & 1) + j, for the two
// layers whose input is the previous layer's accumulators.  Absent rows / columns are zeros.
template <size_t P, class Parts>
std::vector<uint16_t> main_stream(const HostAffine &fc0, const HostAffine &fc1, const HostAffine &v2, uint32_t NB, uint32_t T0, Parts parts) {
  const uint32_t steps = T0 + 4 * NB;
  std::vector<uint16_t> w((size_t)steps * NB * P * 64 * 8, 0);
  auto put = [&](uint32_t t_flat, int layer, const HostAffine &a, uint32_t nb, uint32_t lane, uint32_t j, uint32_t k) {
    const uint32_t n = 32 * nb + (lane & 31);
    if (n >= a.out || k >= a.in) return;
    const std::array<uint16_t, P> part = parts(layer, n, a.w[(size_t)n * a.in + k]);
    const size_t base = ((size_t)t_flat * NB + nb) * P;
    for (size_t q = 0; q < P; ++q) w[((base + q) * 64 + lane) * 8 + j] = part[q];
  };
  for (uint32_t nb = 0; nb < NB; ++nb)
    for (uint32_t lane = 0; lane < 64; ++lane)
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t hb = lane >> 5;
        for (uint32_t t = 0; t < T0; ++t) put(t, 0, fc0, nb, lane, j, 16 * t + 8 * hb + j);
        for (uint32_t t = 0; t < 2 * NB; ++t) {
          const uint32_t reg = 8 * (t & 1) + j, k = 32 * (t >> 1) + (reg & 3) + 8 * (reg >> 2) + 4 * hb;
          put(T0 + t, 1, fc1, nb, lane, j, k);
          put(T0 + 2 * NB + t, 2, v2, nb, lane, j, k);
        }
      }
  return w;
}

// ---- the policy heads ----
// k_policy_rows' A operand of a policy head's fc2 (H -> PH): float4 ((u * PB + b) * 64 + lane) = W[32 b + (lane & 31)][8 u + 4 (lane >> 5) .. + 3]
// (four k-steps per load; the leaf's fc1 row supplies the same columns as the B operand).  Absent rows / columns are zeros.
std::vector<float> policy_frag_order(const HostAffine &a, uint32_t H, uint32_t PB) {
  const uint32_t nu = H / 8;
  std::vector<float> f((size_t)nu * PB * 64 * 4, 0.0f);
  for (uint32_t u = 0; u < nu; ++u)
    for (uint32_t b = 0; b < PB; ++b)
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t e = 0; e < 4; ++e) {
          const uint32_t row = 32 * b + (lane & 31), col = 8 * u + 4 * (lane >> 5) + e;
          if (row < a.out && col < a.in) f[(((size_t)u * PB + b) * 64 + lane) * 4 + e] = a.w[(size_t)row * a.in + col];
        }
  return f;
}
// ... and as bf16 triples, k_policy_rows<PB, true>'s A operand: 16-bit word ((((T * PB + b) * 3 + part) * 64 + lane) * 8 + j) = part of
// W[32 b + (lane & 31)][16 T + 8 (lane >> 5) + j]; absent rows / columns are zeros.
std::vector<uint16_t> policy_triple_order(const HostAffine &a, uint32_t H, uint32_t PB) {
  const uint32_t nT = H / 16;
  std::vector<uint16_t> w((size_t)nT * PB * 3 * 64 * 8, 0);
  for (uint32_t T = 0; T < nT; ++T)
    for (uint32_t b = 0; b < PB; ++b)
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t j = 0; j < 8; ++j) {
          const uint32_t row = 32 * b + (lane & 31), col = 16 * T + 8 * (lane >> 5) + j;
          if (row >= a.out || col >= a.in) continue;
          const std::array<uint16_t, 3> part = bf16_triple(a.w[(size_t)row * a.in + col]);
          const size_t base = ((size_t)T * PB + b) * 3;
          for (size_t q = 0; q < 3; ++q) w[((base + q) * 64 + lane) * 8 + j] = part[q];
        }
  return w;
}
// fc3 of a policy head as k_policy_rows keeps it in LDS: 315 rows of PH floats at a stride of PH + 4, then the 315 biases (padded to 320)
std::vector<float> policy_rows_image(const HostAffine &b, uint32_t PH) {
  const uint32_t stride = PH + 4;
  std::vector<float> img((size_t)315 * stride + 320, 0.0f);
  for (uint32_t r = 0; r < 315 && r < b.out; ++r) {
    for (uint32_t c = 0; c < b.in && c < PH; ++c) img[(size_t)r * stride + c] = b.w[(size_t)r * b.in + c];
    img[(size_t)315 * stride + r] = b.b[r];
  }
  return img;
}

// ---- the embedding nets ----
// k_embed_arows: W0^T padded to 128 floats per row, + an all-zero last row (the move rows are read from this copy)
// + rows AR_COMBINED + i (i = move id - 1, 0..164): the active move row 45 + i PLUS the stored Pokemon's move row 229 + 5 + i --
// the two halves of a move slot hold the same move unless Transform / Mimic replaced the active one, so the pass loads one row
std::vector<float> arows_rows(const HostAffine &a) { // a.w is [out = hidden][in]; row r of W0^T = column r of W
  std::vector<float> d((size_t)(AR_COMBINED + 165) * 128, 0.0f);
  for (uint32_t r = 0; r < a.in; ++r)
    for (uint32_t c = 0; c < a.out && c < 128; ++c) d[(size_t)r * 128 + c] = a.w[(size_t)c * a.in + r];
  for (uint32_t i = 0; i < 165; ++i)
    for (uint32_t c = 0; c < 128; ++c) d[(size_t)(AR_COMBINED + i) * 128 + c] = d[(size_t)(45 + i) * 128 + c] + d[(size_t)(229 + 5 + i) * 128 + c];
  return d;
}
// the dense part of W0 as bf16 triples, the A operand of dense_layer_bf16: 16-bit word ((((T * 4 + blk) * 3 + part) * 64 + lane) * 4 + j)
// = part of W0[channel 4 (lane & 31) + blk][row_of(dense feature d = 8 T + 4 (lane >> 5) + j)]  (d = 0: the bias; d >= F: zero)
template <class RowOf>
std::vector<uint16_t> dense_triple_frag(const HostAffine &a, uint32_t KT, uint32_t F, RowOf row_of) {
  std::vector<uint16_t> w((size_t)KT * 4 * 3 * 64 * 4, 0);
  for (uint32_t T = 0; T < KT; ++T)
    for (uint32_t blk = 0; blk < 4; ++blk)
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t d = 8 * T + 4 * (lane >> 5) + j, c = 4 * (lane & 31) + blk;
          if (d >= F || c >= a.out) continue;
          const std::array<uint16_t, 3> part = bf16_triple(d == 0 ? a.b[c] : a.w[(size_t)c * a.in + row_of(d)]);
          const size_t base = ((size_t)T * 4 + blk) * 3;
          for (size_t q = 0; q < 3; ++q) w[((base + q) * 64 + lane) * 4 + j] = part[q];
        }
  return w;
}
// W1 of an embedding net as scaled fp16 PAIRS in embed_layer2's order (the image keeps the three 1-KB parts per k-step that the
// bf16 triples had before; the third is zeros): 16-bit word ((((nb * 8 + T) * 3 + part) * 64 + lane) * 8 + j) = part (0: h, 1: l) of
// W1[32 nb + (lane & 31)][ar_channel(8 T + j, lane >> 5)] x scales[that row]; absent rows / channels are zeros.
std::vector<uint16_t> embed_pair_order(const HostAffine &a, uint32_t NB, const std::vector<float> &scales) {
  std::vector<uint16_t> w((size_t)NB * 8 * 3 * 64 * 8, 0);
  for (uint32_t nb = 0; nb < NB; ++nb)
    for (uint32_t T = 0; T < 8; ++T)
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t j = 0; j < 8; ++j) {
          const uint32_t o = nb * 32 + (lane & 31), c = (uint32_t)ar_channel((int)(8 * T + j), (int)(lane >> 5));
          if (o >= a.out || c >= a.in) continue;
          const std::array<uint16_t, 2> part = f16_pair(a.w[(size_t)o * a.in + c] * scales[o]).bits();
          const size_t base = ((size_t)nb * 8 + T) * 3;
          for (size_t q = 0; q < 2; ++q) w[((base + q) * 64 + lane) * 8 + j] = part[q];
        }
  return w;
}
// the image of a row kernel's LDS weights: [`sparse` one-hot rows of W0^T (stride ER_RS; slot sl = row sparse_row(sl)) + a zero row |
// dense fragment (KT k-steps, F features, feature d = row dense_row(d)) | W1's fp16 pairs | b1 | 1 / W1's row scales]
template <class SparseRow, class DenseRow>
std::vector<uint8_t> embed_image(const HostAffine &l0, const HostAffine &l1, uint32_t sparse, SparseRow sparse_row, uint32_t KT, uint32_t F, DenseRow dense_row) {
  std::vector<float> rows((size_t)(sparse + 1) * ER_RS, 0.0f);
  for (uint32_t sl = 0; sl < sparse; ++sl)
    for (uint32_t c = 0; c < l0.out && c < 128; ++c) rows[(size_t)sl * ER_RS + c] = l0.w[(size_t)c * l0.in + sparse_row(sl)];
  const uint32_t out32 = up32(l1.out);
  const std::vector<float> scales = row_pair_scales(l1);
  std::vector<uint8_t> img;
  append(img, rows);
  append(img, dense_triple_frag(l0, KT, F, dense_row));
  append(img, embed_pair_order(l1, out32 / 32, scales));
  append(img, pad_vec(l1.b, out32));
  append(img, scale_inverses(scales, out32));
  return img;
}
std::vector<uint8_t> arows_image(const HostAffine &a0, const HostAffine &a1) {
  return embed_image(a0, a1, (uint32_t)AR_SPARSE, [](uint32_t sl) { return (uint32_t)ar_sparse_row((int)sl); },
                     (uint32_t)AR_KT, (uint32_t)AR_FIXED, [](uint32_t d) { return (uint32_t)ar_dense_row((int)d); });
}
// k_embed_prows: slot sl is W0^T row sl + 5; dense feature d = 0 is the bias, d = 1..5 are W0^T rows 0..4 (the stats)
std::vector<uint8_t> prows_image(const HostAffine &p0, const HostAffine &p1) {
  return embed_image(p0, p1, (uint32_t)PR_SPARSE, [](uint32_t sl) { return sl + 5; }, (uint32_t)PR_KT, 6u, [](uint32_t d) { return d - 1; });
}

// ---- the quantized main net (oakgpu_net_load_discrete*): nn/battle/quantized/affine.h:74-99, main-net.h:36-66
std::string float_text(float v) { char buf[64]; snprintf(buf, sizeof buf, "%f", (double)v); return buf; } // std::to_string(float)
// visit_quantized_network's shape checks, in its order (network.h:182-275): the refusal, or empty
std::string quant_shape_check(uint32_t in, uint32_t h, uint32_t vh, uint32_t ph) {
  auto bad = [](const std::string &m) { return "Invalid layer size for quantized net " + m + " (check code for valid sizes)."; };
  auto ok = [](uint32_t x) { return x == 32 || x == 64 || x == 128; };
  if (in != 768) return bad("Side dim: " + std::to_string(in));
  if (!ok(h)) return bad("Hidden: " + std::to_string(h));
  if (!ok(vh)) return bad("Value hidden: " + std::to_string(vh));
  if (!ok(ph)) return bad("Policy hidden: " + std::to_string(ph));
  if (h < vh) return bad("Value hidden cannot be larger than hidden.");
  if (h < ph) return bad("Policy hidden cannot be larger than hidden.");
  return {};
}
// AffineTransform::try_copy_parameters: weight int8 = trunc(w * 64), refused unless strictly inside (-2, 2) (NaN included: its
// text is the reference's); bias int32 = trunc((b * 64) * 127), two fp32 operations (the reference's cast of a bias outside int32
// is undefined: refused here).  `rows` pads the output rows with zeros (the policy fc3 layers: 315 -> 320).  Returns the refusal, or empty.
struct QLayer { std::vector<int8_t> w; std::vector<int32_t> b; };
std::string quantize_layer(const HostAffine &a, uint32_t in, uint32_t out, uint32_t rows, const char *name, QLayer &q) {
  if (a.in != in) return "bad in dim";
  if (std::min(a.out, rows) != out) return "bad out dim";
  q.w.assign((size_t)rows * in, 0);
  q.b.assign(rows, 0);
  for (size_t i = 0; i < (size_t)out * in; ++i) {
    const float x = a.w[i];
    if (!(x < 2.0f) || !(x > -2.0f)) return std::to_string(i) + "non clamped" + float_text(x);
    q.w[i] = (int8_t)(x * 64.0f);
  }
  for (uint32_t i = 0; i < out; ++i) {
    const float x = (a.b[i] * 64.0f) * 127.0f;
    if (!(x >= -2147483648.0f && x < 2147483648.0f))
      return "quantized net: bias " + std::to_string(i) + " of " + name + " is outside int32 (" + float_text(a.b[i]) + ")";
    q.b[i] = (int32_t)x;
  }
  return {};
}
// k_mainnet_i8's LDS image.  fc0: 16 bytes ((t * NB + b) * 64 + lane) = W0[32 b + (lane & 31)][32 t + 16 (lane >> 5) + j];
// fc1 and value_fc2 (input = the previous layer's accumulators): 16 bytes ((s * NBo + b) * 64 + lane) =
// W[32 b + (lane & 31)][32 s + (j & 3) + 8 (j >> 2) + 4 (lane >> 5)] -- the k of byte j of lane half h in an accumulator tile.
std::vector<uint8_t> qnet_image(const QLayer &fc0, const QLayer &fc1, const QLayer &v2, int H, int VH) {
  const int NB = H / 32, NBv = VH / 32;
  std::vector<uint8_t> img(qi_lds_bytes(H, VH), 0);
  uint8_t *p = img.data();
  for (int t = 0; t < QI_T0; ++t)
    for (int b = 0; b < NB; ++b)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 16; ++j)
          p[((size_t)(t * NB + b) * 64 + lane) * 16 + j] = (uint8_t)fc0.w[(size_t)(32 * b + (lane & 31)) * QI_IN + 32 * t + 16 * (lane >> 5) + j];
  p += (size_t)QI_T0 * NB * 1024;
  auto acc_order = [&](const QLayer &q, int nbo) {
    for (int s = 0; s < NB; ++s)
      for (int b = 0; b < nbo; ++b)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 16; ++j)
            p[((size_t)(s * nbo + b) * 64 + lane) * 16 + j] = (uint8_t)q.w[(size_t)(32 * b + (lane & 31)) * H + 32 * s + (j & 3) + 8 * (j >> 2) + 4 * (lane >> 5)];
    p += (size_t)NB * nbo * 1024;
  };
  acc_order(fc1, NB);
  acc_order(v2, NBv);
  return img;
}

// ---- file bytes -> PackedNet.  Returns the refusal text, or empty: `net` is complete only then. ----
std::string pack_net(const void *bytes, size_t size, bool discrete, PackedNet &net) {
  const uint8_t *p = (const uint8_t *)bytes, *end = p + size;
  if (size < 8) return "network file: truncated header";
  const int activation = (int)p[0] + 1; // search.cc:127-131: byte0 = activation - 1
  if (discrete && activation != 2) return "Agent: .discrete was specified but the parsed header does not encode clamped activations.";
  if (activation != 1 && activation != 2) return "network file: unknown activation byte";
  p += 8;
  HostAffine L[12]; // p0 p1 a0 a1 fc0 fc1 v2 v3 q1a q1b q2a q2b
  for (int i = 0; i < 12; ++i)
    if (!read_affine(p, end, L[i])) return "network file: truncated or malformed layer";
  if (p != end) return "network file: trailing bytes (network.h:60-63)";
  // the quantized main net (search.cc:104-122): shapes as visit_quantized_network checks them, then try_copy_parameters layer by
  // layer in main-net.h:36-66's order; a NaN weight is refused there as "non clamped", before the non-finite check below
  QLayer Q[8]; // fc0 fc1 value_fc2 value_fc3 p1_fc2 p2_fc2 p1_fc3 p2_fc3
  if (discrete) {
    const uint32_t qh = L[4].out, qvh = L[6].out, qph = L[8].out;
    std::string bad = quant_shape_check(L[4].in, qh, qvh, qph);
    if (!bad.empty()) return bad;
    const struct { int layer; uint32_t in, out, rows; const char *name; } qs[8] = {
        {4, 768, qh, qh, "main_net.fc0"}, {5, qh, qh, qh, "main_net.fc1"}, {6, qh, qvh, qvh, "main_net.value_fc2"}, {7, qvh, 1, 1, "main_net.value_fc3"},
        {8, qh, qph, qph, "main_net.p1_policy_fc2"}, {10, qh, qph, qph, "main_net.p2_policy_fc2"},
        {9, qph, 315, 320, "main_net.p1_policy_fc3"}, {11, qph, 315, 320, "main_net.p2_policy_fc3"}};
    for (int i = 0; i < 8; ++i) {
      bad = quantize_layer(L[qs[i].layer], qs[i].in, qs[i].out, qs[i].rows, qs[i].name, Q[i]);
      if (!bad.empty()) return bad;
    }
  }
  // Non-finite parameters are refused.  The reference would load them and propagate NaN / inf through every inference (its
  // value_inference asserts !isnan in debug builds, network.h:77); a file with such a parameter is a failed training run, and
  // here an infinite weight would also split into (inf, NaN, NaN) on the bf16 pipe -- a different wrong answer than fp32's.
  static const char *const names[12] = {"pokemon_net.fc0", "pokemon_net.fc1", "active_net.fc0", "active_net.fc1", "main_net.fc0", "main_net.fc1", "main_net.value_fc2",
                                        "main_net.value_fc3", "main_net.p1_policy_fc2", "main_net.p1_policy_fc3", "main_net.p2_policy_fc2", "main_net.p2_policy_fc3"};
  for (int i = 0; i < 12; ++i) {
    bool finite = true;
    for (float v : L[i].b) finite = finite && std::isfinite(v);
    for (float v : L[i].w) finite = finite && std::isfinite(v);
    if (!finite) return std::string("network file: non-finite parameter (NaN / inf) in ") + names[i];
  }
  const HostAffine &p0 = L[0], &p1 = L[1], &a0 = L[2], &a1 = L[3], &fc0 = L[4], &fc1 = L[5], &v2 = L[6], &v3 = L[7];
  const HostAffine &q1a = L[8], &q1b = L[9], &q2a = L[10], &q2b = L[11];
  if (p0.in != 198 || a0.in != 427) return "network file: embedding input dims must be 198 / 427";
  if (p1.in != p0.out || a1.in != a0.out || fc1.in != fc0.out || v2.in != fc1.out || v3.in != v2.out || v3.out != 1)
    return "network file: inconsistent layer dims";
  if (p0.out > 128 || a0.out > 128 || p1.out > 128 || a1.out > 128) return "embedding widths above 128 unsupported";
  const uint32_t side_dim = (1 + a1.out) + 5 * (1 + p1.out);
  if (fc0.in != 2 * side_dim) return "network file: fc0 input != 2 * side embedding";
  if (fc0.out != fc1.out) return "network file: fc0/fc1 widths differ";
  const uint32_t H = up32(fc0.out), VH = up32(v2.out);
  if (H > (uint32_t)MAXH || VH > (uint32_t)MAXH) return "main-net widths above 256 unsupported";
  if (fc0.in % 4) return "embedding dim must be a multiple of 4";
  if (q1a.in != fc1.out || q2a.in != fc1.out || q1b.in != q1a.out || q2b.in != q2a.out || q1a.out != q2a.out || q1b.out != 315 || q2b.out != 315)
    return "network file: inconsistent policy-head dims";
  const uint32_t ph32 = up32(q1a.out);
  if (ph32 > (uint32_t)MAXH) return "policy hidden width above 256 unsupported";
  const uint32_t PB = ph32 > 128 ? 8 : ph32 > 64 ? 4 : ph32 > 32 ? 2 : 1, PH = 32 * PB; // k_policy_rows' block count: absent features are zeros
  const uint32_t nbr = (H > VH ? H : VH) / 32, NB = nbr > 4 ? 8 : nbr > 2 ? 4 : nbr, T0 = 4 * ((fc0.in + 63) / 64);

  net = PackedNet{};
  net.activation = activation;
  net.in_dim = (int)fc0.in; net.hidden = (int)fc0.out; net.value_hidden = (int)v2.out; net.policy_hidden = (int)q1a.out;
  net.p_hidden = (int)p0.out; net.p_out = (int)p1.out; net.a_hidden = (int)a0.out; net.a_out = (int)a1.out; net.side_dim = (int)side_dim;
  net.H = (int)H; net.VH = (int)VH; net.PH = (int)PH;
  net.T0 = (int)T0; net.NB = (int)NB; net.PB = (int)PB;
  net.b3 = v3.b[0];

  // The bf16 triple (h, m, l) of a value x is exact to 2^-24 |x| only while its low parts are normal bf16 numbers (|x| >= ~2^-102);
  // below that a part that flushes loses at most 2^-126 per factor -- an ABSOLUTE error of at most 2^-126 |other factor| per
  // product.  That is harmless unless later layers amplify it: a layer scaled by 2^-120 feeding one scaled by 2^+120 computes an
  // O(1) value in fp32, and there the lost parts would come back multiplied by 2^120.  So the triple form is used only while
  // no main-net weight exceeds 2^20 in magnitude (two layers of 256 such weights amplify by < 2^56: 2^-126 x 768 x 2^56 is
  // nothing); a network with a larger weight runs its main net on fp32 MFMA, whose products need no such care.
  net.split_safe = within_2p20({&fc0, &fc1, &v2});
  // The row kernels of the embedding passes (k_embed_prows / k_embed_arows) multiply the dense part of their first layer as bf16
  // triples (the one-hot and move rows are added in fp32) and their second layer as scaled fp16 pairs.  What a flushed part of a
  // triple loses is amplified by whatever comes BEHIND it -- the embedding nets' own second layers (p1, a1) and the main net -- so a
  // network with a weight above 2^20 in any of those runs its embedding nets through k_embed_lds (fp32 MFMA), whatever the main
  // net's mode (a layer scaled by 2^-110 in front of one scaled by 2^+110 is the same function in fp32).  And the second layers
  // must survive the pairing: pair_layer_ok, rows and columns.
  net.embed_safe = net.split_safe && within_2p20({&p1, &a1}) && pair_layer_ok(p1) && pair_layer_ok(a1);
  // fp16 pairs (k_mainnet_pair, the default): scaled per weight row and per batch row, so no absolute magnitude matters;
  // what must hold is that every weight row survives the pairing to fp32 accuracy and no column is dwarfed (pair_layer_ok)
  net.pair_safe = pair_layer_ok(fc0) && pair_layer_ok(fc1) && pair_layer_ok(v2);
  // the heads' fc2 as triples only while no weight of the heads is above 2^20 in magnitude (as for the main net: split_safe).  fc3
  // counts too: it is the later layer that multiplies back up what a flushed low part lost in fc2 (fc2 x 2^-120 in front of fc3 x
  // 2^+120 is the same function in fp32; on the triples the logits were 2.3e-4 off -- tests/test_gpu_policy.py, down120_up120)
  net.policy_safe = within_2p20({&q1a, &q2a, &q1b, &q2b});

  net.add("p_w0t", transpose(p0));
  net.add("p_b0", p0.b);
  net.add("p_w1", p1.w);
  net.add("a_w1", a1.w);
  net.add("p_b1", pad_vec(p1.b, up32(p1.out))); // (padded: embed_scatter reads whole float4 groups)
  net.add("a_w0t", transpose(a0));
  net.add("a_b0", a0.b);
  net.add("a_b1", pad_vec(a1.b, up32(a1.out)));
  net.add("a_w0d", arows_rows(a0));
  net.add("a_img", arows_image(a0, a1));
  net.add("p_img", prows_image(p0, p1));
  net.add("b0", pad_vec(fc0.b, H));
  net.add("b1", pad_vec(fc1.b, H));
  net.add("b2", pad_vec(v2.b, VH));
  net.add("w3", pad_vec(v3.w, VH));
  net.add("w0g", frag_order_wave(fc0, H));
  net.add("w1g", frag_order_wave(fc1, H));
  net.add("w2g", frag_order_wave(v2, VH));
  net.add("ws", main_stream<3>(fc0, fc1, v2, NB, T0, [](int, uint32_t, float w) { return bf16_triple(w); }));
  {
    // k_mainnet_pair's stream: (h, l) = the fp16 pair of w x its row's scale; wp_inv = 1 / scale of every row:
    // [fc0: H | fc1: H | value_fc2: VH] (padded rows: 0)
    const std::vector<float> sc[3] = {row_pair_scales(fc0), row_pair_scales(fc1), row_pair_scales(v2)};
    std::vector<float> inv = scale_inverses(sc[0], H);
    for (const std::vector<float> &more : {scale_inverses(sc[1], H), scale_inverses(sc[2], VH)}) inv.insert(inv.end(), more.begin(), more.end());
    net.add("wp_inv", inv);
    net.add("wp", main_stream<2>(fc0, fc1, v2, NB, T0, [&](int layer, uint32_t n, float w) { return f16_pair(w * sc[layer][n]).bits(); }));
  }
  net.add("q1a", pad_rows(q1a, PH, H));
  net.add("q1a_b", pad_vec(q1a.b, PH));
  net.add("q1b", pad_rows(q1b, 315, PH));
  net.add("q1b_b", q1b.b);
  net.add("q2a", pad_rows(q2a, PH, H));
  net.add("q2a_b", pad_vec(q2a.b, PH));
  net.add("q2b", pad_rows(q2b, 315, PH));
  net.add("q2b_b", q2b.b);
  net.add("q1a_f", policy_frag_order(q1a, H, PB));
  net.add("q2a_f", policy_frag_order(q2a, H, PB));
  if (PH <= 64) { // (PolicyRows<PB>::WB_LDS: the rows fit the CU's LDS)
    net.add("q1b_img", policy_rows_image(q1b, PH));
    net.add("q2b_img", policy_rows_image(q2b, PH));
  }
  if (net.policy_safe) {
    net.add("q1a_t", policy_triple_order(q1a, H, PB));
    net.add("q2a_t", policy_triple_order(q2a, H, PB));
  }
  net.discrete = discrete;
  if (discrete) {
    net.q_H = (int)fc0.out; net.q_VH = (int)v2.out; net.q_PH = (int)q1a.out;
    const std::vector<uint8_t> img = qnet_image(Q[0], Q[1], Q[2], net.q_H, net.q_VH);
    net.q_img_bytes = (int)img.size();
    net.q_b3 = Q[3].b[0];
    net.add("q.img", img);
    net.add("q.b0", Q[0].b);
    net.add("q.b1", Q[1].b);
    net.add("q.b2", Q[2].b);
    net.add("q.w3", Q[3].w);
    static const char *const head[2][4] = {{"q.pw2[0]", "q.pb2[0]", "q.pw3[0]", "q.pb3[0]"}, {"q.pw2[1]", "q.pb2[1]", "q.pw3[1]", "q.pb3[1]"}};
    for (int hd = 0; hd < 2; ++hd) {
      net.add(head[hd][0], Q[4 + hd].w);
      net.add(head[hd][1], Q[4 + hd].b);
      net.add(head[hd][2], Q[6 + hd].w);
      net.add(head[hd][3], Q[6 + hd].b);
    }
  }
  return {};
}

} // namespace
} // namespace pack
} // namespace oak
