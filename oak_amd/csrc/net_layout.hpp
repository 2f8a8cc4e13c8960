// oak_amd/csrc/net_layout.hpp -- the layout constants and index functions that the leaf kernels (leafnet.hip, mainnet_i8.hpp) and
// the host-side weight packer (net_pack.hpp) share.  Plain C++: a constexpr function is callable from host and device code alike.
// Each is defined here and nowhere else.
#pragma once
#include <stddef.h>

namespace oak {

constexpr int ER_RS = 128; // LDS weight row (floats) of k_embed_arows / k_embed_prows (a half-wave reads a whole row per instruction:
                           // contiguous, conflict-free at any stride -- no padding)

// k_embed_arows
constexpr int AR_SPARSE = 64;                      // LDS-resident one-hot rows (ar_sparse_slot) + a zero row
constexpr int AR_FIXED = 36, AR_KT = (AR_FIXED + 7) / 8; // (dense features in k-steps of eight)
constexpr int AR_COMBINED = 428; // first precombined (active + stored) move row of a_w0d: behind W0^T's 427 rows and the zero row
// channel held by register s (0..63) of a lane in half hh: the C layout of four 32x32 MFMA blocks, block b's row i being
// channel 4 i + b (so that a lane's float4 of a weight row feeds the four blocks)
constexpr int ar_channel(int s, int hh) { return 4 * ((s & 3) + 8 * ((s & 15) >> 2) + 4 * hh) + (s >> 4); }
// W0^T row of dense feature d (1..35; 0 is the bias): active stats, boosts, volatiles, the stored Pokemon's stats
constexpr int ar_dense_row(int d) { return d < 6 ? d - 1 : d < 12 ? 20 + (d - 6) : d < 31 ? 26 + (d - 12) : 229 + (d - 31); }
// W0^T row of a compact LDS one-hot slot (types 5..19, rows 209..228, rows 398..426): the inverse of the kernel's ar_sparse_slot
constexpr int ar_sparse_row(int slot) { return slot < 15 ? slot + 5 : slot < 35 ? slot - 15 + 209 : slot - 35 + 398; }

// k_embed_prows
constexpr int PR_SPARSE = 193, PR_KT = 1; // (6 dense features: one k-step of eight)

constexpr int MAXH = 256; // the widest main-net / policy layer (padded)

// k_mainnet_i8
constexpr int QI_IN = 768;          // the battle embedding (visit_quantized_network: In == 768)
constexpr int QI_T0 = QI_IN / 32;   // fc0's k-steps of 32 bytes
constexpr size_t qi_lds_bytes(int H, int VH) { return (size_t)(QI_T0 * (H / 32) + (H / 32) * (H / 32) + (H / 32) * (VH / 32)) * 1024; }

} // namespace oak
