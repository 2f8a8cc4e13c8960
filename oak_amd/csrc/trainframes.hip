// oak_amd/csrc/trainframes.hip -- training batches from `.battle.data` records on the GPU (the contract is in include/oakgpu.h).
//
//   k_frames_valid   : one lane per record, frames with iterations >= min_iterations (cached per min_iterations by the corpus)
//   k_frames_eligible: a window corpus (replaywindow.hip) only: the eligible records listed on the device, one workgroup, 1,024 records a pass
//   k_frames_draw    : one lane per draw, pyoak.sample's rule with a fast_prng stream per draw -> picks (record, frame)
//   k_frames_order   : picks -> lane order, longest prefix first (one workgroup, counting sort by frame)
//   k_frames_pick    : persistent lanes fed from eight queue heads, one pick at a time: the replay check's walk on the register
//                      engine (record_walk.hpp) up to the picked frame -> a snapshot
//                      (battle, durations, request, both choice lists, status)
//   k_frames_requests: the same snapshot head for states the caller holds (oakgpu_encode_battles_dev)
//   k_frames_encode  : one wave per row: the dense encoder rows built in LDS, streamed out; targets decoded from the frame bytes
// There is no CPU fallback in this library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/oakgpu.h"
#include "gen1_device.hpp"
#include "gen1_regs.hpp"
#include "record_walk.hpp"
#include "oakgpu_internal.h"
#include "encode_index.hpp"
#include "fast_prng.hpp"
#include "game_rows.hpp"

namespace oak {
namespace tf {
using namespace walk;

constexpr uint32_t POKEMON_IN = 198, ACTIVE_IN = 229, POLICY_DIM = 315;
constexpr uint32_t ROW_POKEMON = 2 * 6 * POKEMON_IN, ROW_ACTIVE = 2 * ACTIVE_IN; // floats per row

// A snapshot's head, 12 dwords (three 16-byte stores): [0] status | request << 8 | n1 << 16 | n2 << 24, [1] where, [2] [3] the
// sides' duration words, [4] [5] P1's choice bytes 0..7, [6] [7] P2's, [8] choice byte 8 of P1 | of P2 << 8, [9] the frame's byte
// offset inside its record, [10] the record.  The battle itself is 384 bytes in a slot of its own.
constexpr uint32_t META_WORDS = 12;

template <class C>
__device__ __forceinline__ void store_meta(uint32_t *meta, uint32_t slot, uint32_t status, uint32_t request, uint32_t where, uint32_t d0, uint32_t d1,
                                           const C &l1, const C &l2, uint32_t rel, uint32_t rec) {
  uint4 *m = (uint4 *)(meta + (size_t)slot * META_WORDS);
  m[0] = make_uint4(status | (request << 8) | (l1.n << 16) | (l2.n << 24), where, d0, d1);
  m[1] = make_uint4((uint32_t)l1.lo, (uint32_t)(l1.lo >> 32), (uint32_t)l2.lo, (uint32_t)(l2.lo >> 32));
  m[2] = make_uint4(l1.hi | (l2.hi << 8), rel, rec, 0);
}
__device__ __forceinline__ void store_meta_failed(uint32_t *meta, uint32_t slot, uint32_t status, uint32_t where) {
  uint4 *m = (uint4 *)(meta + (size_t)slot * META_WORDS);
  m[0] = make_uint4(status, where, 0, 0);
  m[1] = make_uint4(0, 0, 0, 0);
  m[2] = make_uint4(0, 0, 0, 0);
}

// ---- sampling --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_frames_valid(const uint8_t *records, const uint64_t *offsets, const uint16_t *frames, const uint8_t *malformed,
                                                      uint32_t n, uint32_t min_iterations, uint32_t *valid) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  uint32_t v = 0;
  if (!malformed[r]) {
    const uint8_t *fp = records + offsets[r] + 391;
    for (uint32_t k = 0, nf = frames[r]; k < nf; ++k) {
      v += load_u32(fp + 3) >= min_iterations;
      fp += frame_bytes(fp[0]);
    }
  }
  valid[r] = v;
}

// draw i: fast_prng seeded with seed + i; record = eligible[uniform_64 % E]; frame = the (uniform_64 % V)-th valid frame of it
__global__ __launch_bounds__(256) void k_frames_draw(const uint8_t *records, const uint64_t *offsets, const uint32_t *valid, const uint32_t *eligible,
                                                     uint32_t n_eligible, uint32_t min_iterations, uint64_t seed, uint32_t n, uint32_t *picks) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  FastPrng g;
  g.seed(seed + i);
  const uint32_t h0 = g.next32(), l0 = g.next32(), h1 = g.next32(), l1 = g.next32(); // uniform_64 = hi << 32 | lo
  const uint32_t r = eligible[(((uint64_t)h0 << 32) | l0) % n_eligible];
  uint32_t j = (uint32_t)((((uint64_t)h1 << 32) | l1) % valid[r]); // (an eligible record has at least one valid frame)
  const uint8_t *fp = records + offsets[r] + 391;
  uint32_t f = 0;
  for (;; ++f) { // ends inside the record: it holds valid[r] > j valid frames
    if (load_u32(fp + 3) >= min_iterations) {
      if (j == 0) break;
      --j;
    }
    fp += frame_bytes(fp[0]);
  }
  *(uint2 *)(picks + 2 * (size_t)i) = make_uint2(r, f);
}

// ---- lane order of a batch of picks: frame descending, longest prefix first
__global__ __launch_bounds__(1024) void k_frames_order(const uint32_t *picks, uint32_t n, uint32_t *order) {
  order_desc(n, order, [&](uint32_t i) { return picks[2 * (size_t)i + 1]; });
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------
struct PickArgs {
  const uint8_t *records;   // the corpus: file bytes, unchanged
  const uint64_t *offsets;  // n_records
  const uint16_t *frames;   // n_records
  const uint8_t *malformed; // n_records
  const uint8_t *aligned;   // n_records x 384 (k_replay_gather)
  const uint8_t *first;     // n_records: the first request
  const uint32_t *picks;    // n x 2
  const uint32_t *order;    // n: queue position -> pick
  uint8_t *snap;            // n x 384
  uint32_t *meta;           // n x META_WORDS
  uint32_t *heads;          // QUEUE_HEADS counters, QUEUE_HEAD_STRIDE words apart (zeroed before every launch)
  uint32_t n_records, n;
};
constexpr int PICK_COLD_BYTES = (sizeof(PickArgs) + 15) & ~15;
constexpr int PICK_LDS_BYTES = 24 * 64 * 4 + TABLE_PAD + PICK_COLD_BYTES;

// Persistent lanes, one pick each, refilled from the queue (record_walk.hpp) when their pick is settled; the queue is k_frames_order's
// order, longest prefix first.  Per frame k of the pick's record: the replay check (frame_check), and on a playable frame at k == f
// the snapshot, else the update.  The grid is the batch's waves up to what the device holds (resident_walk_waves).
template <int WPS>
__global__ __launch_bounds__(64, WPS) void k_frames_pick(PickArgs a_in) {
  extern __shared__ __align__(16) uint8_t smem[];
  lds_u32 *party = (lds_u32 *)smem;
  using ER = EngineR<64, false>;
  Tables T = stage_tables((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4, OAK_MOVE_WORDS, OAK_MOVE_MAXPP, OAK_SPECIES_W0, OAK_SPECIES_W1, OAK_TYPE_CHART, OAK_BOOSTS);
  lds_u32 *cold = (lds_u32 *)((lds_u8 *)smem + ER::PARTY_WORDS * 64 * 4 + TABLE_PAD); // the arguments, parked (cold_ptr_at)
  if (threadIdx.x < sizeof(PickArgs) / 4) cold[threadIdx.x] = ((const uint32_t *)&a_in)[threadIdx.x];
  __syncthreads();
#define PA_PTR(field, type) cold_ptr_at<type>(cold, offsetof(PickArgs, field))
  const uint32_t wl = threadIdx.x & 63;
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)cold[offsetof(PickArgs, n) / 4]);
  ER e;
  e.m = party + threadIdx.x;
  e.T = T;
  uint32_t slot = LANE_NONE, f = 0, k = 0, res = 0, mn = 0, c1 = 0, c2 = 0; // slot: this lane's pick, or none yet / none left
  const uint8_t *fp = nullptr; // frame k of this lane's record
  uint32_t ust = queue_state(blockIdx.x);
  for (;;) {
    const bool need = slot == LANE_NONE;
    const uint64_t mask = __ballot(need);
    bool load = false;
    if (refill_due(ust, mask, __ballot(slot < LANE_DONE) != 0)) {
      uint32_t my = 0;
      const bool got = queue_take(ust, cold, offsetof(PickArgs, heads), n, need, mask, wl, my);
      if (need) {
        if (got) { slot = PA_PTR(order, const uint32_t *)[my]; load = true; }
        else slot = LANE_DONE;
      }
    } else if (need && queue_dry(ust)) slot = LANE_DONE;
    if (__ballot(load)) {
      if (load) { // the pick: settled here when it names no frame of a well-formed, finished game
        const uint2 pk = *(const uint2 *)(PA_PTR(picks, const uint32_t *) + 2 * (size_t)slot);
        const uint32_t r = pk.x;
        f = pk.y;
        uint32_t status = STATUS_PENDING, where = 0;
        if (r >= cold[offsetof(PickArgs, n_records) / 4]) { status = OAKGPU_PICK_RANGE; where = f; }
        else if (PA_PTR(malformed, const uint8_t *)[r]) status = OAKGPU_REPLAY_MALFORMED;
        else {
          const uint32_t nf = PA_PTR(frames, const uint16_t *)[r];
          const uint8_t *rec = PA_PTR(records, const uint8_t *) + PA_PTR(offsets, const uint64_t *)[r];
          const uint32_t stored = rec[390] & 15;
          if (f >= nf) { status = OAKGPU_PICK_RANGE; where = f; }
          else if (stored < R_WIN || stored > R_TIE) { status = OAKGPU_REPLAY_RESULT; where = nf; }
          else {
            e.load_battle_global(PA_PTR(aligned, const uint8_t *) + (size_t)r * 384, 0, 0); // zero durations (frames.h:57-59)
            res = PA_PTR(first, const uint8_t *)[r];
            fp = rec + 391;
            k = 0;
            mn = fp[0]; c1 = fp[1]; c2 = fp[2];
          }
        }
        if (status != STATUS_PENDING) {
          store_meta_failed(PA_PTR(meta, uint32_t *), slot, status, where);
          slot = LANE_NONE;
        }
      }
    }
    if (__ballot(slot != LANE_DONE) == 0) break;
    if (slot < LANE_DONE) {
      typename ER::Choices l1, l2;
      const uint32_t status = frame_check(e, res, mn, c1, c2, l1, l2).status;
      if (status == STATUS_PENDING) {
        if (k == f) { // the picked frame: the snapshot
          const uint32_t r = PA_PTR(picks, const uint32_t *)[2 * (size_t)slot];
          const uint32_t rel = (uint32_t)(fp - (PA_PTR(records, const uint8_t *) + PA_PTR(offsets, const uint64_t *)[r]));
          e.store_battle_global(PA_PTR(snap, uint8_t *) + (size_t)slot * 384);
          store_meta(PA_PTR(meta, uint32_t *), slot, OAKGPU_REPLAY_OK, res, k, e.S.dur, e.F.dur, l1, l2, rel, r);
          slot = LANE_NONE;
        } else {
          res = play_frame(e, fp, mn, c1, c2, true); // (k < f: the next frame exists)
          ++k;
        }
      }
      if (status != STATUS_PENDING) { // (behind the join, as k_replay_records' verdict)
        store_meta_failed(PA_PTR(meta, uint32_t *), slot, status, k);
        slot = LANE_NONE;
      }
    }
  }
#undef PA_PTR
}

// The snapshot head of states the caller holds: durations as given, the engine's legal choices for the request (none when the
// battle has ended).  The battle is encoded from where it is.
__global__ __launch_bounds__(64) void k_frames_requests(const uint8_t *battles, const uint8_t *durations, const uint8_t *results, uint32_t n, uint32_t *meta) {
  __shared__ uint32_t party_s[24 * 64];
  using ER = EngineR<64, false>;
  const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= n) return;
  ER e;
  e.m = (lds_u32 *)party_s + threadIdx.x;
  e.T = Tables{}; // no tables are staged here: load_battle_global and choices() read none, and a null table faults where junk would not
  const uint2 d = *(const uint2 *)(durations + 8 * (size_t)gid);
  e.load_battle_global(battles + (size_t)gid * 384, d.x, d.y);
  const uint32_t res = results[gid];
  typename ER::Choices l1{0, 0, 0}, l2{0, 0, 0};
  if (!(res & 15)) {
    l1 = e.choices(e.S, (res >> 4) & 3);
    l2 = e.choices(e.F, (res >> 6) & 3);
  }
  store_meta(meta, gid, OAKGPU_REPLAY_OK, res, 0, d.x, d.y, l1, l2, 0, 0);
}

// policy_index reads the party through two ids of the state; a state the caller holds (or junk order bytes in a record) may carry
// ids that point outside the 184 bytes of the side
__device__ __forceinline__ bool choice_in_side(const uint8_t *side, uint32_t choice) {
  const uint32_t kind = choice & 3, data = choice >> 2;
  if (kind == 1) return data == 0 || (data <= 4 && side[176] - 1u < 6u);
  if (kind == 2) return data - 1u < 6u && side[176 + data - 1] - 1u < 6u;
  return true;
}

// ---- the rows --------------------------------------------------------------------------------------------------------------------
struct EncodeArgs {
  const uint8_t *battles;  // n x 384: the snapshots, or the caller's states
  const uint32_t *meta;    // n x META_WORDS
  const uint8_t *records;  // targets: the corpus bytes and its record offsets (null: positions only)
  const uint64_t *offsets;
  oakgpu_encoded_frames out;
  uint32_t n;
};

// the DENSE Encode::Battle::Pokemon::write (encode/battle/battle.h:201-206) of 24 stored bytes into 198 cleared cells
__device__ __forceinline__ void write_pokemon(const uint8_t *pk, uint32_t sleep, float *t) {
  t[0] = __fdiv_rn((float)load_u16(pk), 703.0f);
#pragma unroll
  for (uint32_t i = 1; i < 5; ++i) t[i] = __fdiv_rn((float)load_u16(pk + 2 * i), 999.0f);
#pragma unroll
  for (uint32_t s = 0; s < 4; ++s) { // assigned slot by slot: a move held twice shows its last slot (MoveSlots::write, :64-72)
    const uint32_t id = pk[10 + 2 * s], pp = pk[11 + 2 * s];
    if (id - 1u < 164u) t[5 + id - 1] = pp ? 1.0f : 0.0f;
  }
  const uint32_t st = pk[20];
  if (st) {
    const uint32_t idx = status_index(st, sleep);
    if (idx < 14) t[169 + idx] = 1.0f;
  }
  const uint32_t t1 = pk[22] & 15, t2 = pk[22] >> 4;
  if (t1 < 15) t[183 + t1] = 1.0f;
  if (t2 < 15) t[183 + t2] = 1.0f;
}

// the DENSE Encode::Battle::Active::write (:465-479) of the 32 active bytes and the side's duration word into 229 cleared cells.  The
// reference's zero for a disabled move lands behind the move block (at cell 209 + id), where its own duration writer or the next
// row's writer runs over it or it falls outside the row: no cell of the row changes, so nothing is written for it here.
__device__ __forceinline__ void write_active(const uint8_t *act, uint32_t dur, float *t) {
  t[0] = __fdiv_rn((float)load_u16(act), 703.0f);
#pragma unroll
  for (uint32_t i = 1; i < 5; ++i) t[i] = __fdiv_rn((float)load_u16(act + 2 * i), 999.0f);
  const uint32_t t1 = act[11] & 15, t2 = act[11] >> 4;
  if (t1 < 15) t[5 + t1] = 1.0f;
  if (t2 < 15) t[5 + t2] = 1.0f;
#pragma unroll
  for (uint32_t i = 0; i < 6; ++i) { // Boosts::write (:251-264): float(num) / den of libpkmn/data/boosts.h, times 1/4 (acc, eva: 1/3)
    const int st = (int)((((act[12 + (i >> 1)] >> (4 * (i & 1))) & 15) ^ 8) - 8);
    const float num = st == -6 ? 25.f : st == -5 ? 28.f : st == -4 ? 33.f : st == -3 ? 40.f : st == -2 ? 50.f : st == -1 ? 66.f
                      : st == 0 ? 1.f : st == 1 ? 15.f : st == 2 ? 2.f : st == 3 ? 25.f : st == 4 ? 3.f : st == 5 ? 35.f : 4.f;
    const float den = st < 0 ? 100.f : (st == 1 || st == 3 || st == 5) ? 10.f : 1.f;
    t[20 + i] = __fmul_rn(__fdiv_rn(num, den), i < 4 ? 0.25f : (float)(1 / 3.0));
  }
  const uint32_t vlo = load_u32(act + 16), vhi = load_u32(act + 20);
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) t[26 + i] = (float)((vlo >> (i < 2 ? i : i + 2)) & 1); // bide, thrashing, then charging(4) .. transform(17)
  t[42] = __fdiv_rn((float)((vlo >> 24) | ((vhi & 0xFF) << 8)), 65535.0f);
  t[43] = __fdiv_rn((float)((vhi >> 8) & 0xFF), 177.0f);
  t[44] = (float)(vhi >> 27) * 0.0625f;
#pragma unroll
  for (uint32_t s = 0; s < 4; ++s) {
    const uint32_t id = act[24 + 2 * s], pp = act[25 + 2 * s];
    if (id - 1u < 164u) t[45 + id - 1] = pp ? 1.0f : 0.0f;
  }
  const uint32_t confusion = (dur >> 18) & 7, disable = (dur >> 21) & 15, attacking = (dur >> 25) & 7, binding = (dur >> 28) & 7;
  if (confusion - 1u < 5u) t[209 + confusion - 1] = 1.0f;
  if (disable - 1u < 8u) t[214 + disable - 1] = 1.0f;
  if (attacking - 1u < 3u) t[222 + attacking - 1] = 1.0f;
  if (binding - 1u < 4u) t[225 + binding - 1] = 1.0f;
}

// One wave per row.  The row's 12 Pokemon blocks and 2 active blocks are cleared in LDS, lanes 0..13 scatter one block's few dozen
// non-zeros each, and the wave streams the 11.3 KB out (16-byte stores for `pokemon`; a row of `active` is 1,832 bytes, so its rows
// are 8-byte aligned and go out in 8-byte stores).  The small tensors are written straight from registers.
__global__ __launch_bounds__(64) void k_frames_encode(EncodeArgs a) {
  __shared__ __align__(16) float buf[ROW_POKEMON + ROW_ACTIVE + 2];
  const uint32_t row = blockIdx.x, tid = threadIdx.x;
  const uint32_t *mt = a.meta + (size_t)row * META_WORDS;
  const uint32_t m0 = mt[0];
  const uint32_t status = m0 & 0xFF;
  const bool ok = status == OAKGPU_REPLAY_OK;
  const uint8_t *battle = a.battles + (size_t)row * 384;
  for (uint32_t i = tid; i < (ROW_POKEMON + ROW_ACTIVE + 2) / 4; i += 64) ((float4 *)buf)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  if (tid < 12) {
    const uint32_t s = tid / 6, pos = tid - 6 * s;
    float ratio = 0.0f;
    if (ok) {
      const uint8_t *side = battle + 184 * s;
      const uint32_t id = side[176 + pos];
      if (id - 1u < 6u) {
        const uint8_t *pk = side + 24 * (id - 1);
        const uint32_t hp = load_u16(pk + 18);
        if (hp) {
          ratio = __fdiv_rn((float)hp, (float)load_u16(pk));
          write_pokemon(pk, (mt[2 + s] >> (3 * pos)) & 7, buf + tid * POKEMON_IN);
        }
      }
    }
    a.out.hp[(size_t)row * 12 + tid] = ratio;
  } else if (tid < 14 && ok) {
    const uint32_t s = tid - 12;
    const uint8_t *side = battle + 184 * s;
    const uint32_t id = side[176];
    if (id - 1u < 6u && load_u16(side + 24 * (id - 1) + 18) != 0) write_active(side + 144, mt[2 + s], buf + ROW_POKEMON + s * ACTIVE_IN);
  }
  __syncthreads();
  float4 *dp = (float4 *)(a.out.pokemon + (size_t)row * ROW_POKEMON);
  for (uint32_t i = tid; i < ROW_POKEMON / 4; i += 64) dp[i] = ((const float4 *)buf)[i];
  float2 *da = (float2 *)(a.out.active + (size_t)row * ROW_ACTIVE);
  for (uint32_t i = tid; i < ROW_ACTIVE / 2; i += 64) da[i] = ((const float2 *)(buf + ROW_POKEMON))[i];

  const bool targets = a.records != nullptr;
  const uint8_t *fr = ok && targets ? a.records + a.offsets[mt[10]] + mt[9] : nullptr;
  uint32_t k1 = (m0 >> 16) & 0xFF, k2 = m0 >> 24; // positions only: the engine's counts
  if (fr) { k1 = (fr[0] & 15) + 1; k2 = (fr[0] >> 4) + 1; } // (equal to the engine's: the pick is OK)
  if (tid < 18) {
    const uint32_t s = tid / 9, j = tid - 9 * s, kk = s ? k2 : k1;
    int64_t index = 0;
    float emp = 0.0f, nash = 0.0f;
    if (ok) {
      const uint64_t lo = (uint64_t)mt[4 + 2 * s] | ((uint64_t)mt[5 + 2 * s] << 32);
      const uint32_t choice = j < 8 ? (uint32_t)(lo >> (8 * j)) & 0xFF : (mt[8] >> (8 * s)) & 0xFF;
      index = j >= kk ? (int64_t)POLICY_DIM : choice_in_side(battle + 184 * s, choice) ? (int64_t)policy_index(battle + 184 * s, choice) : 0; // (0: as a pass)
      if (fr && j < kk) { // Update::write_to_tensor (train/battle/compressed-frame.h:141-163): u16 / 65535.0f
        const uint8_t *p = fr + 11 + (s ? 4 * k1 : 0);
        emp = __fdiv_rn((float)load_u16(p + 2 * j), 65535.0f);
        nash = __fdiv_rn((float)load_u16(p + 2 * kk + 2 * j), 65535.0f);
      }
    }
    a.out.choice_indices[(size_t)row * 18 + tid] = index;
    if (targets) {
      a.out.empirical_policies[(size_t)row * 18 + tid] = emp;
      a.out.nash_policies[(size_t)row * 18 + tid] = nash;
    }
  } else if (tid < 20) {
    const uint32_t s = tid - 18;
    a.out.k[(size_t)row * 2 + s] = ok ? (uint8_t)(s ? k2 : k1) : 0;
    if (targets) a.out.choice[(size_t)row * 2 + s] = fr ? fr[1 + s] : 0;
  } else if (tid == 20 && targets) {
    a.out.iterations[row] = fr ? load_u32(fr + 3) : 0;
    a.out.empirical_value[row] = fr ? __fdiv_rn((float)load_u16(fr + 7), 65535.0f) : 0.0f;
    a.out.nash_value[row] = fr ? __fdiv_rn((float)load_u16(fr + 9), 65535.0f) : 0.0f;
    float score = 0.0f;
    if (fr) { // PKMN::score (libpkmn/pkmn.h:174-190) of the stored result byte
      const uint32_t type = (a.records + a.offsets[mt[10]])[390] & 15;
      score = type == R_WIN ? 1.0f : type == R_LOSE ? 0.0f : 0.5f;
    }
    a.out.score[row] = score;
    a.out.status[row] = (uint8_t)status;
    a.out.where[row] = mt[1];
  }
}

// A window corpus' eligible records, in record order, listed on the device: one workgroup, 1,024 records a pass (game_rows.hpp's scan)
__global__ __launch_bounds__(1024) void k_frames_eligible(const uint16_t *frames, const uint8_t *malformed, const uint32_t *valid, uint32_t n,
                                                          uint32_t max_battle_length, uint32_t *list, uint32_t *count) {
  __shared__ uint32_t wave_total[16];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t r = base + threadIdx.x;
    const bool in = r < n && !malformed[r] && valid[r] != 0 && (max_battle_length == 0 || frames[r] <= max_battle_length);
    const game_rows::ScanPass<uint32_t> s = game_rows::scan_pass<uint32_t>(in ? 1u : 0u, wave_total);
    if (in) list[carry + s.before] = r;
    carry += s.total;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(256) void k_frames_count_ok(const uint8_t *status, uint32_t n, uint32_t *count) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint64_t b = __ballot(i < n && status[i] == OAKGPU_REPLAY_OK);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (uint32_t)__popcll(b));
}

} // namespace tf
} // namespace oak

// ---- host ------------------------------------------------------------------------------------------------------------------------
// (struct oakgpu_corpus: oakgpu_internal.h -- corpuseval.hip walks the same corpus)

namespace {

void cache_free(oakgpu_corpus *k) { // the sampling caches (the stream must be idle)
  for (auto &v : k->valids) if (v.d) (void)hipFree(v.d);
  for (auto &e : k->eligibles) if (e.d) (void)hipFree(e.d);
  k->valids.clear();
  k->eligibles.clear();
}

void corpus_free(oakgpu_corpus *k) {
  for (void *p : {(void *)k->records, (void *)k->malformed, (void *)k->aligned, (void *)k->first, (void *)k->offsets, (void *)k->frames, (void *)k->picks,
                  (void *)k->order, (void *)k->meta, (void *)k->snap, (void *)k->heads})
    if (p) (void)hipFree(p);
  cache_free(k);
  if (k->eval && k->eval_free) k->eval_free(k->eval);
  if (k->window && k->window_free) k->window_free(k->window);
  delete k;
}

// A window corpus (replaywindow.hip): the valid counts stay on the device, k_frames_eligible lists the records, and the host reads E alone.
int window_eligible(oakgpu_corpus *k, hipStream_t stream, uint32_t min_iterations, uint32_t max_battle_length) {
  using namespace oak::tf;
  const oakgpu_corpus::Valid *va = nullptr;
  for (const auto &v : k->valids) if (v.min_iterations == min_iterations) va = &v;
  if (!va) {
    oakgpu_corpus::Valid v{min_iterations, nullptr, {}};
    if (dev_alloc(v.d, k->n)) return -1;
    if (k->n) hipLaunchKernelGGL(k_frames_valid, dim3((k->n + 255) / 256), dim3(256), 0, stream, k->records, k->offsets, k->frames, k->malformed, k->n, min_iterations, v.d);
    k->valids.push_back(std::move(v)); // (kept even when what follows fails: a kernel may be running on it, and cache_free frees it behind a wait)
    va = &k->valids.back();
  }
  oakgpu_corpus::Eligible e{min_iterations, max_battle_length, 0, nullptr, va->d};
  if (dev_alloc(e.d, (size_t)k->n + 1)) return -1; // the list, and its length behind it
  hipLaunchKernelGGL(k_frames_eligible, dim3(1), dim3(1024), 0, stream, k->frames, k->malformed, va->d, k->n, max_battle_length, e.d, e.d + k->n);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipMemcpyAsync(&e.count, e.d + k->n, 4, hipMemcpyDeviceToHost, stream);
  const hipError_t done = hipStreamSynchronize(stream); // (always: the kernel may be running on e.d)
  if (err == hipSuccess) err = done;
  if (err != hipSuccess) {
    (void)hipFree(e.d);
    return oakgpu_fail_hip((int)err, "oakgpu_frames_sample_dev: k_frames_eligible");
  }
  k->eligibles.push_back(e);
  return 0;
}

int corpus_reserve(oakgpu_corpus *k, uint32_t n) {
  if (n <= k->capacity) return 0;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(k->ctx);
  HIPCHK(hipStreamSynchronize(stream)); // (an earlier batch may still read the old workspace)
  for (void *p : {(void *)k->picks, (void *)k->order, (void *)k->meta, (void *)k->snap}) if (p) (void)hipFree(p);
  k->picks = k->order = k->meta = nullptr;
  k->snap = nullptr;
  k->capacity = 0;
  if (dev_alloc(k->picks, (size_t)n * 2) || dev_alloc(k->order, n) || dev_alloc(k->meta, (size_t)n * oak::tf::META_WORDS) || dev_alloc(k->snap, (size_t)n * 384))
    return -1;
  k->capacity = n;
  return 0;
}

int check_out(const oakgpu_encoded_frames *o, const char *who) {
  static char msg[160];
  if (!o || !o->pokemon || !o->active || !o->hp || !o->choice_indices || !o->k || !o->choice || !o->iterations || !o->empirical_policies ||
      !o->nash_policies || !o->empirical_value || !o->nash_value || !o->score || !o->status || !o->where) {
    snprintf(msg, sizeof msg, "%s: null tensor pointer", who);
    return oakgpu_fail_msg(msg);
  }
  if (((uintptr_t)o->pokemon & 15) || ((uintptr_t)o->active & 7) || ((uintptr_t)o->hp & 3) || ((uintptr_t)o->choice_indices & 7) || ((uintptr_t)o->iterations & 3) ||
      ((uintptr_t)o->empirical_policies & 3) || ((uintptr_t)o->nash_policies & 3) || ((uintptr_t)o->empirical_value & 3) || ((uintptr_t)o->nash_value & 3) ||
      ((uintptr_t)o->score & 3) || ((uintptr_t)o->where & 3)) {
    snprintf(msg, sizeof msg, "%s: misaligned tensor (pokemon: 16 bytes; active, choice_indices: 8; the other 4-byte types: 4)", who);
    return oakgpu_fail_msg(msg);
  }
  return 0;
}

// the per-row bytes of the 14 tensors, in the order of the struct's fields
constexpr size_t ROW_BYTES[14] = {2 * 6 * 198 * 4, 2 * 229 * 4, 12 * 4, 18 * 8, 2, 2, 4, 18 * 4, 18 * 4, 4, 4, 4, 1, 4};
static_assert(sizeof(oakgpu_encoded_frames) == 14 * sizeof(void *), "a struct of 14 pointers");

int encode_picks(oakgpu_ctx *c, oakgpu_corpus *k, const uint32_t *picks, uint32_t n, const oakgpu_encoded_frames *out) {
  using namespace oak::tf;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  hipLaunchKernelGGL(k_frames_order, dim3(1), dim3(1024), 0, stream, picks, n, k->order);
  HIPCHK(hipMemsetAsync(k->heads, 0, QUEUE_HEADS * QUEUE_HEAD_STRIDE * 4, stream));
  const PickArgs pa{k->records, k->offsets, k->frames, k->malformed, k->aligned, k->first, picks, k->order, k->snap, k->meta, k->heads, k->n, n};
  hipLaunchKernelGGL((k_frames_pick<4>), dim3(std::min((n + 63) / 64, k->resident_waves)), dim3(64), PICK_LDS_BYTES, stream, pa);
  const EncodeArgs ea{k->snap, k->meta, k->records, k->offsets, *out, n};
  hipLaunchKernelGGL(k_frames_encode, dim3(n), dim3(64), 0, stream, ea);
  HIPCHK(hipGetLastError());
  return 0;
}

} // namespace

void oakgpu_corpus_drop_caches(oakgpu_corpus *k) {
  cache_free(k);
  if (k->eval && k->eval_free) k->eval_free(k->eval);
  k->eval = nullptr;
}

extern "C" {

int oakgpu_corpus_create(oakgpu_ctx *c, const uint8_t *buffer, size_t size, oakgpu_corpus **out) {
  if (!c || !out || (!buffer && size)) return oakgpu_fail_msg("oakgpu_corpus_create: null argument");
  *out = nullptr;
  uint32_t n = 0;
  size_t stop = 0;
  if (int rc = oakgpu_replay_index(buffer, size, nullptr, nullptr, nullptr, 0, &n, &stop)) return rc;
  std::vector<uint64_t> offs(std::max(n, 1u));
  std::vector<uint16_t> fr(std::max(n, 1u));
  std::vector<uint8_t> mal(std::max(n, 1u));
  if (n) if (int rc = oakgpu_replay_index(buffer, stop, offs.data(), fr.data(), mal.data(), n, &n, nullptr)) return rc;
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  oakgpu_corpus *k = new oakgpu_corpus;
  k->ctx = c;
  k->n = n;
  k->info.records = n;
  k->info.stopped_at = stop;
  for (uint32_t i = 0; i < n; ++i) {
    if (mal[i]) ++k->info.malformed;
    else k->info.frames += fr[i];
  }
  k->h_frames.assign(fr.begin(), fr.begin() + n);
  k->h_malformed.assign(mal.begin(), mal.begin() + n);
  uint32_t *scratch = nullptr;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  int rc = 0;
  if (dev_alloc(k->records, stop) || dev_alloc(k->offsets, n) || dev_alloc(k->frames, n) || dev_alloc(k->malformed, n) || dev_alloc(k->aligned, (size_t)n * 384) ||
      dev_alloc(k->first, n) || dev_alloc(scratch, (size_t)n * 2) || dev_alloc(k->heads, oak::walk::QUEUE_HEADS * oak::walk::QUEUE_HEAD_STRIDE))
    rc = -1;
  int cus = 0;
  if (!rc) {
    const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, oakgpu_ctx_device(c));
    if (e != hipSuccess || cus <= 0) rc = oakgpu_fail_hip((int)e, "oakgpu_corpus_create: hipDeviceGetAttribute");
  }
  k->resident_waves = oak::walk::resident_walk_waves(cus);
  auto up = [&](void *dst, const void *src, size_t bytes) {
    if (rc || !bytes) return;
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) rc = oakgpu_fail_hip((int)e, "oakgpu_corpus_create: upload");
  };
  up(k->records, buffer, stop);
  up(k->offsets, offs.data(), (size_t)n * 8);
  up(k->frames, fr.data(), (size_t)n * 2);
  up(k->malformed, mal.data(), n);
  if (!rc) rc = oakgpu_replay_gather_dev(c, k->records, k->offsets, k->malformed, n, k->aligned, k->first, scratch);
  const hipError_t e = hipStreamSynchronize(stream); // (the uploads read pageable host memory that dies with this call)
  if (!rc && e != hipSuccess) rc = oakgpu_fail_hip((int)e, "oakgpu_corpus_create: hipStreamSynchronize");
  if (scratch) (void)hipFree(scratch);
  if (rc) { corpus_free(k); return rc; }
  *out = k;
  return 0;
}

void oakgpu_corpus_destroy(oakgpu_corpus *k) {
  if (!k) return;
  (void)oakgpu_ctx_enter(k->ctx);
  (void)hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(k->ctx));
  corpus_free(k);
}

int oakgpu_corpus_info(const oakgpu_corpus *k, oakgpu_corpus_stats *info) {
  if (!k || !info) return oakgpu_fail_msg("oakgpu_corpus_info: null argument");
  *info = k->info;
  return 0;
}

int oakgpu_frames_encode_dev(oakgpu_ctx *c, oakgpu_corpus *k, const uint32_t *picks, uint32_t n, const oakgpu_encoded_frames *out) {
  if (!c || !k || k->ctx != c) return oakgpu_fail_msg("oakgpu_frames_encode_dev: the corpus does not belong to this context");
  if (n == 0) return 0;
  if (!picks || ((uintptr_t)picks & 7)) return oakgpu_fail_msg("oakgpu_frames_encode_dev: picks must be an 8-byte aligned device array");
  if (int rc = check_out(out, "oakgpu_frames_encode_dev")) return rc;
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  if (int rc = corpus_reserve(k, n)) return rc;
  return encode_picks(c, k, picks, n, out);
}

int oakgpu_frames_sample_dev(oakgpu_ctx *c, oakgpu_corpus *k, uint32_t n, uint64_t seed, uint32_t max_battle_length, uint32_t min_iterations,
                             uint32_t *picks_out, const oakgpu_encoded_frames *out) {
  using namespace oak::tf;
  if (!c || !k || k->ctx != c) return oakgpu_fail_msg("oakgpu_frames_sample_dev: the corpus does not belong to this context");
  if (picks_out && ((uintptr_t)picks_out & 7)) return oakgpu_fail_msg("oakgpu_frames_sample_dev: picks_out must be 8-byte aligned");
  if (int rc = check_out(out, "oakgpu_frames_sample_dev")) return rc;
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  const oakgpu_corpus::Eligible *el = nullptr;
  for (const auto &e : k->eligibles) if (e.min_iterations == min_iterations && e.max_battle_length == max_battle_length) el = &e;
  if (!el) {
    if (k->eligibles.size() >= oakgpu_corpus::MAX_CACHED) { // a caller that sweeps its filters: start over instead of growing
      HIPCHK(hipStreamSynchronize(stream));                // (an earlier draw may still read a list)
      cache_free(k);
    }
    if (k->window) {
      if (int rc = window_eligible(k, stream, min_iterations, max_battle_length)) return rc;
      el = &k->eligibles.back();
    }
  }
  if (!el) {
    // an entry joins the corpus only once it is filled: a failure below leaves nothing behind that a later call would trust
    const oakgpu_corpus::Valid *va = nullptr;
    for (const auto &v : k->valids) if (v.min_iterations == min_iterations) va = &v;
    if (!va) {
      oakgpu_corpus::Valid v{min_iterations, nullptr, std::vector<uint32_t>(k->n)};
      if (dev_alloc(v.d, k->n)) return -1;
      if (k->n) {
        hipLaunchKernelGGL(k_frames_valid, dim3((k->n + 255) / 256), dim3(256), 0, stream, k->records, k->offsets, k->frames, k->malformed, k->n, min_iterations, v.d);
        hipError_t err = hipGetLastError();
        if (err == hipSuccess) err = hipMemcpyAsync(v.h.data(), v.d, (size_t)k->n * 4, hipMemcpyDeviceToHost, stream);
        const hipError_t done = hipStreamSynchronize(stream); // (always: the kernel may be running on v.d)
        if (err == hipSuccess) err = done;
        if (err != hipSuccess) {
          (void)hipFree(v.d);
          return oakgpu_fail_hip((int)err, "oakgpu_frames_sample_dev: k_frames_valid");
        }
      }
      k->valids.push_back(std::move(v));
      va = &k->valids.back();
    }
    std::vector<uint32_t> list;
    for (uint32_t r = 0; r < k->n; ++r)
      if (!k->h_malformed[r] && va->h[r] != 0 && (max_battle_length == 0 || k->h_frames[r] <= max_battle_length)) list.push_back(r);
    oakgpu_corpus::Eligible e{min_iterations, max_battle_length, (uint32_t)list.size(), nullptr, va->d};
    if (dev_alloc(e.d, list.size())) return -1;
    if (!list.empty()) {
      hipError_t err = hipMemcpyAsync(e.d, list.data(), list.size() * 4, hipMemcpyHostToDevice, stream);
      const hipError_t done = hipStreamSynchronize(stream); // (`list` is pageable host memory that dies with this call)
      if (err == hipSuccess) err = done;
      if (err != hipSuccess) {
        (void)hipFree(e.d);
        return oakgpu_fail_hip((int)err, "oakgpu_frames_sample_dev: eligible list");
      }
    }
    k->eligibles.push_back(e);
    el = &k->eligibles.back();
  }
  if (el->count == 0) return oakgpu_fail_msg("oakgpu_frames_sample_dev: no eligible record (none within max_battle_length with a frame of min_iterations)");
  if (n == 0) return 0;
  if (int rc = corpus_reserve(k, n)) return rc;
  uint32_t *picks = picks_out ? picks_out : k->picks;
  hipLaunchKernelGGL(k_frames_draw, dim3((n + 255) / 256), dim3(256), 0, stream, k->records, k->offsets, el->valid, el->d, el->count, min_iterations, seed, n, picks);
  return encode_picks(c, k, picks, n, out);
}

int oakgpu_encode_battles_dev(oakgpu_ctx *c, const uint8_t *battles, const uint8_t *durations, const uint8_t *results, uint32_t n, float *pokemon, float *active,
                              float *hp, int64_t *choice_indices, uint8_t *kk) {
  using namespace oak::tf;
  if (!c) return oakgpu_fail_msg("null ctx");
  if (n == 0) return 0;
  if (!battles || !durations || !results || !pokemon || !active || !hp || !choice_indices || !kk) return oakgpu_fail_msg("oakgpu_encode_battles_dev: null pointer");
  if (((uintptr_t)battles & 15) || ((uintptr_t)durations & 7) || ((uintptr_t)pokemon & 15) || ((uintptr_t)active & 7) || ((uintptr_t)hp & 3) || ((uintptr_t)choice_indices & 7))
    return oakgpu_fail_msg("oakgpu_encode_battles_dev: misaligned array (battles, pokemon: 16 bytes; durations, active, choice_indices: 8; hp: 4)");
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  uint32_t *meta = (uint32_t *)oakgpu_ctx_workspace(c, 2, (size_t)n * META_WORDS * 4);
  if (!meta) return -1;
  hipLaunchKernelGGL(k_frames_requests, dim3((n + 63) / 64), dim3(64), 0, stream, battles, durations, results, n, meta);
  oakgpu_encoded_frames o{};
  o.pokemon = pokemon; o.active = active; o.hp = hp; o.choice_indices = choice_indices; o.k = kk;
  const EncodeArgs ea{battles, meta, nullptr, nullptr, o, n};
  hipLaunchKernelGGL(k_frames_encode, dim3(n), dim3(64), 0, stream, ea);
  HIPCHK(hipGetLastError());
  return 0;
}

// host arrays: the 14 tensors staged in the context's grow-only cache, the device call, the copies back
static int frames_host(oakgpu_ctx *c, oakgpu_corpus *k, const uint32_t *picks_in, uint32_t *picks_out, uint32_t n, bool sample, uint64_t seed,
                       uint32_t max_battle_length, uint32_t min_iterations, const oakgpu_encoded_frames *out, uint32_t *ok_rows) {
  if (!c || !k) return oakgpu_fail_msg("oakgpu_frames_encode / _sample: null argument");
  if (!out) return oakgpu_fail_msg("oakgpu_frames_encode / _sample: null tensors");
  if (ok_rows) *ok_rows = 0;
  if (int rc = oakgpu_ctx_enter(c)) return rc;
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(c);
  OakHostCall hc(c);
  void *const *host = (void *const *)out;
  oakgpu_encoded_frames dev{};
  void **devp = (void **)&dev;
  for (int t = 0; t < 14; ++t) {
    if (!host[t]) return oakgpu_fail_msg("oakgpu_frames_encode / _sample: null tensor pointer");
    if (!(devp[t] = hc.get(std::max<size_t>(ROW_BYTES[t] * n, 16)))) return -1;
  }
  uint32_t *d_picks = (uint32_t *)hc.get(std::max<size_t>((size_t)n * 8, 16)), *d_count = (uint32_t *)hc.get(16);
  if (!d_picks || !d_count) return -1;
  HIPCHK(hipMemsetAsync(d_count, 0, 4, stream));
  if (sample) {
    if (int rc = oakgpu_frames_sample_dev(c, k, n, seed, max_battle_length, min_iterations, d_picks, &dev)) return rc;
  } else {
    if (n && !picks_in) return oakgpu_fail_msg("oakgpu_frames_encode: null picks");
    if (n) HIPCHK(hipMemcpyAsync(d_picks, picks_in, (size_t)n * 8, hipMemcpyHostToDevice, stream));
    if (int rc = oakgpu_frames_encode_dev(c, k, d_picks, n, &dev)) return rc;
  }
  if (n) {
    hipLaunchKernelGGL(oak::tf::k_frames_count_ok, dim3((n + 255) / 256), dim3(256), 0, stream, dev.status, n, d_count);
    HIPCHK(hipGetLastError());
    for (int t = 0; t < 14; ++t) HIPCHK(hipMemcpyAsync(host[t], devp[t], ROW_BYTES[t] * n, hipMemcpyDeviceToHost, stream));
    if (picks_out) HIPCHK(hipMemcpyAsync(picks_out, d_picks, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    if (ok_rows) HIPCHK(hipMemcpyAsync(ok_rows, d_count, 4, hipMemcpyDeviceToHost, stream));
  }
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_frames_encode(oakgpu_ctx *c, oakgpu_corpus *k, const uint32_t *picks, uint32_t n, const oakgpu_encoded_frames *out, uint32_t *ok_rows) {
  return frames_host(c, k, picks, nullptr, n, false, 0, 0, 0, out, ok_rows);
}

int oakgpu_frames_sample(oakgpu_ctx *c, oakgpu_corpus *k, uint32_t n, uint64_t seed, uint32_t max_battle_length, uint32_t min_iterations, uint32_t *picks_out,
                         const oakgpu_encoded_frames *out, uint32_t *ok_rows) {
  return frames_host(c, k, nullptr, picks_out, n, true, seed, max_battle_length, min_iterations, out, ok_rows);
}

} // extern "C"
