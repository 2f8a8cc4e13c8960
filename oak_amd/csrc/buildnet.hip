// oak_amd/csrc/buildnet.hip -- the team-building network on the device: TeamBuilding::Provider::get_trajectory
// (cpp/include/util/team-building.h:190-241) with rollout_build_network (:36-84), and the CompressedTrajectory NoTeam records of
// `.build.data` (encode/build/compressed-trajectory.h:23-105).  The contract is in include/oakgpu.h.
//
// k_build_rollout: one wave per team, one launch for the whole rollout of every team.  The team, the bitmask of the input x, the three
// activation vectors, the legal list with its logits and policy live in LDS (7 KiB).  Lane 0 runs what the reference runs sequentially
// and what must stay in its order -- the provider's prelude, the double sum of the softmax, the pick's walk, the applied action; all 64
// lanes build the legal list (a ballot per 64 candidates keeps the reference's order) and run the layers:
//   layer 1  a1 = b1 + sum of W1's columns at the ones of x, kept as a running pre-activation: a cell that becomes 1 adds its column once
//            (W1 is stored transposed, a column is `hidden` contiguous floats).  Order: the initial team's cells in slot order, then the
//            updates in step order.
//   layer 2  lane j owns outputs j, j + 64, ...: b2[j] then k ascending, fmaf (W2 stored transposed: coalesced over j).
//   layer 3  only at the legal cells, four entries of the list a pass: 16 lanes share row c of W3, each sums its k (4 sub .. 4 sub + 3, then
//            every 64 further on; fmaf, ascending), the 16 partial sums meet in a butterfly of four steps, b3[c] is added last.
// No atomics, no dependence on the grid: a row's bits depend on its team and seed alone.
#include <cmath>
#include <cstring>
#include <string>

#include "oakgpu_internal.h"
#include "selfplay_pick.hpp"

struct oakgpu_build_net {
  oakgpu_ctx *ctx = nullptr;
  uint32_t hidden = 0, value_hidden = 0;
  float *block = nullptr; // one allocation: w1t [n_dim][h], b1 [h], w2t [h][h] (in-major), b2 [h], w3 [n_dim][h], b3 [n_dim]
  float *w1t = nullptr, *b1 = nullptr, *w2t = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
};

namespace {
#define RC(x) do { int _r = (x); if (_r) return _r; } while (0)

namespace host_tab {
#define OAK_BUILD_TABLE static const
#include "build_tables.inc"
#undef OAK_BUILD_TABLE
} // namespace host_tab
namespace dev_tab {
#define OAK_BUILD_TABLE static __device__ const
#include "build_tables.inc"
#undef OAK_BUILD_TABLE
} // namespace dev_tab

constexpr uint32_t N_DIM = OAK_BUILD_N_DIM, MAX_ACTIONS = OAK_BUILD_MAX_ACTIONS, N_LEGAL = OAK_BUILD_N_LEGAL, NO_CELL = OAK_BUILD_NO_CELL;
constexpr uint32_t STEPS = OAKGPU_BUILD_MAX_STEPS, MAX_HIDDEN = 256, WAVE = 64, X_WORDS = (N_DIM + 31) / 32;
static_assert(N_DIM == OAKGPU_BUILD_N_DIM && MAX_ACTIONS == OAKGPU_BUILD_MAX_ACTIONS, "include/oakgpu.h and build_tables.inc disagree");
constexpr uint8_t INVALID_ROW = 255; // n_updates of a row whose team does not pass oakgpu_build_teams_check

// species_move_table[s][m]: NO_CELL when s is not legal or m is not in its pool.  One text for the host checks and the kernels.
#define OAK_BUILD_CELL_OF(T)                                                     \
  inline uint32_t cell_of(uint32_t s, uint32_t m) {                              \
    if (s == 0 || s >= 152 || T::CELL_BASE[s] == NO_CELL) return NO_CELL;        \
    const uint32_t base = T::CELL_BASE[s];                                       \
    if (m == 0) return base;                                                     \
    for (uint32_t p = 0; p < T::POOL_SIZE[s]; ++p)                               \
      if (T::CELL_MOVE[base + 1 + p] == m) return base + 1 + p;                  \
    return NO_CELL;                                                              \
  }
namespace host_tab { OAK_BUILD_CELL_OF(host_tab) }
namespace dev_tab { __device__ OAK_BUILD_CELL_OF(dev_tab) }

struct BuildArgs {
  const float *w1t, *b1, *w2t, *b2, *w3, *b3;
  uint32_t hidden, n;
  const uint8_t *teams, *sizes; // rollout: the teams and their sizes (nullable: 6); provide: the pool (pool_n teams)
  const uint64_t *seeds;
  int input_update, provide;
  uint32_t pool_n, max_pokemon;
  double pokemon_delete_prob, move_delete_prob, team_modify_prob;
  uint8_t *teams_init, *sizes_out; // provide only
  int32_t *team_index;            // provide only
  uint8_t *teams_out, *n_updates;
  uint16_t *action, *index, *n_legal;
  float *prob;
  int16_t *trace_legal; // nullable, with the two below
  float *trace_logits, *trace_policy;
};

// The whole wave (all 64 lanes, in uniform control flow): the legal list of the current team into s_cell, in the reference's order -- lane
// l looks at candidate base + l, a ballot keeps the order, the lanes below a lane in the mask give its position.  Returns the list's length,
// the same in every lane.
__device__ uint32_t legal_additions(const uint8_t *team, uint32_t size, uint16_t *s_cell, uint32_t lane) {
  uint32_t count = 0;
  const uint64_t below = (1ull << lane) - 1;
  bool gap = false;
  for (uint32_t i = 0; i < size; ++i) gap = gap || team[5 * i] == 0;
  if (gap)
    for (uint32_t first = 0; first < N_LEGAL; first += WAVE) {
      const uint32_t q = first + lane;
      const uint32_t s = q < N_LEGAL ? dev_tab::LEGAL_SPECIES[q] : 0;
      bool free = q < N_LEGAL;
      for (uint32_t i = 0; i < size; ++i) free = free && team[5 * i] != s;
      const uint64_t mask = __ballot(free);
      const uint32_t at = count + __popcll(mask & below);
      if (free && at < MAX_ACTIONS) s_cell[at] = dev_tab::CELL_BASE[s];
      count += __popcll(mask);
    }
  for (uint32_t i = 0; i < size; ++i) {
    const uint32_t s = team[5 * i];
    const uint32_t m0 = team[5 * i + 1], m1 = team[5 * i + 2], m2 = team[5 * i + 3], m3 = team[5 * i + 4];
    if (s == 0 || (m0 && m1 && m2 && m3)) continue;
    const uint32_t base = dev_tab::CELL_BASE[s], pool = dev_tab::POOL_SIZE[s];
    for (uint32_t first = 0; first < pool; first += WAVE) {
      const uint32_t p = first + lane;
      const uint32_t m = p < pool ? dev_tab::CELL_MOVE[base + 1 + p] : 0;
      const bool free = p < pool && m != m0 && m != m1 && m != m2 && m != m3;
      const uint64_t mask = __ballot(free);
      const uint32_t at = count + __popcll(mask & below);
      if (free && at < MAX_ACTIONS) s_cell[at] = (uint16_t)(base + 1 + p);
      count += __popcll(mask);
    }
  }
  return count < MAX_ACTIONS ? count : MAX_ACTIONS;
}

// lane 0: Omitter::delete_info on the first `size` slots
__device__ bool delete_info(uint8_t *team, uint32_t size, uint64_t &rng, double pokemon_delete_prob, double move_delete_prob) {
  bool modified = false;
  for (uint32_t i = 0; i < size; ++i) {
    if (team[5 * i] != 0 && oak_pick::uniform01(rng) < pokemon_delete_prob) {
      for (int b = 0; b < 5; ++b) team[5 * i + b] = 0;
      modified = true;
    } else {
      for (int j = 1; j < 5; ++j)
        if (team[5 * i + j] != 0 && oak_pick::uniform01(rng) < move_delete_prob) {
          team[5 * i + j] = 0;
          modified = true;
        }
    }
  }
  return modified;
}

enum { CTL_SIZE = 0, CTL_STOP = 1, CTL_PENDING = 2, CTL_WORDS = 4 };

__global__ __launch_bounds__(WAVE) void k_build_rollout(const BuildArgs a) {
  __shared__ uint8_t s_team[32];
  __shared__ uint32_t s_x[X_WORDS];
  __shared__ float s_a1[MAX_HIDDEN], s_h1[MAX_HIDDEN], s_h2[MAX_HIDDEN];
  __shared__ uint16_t s_cell[MAX_ACTIONS + 1];
  __shared__ uint16_t s_pending[32];
  __shared__ float s_logit[MAX_ACTIONS + 1], s_policy[MAX_ACTIONS + 1];
  __shared__ double s_sum;
  __shared__ uint32_t s_ctl[CTL_WORDS];
  const uint32_t g = blockIdx.x, tid = threadIdx.x, h = a.hidden;
  if (g >= a.n) return;
  uint64_t rng = 0;       // lane 0's own
  uint32_t steps = 0;     // lane 0's own
  uint32_t size = 6;      // lane 0's until the barrier below, then every lane's
  bool swapped = false;   // the same in every lane: the lead swaps have been listed

  for (uint32_t w = tid; w < X_WORDS; w += WAVE) s_x[w] = 0;
  if (tid == 0) {
    rng = a.seeds[g];
    bool stop = false;
    if (a.provide) { // Provider::get_trajectory up to the rollout
      const uint32_t pick = (uint32_t)(oak_pick::splitmix64(rng) % a.pool_n);
      uint32_t count = 0;
      for (int b = 0; b < 30; ++b) s_team[b] = a.teams[(size_t)pick * 30 + b];
      for (int i = 0; i < 6; ++i) count += s_team[5 * i] != 0;
      size = count < a.max_pokemon ? count : a.max_pokemon;
      bool changed = size < count;
      for (uint32_t b = 5 * size; b < 30; ++b) s_team[b] = 0;
      if (oak_pick::uniform01(rng) < a.team_modify_prob && !changed) changed = delete_info(s_team, size, rng, a.pokemon_delete_prob, a.move_delete_prob);
      for (int b = 0; b < 30; ++b) a.teams_init[(size_t)g * 30 + b] = s_team[b];
      a.sizes_out[g] = (uint8_t)size;
      a.team_index[g] = changed ? -1 : (int32_t)pick;
      stop = !changed;
    } else {
      size = a.sizes ? a.sizes[g] : 6;
      if (size > 6) size = 6;
      for (uint32_t b = 0; b < 30; ++b) s_team[b] = b < 5 * size ? a.teams[(size_t)g * 30 + b] : 0;
    }
    // Tensorizer::write: the cells of the team, in slot order, each once
    uint32_t pending = 0;
    bool valid = true;
    for (uint32_t i = 0; i < size && !stop; ++i) {
      const uint32_t s = s_team[5 * i];
      for (uint32_t j = 0; j < 5; ++j) {
        const uint32_t m = j ? s_team[5 * i + j] : 0;
        if (s == 0) { valid = valid && m == 0; continue; }
        if (j && m == 0) continue;
        const uint32_t c = dev_tab::cell_of(s, m);
        if (c == NO_CELL) { valid = false; continue; }
        if (!(s_x[c >> 5] >> (c & 31) & 1)) {
          s_x[c >> 5] |= 1u << (c & 31);
          if (pending < 30) s_pending[pending++] = (uint16_t)c;
        } else if (j == 0) valid = false; // the species is on the team twice
      }
    }
    if (!valid) { // refused by oakgpu_build_teams_check: the row is marked and left
      a.n_updates[g] = INVALID_ROW;
      for (int b = 0; b < 30; ++b) a.teams_out[(size_t)g * 30 + b] = 0;
      stop = true;
    } else if (stop) {
      a.n_updates[g] = 0;
      for (int b = 0; b < 30; ++b) a.teams_out[(size_t)g * 30 + b] = s_team[b];
    }
    s_ctl[CTL_STOP] = stop;
    s_ctl[CTL_PENDING] = pending;
    s_ctl[CTL_SIZE] = size;
  }
  __syncthreads();
  if (s_ctl[CTL_STOP]) return;
  size = s_ctl[CTL_SIZE];
  for (uint32_t j = tid; j < h; j += WAVE) s_a1[j] = a.b1[j];

  for (uint32_t step = 0; step <= STEPS; ++step) {
    // layer 1: the columns of the cells that became 1 (lane j's own entries of a1: no barrier between the columns)
    const uint32_t pending = s_ctl[CTL_PENDING];
    for (uint32_t q = 0; q < pending; ++q) {
      const float *col = a.w1t + (size_t)s_pending[q] * h;
      for (uint32_t j = tid; j < h; j += WAVE) s_a1[j] += col[j];
    }
    for (uint32_t j = tid; j < h; j += WAVE) s_h1[j] = fmaxf(s_a1[j], 0.f);
    __syncthreads();
    // the legal list, by the whole wave: the additions, and once they are used up the lead swaps (after which nothing is listed)
    uint32_t count = 0;
    bool swap = false;
    if (!swapped && step < STEPS) {
      count = legal_additions(s_team, size, s_cell, tid);
      if (count == 0) {
        swapped = swap = true;
        for (uint32_t i = 1; i < size; ++i)
          if (s_team[5 * i]) {
            if (tid == 0) s_cell[count] = dev_tab::CELL_BASE[s_team[5 * i]];
            ++count;
          }
      }
    }
    __syncthreads();
    if (count == 0) break;
    // layer 2
    for (uint32_t j = tid; j < h; j += WAVE) {
      float acc = a.b2[j];
      for (uint32_t k = 0; k < h; ++k) acc = fmaf(a.w2t[(size_t)k * h + j], s_h1[k], acc);
      s_h2[j] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    // layer 3 at the legal cells, and expf of each logit
    // 16 lanes share a row of W3 (four cells a pass), so a pass reads four contiguous rows, not 64 scattered cache lines
    for (uint32_t first = 0; first < count; first += 4) {
      const uint32_t sub = tid & 15, i = first + (tid >> 4);
      const bool live = i < count;
      const uint32_t c = s_cell[live ? i : first];
      const float *row = a.w3 + (size_t)c * h;
      float acc = 0.f;
      if ((h & 3) == 0) { // rows are 16-byte aligned
        for (uint32_t k = 4 * sub; k < h; k += 64) {
          const float4 w = *reinterpret_cast<const float4 *>(row + k);
          acc = fmaf(w.x, s_h2[k], acc);
          acc = fmaf(w.y, s_h2[k + 1], acc);
          acc = fmaf(w.z, s_h2[k + 2], acc);
          acc = fmaf(w.w, s_h2[k + 3], acc);
        }
      } else {
        for (uint32_t k = sub; k < h; k += 16) acc = fmaf(row[k], s_h2[k], acc);
      }
      for (int m = 1; m < 16; m <<= 1) acc += __shfl_xor(acc, m); // both partners add the same two numbers: the 16 lanes agree
      if (live && sub == 0) {
        const float logit = acc + a.b3[c];
        s_logit[i] = logit;
        s_policy[i] = expf(logit);
      }
    }
    __syncthreads();
    if (tid == 0) { // std::accumulate(..., 0.0): in double, in list order
      double sum = 0.0;
      for (uint32_t i = 0; i < count; ++i) sum += (double)s_policy[i];
      s_sum = sum;
    }
    __syncthreads();
    {
      const double sum = s_sum;
      const size_t at = ((size_t)g * STEPS + step) * MAX_ACTIONS;
      for (uint32_t i = tid; i < count; i += WAVE) {
        const float p = (float)((double)s_policy[i] / sum);
        s_policy[i] = p;
        if (a.trace_legal) {
          a.trace_legal[at + i] = (int16_t)s_cell[i];
          a.trace_logits[at + i] = s_logit[i];
          a.trace_policy[at + i] = p;
        }
      }
    }
    __syncthreads();
    if (tid == 0) { // device.sample_pdf, apply_basic_action, input[index] = 1
      double p = oak_pick::uniform01(rng);
      uint32_t index = 0;
      for (uint32_t i = 0; i < count; ++i) {
        p -= (double)s_policy[i];
        if (p <= 0) { index = i; break; }
      }
      const uint32_t c = s_cell[index], species = dev_tab::CELL_SPECIES[c], move = dev_tab::CELL_MOVE[c];
      if (swap) { // a lead swap: slot 0 <-> the slot that holds the species
        for (uint32_t i = 1; i < size; ++i)
          if (s_team[5 * i] == species) {
            for (int b = 0; b < 5; ++b) { const uint8_t t = s_team[b]; s_team[b] = s_team[5 * i + b]; s_team[5 * i + b] = t; }
            break;
          }
      } else if (move == 0) { // the species goes to the first empty slot
        for (uint32_t i = 0; i < size; ++i)
          if (s_team[5 * i] == 0) { s_team[5 * i] = (uint8_t)species; break; }
      } else { // the move goes to the first empty move slot of the set that holds the species
        for (uint32_t i = 0; i < size; ++i)
          if (s_team[5 * i] == species) {
            for (int j = 1; j < 5; ++j)
              if (s_team[5 * i + j] == 0) { s_team[5 * i + j] = (uint8_t)move; break; }
            break;
          }
      }
      const size_t at = (size_t)g * STEPS + step;
      a.action[at] = (uint16_t)c;
      a.index[at] = (uint16_t)index;
      a.n_legal[at] = (uint16_t)count;
      a.prob[at] = s_policy[index];
      ++steps;
      const uint32_t xc = a.input_update ? c : index; // the reference sets x at the POSITION in the list (team-building.h:67)
      uint32_t pending = 0;
      if (!(s_x[xc >> 5] >> (xc & 31) & 1)) {
        s_x[xc >> 5] |= 1u << (xc & 31);
        s_pending[pending++] = (uint16_t)xc;
      }
      s_ctl[CTL_PENDING] = pending;
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.n_updates[g] = (uint8_t)steps;
    for (int b = 0; b < 30; ++b) a.teams_out[(size_t)g * 30 + b] = s_team[b];
  }
}

// ---- records: one block walks the rows in order, so the built rows' records are packed in row order
struct RecordArgs {
  const uint8_t *teams, *sizes, *n_updates;
  const uint16_t *action;
  const float *prob, *value, *score;
  uint32_t n;
  uint8_t *records;
  uint32_t *count;
};
constexpr uint32_t RECORD_BLOCK = 256, RECORD_BYTES = OAKGPU_BUILD_RECORD_BYTES;

// one record (include/oakgpu.h, RECORDS) of a row's k updates, for both record kernels: team = the row's initial 30 bytes, action / prob =
// the row's step arrays
__device__ __forceinline__ void write_record(uint32_t *out, const uint8_t *team, uint32_t size, uint32_t k, const uint16_t *action, const float *prob, float value,
                                             float score) {
#pragma clang fp contract(off)
  const uint32_t score8 = (score >= 0.f) ? (uint32_t)(uint8_t)(2.f * score) : 255u; // NaN or negative: no score
  out[0] = 0u | score8 << 8 | (uint32_t)(uint16_t)(value * 65535.f) << 16;
  uint32_t at = 0;
  for (uint32_t i = 0; i < size; ++i) { // the initial team: per slot the species cell, then its held moves
    const uint32_t s = team[5 * i];
    if (s == 0) continue;
    for (uint32_t j = 0; j < 5; ++j) {
      const uint32_t m = j ? team[5 * i + j] : 0;
      if (j && m == 0) continue;
      const uint32_t c = dev_tab::cell_of(s, m);
      if (at < STEPS) out[1 + at++] = c & 0xFFFF;
    }
  }
  for (uint32_t u = 0; u < k && at < STEPS; ++u) {
    const float p = prob[u];
    uint32_t q = (uint16_t)(65535.f * p);
    if (p != 0.f && q == 0) q = 1;
    out[1 + at++] = (uint32_t)action[u] | q << 16;
  }
  for (; at < STEPS; ++at) out[1 + at] = 0;
}

__global__ __launch_bounds__(RECORD_BLOCK) void k_build_records(const RecordArgs a) {
  __shared__ uint32_t s_scan[RECORD_BLOCK];
  __shared__ uint32_t s_base;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (uint32_t first = 0; first < a.n; first += RECORD_BLOCK) {
    const uint32_t g = first + tid;
    const uint32_t k = g < a.n ? a.n_updates[g] : 0;
    const bool built = k > 0 && k <= STEPS;
    s_scan[tid] = built;
    __syncthreads();
    for (uint32_t d = 1; d < RECORD_BLOCK; d <<= 1) { // inclusive scan
      const uint32_t v = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    const uint32_t base = s_base;
    if (built) {
      uint32_t *out = (uint32_t *)(a.records + (size_t)(base + s_scan[tid] - 1) * RECORD_BYTES);
      const uint32_t size = a.sizes ? (a.sizes[g] > 6 ? 6u : a.sizes[g]) : 6u;
      write_record(out, a.teams + (size_t)g * 30, size, k, a.action + (size_t)g * STEPS, a.prob + (size_t)g * STEPS, a.value[g], a.score[g]);
    }
    __syncthreads();
    if (tid == RECORD_BLOCK - 1) s_base = base + s_scan[tid];
    __syncthreads();
  }
  if (tid == 0) *a.count = s_base;
}

// ---- both seats' records of a batch of games (generate.cc:361-383): a game with status OK or SKIPPED gives one record per built seat, p1's
// before p2's, games in order.  The value / score rule is one text for this kernel and oakgpu_build_game_targets_host.
__host__ __device__ inline bool game_targets(uint32_t status, uint32_t result, double matchup, int seat, float *value, float *score) {
#pragma clang fp contract(off)
  if (status != OAKGPU_FSP_OK && status != OAKGPU_FSP_SKIPPED) return false; // dropped or stopped: the reference's catch ... continue
  *value = seat == 0 ? (float)matchup : (float)(1.0 - matchup);
  if (status == OAKGPU_FSP_SKIPPED) { *score = -1.f; return true; } // no battle: no score
  const uint32_t type = result & 15;
  const float s = type == 1 ? 1.f : type == 2 ? 0.f : 0.5f; // PKMN::score: win, lose, tie
  *score = seat == 0 ? s : 1.f - s;
  return true;
}

struct GameRecordArgs {
  oakgpu_build_seat_arrays seat[2];
  const uint8_t *status, *results;
  const double *matchup;
  uint32_t n;
  uint8_t *records;
  uint32_t *count;
};

__global__ __launch_bounds__(RECORD_BLOCK) void k_build_game_records(const GameRecordArgs a) {
  __shared__ uint32_t s_scan[RECORD_BLOCK];
  __shared__ uint32_t s_base;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (uint32_t first = 0; first < a.n; first += RECORD_BLOCK) {
    const uint32_t g = first + tid;
    uint32_t k[2] = {0, 0};
    float value[2] = {0.f, 0.f}, score[2] = {0.f, 0.f};
    if (g < a.n)
      for (int s = 0; s < 2; ++s) {
        const uint32_t updates = a.seat[s].n_updates[g];
        if (updates > 0 && updates <= STEPS && game_targets(a.status[g], a.results[g], a.matchup[g], s, &value[s], &score[s])) k[s] = updates;
      }
    const uint32_t own = (k[0] != 0) + (k[1] != 0);
    s_scan[tid] = own;
    __syncthreads();
    for (uint32_t d = 1; d < RECORD_BLOCK; d <<= 1) { // inclusive scan
      const uint32_t v = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    const uint32_t base = s_base;
    uint32_t at = base + s_scan[tid] - own;
    for (int s = 0; s < 2; ++s)
      if (k[s]) {
        const oakgpu_build_seat_arrays &p = a.seat[s];
        const uint32_t size = p.sizes ? (p.sizes[g] > 6 ? 6u : p.sizes[g]) : 6u;
        write_record((uint32_t *)(a.records + (size_t)at * RECORD_BYTES), p.teams_init + (size_t)g * 30, size, k[s], p.action + (size_t)g * STEPS,
                     p.prob + (size_t)g * STEPS, value[s], score[s]);
        ++at;
      }
    __syncthreads();
    if (tid == RECORD_BLOCK - 1) s_base = base + s_scan[tid];
    __syncthreads();
  }
  if (tid == 0) *a.count = s_base;
}

// ---- host: the file, the refusals
struct Layer { uint32_t in, out; const uint8_t *bias, *weight; };

const char *parse_net(const uint8_t *bytes, size_t len, Layer layers[6]) {
  if (!bytes) return "null bytes";
  size_t pos = 0;
  for (int k = 0; k < 6; ++k) {
    if (len - pos < 8) return "truncated file";
    uint32_t dims[2];
    memcpy(dims, bytes + pos, 8);
    const uint64_t body = 4ull * dims[1] + 4ull * dims[1] * dims[0];
    if (dims[0] == 0 || dims[1] == 0 || dims[0] > (1u << 20) || dims[1] > (1u << 20)) return "layer dimensions out of range";
    if (len - pos - 8 < body) return "truncated file";
    layers[k] = Layer{dims[0], dims[1], bytes + pos + 8, bytes + pos + 8 + 4ull * dims[1]};
    pos += 8 + body;
  }
  if (pos != len) return "trailing bytes";
  for (int net = 0; net < 2; ++net) {
    const Layer *l = layers + 3 * net;
    if (l[0].out != l[1].in || l[1].out != l[2].in) return "layer dimensions do not chain";
    if (l[0].in != N_DIM) return "a net does not start at n_dim";
  }
  if (layers[2].out != N_DIM) return "the policy net does not end at n_dim";
  if (layers[5].out != 1) return "the value net does not end at 1";
  if (layers[0].out != layers[1].out) return "the policy net's hidden widths differ";
  if (layers[0].out > MAX_HIDDEN) return "policy hidden width above 256";
  for (int k = 0; k < 6; ++k) {
    const size_t count = (size_t)layers[k].out * (layers[k].in + 1);
    for (size_t i = 0; i < count; ++i) {
      float v;
      memcpy(&v, layers[k].bias + 4 * i, 4);
      if (std::isnan(v)) return "NaN parameter";
    }
  }
  return nullptr;
}

int fail(const char *fn, const std::string &what) { return oakgpu_fail_msg((std::string(fn) + ": " + what).c_str()); }

const char *team_fault(const uint8_t *team, uint32_t size) {
  for (uint32_t i = 0; i < size; ++i) {
    const uint32_t s = team[5 * i];
    if (s == 0) {
      for (int j = 1; j < 5; ++j) if (team[5 * i + j]) return "a move outside its species' pool";
      continue;
    }
    if (host_tab::cell_of(s, 0) == NO_CELL) return "a species outside legal_species";
    for (uint32_t q = 0; q < i; ++q) if (team[5 * q] == s) return "a duplicate species";
    for (int j = 1; j < 5; ++j) if (team[5 * i + j] && host_tab::cell_of(s, team[5 * i + j]) == NO_CELL) return "a move outside its species' pool";
  }
  return nullptr;
}

int launch_rollout(oakgpu_ctx *ctx, const BuildArgs &a) {
  hipLaunchKernelGGL(k_build_rollout, dim3(a.n), dim3(WAVE), 0, (hipStream_t)oakgpu_ctx_stream(ctx), a);
  HIPCHK(hipGetLastError());
  return 0;
}

BuildArgs net_args(const oakgpu_build_net *net) {
  BuildArgs a{};
  a.w1t = net->w1t; a.b1 = net->b1; a.w2t = net->w2t; a.b2 = net->b2; a.w3 = net->w3; a.b3 = net->b3;
  a.hidden = net->hidden;
  return a;
}

} // namespace

extern "C" {

int oakgpu_build_tables(uint8_t *legal_species, uint8_t *cells, int32_t *table) {
  if (legal_species) memcpy(legal_species, host_tab::LEGAL_SPECIES, N_LEGAL);
  if (cells)
    for (uint32_t c = 0; c < N_DIM; ++c) { cells[2 * c] = host_tab::CELL_SPECIES[c]; cells[2 * c + 1] = host_tab::CELL_MOVE[c]; }
  if (table) {
    for (uint32_t i = 0; i < 152 * 166; ++i) table[i] = -1;
    for (uint32_t c = 0; c < N_DIM; ++c) table[host_tab::CELL_SPECIES[c] * 166 + host_tab::CELL_MOVE[c]] = (int32_t)c;
  }
  return 0;
}

int oakgpu_build_net_check(const uint8_t *bytes, size_t len) {
  Layer layers[6];
  const char *fault = parse_net(bytes, len, layers);
  return fault ? fail("oakgpu_build_net_check", fault) : 0;
}

int oakgpu_build_net_load(oakgpu_ctx *ctx, const uint8_t *bytes, size_t len, oakgpu_build_net **out) {
  if (!ctx || !out) return oakgpu_fail_msg("oakgpu_build_net_load: null argument");
  *out = nullptr;
  Layer layers[6];
  if (const char *fault = parse_net(bytes, len, layers)) return fail("oakgpu_build_net_load", fault);
  RC(oakgpu_ctx_enter(ctx));
  const uint32_t h = layers[0].out;
  const size_t count = (size_t)N_DIM * h + h + (size_t)h * h + h + (size_t)N_DIM * h + N_DIM;
  std::vector<float> host(count);
  float *w1t = host.data(), *b1 = w1t + (size_t)N_DIM * h, *w2t = b1 + h, *b2 = w2t + (size_t)h * h, *w3 = b2 + h, *b3 = w3 + (size_t)N_DIM * h;
  std::vector<float> w((size_t)N_DIM * h);
  memcpy(w.data(), layers[0].weight, w.size() * 4); // [h][n_dim] -> [n_dim][h]
  for (uint32_t j = 0; j < h; ++j)
    for (uint32_t c = 0; c < N_DIM; ++c) w1t[(size_t)c * h + j] = w[(size_t)j * N_DIM + c];
  memcpy(b1, layers[0].bias, 4 * h);
  memcpy(w.data(), layers[1].weight, (size_t)h * h * 4); // [out][in] -> [in][out]
  for (uint32_t j = 0; j < h; ++j)
    for (uint32_t k = 0; k < h; ++k) w2t[(size_t)k * h + j] = w[(size_t)j * h + k];
  memcpy(b2, layers[1].bias, 4 * h);
  memcpy(w3, layers[2].weight, (size_t)N_DIM * h * 4);
  memcpy(b3, layers[2].bias, 4 * N_DIM);
  oakgpu_build_net *net = new oakgpu_build_net;
  net->ctx = ctx;
  net->hidden = h;
  net->value_hidden = layers[3].out;
  if (int rc = dev_alloc(net->block, count)) { delete net; return rc; }
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  hipError_t e = hipMemcpyAsync(net->block, host.data(), count * 4, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { (void)hipFree(net->block); delete net; return oakgpu_fail_hip((int)e, "oakgpu_build_net_load: copy"); }
  net->w1t = net->block; net->b1 = net->w1t + (size_t)N_DIM * h; net->w2t = net->b1 + h; net->b2 = net->w2t + (size_t)h * h;
  net->w3 = net->b2 + h; net->b3 = net->w3 + (size_t)N_DIM * h;
  *out = net;
  return 0;
}

void oakgpu_build_net_destroy(oakgpu_build_net *net) {
  if (!net) return;
  if (net->ctx && oakgpu_ctx_enter(net->ctx) == 0) (void)hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(net->ctx));
  (void)hipFree(net->block);
  delete net;
}

int oakgpu_build_net_shape(const oakgpu_build_net *net, uint32_t *policy_hidden, uint32_t *value_hidden) {
  if (!net) return oakgpu_fail_msg("oakgpu_build_net_shape: null net");
  if (policy_hidden) *policy_hidden = net->hidden;
  if (value_hidden) *value_hidden = net->value_hidden;
  return 0;
}

int oakgpu_build_teams_check(const uint8_t *teams, const uint8_t *sizes, uint32_t n, int input_update) {
  const char *fn = "oakgpu_build_teams_check";
  if (n == 0) return fail(fn, "n == 0");
  if (input_update != 0 && input_update != 1) return fail(fn, "input_update outside {0, 1}");
  if (!teams) return fail(fn, "null teams");
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t size = sizes ? sizes[g] : 6;
    if (size > 6) return fail(fn, "team " + std::to_string(g) + ": size > 6");
    if (const char *fault = team_fault(teams + (size_t)g * 30, size)) return fail(fn, "team " + std::to_string(g) + ": " + fault);
  }
  return 0;
}

int oakgpu_build_provide_check(const uint8_t *pool, uint32_t pool_n, uint32_t n, int max_pokemon, double pokemon_delete_prob, double move_delete_prob,
                               double team_modify_prob) {
  const char *fn = "oakgpu_build_provide_check";
  if (n == 0) return fail(fn, "n == 0");
  if (pool_n == 0 || !pool) return fail(fn, "an empty pool");
  if (max_pokemon < 1 || max_pokemon > 6) return fail(fn, "max_pokemon outside 1..6");
  const double probs[3] = {pokemon_delete_prob, move_delete_prob, team_modify_prob};
  const char *names[3] = {"pokemon_delete_prob", "move_delete_prob", "team_modify_prob"};
  for (int k = 0; k < 3; ++k)
    if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return fail(fn, std::string(names[k]) + " outside [0, 1]");
  for (uint32_t t = 0; t < pool_n; ++t) {
    const uint8_t *team = pool + (size_t)t * 30;
    if (const char *fault = team_fault(team, 6)) return fail(fn, "pool team " + std::to_string(t) + ": " + fault);
    bool gap = false;
    for (int i = 0; i < 6; ++i) {
      if (team[5 * i] && gap) return fail(fn, "pool team " + std::to_string(t) + ": an empty slot before a Pokemon");
      gap = gap || !team[5 * i];
    }
    if (!team[0]) return fail(fn, "pool team " + std::to_string(t) + ": an empty team");
  }
  return 0;
}

int oakgpu_build_rollout_dev(oakgpu_ctx *ctx, const oakgpu_build_net *net, const uint8_t *teams, const uint8_t *sizes, const uint64_t *seeds, uint32_t n,
                             int input_update, const oakgpu_build_outputs *out) {
  const char *fn = "oakgpu_build_rollout_dev";
  if (!ctx || !net || !teams || !seeds || !out) return fail(fn, "null argument");
  if (n == 0) return fail(fn, "n == 0");
  if (input_update != 0 && input_update != 1) return fail(fn, "input_update outside {0, 1}");
  if (!out->teams_out || !out->n_updates || !out->action || !out->index || !out->n_legal || !out->prob) return fail(fn, "a required output is null");
  if ((out->trace_legal != nullptr) != (out->trace_logits != nullptr) || (out->trace_legal != nullptr) != (out->trace_policy != nullptr))
    return fail(fn, "the trace arrays come together or not at all");
  if (net->ctx != ctx) return fail(fn, "the net belongs to another context");
  RC(oakgpu_ctx_enter(ctx));
  BuildArgs a = net_args(net);
  a.n = n; a.teams = teams; a.sizes = sizes; a.seeds = seeds; a.input_update = input_update;
  a.teams_out = out->teams_out; a.n_updates = out->n_updates; a.action = out->action; a.index = out->index; a.n_legal = out->n_legal; a.prob = out->prob;
  a.trace_legal = out->trace_legal; a.trace_logits = out->trace_logits; a.trace_policy = out->trace_policy;
  return launch_rollout(ctx, a);
}

int oakgpu_build_provide_dev(oakgpu_ctx *ctx, const oakgpu_build_net *net, const uint8_t *pool, uint32_t pool_n, const uint64_t *seeds, uint32_t n,
                             const oakgpu_build_provider *prm, const oakgpu_build_outputs *out) {
  const char *fn = "oakgpu_build_provide_dev";
  if (!ctx || !net || !pool || !seeds || !prm || !out) return fail(fn, "null argument");
  if (n == 0) return fail(fn, "n == 0");
  if (pool_n == 0) return fail(fn, "an empty pool");
  if (prm->max_pokemon < 1 || prm->max_pokemon > 6) return fail(fn, "max_pokemon outside 1..6");
  if (prm->input_update != 0 && prm->input_update != 1) return fail(fn, "input_update outside {0, 1}");
  const double probs[3] = {prm->pokemon_delete_prob, prm->move_delete_prob, prm->team_modify_prob};
  for (double p : probs) if (!(p >= 0.0 && p <= 1.0)) return fail(fn, "a probability outside [0, 1]");
  if (!out->teams_out || !out->n_updates || !out->action || !out->index || !out->n_legal || !out->prob || !out->teams_init || !out->sizes_out || !out->team_index)
    return fail(fn, "a required output is null");
  if ((out->trace_legal != nullptr) != (out->trace_logits != nullptr) || (out->trace_legal != nullptr) != (out->trace_policy != nullptr))
    return fail(fn, "the trace arrays come together or not at all");
  if (net->ctx != ctx) return fail(fn, "the net belongs to another context");
  RC(oakgpu_ctx_enter(ctx));
  BuildArgs a = net_args(net);
  a.n = n; a.teams = pool; a.pool_n = pool_n; a.seeds = seeds; a.input_update = prm->input_update; a.provide = 1;
  a.max_pokemon = (uint32_t)prm->max_pokemon;
  a.pokemon_delete_prob = prm->pokemon_delete_prob; a.move_delete_prob = prm->move_delete_prob; a.team_modify_prob = prm->team_modify_prob;
  a.teams_init = out->teams_init; a.sizes_out = out->sizes_out; a.team_index = out->team_index;
  a.teams_out = out->teams_out; a.n_updates = out->n_updates; a.action = out->action; a.index = out->index; a.n_legal = out->n_legal; a.prob = out->prob;
  a.trace_legal = out->trace_legal; a.trace_logits = out->trace_logits; a.trace_policy = out->trace_policy;
  return launch_rollout(ctx, a);
}

int oakgpu_build_records_dev(oakgpu_ctx *ctx, const uint8_t *teams_init, const uint8_t *sizes, const uint8_t *n_updates, const uint16_t *action,
                             const float *prob, const float *value, const float *score, uint32_t n, uint8_t *records, uint32_t *count) {
  const char *fn = "oakgpu_build_records_dev";
  if (!ctx || !teams_init || !n_updates || !action || !prob || !value || !score || !records || !count) return fail(fn, "null argument");
  if (n == 0) return fail(fn, "n == 0");
  if ((uintptr_t)records & 3) return fail(fn, "records must be 4-byte aligned");
  RC(oakgpu_ctx_enter(ctx));
  const RecordArgs a{teams_init, sizes, n_updates, action, prob, value, score, n, records, count};
  hipLaunchKernelGGL(k_build_records, dim3(1), dim3(RECORD_BLOCK), 0, (hipStream_t)oakgpu_ctx_stream(ctx), a);
  HIPCHK(hipGetLastError());
  return 0;
}

int oakgpu_build_game_records_dev(oakgpu_ctx *ctx, const oakgpu_build_seat_arrays *p1, const oakgpu_build_seat_arrays *p2, const uint8_t *status,
                                  const uint8_t *results, const double *matchup, uint32_t n, uint8_t *records, uint32_t *count) {
  const char *fn = "oakgpu_build_game_records_dev";
  if (!ctx || !p1 || !p2 || !status || !results || !matchup || !records || !count) return fail(fn, "null argument");
  for (const oakgpu_build_seat_arrays *p : {p1, p2})
    if (!p->teams_init || !p->n_updates || !p->action || !p->prob) return fail(fn, "a seat's array is null");
  if (n == 0) return fail(fn, "n == 0");
  if ((uintptr_t)records & 3) return fail(fn, "records must be 4-byte aligned");
  RC(oakgpu_ctx_enter(ctx));
  const GameRecordArgs a{{*p1, *p2}, status, results, matchup, n, records, count};
  hipLaunchKernelGGL(k_build_game_records, dim3(1), dim3(RECORD_BLOCK), 0, (hipStream_t)oakgpu_ctx_stream(ctx), a);
  HIPCHK(hipGetLastError());
  return 0;
}

int oakgpu_build_game_targets_host(int status, uint8_t result, double matchup, int seat, float *value, float *score) {
  const char *fn = "oakgpu_build_game_targets_host";
  if (!value || !score) return fail(fn, "null argument");
  if (seat != 0 && seat != 1) return fail(fn, "seat outside {0, 1}");
  *value = 0.f; *score = -1.f;
  return game_targets((uint32_t)status, result, matchup, seat, value, score) ? 1 : 0;
}

// ---- host-pointer wrappers: staged in, staged out, complete on return
namespace {
struct Staged {
  oakgpu_build_outputs dev{};
  uint32_t n = 0;
  bool provide = false, trace = false;
};
int stage_outputs(OakHostCall &call, uint32_t n, bool provide, bool trace, Staged &s) {
  s.n = n; s.provide = provide; s.trace = trace;
  auto get = [&](size_t bytes) { return call.get(bytes); };
  s.dev.teams_out = (uint8_t *)get((size_t)n * 30);
  s.dev.n_updates = (uint8_t *)get(n);
  s.dev.action = (uint16_t *)get((size_t)n * STEPS * 2);
  s.dev.index = (uint16_t *)get((size_t)n * STEPS * 2);
  s.dev.n_legal = (uint16_t *)get((size_t)n * STEPS * 2);
  s.dev.prob = (float *)get((size_t)n * STEPS * 4);
  if (!s.dev.teams_out || !s.dev.n_updates || !s.dev.action || !s.dev.index || !s.dev.n_legal || !s.dev.prob) return -1;
  if (provide) {
    s.dev.teams_init = (uint8_t *)get((size_t)n * 30);
    s.dev.sizes_out = (uint8_t *)get(n);
    s.dev.team_index = (int32_t *)get((size_t)n * 4);
    if (!s.dev.teams_init || !s.dev.sizes_out || !s.dev.team_index) return -1;
  }
  if (trace) {
    const size_t cells = (size_t)n * STEPS * MAX_ACTIONS;
    s.dev.trace_legal = (int16_t *)get(cells * 2);
    s.dev.trace_logits = (float *)get(cells * 4);
    s.dev.trace_policy = (float *)get(cells * 4);
    if (!s.dev.trace_legal || !s.dev.trace_logits || !s.dev.trace_policy) return -1;
  }
  return 0;
}
// the per-step arrays and the trace go in as the caller holds them and come back whole: what the kernel leaves alone stays the caller's
int copy_outputs(hipStream_t stream, const Staged &s, const oakgpu_build_outputs *host, hipMemcpyKind kind) {
  const size_t n = s.n, steps = n * STEPS, cells = steps * MAX_ACTIONS;
  auto move = [&](void *d, void *h, size_t bytes) -> hipError_t {
    return kind == hipMemcpyHostToDevice ? hipMemcpyAsync(d, h, bytes, kind, stream) : hipMemcpyAsync(h, d, bytes, kind, stream);
  };
  HIPCHK(move(s.dev.teams_out, host->teams_out, n * 30));
  HIPCHK(move(s.dev.n_updates, host->n_updates, n));
  HIPCHK(move(s.dev.action, host->action, steps * 2));
  HIPCHK(move(s.dev.index, host->index, steps * 2));
  HIPCHK(move(s.dev.n_legal, host->n_legal, steps * 2));
  HIPCHK(move(s.dev.prob, host->prob, steps * 4));
  if (s.provide) {
    HIPCHK(move(s.dev.teams_init, host->teams_init, n * 30));
    HIPCHK(move(s.dev.sizes_out, host->sizes_out, n));
    HIPCHK(move(s.dev.team_index, host->team_index, n * 4));
  }
  if (s.trace) {
    HIPCHK(move(s.dev.trace_legal, host->trace_legal, cells * 2));
    HIPCHK(move(s.dev.trace_logits, host->trace_logits, cells * 4));
    HIPCHK(move(s.dev.trace_policy, host->trace_policy, cells * 4));
  }
  return 0;
}
} // namespace

int oakgpu_build_rollout(oakgpu_ctx *ctx, const oakgpu_build_net *net, const uint8_t *teams, const uint8_t *sizes, const uint64_t *seeds, uint32_t n,
                         int input_update, const oakgpu_build_outputs *out) {
  RC(oakgpu_build_teams_check(teams, sizes, n, input_update));
  if (!ctx || !net || !seeds || !out) return oakgpu_fail_msg("oakgpu_build_rollout: null argument");
  if (!out->teams_out || !out->n_updates || !out->action || !out->index || !out->n_legal || !out->prob)
    return oakgpu_fail_msg("oakgpu_build_rollout: a required output is null");
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall call(ctx);
  Staged s;
  RC(stage_outputs(call, n, false, out->trace_legal != nullptr, s));
  if (s.trace && (!out->trace_logits || !out->trace_policy)) return oakgpu_fail_msg("oakgpu_build_rollout: the trace arrays come together or not at all");
  uint8_t *d_teams = (uint8_t *)call.get((size_t)n * 30), *d_sizes = sizes ? (uint8_t *)call.get(n) : nullptr;
  uint64_t *d_seeds = (uint64_t *)call.get((size_t)n * 8);
  if (!d_teams || !d_seeds || (sizes && !d_sizes)) return -1;
  HIPCHK(hipMemcpyAsync(d_teams, teams, (size_t)n * 30, hipMemcpyHostToDevice, stream));
  if (sizes) HIPCHK(hipMemcpyAsync(d_sizes, sizes, n, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_seeds, seeds, (size_t)n * 8, hipMemcpyHostToDevice, stream));
  RC(copy_outputs(stream, s, out, hipMemcpyHostToDevice));
  RC(oakgpu_build_rollout_dev(ctx, net, d_teams, d_sizes, d_seeds, n, input_update, &s.dev));
  RC(copy_outputs(stream, s, out, hipMemcpyDeviceToHost));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_build_provide(oakgpu_ctx *ctx, const oakgpu_build_net *net, const uint8_t *pool, uint32_t pool_n, const uint64_t *seeds, uint32_t n,
                         const oakgpu_build_provider *prm, const oakgpu_build_outputs *out) {
  if (!prm) return oakgpu_fail_msg("oakgpu_build_provide: null argument");
  RC(oakgpu_build_provide_check(pool, pool_n, n, prm->max_pokemon, prm->pokemon_delete_prob, prm->move_delete_prob, prm->team_modify_prob));
  if (prm->input_update != 0 && prm->input_update != 1) return oakgpu_fail_msg("oakgpu_build_provide: input_update outside {0, 1}");
  if (!ctx || !net || !seeds || !out) return oakgpu_fail_msg("oakgpu_build_provide: null argument");
  if (!out->teams_out || !out->n_updates || !out->action || !out->index || !out->n_legal || !out->prob || !out->teams_init || !out->sizes_out || !out->team_index)
    return oakgpu_fail_msg("oakgpu_build_provide: a required output is null");
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall call(ctx);
  Staged s;
  RC(stage_outputs(call, n, true, out->trace_legal != nullptr, s));
  if (s.trace && (!out->trace_logits || !out->trace_policy)) return oakgpu_fail_msg("oakgpu_build_provide: the trace arrays come together or not at all");
  uint8_t *d_pool = (uint8_t *)call.get((size_t)pool_n * 30);
  uint64_t *d_seeds = (uint64_t *)call.get((size_t)n * 8);
  if (!d_pool || !d_seeds) return -1;
  HIPCHK(hipMemcpyAsync(d_pool, pool, (size_t)pool_n * 30, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_seeds, seeds, (size_t)n * 8, hipMemcpyHostToDevice, stream));
  RC(copy_outputs(stream, s, out, hipMemcpyHostToDevice));
  RC(oakgpu_build_provide_dev(ctx, net, d_pool, pool_n, d_seeds, n, prm, &s.dev));
  RC(copy_outputs(stream, s, out, hipMemcpyDeviceToHost));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_build_records(oakgpu_ctx *ctx, const uint8_t *teams_init, const uint8_t *sizes, const uint8_t *n_updates, const uint16_t *action, const float *prob,
                         const float *value, const float *score, uint32_t n, uint8_t *records, uint32_t *count) {
  const char *fn = "oakgpu_build_records";
  if (!ctx || !teams_init || !n_updates || !action || !prob || !value || !score || !records || !count) return fail(fn, "null argument");
  if (n == 0) return fail(fn, "n == 0");
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t size = sizes ? sizes[g] : 6;
    if (size > 6) return fail(fn, "team " + std::to_string(g) + ": size > 6");
    if (n_updates[g] > STEPS) return fail(fn, "team " + std::to_string(g) + ": n_updates above 31");
    if (const char *fault = team_fault(teams_init + (size_t)g * 30, size)) return fail(fn, "team " + std::to_string(g) + ": " + fault);
  }
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  OakHostCall call(ctx);
  const size_t steps = (size_t)n * STEPS;
  uint8_t *d_teams = (uint8_t *)call.get((size_t)n * 30), *d_sizes = sizes ? (uint8_t *)call.get(n) : nullptr, *d_updates = (uint8_t *)call.get(n);
  uint16_t *d_action = (uint16_t *)call.get(steps * 2);
  float *d_prob = (float *)call.get(steps * 4), *d_value = (float *)call.get((size_t)n * 4), *d_score = (float *)call.get((size_t)n * 4);
  uint8_t *d_records = (uint8_t *)call.get((size_t)n * RECORD_BYTES);
  uint32_t *d_count = (uint32_t *)call.get(4);
  if (!d_teams || (sizes && !d_sizes) || !d_updates || !d_action || !d_prob || !d_value || !d_score || !d_records || !d_count) return -1;
  HIPCHK(hipMemcpyAsync(d_teams, teams_init, (size_t)n * 30, hipMemcpyHostToDevice, stream));
  if (sizes) HIPCHK(hipMemcpyAsync(d_sizes, sizes, n, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_updates, n_updates, n, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_action, action, steps * 2, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_prob, prob, steps * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_value, value, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_score, score, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  RC(oakgpu_build_records_dev(ctx, d_teams, d_sizes, d_updates, d_action, d_prob, d_value, d_score, n, d_records, d_count));
  HIPCHK(hipMemcpyAsync(count, d_count, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (*count) HIPCHK(hipMemcpyAsync(records, d_records, (size_t)*count * RECORD_BYTES, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

} // extern "C"
