// oak_amd/csrc/build_traj.hpp -- the rule that turns one 128-byte NoTeam record of `.build.data` into a training trajectory: the reference's
// Py::Build::Trajectories::write (cpp/include/py/build/trajectories.h:145-233) with its TeamHelper / SetHelper (:17-101), statement for
// statement where the reference is defined, and a status where it asserts or runs out of bounds.  One text for the host and the device
// (as nash.hpp and selfplay_pick.hpp are): buildtraj.hip's kernel walks a record with a wave, oakgpu_build_traj_check and the stand-alone
// check (tests/cpp_build_traj_check.cc) walk it with one thread.  The contract is in include/oakgpu.h.
//
// The helper keeps what is MISSING, as the reference's does, in a form a wave can read at once:
//   * a set is {species, counted moves, remaining pool}.  In build_tables.inc a species' pool occupies the contiguous cells
//     CELL_BASE[s] + 1 .. CELL_BASE[s] + POOL_SIZE[s] in pool order and no pool holds more than 64 moves, so a remaining pool is a 64-bit
//     mask and std::remove of a move is one cleared bit (the order of the rest is kept, as std::remove keeps it);
//   * the available species are the legal species that no set holds: std::erase(available_species, s) removes every s, sets are only ever
//     added, so "not in the team" is the same list.
// Every list is then a stable compaction of flags in cell order within a set, and the PLACE of an entry is a count of the flags in front
// of it -- no entry waits for another one.  list_write takes (lane, lanes): one thread writes a list alone with (0, 1), a wave with
// (lane, 64).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OAK_BT_HD __host__ __device__
#else
#define OAK_BT_HD
#endif

namespace oak_build_traj {

namespace host_tab {
#define OAK_BUILD_TABLE static const
#include "build_tables.inc"
#undef OAK_BUILD_TABLE
} // namespace host_tab
#if defined(__HIPCC__)
namespace dev_tab {
#define OAK_BUILD_TABLE static __device__ const
#include "build_tables.inc"
#undef OAK_BUILD_TABLE
} // namespace dev_tab
#endif
#if defined(__HIP_DEVICE_COMPILE__)
namespace tab = dev_tab;
#else
namespace tab = host_tab;
#endif

constexpr uint32_t N_DIM = OAK_BUILD_N_DIM, MAX_ACTIONS = OAK_BUILD_MAX_ACTIONS, N_LEGAL = OAK_BUILD_N_LEGAL;
constexpr uint32_t STEPS = 31, RECORD_BYTES = 128, MAX_SETS = 6;

// the status of a record (include/oakgpu.h: OAKGPU_BUILD_TRAJ_*)
enum : uint8_t { OK = 0, BAD_ACTION = 1, NO_SPECIES = 2, TEAM_FULL = 3, NOT_LEGAL = 4, LIST_OVERFLOW = 5, N_STATUS = 6 };

OAK_BT_HD inline uint32_t popcount64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}

// ---- the record: {u8 format, u8 score, u16 value, 31 x {u16 action, u16 probability}}, little endian -------------------------------------
OAK_BT_HD inline uint32_t rec_action(const uint8_t *r, uint32_t i) { return (uint32_t)r[4 + 4 * i] | ((uint32_t)r[5 + 4 * i] << 8); }
OAK_BT_HD inline uint32_t rec_probability(const uint8_t *r, uint32_t i) { return (uint32_t)r[6 + 4 * i] | ((uint32_t)r[7 + 4 * i] << 8); }
// x / 65535.0f, a correctly rounded float division on both sides (not a reciprocal multiply)
OAK_BT_HD inline float over_65535(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn((float)x, 65535.0f);
#else
  return (float)x / 65535.0f;
#endif
}
OAK_BT_HD inline float rec_value(const uint8_t *r) { return over_65535((uint32_t)r[2] | ((uint32_t)r[3] << 8)); }
// header.score / 2.0 rounded to float (exact).  The reference compares the 8-bit score with 65,535, so a record without a score (255)
// reads as 127.5; no_score gives the -1 it meant.
OAK_BT_HD inline float rec_score(const uint8_t *r, int no_score) { return (no_score && r[1] == 255) ? -1.0f : (float)r[1] * 0.5f; }
OAK_BT_HD inline float probability_of(uint32_t q) { return over_65535(q); }

// ---- the bounds, as the loops of trajectories.h:159-187 take them -----------------------------------------------------------------------
struct Bounds { int32_t start, end, swap, full; };

OAK_BT_HD inline Bounds bounds_of(const uint8_t *r) {
  Bounds b{0, 0, 0, 0};
  for (int32_t i = 0; i < (int32_t)STEPS; ++i)
    if (rec_probability(r, i) != 0) { b.start = i; break; }
  for (int32_t i = (int32_t)STEPS - 1; i >= 0; --i) {
    if (rec_probability(r, i) == 0) continue;
    const uint32_t a = rec_action(r, i);
    const bool none = a < N_DIM && tab::CELL_MOVE[a] == 0; // (an action outside the table makes the record BAD_ACTION below)
    if (b.end == 0) {
      b.end = i + 1;
      b.swap = b.end - (none ? 1 : 0);
    } else if (none) {
      b.full = i + 1;
      break;
    }
  }
  return b;
}

// ---- the helper ---------------------------------------------------------------------------------------------------------------------------
struct Helper {
  uint32_t n_sets;
  uint8_t species[MAX_SETS], n_moves[MAX_SETS];
  uint64_t remaining[MAX_SETS];
};

OAK_BT_HD inline void helper_init(Helper &h) {
  h.n_sets = 0;
  for (uint32_t j = 0; j < MAX_SETS; ++j) { h.species[j] = 0; h.n_moves[j] = 0; h.remaining[j] = 0; }
}
OAK_BT_HD inline bool set_complete(const Helper &h, uint32_t j) { return h.n_moves[j] >= 4 || h.remaining[j] == 0; }
OAK_BT_HD inline bool holds_species(const Helper &h, uint32_t s) {
  bool held = false;
  for (uint32_t j = 0; j < h.n_sets; ++j) held = held || h.species[j] == s;
  return held;
}
// the distinct species of the team below `limit` (a pre-start species that is already in the team adds a second set: count it once)
OAK_BT_HD inline uint32_t distinct_below(const Helper &h, uint32_t limit) {
  uint32_t count = 0;
  for (uint32_t j = 0; j < h.n_sets; ++j) {
    bool first = h.species[j] < limit;
    for (uint32_t k = 0; k < j; ++k) first = first && h.species[k] != h.species[j];
    count += first ? 1u : 0u;
  }
  return count;
}
OAK_BT_HD inline uint32_t available_count(const Helper &h) { return N_LEGAL - distinct_below(h, 256); }
// legal species in front of s (LEGAL_SPECIES ascends: a bisection)
OAK_BT_HD inline uint32_t legal_below(uint32_t s) {
  uint32_t lo = 0, hi = N_LEGAL;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tab::LEGAL_SPECIES[mid] < s) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// TeamHelper::apply_action of a cell below N_DIM: what it would do wrong (OK: nothing), then the action itself
OAK_BT_HD inline uint8_t apply_fault(const Helper &h, uint32_t cell) {
  if (tab::CELL_MOVE[cell] == 0) return h.n_sets >= MAX_SETS ? TEAM_FULL : OK;
  return holds_species(h, tab::CELL_SPECIES[cell]) ? OK : NO_SPECIES;
}
OAK_BT_HD inline void apply_action(Helper &h, uint32_t cell) {
  const uint32_t s = tab::CELL_SPECIES[cell];
  if (tab::CELL_MOVE[cell] == 0) {
    const uint32_t j = h.n_sets++;
    const uint32_t pool = tab::POOL_SIZE[s];
    h.species[j] = (uint8_t)s;
    h.n_moves[j] = 0;
    h.remaining[j] = pool >= 64 ? ~0ull : (1ull << pool) - 1;
    return;
  }
  uint32_t j = 0;
  while (h.species[j] != s) ++j; // find_if: the first set of the species (apply_fault says there is one)
  const uint64_t bit = 1ull << (cell - tab::CELL_BASE[s] - 1);
  if (h.remaining[j] & bit) { // add_move of a move that is not in the remaining pool changes nothing
    h.remaining[j] &= ~bit;
    ++h.n_moves[j];
  }
}

// ---- the list of step i (start <= i < end): species if i < full, then the incomplete sets' remaining pools if i < swap; the sets' species
// cells if i >= swap -------------------------------------------------------------------------------------------------------------------------
OAK_BT_HD inline uint32_t list_length(const Helper &h, int32_t i, const Bounds &b) {
  if (i >= b.swap) return h.n_sets;
  uint32_t n = i < b.full ? available_count(h) : 0;
  for (uint32_t j = 0; j < h.n_sets; ++j)
    if (!set_complete(h, j)) n += popcount64(h.remaining[j]);
  return n;
}

// std::find of the taken action in the list: its place, or -1
OAK_BT_HD inline int32_t list_find(const Helper &h, int32_t i, const Bounds &b, uint32_t cell) {
  const uint32_t s = tab::CELL_SPECIES[cell], m = tab::CELL_MOVE[cell];
  if (i >= b.swap) {
    if (m != 0) return -1;
    for (uint32_t j = 0; j < h.n_sets; ++j)
      if (h.species[j] == s) return (int32_t)j;
    return -1;
  }
  if (m == 0) {
    if (i >= b.full || holds_species(h, s)) return -1;
    return (int32_t)(legal_below(s) - distinct_below(h, s));
  }
  uint32_t offset = i < b.full ? available_count(h) : 0;
  const uint32_t p = cell - tab::CELL_BASE[s] - 1;
  for (uint32_t j = 0; j < h.n_sets; ++j) {
    if (set_complete(h, j)) continue;
    if (h.species[j] == s && ((h.remaining[j] >> p) & 1)) return (int32_t)(offset + popcount64(h.remaining[j] & ((1ull << p) - 1)));
    offset += popcount64(h.remaining[j]);
  }
  return -1;
}

// The list into row[0 .. MAX_ACTIONS): this caller writes the entries lane, lane + lanes, ... of every part; nothing at or past MAX_ACTIONS.
OAK_BT_HD inline void list_write(const Helper &h, int32_t i, const Bounds &b, uint32_t lane, uint32_t lanes, int16_t *row) {
  if (i >= b.swap) {
    for (uint32_t j = lane; j < h.n_sets; j += lanes) row[j] = (int16_t)tab::CELL_BASE[h.species[j]];
    return;
  }
  uint32_t offset = 0;
  if (i < b.full) {
    for (uint32_t q = lane; q < N_LEGAL; q += lanes) {
      const uint32_t s = tab::LEGAL_SPECIES[q];
      if (holds_species(h, s)) continue;
      const uint32_t at = q - distinct_below(h, s);
      if (at < MAX_ACTIONS) row[at] = (int16_t)tab::CELL_BASE[s];
    }
    offset = available_count(h);
  }
  for (uint32_t j = 0; j < h.n_sets; ++j) {
    if (set_complete(h, j)) continue;
    const uint32_t s = h.species[j], base = tab::CELL_BASE[s], pool = tab::POOL_SIZE[s];
    const uint64_t left = h.remaining[j];
    for (uint32_t p = lane; p < pool; p += lanes) {
      if (!((left >> p) & 1)) continue;
      const uint32_t at = offset + popcount64(left & ((1ull << p) - 1));
      if (at < MAX_ACTIONS) row[at] = (int16_t)(base + 1 + p);
    }
    offset += popcount64(left);
  }
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------------------
// The visitor says who changes the helper and sees every list:
//   bool leader()                                         whether this caller applies the actions (one thread: always; a wave: lane 0)
//   void sync()                                           the helper's change becomes visible to every caller (one thread: nothing)
//   void row(i, bounds, helper, length, place, action)    the list of read step i, complete and legal, before its action is applied
// Returns the record's status.  BAD_ACTION is looked for first, over every step below `end` (the steps whose action the reference looks up
// in species_move_list); the other faults in step order.  The action of the last read step (i == end - 1) is NOT applied: the reference
// applies it after the step's list is written and no later step reads the helper, so no defined output depends on it -- and on a team of
// six, where that action is the lead swap, the reference's helper writes a seventh set out of bounds.
template <class Visitor> OAK_BT_HD inline uint8_t walk(const uint8_t *r, const Bounds &b, Helper &h, Visitor &v) {
  for (int32_t i = 0; i < b.end; ++i)
    if (rec_action(r, i) >= N_DIM) return BAD_ACTION;
  if (v.leader()) helper_init(h);
  v.sync();
  for (int32_t i = 0; i < b.end; ++i) {
    const uint32_t a = rec_action(r, i);
    if (i >= b.start) {
      const uint32_t length = list_length(h, i, b);
      if (length > MAX_ACTIONS) return LIST_OVERFLOW;
      const int32_t place = list_find(h, i, b, a);
      if (place < 0) return NOT_LEGAL;
      v.row(i, b, h, length, (uint32_t)place, a);
    }
    if (i == b.end - 1) break;
    const uint8_t fault = apply_fault(h, a);
    if (fault != OK) return fault;
    v.sync(); // (every caller has read the helper)
    if (v.leader()) apply_action(h, a);
    v.sync();
  }
  return OK;
}

struct StatusVisitor {
  OAK_BT_HD bool leader() const { return true; }
  OAK_BT_HD void sync() const {}
  OAK_BT_HD void row(int32_t, const Bounds &, const Helper &, uint32_t, uint32_t, uint32_t) const {}
};

OAK_BT_HD inline uint8_t record_status(const uint8_t *r) {
  const Bounds b = bounds_of(r);
  Helper h;
  StatusVisitor v;
  return walk(r, b, h, v);
}

} // namespace oak_build_traj
