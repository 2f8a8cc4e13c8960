// oak_amd/csrc/gen1_device.hpp -- what the device-side gen-1 (RBY) engine is written in terms of; the
// turn resolution itself is gen1_regs.hpp's EngineR.
//
// Here: the rule switches (OAK_*), the result / choice encodings, the byte layout of the 384-byte
// battle (identical to cpp/include/libpkmn/layout.h so AoS buffers round-trip unchanged), volatile,
// status and chance-action bits, the LDS pointer types, and the engine's tables -- move / species /
// type-chart / stage / reciprocal tables and the per-effect descriptors (struct Tables), built
// once into LDS by stage_tables from the packed images in gen1_tables.inc -- with struct Move.
// Build configuration of libpkmn mirrored: dev/libpkmn:9 of the reference (showdown, miss=false,
// advance=false, ebc=false, key=true, chance, calc).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oak {

#include "gen1_tables.inc"

// Roll-order choices that pkmn/engine's -Dshowdown path settles by following Pokemon Showdown's own code (the reference builds
// libpkmn with -Dshowdown: /root/reference/dev/libpkmn:9).  Same names and defaults in the CPU checker's restatement of the engine (the tests hold the two to each other); 0 = rounds 1-3:
//   OAK_MULTIHIT_ROLL_FIRST  multi-hit count rolled behind the accuracy check, before crit / damage (gen-1 tryMoveHit)
//   OAK_PSYWAVE_SHOWDOWN     Psywave = random(0, level * 3 / 2), a 0 fails (Desync Clause Mod); the action holds the roll + 1
#ifndef OAK_MULTIHIT_ROLL_FIRST
#define OAK_MULTIHIT_ROLL_FIRST 1
#endif
#ifndef OAK_PSYWAVE_SHOWDOWN
#define OAK_PSYWAVE_SHOWDOWN 1
#endif
//   OAK_COUNTER_SHOWDOWN     (round 5, default 0) Counter hits iff the target side's last USED and last SELECTED move are both counterable
//                            (bp > 0, Normal / Fighting, not Counter) and last_damage > 0 -- Showdown's gen-1 damageCallback; 0: the
//                            `counterable` byte of last_moves[]
//   OAK_ACCURACY_LAST        (round 5, default 0) cartridge roll order of ordinary damaging moves: crit, damage roll, THEN accuracy
#ifndef OAK_COUNTER_SHOWDOWN
#define OAK_COUNTER_SHOWDOWN 0
#endif
#ifndef OAK_ACCURACY_LAST
#define OAK_ACCURACY_LAST 0
#endif
#if OAK_ACCURACY_LAST && OAK_MULTIHIT_ROLL_FIRST
#error "OAK_ACCURACY_LAST needs -DOAK_MULTIHIT_ROLL_FIRST=0 (the count is rolled behind the accuracy check)"
#endif

// ---- result / choice encodings (cpp/include/libpkmn/pkmn.h:108-133,214-233) ------------
enum : uint32_t { R_NONE = 0, R_WIN = 1, R_LOSE = 2, R_TIE = 3, R_ERROR = 4 };
enum : uint32_t { C_PASS = 0, C_MOVE = 1, C_SWITCH = 2 };
__device__ __forceinline__ uint32_t mk_result(uint32_t t, uint32_t p1, uint32_t p2) { return t | (p1 << 4) | (p2 << 6); }

// ---- byte offsets (cpp/include/libpkmn/layout.h:15-50) ---------------------------------
enum : int {
  SIDE_SZ = 184, PK_SZ = 24,
  O_ACTIVE = 144, O_ORDER = 176, O_LAST_SEL = 182, O_LAST_USED = 183,
  P_HP_MAX = 0, P_ATK = 2, P_DEF = 4, P_SPE = 6, P_SPC = 8, P_MOVES = 10, P_HP = 18, P_STATUS = 20,
  P_SPECIES = 21, P_TYPES = 22, P_LEVEL = 23,
  A_STATS = 0, A_SPECIES = 10, A_TYPES = 11, A_BOOSTS = 12, A_VOL = 16, A_MOVES = 24,
  B_TURN = 368, B_LAST_DAMAGE = 370, B_LAST_MOVES = 372, B_RNG = 376,
};

// volatiles (layout.h:69-96), split over the two dwords at A_VOL / A_VOL+4
enum : uint32_t {
  V_BIDE = 1u << 0, V_THRASHING = 1u << 1, V_MULTIHIT = 1u << 2, V_FLINCH = 1u << 3, V_CHARGING = 1u << 4,
  V_BINDING = 1u << 5, V_INVULNERABLE = 1u << 6, V_CONFUSION = 1u << 7, V_MIST = 1u << 8,
  V_FOCUSENERGY = 1u << 9, V_SUBSTITUTE = 1u << 10, V_RECHARGING = 1u << 11, V_RAGE = 1u << 12,
  V_LEECHSEED = 1u << 13, V_TOXIC = 1u << 14, V_LIGHTSCREEN = 1u << 15, V_REFLECT = 1u << 16,
  V_TRANSFORM = 1u << 17,
};
enum : uint32_t { ST_SLP = 7, ST_PSN = 0x08, ST_BRN = 0x10, ST_FRZ = 0x20, ST_PAR = 0x40, ST_EXT = 0x80, ST_TOX = 0x88 };

// chance-action bit offsets (layout.h:98-117)
enum : int { AC_DAMAGE = 0, AC_HIT = 8, AC_CRIT = 10, AC_SECONDARY = 12, AC_SPEEDTIE = 14, AC_CONFUSED = 16,
             AC_PARALYZED = 18, AC_SLEEP = 24, AC_CONFUSION = 26, AC_DISABLE = 29, AC_ATTACKING = 31,
             AC_BINDING = 33, AC_MOVESLOT = 36, AC_MULTIHIT = 44, AC_PSYWAVE = 48, AC_METRONOME = 56 };
enum : uint32_t { OBS_STARTED = 1, OBS_CONTINUING = 2, OBS_ENDED = 3 };

// LDS-address-space pointer types: keeping the address space in the type makes hipcc emit
// ds_read/ds_write (lgkmcnt only) instead of flat_load/flat_store for every state access.
#define OAK_LDS __attribute__((address_space(3)))
typedef OAK_LDS uint32_t lds_u32;
typedef OAK_LDS uint16_t lds_u16;
typedef OAK_LDS uint8_t lds_u8;

struct Tables {
  const lds_u32 *mv;     // [166] effect | bp<<8 | type<<16 | acc<<24
  const lds_u8 *maxpp;   // [166]
  const lds_u32 *sp0;    // [152]
  const lds_u32 *sp1;    // [152]
  const lds_u8 *chart;   // [225]
  const lds_u32 *boost;  // [13] ceil(2^29 * num / den): x * num / den == umulhi(x << 3, boost) for x < 2^16
  const lds_u32 *rcp;    // [256] floor((2^32-1)/d) + 1: exact x / d by one mul-hi for x < 2^24, d in 2..255
  const lds_u16 *fx;     // [68] per-effect descriptor (fx_desc below): gate / action class / secondary effect
  const lds_u16 *bits;   // [32] the set-bit positions of a mask < 32, lowest first, 3 bits each (bit_list below): the random policy's pick
};
static constexpr int TABLE_LDS_BYTES = 166 * 4 + 168 + 152 * 4 + 152 * 4 + 228 + 13 * 4 + 256 * 4 + 68 * 2 + 32 * 2;

// ---- per-effect descriptors: what gen1_regs.hpp's run_move needs to know about a move effect, as data.
// Lanes of a wave run different moves; a `switch (effect)` costs the wave every case any lane takes plus the
// exec-mask bookkeeping of all of them, a table lookup costs one LDS read and a few selects for everybody.
//   status moves (bp == 0):  bits 0-3 gate (can the move fail before / instead of its accuracy check),
//                            bits 4-6 action class, bits 7-11 its parameter
//   damaging moves:          bits 0-2 secondary-effect kind, 3-5 chance index, 6-8 parameter
enum : uint32_t { G_NONE = 0, G_SUB, G_INVUL, G_GRASS, G_HIT, G_PAR, G_PSN, G_TELE, G_SLEEP, G_DISABLE };
enum : uint32_t { A_NONE = 0, A_BOOST, A_UNBOOST, A_SVOL, A_FVOL, A_PAR, A_CONF, A_HEAVY };
enum : uint32_t { SEC_NONE = 0, SEC_STATUS = 1, SEC_FLINCH = 2, SEC_CONF = 3, SEC_UNBOOST = 4 };
// chance index -> x/256: 0: 26 (10%), 1: 77 (30%), 2: 52 (20%), 3: 103 (40%), 4: 25 (confusion), 5: 85 (stat drop)
static constexpr uint64_t FX_CHANCES = 26ull | (77ull << 8) | (52ull << 16) | (103ull << 24) | (25ull << 32) | (85ull << 40);
constexpr uint32_t fx_status(uint32_t gate, uint32_t cls, uint32_t par) { return gate | (cls << 4) | (par << 7); }
constexpr uint32_t fx_stage(uint32_t idx, uint32_t n) { return idx | ((n - 1) << 3); } // stat idx 0 atk 1 def 2 spe 3 spc 4 acc 5 eva
constexpr uint32_t fx_sec(uint32_t kind, uint32_t chance_idx, uint32_t par) { return kind | (chance_idx << 3) | (par << 6); }
constexpr uint32_t fx_desc(uint32_t e) {
  switch (e) {
  case E_Confusion: return fx_status(G_SUB, A_CONF, 0);
  case E_Conversion: case E_Transform: return fx_status(G_INVUL, A_HEAVY, 0);
  case E_FocusEnergy: return fx_status(G_NONE, A_SVOL, 9);   // V_FOCUSENERGY
  case E_LightScreen: return fx_status(G_NONE, A_SVOL, 15);  // V_LIGHTSCREEN
  case E_Reflect: return fx_status(G_NONE, A_SVOL, 16);      // V_REFLECT
  case E_Mist: return fx_status(G_NONE, A_SVOL, 8);          // V_MIST
  case E_LeechSeed: return fx_status(G_GRASS, A_FVOL, 13);   // V_LEECHSEED
  case E_Haze: case E_Heal: case E_Substitute: case E_Bide: return fx_status(G_NONE, A_HEAVY, 0);
  case E_Mimic: return fx_status(G_HIT, A_HEAVY, 0);
  case E_Paralyze: return fx_status(G_PAR, A_PAR, 0);
  case E_Poison: return fx_status(G_PSN, A_HEAVY, 0);
  case E_SwitchAndTeleport: return fx_status(G_TELE, A_NONE, 0);
  case E_Sleep: return fx_status(G_SLEEP, A_HEAVY, 0);
  case E_Disable: return fx_status(G_DISABLE, A_HEAVY, 0);
  case E_AccuracyDown1: return fx_status(G_SUB, A_UNBOOST, fx_stage(4, 1));
  case E_AttackDown1: return fx_status(G_SUB, A_UNBOOST, fx_stage(0, 1));
  case E_DefenseDown1: return fx_status(G_SUB, A_UNBOOST, fx_stage(1, 1));
  case E_DefenseDown2: return fx_status(G_SUB, A_UNBOOST, fx_stage(1, 2));
  case E_SpeedDown1: return fx_status(G_SUB, A_UNBOOST, fx_stage(2, 1));
  case E_AttackUp1: return fx_status(G_NONE, A_BOOST, fx_stage(0, 1));
  case E_AttackUp2: return fx_status(G_NONE, A_BOOST, fx_stage(0, 2));
  case E_DefenseUp1: return fx_status(G_NONE, A_BOOST, fx_stage(1, 1));
  case E_DefenseUp2: return fx_status(G_NONE, A_BOOST, fx_stage(1, 2));
  case E_SpeedUp2: return fx_status(G_NONE, A_BOOST, fx_stage(2, 2));
  case E_SpecialUp1: return fx_status(G_NONE, A_BOOST, fx_stage(3, 1));
  case E_SpecialUp2: return fx_status(G_NONE, A_BOOST, fx_stage(3, 2));
  case E_EvasionUp1: return fx_status(G_NONE, A_BOOST, fx_stage(5, 1));
  // damaging: secondary effects; the status parameter p means status byte 8 << p (PSN BRN FRZ PAR)
  case E_PoisonChance1: case E_Twineedle: return fx_sec(SEC_STATUS, 2, 0);
  case E_PoisonChance2: return fx_sec(SEC_STATUS, 3, 0);
  case E_BurnChance1: return fx_sec(SEC_STATUS, 0, 1);
  case E_BurnChance2: return fx_sec(SEC_STATUS, 1, 1);
  case E_FreezeChance: return fx_sec(SEC_STATUS, 0, 2);
  case E_ParalyzeChance1: return fx_sec(SEC_STATUS, 0, 3);
  case E_ParalyzeChance2: return fx_sec(SEC_STATUS, 1, 3);
  case E_FlinchChance1: return fx_sec(SEC_FLINCH, 0, 0);
  case E_FlinchChance2: return fx_sec(SEC_FLINCH, 1, 0);
  case E_ConfusionChance: return fx_sec(SEC_CONF, 4, 0);
  case E_AttackDownChance: return fx_sec(SEC_UNBOOST, 5, 0);
  case E_DefenseDownChance: return fx_sec(SEC_UNBOOST, 5, 1);
  case E_SpeedDownChance: return fx_sec(SEC_UNBOOST, 5, 2);
  case E_SpecialDownChance: return fx_sec(SEC_UNBOOST, 5, 3);
  default: return 0; // Splash, plain damage, effects handled outside run_move
  }
}
// the positions of the set bits of a mask < 32, lowest first, packed 3 bits each: (bit_list(m) >> 3 * k) & 7 is the k-th set bit of m
constexpr uint32_t bit_list(uint32_t mask) {
  uint32_t list = 0, k = 0;
  for (uint32_t b = 0; b < 5; ++b)
    if ((mask >> b) & 1) list |= b << (3 * k++);
  return list;
}
struct FxTable {
  uint16_t d[68];
  constexpr FxTable() : d{} { for (uint32_t e = 0; e < 68; ++e) d[e] = (uint16_t)fx_desc(e); }
};
static __device__ const FxTable OAK_FX{};
struct BitListTable {
  uint16_t d[32];
  constexpr BitListTable() : d{} { for (uint32_t m = 0; m < 32; ++m) d[m] = (uint16_t)bit_list(m); }
};
static __device__ const BitListTable OAK_BIT_LISTS{};

// where each table sits in the workgroup's LDS table area (TABLE_LDS_BYTES)
__device__ __forceinline__ Tables tables_at(lds_u8 *lds) {
  lds_u32 *mv = (lds_u32 *)lds;
  lds_u8 *pp = lds + 166 * 4;
  lds_u32 *sp0 = (lds_u32 *)(pp + 168);
  lds_u32 *sp1 = sp0 + 152;
  lds_u8 *chart = (lds_u8 *)(sp1 + 152);
  lds_u32 *boost = (lds_u32 *)(chart + 228);
  lds_u32 *rcp = boost + 13;
  lds_u16 *fx = (lds_u16 *)(rcp + 256);
  Tables t{mv, pp, sp0, sp1, chart, boost, rcp, fx, fx + 68};
  return t;
}

// builds the tables in LDS from the packed images; call with all threads of the workgroup, then barrier.  (Only the
// table-image builder does this: the rollout kernels copy the finished image, see stage_default_tables.)  BIT_LISTS: fill
// Tables::bits too -- the image builder does; only the random policy's pick reads that table, and only kernels that copy the image
// play it, so a kernel that stages its own tables leaves it out.
template <bool BIT_LISTS = false>
__device__ inline Tables stage_tables(lds_u8 *lds, const uint32_t *g_mv, const uint8_t *g_pp, const uint32_t *g_sp0,
                                      const uint32_t *g_sp1, const uint8_t *g_chart, const uint32_t *g_boost) {
  lds_u32 *mv = (lds_u32 *)lds;
  lds_u8 *pp = lds + 166 * 4;
  lds_u32 *sp0 = (lds_u32 *)(pp + 168);
  lds_u32 *sp1 = sp0 + 152;
  lds_u8 *chart = (lds_u8 *)(sp1 + 152);
  lds_u32 *boost = (lds_u32 *)(chart + 228);
  lds_u32 *rcp = boost + 13;
  lds_u16 *fx = (lds_u16 *)(rcp + 256);
  for (int i = threadIdx.x; i < 256; i += blockDim.x) rcp[i] = i ? 0xFFFFFFFFu / (uint32_t)i + 1u : 0u;
  for (int i = threadIdx.x; i < 68; i += blockDim.x) fx[i] = OAK_FX.d[i];
  for (int i = threadIdx.x; i < 166; i += blockDim.x) { mv[i] = g_mv[i]; pp[i] = g_pp[i]; }
  for (int i = threadIdx.x; i < 152; i += blockDim.x) { sp0[i] = g_sp0[i]; sp1[i] = g_sp1[i]; }
  for (int i = threadIdx.x; i < 225; i += blockDim.x) chart[i] = g_chart[i];
  for (int i = threadIdx.x; i < 13; i += blockDim.x) boost[i] = g_boost[i];
  if constexpr (BIT_LISTS)
    for (int i = threadIdx.x; i < 32; i += blockDim.x) fx[68 + i] = OAK_BIT_LISTS.d[i];
  Tables t{mv, pp, sp0, sp1, chart, boost, rcp, fx, fx + 68};
  return t;
}

struct Move { // unpacked move word
  uint32_t w;
  __device__ __forceinline__ uint32_t effect() const { return w & 0xFF; }
  __device__ __forceinline__ uint32_t bp() const { return (w >> 8) & 0xFF; }
  __device__ __forceinline__ uint32_t type() const { return (w >> 16) & 0xFF; }
  __device__ __forceinline__ uint32_t acc() const { return w >> 24; }
};

} // namespace oak
