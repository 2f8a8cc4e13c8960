/* include/oakgpu.h -- C ABI of liboakgpu.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE hot path of lab-oak/oak: batched random-playout turn stepping
 * and MLP leaf evaluation.  Every entry point is plain C (pointers + sizes, no torch / C++
 * types) so the reference's own FFI layers (C++ headers, pybind11) can bind it directly.
 * Each function cites the reference interface it replaces; INTEGRATION.md shows the
 * reference-side glue.
 *
 * Conventions
 *   - `*_dev` functions take DEVICE pointers and enqueue on the context's HIP stream
 *     without synchronising; the un-suffixed forms take HOST pointers, copy, run, copy
 *     back and synchronise (PCIe-inclusive; never the benchmarked path).
 *   - Battles are the reference's 384-byte POD (cpp/include/libpkmn/layout.h:5-31), AoS,
 *     n x 384 bytes; durations n x 8 bytes (data.h:270-311); choices / results one byte.
 *   - Return value 0 = success; otherwise a hipError_t-compatible code (or -1 for
 *     argument errors) and oakgpu_last_error() describes it.  There is NO CPU fallback:
 *     without a usable HIP device every call fails.
 */
#ifndef OAKGPU_H
#define OAKGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OAKGPU_BATTLE_SIZE 384
#define OAKGPU_DURATIONS_SIZE 8
#define OAKGPU_ACTIONS_SIZE 16
#define OAKGPU_MAX_CHOICES 9
#define OAKGPU_TEAMS_SIZE 60 /* 2 sides x 6 sets x {species, move x4} */

typedef struct oakgpu_ctx oakgpu_ctx;
typedef struct oakgpu_net oakgpu_net; /* a loaded .battle.net (see oakgpu_net_load below) */

int oakgpu_create(oakgpu_ctx **out, int device);
void oakgpu_destroy(oakgpu_ctx *ctx);
const char *oakgpu_last_error(void);
/* Use an existing hipStream_t (e.g. torch's current stream) for all *_dev launches. */
int oakgpu_set_stream(oakgpu_ctx *ctx, void *hip_stream);
/* The hipStream_t all *_dev launches of this context go to (own stream unless oakgpu_set_stream was called). */
void *oakgpu_get_stream(oakgpu_ctx *ctx);
int oakgpu_synchronize(oakgpu_ctx *ctx);
/* Diagnostics: with timing on, every oakgpu_leaf_eval*_dev call records HIP events around its three kernels on the
 * context's stream; oakgpu_get_leaf_kernel_ms waits for the last call and returns {party-slot embedding pass, actives'
 * embedding pass, main net} in milliseconds.  Off by default (the events cost a few microseconds per call). */
int oakgpu_set_kernel_timing(oakgpu_ctx *ctx, int on);
int oakgpu_get_leaf_kernel_ms(oakgpu_ctx *ctx, float ms[3]);
/* Rollout scheduling (results never depend on it).  k = 1 launches one lane per playout; k > 1 (default 2)
 * launches n/k persistent lanes that refill from an atomic playout queue as playouts finish. */
int oakgpu_set_playouts_per_lane(oakgpu_ctx *ctx, int k);
/* Regrouping rounds of the queue schedule (off unless this is called): the rollout runs as `rounds` dispatches (1..8); in
 * every round but the last a wave whose queue is dry and that has fewer than `suspend_below` (0..64) playouts still running
 * parks them (bit-exact state image) for the next round, which packs them 64 to a wave again on 1/`shrink` (>= 1) of the
 * waves.  It paid off while many small launches ran side by side on many streams (round 1); a lone launch is faster as one
 * dispatch (measured at every size, round 3), which is the default.  rounds = 1 or suspend_below = 0 disables it again. */
int oakgpu_set_regroup(oakgpu_ctx *ctx, int rounds, int suspend_below, int shrink);
/* The tail of a launch that saturates the device (a group of batches): when the playout queue is dry, a wave with fewer
 * than `below` (1..64; 0 = off) playouts still running parks them, and ONE follow-up dispatch of `waves` waves (0 = one
 * per compute unit) finishes the parked playouts, `lanes` of them per wave at a time (0 = 64).  The survivors are the rare
 * playouts that run into the step cap; a wave that holds one of them alone advances it no faster than a wave that holds
 * a few, and hundreds of such waves slow each other down.  Results never depend on it. */
int oakgpu_set_tail_pack(oakgpu_ctx *ctx, int below, int waves, int lanes);
/* The yielding schedule: the tail pack for a context whose saturating group launches alternate with another context's on the same
 * device.  The launch runs R = `waves` (0 = one per compute unit) waves FEWER than the device holds; when its queue is dry a wave with
 * fewer than `below` (1..64) playouts still running parks them and leaves, so its slot goes to the other context's pending launch; ONE
 * follow-up dispatch of at most R waves finishes the parked playouts, `lanes` per wave at a time (0 = 64), in the slots the other
 * context's launch leaves free.  Migration is off in it and no wave waits for another: correct whatever part of a grid is resident.
 * mode 0: off.  mode 1: automatic -- a launch that saturates the device with max_steps >= 500, when another live context of the device
 * has issued such a launch since this context's previous one (a host-side registry: no device query, no synchronisation); a context on
 * its own keeps the single dispatch with migration.  mode 2: every group launch of two waves or more (tests: a small launch parks with
 * a quarter of its waves as R).  Results never depend on it.  Also OAKGPU_YIELD_SCHEDULE / _BELOW / _WAVES / _LANES at context
 * creation.  Defaults below.
 * oakgpu_set_yield_saturation: automatic mode counts a launch of `waves` waves or more as saturating (0 = the device's resident waves;
 * tests lower it).  oakgpu_last_launch_yield: 1 if the context's last group launch took the schedule.  oakgpu_last_launch_parked
 * (synchronises the stream): the playouts the last group launch parked for its follow-up dispatch, 0 for a single dispatch. */
#define OAKGPU_YIELD_SCHEDULE_DEFAULT 1
#define OAKGPU_YIELD_BELOW_DEFAULT 12
#define OAKGPU_YIELD_WAVES_DEFAULT 256
#define OAKGPU_YIELD_LANES_DEFAULT 0
int oakgpu_set_yield_schedule(oakgpu_ctx *ctx, int mode, int below, int waves, int lanes);
int oakgpu_set_yield_saturation(oakgpu_ctx *ctx, int waves);
int oakgpu_last_launch_yield(oakgpu_ctx *ctx);
int oakgpu_last_launch_parked(oakgpu_ctx *ctx, uint32_t *parked);
/* Queue order of a launch of >= 8,192 playouts (default on): playouts with a Ghost-type Pokemon or a Ditto on either team are
 * handed out first.  They hold practically all of the playouts that run into the step cap (Normal-type Rage / Struggle locks
 * against a Ghost), and the launch ends with its longest playout: started early, the 1,000-step chains are mostly done when
 * the queue runs dry.  Pure scheduling: results are indexed by playout and never depend on it. */
int oakgpu_set_queue_order(oakgpu_ctx *ctx, int on);
/* Launches that do not fill the device use its empty wave slots: every wave takes only `lanes` playouts at a time, on as many
 * more waves as that needs (never more than the device holds).  -1 (default) = automatic: as few lanes per wave as fill the
 * device, at least 4; 0 or 64 = off.  Results never depend on it. */
int oakgpu_set_spread(oakgpu_ctx *ctx, int lanes);
/* Long-playout migration inside a launch (mode 0 off, 1 = launches that saturate the device (default), 2 = every queue launch:
 * tests): a wave hands a playout that is still running after `long_steps` turn-steps (default 300; 99.5% end before 250) to
 * `adopters` dedicated waves (0 = one per four compute units), which from the first donation on hold only such playouts -- a dozen
 * per wave at the top priority of their SIMD -- so the 1,000-step chains that end a launch advance at a sparse wave's pace
 * long before the device drains.  State travels as the regrouping rounds' bit-exact image; results never depend on it.
 * Co-residency of the launch's waves is NOT required (other launches may share the device, e.g. a second context's group launch):
 * a bulk wave never waits for anybody, so it always runs to its end and counts itself out; an adopter waits only for bulk waves
 * (bounded: ~10 s of polls, then the sticky error word and a failed oakgpu_synchronize) and holds nothing a bulk wave needs --
 * tests/test_gpu_parity.py::test_two_contexts_migrate_concurrently_on_one_device. */
int oakgpu_set_migration(oakgpu_ctx *ctx, int mode, int long_steps, int adopters);
/* ... and, earlier than that, a playout whose two active Pokemon have stood still -- same slots, same hp -- for `window`
 * consecutive turn-steps (default 48; 0 = off; at most 255): the playouts that run into the 1,000-step cap are stalemates whose
 * hp stop changing at a median of turn-step 85, so they leave their full wave at ~step 135 instead of 300.  A heuristic about
 * WHO finishes a playout only; results never depend on it. */
int oakgpu_set_migration_window(oakgpu_ctx *ctx, int window);
/* The queue kernel takes a PROVEN inert standstill to its last turn-step in one go: each side is either frozen with no way out (gen 1
 * never thaws by itself) or forced -- Rage-locked, or down to Struggle on its last Pokemon -- into a move the foe's types are immune
 * to, and nothing else acts on either.  Every such turn-step changes nothing but the turn counter and battle.rng, by a constant 0..3
 * draws (speed tie, full-paralysis rolls), which the skip applies as one jump of the generator (exact;
 * tests/test_gpu_inert_standstill.py, tests/test_gpu_parity.py::test_frozen_standstill_skip_is_exact).  on = 0 plays every turn-step
 * instead (A / B; also OAKGPU_STANDSTILL_SKIP=0 at context creation).  Default 1.  The one-lane-per-playout kernels (k_rollout_regs,
 * k_root_step) never skip. */
int oakgpu_set_standstill_skip(oakgpu_ctx *ctx, int on);
/* Move carry of the queue kernel.  A turn is up to two actions and a wave walks one copy of the action code once per action; a switch
 * goes before a move, so both walks hold the move pipeline for well under half of the wave's lanes.  With below > 0 a lane's second
 * action waits for the wave's NEXT walk -- beside the other lanes' first actions of their next turn -- unless at least `below` lanes
 * of the wave want it now.  below = 0: off, both actions of a turn in one wave iteration; 1..64: carry (64: whenever any lane of
 * the wave has no second action to run).  Dry waves (but see oakgpu_set_move_carry_dry), adopting waves, resume / tail rounds and
 * launches spread over part of their lanes never carry, so every playout that is written out, parked or donated stands at a turn boundary.  Every playout executes
 * the same engine operations and draws in the same order: results never depend on it.  Range checked; applies to launches made
 * after the call (also OAKGPU_MOVE_CARRY at context creation).  Default OAKGPU_MOVE_CARRY_DEFAULT. */
#define OAKGPU_MOVE_CARRY_DEFAULT 32
int oakgpu_set_move_carry(oakgpu_ctx *ctx, int below);
/* ... in DRY waves.  With below > 0 a bulk wave whose queue has run dry goes on carrying (at the threshold above) while at least
 * `below` of its lanes play -- and no fewer than a regrouping or tail launch suspends at -- and runs the schedule without carrying
 * below that; a wave flushes before it suspends, so every image is still a completed turn's.  below = 0: a dry wave never carries.
 * Adopter waves never do.  No effect while oakgpu_set_move_carry is 0.  Results never depend on it.  Range checked; also
 * OAKGPU_MOVE_CARRY_DRY at context creation.  Default OAKGPU_MOVE_CARRY_DRY_DEFAULT. */
#define OAKGPU_MOVE_CARRY_DRY_DEFAULT 0
int oakgpu_set_move_carry_dry(oakgpu_ctx *ctx, int below);
/* Lean rollout.  The chance durations are observational state -- the caller's hidden-variable resampling and the leaf network's
 * encoder read them, the engine's transitions never do (tests/test_durations_observational.py).  With on != 0 a group launch (the
 * queue kernel) NONE of whose batches gives a durations_out runs an instantiation that keeps no durations at all: it reads a batch's
 * durations for the prep of a fresh playout only (with prep = 0 the instantiation has no prep code either), parks none with a
 * donated or suspended playout and writes none.  Any prep and any
 * battles_out go with it; one batch with a durations_out and the whole group runs the kernel that keeps them.  Results, step counts,
 * values, battles and the advanced prng are byte for byte the same either way (tests/test_gpu_lean_rollout.py).  on = 0: always the
 * kernel that keeps durations (A / B; also OAKGPU_LEAN_ROLLOUT=0 at context creation).  Default OAKGPU_LEAN_ROLLOUT_DEFAULT.
 * oakgpu_last_launch_lean: 1 if the context's last group launch ran lean, else 0.
 * The sliced search steps (oakgpu_root_steps_*) return aggregates only and run lean the same way: a handle takes the setting when it
 * is created and keeps it for its life (the carried playouts' records are laid out for the one kernel); aggregates, turn-step counts
 * and lane streams are the same either way (tests/test_gpu_lean_root_step.py). */
#define OAKGPU_LEAN_ROLLOUT_DEFAULT 1
int oakgpu_set_lean_rollout(oakgpu_ctx *ctx, int on);
int oakgpu_last_launch_lean(oakgpu_ctx *ctx);
/* Words of that block written by the queue kernel's standstill skip (cleared by every queue launch). */
#define OAKGPU_CTL_FAST_FORWARDED 44 /* playouts whose inert standstill was taken in one go */
#define OAKGPU_CTL_SKIPPED_STEPS 45  /* turn-steps those playouts skipped (they are part of steps_out) */
/* Diagnostic (synchronises the stream): the 64 control words of the last queue launch -- [32] / [33]
 * or [34] / [35] the queue order's two counters (launches take the pairs in turn: each clears the next one's), [40] donations, [41] adoptions, [42] bulk waves that left, [44] / [45] above, [63] error bits (0 = none:
 * 1 a ticket never arrived, 2 an adopter gave up waiting) -- STICKY: no launch clears them; oakgpu_synchronize reports a
 * non-zero word as a failed call and clears it, so the error of any launch since the last synchronize is seen, not only the
 * last launch's. */
int oakgpu_get_queue_counters(oakgpu_ctx *ctx, uint32_t *out64);
/* One engine runs everything in this header: the register-resident one (oak_amd/csrc/gen1_regs.hpp), held to the CPU oracle byte for
 * byte by tests/.  (The LDS-resident engine written first, and the setter that selected it for rollouts, are gone: DESIGN_HISTORY.md.) */
int oakgpu_device_count(void);

/* ---- rollout: replaces MCTS::Search::init_stats_and_rollout (search/mcts.h:448-496) and,
 * with prep != 0, the per-iteration prep of run_root_iteration (mcts.h:250-263:
 * battle.rng = device.uniform_64(); randomize_hidden_variables (search/durations.h:25-97)).
 * Device RNG = the reference's fast_prng (util/random.h:67-133), 8 bytes of state per lane,
 * advanced in place.  Per lane: play uniformly random legal joint choices
 * (c1 = p1_choices[seed % m]; c2 = p2_choices[(seed >> 32) % n]) until the result type is
 * non-zero or max_steps turn-steps were made.
 *   results_out[i] : final pkmn_result byte (type 0 = hit the step cap)
 *   steps_out[i]   : number of pkmn_gen1_battle_update-equivalent turn-steps executed
 *   values_out[i]  : 1 / 0 / 0.5 for win / lose / (tie or capped)  (mcts.h:481-495)
 *   battles_out / durations_out (nullable): final state bytes (parity checks, stepping a resident batch).
 * Every output may alias its input (battles_out == battles, durations_out == durations, results_out ==
 * results_in): lane i only ever reads and writes row i. */
int oakgpu_rollout_dev(oakgpu_ctx *ctx, const uint8_t *battles, const uint8_t *durations,
                       const uint8_t *results_in, uint8_t *prng_state, uint32_t n, uint32_t max_steps,
                       int prep, uint8_t *results_out, uint32_t *steps_out, float *values_out,
                       uint8_t *battles_out, uint8_t *durations_out);
int oakgpu_rollout(oakgpu_ctx *ctx, const uint8_t *battles, const uint8_t *durations,
                   const uint8_t *results_in, uint8_t *prng_state, uint32_t n, uint32_t max_steps, int prep,
                   uint8_t *results_out, uint32_t *steps_out, float *values_out, uint8_t *battles_out,
                   uint8_t *durations_out);

/* Group launch: `count` (<= 64) independent batches drained by ONE launch through one playout queue, so the group has
 * a single tail instead of one per batch (root-parallel MCTS submits its roots' batches together).  Same per-batch
 * contract as oakgpu_rollout_dev (outputs may alias inputs; results never depend on the grouping); batches with
 * n == 0 are skipped.  oakgpu_rollout_dev is the group of one.  Call it for every launch: a group launch must not be replayed
 * from a captured HIP graph (its kernel arguments carry per-launch host state -- the table slot, the adoption tickets' epoch). */
typedef struct {
  const uint8_t *battles, *durations, *results_in;
  uint8_t *prng_state;
  uint32_t n;
  uint8_t *results_out;
  uint32_t *steps_out;
  float *values_out;
  uint8_t *battles_out, *durations_out; /* nullable */
} oakgpu_rollout_batch;
int oakgpu_rollout_group_dev(oakgpu_ctx *ctx, const oakgpu_rollout_batch *batches, uint32_t count, uint32_t max_steps,
                             int prep);
int oakgpu_rollout_group(oakgpu_ctx *ctx, const oakgpu_rollout_batch *batches, uint32_t count, uint32_t max_steps, int prep);
/* Diagnostic (tests): the queue order of oakgpu_set_queue_order alone, at any total, for HOST battles (of `batches` only .battles
 * and .n are read; no batch may be empty): order_out receives sum(n) playout indices -- the `*suspects_out` playouts that a launch
 * hands out first at the front, the others behind them.  Synchronises, and clears the control words like a launch. */
int oakgpu_queue_order(oakgpu_ctx *ctx, const oakgpu_rollout_batch *batches, uint32_t count, uint32_t *order_out, uint32_t *suspects_out);

/* ---- rollouts driven by a caller-supplied draw stream (a SHARED sequential device generator).
 * The reference's benchmark / search drive every playout from ONE std::mt19937 (benchmark.cc:24, search.cc:150), so
 * playout i starts in the generator's output where playout i-1 stopped.  `draws` holds that output: one u64 per
 * device.uniform_64() call (mcts.h:255-257: battle.rng of the root iteration when prep != 0; mcts.h:452: one per
 * turn-step).
 *   oakgpu_mt19937_fill           : std::mt19937{seed} -> uniform_64() values (util/random.h:10-65), host side.
 *   oakgpu_rollout_draws_dev      : lane i plays from draws[offsets[i]] (offsets == NULL: from draws[i]); strides of 0
 *                                   make every lane start from the same root; every output is nullable; used_out[i] =
 *                                   draws consumed, 0xFFFFFFFF if the lane ran off the end of the stream.
 *   oakgpu_rollout_shared_device  : (host pointers) n playouts from ONE root in the sequential order of the reference:
 *                                   offsets resolved on the device by playing a playout from every start offset first.
 *                                   Fails (-1) if the stream is too short.  offsets_out / draws_consumed nullable. */
int oakgpu_mt19937_fill(uint32_t seed, uint64_t skip, uint64_t *out, size_t count);
int oakgpu_rollout_draws_dev(oakgpu_ctx *ctx, const uint8_t *battles, uint32_t battle_stride, const uint8_t *durations,
                             uint32_t durations_stride, const uint8_t *results_in, uint32_t results_stride,
                             const uint64_t *draws, uint32_t n_draws, const uint32_t *offsets, uint32_t n,
                             uint32_t max_steps, int prep, uint8_t *results_out, uint32_t *steps_out, float *values_out,
                             uint8_t *battles_out, uint8_t *durations_out, uint32_t *used_out);
int oakgpu_rollout_shared_device(oakgpu_ctx *ctx, const uint8_t *battle, const uint8_t *durations, uint8_t result,
                                 const uint64_t *draws, uint32_t n_draws, uint32_t n, uint32_t max_steps, int prep,
                                 uint8_t *results_out, uint32_t *steps_out, float *values_out, uint8_t *battles_out,
                                 uint8_t *durations_out, uint32_t *offsets_out, uint64_t *draws_consumed);

/* ---- batched pkmn_gen1_battle_update (call sites mcts.h:278,350,463,479; wrapper
 * libpkmn/pkmn.h:106-139).  In place on battles; durations in/out (chance options);
 * device battles of the _dev forms of this call, oakgpu_choices, oakgpu_init_battles and oakgpu_random_ou_battles: on a 4-byte boundary
 * at least (16-byte aligned battles, as hipMalloc gives them, move in 16-byte pieces, others in dwords);
 * actions (nullable) receives the 16-byte chance-actions key of each update (mcts.h:93-98);
 * overrides (nullable, n x 16) are the calc damage-roll overrides (mcts.h:575-588). */
int oakgpu_update_dev(oakgpu_ctx *ctx, uint8_t *battles, const uint8_t *c1, const uint8_t *c2,
                      uint8_t *durations, uint8_t *actions, const uint8_t *overrides, uint32_t n,
                      uint8_t *results);
int oakgpu_update(oakgpu_ctx *ctx, uint8_t *battles, const uint8_t *c1, const uint8_t *c2, uint8_t *durations,
                  uint8_t *actions, const uint8_t *overrides, uint32_t n, uint8_t *results);

/* ---- batched pkmn_gen1_battle_choices (mcts.h:161-166,337-342; pkmn.h:141-156).
 * requests come from the per-lane result byte (p1: bits 4-5, p2: bits 6-7).
 * out: n x 9 bytes, counts: n bytes. */
int oakgpu_choices_dev(oakgpu_ctx *ctx, const uint8_t *battles, const uint8_t *results, int player,
                       uint8_t *out, uint8_t *counts, uint32_t n);
int oakgpu_choices(oakgpu_ctx *ctx, const uint8_t *battles, const uint8_t *results, int player, uint8_t *out,
                   uint8_t *counts, uint32_t n);

/* ---- PokeEngine::Eval (search/poke-engine-evaluate.h:9-204), batched: scores[i] = evaluate_battle(battle i)
 * (Eval::get_root_score for a batch of one), values[i] = scaled_sigmoid(scores[i] - root_score) = Eval::evaluate.
 * Either output may be null. */
int oakgpu_poke_engine_eval_dev(oakgpu_ctx *ctx, const uint8_t *battles, uint32_t n, float root_score, float *values,
                                float *scores);
int oakgpu_poke_engine_eval(oakgpu_ctx *ctx, const uint8_t *battles, uint32_t n, float root_score, float *values,
                            float *scores);

/* ---- one tree level for a batch of descents (MCTS::Search::run_iteration, search/mcts.h:304-389): apply
 * the joint action of every lane (c1[i] == 0xFF: lane i is finished, leave it untouched), in place, and
 * report result, the 16-byte observation key (pkmn_gen1_battle_options_chance_actions; tree edge key,
 * mcts.h:93-98,359) and BOTH players' legal choices in the new state (n x 9 + n counts each; counts are 0
 * for terminal results).  rolls in {1, 2, 3, 20, 39}: damage-roll clamping of battle_options_set
 * (mcts.h:569-604; 39 = off), override bytes derived from the last two bytes of battle.rng.  The level runs on the register-resident engine
 * (k_tree_step_staged): 16-byte aligned battles move through it in 16-byte pieces, battles on a 4-byte boundary in dwords; both forms
 * are held to the oracle byte for byte (tests/tree_step_check.py, test_gpu_move_coverage.py). */
int oakgpu_tree_step_dev(oakgpu_ctx *ctx, uint8_t *battles, uint8_t *durations, uint8_t *results, const uint8_t *c1,
                         const uint8_t *c2, uint32_t n, uint32_t rolls, uint8_t *actions, uint8_t *p1_choices,
                         uint8_t *p1_counts, uint8_t *p2_choices, uint8_t *p2_counts);

/* ---- tree search with batched leaves: MCTS::Search::run (search/mcts.h:154-247) with a Node heap
 * (mcts.h:95-105), joint UCB / PUCB bandits (search/bandit/ucb.h:17-66, pucb.h:17-75) and the Monte-Carlo or
 * network evaluator.  `batch` descents walk the host-side tree together, one oakgpu_tree_step_dev launch per
 * level, all battle states resident on the device; lanes of a batch repel each other with a virtual loss.
 * The root matrices come back as in MCTS::Output (mcts.h:68-90), with process_output's exact Nash solve
 * (mcts.h:620-659) in nash_value / p1_nash / p2_nash. */
typedef struct {
  uint64_t iterations;   /* root iterations (mcts.h:231-235, integer budget) */
  uint32_t batch;        /* descents in flight (GPU lanes); 1 reproduces the reference's one-at-a-time order */
  float ucb_c;           /* Bandit::Params.c (UCB, PUCB, UCB1) or gamma (Exp3, PExp3) */
  int32_t bandit;        /* 0: UCB (bandit/ucb.h), 1: PUCB (pucb.h), 2: UCB1 (ucb1.h), 3: Exp3 (exp3.h), 4: PExp3 (pexp3.h);
                          * PUCB / PExp3 take priors from the policy heads and need eval = 1 */
  int32_t eval;          /* 0: MCTS::MonteCarlo rollouts (mcts.h:448-496), 1: network value (network.h:72-123),
                          * 2: PokeEngine::Eval (poke-engine-evaluate.h:186-202; root score taken at the root) */
  uint32_t max_depth;    /* descent depth at which a node is evaluated even if already expanded (0 = 100) */
  uint32_t root_rolls;   /* SearchOptions.root_rolls / other_rolls (mcts.h:107-131): 1, 2, 3, 20 or 39 (= no clamping) */
  uint32_t other_rolls;
  uint64_t seed;         /* seeds the per-lane fast_prng streams (root resampling draws + rollouts) */
  /* MatrixUCBParams (mcts.h:107-113, 263-302, 498-566): once `mucb_delay` iterations are done the ROOT joint action is no
   * longer picked by the bandits but sampled from the Nash strategies of the optimistic / pessimistic UCB matrices
   * (cells below `mucb_minimum` visits are forced first).  The matrices are re-solved once per batch (the reference's
   * `interval` = batch here).  matrix_ucb = 0 disables it. */
  int32_t matrix_ucb;
  uint32_t mucb_delay;
  uint32_t mucb_minimum;
  float mucb_c;
  float exp3_alpha;      /* Exp3 / PExp3 uniform mixing (search.cc:268-286); negative (OAKGPU_EXP3_ALPHA_DEFAULT) = the reference's
                          * default 0.05 (its value when the agent string has no third field); 0 is honoured as 0, as the
                          * reference honours it -- so a ZERO-INITIALISED struct asks for no mixing at all: start from
                          * OAKGPU_SEARCH_PARAMS_INIT (or set this field) when Exp3 / PExp3 is used.  With alpha = 0 an arm's
                          * probability can underflow to 0; the importance-weighted update then divides by the smallest
                          * normal float instead (the reference would divide by zero) */
  uint64_t duration_us;  /* time budget (search.cc:300-306): when non-zero, `iterations` is ignored and whole batches are
                          * started until this much time has elapsed; output.iterations tells how many ran */
} oakgpu_search_params;
/* Return code of oakgpu_search_heap / oakgpu_search_agent_heap (every other failure is -1 or a HIP error code): the heap's root was
 * initialised with other action counts than the position passed in -- Heap::update was not called with the move that was played, or
 * (--keep-node self-play) the kept child was expanded under other resampled hidden variables than the game really reached. */
#define OAKGPU_E_ROOT_MISMATCH (-2)
#define OAKGPU_EXP3_ALPHA_DEFAULT (-1.0f)
/* the reference's defaults where a zero is not one: UCB c = 2 is the caller's business (agent strings carry it), root / other
 * rolls = default_search {3, 1} (mcts.h:131), Exp3 mixing = the default of an absent field */
#define OAKGPU_SEARCH_PARAMS_INIT {0, 0, 0.0f, 0, 0, 0, 3, 1, 0, 0, 0, 0, 0.0f, OAKGPU_EXP3_ALPHA_DEFAULT, 0}
typedef struct {
  uint8_t m, n;                 /* legal choices per side at the root */
  uint8_t p1_choices[9], p2_choices[9];
  uint64_t visit_matrix[81];    /* [i * 9 + j] */
  double value_matrix[81];      /* cumulative P1 values */
  uint64_t iterations;
  double empirical_value, initial_value;
  double p1_empirical[9], p2_empirical[9];
  uint64_t nodes, total_depth;
  double duration_us;
  /* MCTS::Search::process_output (mcts.h:620-659): equilibrium of the empirical root matrix (x 256 as integers, solved
   * exactly, see oakgpu_solve_matrix) */
  double nash_value, p1_nash[9], p2_nash[9];
  /* Output::Side::logit / prior (mcts.h:70-77): the policy heads' logits of the root's legal choices and their softmax,
   * filled when a contextual bandit (PUCB / PExp3) initialises a FRESH root (mcts.h:196-209); otherwise as passed in */
  double p1_logit[9], p2_logit[9], p1_prior[9], p2_prior[9];
} oakgpu_search_output;
/* LRSNash::solve_fast as the reference calls it (mcts.h:643-649, pyoak solve_matrix pyoak.cc:394-426): exact Nash
 * equilibrium of the m x n (<= 9 x 9) zero-sum game whose ROW player maximises the integer payoffs[i * n + j]
 * (|payoff| <= 2^20; the reference passes value * discretize_factor).  No floating point in the solve (integer-pivoting
 * simplex on 512-bit integers; the reference's lrsnash + GMP is absent).  p1[m], p2[n] = equilibrium strategies, *value =
 * game value / discretize_factor.  Host code: no GPU involved. */
int oakgpu_solve_matrix(const int32_t *payoffs, int m, int n, int discretize_factor, double *p1, double *p2, double *value);
/* The same solve on the device (nashdev.hip), bit for bit oakgpu_solve_matrix's: the integer simplex is the same text (nash.hpp) on
 * integers of 4 or 8 limbs (chosen per matrix from its largest shifted entry by Hadamard's bound), the final roundings are the host's
 * x87 long double operations restated in integer arithmetic.
 * oakgpu_nash_solve_dev: device pointers, on the context's stream, nothing is synchronised.  pay = rows x 82 int32 as the forest loops'
 *   payoff kernel writes them (row-major m x n payoffs, m | n << 8 at index 81); nash = rows x 9 p1 strategies, rows x 9 p2 strategies,
 *   rows values / 256.0.  A row the solver refuses (m or n outside 1 ... 9, a payoff beyond +-2^20) comes back as zeros.
 * oakgpu_solve_matrices: host arrays; matrix k = the m[k] x n[k] row-major ints at payoffs + 81 k, its results at p1 + 9 k, p2 + 9 k (the
 *   entries past m[k] / n[k] are 0) and value[k].  Entry k is oakgpu_solve_matrix of matrix k; what that call refuses fails the whole
 *   call before anything is launched, naming the lowest such k. */
int oakgpu_nash_solve_dev(oakgpu_ctx *ctx, const int32_t *pay, uint32_t rows, double *nash);
int oakgpu_solve_matrices(oakgpu_ctx *ctx, const int32_t *payoffs, const int32_t *m, const int32_t *n, uint32_t count, int discretize_factor,
                          double *p1, double *p2, double *value);
/* Host-only diagnostics of the device solver's text (no GPU).  _soft_host: matrices laid out as for oakgpu_solve_matrices, solved by
 *   solve_soft at `limbs` = 4, 8 or 0 (the selector's choice); value in payoff units; width[k] = the selector's choice, 0 for a refused
 *   matrix (whose results are zeros).  _round_host: num / den are count x 8 64-bit limbs (two's complement, least significant first);
 *   hard[k] = (double)(num.to_ld() / den.to_ld() - (long double)shift[k]) in x87 arithmetic, soft[k] = the integer restatement of it.
 *   _width4_max_entry: the largest shifted entry the 4-limb width takes. */
int oakgpu_nash_soft_host(const int32_t *payoffs, const int32_t *m, const int32_t *n, uint32_t count, int limbs, double *p1, double *p2, double *value,
                          uint8_t *width);
int oakgpu_nash_round_host(const uint64_t *num, const uint64_t *den, const int64_t *shift, uint32_t count, double *hard, double *soft);
int oakgpu_nash_width4_max_entry(void);
/* RuntimeSearch::run (util/search.h:17-66, search.cc:150-313): the search configured by the Agent's strings, as the
 * reference's binaries and pyoak.search configure it.  budget "4096" | "100ms" | "8s"; bandit "ucb-1.0" | "ucb1-2.0" |
 * "pucb-1.5" | "exp3-<gamma>[-<alpha>]" | "pexp3-..."; eval "" / "mc" | "fp" | <.battle.net path> (loaded once per device
 * and kept, like Agent::network_ptr); matrix_ucb "" | "<delay>-<interval>-<minimum>-<c>".  Unparsable strings fail with
 * the reference's error texts (where it throws std::runtime_error); `table` agents are refused (transposition-table heaps are
 * not built).  `discrete` loads the <.battle.net> through oakgpu_net_load_discrete (the int8 main net, kept apart from the fp32
 * network of the same path).  batch = descents in flight, 0 = chosen from the budget. */
typedef struct {
  const char *budget, *bandit, *eval, *matrix_ucb;
  int discrete, table;
} oakgpu_agent;
int oakgpu_search_agent(oakgpu_ctx *ctx, const uint8_t *battle, const uint8_t *durations, uint8_t result, const oakgpu_agent *agent,
                        uint32_t batch, uint64_t seed, oakgpu_search_output *out);
void oakgpu_agent_networks_clear(oakgpu_ctx *ctx);
/* The parser of oakgpu_search_agent* alone: the Agent's strings -> *params (batch as above, seed as given) and *net (the agent's
 * network, loaded once per device and kept; NULL for "mc" / "fp"), with the same error texts.  For callers that run the search
 * themselves, e.g. the forest search below. */
int oakgpu_agent_params(oakgpu_ctx *ctx, const oakgpu_agent *agent, uint32_t batch, uint64_t seed, oakgpu_search_params *params,
                        oakgpu_net **net);

/* Diagnostic (no GPU involved): ONE player's bandit of the search above replayed for `steps` rounds -- select, then
 * update with values[t] -- so its arithmetic can be compared with the reference's bandit headers.  kind as in
 * oakgpu_search_params.bandit; c = Params.c (UCB / PUCB / UCB1) or gamma (Exp3 / PExp3); logits (k floats): PUCB /
 * PExp3 priors; uniforms: the device.uniform() draw of each sampled selection (Exp3 / PExp3, k > 1).  Outputs: selected
 * index (and probability) per round, final stats_out[0..8] = scores / gains, [9..17] = priors, visits_out[0..8]. */
int oakgpu_bandit_replay(int kind, float c, float alpha, uint32_t k, const float *logits, uint32_t steps,
                         const double *uniforms, const float *values, uint8_t *index_out, float *prob_out,
                         float *stats_out, uint32_t *visits_out);
/* Diagnostic (no GPU involved): `count` select + visit rounds of one bandit from the given state (scores[9], priors[9],
 * visits[9]), once through the register-resident run the batched search uses at the root and once as the plain loop: the two
 * index sequences (run_out, loop_out: count bytes each) and final visit counts must be identical. */
int oakgpu_bandit_select_run(int kind, float c, float alpha, uint32_t k, const float *scores, const float *priors,
                             const uint32_t *visits, uint32_t count, uint8_t *run_out, uint8_t *loop_out, uint32_t *visits_run,
                             uint32_t *visits_loop);
int oakgpu_search(oakgpu_ctx *ctx, oakgpu_net *net /* nullable for eval = 0 */, const uint8_t *battle /* 384 */,
                  const uint8_t *durations /* 8 */, uint8_t result, const oakgpu_search_params *params,
                  oakgpu_search_output *out);
/* Diagnostic (synchronises the search's stream): the continuing fast_prng state of lane 0 of the first batch slot of the LAST search on
 * this context -- with batch = 1 the one stream that search drew from (what a tree of the forest search below must end on). */
int oakgpu_search_stream(oakgpu_ctx *ctx, uint64_t *state);

/* ---- RuntimeSearch::Heap (util/search.h:17-32, search.cc:17-58) and the resumable form of Search::run.
 * A heap keeps the tree of a search -- every node's bandit statistics -- between searches:
 *   oakgpu_heap_empty   = Heap::empty(): 1 until a search has used the heap (std::monostate);
 *   oakgpu_heap_update  = Heap::update(i, j, obs) (search.cc:27-52) after the joint action (p1 index i, p2 index j) was PLAYED
 *                         and produced the 16-byte observation `obs` (pkmn_gen1_battle_options_chance_actions): the child
 *                         becomes the root with its whole subtree, the rest is dropped; returns 1.  Returns 0 -- and
 *                         leaves an uninitialised root, like `node = {}` -- when the searches never took that edge, when
 *                         the root was never initialised, or when the heap is empty;
 *   a heap holds one bandit type (the first search fixes it, like the variant, search.cc:205-213): searching it with another
 *   fails with "RuntimeSearch: Bad Heap access. Expecting ...".
 * oakgpu_search_heap = MCTS::Search::run(device, budget, params, heap, eval, input, output) (mcts.h:153-248):
 *   heap      nullable: NULL = a fresh tree for this call (oakgpu_search);
 *   previous  nullable: MCTS::Output is passed BY VALUE and added to -- visit / value matrices, `iterations` and `duration`
 *             accumulate (:231-247), process_output (:620-659) then runs over the sums; MatrixUCB's delay counts
 *             the accumulated iterations (:270).  `previous` and `out` may be the same object.
 *   params->iterations == 0 with duration_us == 0 is legal here: no iteration runs and the output carries the fresh root's
 *   initial_value / logits / priors (what the reference's cpp_inference reads, pyoak.cc:331-392); the empirical fields are
 *   then 0 / 0 as in the reference.  A time budget always runs at least one batch (mcts.h:219-226), and its clock -- like
 *   `duration_us` in the output -- covers the iteration loop only, not the set-up. */
typedef struct oakgpu_heap oakgpu_heap;
int oakgpu_heap_create(oakgpu_heap **out);
void oakgpu_heap_destroy(oakgpu_heap *heap);
int oakgpu_heap_empty(const oakgpu_heap *heap);
void oakgpu_heap_clear(oakgpu_heap *heap);                       /* back to std::monostate */
int oakgpu_heap_kind(const oakgpu_heap *heap);                   /* -1 empty, else oakgpu_search_params.bandit of its nodes */
uint64_t oakgpu_heap_nodes(const oakgpu_heap *heap);
int oakgpu_heap_update(oakgpu_heap *heap, uint8_t i, uint8_t j, const uint8_t *obs16);
/* diagnostics of the host tree's sharding (tests): edges whose child sits in another table's arena (0 in a consistent tree);
 * a host-only self-test (no GPU) that grows a random tree with the search's own threaded resolve phase, promotes a child,
 * checks the shards and grows on: 0 = every check held; out = {nodes before, nodes kept, nodes at the end, shard violations} */
uint64_t oakgpu_heap_check_shards(const oakgpu_heap *heap);
int oakgpu_heap_selftest(uint32_t rounds, uint32_t lanes, uint64_t seed, int threads, uint64_t out[4]);
/* the root's bandit of one player (0 / 1): scores[9] (Exp3: gains), priors[9], visits[9], k (0 = root not initialised) */
int oakgpu_heap_root_stats(const oakgpu_heap *heap, int player, float *scores, float *priors, uint32_t *visits, uint8_t *k);
/* the same view of the child that oakgpu_heap_update(i, j, obs16) would promote; k = 0: no such (initialised) child */
int oakgpu_heap_child_stats(const oakgpu_heap *heap, uint8_t i, uint8_t j, const uint8_t *obs16, int player, float *scores,
                            float *priors, uint32_t *visits, uint8_t *k);
int oakgpu_search_heap(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_heap *heap, const uint8_t *battle, const uint8_t *durations,
                       uint8_t result, const oakgpu_search_params *params, const oakgpu_search_output *previous,
                       oakgpu_search_output *out);
/* RuntimeSearch::run(device, input, heap, agent, output) (util/search.h:66): oakgpu_search_agent with the heap and the
 * output to resume. */
/* n independent searches at once on ONE GPU: one tree per root (the positions of n self-play games; the reference runs them as N worker
 * threads that never wait for each other, generate.cc:527-536), search i on ctxs[i] -- every search needs a context of its own (its
 * stream and batch slots) and, when heaps != NULL, a heap of its own -- with battles n x 384, durations n x 8, results n, params n
 * entries (seeds!), outs n entries.  Each search is exactly oakgpu_search_heap(ctxs[i], net, heaps[i], ..., NULL, &outs[i]): same output,
 * same heap, whatever runs beside it.  threads_per_search: host threads of each tree walk (1, 2, 4, 8, 16); 0 = the usable cores shared
 * evenly (OAKGPU_SEARCH_CORES overrides the affinity mask's count, e.g. under a cgroup quota). */
int oakgpu_search_many(oakgpu_ctx *const *ctxs, oakgpu_net *net, oakgpu_heap *const *heaps, const uint8_t *battles, const uint8_t *durations,
                       const uint8_t *results, const oakgpu_search_params *params, uint32_t n, int threads_per_search,
                       oakgpu_search_output *outs);
int oakgpu_search_agent_heap(oakgpu_ctx *ctx, oakgpu_heap *heap, const uint8_t *battle, const uint8_t *durations, uint8_t result,
                             const oakgpu_agent *agent, uint32_t batch, uint64_t seed, const oakgpu_search_output *previous,
                             oakgpu_search_output *out);

/* ---- the forest search: n independent searches at once, ONE LANE PER TREE, every tree resident on the device (forest.hip).
 * Where oakgpu_search parallelises inside one tree (a batch of descents, virtual loss, a host tree), this parallelises across trees:
 * each tree runs the reference's strictly sequential iteration (mcts.h:250-447, no virtual loss) and the n trees advance in lockstep,
 * so every kernel of an iteration -- root prep, tree step, leaf evaluation, back-up -- runs over n rows.  The form a game loop needs:
 * thousands of positions, one small-budget search each.
 *   Semantics.  Tree g of a call is the search oakgpu_search(ctx, net, battles + 384 g, durations + 8 g, results[g], {params with seed =
 *   seeds[g], batch = 1}) runs, iteration for iteration; per iteration, in order: (1) root prep, oakgpu_rollout_dev(max_steps 0, prep 1)
 *   on the tree's own fast_prng stream, whose state starts as the first splitmix64 output of seeds[g], | 1; (2) Bandit select, then visit,
 *   for both players; (3) oakgpu_tree_step_dev with root_rolls at depth 0 and other_rolls below; (4) the walk goes on while the edge is
 *   not terminal (a terminal edge ends it with the value of the result byte) and the child of (parent, i, j, 16-byte observation) --
 *   created when new -- is initialised and above max_depth; (5) else the leaf is evaluated as oakgpu_search evaluates it, over ALL n
 *   rows, finished ones included, so every stream advances as in the single search; (6) init (+ priors from the logits) at a node's first
 *   evaluation; (7) update along the path; (8) root matrices: ++visits, value += the P1 value, in double.
 *   Arithmetic.  The bandits are bandit.hpp's, compiled for the device without contraction; UCB trees equal the host search bit for bit in
 *   every output.  PUCB priors use the device's expf where the host search uses the host's: a PUCB tree may differ from the host search and
 *   is held to its own trace instead (tests/forest_ref.py).
 *   Supported: bandit 0 (UCB) and 1 (PUCB, a forest created `contextual`, eval = 1); eval 0 / 1 / 2; integer budgets; fp32 and discrete
 *   network handles.  Refused by name before any launch (oakgpu_forest_check): time budgets, matrix_ucb, UCB1 / Exp3 / PExp3,
 *   iterations == 0 or > max_iterations, n > max_trees, a terminal root, a trace with trace_levels < max_depth.
 *   Capacity.  A tree owns an arena of max_iterations + 1 nodes (an iteration creates at most one) and an open-addressing edge table of
 *   at least twice as many slots; nothing grows during a call.  A full arena or table (impossible within the limits above) sets a sticky
 *   error word: the lane stops, the call returns -1.
 *   Outputs (oakgpu_forest_outputs: device arrays, all required): per tree m, n and the choice lists, the root matrices, iterations,
 *   nodes, total_depth, initial_value and root logits / priors (PUCB; else 0), and the tree's continuing fast_prng state.
 *   Trace (nullable; tests): n x iterations records, record (g, t) at byte (g * iterations + t) * OAKGPU_FOREST_TRACE_BYTES(trace_levels):
 *   an oakgpu_forest_trace_head, then trace_levels oakgpu_forest_trace_level entries of which the first `levels` are meaningful (the rest 0).
 *   Node ids count a tree's nodes in creation order, the root is 0.
 * The calls: _create allocates the arenas on the context's device (the context must outlive the forest; all work runs on its stream);
 * _search_dev takes device arrays and returns with the search complete (the host reads a 4-byte live count per tree level);
 * _search takes host arrays, fills one oakgpu_search_output per tree as oakgpu_search does (process_output's empirical fields; the exact
 * Nash solve only with solve_nash, else those fields are 0 -- 1: one host solve per tree, 2: one oakgpu_nash_solve_dev over all n trees,
 * the same bits; duration_us = the whole call's), streams_out (nullable) n x u64, trace
 * (nullable) a host buffer; _nodes reads `count` node records of one tree of the LAST call, from node `first`, into host memory;
 * _check is the host-only validation both searches run first (results: host bytes, nullable = not checked). */
typedef struct oakgpu_forest oakgpu_forest;
typedef struct {
  uint8_t *m, *n;                       /* n trees each */
  uint8_t *p1_choices, *p2_choices;     /* n x 9 */
  uint64_t *visit_matrix;               /* n x 81, [i * 9 + j] */
  double *value_matrix;                 /* n x 81 */
  uint64_t *iterations, *nodes, *total_depth;
  double *initial_value;
  double *p1_logit, *p2_logit, *p1_prior, *p2_prior; /* n x 9 */
  uint64_t *stream;                     /* n: fast_prng state after the last iteration */
} oakgpu_forest_outputs;
typedef struct { float scores[9], priors[9]; uint32_t visits[9]; uint8_t k, pad[3]; } oakgpu_forest_bandit; /* k = 0: not initialised */
typedef struct { oakgpu_forest_bandit p1, p2; } oakgpu_forest_node;
typedef struct {
  uint32_t levels;        /* tree levels walked = joint actions applied */
  uint32_t leaf;          /* node the walk stopped at to evaluate; OAKGPU_FOREST_NO_NODE after a terminal edge */
  uint8_t initialised;    /* 1: the leaf was initialised in this iteration */
  uint8_t result_type;    /* result byte & 15 of the last edge: 0 = not terminal */
  uint8_t pad[2];
  float value;            /* the P1 value backed up */
  float logits[18];       /* PUCB, initialised = 1: the leaf's p1 / p2 logits (9 each); else 0 */
} oakgpu_forest_trace_head;
typedef struct { uint32_t node; uint8_t i, j, pad[2]; } oakgpu_forest_trace_level;
#define OAKGPU_FOREST_NO_NODE 0xFFFFFFFFu
#define OAKGPU_FOREST_TRACE_BYTES(levels) (sizeof(oakgpu_forest_trace_head) + (size_t)(levels) * sizeof(oakgpu_forest_trace_level))
int oakgpu_forest_create(oakgpu_ctx *ctx, uint32_t max_trees, uint32_t max_iterations, int contextual, oakgpu_forest **out);
void oakgpu_forest_destroy(oakgpu_ctx *ctx, oakgpu_forest *forest); /* waits for ctx's stream; ctx == NULL (the context is gone): for the device */
int oakgpu_forest_check(uint32_t max_trees, uint32_t max_iterations, int contextual, const oakgpu_search_params *params, int has_net,
                        uint32_t n, const uint8_t *results, int has_trace, uint32_t trace_levels);
int oakgpu_forest_search_dev(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_search_params *params, const uint8_t *battles,
                             const uint8_t *durations, const uint8_t *results, const uint64_t *seeds, uint32_t n,
                             const oakgpu_forest_outputs *dev_out, void *trace, uint32_t trace_levels);
int oakgpu_forest_search(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_search_params *params, const uint8_t *battles,
                         const uint8_t *durations, const uint8_t *results, const uint64_t *seeds, uint32_t n, oakgpu_search_output *out,
                         int solve_nash, uint64_t *streams_out, void *trace, uint32_t trace_levels);
int oakgpu_forest_nodes(oakgpu_forest *forest, uint32_t tree, uint32_t first, uint32_t count, oakgpu_forest_node *out);
/* Diagnostic: the schedule of the forest's last call -- iterations run, tree levels stepped (= tree-step launches), kernel launches
 * made (prep, steps, level kernels, evaluations, back-ups; an evaluation counts as one), host reads of the live count. */
int oakgpu_forest_last_stats(const oakgpu_forest *forest, uint64_t out[4]);
/* ---- per-tree budgets.  The four _budgets calls take their namesakes' arguments plus budgets: n x u32 (device memory for _dev, host
 * memory otherwise) in front of n.  Tree g runs exactly budgets[g] iterations, 1 <= budgets[g] <= params->iterations <= max_iterations;
 * params->iterations sizes the trace, the loop runs max(budgets) iterations.
 *   Contract.  Every output of tree g -- m, n, choices, both root matrices, iterations, nodes, total_depth, initial value, logits, priors,
 *   the continuing stream -- and every node of it is bit for bit what the call without budgets gives that tree with iterations =
 *   budgets[g] and the same seed: UCB and PUCB, all three evaluators, plain and kept forests.  Trace records (g, t >= budgets[g]) are
 *   not written.  A tree whose budget is spent is inert for the rest of the call (a state of its own, not the error lane's): it selects
 *   and visits nothing, is not counted live, touches neither its root matrices nor its trace, and its stream is the one it had after its
 *   last iteration, whatever later launches over its row draw.
 *   Rows.  Iteration t launches root prep, the level kernels, the tree step, the evaluator and the back-up over the rows [0, n_t) only, n_t
 *   = 1 + max{g : budgets[g] > t}: with budgets non-increasing in row order no launch covers a finished tree; any other order costs the
 *   saving and nothing else.  oakgpu_forest_last_rows: out[0] = tree-iterations launched (the sum of the n_t), out[1] = tree-iterations
 *   run (the sum of the budgets) of the forest's last search; both n * iterations after a call without budgets.
 *   Refused by name before any launch, naming the lowest offending tree: a budget of 0, a budget above params->iterations
 *   (oakgpu_forest_budgets_check, host only).  _dev copies the budgets to the host once, with the result bytes. */
int oakgpu_forest_budgets_check(const uint32_t *budgets, uint32_t n, uint64_t iterations);
int oakgpu_forest_search_budgets_dev(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_search_params *params, const uint8_t *battles,
                                     const uint8_t *durations, const uint8_t *results, const uint64_t *seeds, const uint32_t *budgets, uint32_t n,
                                     const oakgpu_forest_outputs *dev_out, void *trace, uint32_t trace_levels);
int oakgpu_forest_search_budgets(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_search_params *params, const uint8_t *battles,
                                 const uint8_t *durations, const uint8_t *results, const uint64_t *seeds, const uint32_t *budgets, uint32_t n,
                                 oakgpu_search_output *out, int solve_nash, uint64_t *streams_out, void *trace, uint32_t trace_levels);
int oakgpu_forest_search_budgets_kept_dev(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_search_params *params, const uint8_t *battles,
                                          const uint8_t *durations, const uint8_t *results, const uint64_t *seeds, const uint32_t *budgets, uint32_t n,
                                          const oakgpu_forest_outputs *dev_out, void *trace, uint32_t trace_levels);
int oakgpu_forest_search_budgets_kept(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_search_params *params, const uint8_t *battles,
                                      const uint8_t *durations, const uint8_t *results, const uint64_t *seeds, const uint32_t *budgets, uint32_t n,
                                      oakgpu_search_output *out, int solve_nash, uint64_t *streams_out, void *trace, uint32_t trace_levels);
int oakgpu_forest_last_rows(const oakgpu_forest *forest, uint64_t out[2]);

/* ---- kept forests: a tree goes on into the next turn (generate's --keep-node: generate.cc:324-333, Heap::update in search.cc:27-52).
 * oakgpu_forest_create_kept makes a forest whose trees hold keep_arena nodes each (>= max_iterations + 1; 0 = 4 * max_iterations + 1) and
 * whose node arenas and edge tables exist TWICE, front and back; the slot count follows from keep_arena by the plain forest's rule (the
 * power of two >= max(16, 2 * keep_arena)).  Device memory per tree, beside the per-tree rows every forest has:
 *     2 * (keep_arena * 224 + slots * 32) bytes           (oakgpu_forest_kept_tree_bytes; 0 for refused arguments)
 *   plus 4 * keep_arena for the advance's map.  A failed allocation names the bytes asked for.  Such a forest serves every call of a plain
 *   one unchanged; a plain forest answers the calls below with a refusal that says it was created without keep.
 * oakgpu_forest_advance_dev(forest, i, j, obs, src_tree, n_new, kept_out), all device pointers (src_tree nullable = the same row): new
 *   tree t continues tree src_tree[t] of the last call along the played cell (i[t], j[t]) and the update's 16-byte observation obs + 16 t
 *   (oakgpu_update_dev's `actions`) -- ONE launch, one wave per new tree, that re-roots the tree and moves it to its new row; it reads the
 *   front copy, writes the back copy, and the two swap.  The rule per tree is oakgpu_heap_update's: a source that was never searched or
 *   whose root was never initialised, or a cell / observation no iteration took: nothing is kept, kept_out[t] = 0, the new tree is empty
 *   with an uninitialised root.  Otherwise the child becomes node 0 and its whole subtree is kept, bandits byte for byte, node ids still
 *   in creation order, kept_out[t] = 1 -- also when the child itself is uninitialised: the next search then initialises it, priors
 *   included.  The tree's fast_prng word stays in its old row: every search reseeds it.  src_tree values need not be distinct.
 *   Capacity: a kept subtree that leaves fewer than max_iterations free nodes (kept + max_iterations > keep_arena) is DROPPED to an empty
 *   tree, kept_out[t] = 0, and counted (oakgpu_forest_keep_stats).  This is the one place where the device departs from the host's
 *   oakgpu_heap_update, whose heap is unbounded; with the default keep_arena it takes a subtree of more than 3 * max_iterations nodes.
 * oakgpu_forest_search_kept_dev / _search_kept take oakgpu_forest_search_dev's / _search's arguments and go on in the trees the forest
 *   holds (after an advance, or after an earlier search), as oakgpu_search_heap does on a heap (mcts.h:185-212): an initialised root whose
 *   choice counts are the position's is left alone with all its nodes -- initial_value, root logits and priors of the outputs are then 0, no
 *   root inference having run, so policy mode `p` sees a zero prior as in the reference; an uninitialised root (also: a tree beyond those
 *   the last advance wrote) starts as in oakgpu_forest_search_dev; an initialised root with OTHER counts (OAKGPU_E_ROOT_MISMATCH on the
 *   host) has its tree cleared and starts afresh, flagged in a per-tree byte (oakgpu_forest_mismatch: the last kept search's n bytes, to
 *   host or device memory).  `iterations`, the root matrices and total_depth are this call's alone; `nodes` counts the kept ones too.
 * oakgpu_forest_keep_stats: out = { keep_arena, slots per tree, advance launches, trees dropped } since the forest was made. */
#define OAKGPU_FOREST_KEPT 2 /* or-ed into `contextual` of oakgpu_forest_selfplay_check: the limits are a kept forest's */
int oakgpu_forest_create_kept(oakgpu_ctx *ctx, uint32_t max_trees, uint32_t max_iterations, int contextual, uint32_t keep_arena, oakgpu_forest **out);
int oakgpu_forest_create_kept_check(uint32_t max_trees, uint32_t max_iterations, uint32_t keep_arena); /* host only */
uint64_t oakgpu_forest_kept_tree_bytes(uint32_t max_iterations, uint32_t keep_arena);
int oakgpu_forest_advance_dev(oakgpu_forest *forest, const uint8_t *i, const uint8_t *j, const uint8_t *obs, const uint32_t *src_tree, uint32_t n_new,
                              uint8_t *kept_out);
int oakgpu_forest_advance(oakgpu_forest *forest, const uint8_t *i, const uint8_t *j, const uint8_t *obs, const uint32_t *src_tree, uint32_t n_new,
                          uint8_t *kept_out); /* host arrays */
int oakgpu_forest_search_kept_dev(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_search_params *params, const uint8_t *battles,
                                  const uint8_t *durations, const uint8_t *results, const uint64_t *seeds, uint32_t n,
                                  const oakgpu_forest_outputs *dev_out, void *trace, uint32_t trace_levels);
int oakgpu_forest_search_kept(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_search_params *params, const uint8_t *battles,
                              const uint8_t *durations, const uint8_t *results, const uint64_t *seeds, uint32_t n, oakgpu_search_output *out,
                              int solve_nash, uint64_t *streams_out, void *trace, uint32_t trace_levels);
int oakgpu_forest_keep_stats(oakgpu_forest *forest, uint64_t out[4]);
int oakgpu_forest_mismatch(oakgpu_forest *forest, uint8_t *out, uint32_t n, int to_device);
/* the node counts of the first n trees the forest's last call (a search or an advance) left, to host or device memory; any forest */
int oakgpu_forest_node_counts(oakgpu_forest *forest, uint32_t *out, uint32_t n, int to_device);

/* ---- the path's one exchange step: per-root pre-reduction on the device + RCCL all-gather over xGMI.
 * Root-parallel MCTS shards its roots contiguously over the GPUs of a node; each rank reduces its playouts' leaf values to
 * one mean per root (oakgpu_segment_mean_dev: out[s] = mean(values[s * per_segment .. (s + 1) * per_segment))) and ONE
 * ncclAllGather of `count` floats per rank (oakgpu_all_gather_dev, on the context's stream) gives every rank all means:
 * recv = world x count floats, rank-major.  One process per GPU: rank 0 makes the 128-byte id (oakgpu_comm_unique_id),
 * hands it to the others out of band, and every rank calls oakgpu_comm_create.  RCCL is bound at run time (dlopen);
 * without it these calls fail with a message.  The reference has no collective: its playouts are unrelated threads
 * (cpp/src/generate.cc:527-536). */
typedef struct oakgpu_comm oakgpu_comm;
int oakgpu_segment_mean_dev(oakgpu_ctx *ctx, const float *values, uint32_t segments, uint32_t per_segment, float *out);
int oakgpu_comm_unique_id(uint8_t *id128);
int oakgpu_comm_create(oakgpu_ctx *ctx, const uint8_t *id128, int rank, int world, oakgpu_comm **out);
void oakgpu_comm_destroy(oakgpu_comm *comm);
int oakgpu_all_gather_dev(oakgpu_ctx *ctx, oakgpu_comm *comm, const float *send, float *recv, size_t count);

/* ---- root-parallel search steps that do not wait for their longest playout (BASELINE configs[3]).
 * One search step of root-parallel MCTS = `reps` fresh playouts per root (run_root_iteration's prep, mcts.h:250-263, then the
 * rollout loop of mcts.h:448-496) -> one aggregate per root.  The reference's workers never wait for each other
 * (generate.cc:527-536); a step here does not wait for its stragglers either: every launch advances each playout in flight by at
 * most `slice` turn-steps (a power of two; 0 = run to terminal inside the step, the plain rollout's behaviour).  A playout of
 * `len` turn-steps started in step k is credited to step k + (len - 1) / slice (len = 0: step k) -- a function of its own length,
 * not of the schedule -- and travels between launches as a bit-exact state image on a carry list owned by this object.  Values
 * never change, only the step they are credited to.
 *   Streams: lane_prng (n_roots * reps x 8 bytes, device) holds one fast_prng stream per (root, replica), advanced by ONE
 * uniform_64 per step; that draw is the 8-byte state of the fresh playout's own stream (all-zero -> s1 = 1), which supplies
 * battle.rng for the prep and then the choices.
 *   report (device, n_roots + 2 u64, written by the launch): [r] = playouts credited to this step for root r: count | (sum of
 * 2 x value) << 32 -- integers, so independent of the order playouts finish in; [n_roots] = turn-steps this launch executed;
 * [n_roots + 1] = playouts carried into the next step | error word << 32 (bit 0: the carry list overflowed -- playouts were
 * lost; sticky).  fresh = 0 launches a DRAIN step: no new playouts, the carried ones advance one more slice (root_battles must still
 * be the roots' battles, unchanged since the playouts started: a carried playout reads its Pokemon's immutable data from there).
 * When the roots themselves change (the games move on to new positions), drain first -- fresh = 0 until `carried` is 0, at most
 * ceil(max_steps / slice) launches -- or the old roots' stragglers are credited to the new roots' steps.
 * Everything is asynchronous on the context's stream; consecutive launches need no host round trip. */
typedef struct oakgpu_root_steps oakgpu_root_steps;
int oakgpu_root_steps_create(oakgpu_ctx *ctx, uint32_t n_roots, uint32_t reps, uint32_t slice, uint32_t max_steps, oakgpu_root_steps **out);
void oakgpu_root_steps_destroy(oakgpu_root_steps *rs);
int oakgpu_root_steps_launch_dev(oakgpu_root_steps *rs, const uint8_t *root_battles, const uint8_t *root_durations,
                                 const uint8_t *root_results, uint8_t *lane_prng, int fresh, unsigned long long *report);
/* The carry lists hold 1 + 256 / slice steps' worth of playouts by default (3-4x what random OU roots keep in flight).  Roots whose
 * playouts mostly run into the step cap need up to ceil(max_steps / slice) - 1 steps' worth: a caller whose capacity is below
 * 2 x (carried + n_roots x reps) -- what the next launch may carry, doubled for the shards' imbalance -- reserves more BEFORE that launch
 * (synchronises the stream, keeps the playouts in flight; oak_amd.dist.RootSteps does).  An overflow is never
 * silent either way (sticky error word in the report). */
int oakgpu_root_steps_capacity(const oakgpu_root_steps *rs, uint32_t *capacity);
int oakgpu_root_steps_reserve(oakgpu_root_steps *rs, uint64_t playouts);

/* ---- `.battle.data` training frames + self-play on the GPU path.
 * oakgpu_frames_write / _read = Train::Battle::CompressedFrames::write / read (train/battle/compressed-frame.h:37-243):
 * one game = u32 record length, u16 frame count, the 384-byte battle after the opening update, the final result byte,
 * then per turn {(m-1) | (n-1) << 4, c1, c2, u32 iterations, u16 empirical value, u16 nash value, m + m + n + n u16
 * probabilities}; probabilities and values are stored as x * 65535 truncated to u16.  A `.battle.data` file is a plain
 * concatenation of such records.  oakgpu_frames_size = the record's byte length. */
typedef struct {
  uint8_t m, n;          /* legal choices per side at this turn */
  uint8_t c1, c2;        /* the pkmn_choices played */
  uint32_t iterations;
  double empirical_value, nash_value;
  double p1_empirical[9], p1_nash[9], p2_empirical[9], p2_nash[9];
} oakgpu_frame_update;
size_t oakgpu_frames_size(const oakgpu_frame_update *updates, uint32_t count);
int oakgpu_frames_write(const uint8_t *battle /* 384 */, uint8_t result, const oakgpu_frame_update *updates, uint32_t count,
                        uint8_t *buffer, size_t capacity, size_t *written);
int oakgpu_frames_read(const uint8_t *buffer, size_t size, uint8_t *battle /* 384, nullable */, uint8_t *result /* nullable */,
                       oakgpu_frame_update *updates /* nullable */, uint32_t capacity, uint32_t *count, size_t *consumed);

/* ---- Replay check of `.battle.data` records (cpp/include/py/battle/frames.h:52-67, for a whole corpus at once): every game is
 * replayed on the GPU from its stored battle (zero durations, default options) through its stored choices.  Per frame k, in
 * this order, the first failing check ends the game: the engine's result is already terminal (EARLY_END); P1's, then P2's
 * legal-choice count differs from m, n (COUNT); c1, then c2 is not among its player's legal choices (ILLEGAL, membership: the
 * record does not fix the list's order); then update(c1, c2).  After the last frame: the engine's result differs from the stored
 * result byte, a result that is not terminal included (RESULT), else OK.  A record damaged inside its own length (the ones
 * oakgpu_frames_read refuses with "truncated update", "malformed update" or "frame count does not match the record") is
 * MALFORMED and not replayed.  A game's report depends on its own record only.
 *   report: frame = the frame index of the verdict (the frame count for OK and RESULT; 0 for MALFORMED); player = 1, 2 or 0;
 * expected = the record's byte (m, n, c1 / c2, or the stored result for EARLY_END, RESULT and OK); got = the engine's byte: its
 * legal-choice count for that player (COUNT, ILLEGAL), its result byte (EARLY_END, RESULT, OK).
 *   battles / durations (nullable, n x 384 / n x 8): the state at the verdict -- before frame k's update for EARLY_END, COUNT and
 * ILLEGAL, after the last update for OK and RESULT; zeros for MALFORMED. */
typedef struct { uint32_t frame; uint8_t status, player, expected, got; } oakgpu_replay_report;
enum { OAKGPU_REPLAY_OK = 0, OAKGPU_REPLAY_COUNT = 1, OAKGPU_REPLAY_ILLEGAL = 2, OAKGPU_REPLAY_EARLY_END = 3, OAKGPU_REPLAY_RESULT = 4,
       OAKGPU_REPLAY_MALFORMED = 5 };
/* host: record boundaries + oakgpu_frames_read's validation of every record.  Indexing stops at the first record whose length
 * field cannot be trusted (a header cut short, a length below 391 bytes or past the buffer's end): *stopped_at = that byte offset
 * (size when the whole buffer was indexed), *n_records = the records in front of it.  offsets / frames / malformed all NULL:
 * count only; otherwise all three, with capacity >= *n_records. */
int oakgpu_replay_index(const uint8_t *buffer, size_t size, uint64_t *offsets, uint16_t *frames, uint8_t *malformed,
                        uint32_t capacity, uint32_t *n_records, size_t *stopped_at);
/* device: records (the file bytes, unchanged) + their index (device arrays) -> one report per record (device), in the context's
 * stream.  The frame counts are read back to order the games longest first (the call waits for the stream once, before the launch). */
int oakgpu_replay_records_dev(oakgpu_ctx *ctx, const uint8_t *records, const uint64_t *offsets, const uint16_t *frames,
                              const uint8_t *malformed, uint32_t n, oakgpu_replay_report *reports,
                              uint8_t *battles /* n x 384, nullable */, uint8_t *durations /* n x 8, nullable */);
/* host buffer in, host reports out: index, upload, replay, download.  Fails when the buffer holds more than `capacity` records. */
int oakgpu_replay_records(oakgpu_ctx *ctx, const uint8_t *buffer, size_t size, oakgpu_replay_report *reports, uint32_t capacity,
                          uint32_t *n_records, size_t *stopped_at, uint8_t *battles /* nullable */, uint8_t *durations /* nullable */);
/* ---- Training batches from `.battle.data` records (the reference's loader: pyoak.sample + EncodedBattleFrames, cpp/src/pyoak.cc:111-245,
 * py/battle/encoded-frames.h, py/battle/target.h -- there on CPU threads, one file open and one replay per sample).
 * A corpus is a buffer of records uploaded once, indexed by oakgpu_replay_index's rules (records behind `stopped_at` are not part of
 * it) with every stored battle copied to an aligned slot.  A PICK is (record r, frame f); its row holds what EncodedFrames::write and
 * Target::write produce for the state reached from the record's stored battle by update() through the stored choices of frames
 * 0 .. f-1 (zero durations at the start, no damage-roll clamp: the replay check's walk):
 *   pokemon [n,2,6,198] f32  slot 0: the DENSE Encode::Battle::Pokemon::write of the active's stored Pokemon with duration.sleep(0);
 *                            slots 1..5: the Pokemon at order[slot] with duration.sleep(slot); all zero when order[slot] == 0 or hp == 0
 *   active  [n,2,1,229] f32  the DENSE Encode::Battle::Active::write(side.active, duration); all zero when the active's stored hp is 0
 *   hp      [n,2,6,1]   f32  (float)hp / (float)stats.hp, 0 for the dead and empty slots above
 *   choice_indices [n,2,9] i64  Policy::get_index of the engine's legal choices for the state's request, in the engine's order, for
 *                            i < k; 315 (Policy::n_dim) in every other cell
 *   k, choice [n,2,1] u8     the frame's m, n and c1, c2;  iterations [n,1] u32
 *   empirical_policies, nash_policies [n,2,9] f32   (float)u16 / 65535.0f for the first k entries, 0 behind them
 *   empirical_value, nash_value [n,1] f32 likewise;  score [n,1] f32: WIN 1, LOSE 0, TIE 0.5 of the stored result
 *   status [n] u8, where [n] u32   below
 * The dense encoders are not the leaf evaluator's sparse ones: a move cell is ASSIGNED bool(pp) slot by slot, so a move held in two
 * slots shows its last slot's value (the sparse form adds 1 per slot with PP); the disabled move's cell is left as it is (the
 * reference's zero lands behind the move block, where the duration writer or the next row overwrites it); equal types give one 1.
 * Every quotient is a correctly rounded fp32 division: rows are bit for bit the reference's.
 *   A pick is OK when r names a record that is not MALFORMED (else MALFORMED, where = 0) and f < frames[r] (else OAKGPU_PICK_RANGE,
 * as for r past the last record; where = f), the stored result byte's type is 1..3 (else RESULT, where = frames[r]: there is no
 * score), and on every frame 0 .. f the replay check's per-frame checks hold in its order: the game has not ended (EARLY_END), both
 * legal-choice counts equal m, n (COUNT), both stored choices are legal (ILLEGAL); where = the failing frame, and f itself for an OK pick.  The game's FINAL
 * result is not re-derived for a pick -- a record whose last update ends elsewhere than its result byte says still yields OK picks;
 * that check is oakgpu_replay_records'.  Every cell of rows 0 .. n-1 of every tensor is written by the call (all zero for a pick
 * that is not OK, status and where excepted), nothing outside them is touched, and row i depends on pick i alone. */
enum { OAKGPU_PICK_RANGE = 6 };
typedef struct oakgpu_corpus oakgpu_corpus;
typedef struct {
  float *pokemon, *active, *hp;   /* pokemon: 16-byte aligned; active, hp: 8 */
  int64_t *choice_indices;
  uint8_t *k, *choice;
  uint32_t *iterations;
  float *empirical_policies, *nash_policies, *empirical_value, *nash_value, *score;
  uint8_t *status;
  uint32_t *where;
} oakgpu_encoded_frames;
typedef struct { uint32_t records, malformed; uint64_t frames /* of the records that are not malformed */; size_t stopped_at; } oakgpu_corpus_stats;
/* buffer: host bytes (copied; the caller's buffer is free when the call returns).  The corpus belongs to ctx and must be destroyed
 * before it. */
int oakgpu_corpus_create(oakgpu_ctx *ctx, const uint8_t *buffer, size_t size, oakgpu_corpus **out);
void oakgpu_corpus_destroy(oakgpu_corpus *corpus);
int oakgpu_corpus_info(const oakgpu_corpus *corpus, oakgpu_corpus_stats *info);
/* picks: n x 2 u32 (r, f), device.  Asynchronous on the context's stream (the corpus' workspace grows on the first call of a size). */
int oakgpu_frames_encode_dev(oakgpu_ctx *ctx, oakgpu_corpus *corpus, const uint32_t *picks, uint32_t n, const oakgpu_encoded_frames *out);
/* pyoak.sample's rule with a stream per draw.  Eligible records: not MALFORMED, frames <= max_battle_length (0 = no limit), at least
 * one frame with iterations >= min_iterations; in record order, E of them (E == 0 fails).  Draw i: fast_prng seeded with seed + i;
 * r = eligible[uniform_64 % E]; f = the (uniform_64 % V[r])-th of r's V[r] valid frames in frame order.  So draw i does not depend
 * on n.  picks_out (nullable, n x 2 u32, device) receives the picks.  The first call with a new (max_battle_length, min_iterations)
 * counts the valid frames on the GPU and waits for the stream once to list the eligible records; later calls are asynchronous. */
int oakgpu_frames_sample_dev(oakgpu_ctx *ctx, oakgpu_corpus *corpus, uint32_t n, uint64_t seed, uint32_t max_battle_length,
                             uint32_t min_iterations, uint32_t *picks_out, const oakgpu_encoded_frames *out);
/* The position encoder alone, for callers that hold states: battles n x 384 (16-byte aligned), durations n x 8, results n (the
 * request bytes) -> pokemon, active, hp, choice_indices and k (the engine's legal-choice counts; 0 for a finished battle). */
int oakgpu_encode_battles_dev(oakgpu_ctx *ctx, const uint8_t *battles, const uint8_t *durations, const uint8_t *results, uint32_t n,
                              float *pokemon, float *active, float *hp, int64_t *choice_indices, uint8_t *k);
/* host arrays in and out (staged; the calls wait for the stream).  ok_rows (nullable): how many rows have status OK. */
int oakgpu_frames_encode(oakgpu_ctx *ctx, oakgpu_corpus *corpus, const uint32_t *picks, uint32_t n, const oakgpu_encoded_frames *out,
                         uint32_t *ok_rows);
int oakgpu_frames_sample(oakgpu_ctx *ctx, oakgpu_corpus *corpus, uint32_t n, uint64_t seed, uint32_t max_battle_length,
                         uint32_t min_iterations, uint32_t *picks_out, const oakgpu_encoded_frames *out, uint32_t *ok_rows);

/* ---- A replay window: a corpus that starts empty and that self-play appends to on the device -- the moving window of the newest data
 * that the reference's reinforcement loop keeps on disk (src/oak/common_args.py:83-131: --data-window, --min-files; src/oak/rl.py runs
 * generate and battle.py on one directory).  The window holds the newest records, in arrival order, such that records <= max_records and
 * bytes <= max_bytes; older ones leave first, whole records at a time.  A batch that exceeds the window on its own leaves its newest
 * tail; a record larger than max_bytes leaves an empty window and counts as evicted.
 *   THE CONTRACT.  After any sequence of appends, every corpus call above and below (info -- with stopped_at = the surviving bytes --,
 * frame_bases, frames_sample(_dev) for any filter pair and seed, frames_encode(_dev), corpus_states, _inference, _loss_dev, _evaluate) returns
 * on the window bit for bit what it returns on oakgpu_corpus_create over the concatenation of the surviving records' bytes in order, and
 * oakgpu_corpus_records returns exactly that concatenation (so it is also how a window is saved as a `.battle.data` file).  Where the records
 * sit inside the window is the library's own business (each at a 16-byte aligned offset of one of two buffers that change places).
 *   append_dev: `stream` and `offsets` (n + 1, 8-byte aligned) are device arrays as oakgpu_forest_selfplay_records and
 * oakgpu_forest_match_records leave them with to_device = 1: record i is bytes offsets[i] .. offsets[i+1].  A slice of zero bytes is a
 * dropped game and is skipped (the offsets must lie inside `stream`: that is the caller's to keep, as for every device array).  Every other slice is checked on the device by the rules of oakgpu_frames_read: a slice whose length field
 * is not the slice's length (or is below the fixed 391 bytes) is REJECTED -- not appended, counted; a record damaged inside its own length
 * (truncated or malformed update, frame count that disagrees) is appended with its malformed flag set, as oakgpu_replay_index does.
 *   append: host bytes; the record boundaries are found by oakgpu_replay_index's length walk, bytes behind a length that cannot be
 * trusted are left out (as oakgpu_corpus_create leaves them out), and the same device path runs.
 *   Both wait for the context's stream ONCE and read one summary of 40 bytes plus the batch's own frame counts and classes (3 bytes per
 * slice): nothing is read in proportion to the window.  (A call that has to grow one of the window's buffers waits once more.)  After an
 * append the sampler's lists are rebuilt on the device at the next oakgpu_frames_sample_dev of a filter pair: the valid-frame counts, the
 * eligibility flags, a scan and a scatter in record order; the host reads the count E alone.
 *   Refused before anything is launched, by a message that names the argument: max_records == 0 or max_bytes < 391 (window_check, host
 * only); a corpus that oakgpu_corpus_create_window did not make; a corpus of another ctx; null or misaligned offsets.
 *   window_stats: out = {records, bytes, appended, evicted, rejected, appends} -- the window now, then lifetime counts: records that joined,
 * records that left (those of a batch that never fitted included), slices refused, calls.
 *   records: the window's bytes into `out` (device memory when to_device, else host memory; the host form waits for the stream); *bytes
 * receives their number, and `out` NULL asks for the number alone. */
int oakgpu_corpus_window_check(uint32_t max_records, size_t max_bytes);
int oakgpu_corpus_create_window(oakgpu_ctx *ctx, uint32_t max_records, size_t max_bytes, oakgpu_corpus **out);
int oakgpu_corpus_append_dev(oakgpu_ctx *ctx, oakgpu_corpus *corpus, const uint8_t *stream, const uint64_t *offsets, uint32_t n);
int oakgpu_corpus_append(oakgpu_ctx *ctx, oakgpu_corpus *corpus, const uint8_t *buffer, size_t size);
int oakgpu_corpus_window_stats(const oakgpu_corpus *corpus, uint64_t out[6]);
int oakgpu_corpus_records(oakgpu_ctx *ctx, oakgpu_corpus *corpus, uint8_t *out, size_t capacity, size_t *bytes, int to_device);
/* Diagnostic (no GPU involved): the slice rule of append_dev on host arrays, the text the device pass compiles (oak_amd/csrc/record_scan.hpp).
 * kinds[i]: 0 dropped, 1 record, 2 record with its malformed flag, 3 rejected; frames[i]: the header's frame count of a record, else 0. */
int oakgpu_window_scan_host(const uint8_t *stream, const uint64_t *offsets, uint32_t n, uint8_t *kinds, uint16_t *frames);

/* ---- A network evaluated on EVERY frame of a corpus: what pyoak.cpp_inference (cpp/src/pyoak.cc:331-392) returns for one record and
 * the terms battle.py's loss (src/oak/battle.py:203-262) would report, for all records at once.  Each record is walked ONCE (the walk of
 * a pick, with every frame written down) and the evaluator runs once per CHUNK: a range of consecutive whole records.
 *   Rows.  Record r owns rows bases[r] .. bases[r+1]-1 of the corpus, one per frame in frame order; bases = prefix sums of the frame
 * counts, a MALFORMED record counting 0 (it has no rows).  Inside a chunk that starts at record `first` the rows are numbered from
 * bases[first].  Row (r, f) holds the state in front of frame f: battle, durations, the request byte, both sides' legal choices in
 * the engine's order with their counts.  status / where of the row are those of the pick (r, f) above: OK (where = f), or the
 * record's verdict -- COUNT, ILLEGAL, EARLY_END with where = the failing frame, from that frame on; RESULT with where = frames[r]
 * on every row.  A row that is not OK is all zero apart from status and where, in every array of every call below.
 *   The calls write every cell of the chunk's rows and nothing outside them; a row depends on its record alone, so the chunking
 * changes no result.  They fail, before anything is launched, when the chunk's rows exceed rows_capacity (what the caller's arrays
 * hold) or the record range leaves the corpus.  The *_dev calls take device arrays and are asynchronous on the context's stream (the
 * corpus' workspace grows on the first call of a size, waiting for the stream then); the others take host arrays and return complete. */
int oakgpu_corpus_frame_bases(const oakgpu_corpus *corpus, uint64_t *bases /* records + 1 */);
/* Host only, no GPU: consecutive record ranges, each as large as fits in chunk_rows (0 = 65,536) rows.  Chunk i is records
 * first_record[i] .. first_record[i+1]-1; first_record[*n_chunks] = n.  first_record NULL: count only; otherwise capacity >=
 * *n_chunks + 1.  Fails when one record alone has more frames than chunk_rows; the message names the record.  malformed is nullable. */
int oakgpu_corpus_chunks(const uint16_t *frames, const uint8_t *malformed, uint32_t n, uint32_t chunk_rows, uint32_t *first_record,
                         uint32_t capacity, uint32_t *n_chunks);
/* The walk alone: battles rows x 384 (16-byte aligned), durations rows x 8 (8-byte aligned), results rows, choices rows x 9 and
 * counts rows per side, status rows, where rows (u32). */
int oakgpu_corpus_states_dev(oakgpu_ctx *ctx, oakgpu_corpus *corpus, uint32_t first_record, uint32_t n_records, uint32_t rows_capacity,
                             uint8_t *battles, uint8_t *durations, uint8_t *results, uint8_t *p1_choices, uint8_t *p1_counts,
                             uint8_t *p2_choices, uint8_t *p2_counts, uint8_t *status, uint32_t *where);
int oakgpu_corpus_states(oakgpu_ctx *ctx, oakgpu_corpus *corpus, uint32_t first_record, uint32_t n_records, uint32_t rows_capacity,
                         uint8_t *battles, uint8_t *durations, uint8_t *results, uint8_t *p1_choices, uint8_t *p1_counts,
                         uint8_t *p2_choices, uint8_t *p2_counts, uint8_t *status, uint32_t *where);
/* The walk, then the leaf evaluator's value-and-policy call over the chunk's rows in ONE call of that many leaves (fp32 and discrete
 * networks alike), then the policies.  Every pointer is nullable:
 *   value [rows] f32; policy_logit [rows,2,9] f32: the legal logits, 0 behind the count; policy [rows,2,9] f32: the fp32 softmax over
 * the first k logits (shifted by their maximum), 0 behind them -- cpp_inference's `policy`; k [rows,2] u8; choices [rows,2,9] u8;
 * status [rows] u8; where [rows] u32. */
typedef struct {
  float *value, *policy_logit, *policy;
  uint8_t *k, *choices, *status;
  uint32_t *where;
} oakgpu_corpus_eval;
int oakgpu_corpus_inference_dev(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_corpus *corpus, uint32_t first_record, uint32_t n_records,
                                uint32_t rows_capacity, const oakgpu_corpus_eval *out);
/* The loss terms of a row against its frame's stored targets (u16 / 65535.0f, the values the training rows carry), in fp32:
 *   sq_err = (value - vt)^2 with vt = (wn * nash_value + we * empirical_value) + ws * score           (battle.py:227-231)
 *   ce[s]  = -sum_i t_i * logp_i / max(1, #{t_i != 0}), t_i = (1 - pn) * empirical_i + pn * nash_i over side s' k legal choices,
 *            logp = the log-softmax of its k legal logits                                                (battle.py:203-209, 238-245)
 * A row that is not OK (excluded = 2) or whose iterations are below min_iterations (excluded = 1) has zero terms; the others have
 * excluded = 0.  Per record of the chunk: record_sums [n_records,3] f64 = the sums of sq_err, ce[0], ce[1] over its rows with
 * excluded = 0, in frame order; record_counts [n_records,3] u32 = how many of its rows have excluded = 0, 1, 2.  All five arrays of
 * `terms` are required (record_sums 8-byte aligned); `out` is nullable, as is each pointer in it. */
typedef struct { float wn, we, ws, pn; uint32_t min_iterations; } oakgpu_loss_params;
typedef struct {
  float *sq_err, *ce /* [rows,2] */;
  uint8_t *excluded;
  double *record_sums;
  uint32_t *record_counts;
} oakgpu_corpus_terms;
int oakgpu_corpus_loss_dev(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_corpus *corpus, uint32_t first_record, uint32_t n_records,
                           uint32_t rows_capacity, const oakgpu_loss_params *p, const oakgpu_corpus_eval *out, const oakgpu_corpus_terms *terms);
/* Host forms, chunk by chunk (chunk_rows = 0: 65,536).  inference: host arrays of bases[first + n] - bases[first] rows.  evaluate:
 * the whole corpus; the per-record float64 sums are added in record order on the host, so the totals do not depend on chunk_rows.
 *   sq_err, ce1, ce2: the sums over the `rows` included rows; excluded: rows left out for their iterations; failed: rows that are not
 * OK; mse = sq_err / rows, ce_p1 = ce1 / rows, ce_p2 = ce2 / rows (battle.py's batch means; 0 when rows = 0).  per_record (nullable):
 * one entry per record of the corpus. */
typedef struct { double sq_err, ce1, ce2; uint64_t rows, excluded, failed; double mse, ce_p1, ce_p2; } oakgpu_corpus_losses;
int oakgpu_corpus_inference(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_corpus *corpus, uint32_t first_record, uint32_t n_records,
                            uint32_t chunk_rows, const oakgpu_corpus_eval *out);
int oakgpu_corpus_evaluate(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_corpus *corpus, const oakgpu_loss_params *p, uint32_t chunk_rows,
                           oakgpu_corpus_losses *total, oakgpu_corpus_losses *per_record);

/* ---- Batches of whole games between two policies, resident on the device: the reference's `vs` (cpp/src/vs.cc:107-408) in the one
 * form that needs no tree,   vs --budget=0 --bandit=pucb-1.0 --policy-mode=p --p1-eval=A --p2-eval=B   -- with a zero budget a contextual
 * bandit's Output carries only the root prior, the softmax of the policy head's legal logits (search/mcts.h:196-209), and mode `p` samples
 * from it (util/policy.h:22-106): each side plays its network's raw policy.  n games start from the caller's states (as oakgpu_rollout_dev
 * takes them) and run turn by turn -- oakgpu_tree_step_dev, oakgpu_leaf_eval_policy_dev, the pick -- until each has ended or made
 * max_turns updates (result type 0 then, value 0.5).
 *   Draws per game and turn, from the game's own fast_prng state (8 bytes, in / out):
 *     both seats RANDOM: one uniform_64; c1 = p1_choices[seed % m], c2 = p2_choices[(seed >> 32) % n] -- the rollout kernels' rule, so such
 *       a call equals oakgpu_rollout_dev with prep = 0 in every output byte;
 *     otherwise seat p1 first, then seat p2: a POLICY seat with one legal choice draws nothing and plays it (vs.cc:258,273); a POLICY seat with
 *       k > 1 draws one uniform (util/random.h:109-112) and takes sample_pdf of its policy (random.h:123-132); a RANDOM seat draws one
 *       uniform_64 and plays choices[seed % k].
 *   The policy of a POLICY seat over its k legal logits l, in the network's order: prior_i = expf(l_i) / sum with the sum in fp32 in index
 *   order and the quotient in double (search/util/softmax.h:5-15 into Output's doubles); temp != 1: pow(x, temp), renormalised; entries below
 *   `min` zeroed, renormalised (policy.h:70-95).  A policy zeroed entirely is the reference's "RuntimePolicy: zero policy, mode: p": refused
 *   before anything is launched where that is known (min > 1); otherwise that game stops there with values_out = NaN and results_out = 0xFF, counts in
 *   none of the four counters, and the call returns -1 with the lowest such game index in its message -- every other game's outputs are complete.
 *   Outputs are indexed by the caller's game index and depend on nothing but the game: not on poll, compact_below, n or the rest of the batch.
 * turns_out: updates made; values_out: 1 / 0 / 0.5 as the rollout's; battles_out / durations_out (nullable; battles_out 16-byte aligned): the
 * final states; choice_log (nullable): n x log_turns x 2 bytes (c1, c2), game-major, the first log_turns turns of every game -- entries no
 * game reaches are not written.  counts_out (host, nullable): wins, ties, losses of seat p1, games stopped at max_turns.
 *   Schedule: finished rows are retired, and the host reads the live count, every `poll` turns; when the live share of the resident rows falls
 * below compact_below the live rows are compacted (stable, into the other half of a double buffer) and the evaluator and the tree step run on
 * the live prefix only.  The workspace belongs to the context.  The _dev call takes device arrays and returns with the games complete (it
 * waits for the stream at every poll); the other takes host arrays. */
#define OAKGPU_SEAT_RANDOM 0   /* the rollout kernel's rule */
#define OAKGPU_SEAT_POLICY 1   /* the network's prior, RuntimePolicy mode "p" with budget 0 */
typedef struct {
  int32_t kind;                /* OAKGPU_SEAT_* */
  oakgpu_net *net;             /* POLICY: required (fp32 or discrete handle, loaded on the context's device); RANDOM: ignored */
  double temp, min;            /* RuntimePolicy::Options temp / min (util/policy.h:70-95); 0 / 0 mean 1 / 0 */
} oakgpu_seat;
typedef struct {
  oakgpu_seat p1, p2;
  uint32_t max_turns;          /* updates per game before it is stopped with result type 0 (0 = 1000) */
  uint32_t poll;               /* host looks at the live count every `poll` turns (0 = 16) */
  float compact_below;         /* compact the resident rows when live / rows falls below this (0 = 0.5; > 1 = at every poll; < 0 = never) */
  uint32_t log_turns;          /* capacity of choice_log per game, 0 = no log */
} oakgpu_policy_games_params;
int oakgpu_policy_games_dev(oakgpu_ctx *ctx, const oakgpu_policy_games_params *params, const uint8_t *battles, const uint8_t *durations,
                            const uint8_t *results_in, uint8_t *prng_state, uint32_t n, uint8_t *results_out, uint32_t *turns_out,
                            float *values_out, uint8_t *battles_out, uint8_t *durations_out, uint8_t *choice_log, uint64_t counts_out[4]);
int oakgpu_policy_games(oakgpu_ctx *ctx, const oakgpu_policy_games_params *params, const uint8_t *battles, const uint8_t *durations,
                        const uint8_t *results_in, uint8_t *prng_state, uint32_t n, uint8_t *results_out, uint32_t *turns_out,
                        float *values_out, uint8_t *battles_out, uint8_t *durations_out, uint8_t *choice_log, uint64_t counts_out[4]);
/* Diagnostic: the schedule of the calling thread's last oakgpu_policy_games* call -- rows the evaluator and the tree step ran over, summed
 * over the turns (the games' own need is the sum of turns_out); turns looped; compactions; polls. */
int oakgpu_policy_games_last_stats(uint64_t out[4]);

/* the compile-time engine switches this library was built with (DESIGN 0 order): MULTIHIT_ROLL_FIRST, PSYWAVE_SHOWDOWN,
 * COUNTER_SHOWDOWN, ACCURACY_LAST.  The default build reports 1, 1, 0, 0. */
int oakgpu_engine_switches(int out[4]);
/* One self-play game, the per-game loop of the reference's data generator (cpp/src/generate.cc:238-322): PKMN::battle(teams,
 * battle_seed) + opening update, then per turn oakgpu_search -> RuntimePolicy::process_and_sample for both sides
 * (util/policy.h:22-106; mode words e / n / x / p with optional weights, e.g. "e0.9-x0.1"; p = prior + empirical, the
 * reference's fall-through, useful with the contextual bandits only) -> frame -> update, until the result
 * is terminal; the finished record is written to `buffer`.  Every battle operation runs on the GPU.  Fails (no record
 * written) when the game exceeds max_battle_length updates, like the reference (generate.cc:268-271); 0 = no limit, the reference's
 * default: the engine ends a game at turn 1,000 by itself (records of up to ~1,010 frames). */
typedef struct {
  oakgpu_search_params search; /* seed is replaced per turn from `seed` below */
  char policy_mode[16];
  double policy_temp, policy_min;
  uint32_t max_battle_length;
  uint64_t seed;
  int32_t keep_node;           /* generate's --keep-node (generate.cc:324-333): one heap for the game, Heap::update with the played
                                * indices and the observation after every turn (the subtree is searched on); 0 = a fresh heap per turn */
  uint32_t nodes_kept;         /* out: how many of the game's updates found their child (RuntimeData::update_with_node_counter) */
  /* Fast searches (generate's --fast-budget / --fast-search-prob, generate.cc:292-299; rl.py trains with --min-iterations = fast_budget
   * + 1, so only the full-budget frames reach the loss).  With fast_search_prob > 0 every turn starts with use_fast = uniform01(rng) <
   * fast_search_prob on the game's stream, BEFORE the search seed is drawn; a fast turn is searched with fast_budget iterations and
   * picked with fast_policy_mode, every other turn with search.iterations and policy_mode; the frame stores the iterations that ran, and
   * every frame is written.  The rule is oak_amd/csrc/selfplay_pick.hpp's turn_prelude, one text for the host and the device loop.
   * Two departures from the reference: the draw comes from the game's own stream (the reference: the worker thread's device), and it is
   * skipped when fast_search_prob is 0 -- all zeros is a game without fast searches, byte for byte. */
  uint32_t fast_budget;        /* 0 = search.iterations */
  double fast_search_prob;     /* 0 = off */
  char fast_policy_mode[16];   /* "" = policy_mode */
} oakgpu_selfplay_params;
/* Skipped battles (generate's --battle-skip-prob / --t1-budget, generate.cc:233-236, 293-296, 303-309, 344), for the forest loop's _build
 * calls alone; oakgpu_selfplay_game(s), the host per-game loop, know nothing of them.  A game with a built seat is skipped with
 * probability battle_skip_prob: its first turn is searched with t1_budget iterations for its matchup value, and it is dropped with
 * status OAKGPU_FSP_SKIPPED.  The rule is selfplay_pick.hpp's game_is_skipped; the draw has a stream of its own (see the _build calls).
 * A struct of its own beside oakgpu_selfplay_params, whose size and layout stay what they were. */
typedef struct {
  uint32_t t1_budget;          /* a skipped game's one search; 0 = search.iterations */
  double battle_skip_prob;     /* 0 = off */
} oakgpu_selfplay_skip;
/* endless_battle_check (cpp/src/generate.cc:127-152): 1 when every pairing of the two teams (2 x 6 x {species, 4 moves}) is a Ghost against a
 * Ghost with no move on either side that can hit a Ghost (type Normal / Fighting or base power 0) -- with ebc=false such a game runs to turn
 * 1,000; the generator draws other teams, and oakgpu_selfplay_game(s) refuse the pair with "EBC check failed". */
int oakgpu_endless_battle_check(const uint8_t *teams);
int oakgpu_selfplay_game(oakgpu_ctx *ctx, oakgpu_net *net /* nullable for eval != 1 */, const uint8_t *teams /* 60 */,
                         uint64_t battle_seed, oakgpu_selfplay_params *params, uint8_t *buffer, size_t capacity,
                         size_t *written, uint32_t *n_frames, uint8_t *result);

/* n self-play games at once on one GPU (the generator's N worker threads, generate.cc:527-536): game g on ctxs[g] -- a context of its own
 * each -- with teams + 60 g, battle_seeds[g], params[g]; its record goes to buffers + g * capacity_each, written[g] / n_frames[g] /
 * results[g] as oakgpu_selfplay_game returns them.  Every game is byte for byte the game it would be alone.  threads_per_game: host
 * threads of each game's tree walks (1, 2, 4, 8, 16); 0 = the usable cores shared evenly. */
int oakgpu_selfplay_games(oakgpu_ctx *const *ctxs, oakgpu_net *net, const uint8_t *teams, const uint64_t *battle_seeds, oakgpu_selfplay_params *params,
                          uint32_t n, int threads_per_game, uint8_t *buffers, size_t capacity_each, size_t *written, uint32_t *n_frames,
                          uint8_t *results);

/* ---- self-play over the forest search: a batch of n games resident on one device, `.battle.data` out (forestplay.hip).
 * Per turn: one oakgpu_forest_search_dev over the live games, one pick kernel, oakgpu_update_dev, retire + compact; at the end a pack
 * kernel writes the finished CompressedFrames records as one contiguous byte stream, in game order.
 *   Semantics.  Game g is oakgpu_selfplay_game(teams + 60 g, battle_seeds[g], {params with seed = seeds[g], search.batch = 1, keep_node
 *   = 0}): oakgpu_init_battles_dev with the opening update (the record's stored battle); rng = seeds[g] ^ 0x9FB21C651E98DF25; while the
 *   result is not terminal: search seed = splitmix64(rng), tree g of the forest search, process_output in double, get_policy for both
 *   sides, i = sample_pdf(pol1), j = sample_pdf(pol2), the frame's update, oakgpu_update_dev with (c1, c2).  One text states the rule on
 *   both sides (oak_amd/csrc/selfplay_pick.hpp); a UCB game's record equals the host loop's byte for byte, a PUCB game (device expf priors)
 *   and any game with policy_temp != 1 (device pow) are held to the forest search's own outputs.  params->search.seed and search.batch
 *   are ignored; keep_node must be 0 on a plain forest (see below for a kept one).
 *   Game length.  A game that already holds max_battle_length frames (0 = 2,048) when another is due is dropped: status
 *   OAKGPU_FSP_MAX_LENGTH, zero bytes in the stream, stored result unspecified; the call still returns 0.  A policy the minimum cut zeroes
 *   entirely stops that game alone with OAKGPU_FSP_ZERO_POLICY and no record.
 *   solve_nash = 1: the integer payoffs are formed on the device, solved on up to 16 host threads (oakgpu_solve_matrix's solver) and go
 *   back up before the pick -- what oakgpu_forest_search(solve_nash = 1) computes.  0: the nash fields are stored as 0.
 *   solve_nash = 2: the same strategies and values, bit for bit, from oakgpu_nash_solve_dev between the payoff kernel and the pick, on the
 *   stream: no copy down, no host threads, no upload and neither of the two synchronisations that 1 adds to every turn.
 *   Refused before any launch (oakgpu_forest_selfplay_check; teams: host bytes, nullable = not checked): keep_node on a plain forest, an unknown mode
 *   letter or 'b' or more than 8 words, policy_min > 1, an 'n' word without solve_nash, a team pair that fails
 *   oakgpu_endless_battle_check (the lowest such game is named), and everything oakgpu_forest_check refuses.
 *   Independence.  Game g's record, frame count, result and status depend on its own inputs and the parameters only.
 * _dev takes device teams (n x 60), battle_seeds and seeds (n x u64) and returns with the games complete and the stream resident in
 * the forest's workspace; _records copies the last call's stream (stream nullable: *bytes alone is the size query), offsets[n + 1],
 * n_frames[n], results[n] and status[n] out -- to device memory with to_device != 0; every output nullable; the forest-less form takes host
 * arrays.  _last_stats: turns looped, rows searched summed over turns, compactions, host reads of the live count.
 * oakgpu_selfplay_pick_host (no GPU involved) is the pick rule alone on one root output: process_output's empirical fields, both
 * policies, i, j, the advanced rng and the encoded update bytes (update: 83 bytes, nullable; nash / prior / choice arrays nullable = 0 /
 * the index itself). */
#define OAKGPU_FSP_OK 0
#define OAKGPU_FSP_MAX_LENGTH 1
#define OAKGPU_FSP_ZERO_POLICY 2
#define OAKGPU_FSP_SKIPPED 3 /* the _build calls: searched once for its matchup value, not played (see below) */
int oakgpu_forest_selfplay_check(uint32_t max_trees, uint32_t max_iterations, int contextual, const oakgpu_selfplay_params *params, int has_net,
                                 uint32_t n, const uint8_t *teams, int solve_nash);
int oakgpu_forest_selfplay_dev(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_selfplay_params *params, const uint8_t *teams,
                               const uint64_t *battle_seeds, const uint64_t *seeds, uint32_t n, int solve_nash);
int oakgpu_forest_selfplay_records(oakgpu_forest *forest, uint8_t *stream, size_t capacity, size_t *bytes, uint64_t *offsets, uint32_t *n_frames,
                                   uint8_t *results, uint8_t *status, int to_device);
int oakgpu_forest_selfplay(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_selfplay_params *params, const uint8_t *teams,
                           const uint64_t *battle_seeds, const uint64_t *seeds, uint32_t n, int solve_nash);
int oakgpu_forest_selfplay_last_stats(const oakgpu_forest *forest, uint64_t out[4]);
/* The last call's turn loop as the host saw it: out[0] = stream synchronisations, out[1] = copies between host and device.  Per turn one
 * of each for the live count (what _last_stats counts), and with solve_nash = 1 two more of each for the payoffs and the strategies. */
int oakgpu_forest_selfplay_last_traffic(const oakgpu_forest *forest, uint64_t out[2]);
/* keep_node = 1 on a kept forest (oakgpu_forest_create_kept; `contextual | OAKGPU_FOREST_KEPT` in _check): the game's tree goes on from turn
 * to turn as oakgpu_selfplay_game's heap does (generate.cc:324-333).  The pick leaves the played cell in the row, oakgpu_update_dev its
 * observation; the next turn's compaction hands its source-row list to ONE oakgpu_forest_advance_dev, which re-roots every live tree and
 * moves it with its row (no new host read), and the turn's search is oakgpu_forest_search_kept_dev; a retired row has no successor.  Per
 * game, nodes_kept counts the advances that kept a subtree, minus 1 per root mismatch but never below 0 (selfplay.hip:250-256,275), gathered
 * by game index with the other per-game results and read once at the end (_nodes_kept: n x u32, zeros after a call without keep_node).
 * A game is the host loop's game with keep_node = 1 as long as no tree is dropped for want of room (see oakgpu_forest_advance_dev), which
 * _keep_stats reports: out = { sum of nodes_kept, trees dropped, root mismatches, nodes carried into the turns' searches } of the last call. */
int oakgpu_forest_selfplay_nodes_kept(oakgpu_forest *forest, uint32_t *nodes_kept, int to_device);
/* Fast searches on the forest (params->fast_search_prob > 0; the rule is with oakgpu_selfplay_params).  The flag is drawn with the turn
 * prelude; the turn's compaction becomes a stable two-class partition -- the live rows of the larger budget first, those of the smaller
 * after -- so the turn's ONE oakgpu_forest_search_budgets(_kept)_dev gets non-increasing budgets and launches exactly the tree-iterations
 * it runs; with keep_node the trees follow their rows through the advance's source-row list.  With fast_search_prob == 0 the order, the
 * calls and the bytes are those of a call without the fields.  The per-turn host read stays the one of the live count.
 * _check also refuses by name: fast_search_prob outside [0, 1] or NaN, fast_budget above max_iterations, and a fast_policy_mode that
 * policy_mode would be refused for (an 'n' word without solve_nash included).
 * _fast_stats: out = { fast frames, full frames (both of the records kept), tree-iterations launched, tree-iterations run } of the last call.
 * _set_partition(0) (benchmarks only: tools/fast_search_bench.py's control run) leaves the rows of the forest's NEXT self-play call in game
 * order, so that launched exceeds run; the call after it partitions again. */
int oakgpu_forest_selfplay_fast_stats(oakgpu_forest *forest, uint64_t out[4]);
int oakgpu_forest_selfplay_set_partition(oakgpu_forest *forest, int on);
/* host only: selfplay_pick.hpp's turn prelude on one stream -- *rng advances, *use_fast and *search_seed are the turn's */
int oakgpu_selfplay_prelude_host(uint64_t *rng, double fast_search_prob, int32_t *use_fast, uint64_t *search_seed);
int oakgpu_forest_selfplay_keep_stats(const oakgpu_forest *forest, uint64_t out[4]);
/* Matchup values and skipped battles: the build network's side of self-play (generate.cc:233-236, 293-309, 344, 361-383).
 * _matchup: n doubles, to host or device memory, valid after any forest self-play call: the empirical value (process_output's) of each
 *   game's FIRST search, p1's view -- what generate stores as a built seat's trajectory value (p2's is 1 - it); NaN for a game that was
 *   never searched.  The pick kernel scatters it by game index on the row's first frame; no other output changes.
 * _build_dev / _build are _dev / the host-array call plus `built`: n bytes (device memory for _build_dev, host memory otherwise), bit 0 =
 *   p1's team was built, bit 1 = p2's; NULL = no game is built, and that IS the call without it, byte for byte.
 *   Skip rule (selfplay_pick.hpp's game_is_skipped; oakgpu_selfplay_skip_host is the same text on the host): game g is skipped when
 *   built[g] != 0 && battle_skip_prob > 0 && uniform01(x) < battle_skip_prob, x = seeds[g] ^ 0x5B1D7C83A46E20F9.  Departure from the
 *   reference, which draws from its worker thread's device: the draw has a stream of its own and the game's stream is untouched, so a
 *   game that is NOT skipped is byte for byte the game of a call without the fields, whatever `built` says.
 *   A skipped game runs turn 1's prelude as any game (with fast searches: the flag, then the search seed), is searched by the turn's one
 *   search with t1_budget iterations whatever the flag (generate.cc:293-296; 0 = search.iterations), and the pick writes its matchup and
 *   nothing else: no policy draw, no frame, no update bytes.  The next retire pass retires it with OAKGPU_FSP_SKIPPED: zero bytes in the
 *   stream, n_frames 0, result byte 0; from turn 2 on it is in no launch.  On a kept forest its tree simply has no successor.
 *   Turn 1's search is a budgets search whenever a skipped row's budget differs from another row's; its rows are NOT sorted by budget
 *   on that one turn, so _fast_stats' launched may exceed run by that turn's slack.  _last_stats' rows searched counts a skipped game once.
 *   `skip` (nullable = all zeros: nothing is skipped) holds battle_skip_prob and t1_budget.
 * oakgpu_forest_selfplay_skip_check (host only; the _build calls run it after oakgpu_forest_selfplay_check, before any launch) refuses by
 *   name: battle_skip_prob outside [0, 1] or NaN, t1_budget above the forest's max_iterations. */
int oakgpu_forest_selfplay_skip_check(uint32_t max_iterations, const oakgpu_selfplay_skip *skip);
int oakgpu_forest_selfplay_build_dev(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_selfplay_params *params, const oakgpu_selfplay_skip *skip,
                                     const uint8_t *teams, const uint64_t *battle_seeds, const uint64_t *seeds, const uint8_t *built, uint32_t n,
                                     int solve_nash);
int oakgpu_forest_selfplay_build(oakgpu_forest *forest, oakgpu_net *net, const oakgpu_selfplay_params *params, const oakgpu_selfplay_skip *skip,
                                 const uint8_t *teams, const uint64_t *battle_seeds, const uint64_t *seeds, const uint8_t *built, uint32_t n,
                                 int solve_nash);
int oakgpu_forest_selfplay_matchup(oakgpu_forest *forest, double *out, int to_device);
/* host only: 1 when the game of this seed is skipped, else 0 (probability 0 or built == 0: no draw) */
int oakgpu_selfplay_skip_host(uint64_t seed, double prob, int built);
int oakgpu_selfplay_pick_host(uint32_t m, uint32_t n, const uint64_t *visit_matrix, const double *value_matrix, uint64_t iterations,
                              const double *p1_nash, const double *p2_nash, double nash_value, const double *p1_prior, const double *p2_prior,
                              const uint8_t *p1_choices, const uint8_t *p2_choices, const char *policy_mode, double policy_temp,
                              double policy_min, uint64_t *rng, double *empirical_value, double *p1_empirical, double *p2_empirical,
                              double *p1_policy, double *p2_policy, int32_t *i_out, int32_t *j_out, uint8_t *update, uint32_t *update_len);

/* ---- matches between two SEARCH agents over the forest search: the reference's `vs` with a budget (cpp/src/vs.cc:230-345), a batch of n
 * games resident on one device (forestmatch.hip).  Seat p1 and seat p2 are independent agents: each has its own oakgpu_search_params
 * (bandit, budget, evaluator), its own network and its own RuntimePolicy options; each searches for itself and plays its own side's move.
 *   Semantics.  Game g starts from battles + 384 g, durations + 8 g, results_in[g] (as oakgpu_policy_games_dev takes them) and seeds[g].
 *   A game whose input result is terminal is retired at once: results_out[g] = results_in[g], turns_out[g] = 0, status OK.  Otherwise
 *   rng = seeds[g] ^ 0x9FB21C651E98DF25 and, while the result is not terminal and fewer than max_turns updates were made, per turn:
 *   (1) m, n = the legal choice counts of p1, p2.  (2) Seeds, seat p1 first, then seat p2: a seat with more than one choice draws its tree
 *   seed as one splitmix64(rng); a seat with exactly one choice draws nothing and is NOT searched (vs.cc:258,273).  (3) Seat p1's search
 *   is one oakgpu_forest_search_dev with p1's parameters (batch = 1, seed ignored) and net over exactly the live rows with m > 1, gathered
 *   into a contiguous buffer in row order; then seat p2's over the rows with n > 1; a seat without rows makes no call.  Tree k of a call
 *   is the standalone search of that state with that seed.  (4) solve_nash != 0: the exact Nash solve of every searched row's payoffs, as
 *   oakgpu_forest_selfplay does it (1: device payoffs, host threads, upload; 2: oakgpu_nash_solve_dev on the stream).  (5) Pick, seat p1 first, then seat p2, each from ITS OWN
 *   search's output: process_output in double, get_policy for that seat's side with that seat's {policy_mode, policy_temp, policy_min},
 *   index = sample_pdf(policy, rng), the choice at that index; ev = the output's empirical_value (P1's point of view for both seats).  An
 *   unsearched seat plays its one choice, draws nothing, ev = 0.  The rule is selfplay_pick.hpp's text without contraction; pow
 *   (policy_temp != 1) and expf (PUCB priors) are the device's.  (6) Early stop (vs.cc:263,287,300; early_stop = 0: off): a searched seat's
 *   sign is s = +1 when t >= 1, -1 when t <= -1, else 0, with t = (log(ev) - log(1 - ev)) / early_stop in double (ev = 1 / 0 give +-inf
 *   and so +-1; the reference's int cast is undefined there and equals this wherever it is defined); an unsearched seat has s = 0.
 *   s1 * s2 > 0 ends the game BEFORE the update: result byte 1 (Win) for s1 > 0, else 2 (Lose), status EARLY_STOP, the turn not counted in
 *   turns_out.  (7) A policy the minimum cut zeroes entirely stops that game alone: status ZERO_POLICY, result 0xFF, no counter, no log
 *   record for that turn, and when it was seat p1's then seat p2 draws nothing; the call still returns 0.  (8) Otherwise
 *   oakgpu_update_dev with (c1, c2).  A game cut at max_turns (0 = 1,000) has status MAX_TURNS and its last result byte (type 0).
 *   Independence.  Game g's outputs depend on its own inputs and the parameters only -- not on n, its neighbours, the compaction, the
 *   forest's capacity or earlier calls.
 *   Outputs, by game index (device arrays in _dev, all nullable): results_out n bytes, turns_out n x u32 (updates made), status_out n
 *   bytes (OAKGPU_FM_*), turn_log n x log_turns records of 24 bytes {u8 c1, c2, m, n; u32 0; double ev_p1, ev_p2} -- record (g, t) is the
 *   game's t-th turn, entries no game reaches are not written, the early-stop turn writes c1 = c2 = 0; counts_out (host, nullable): wins,
 *   ties, losses of seat p1 (early stops included), games stopped at max_turns.
 *   Schedule.  Per turn: oakgpu_choices_dev for both sides over the resident rows, retire by scatter on game index, the compaction into the
 *   other half of a double buffer (the choice counts ride along), and ONE prelude kernel (streams, both seats' tree seeds, both row lists by
 *   a stable prefix sum) that leaves one 12-byte record -- live rows, p1 rows, p2 rows -- which is the loop's single host read per turn (the forest
 *   search and the Nash solve read what they read by themselves); per seat a gather (393 bytes per row, the battle in 16-byte pieces),
 *   the search, the pick scattered back by row list; one kernel for the early stop and the log; the update.  The two seats' searches run
 *   one after the other on the same forest; the workspace belongs to the forest.
 *   Refused by name before any launch (oakgpu_forest_match_check, host only): for either seat everything oakgpu_forest_check refuses --
 *   time budgets, matrix_ucb, UCB1 / Exp3 / PExp3, iterations 0 or above max_iterations, PUCB on a non-contextual forest, a network
 *   evaluator without a net -- n above max_trees, an unknown mode letter or 'b' or more than 8 words, policy_min > 1, an 'n' word without
 *   solve_nash, early_stop < 0 or NaN.  There are no keep_node-style options.
 * _dev takes device arrays (battles 16-byte aligned) and returns with the games complete; the other form takes host arrays.
 * _last_stats: turns looped, p1 rows searched, p2 rows searched (summed over the turns), host reads of the per-turn record.
 * oakgpu_match_pick_host (no GPU involved) is ONE seat's pick and early-stop sign from one root output: side 0 / 1, the root matrices and
 * iterations, that side's nash and prior (nullable = 0), the seat's mode / temp / min, early_stop, rng in and out -> policy[9], index, ev,
 * sign.  A zeroed policy fails ("zero policy").
 *   Records (vs.cc:221-222,308-309,329-333,380-395: the p1/ and p2/ `.battle.data` of a match).  oakgpu_forest_match_set_records(forest, 1)
 *   switches recording on for the forest's later match calls (default 0; refused by name for a null forest and for `on` outside 0 and 1;
 *   nothing else about the forest refuses it).  With it off a call is exactly the call described above: the same launches, host reads
 *   (_last_stats), memory and outputs.  With it on every game is also written as TWO CompressedFrames records, one per seat, and the
 *   call ends with each seat's records packed into one contiguous `.battle.data` byte stream in game order, resident in the forest's
 *   workspace until the forest's next match call; no host read per turn is added.
 *     A record is {u32 bytes, u16 frames, the game's INPUT battle (384 bytes; durations have no field, as in vs), result byte, updates}.
 *     Every turn that makes its update -- the turns turns_out counts -- adds one update to each seat's record, encoded as self-play's
 *     (selfplay_pick.hpp's encode_update, without contraction), both with the turn's JOINT choice (c1, c2).  A searched seat's update
 *     holds its own search's output: the root's m and n, its iterations, empirical_value, nash_value and both sides' Nash strategies (zeros
 *     without solve_nash), both sides' empirical strategies from process_output.  An unsearched seat's update (a seat with one choice) holds
 *     the real m and n, iterations = 0 and 0 for both values and all four strategies.  THIS DEPARTS FROM THE REFERENCE, which stores a
 *     value-initialised MCTS::Output there: its k = 0 makes the head byte 0xFF and the update 11 bytes long, which no reader can parse,
 *     the reference's own included (compressed-frame.h:99,126-127 reads it as m = n = 16).  The form here is well-formed: a loader's
 *     min_iterations filter skips it and a replay walks through it.  Both seats' updates of a turn have the same length, so the two
 *     streams share offsets and frame counts.
 *     An early-stop turn and a zeroed-policy turn add nothing.  Status OK: the record's result byte is the terminal byte.  EARLY_STOP: the
 *     frames up to the stop, result byte 1 or 2.  MAX_TURNS and ZERO_POLICY: NO record -- zero bytes in both streams, the frame count
 *     still reported -- as forest self-play drops its MAX_LENGTH / ZERO_POLICY games.  A game whose input result is terminal: a record
 *     with 0 frames.  Independence holds as stated above: game g's two records depend on its own inputs and the parameters only.
 *   oakgpu_forest_match_records copies seat `seat`'s (0 = p1, 1 = p2) stream of the forest's last match call out, with the shape and
 *   nullable-output rules of oakgpu_forest_selfplay_records: stream nullable (*bytes alone is the size query), offsets[n + 1],
 *   n_frames[n] (= turns_out), results[n], status[n] (OAKGPU_FM_*), to device memory with to_device != 0.  It fails by name when that
 *   call was made with recording off (or none was made), and for a seat outside 0 and 1. */
#define OAKGPU_FM_OK 0
#define OAKGPU_FM_MAX_TURNS 1
#define OAKGPU_FM_ZERO_POLICY 2
#define OAKGPU_FM_EARLY_STOP 3
typedef struct {
  oakgpu_search_params search; /* batch and seed are ignored (1, the turn's draw) */
  oakgpu_net *net;             /* required for eval = 1 / PUCB, else ignored */
  char policy_mode[16];
  double policy_temp, policy_min; /* policy_temp <= 0 means 1 */
} oakgpu_match_seat;
typedef struct {
  oakgpu_match_seat p1, p2;
  uint32_t max_turns;          /* updates per game before it is stopped (0 = 1000) */
  double early_stop;           /* 0 = off; the reference's default is 10.0 */
  uint32_t log_turns;          /* capacity of turn_log per game, 0 = no log */
  int32_t solve_nash;
} oakgpu_forest_match_params;
typedef struct { uint8_t c1, c2, m, n; uint32_t zero; double ev_p1, ev_p2; } oakgpu_match_turn;
int oakgpu_forest_match_check(uint32_t max_trees, uint32_t max_iterations, int contextual, const oakgpu_forest_match_params *params, uint32_t n);
int oakgpu_forest_match_dev(oakgpu_forest *forest, const oakgpu_forest_match_params *params, const uint8_t *battles, const uint8_t *durations,
                            const uint8_t *results_in, const uint64_t *seeds, uint32_t n, uint8_t *results_out, uint32_t *turns_out,
                            uint8_t *status_out, oakgpu_match_turn *turn_log, uint64_t counts_out[4]);
int oakgpu_forest_match(oakgpu_forest *forest, const oakgpu_forest_match_params *params, const uint8_t *battles, const uint8_t *durations,
                        const uint8_t *results_in, const uint64_t *seeds, uint32_t n, uint8_t *results_out, uint32_t *turns_out,
                        uint8_t *status_out, oakgpu_match_turn *turn_log, uint64_t counts_out[4]);
int oakgpu_forest_match_last_stats(const oakgpu_forest *forest, uint64_t out[4]);
int oakgpu_forest_match_set_records(oakgpu_forest *forest, int on);
int oakgpu_forest_match_records(oakgpu_forest *forest, int seat, uint8_t *stream, size_t capacity, size_t *bytes, uint64_t *offsets, uint32_t *n_frames,
                                uint8_t *results, uint8_t *status, int to_device);
int oakgpu_match_pick_host(int side, uint32_t m, uint32_t n, const uint64_t *visit_matrix, const double *value_matrix, uint64_t iterations,
                           const double *nash, const double *prior, const char *policy_mode, double policy_temp, double policy_min,
                           double early_stop, uint64_t *rng, double *policy, int32_t *index, double *empirical_value, int32_t *sign);

/* ---- batched PKMN::battle(p1, p2, seed) (pkmn.h:50-57, init.h:90-154), level 100 sets.
 * teams: n x 60 bytes; seeds: n x u64; with first_update != 0 also performs the opening
 * update(battle, 0, 0) (benchmark.cc:29) and writes its result byte. */
int oakgpu_init_battles_dev(oakgpu_ctx *ctx, const uint8_t *teams, const uint64_t *seeds, uint32_t n,
                            int first_update, uint8_t *battles, uint8_t *durations, uint8_t *results);
int oakgpu_init_battles(oakgpu_ctx *ctx, const uint8_t *teams, const uint64_t *seeds, uint32_t n,
                        int first_update, uint8_t *battles, uint8_t *durations, uint8_t *results);

/* ---- SURVEY 8(d) config-2 synthetic input: n random OU team pairs generated ON DEVICE.
 * Lane i: fast_prng::seed(state, seed0 + i); 2 x 6 distinct legal species, min(4, pool)
 * distinct moves each (legal[next32 % 149], pool[next32 % size], rejection on duplicates);
 * battle.rng = uniform_64(); opening update(0,0).  prng_state receives the continuing
 * stream.  ou_legal: 149 species ids; ou_pools: 152 x 48 move ids; ou_sizes: 152. */
int oakgpu_set_ou_pools(oakgpu_ctx *ctx, const uint8_t *ou_legal, int n_legal, const uint8_t *ou_pools,
                        const uint8_t *ou_sizes);
int oakgpu_random_ou_battles_dev(oakgpu_ctx *ctx, uint64_t seed0, uint32_t n, uint8_t *battles,
                                 uint8_t *durations, uint8_t *prng_state, uint8_t *results);

/* ---- leaf evaluator: replaces NN::Battle::NetworkImpl (cpp/include/nn/battle/network.h:22-176).
 * oakgpu_net_load parses a `.battle.net` parameter file exactly as the reference does (8-byte
 * header, byte 0 = activation - 1: cpp/src/search.cc:127-131; then 12 Affine blocks
 * `u32 in, u32 out, f32 bias[out], f32 W[out][in]`: nn/affine.h:35-70; must end at EOF:
 * network.h:60-63) and uploads the weights.  Errors (unreadable file, malformed / trailing
 * bytes, unsupported widths) return non-zero with a message, where the reference throws
 * std::runtime_error (search.cc:81,92,103,138,146).
 * oakgpu_leaf_eval* = value_inference(battle, durations) for n leaves (network.h:72-79):
 * encode + both embedding nets + MainNet value path + sigmoid, fp32 results throughout (the embedding nets' dense layers on
 * fp32 MFMA, the main net's as exact bf16 triples on the bf16 matrix pipe unless oakgpu_net_set_main_precision says
 * otherwise).  embedding_out (nullable): the n x in_dim battle embeddings (network.h:131-175). */
int oakgpu_net_load(oakgpu_ctx *ctx, const char *path, oakgpu_net **out);
int oakgpu_net_load_memory(oakgpu_ctx *ctx, const void *bytes, size_t size, oakgpu_net **out);
void oakgpu_net_free(oakgpu_ctx *ctx, oakgpu_net *net);
/* The quantized ("discrete") network: Agent.discrete (search.cc:100-147, nn/battle/quantized).  The file's header must encode
 * clamp activations; the main net must be 768-H-H-VH-1 with H, VH, PH in {32, 64, 128}, VH <= H, PH <= H; every main-net weight
 * strictly inside (-2, 2).  Failures carry the reference's texts ("Agent: .discrete was specified but ...", "Invalid layer size
 * for quantized net ...", "<i>non clamped<w>").  Main-net weights become int8 trunc(64 w), biases int32 trunc((64 b) 127); the
 * embedding nets stay fp32 (party slots evaluated with ReLU, the actives with clamp, as the reference's caches fill them).  The
 * leaf entry points (oakgpu_leaf_eval*, oakgpu_leaf_eval_policy*, oakgpu_leaf_eval_cached_dev) take such a handle: the
 * embedding becomes bytes static_cast<uint8_t>(127 f) and the main net runs in int32 on the i8 matrix pipe (k_mainnet_i8),
 * bit-exact to the reference's integer arithmetic; embedding_out stays the fp32 embedding before quantization. */
int oakgpu_net_load_discrete(oakgpu_ctx *ctx, const char *path, oakgpu_net **out);
int oakgpu_net_load_discrete_memory(oakgpu_ctx *ctx, const void *bytes, size_t size, oakgpu_net **out);
int oakgpu_net_is_discrete(const oakgpu_net *net);
/* Diagnostic: the quantized network's integer intermediates for n leaves -- q_embedding (n x 768 bytes, the main net's input)
 * and value_acc (n int32: value_fc3's output; value = sigmoid(value_acc / 8128)).  Device pointers; the network must be discrete. */
int oakgpu_leaf_eval_discrete_raw_dev(oakgpu_ctx *ctx, oakgpu_net *net, const uint8_t *battles, const uint8_t *durations, uint32_t n,
                                      uint8_t *q_embedding, int32_t *value_acc);
/* MainNet::shape() (main-net.h:32-34): fc0.in, fc0.out, value_fc2.out, p1_policy_fc2.out */
int oakgpu_net_shape(const oakgpu_net *net, int *in_dim, int *hidden, int *value_hidden, int *policy_hidden);
/* How the main net's three dense layers are multiplied (results are fp32 either way, held to the same 1e-5 against the
 * oracle and to 1e-6 against a float64 evaluation): OAKGPU_MAIN_PAIR (default since round 5) = every fp32 value times an exact
 * power of two (one per weight row = output feature, one per batch row for the activations) as the sum of two round-to-nearest fp16
 * parts, three fp16 MFMAs per multiply-add block, fp32 accumulation (k_mainnet_pair); OAKGPU_MAIN_SPLIT = every fp32 value as
 * an exact sum of three bf16 parts, six bf16 MFMAs per block (k_mainnet_split: 190-200 us per 65,536 leaves); OAKGPU_MAIN_FP32 =
 * fp32 MFMA (k_mainnet_wave: 336 us).  The environment variable OAKGPU_MAIN_NET=fp32 / bf16x3 makes one of the latter the
 * default of networks loaded after it is set.  Returns the previous mode, -1 on a bad argument. */
#define OAKGPU_MAIN_FP32 0
#define OAKGPU_MAIN_SPLIT 1
#define OAKGPU_MAIN_PAIR 2
#define OAKGPU_MAIN_INT8 3 /* a network of oakgpu_net_load_discrete*: reported only, never settable (set returns -1) */
int oakgpu_net_set_main_precision(oakgpu_net *net, int mode);
/* Edges of the bf16-triple form.  (1) A parameter file with a NaN / inf anywhere is REFUSED by oakgpu_net_load* ("non-finite
 * parameter ... in <layer>"); the reference loads it and propagates NaN (nn/affine.h:72-85 is a plain fp32 W x + b).  (2) A
 * triple carries a value to fp32 accuracy only while its low parts are normal bf16 numbers (|x| >= ~2^-102); what a flushed
 * part loses is at most 2^-126 per factor, harmless unless later layers multiply it back up.  So a network with a main-net
 * weight (fc0 / fc1 / value_fc2) above 2^20 in magnitude runs its main net on fp32 MFMA, and a request for OAKGPU_MAIN_SPLIT
 * is not honoured for it (tests/test_gpu_leafnet.py: layers scaled by 2^-100 / 2^-120 / 2^+100, alone and compensated).  The
 * embedding nets' passes multiply as bf16 triples as well; a weight above 2^20 in their second layers or in the main net sends them
 * through the fp32-MFMA form (k_embed_lds) instead.  (3) The fp16 pairs are scaled per weight row and per batch row, so no absolute
 * magnitude matters to them; what must hold is that every weight ROW survives the pairing to fp32 accuracy under its own scale (the
 * sum of what its pairs miss within 2^-23 of the sum of its magnitudes: only rows beyond 2^+-100 fail) and
 * that no non-zero weight COLUMN lies more than 2^18 below the layer's largest weight (a network that compensates tiny weights
 * with huge inputs is the same function in fp32 but not in a 5-bit exponent) -- a network that fails either runs on the triples, or
 * on fp32 MFMA by (2).  Returns the mode in effect (-1: null net); *split_allowed
 * (nullable) = 0 for a network of case (2). */
int oakgpu_net_main_precision(const oakgpu_net *net, int *split_allowed);
/* The policy heads (oakgpu_leaf_eval_policy*) follow rule (2) with a check of their own: their fc2 multiplies as bf16 triples beside a
 * main net on pairs or triples, and on fp32 MFMA beside a main net on fp32 MFMA -- or when ANY weight of the heads, fc2 or fc3, is
 * above 2^20 in magnitude, whatever the main net's mode.  fc3 counts because it is the later layer of (2): fc2 x 2^-120 in front
 * of fc3 x 2^+120 is the same function in fp32, but on the triples what fc2's low parts lose comes back multiplied up (measured
 * with fc2 alone checked: logits 2.3e-4 off at 2^+-120, still 3.3e-7 at 2^+-110 -- the bf16 pipe keeps subnormal parts;
 * tests/test_gpu_policy.py::test_compensated_heads).  Diagnostic: the form fc2 takes now (-1: null net). */
#define OAKGPU_POLICY_FORM_FP32 0
#define OAKGPU_POLICY_FORM_TRIPLE 1
#define OAKGPU_POLICY_FORM_INT8 2 /* a network of oakgpu_net_load_discrete*: k_policy_i8 */
int oakgpu_net_policy_form(const oakgpu_net *net);
int oakgpu_leaf_eval_dev(oakgpu_ctx *ctx, oakgpu_net *net, const uint8_t *battles, const uint8_t *durations,
                         uint32_t n, float *values, float *embedding_out);
int oakgpu_leaf_eval(oakgpu_ctx *ctx, oakgpu_net *net, const uint8_t *battles, const uint8_t *durations, uint32_t n,
                     float *values, float *embedding_out);

/* value_inference for a RESIDENT batch evaluated again and again (BASELINE configs[2]: every lane, every turn), with the
 * party-slot embeddings cached like NN::Battle::PokemonCache (nn/battle/cache.h:18-131, key encode/battle/key.h:65-71):
 * the caller keeps `embedding` (n x in_dim floats) and `slot_tags` (n x 10 x OAKGPU_SLOT_TAG_WORDS u32) between calls; a
 * bench slot is re-embedded only when what its embedding depends on changed -- the stored Pokemon's bytes with PP reduced
 * to has-PP bits and the status to its encoder index, compared exactly (no hashing).  Fill slot_tags with 0xFF bytes before
 * the first call; after that nothing needs resetting, not even when other battles are put into the lanes (a tag holds the
 * slot's whole identity).  Results are identical to oakgpu_leaf_eval_dev. */
#define OAKGPU_SLOT_TAG_WORDS 6
int oakgpu_leaf_eval_cached_dev(oakgpu_ctx *ctx, oakgpu_net *net, const uint8_t *battles, const uint8_t *durations, uint32_t n,
                                float *values, float *embedding, uint32_t *slot_tags);
/* Diagnostic (synchronises the context's stream): how many party slots the LAST oakgpu_leaf_eval_cached_dev call of this
 * context re-embedded (the cache misses of nn/battle/cache.h:81-126), of the n x 10 it looked at. */
int oakgpu_leaf_cache_last_count(oakgpu_ctx *ctx, uint32_t *slots_recomputed);
/* Diagnostic (read-only, no launch): the kernel each embedding pass of an oakgpu_leaf_eval*_dev call of this context would take
 * for this network now -- the routing leaf_eval_impl itself launches by (the network's widths, whether its embedding nets are
 * safe on the bf16 pipe, the context's kernel timing, the OAKGPU_EMBED_* environment).  The cached call runs the work-list
 * form of the same party kernel.  *party / *actives (nullable) = OAKGPU_EMBED_FORM_*, 0 where the pass is switched off;
 * *party_blocks (nullable) = the 32-wide output blocks each wave of the party row kernel computes (1 or 2), 0 for the tile form. */
#define OAKGPU_EMBED_FORM_TILE 1  /* k_embed_lds: 64-item tiles, fp32 MFMA */
#define OAKGPU_EMBED_FORM_ROWS 2  /* k_embed_prows / k_embed_arows, one launch each */
#define OAKGPU_EMBED_FORM_FUSED 3 /* k_embed_both: the two row kernels in one launch */
int oakgpu_leaf_embed_forms(oakgpu_ctx *ctx, const oakgpu_net *net, int *party, int *actives, int *party_blocks);

/* value_policy_inference (network.h:102-123): value plus, per side, the logits of the <= 9 legal choices
 * (choices n x 9 bytes + counts n bytes per side, as produced by oakgpu_choices*; logits n x 9 floats,
 * entries past the count are 0).  Choice -> policy row via Encode::Battle::Policy::get_index
 * (encode/battle/policy.h:29-58): move -> stored move id - 1, switch -> 164 + species - 1, pass -> 0. */
int oakgpu_leaf_eval_policy_dev(oakgpu_ctx *ctx, oakgpu_net *net, const uint8_t *battles, const uint8_t *durations,
                                uint32_t n, const uint8_t *p1_choices, const uint8_t *p1_counts,
                                const uint8_t *p2_choices, const uint8_t *p2_counts, float *values, float *p1_logits,
                                float *p2_logits);
int oakgpu_leaf_eval_policy(oakgpu_ctx *ctx, oakgpu_net *net, const uint8_t *battles, const uint8_t *durations, uint32_t n,
                            const uint8_t *p1_choices, const uint8_t *p1_counts, const uint8_t *p2_choices,
                            const uint8_t *p2_counts, float *values, float *p1_logits, float *p2_logits);

/* The bench-slot embedding table of a search: NN::Battle::PokemonCache (nn/battle/cache.h:18-131) as the reference uses it -- 240
 * embeddings (16 has-PP patterns x 15 status indices, key = Encode::Battle::pokemon_key, encode/battle/key.h:65-71) for each of the
 * 12 stored Pokemon of a ROOT battle, computed once, after which a leaf's ten bench slots are row copies and only its two actives
 * go through an embedding network.  A table holds up to max_roots roots and belongs to one network, which must outlive it (a quantized network's table
 * holds the ReLU embeddings its party slots take) and one device; any context of that device may fill or read it.
 *   fill: the 2,880 variants of every root through the party kernel's work-list form, in the form the plain call takes for this
 * network and context, so a row equals what oakgpu_leaf_eval_dev computes for that variant, bit for bit.  The device-pointer fill
 * is asynchronous on the context's stream (a table call on ANOTHER stream waits for it through an event; do not refill while other
 * streams still read) and, like every device array of battles in this header, wants root_battles aligned to 8 bytes (the kernels read
 * them two dwords at a time; any hipMalloc'd array of whole battles is); the host-pointer fill returns with the table complete.  A fill replaces all roots: n_roots in 1..max_roots.
 *   lookup (the two eval calls): oakgpu_leaf_eval_dev / oakgpu_leaf_eval_policy_dev with the party pass replaced.  Leaf i belongs to
 * root root_of[i] (device array of n; NULL = all root 0).  A live bench slot whose stored identity -- stats, move ids, species, types,
 * level -- equals the table's Pokemon at (root, side, team index) takes that Pokemon's row; any other live slot is embedded by the
 * work-list kernel as the cached call's changed slots are, so the results equal the plain call's for ANY leaf, descended from the
 * root or not.  A root_of entry beyond the filled roots is never followed: the leaf's slots are embedded as misses and the leaf is
 * counted (see the diagnostic).  Refused: null pointers, a table of another network or device, n_roots of 0 or above max_roots, an
 * eval before the first fill. */
typedef struct oakgpu_party_table oakgpu_party_table;
int oakgpu_party_table_create(oakgpu_ctx *ctx, oakgpu_net *net, uint32_t max_roots, oakgpu_party_table **out);
void oakgpu_party_table_destroy(oakgpu_ctx *ctx, oakgpu_party_table *table); /* synchronises the device; ctx may be NULL */
int oakgpu_party_table_fill_dev(oakgpu_ctx *ctx, oakgpu_party_table *table, const uint8_t *root_battles, uint32_t n_roots);
int oakgpu_party_table_fill(oakgpu_ctx *ctx, oakgpu_party_table *table, const uint8_t *root_battles, uint32_t n_roots);
int oakgpu_leaf_eval_table_dev(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_party_table *table, const uint32_t *root_of, const uint8_t *battles,
                               const uint8_t *durations, uint32_t n, float *values, float *embedding_out);
int oakgpu_leaf_eval_policy_table_dev(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_party_table *table, const uint32_t *root_of, const uint8_t *battles,
                                      const uint8_t *durations, uint32_t n, const uint8_t *p1_choices, const uint8_t *p1_counts,
                                      const uint8_t *p2_choices, const uint8_t *p2_counts, float *values, float *p1_logits, float *p2_logits);
/* The same two calls on host arrays (root_of too), staged like oakgpu_leaf_eval / oakgpu_leaf_eval_policy: PCIe-inclusive conveniences. */
int oakgpu_leaf_eval_table(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_party_table *table, const uint32_t *root_of, const uint8_t *battles,
                           const uint8_t *durations, uint32_t n, float *values, float *embedding_out);
int oakgpu_leaf_eval_policy_table(oakgpu_ctx *ctx, oakgpu_net *net, oakgpu_party_table *table, const uint32_t *root_of, const uint8_t *battles,
                                  const uint8_t *durations, uint32_t n, const uint8_t *p1_choices, const uint8_t *p1_counts,
                                  const uint8_t *p2_choices, const uint8_t *p2_counts, float *values, float *p1_logits, float *p2_logits);
/* Diagnostic (synchronises the context's stream): the bench slots the LAST table eval of this context found no row for and
 * embedded, of the n x 10 it looked at.  Fails, with the count in the message and *slots still set, when that call had root_of
 * entries beyond the filled roots.  Refused when the context's last work-list call was not an eval through this table (none yet, or
 * oakgpu_leaf_eval_cached_dev or a training-batch call since: they share the counters' memory). */
int oakgpu_party_table_last_misses(oakgpu_ctx *ctx, oakgpu_party_table *table, uint32_t *slots);
/* Diagnostic: the 240 rows (rows: host, 240 x the party embedding width, row = key) of Pokemon `pokemon` (0..5, team order) of
 * `side` (0, 1) of filled root `root`; the width itself (the party embedding net's output size; -1: null table). */
int oakgpu_party_table_rows(oakgpu_ctx *ctx, oakgpu_party_table *table, uint32_t root, int side, int pokemon, float *rows);
int oakgpu_party_table_width(const oakgpu_party_table *table);
/* Host only, no GPU: the key of a stored Pokemon (24 bytes) with its public sleep turns, and the variant the fill stores under a key
 * (`out`, `sleep` nullable; differs from `base` in the four PP bytes and the status byte only; non-zero for key >= 240) -- the
 * inline functions the kernels use. */
uint8_t oakgpu_party_key(const uint8_t pokemon[24], uint8_t sleep);
int oakgpu_party_variant(const uint8_t base[24], uint8_t key, uint8_t out[24], uint8_t *sleep);
/* The tree search (oakgpu_search, _search_heap, _search_agent(_heap), _search_many, oakgpu_selfplay_game(s)) with a network
 * evaluator, fp32 or quantized, on this context: on = 1 fills a one-root table from the search's root before the first batch and
 * sends the evaluation of every leaf batch through it (a contextual bandit's root priors, a batch of one before the table exists,
 * stay on the plain call).  No result changes (tests/test_gpu_party_table.py).  Returns the previous value; default 0, or 1 for
 * contexts created while OAKGPU_PARTY_TABLE=1 is set.  The diagnostic counts, since the context was created, the searches on it that
 * filled a table and the leaf batches they evaluated through one (fills, evals nullable). */
int oakgpu_set_search_party_table(oakgpu_ctx *ctx, int on);
int oakgpu_search_party_table_stats(oakgpu_ctx *ctx, uint64_t *fills, uint64_t *evals);

/* ---- Training the battle network: the optimiser step of the reference's `battle` program (src/oak/battle.py:203-262 around
 * BattleNetwork.inference, src/oak/torch.py:399-430) on rows 0 .. n-1 of an oakgpu_encoded_frames, the tensors oakgpu_frames_sample_dev
 * fills.  A TRAINER owns, for one network, the fp32 parameters of the 12 Affine blocks of a `.battle.net` (24 tensors in file order:
 * bias, then weight [out][in], per block), a gradient block and Adam's m and v of the same layout -- each `count` floats, the tensors
 * back to back -- and workspaces for up to max_rows rows.  It is made from the bytes of a `.battle.net`; header byte 0 gives the
 * activation (0 relu, 1 clamp[0,1]).  The widths are held to the loader's limits, so every trained network loads into the evaluators:
 * embedding widths <= 128, main / value / policy hidden <= 256, inputs 198 / 427, policy output 315, fc0's input = 2 x side.
 *   Forward, per row:  party = act(pokemon_net(pokemon[:, :, 1:6])) and active = act(active_net(cat(active[:, :, 0], pokemon[:, :, 0])))
 * -- both layers of an embedding net are activated -- each times (hp != 0) of its slot; side = [hp_0, active, 5 x (hp_slot, party_slot)];
 * h = act(fc1(act(fc0(cat(side_0, side_1))))); value = sigmoid(value_fc3(act(value_fc2(h)))); per side s, with q = act(policy_fc2_s(h)):
 * logit_i = policy_fc3_s(q)[choice_indices[s][i]] for i < k[s], and only those (an index outside 0 .. 314 names nothing: logit 0, no gradient;
 * k above 9 counts as 9).
 *   Loss: vt = (wn * nash_value + we * empirical_value) + ws * score;  sq_err = (value - vt)^2;  ce[s] = -sum_i t_i logp_i / max(1, #{t_i != 0})
 * with t = (1 - pn) * empirical + pn * nash and logp the log-softmax over the k legal logits (oakgpu_corpus_loss_dev's terms);
 * mse, ce_p1, ce_p2 = their means over the rows whose status is OK;  loss = value_weight * mse + policy_weight * (ce_p1 + ce_p2).  A row that
 * is not OK contributes nothing to any term or gradient whatever its other tensors hold (NaN included), its per-row outputs are 0.
 * value_weight == 0 && policy_weight == 0 is refused.
 *   Backward: the exact gradient of `loss`, with torch autograd's conventions at the kinks (relu: 0 at 0; clamp: 1 at both ends).  Every
 * sum over rows runs in a fixed order -- accumulation chains of 32 terms, their sums combined in a fixed order, no float
 * atomics -- so two calls on the same inputs give the same bits.
 *   Adam: torch.optim.Adam's defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay, bias correction): m = b1 m + (1-b1) g; v = b2 v +
 * (1-b2) g g; p -= [lr / (1 - b1^t)] * m / (sqrt(v) / sqrt(1 - b2^t) + eps), the two bracketed scalars computed on the host in double per
 * step and passed as floats; clamp_weights: the weights (not the biases) are clamped to [-2, 2] after the update.  Three parameter GROUPS,
 * each with its own step count t: TRUNK (both embedding nets, fc0, fc1), VALUE (value_fc2, value_fc3), POLICY (the four policy blocks).  A
 * group whose loss weight is zero receives no gradient: its gradients, parameters, m, v and t stay bit for bit as they are.
 *   A gradients / step call with no OK row: the report says rows = 0, the gradient block of the groups that receive one is zero, and
 * step's update does not happen: parameters, m and v stay as they are, and the groups' t are set back at the next oakgpu_trainer_report.
 *   The _dev calls take device rows and are asynchronous on the context's stream; nothing in a loop of steps waits for the device.  The report lives
 * in device memory; oakgpu_trainer_report copies it out and is the call that waits. */
/* battle.py's symmetries (permute_sides, permute_pokemon: it applies them to every batch unless told not to) on rows 0 .. n-1, in place, on the
 * device, asynchronous on the context's stream.  Row i draws from its own fast_prng stream seeded seed + i, as the sampler's draws do, so a row
 * does not depend on the batch: the first uniform_64 flips the sides when its lowest bit is set -- pokemon, active, hp, choice_indices, k,
 * empirical_policies and nash_policies swap along the side axis, empirical_value, nash_value and score become 1 - x; four more draws make a
 * Fisher-Yates permutation of the five bench slots (q = 4 .. 1: slot q <-> slot draw % (q + 1)), the same on both sides.  All five draws are
 * made whatever flip_sides / permute_bench switch off.  DEPARTURE from the reference: hp[:, :, 1:] moves with its Pokemon (src/oak/torch.py:30-35
 * leaves it in place, which pairs a Pokemon's embedding with another slot's hp and mask).  A row that is not OK is left as it is. */
int oakgpu_frames_symmetries_dev(oakgpu_ctx *ctx, const oakgpu_encoded_frames *rows, uint32_t n, uint64_t seed, int flip_sides, int permute_bench);
typedef struct oakgpu_trainer oakgpu_trainer;
typedef struct { float wn, we, ws, pn, value_weight, policy_weight; } oakgpu_train_loss;
typedef struct { double loss, mse, ce_p1, ce_p2; uint64_t rows; } oakgpu_train_report;
/* each nullable: value [n], logits [n,2,9] (0 behind the counts), sq_err [n], ce [n,2] */
typedef struct { float *value, *logits, *sq_err, *ce; } oakgpu_train_outputs;
enum { OAKGPU_TRAIN_PARAMETERS = 0, OAKGPU_TRAIN_GRADIENTS = 1, OAKGPU_TRAIN_M = 2, OAKGPU_TRAIN_V = 3 };
enum { OAKGPU_GROUP_TRUNK = 1, OAKGPU_GROUP_VALUE = 2, OAKGPU_GROUP_POLICY = 4 };
/* Host only, no GPU: every refusal of create (the file, max_rows) and of a call (n > max_rows; loss, nullable: both weights zero), by name. */
int oakgpu_trainer_check(const uint8_t *net, size_t size, uint32_t max_rows, uint32_t n, const oakgpu_train_loss *loss);
/* The trainer belongs to ctx and must be destroyed before it. */
int oakgpu_trainer_create(oakgpu_ctx *ctx, const uint8_t *net, size_t size, uint32_t max_rows, oakgpu_trainer **out);
void oakgpu_trainer_destroy(oakgpu_trainer *trainer);
/* dims (nullable): in, out of the 12 blocks; count (nullable): floats per block of parameters; max_rows (nullable). */
int oakgpu_trainer_shape(const oakgpu_trainer *trainer, uint32_t dims[24], size_t *count, uint32_t *max_rows);
/* forward + loss: the report and, where asked for, the per-row outputs.  No gradient, no parameter is touched. */
int oakgpu_trainer_forward_dev(oakgpu_ctx *ctx, oakgpu_trainer *trainer, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss,
                               const oakgpu_train_outputs *out /* nullable */);
/* forward + backward into the gradient block (and the report) */
int oakgpu_trainer_gradients_dev(oakgpu_ctx *ctx, oakgpu_trainer *trainer, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss);
/* the Adam update alone, from the gradient block as it stands, of the groups named (OAKGPU_GROUP_* or-ed); their t advance by one */
int oakgpu_trainer_adam_dev(oakgpu_ctx *ctx, oakgpu_trainer *trainer, float lr, int clamp_weights, uint32_t groups);
/* gradients, then adam of the groups whose loss weight is not zero */
int oakgpu_trainer_step_dev(oakgpu_ctx *ctx, oakgpu_trainer *trainer, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss, float lr,
                            int clamp_weights);
/* Waits for the stream.  out (nullable): the last forward / gradients / step call's report; steps (nullable): t of the three groups. */
int oakgpu_trainer_report(oakgpu_ctx *ctx, oakgpu_trainer *trainer, oakgpu_train_report *out, uint64_t steps[3]);
/* which = OAKGPU_TRAIN_*: `count` floats to the host, the 24 tensors in file order (waits for the stream) */
int oakgpu_trainer_read(oakgpu_ctx *ctx, oakgpu_trainer *trainer, int which, float *host, size_t count);
/* overwrites the gradient block from the host (the Adam update can then be run alone on any gradient) */
int oakgpu_trainer_set_gradients(oakgpu_ctx *ctx, oakgpu_trainer *trainer, const float *host, size_t count);
/* The parameters as `.battle.net` bytes: *size always; the bytes when out is not NULL and capacity >= *size.  Before any update these
 * are exactly the bytes the trainer was made from. */
int oakgpu_trainer_net_bytes(oakgpu_ctx *ctx, oakgpu_trainer *trainer, uint8_t *out, size_t capacity, size_t *size);
/* host rows in (staged), host outputs out; the calls return complete */
int oakgpu_trainer_forward(oakgpu_ctx *ctx, oakgpu_trainer *trainer, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss,
                           const oakgpu_train_outputs *out /* nullable */);
int oakgpu_trainer_gradients(oakgpu_ctx *ctx, oakgpu_trainer *trainer, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss);
int oakgpu_trainer_step(oakgpu_ctx *ctx, oakgpu_trainer *trainer, const oakgpu_encoded_frames *rows, uint32_t n, const oakgpu_train_loss *loss, float lr,
                        int clamp_weights);

/* ---- Team building: the other half of the reference's `generate` -- TeamBuilding::Provider::get_trajectory (cpp/include/util/team-building.h:
 * 190-241), which completes teams with the BUILD NETWORK one species or move at a time (rollout_build_network, :36-84), and the
 * CompressedTrajectory NoTeam records of `N.build.data` (encode/build/compressed-trajectory.h:23-105).
 *   A TEAM is 30 bytes, 6 x {species, 4 moves}, with a SIZE, the slots in play (the reference's vector length); slots at or beyond it are
 * not part of the team and come back as zeros.  A CELL is one (species, move) pair of Encode::Build::Tensorizer<Format::OU>: cells are
 * numbered in legal_species order, within a species the (species, None) cell first, then its move pool in pool order; there are
 * OAKGPU_BUILD_N_DIM of them.  The input x of the net has one float per cell.
 *   A `.build.net` is policy_net then value_net, each three Affine layers `u32 in_dim, u32 out_dim, out_dim f32 biases, out_dim x in_dim f32
 * weights row-major` (nn/affine.h:35-70); the policy net is n_dim -> h -> h -> n_dim with relu, relu, none (h <= 256 here), the value net
 * n_dim -> v -> v -> 1, read and unused as in the reference.
 *   THE ROLLOUT of one team, statement for statement the reference's: x = Tensorizer::write(team); the stream is splitmix64 (the self-play
 * pick's) seeded with the row's seed.  Loop: the LEGAL LIST (Actions::get_singleton_additions) -- if a slot below size is empty, every
 * legal species not on the team, in legal_species order, aimed at the FIRST empty slot; then, for each slot in order that holds a species
 * and has an empty move slot, its pool moves in pool order minus the moves it holds, aimed at its first empty move slot -- and an empty
 * list ends the loop.  One STEP: logits = policy_net(x); the softmax over the legal cells with expf in float, no maximum subtracted, the
 * sum accumulated in double in list order, each quotient rounded to float; index = sample_pdf(policy) with one uniform01, the list walked
 * sequentially with p -= (double)policy[i], p <= 0 stops, falling off the end gives 0; the action is applied; then x[index] = 1 -- the
 * POSITION in the list, not the action's cell: what the reference does (team-building.h:67) and what nets trained by build.py have seen
 * (input_update = 0).  input_update = 1 sets the action's own cell instead.  After the loop the slots 1 .. size-1 that hold a species are
 * the LEAD SWAPS (cell: (species, None)); if there are any, one more step over them swaps slot 0 with the chosen one.  At most
 * OAKGPU_BUILD_MAX_STEPS steps.
 *   Numerics: fp32 with fp32 accumulation in a fixed order (buildnet.hip's header); only W1's columns at the ones of x and W3's rows at the
 * legal cells are touched.  No float atomics: two calls give the same bits, and a row depends on its own team and seed alone.
 *   THE PROVIDER, per row from the row's stream in the reference's draw order: team_index = uniform_64 % T over a pool of T teams (their
 * Pokemon packed in the leading slots); truncation to max_pokemon, `changed` when that removed a Pokemon; one uniform, and only if it is
 * < team_modify_prob and changed is still false, Omitter::delete_info (per slot in order: a present species with u < pokemon_delete_prob
 * has its whole set cleared, no move draws for it; otherwise each present move with u < move_delete_prob is cleared).  Changed rows are
 * rolled out, the stream continuing; they report team_index -1.  The others keep their team, n_updates 0, and report their team_index.
 * The reference's team_shuffle_prob, which `generate` never sets, is left out.
 *   RECORDS: 128 bytes, {u8 format 0, u8 score = 2 * score or 255 for none, u16 value = value * 65535}, then 31 x {u16 action, u16
 * probability}: the INITIAL team's cells with probability 0 (per slot the species cell, then its held moves in slot order), then the
 * updates with probability = (u16)(65535.0f * p), 1 when a p != 0 rounds to 0, then zeros.  Only rows with n_updates > 0 give a record,
 * packed in row order.  A score that is negative or NaN means none.
 *   The _dev calls take device arrays, launch ONE kernel and are asynchronous on the context's stream; they trust the teams: a row whose
 * team would not pass oakgpu_build_teams_check is left with n_updates 255 and a zero team.  The host calls check first, stage, and return
 * complete; per-step entries at or past n_updates and trace entries past n_legal keep what the caller's arrays held. */
enum { OAKGPU_BUILD_N_DIM = 3749, OAKGPU_BUILD_MAX_ACTIONS = 339, OAKGPU_BUILD_MAX_STEPS = 31, OAKGPU_BUILD_RECORD_BYTES = 128 };
typedef struct oakgpu_build_net oakgpu_build_net;
typedef struct {
  uint8_t *teams_out;          /* [n, 30] */
  uint8_t *n_updates;          /* [n] */
  uint16_t *action;            /* [n, 31]: the cell of each step's action */
  uint16_t *index;             /* [n, 31]: its position in the legal list */
  uint16_t *n_legal;           /* [n, 31] */
  float *prob;                 /* [n, 31]: policy[index] */
  int16_t *trace_legal;        /* nullable, all three or none: [n, 31, 339] the legal cells, */
  float *trace_logits;         /*   their logits */
  float *trace_policy;         /*   and the policy */
  uint8_t *teams_init;         /* provide only: [n, 30] the team before the rollout (the record's initial team) */
  uint8_t *sizes_out;          /* provide only: [n] */
  int32_t *team_index;         /* provide only: [n] */
} oakgpu_build_outputs;
typedef struct { int32_t max_pokemon, input_update; double pokemon_delete_prob, move_delete_prob, team_modify_prob; } oakgpu_build_provider;
/* The generated tables (each nullable): legal_species [149]; cells [3749, 2] = species_move_list; table [152, 166] = species_move_table, -1
 * where there is no cell. */
int oakgpu_build_tables(uint8_t *legal_species, uint8_t *cells, int32_t *table);
/* Host only: refuses by name a truncated file, trailing bytes, dimensions that do not chain or do not start and end at n_dim, a NaN parameter. */
int oakgpu_build_net_check(const uint8_t *bytes, size_t len);
/* The net belongs to ctx and must be destroyed before it. */
int oakgpu_build_net_load(oakgpu_ctx *ctx, const uint8_t *bytes, size_t len, oakgpu_build_net **out);
void oakgpu_build_net_destroy(oakgpu_build_net *net);
int oakgpu_build_net_shape(const oakgpu_build_net *net, uint32_t *policy_hidden, uint32_t *value_hidden);
/* Host only, by name: n == 0, input_update outside {0, 1}, size > 6, a species outside legal_species, a duplicate species, a move outside its
 * species' pool.  sizes nullable: 6. */
int oakgpu_build_teams_check(const uint8_t *teams, const uint8_t *sizes, uint32_t n, int input_update);
/* Host only, by name: n == 0, an empty pool, max_pokemon outside 1..6, a probability outside [0, 1], and the pool's teams as above. */
int oakgpu_build_provide_check(const uint8_t *pool, uint32_t pool_n, uint32_t n, int max_pokemon, double pokemon_delete_prob, double move_delete_prob,
                               double team_modify_prob);
int oakgpu_build_rollout_dev(oakgpu_ctx *ctx, const oakgpu_build_net *net, const uint8_t *teams, const uint8_t *sizes /* nullable */, const uint64_t *seeds,
                             uint32_t n, int input_update, const oakgpu_build_outputs *out);
int oakgpu_build_provide_dev(oakgpu_ctx *ctx, const oakgpu_build_net *net, const uint8_t *pool, uint32_t pool_n, const uint64_t *seeds, uint32_t n,
                             const oakgpu_build_provider *prm, const oakgpu_build_outputs *out);
/* records: room for n x 128 bytes, 4-byte aligned; count: one device word, the number of records written */
int oakgpu_build_records_dev(oakgpu_ctx *ctx, const uint8_t *teams_init, const uint8_t *sizes /* nullable */, const uint8_t *n_updates, const uint16_t *action,
                             const float *prob, const float *value, const float *score, uint32_t n, uint8_t *records, uint32_t *count);
/* Both seats' records of a batch of self-play games, on the device (generate.cc:361-383): ONE launch, asynchronous on the context's stream.
 * p1 / p2: the seat's oakgpu_build_provide_dev outputs (n rows each; sizes nullable = 6); status / results / matchup: the game loop's
 * per-game outputs (oakgpu_forest_selfplay_records, _matchup), all device arrays.  A game with status OAKGPU_FSP_OK or _SKIPPED gives one
 * record per seat with n_updates > 0; a dropped or stopped game gives none.  Order: game-major, p1 before p2.  p1's value = (float)matchup,
 * p2's = (float)(1.0 - matchup); p1's score = PKMN::score(result) (win 1, lose 0, tie 0.5), p2's = 1 - it; a skipped game has no score
 * (byte 255).  The bytes are otherwise oakgpu_build_records' (one record writer).  records: room for 2 n x 128 bytes, 4-byte aligned, left
 * alone beyond the records written; count: one device word.
 * oakgpu_build_game_targets_host (no GPU) is the value / score rule alone: returns 1 when a game of this status gives records (then *value,
 * and *score, negative = none, are a `seat`'s, 0 = p1), 0 when it gives none, -1 for a refused argument. */
typedef struct {
  const uint8_t *teams_init, *sizes, *n_updates;
  const uint16_t *action;
  const float *prob;
} oakgpu_build_seat_arrays;
int oakgpu_build_game_records_dev(oakgpu_ctx *ctx, const oakgpu_build_seat_arrays *p1, const oakgpu_build_seat_arrays *p2, const uint8_t *status,
                                  const uint8_t *results, const double *matchup, uint32_t n, uint8_t *records, uint32_t *count);
int oakgpu_build_game_targets_host(int status, uint8_t result, double matchup, int seat, float *value, float *score);
/* host arrays in and out */
int oakgpu_build_rollout(oakgpu_ctx *ctx, const oakgpu_build_net *net, const uint8_t *teams, const uint8_t *sizes /* nullable */, const uint64_t *seeds,
                         uint32_t n, int input_update, const oakgpu_build_outputs *out);
int oakgpu_build_provide(oakgpu_ctx *ctx, const oakgpu_build_net *net, const uint8_t *pool, uint32_t pool_n, const uint64_t *seeds, uint32_t n,
                         const oakgpu_build_provider *prm, const oakgpu_build_outputs *out);
int oakgpu_build_records(oakgpu_ctx *ctx, const uint8_t *teams_init, const uint8_t *sizes /* nullable */, const uint8_t *n_updates, const uint16_t *action,
                         const float *prob, const float *value, const float *score, uint32_t n, uint8_t *records, uint32_t *count);

/* ---- Reading `.build.data` back: the reference's read_build_trajectories (cpp/src/pyoak.cc:247-329) with Py::Build::Trajectories::write
 * (cpp/include/py/build/trajectories.h:145-233), and the network-free half of build.py's process_targets (src/oak/build.py:119-129, 157-195).
 * The rule is one text for the host and the device, oak_amd/csrc/build_traj.hpp; the kernels are oak_amd/csrc/buildtraj.hip.  Decoding runs
 * on the GPU only; oakgpu_build_traj_check (statuses) is the one host form of the rule.
 *   THE RULE, per 128-byte NoTeam record.  start = the first i with probability != 0 (none: 0); end = the last such i + 1 (none: 0); swap =
 * end - 1 if the action at end - 1 is a (species, None) cell, else end; full = 1 + the last i < end - 1 with probability != 0 whose action is
 * a (species, None) cell (none: 0) -- as the loops of trajectories.h:159-187 take them.  A HELPER holds the team: sets in the order they were
 * added, each {species, counted moves, remaining pool}; a (species, None) action adds a set with the species' whole pool (a species already
 * in the team adds a second set), a (species, move) action takes the move out of the remaining pool of the FIRST set of that species and
 * counts it -- a move that is not in the remaining pool changes nothing.  A set is complete at 4 counted moves or an empty remaining pool.
 *   Steps i < start: action -1, policy 0, mask row all -1; the action is applied to the helper.  Steps start <= i < end: action = the
 * record's, policy = probability / 65535.0f (a correctly rounded float division); the mask row is, if i < swap, the (species, None) cells of
 * the legal species no set holds, in legal_species order, when i < full, then for each incomplete set in team order its remaining pool in
 * pool order; if i >= swap, every set's species cell in team order; the rest of the row is -1; the taken action is exchanged with entry 0;
 * then the action is applied UNLESS i == end - 1.  (The reference applies that one too, after the row is written and with no later reader;
 * on a team of six, where it is the lead swap, its helper writes a seventh set out of bounds.  Leaving it out gives the same arrays wherever
 * the reference is defined.)  Steps i >= end: action -1, policy 0, mask row all -1.
 *   value = header.value / 65535.0f.  score = header.score / 2.0 rounded to float; the reference compares the 8-bit score with 65,535, so a
 * record without a score (byte 255) reads as 127.5: no_score = 0 keeps that, no_score = 1 gives the -1 it meant.
 *   STATUS, one byte per record.  Where the reference asserts or runs out of bounds the record is not OK and is written as an ENDED
 * trajectory: every action -1, policy 0, mask -1, n_legal 0, start = end = 0; value and score are still decoded.  BAD_ACTION: the action of a
 * step below end is >= n_dim (looked for first).  Then in step order -- NO_SPECIES: a move of a species that is not in the team; TEAM_FULL: a
 * (species, None) action applied to six sets; NOT_LEGAL: the taken action is not in its own step's list (the reference would write -1 into
 * entry 0 and train on cell 0: the one place this deviates from a defined behaviour of the reference); LIST_OVERFLOW: a list longer than
 * 339 entries (only duplicate pre-start species reach it; the reference writes past the row).  BAD_PICK (255) is not a record's status: a
 * pick of a _dev call at or past the corpus' records reads nothing and gives an ended trajectory with value = score = 0.
 *   A CORPUS is the bytes of one or more files on the device, copied once.  DRAWS follow the reference's two-stage rule with a stream per
 * draw (oakgpu_frames_sample_dev's convention): draw i seeds fast_prng with seed + i; file = uniform_64 % n_files; record = uniform_64 %
 * records(file); with replacement, draw i does not depend on n; records that are not OK are drawn like any other and show in status.  A
 * PICK is a u32 global record index (the files' records in file order).
 *   TARGETS from the decoded arrays: valid = action != -1 && policy > 0; rows = the (b, t) of the valid steps in row-major order (torch's
 * x[valid]), compacted with game_rows.hpp's scan; the state of a valid step = the actions of the steps in front of it that are not -1, in
 * step order (get_state sees the trajectory's actions, not the initial team: pre-start steps are -1 and vanish) as state_cells / state_n, the
 * sparse form the rollout kernel's layer 1 consumes, padded with 65,535; old_logp = (float)log((double)policy): the device library's DOUBLE log (within 3 ulp
 * of double, OpenCL's bound for log) rounded to float once, so within 0.5 + 3 x 2^-29 ulp of float of the exact logarithm, and exactly 0 at
 * policy 1 -- the float logf of the same library promises 3 ulp and measures up to 1.9; rewards = value_weight * value + (1 - value_weight)
 * x score at end - 1 and 0 elsewhere, the difference in
 * double and both products and the sum rounded to float as torch computes build.py's line (a row with end == 0 is all 0).
 *   The _dev calls take device arrays and are asynchronous on the context's stream.  Every byte of every non-null output of rows 0 .. n-1 is
 * written (of the compacted arrays: of rows 0 .. n_valid-1), nothing outside them; two calls give the same bits; a row depends on its record
 * alone; no float atomics.  The host forms stage, refuse a pick outside the corpus by name, and return complete. */
enum { OAKGPU_BUILD_TRAJ_OK = 0, OAKGPU_BUILD_TRAJ_BAD_ACTION = 1, OAKGPU_BUILD_TRAJ_NO_SPECIES = 2, OAKGPU_BUILD_TRAJ_TEAM_FULL = 3,
       OAKGPU_BUILD_TRAJ_NOT_LEGAL = 4, OAKGPU_BUILD_TRAJ_LIST_OVERFLOW = 5, OAKGPU_BUILD_TRAJ_N_STATUS = 6, OAKGPU_BUILD_TRAJ_BAD_PICK = 255 };
enum { OAKGPU_BUILD_MASK_INT64 = 0 /* the reference's */, OAKGPU_BUILD_MASK_INT16 = 1 /* every value is -1 .. 3,748: a quarter of the bytes */ };
typedef struct oakgpu_build_corpus oakgpu_build_corpus;
typedef struct { uint32_t records, files, status_count[OAKGPU_BUILD_TRAJ_N_STATUS]; } oakgpu_build_corpus_stats;
typedef struct { int32_t mask_dtype, no_score; } oakgpu_build_traj_params;
typedef struct {             /* all nullable except status; a null mask makes the call cheap */
  int64_t *action;           /* [n, 31] */
  void *mask;                /* [n, 31, 339] int64 or int16 (mask_dtype), aligned to its entries */
  uint16_t *n_legal;         /* [n, 31]: the length of each step's list, 0 outside [start, end) */
  float *policy;             /* [n, 31] */
  float *value, *score;      /* [n] */
  int64_t *start, *end;      /* [n] */
  uint8_t *status;           /* [n] */
  uint32_t *t_max;           /* one word: max(end) */
} oakgpu_build_trajectories;
typedef struct {             /* all nullable except n_valid */
  uint8_t *valid;            /* [n, 31] */
  uint32_t *n_valid;         /* one word: V */
  uint32_t *rows;            /* [V, 2] (b, t); room for n x 31 rows, like the three below */
  uint16_t *state_cells;     /* [V, 31] */
  uint8_t *state_n;          /* [V] */
  float *old_logp;           /* [V] */
  float *rewards;            /* [n, 31] */
} oakgpu_build_target_outputs;
/* Host only, no GPU needed: the status of every record by the header's host form.  Refuses by name no records, a length that is not a
 * multiple of 128 and a record whose format byte is not 0. */
int oakgpu_build_traj_check(const uint8_t *bytes, size_t len, uint8_t *status_out);
/* buffer: the files' bytes one after the other; file_sizes [n_files] add up to size.  Refuses by name (before it looks at ctx) an empty
 * corpus, an empty file, a file size that is not a multiple of 128 and a record whose format byte is not 0, with the file and the record.
 * The corpus belongs to ctx and must be destroyed before it. */
int oakgpu_build_corpus_create(oakgpu_ctx *ctx, const uint8_t *buffer, size_t size, const size_t *file_sizes, uint32_t n_files, oakgpu_build_corpus **out);
void oakgpu_build_corpus_destroy(oakgpu_build_corpus *corpus);
/* ---- the build window: the newest max_records `.build.data` records resident on the device, appended to by self-play (buildwindow.hip;
 * the build side's counterpart of oakgpu_corpus_create_window).
 *   Contract.  After any sequence of appends, every corpus call on oakgpu_build_window_corpus(w) -- _scan_dev, _info, oakgpu_build_traj(_dev),
 *   oakgpu_build_traj_sample(_dev) -- returns bit for bit what it returns on oakgpu_build_corpus_create over the surviving records' bytes as
 *   ONE file, oldest first: the two-stage draw still draws the file (% 1), then the record.  The oldest records leave first; a batch larger
 *   than the window keeps its newest max_records; a record whose format byte is not 0 is rejected (counted, not appended); an append of 0
 *   records is a no-op.  A window that holds no record refuses the trajectory calls by name; its _info reports 0 records.
 *   _append_dev: records = max_count x 128 device bytes, 16-byte aligned; count = one device word (oakgpu_build_game_records_dev's), cut to
 *   max_count.  Two launches on the context's stream (an append that evicts compacts into the window's second buffer); the host waits for
 *   the stream ONCE and reads two words, the batch's accepted and rejected totals -- nothing in proportion to the window.  _append takes
 *   host bytes (a multiple of 128).  _corpus is BORROWED: it lives as long as the window and is not to be destroyed.  _records copies the
 *   held bytes to the host (out nullable: *bytes alone is the size query).  _stats: out = { records held, appended, evicted, rejected }
 *   since creation; appended counts every accepted record, evicted those that left or never fitted: held = appended - evicted.
 *   Refused by name: a null argument, max_records 0 or above 2^31 - 1, a window of another context, misaligned records, host bytes that are
 *   no multiple of 128. */
typedef struct oakgpu_build_window oakgpu_build_window;
int oakgpu_build_window_create(oakgpu_ctx *ctx, uint32_t max_records, oakgpu_build_window **out);
void oakgpu_build_window_destroy(oakgpu_build_window *window);
int oakgpu_build_window_append_dev(oakgpu_ctx *ctx, oakgpu_build_window *window, const uint8_t *records, const uint32_t *count, uint32_t max_count);
int oakgpu_build_window_append(oakgpu_ctx *ctx, oakgpu_build_window *window, const uint8_t *bytes, size_t len);
oakgpu_build_corpus *oakgpu_build_window_corpus(oakgpu_build_window *window);
int oakgpu_build_window_records(oakgpu_build_window *window, uint8_t *out, size_t capacity, size_t *bytes);
int oakgpu_build_window_stats(const oakgpu_build_window *window, uint64_t out[4]);
/* One lane per record: every record's status and the count per status, kept by the corpus (asynchronous). */
int oakgpu_build_corpus_scan_dev(oakgpu_ctx *ctx, oakgpu_build_corpus *corpus);
/* records, files and the count per status: of the last _scan_dev, or of a scan this call makes when there was none; synchronises once. */
int oakgpu_build_corpus_info(oakgpu_build_corpus *corpus, oakgpu_build_corpus_stats *info);
/* picks: n device words */
int oakgpu_build_traj_dev(oakgpu_ctx *ctx, const oakgpu_build_corpus *corpus, const uint32_t *picks, uint32_t n, const oakgpu_build_traj_params *params,
                          const oakgpu_build_trajectories *out);
/* picks_out: nullable, n device words */
int oakgpu_build_traj_sample_dev(oakgpu_ctx *ctx, oakgpu_build_corpus *corpus, uint32_t n, uint64_t seed, const oakgpu_build_traj_params *params,
                                 uint32_t *picks_out, const oakgpu_build_trajectories *out);
/* traj: action and policy (for rewards also value, score, end) of n decoded rows, device arrays */
int oakgpu_build_targets_dev(oakgpu_ctx *ctx, const oakgpu_build_trajectories *traj, uint32_t n, double value_weight, const oakgpu_build_target_outputs *out);
/* The dense 0/1 state of the valid rows lo .. hi-1 as f32 [hi - lo, 3749]: get_state(action)[valid][lo:hi], bit for bit. */
int oakgpu_build_state_dense_dev(oakgpu_ctx *ctx, const uint16_t *state_cells, const uint8_t *state_n, uint32_t lo, uint32_t hi, float *out);
/* host arrays in and out */
int oakgpu_build_traj(oakgpu_ctx *ctx, const oakgpu_build_corpus *corpus, const uint32_t *picks, uint32_t n, const oakgpu_build_traj_params *params,
                      const oakgpu_build_trajectories *out);
int oakgpu_build_traj_sample(oakgpu_ctx *ctx, oakgpu_build_corpus *corpus, uint32_t n, uint64_t seed, const oakgpu_build_traj_params *params,
                             uint32_t *picks_out, const oakgpu_build_trajectories *out);
int oakgpu_build_targets(oakgpu_ctx *ctx, const oakgpu_build_trajectories *traj, uint32_t n, double value_weight, const oakgpu_build_target_outputs *out);
int oakgpu_build_state_dense(oakgpu_ctx *ctx, const uint16_t *state_cells, const uint8_t *state_n, uint32_t lo, uint32_t hi, float *out);

/* ---- Training the build network: the optimiser step of the reference's `build` program (src/oak/build.py:153-251, 292-338) on the
 * device -- process_targets, compute_loss_from_targets, backward() per chunk, torch.optim.Adam and rolling_average.  The kernels are
 * oak_amd/csrc/buildtrain.hip; the two 31-step recursions are oak_amd/csrc/build_loss.hpp, one text for the host and the device.
 *   WHICH NETWORK.  The network trained is the one this library's rollout READS (NN::Build::Network, oakgpu_build_net_check): two nets of
 * three Affine blocks, policy 3749 -> h -> h -> 3749 (relu, relu, none) and value 3749 -> v1 -> v2 -> 1 (relu, relu, none, then sigmoid).
 * This deviates from build.py, which trains two-layer EmbeddingNets (torch.py:448-475) that the reference's own C++ reader cannot load.
 * Refused by name: whatever oakgpu_build_net_check refuses, and a value hidden width above 256.  v1 != v2 and ragged widths are allowed.
 *   A CHUNK is n decoded trajectories with their targets, all device arrays, untrimmed, as oakgpu_build_traj_dev and
 * oakgpu_build_targets_dev write them: mask (int64 or int16), n_legal, valid, rewards, and of the V = n_valid valid rows rows (b, t),
 * state_cells, state_n; a nullable keep u8 [V] (the caller's torch.rand(...) < keep_prob); the scalars gamma, gamma_lam (doubles, each
 * rounded to float once; gamma_lam is gamma * lam computed in double), the three loss weights, total (the batch size) and remaining.
 * old_logp is not read (the reference's ratio is commented out).
 *   THE RULE, for valid row i = (b, t) with state cells S_i (a cell counts once) and list L_i = mask[b, t, :n_legal[b, t]], entry 0 the
 * taken action:
 *     both nets: a1 = b1 + sum_{c in S_i} W1[:, c] (in the order of state_cells), h1 = relu(a1), h2 = relu(W2 h1 + b2)
 *     z_j = W3[L_j, :] . h2 + b3[L_j] at the legal cells only;  val_i = sigmoid(W3v . h2v + b3v)
 *     S = sum_j exp(z_j), NO maximum subtracted (torch.exp + normalize(p=1)); q_j = exp(z_j) / max(S, 1e-12); lp_i = log(q_0)
 *     value_full[b, t] = val at valid steps, 0 elsewhere;  delta = rewards + gamma value_full[b, t+1] - value_full[b, t]
 *     gae[b, t] = valid delta + gamma_lam gae[b, t+1] (t descending from 30, from 0);  ret = gae + value_full
 *     cf_i = [z_0 > -2] min(gae_i, 0) + [z_0 < 2] max(gae_i, 0), detached;  forced_i = z_0 cf_i
 *     k = sum keep (V when keep is null);  n_cap = min(k, remaining);  row i is SELECTED when it is kept and fewer than n_cap kept rows
 *     stand in front of it (the [:n] slices after x[mask]);  k == 0 adds nothing
 *     loss = (1 / total) sum_sel [ -pw forced_i + vw (ret_i - val_i)^2 + ew lp_i exp(lp_i) ]
 *   THE GRADIENT is exact, and gae is NOT detached inside ret (the value loss trains through the whole recursion; the direct paths through
 * value_full cancel).  With c = 1 / total and r_i = ret_i - val_i as computed in float:
 *     dL/dz_{i,j} = sel_i c [ -pw cf_i [j = 0] + ew q_{i,0} (1 + lp_i) ([j = 0] - q_{i,j}) ]      (S < 1e-12: the q_{i,j} term is 0)
 *     G[b, t] = sel 2 c vw r at valid rows, 0 elsewhere;  A[b, t] = G[b, t] + gamma_lam A[b, t-1] (t ascending);  D = valid A
 *     dL/dvalue_full[b, t] = -D[b, t] + gamma D[b, t-1], times val (1 - val) at valid rows: unselected valid rows receive value gradient too
 * then three layers per net; torch.relu has no gradient at 0.  An entry no row reaches (a W1 column whose cell is in no state; a W3 row
 * and b3 entry whose cell is in no selected row's list) is exactly unchanged by a call.
 *   ACCUMULATION.  _accumulate_dev forms the chunk's gradient on its own and adds it to the gradient block once per entry: after two
 * calls the block is bit for bit fl(g1 + g2).  _adam_dev is torch.optim.Adam's defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay)
 * over all twelve tensors as one group at a host-given lr; _average_dev is avg = avg g + (1 - g) p on a second parameter block that starts
 * equal to the initial parameters.
 *   NUMERICS.  fp32 throughout.  No float atomics: every sum runs in a fixed order that depends on the rows alone (dense products: k_gemm's
 * chains of 32 terms, 16 chains a middle sum; the transposed sparse products dW1 and dW3|db3: the entries of a cell in ascending entry
 * order, in pieces of OAKGPU_BUILD_TRAINER_SEGMENT entries summed in chains of 32, the pieces combined pairwise).  Two calls give the same
 * bits, and bits do not depend on the grid.  No workspace is allocated inside a call: capacities (31 max_traj rows, 339 x 31 max_traj list
 * entries) are fixed at create.  Every _dev call is asynchronous on the context's stream; _report is the only call that waits.
 *   _read / _set_gradients speak FILE ORDER: per layer the biases then the weights [out][in], policy net then value net -- a `.build.net`
 * without its dims. */
enum { OAKGPU_BUILD_TRAIN_PARAMETERS = 0, OAKGPU_BUILD_TRAIN_GRADIENTS = 1, OAKGPU_BUILD_TRAIN_M = 2, OAKGPU_BUILD_TRAIN_V = 3, OAKGPU_BUILD_TRAIN_AVERAGE = 4 };
enum { OAKGPU_BUILD_TRAINER_SEGMENT = 256, OAKGPU_BUILD_TRAINER_MAX_TRAJ = 32768 };
typedef struct oakgpu_build_trainer oakgpu_build_trainer;
typedef struct {
  const void *mask;             /* [n, 31, 339] int64 or int16 */
  int32_t mask_dtype;           /* OAKGPU_BUILD_MASK_INT64 / _INT16 */
  uint32_t n;                   /* trajectories */
  const uint16_t *n_legal;      /* [n, 31] */
  const uint8_t *valid;         /* [n, 31] */
  const float *rewards;         /* [n, 31] */
  uint32_t n_valid;             /* V, as the host knows it */
  const uint32_t *rows;         /* [V, 2] */
  const uint16_t *state_cells;  /* [V, 31] */
  const uint8_t *state_n;       /* [V] */
  const uint8_t *keep;          /* nullable [V] */
  double gamma, gamma_lam;
  float policy_loss_weight, value_loss_weight, entropy_loss_weight;
  uint32_t total, remaining;
} oakgpu_build_chunk;
typedef struct {                /* all nullable, per valid row */
  float *logits;                /* [V, 339], NaN beyond n_legal */
  float *value, *logp, *gae, *returns, *forced;   /* [V] */
  uint8_t *selected;            /* [V] */
  float *du;                    /* [V]: dL/d(the value net's output before the sigmoid), as the last call's weights and selection make it */
} oakgpu_build_train_outputs;
typedef struct {                /* of the last _forward_dev / _accumulate_dev: the means are over the n_cap selected rows */
  uint32_t rows, kept, n_cap, reserved;   /* V, k, n_cap */
  double policy_loss, value_loss, entropy, loss;
  uint64_t steps;               /* _adam_dev calls so far */
} oakgpu_build_train_report;
/* Host only, no GPU needed: the refusals of _create, by name. */
int oakgpu_build_trainer_check(const uint8_t *net, size_t size, uint32_t max_traj);
/* net: the bytes of a `.build.net`.  The trainer belongs to ctx and must be destroyed before it. */
int oakgpu_build_trainer_create(oakgpu_ctx *ctx, const uint8_t *net, size_t size, uint32_t max_traj, oakgpu_build_trainer **out);
void oakgpu_build_trainer_destroy(oakgpu_build_trainer *t);
/* dims: (in, out) of the six layers in file order; count: floats of one parameter block */
int oakgpu_build_trainer_shape(const oakgpu_build_trainer *t, uint32_t dims[12], size_t *count, uint32_t *max_traj);
int oakgpu_build_trainer_forward_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t, const oakgpu_build_chunk *chunk, const oakgpu_build_train_outputs *out /* nullable */);
int oakgpu_build_trainer_accumulate_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t, const oakgpu_build_chunk *chunk);
int oakgpu_build_trainer_zero_gradients_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t);
int oakgpu_build_trainer_adam_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t, float lr);
int oakgpu_build_trainer_average_dev(oakgpu_ctx *ctx, oakgpu_build_trainer *t, double g);
/* the only call that waits */
int oakgpu_build_trainer_report(oakgpu_ctx *ctx, oakgpu_build_trainer *t, oakgpu_build_train_report *out);
/* which: OAKGPU_BUILD_TRAIN_*; host: count floats in file order (these two wait for the copy) */
int oakgpu_build_trainer_read(oakgpu_ctx *ctx, oakgpu_build_trainer *t, int which, float *host, size_t count);
int oakgpu_build_trainer_set_gradients(oakgpu_ctx *ctx, oakgpu_build_trainer *t, const float *host, size_t count);
/* which: _PARAMETERS (the net) or _AVERAGE.  out null: *size alone.  The bytes pass oakgpu_build_net_check. */
int oakgpu_build_trainer_net_bytes(oakgpu_ctx *ctx, oakgpu_build_trainer *t, int which, uint8_t *out, size_t capacity, size_t *size);

#ifdef __cplusplus
}
#endif
#endif
