// oak_amd/csrc/oakgpu_internal.h -- shared between the translation units of liboakgpu.so.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/oakgpu.h"
struct oakgpu_ctx;
int oakgpu_fail_hip(int hip_error, const char *what); // records hipGetErrorString, returns the code
int oakgpu_fail_msg(const char *what);                 // records the message, returns -1
int oakgpu_ctx_device(const oakgpu_ctx *ctx);
// A failed HIP call ends the calling function with its code, recorded (oakgpu.hip replaces this form by one through its own fail())
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return oakgpu_fail_hip((int)_e, #x); } while (0)
template <class T>
int dev_alloc(T *&p, size_t count) { // hipMalloc of `count` elements (at least 16 bytes)
  HIPCHK(hipMalloc((void **)&p, std::max<size_t>(count * sizeof(T), 16)));
  return 0;
}
// One `.battle.data` record at the head of a buffer (selfplay.hip): OAKGPU_RECORD_OK, _MALFORMED (damaged inside its own length; *total
// is trustworthy) or _STOP (the length field is not).  *msg: oakgpu_frames_read's message.  _length checks the header only.
enum { OAKGPU_RECORD_OK = 0, OAKGPU_RECORD_MALFORMED = 1, OAKGPU_RECORD_STOP = 2 };
int oakgpu_record_scan(const uint8_t *buffer, size_t size, uint32_t *total, uint16_t *n_frames, const char **msg);
int oakgpu_record_scan_length(const uint8_t *buffer, size_t size, uint32_t *total, uint16_t *n_frames, const char **msg);
void *oakgpu_ctx_stream(const oakgpu_ctx *ctx);        // hipStream_t
int oakgpu_ctx_enter(oakgpu_ctx *ctx);                 // hipSetDevice(ctx->device): first line of every entry point that launches or allocates
// Per-context device workspaces (slot 0: battle embeddings, 1: policy activations, 2: party-slot work list): grow-only, one per context = one
// per stream, so two contexts evaluating the same network never share scratch memory.  nullptr on failure (error recorded).
void *oakgpu_ctx_workspace(oakgpu_ctx *ctx, int slot, size_t bytes);
// The whole-game loop's rows (policyplay.hip): one more grow-only block of the context, freed by oakgpu_destroy.  nullptr on failure.
void *oakgpu_ctx_games_workspace(oakgpu_ctx *ctx, size_t bytes);
// Staging buffers of the host-pointer entry points: a grow-only cache owned by the context (slot k of a call = the k-th
// buffer it asks for).  A HostCall brackets one host-pointer call: its destructor synchronises the context's stream on
// EVERY exit path, so no async copy to / from the caller's buffers is still in flight when the call returns.
void *oakgpu_stage_get(oakgpu_ctx *ctx, size_t bytes); // nullptr on failure (error recorded)
void oakgpu_stage_begin(oakgpu_ctx *ctx);
void oakgpu_stage_end(oakgpu_ctx *ctx);
struct OakHostCall {
  oakgpu_ctx *c;
  explicit OakHostCall(oakgpu_ctx *ctx) : c(ctx) { oakgpu_stage_begin(c); }
  ~OakHostCall() { oakgpu_stage_end(c); }
  void *get(size_t bytes) { return oakgpu_stage_get(c, bytes); }
};
// oakgpu.hip: k_replay_gather alone (aligned battles + first requests of n indexed records; `reports` = n x 2 dwords of scratch)
extern "C" int oakgpu_replay_gather_dev(oakgpu_ctx *ctx, const uint8_t *records, const uint64_t *offsets, const uint8_t *malformed, uint32_t n,
                                        uint8_t *aligned, uint8_t *first, uint32_t *reports);
extern "C" int oakgpu_leaf_set_lds_limits(void);                // leafnet.hip: per-device kernel attributes (called by oakgpu_create)
// Optional per-kernel timing of the leaf evaluator (oakgpu_set_kernel_timing): 4 events = before the party-slot
// embedding pass, before the actives' pass, before the main net, after it.  nullptr when timing is off.
void **oakgpu_ctx_timing_events(oakgpu_ctx *ctx);
// One opaque attachment per context, freed (through its destructor) by oakgpu_destroy before the context's own resources:
// the tree search keeps its batch slots (second context, device arrays, pinned mirrors) here between searches.
void *oakgpu_ctx_attachment(const oakgpu_ctx *ctx);
void oakgpu_ctx_set_attachment(oakgpu_ctx *ctx, void *p, void (*dtor)(void *));
// A caller that keeps several contexts busy at the same time (the tree search: two batches in flight) says so: launches that
// do not fill the device then run in regrouping rounds, whose dispatch boundaries let the other context's small kernels in.
// Returns the previous value.
int oakgpu_ctx_set_concurrent_hint(oakgpu_ctx *ctx, int on);
int oakgpu_ctx_search_party_table(const oakgpu_ctx *ctx); // oakgpu_set_search_party_table's switch
void oakgpu_ctx_count_search_table(oakgpu_ctx *ctx, uint64_t fills, uint64_t evals); // oakgpu_search_party_table_stats' counters
// Workspace 2's first words are the last work-list call's counters.  A table eval names its table as their owner once it has the block;
// any later oakgpu_ctx_workspace(ctx, 2, ...) -- the cached call, the training-batch call -- clears the owner again.
void oakgpu_ctx_set_ws2_owner(oakgpu_ctx *ctx, const void *table);
const void *oakgpu_ctx_ws2_owner(const oakgpu_ctx *ctx);
// leafnet.hip: whether the bench-slot table was made for this network (and not for one since freed at the same address)
struct oakgpu_party_table;
struct oakgpu_net;
extern "C" int oakgpu_party_table_is_for(const oakgpu_party_table *table, const oakgpu_net *net);
extern "C" int oakgpu_net_device(const oakgpu_net *net); // leafnet.hip: the device the weights live on (-1: null)
// Host threads of the tree walks started by the CALLING thread (0 = the default rule): callers that run several searches side
// by side -- oakgpu_search_many, oakgpu_selfplay_games -- give each its share of the cores.
void oakgpu_set_thread_search_threads(int threads);
// Cores the process may really use (affinity mask capped by the cgroup CPU quota; OAKGPU_SEARCH_CORES overrides): search_host.hip.
unsigned oakgpu_usable_cores();
// forest.hip: what the game loop over the forest (forestplay.hip) needs of a forest -- its context, its limits, and one attachment (the
// loop's workspace) that oakgpu_forest_destroy frees through `dtor` while the device is idle.
struct oakgpu_forest;
oakgpu_ctx *oakgpu_forest_ctx(const oakgpu_forest *forest);
void oakgpu_forest_limits(const oakgpu_forest *forest, uint32_t *max_trees, uint32_t *max_iterations, int *contextual);
// a kept forest (oakgpu_forest_create_kept) and, for the game loop's pick kernel, its per-tree device arrays: the last kept search's mismatch
// bytes and carried node counts, and the counter of dropped trees
int oakgpu_forest_is_kept(const oakgpu_forest *forest);
void oakgpu_forest_keep_arrays(const oakgpu_forest *forest, const uint8_t **mismatch, const uint32_t **carried, const uint32_t **dropped);
void *oakgpu_forest_attachment(const oakgpu_forest *forest);
void oakgpu_forest_set_attachment(oakgpu_forest *forest, void *p, void (*dtor)(void *));
// a second one of the same kind for the match loop (forestmatch.hip), so that one forest serves self-play and matches in turn
void *oakgpu_forest_match_attachment(const oakgpu_forest *forest);
void oakgpu_forest_set_match_attachment(oakgpu_forest *forest, void *p, void (*dtor)(void *));
// A resident `.battle.data` corpus (trainframes.hip creates and frees it; corpuseval.hip evaluates it chunk by chunk)
struct oakgpu_corpus {
  oakgpu_ctx *ctx = nullptr;
  uint32_t n = 0;
  oakgpu_corpus_stats info{};
  uint8_t *records = nullptr, *malformed = nullptr, *aligned = nullptr, *first = nullptr;
  uint64_t *offsets = nullptr;
  uint16_t *frames = nullptr;
  std::vector<uint16_t> h_frames;
  std::vector<uint8_t> h_malformed;
  // workspace of a batch of picks: grow-only
  uint32_t capacity = 0;
  uint32_t *picks = nullptr, *order = nullptr, *meta = nullptr, *heads = nullptr;
  uint32_t resident_waves = 0; // what the device holds of k_frames_pick: four waves per SIMD
  uint8_t *snap = nullptr;
  // sampling: valid-frame counts per min_iterations, eligible lists per (min_iterations, max_battle_length)
  struct Valid { uint32_t min_iterations; uint32_t *d; std::vector<uint32_t> h; };
  struct Eligible { uint32_t min_iterations, max_battle_length, count; uint32_t *d; const uint32_t *valid; };
  static constexpr size_t MAX_CACHED = 16; // eligible lists kept; one more filter pair empties both caches
  std::vector<Valid> valids;
  std::vector<Eligible> eligibles;
  // corpuseval.hip's workspace of a chunk of rows (freed through eval_free; the stream must be idle)
  void *eval = nullptr;
  void (*eval_free)(void *) = nullptr;
  // replaywindow.hip's half of a window corpus (oakgpu_corpus_create_window), null for a corpus made from a buffer: on such a corpus the
  // arrays above change with every append, and the sampler lists the eligible records on the device
  void *window = nullptr;
  void (*window_free)(void *) = nullptr;
};
// trainframes.hip: the sampling caches and the evaluation workspace of a corpus whose records have changed (the stream must be idle)
void oakgpu_corpus_drop_caches(oakgpu_corpus *corpus);
