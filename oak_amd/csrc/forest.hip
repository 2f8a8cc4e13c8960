// oak_amd/csrc/forest.hip -- the forest search: n independent tree searches at once, one lane per tree, every tree resident on the
// device (the contract is in include/oakgpu.h).
//
// search_host.hip parallelises INSIDE one tree: a batch of descents, a virtual loss to keep them apart, the tree on the host and a
// host round trip per level.  Here the parallelism is ACROSS trees: tree g is walked by lane g alone, exactly as the reference walks
// it (one descent at a time, mcts.h:250-447), and the n trees advance in lockstep, so the kernels under the search -- root prep
// (the rollout kernel with max_steps 0), oakgpu_tree_step_dev, the leaf evaluators -- each run over n rows per launch.  What is new
// here is small: the tree itself (node arena, edge table), the bandits (bandit.hpp, compiled for the device) and the back-up.
//
// Layout.  Tree g owns `arena` = max_iterations + 1 node records at nodes[g * arena ..] -- a node is bandit.hpp's two Bandits, 224
// bytes, array-of-structures: a lane touches ONE node per level and reads all of it (scores, priors, visits of both players), so a
// structure-of-arrays would turn one 224-byte run into 56 scattered dwords; trees are far apart either way.  A node id is its index in
// the tree's arena = its creation order, the root is 0.  Edges (parent, i, j, 16-byte observation) -> child live in the tree's own
// open-addressing table of `slots` = 2^k >= 2 * arena 32-byte slots (load <= 1/2, linear probing, every probe loop bounded by `slots`);
// a slot is live when its 16-bit stamp equals the call's, so a new call clears nothing (a real clear every 65,535 calls).  No lane ever
// touches another tree's arena or table: no atomics but the per-level live count, no waiting on another block.
//
// Schedule of one iteration: prep launch; k_forest_level(0) = selection at the root; then per level the tree step and
// k_forest_level(d), which resolves the edge just taken, selects at the child of a continuing lane (c1 / c2 = 0xFF for a finished
// one) and appends to the lane's path; the host reads that level's 4-byte live count and stops at 0.  Then the evaluator over all n
// rows and k_forest_backup: init (+ priors) of a new leaf, update along the path, the root matrices, the trace record.
//
// Kept forests (oakgpu_forest_create_kept; generate's --keep-node, Heap::update in search.cc:27-52).  Such a forest owns its node arenas
// and edge tables twice, front and back, with `arena` = keep_arena nodes per tree.  k_forest_advance, one wave per NEW tree t, reads tree
// src_tree[t] of the front copy and writes tree t of the back copy: the child along the played (i, j, observation) becomes node 0, its
// subtree is kept byte for byte, the rest is left behind; then front and back swap.  A node id is its creation order and a child is
// created after its parent, so once every node's parent is known (one scan of the tree's own table for live stamps) "is in the subtree"
// resolves in one ascending pass over ids, 64 at a time; the new id of a kept node is the count of kept nodes below it.  The kept edges
// are re-inserted with renumbered ends under a new stamp.  The kept form of the search (k_forest_begin with keep = 1) leaves an
// initialised root with the position's choice counts alone and runs on under the stamp the advance wrote.
//
// Per-tree budgets (oakgpu_forest_search_budgets*; self-play's fast searches).  Tree g runs budgets[g] iterations and must be, bit for bit, the
// tree of a call with that many.  Its last back-up marks it ST_DONE and writes its stream to the outputs, because the launches that still
// cover its row go on drawing from prng[g] (root prep, the Monte-Carlo evaluator).  A done tree is inert: k_forest_level(0) does not revive it
// and leaves c1 / c2 = 0xFF for the tree step, it is not counted live, and the back-up returns before it touches bandits, root matrices or
// trace.  The host knows the budgets (one copy, with the result bytes), so iteration t launches every kernel over rows [0, n_t) only, n_t = one
// past the last tree with budgets[g] > t; the path stride stays the call's n.  Budgets that do not increase in row order (the game loop's
// partition) therefore cost no launch over a finished tree.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

// select / update / the softmax must round as the host's do: c * prior * sqrtN + score fused into an FMA is another number
#pragma clang fp contract(off)

#include "../../include/oakgpu.h"
#include "oakgpu_internal.h"
#include "bandit.hpp"
#include "nash.hpp"
#include "selfplay_pick.hpp"

namespace {
using namespace oak_search;

struct FNode { Bandit p1, p2; };
static_assert(sizeof(Bandit) == sizeof(oakgpu_forest_bandit) && sizeof(FNode) == sizeof(oakgpu_forest_node), "oakgpu_forest_node mirrors the node record");
static_assert(offsetof(Bandit, priors) == offsetof(oakgpu_forest_bandit, priors) && offsetof(Bandit, visits) == offsetof(oakgpu_forest_bandit, visits) &&
              offsetof(Bandit, k) == offsetof(oakgpu_forest_bandit, k), "oakgpu_forest_bandit mirrors Bandit");
struct FEdge { uint64_t obs0, obs1; uint32_t parent, child; uint8_t i, j; uint16_t gen; };
static_assert(sizeof(FEdge) == 32, "one edge slot is 32 bytes");
static_assert(offsetof(FEdge, i) == 24 && offsetof(FEdge, j) == 25 && offsetof(FEdge, gen) == 26, "i, j and the stamp share the slot's dword 6");
static_assert(sizeof(oakgpu_forest_trace_head) == 88 && sizeof(oakgpu_forest_trace_level) == 8, "trace record layout");

// ST_DONE: a tree whose own budget is spent (the budgets calls): inert for the rest of the call -- it selects nothing, visits nothing, is not
// counted live and keeps c1 / c2 = 0xFF for the tree step -- where ST_DEAD is an error lane
enum : uint8_t { ST_WALK = 0, ST_TERMINAL = 1, ST_LEAF = 2, ST_DEAD = 3, ST_DONE = 4 };
enum : uint32_t { ERR_ARENA_FULL = 1, ERR_TABLE_FULL = 2 };
constexpr uint32_t NONE = OAKGPU_FOREST_NO_NODE;
constexpr int FBLOCK = 64;

struct ForestArgs {
  FNode *nodes;
  FEdge *edges;
  uint32_t arena, slots, gen, n;
  uint32_t stride;          // lanes per path level (= n)
  // per lane
  uint32_t *cur, *leaf, *levels, *n_nodes;
  uint8_t *status;
  uint32_t *path_node;      // [level][lane]
  uint8_t *path_i, *path_j; // [level][lane]
  // the tree step's arrays
  const uint8_t *results, *act, *ch1, *cnt1, *ch2, *cnt2, *root_ch1, *root_ch2;
  uint8_t *c1, *c2;
  uint32_t *ctl;            // [0]: sticky error word; [1 + d]: lanes that go on after k_forest_level(d)
  uint64_t *total_depth;
  BanditParams P;
  uint32_t max_depth;
};

__device__ __forceinline__ uint64_t edge_hash(uint32_t parent, uint32_t i, uint32_t j, uint64_t a, uint64_t b) {
  uint64_t h = (a ^ (uint64_t)parent * 0x9E3779B97F4A7C15ull) * 0xBF58476D1CE4E5B9ull;
  h = (h ^ (h >> 29) ^ b) * 0x94D049BB133111EBull;
  h = (h ^ (h >> 32) ^ (i | j << 8)) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 31);
}

// heap.children[{i, j, obs}] (mcts.h:359-361): the child along the edge, created (uninitialised) when absent.  NONE + the error
// word when the table or the arena is full; at most `slots` probes.
__device__ uint32_t edge_child(const ForestArgs &a, uint32_t lane, uint32_t parent, uint32_t i, uint32_t j, uint64_t o0, uint64_t o1) {
  FEdge *tab = a.edges + (size_t)lane * a.slots;
  const uint32_t mask = a.slots - 1;
  uint32_t s = (uint32_t)edge_hash(parent, i, j, o0, o1) & mask;
  for (uint32_t probe = 0; probe < a.slots; ++probe, s = (s + 1) & mask) {
    FEdge &e = tab[s];
    if (e.gen != (uint16_t)a.gen) {
      const uint32_t id = a.n_nodes[lane];
      if (id >= a.arena) { atomicOr(a.ctl, ERR_ARENA_FULL); return NONE; }
      e.obs0 = o0; e.obs1 = o1; e.parent = parent; e.child = id; e.i = (uint8_t)i; e.j = (uint8_t)j; e.gen = (uint16_t)a.gen;
      FNode &nd = a.nodes[(size_t)lane * a.arena + id];
      nd.p1.k = 0; nd.p2.k = 0;
      a.n_nodes[lane] = id + 1;
      return id;
    }
    if (e.parent == parent && e.i == i && e.j == j && e.obs0 == o0 && e.obs1 == o1) return e.child;
  }
  atomicOr(a.ctl, ERR_TABLE_FULL);
  return NONE;
}

// Level d of every tree: d = 0 selects at the root; d > 0 first resolves the edge that tree step d - 1 took.
__global__ __launch_bounds__(FBLOCK) void k_forest_level(ForestArgs a, uint32_t depth) {
  const uint32_t lane = blockIdx.x * FBLOCK + threadIdx.x;
  bool go = false;
  if (lane < a.n) {
    uint32_t node = 0;
    const uint8_t st = a.status[lane];
    if (depth == 0) {
      if (st != ST_DEAD && st != ST_DONE) { go = true; a.status[lane] = ST_WALK; a.levels[lane] = 0; }
      else { a.c1[lane] = 0xFF; a.c2[lane] = 0xFF; }
    } else if (st == ST_WALK) {
      if ((a.results[lane] & 15) != 0) { // terminal edge: the value comes from the result byte (mcts.h:427-441)
        a.status[lane] = ST_TERMINAL;
      } else {
        const size_t p = (size_t)(depth - 1) * a.stride + lane;
        const uint64_t *obs = (const uint64_t *)(a.act + (size_t)lane * 16);
        node = edge_child(a, lane, a.cur[lane], a.path_i[p], a.path_j[p], obs[0], obs[1]);
        if (node == NONE) a.status[lane] = ST_DEAD;
        else if (a.nodes[(size_t)lane * a.arena + node].p1.is_init() && depth < a.max_depth) go = true;
        else { a.status[lane] = ST_LEAF; a.leaf[lane] = node; } // first visit (or the depth cap): evaluate here (mcts.h:391-426)
      }
      if (!go) {
        a.levels[lane] = depth;
        if (node != NONE) a.total_depth[lane] += depth;
        a.c1[lane] = 0xFF; a.c2[lane] = 0xFF; // the tree step leaves the lane untouched from here on
      }
    }
    if (go) {
      FNode &nd = a.nodes[(size_t)lane * a.arena + node];
      float pr;
      const uint8_t i = nd.p1.select(a.P, [] { return 0.0; }, pr);
      const uint8_t j = nd.p2.select(a.P, [] { return 0.0; }, pr);
      nd.p1.visit(a.P, i);
      nd.p2.visit(a.P, j);
      a.c1[lane] = (depth == 0 ? a.root_ch1 : a.ch1)[(size_t)lane * 9 + i];
      a.c2[lane] = (depth == 0 ? a.root_ch2 : a.ch2)[(size_t)lane * 9 + j];
      const size_t p = (size_t)depth * a.stride + lane;
      a.path_node[p] = node; a.path_i[p] = i; a.path_j[p] = j;
      a.cur[lane] = node;
    }
  }
  const uint64_t going = __ballot(go);
  if (threadIdx.x == 0 && going) atomicAdd(a.ctl + 1 + depth, (uint32_t)__popcll(going));
}

struct BeginArgs {
  FNode *nodes;
  uint32_t arena, n, pucb;
  const uint64_t *seeds;
  const uint8_t *root_cnt1, *root_cnt2, *root_ch1, *root_ch2;
  const float *values, *l1, *l2;
  uint64_t *prng;
  uint32_t *n_nodes;
  uint8_t *status;
  uint64_t *total_depth;
  BanditParams P;
  oakgpu_forest_outputs out;
  // the kept form (keep = 1): trees below `valid` hold what the last advance or kept search left; the tree's table, to clear after a mismatch
  uint32_t keep, valid, slots, gen;
  FEdge *edges;
  uint8_t *mismatch;   // per tree: 1 = an initialised root with other choice counts than the position's (OAKGPU_E_ROOT_MISMATCH on the host)
  uint32_t *carried;   // per tree: nodes the call started with (0 = a fresh tree)
};

// Start of a call: the tree's stream (search_host.hip: slot 0, lane 0 -- the first splitmix64 output of the seed, never zero), the
// root's stats.init(m, n) + priors (mcts.h:177-210), the zeroed outputs.  The kept form (mcts.h:185-212, search_host.hip's heap): an
// initialised root with the position's m and n stays as it is with all its nodes, and the call's initial_value, logits and priors are
// zeros (no root inference ran); a root with other counts starts afresh after the lane has cleared its own tree's live slots.
__global__ __launch_bounds__(FBLOCK) void k_forest_begin(BeginArgs a) {
  const uint32_t lane = blockIdx.x * FBLOCK + threadIdx.x;
  if (lane >= a.n) return;
  uint64_t z = a.seeds[lane] + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  a.prng[lane] = (z ^ (z >> 31)) | 1;
  const uint8_t m = a.root_cnt1[lane], n = a.root_cnt2[lane];
  FNode &root = a.nodes[(size_t)lane * a.arena];
  bool fresh = true;
  if (a.keep) {
    uint8_t other = 0;
    uint32_t had = 0;
    if (lane < a.valid && a.n_nodes[lane] != 0 && root.p1.is_init()) {
      if (root.p1.k == m && root.p2.k == n) { fresh = false; had = a.n_nodes[lane]; }
      else {
        other = 1;
        FEdge *tab = a.edges + (size_t)lane * a.slots;
        for (uint32_t s = 0; s < a.slots; ++s) if (tab[s].gen == (uint16_t)a.gen) tab[s].gen = 0;
      }
    }
    a.mismatch[lane] = other;
    a.carried[lane] = had;
  }
  if (fresh) {
    root.p1.init(m, a.P.kind);
    root.p2.init(n, a.P.kind);
    a.n_nodes[lane] = 1;
  }
  a.status[lane] = ST_WALK;
  a.total_depth[lane] = 0;
  a.out.m[lane] = m; a.out.n[lane] = n;
  for (int q = 0; q < 9; ++q) { a.out.p1_choices[(size_t)lane * 9 + q] = a.root_ch1[(size_t)lane * 9 + q]; a.out.p2_choices[(size_t)lane * 9 + q] = a.root_ch2[(size_t)lane * 9 + q]; }
  for (int q = 0; q < 81; ++q) { a.out.visit_matrix[(size_t)lane * 81 + q] = 0; a.out.value_matrix[(size_t)lane * 81 + q] = 0.0; }
  double *lg[2] = {a.out.p1_logit + (size_t)lane * 9, a.out.p2_logit + (size_t)lane * 9}, *pr[2] = {a.out.p1_prior + (size_t)lane * 9, a.out.p2_prior + (size_t)lane * 9};
  for (int s = 0; s < 2; ++s) for (int q = 0; q < 9; ++q) { lg[s][q] = 0.0; pr[s][q] = 0.0; }
  a.out.initial_value[lane] = 0.0;
  if (a.pucb && fresh) {
    const float *l[2] = {a.l1 + (size_t)lane * 9, a.l2 + (size_t)lane * 9};
    root.p1.set_logits(a.P, l[0]);
    root.p2.set_logits(a.P, l[1]);
    a.out.initial_value[lane] = a.values[lane];
    for (int s = 0; s < 2; ++s) { // softmax(output.p1.prior, logits, k) into Output's doubles (search/util/softmax.h:5-15)
      const int k = s ? n : m;
      float sum = 0;
      for (int q = 0; q < k; ++q) { const float y = std::exp(l[s][q]); pr[s][q] = y; sum += y; lg[s][q] = l[s][q]; }
      for (int q = 0; q < k; ++q) pr[s][q] /= sum;
    }
  }
}

struct BackupArgs {
  FNode *nodes;
  uint32_t arena, n, stride, pucb, eval, iteration, iterations, trace_levels;
  const uint32_t *leaf, *levels, *path_node;
  uint8_t *status;
  const uint8_t *path_i, *path_j, *results, *cnt1, *cnt2;
  const float *values, *pe_root, *pe_score, *l1, *l2;
  uint64_t *visit_matrix;
  double *value_matrix;
  uint8_t *trace;
  BanditParams P;
  // the budgets calls (else null): tree g runs budgets[g] iterations; after its last one it is ST_DONE and its stream, which later launches
  // over its row would advance, goes to the outputs here
  const uint32_t *budgets;
  const uint64_t *prng;
  uint64_t *stream_out;
};

// End of an iteration: the leaf's init (+ set_logits) at its first evaluation, Bandit::update along the path, the root matrices.
__global__ __launch_bounds__(FBLOCK) void k_forest_backup(BackupArgs a) {
  const uint32_t lane = blockIdx.x * FBLOCK + threadIdx.x;
  if (lane >= a.n) return;
  const uint32_t budget = a.budgets ? a.budgets[lane] : a.iterations;
  if (a.iteration >= budget) return; // a finished tree inside the launch's rows: no update, no root cell, no trace record
  const uint8_t st = a.status[lane];
  const uint32_t L = st == ST_DEAD ? 0 : a.levels[lane];
  const uint32_t t = a.results[lane] & 15;
  float v1 = 0.5f;
  uint32_t leaf = NONE;
  uint8_t fresh = 0;
  FNode *tree = a.nodes + (size_t)lane * a.arena;
  if (st != ST_DEAD) {
    if (t != 0) v1 = t == 1 ? 1.0f : t == 2 ? 0.0f : 0.5f;
    else if (a.eval == 2) v1 = 1.0f / (1.0f + expf(-0.0125f * (a.pe_score[lane] - a.pe_root[lane]))); // k_poke_engine's scaled_sigmoid, per-tree root score
    else v1 = a.values[lane];
    if (st == ST_LEAF) {
      leaf = a.leaf[lane];
      FNode &lf = tree[leaf];
      if (!lf.p1.is_init() && a.cnt1[lane] && a.cnt2[lane]) {
        lf.p1.init(a.cnt1[lane], a.P.kind);
        lf.p2.init(a.cnt2[lane], a.P.kind);
        if (a.pucb) { lf.p1.set_logits(a.P, a.l1 + (size_t)lane * 9); lf.p2.set_logits(a.P, a.l2 + (size_t)lane * 9); }
        fresh = 1;
      }
    }
    for (uint32_t d = 0; d < L; ++d) {
      const size_t p = (size_t)d * a.stride + lane;
      FNode &nd = tree[a.path_node[p]];
      nd.p1.update(a.P, a.path_i[p], v1, 1.0f);
      nd.p2.update(a.P, a.path_j[p], 1.0f - v1, 1.0f);
    }
    if (L) {
      const uint32_t cell = a.path_i[lane] * 9 + a.path_j[lane];
      ++a.visit_matrix[(size_t)lane * 81 + cell];
      a.value_matrix[(size_t)lane * 81 + cell] += v1;
    }
  }
  if (a.trace) {
    const size_t rec = sizeof(oakgpu_forest_trace_head) + (size_t)a.trace_levels * sizeof(oakgpu_forest_trace_level);
    uint8_t *r = a.trace + ((size_t)lane * a.iterations + a.iteration) * rec;
    oakgpu_forest_trace_head h;
    h.levels = L; h.leaf = leaf; h.initialised = fresh; h.result_type = (uint8_t)t; h.pad[0] = h.pad[1] = 0; h.value = v1;
    for (int q = 0; q < 18; ++q) h.logits[q] = 0.0f;
    if (fresh && a.pucb) for (int q = 0; q < 9; ++q) { h.logits[q] = a.l1[(size_t)lane * 9 + q]; h.logits[9 + q] = a.l2[(size_t)lane * 9 + q]; }
    *(oakgpu_forest_trace_head *)r = h;
    oakgpu_forest_trace_level *lv = (oakgpu_forest_trace_level *)(r + sizeof h);
    for (uint32_t d = 0; d < a.trace_levels; ++d) {
      oakgpu_forest_trace_level x{0, 0, 0, {0, 0}};
      if (d < L) { const size_t p = (size_t)d * a.stride + lane; x.node = a.path_node[p]; x.i = a.path_i[p]; x.j = a.path_j[p]; }
      lv[d] = x;
    }
  }
  if (a.budgets && a.iteration + 1 == budget) {
    if (st != ST_DEAD) a.status[lane] = ST_DONE;
    a.stream_out[lane] = a.prng[lane];
  }
}

// budgets (nullable): the tree's own iteration count; its stream was written by its last back-up
__global__ __launch_bounds__(FBLOCK) void k_forest_finish(uint32_t n, uint64_t iterations, const uint32_t *n_nodes, const uint64_t *total_depth, const uint64_t *prng,
                                                          const uint32_t *budgets, oakgpu_forest_outputs out) {
  const uint32_t lane = blockIdx.x * FBLOCK + threadIdx.x;
  if (lane >= n) return;
  out.iterations[lane] = budgets ? (uint64_t)budgets[lane] : iterations;
  out.nodes[lane] = n_nodes[lane];
  out.total_depth[lane] = total_depth[lane];
  if (!budgets) out.stream[lane] = prng[lane];
}

struct AdvanceArgs {
  const FNode *src_nodes;      // the front copy: read only
  const FEdge *src_edges;
  const uint32_t *src_n_nodes;
  FNode *dst_nodes;            // the back copy: tree t is written by wave t alone
  FEdge *dst_edges;
  uint32_t *dst_n_nodes;
  uint32_t *map;               // [new tree][arena]: a node's parent, then its new id (NONE = left behind)
  const uint8_t *i, *j, *obs;  // per new tree: the played cell and the update's 16-byte observation
  const uint32_t *src_tree;    // per new tree: the front tree it continues; null = the same row
  uint8_t *kept_out;
  uint32_t *dropped;           // trees dropped for want of room, since the forest was made
  uint32_t arena, slots, gen_old, gen_new, n_new, valid, max_iterations;
};

// Heap::update(i, j, obs) of every tree (search.cc:27-52; oakgpu_heap_update's rule), and the move to another row: one wave per new tree.
// Every loop is bounded by `slots`, `arena` or 64; the only atomics are the wave's own claims of slots in its own back table (and the
// drop counter, when a tree is dropped).
__global__ __launch_bounds__(64) void k_forest_advance(AdvanceArgs a) {
  const uint32_t t = blockIdx.x, lane = threadIdx.x;
  if (t >= a.n_new) return;
  FNode *dn = a.dst_nodes + (size_t)t * a.arena;
  FEdge *dt = a.dst_edges + (size_t)t * a.slots;
  const uint32_t src = a.src_tree ? a.src_tree[t] : t;
  uint32_t nn = src < a.valid ? a.src_n_nodes[src] : 0; // 0: never searched
  if (nn > a.arena) nn = a.arena;
  const size_t from = src < a.valid ? src : 0;
  const FNode *sn = a.src_nodes + from * a.arena;
  const FEdge *st = a.src_edges + from * a.slots;
  const uint32_t mask = a.slots - 1;
  const uint16_t live = (uint16_t)a.gen_old, stamp = (uint16_t)a.gen_new;
  uint32_t child = NONE;
  if (nn != 0 && sn[0].p1.k != 0) { // the edge (root, i, j, obs), every lane the same probes
    const uint32_t i = a.i[t], j = a.j[t];
    uint64_t o0, o1;
    memcpy(&o0, a.obs + (size_t)t * 16, 8);
    memcpy(&o1, a.obs + (size_t)t * 16 + 8, 8);
    uint32_t s = (uint32_t)edge_hash(0, i, j, o0, o1) & mask;
    for (uint32_t probe = 0; probe < a.slots; ++probe, s = (s + 1) & mask) {
      const FEdge &e = st[s];
      if (e.gen != live) break;
      if (e.parent == 0 && e.i == i && e.j == j && e.obs0 == o0 && e.obs1 == o1) { child = e.child; break; }
    }
    if (child == 0 || child >= nn) child = NONE;
  }
  child = __builtin_amdgcn_readfirstlane(child); // (the same in every lane: the barriers below are reached by all or none)
  uint32_t kept = 0;
  if (child != NONE) {
    uint32_t *map = a.map + (size_t)t * a.arena;
    for (uint32_t id = lane; id < nn; id += 64) map[id] = NONE;
    __syncthreads();
    for (uint32_t s = lane; s < a.slots; s += 64) { // every node but the root is the child of exactly one live edge
      const FEdge &e = st[s];
      if (e.gen == live && e.child < nn) map[e.child] = e.parent;
    }
    __syncthreads();
    // ascending over ids from the child on, 64 at a time: kept = the parent is kept.  A parent in an earlier chunk is read from the map (it
    // holds new ids there already); a parent in the same chunk sits in a lower lane and is reached by pointer jumping, 6 rounds for 64 lanes.
    for (uint32_t base = child; base < nn; base += 64) {
      const uint32_t id = base + lane;
      const bool in = id < nn;
      const uint32_t p = in ? map[id] : NONE;
      int state = 0; // 0 left behind, 1 kept, 2 waits for a lower lane
      uint32_t anc = 0;
      if (in) {
        if (id == child) state = 1;
        else if (p == NONE || p < child || p >= id) state = 0;
        else if (p == child) state = 1;
        else if (p < base) state = map[p] != NONE;
        else { state = 2; anc = p - base; }
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const int s2 = __shfl(state, (int)anc);
        const uint32_t a2 = __shfl(anc, (int)anc);
        if (state == 2) { if (s2 != 2) state = s2; else anc = a2; }
      }
      const bool k = state == 1;
      const unsigned long long m = __ballot(k);
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (in) map[id] = k ? kept + below : NONE;
      kept += (uint32_t)__popcll(m);
      __syncthreads();
    }
  }
  // room for a whole call below the kept nodes, or the tree is dropped (the host's heap is unbounded: the one departure from it)
  const bool drop = child != NONE && (uint64_t)kept + a.max_iterations > a.arena;
  const bool keep = child != NONE && !drop;
  if (keep) {
    const uint32_t *map = a.map + (size_t)t * a.arena;
    for (uint32_t base = child; base < nn; base += 64) { // the records, 14 x 16 bytes each, 64 nodes a round
      const uint32_t id = base + lane;
      const uint32_t to = id < nn ? map[id] : NONE;
#pragma unroll 2
      for (uint32_t q = 0; q < 14; ++q) {
        const uint32_t idx = q * 64 + lane, node = idx / 14, part = idx - node * 14;
        const uint32_t dst = __shfl(to, (int)node);
        if (dst != NONE) ((uint4 *)(dn + dst))[part] = ((const uint4 *)(sn + base + node))[part];
      }
    }
    for (uint32_t s0 = lane; s0 < a.slots; s0 += 64) { // the edges between kept nodes, renumbered, under the new stamp
      const FEdge e = st[s0];
      if (e.gen != live || e.child >= nn || e.child <= child || e.parent < child || e.parent >= e.child) continue;
      const uint32_t nc = map[e.child], np = map[e.parent];
      if (nc == NONE || np == NONE) continue;
      const uint32_t word = (uint32_t)e.i | (uint32_t)e.j << 8 | (uint32_t)stamp << 16; // i, j, gen: one dword of the slot, claimed as one
      uint32_t s = (uint32_t)edge_hash(np, e.i, e.j, e.obs0, e.obs1) & mask;
      for (uint32_t probe = 0; probe < a.slots; ++probe, s = (s + 1) & mask) {
        uint32_t *w = (uint32_t *)(dt + s) + offsetof(FEdge, i) / 4;
        const uint32_t seen = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint16_t)(seen >> 16) == stamp) continue; // taken by another lane of this wave
        if (atomicCAS(w, seen, word) != seen) continue; // lost the slot to one
        FEdge &d = dt[s];
        d.obs0 = e.obs0; d.obs1 = e.obs1; d.parent = np; d.child = nc;
        break;
      }
    }
  }
  if (lane == 0) {
    if (!keep) { dn[0].p1.k = 0; dn[0].p2.k = 0; } // `node = {}`: an empty tree, the next search initialises its root
    a.dst_n_nodes[t] = keep ? kept : 1;
    a.kept_out[t] = keep ? 1 : 0;
    if (drop) atomicAdd(a.dropped, 1u);
  }
}

#define RC(x) do { int _r = (x); if (_r) return _r; } while (0)
} // namespace

struct oakgpu_forest {
  oakgpu_ctx *ctx = nullptr;
  int device = 0;
  uint32_t max_trees = 0, max_iterations = 0, arena = 0, slots = 0, gen = 0, last_n = 0;
  bool contextual = false;
  std::vector<void *> dev;
  FNode *nodes = nullptr;
  FEdge *edges = nullptr;
  uint8_t *b = nullptr, *d = nullptr, *r = nullptr, *c1 = nullptr, *c2 = nullptr, *act = nullptr, *ch1 = nullptr, *cnt1 = nullptr, *ch2 = nullptr, *cnt2 = nullptr,
          *rout = nullptr, *root_ch1 = nullptr, *root_cnt1 = nullptr, *root_ch2 = nullptr, *root_cnt2 = nullptr, *status = nullptr;
  uint64_t *prng = nullptr, *total_depth = nullptr;
  uint32_t *steps = nullptr, *cur = nullptr, *leaf = nullptr, *levels = nullptr, *n_nodes = nullptr, *ctl = nullptr;
  float *values = nullptr, *l1 = nullptr, *l2 = nullptr, *pe_root = nullptr, *pe_score = nullptr;
  // the lanes' paths, [level][lane], and the control words (error word + one live count per level): grow-only, sized by the deepest max_depth asked for
  uint32_t path_levels = 0;
  uint32_t *path_node = nullptr;
  uint8_t *path_i = nullptr, *path_j = nullptr;
  uint32_t *h_live = nullptr; // pinned
  // the host-array call's staging (made by its first use)
  uint8_t *stage = nullptr, *trace_stage = nullptr;
  size_t trace_stage_bytes = 0;
  uint64_t stats[4] = {0, 0, 0, 0};
  uint64_t rows[2] = {0, 0};  // the last search's tree-iterations: launched (the sum of the iterations' row counts) and run (the sum of the budgets)
  uint32_t *budget_stage = nullptr; // the host-array budgets calls' staging (made by their first use)
  // a kept forest (oakgpu_forest_create_kept): the back copy of arenas, tables and node counts that k_forest_advance writes and that then
  // becomes the front (nodes / edges / n_nodes above); `valid` = the trees of the front copy that hold what a call left
  bool kept = false;
  FNode *nodes_back = nullptr;
  FEdge *edges_back = nullptr;
  uint32_t *n_nodes_back = nullptr, *map = nullptr, *carried = nullptr, *dropped = nullptr, *adv_src = nullptr;
  uint8_t *mismatch = nullptr, *adv_in = nullptr;
  uint32_t valid = 0;
  uint64_t advances = 0;
  // the game loop's workspace (forestplay.hip), freed with the forest
  void *attachment = nullptr;
  void (*attachment_free)(void *) = nullptr;
  // the match loop's (forestmatch.hip), likewise
  void *match_attachment = nullptr;
  void (*match_attachment_free)(void *) = nullptr;
  template <class T> int get(T *&p, size_t count) {
    RC(dev_alloc(p, count));
    dev.push_back(p);
    return 0;
  }
  void release() {
    if (attachment && attachment_free) attachment_free(attachment);
    attachment = nullptr;
    if (match_attachment && match_attachment_free) match_attachment_free(match_attachment);
    match_attachment = nullptr;
    for (void *p : dev) (void)hipFree(p);
    dev.clear();
    if (path_node) (void)hipFree(path_node);
    if (path_i) (void)hipFree(path_i);
    if (path_j) (void)hipFree(path_j);
    if (ctl) (void)hipFree(ctl);
    if (stage) (void)hipFree(stage);
    if (trace_stage) (void)hipFree(trace_stage);
    if (budget_stage) (void)hipFree(budget_stage);
    if (h_live) (void)hipHostFree(h_live);
  }
};

namespace {
// bytes of one tree's outputs in the host-array call's staging block, every array 8-byte aligned for any n
constexpr size_t OUT_BYTES = 8 + 8 + 16 + 16 + 81 * 8 + 81 * 8 + 3 * 8 + 8 + 4 * 72 + 8;
constexpr size_t IN_BYTES = 384 + 8 + 8 + 8;

void carve_outputs(uint8_t *p, size_t n, oakgpu_forest_outputs *o) {
  auto take = [&](size_t bytes_per) { uint8_t *q = p; p += ((bytes_per * n + 15) / 16) * 16; return q; };
  o->visit_matrix = (uint64_t *)take(81 * 8); o->value_matrix = (double *)take(81 * 8);
  o->iterations = (uint64_t *)take(8); o->nodes = (uint64_t *)take(8); o->total_depth = (uint64_t *)take(8);
  o->initial_value = (double *)take(8);
  o->p1_logit = (double *)take(72); o->p2_logit = (double *)take(72); o->p1_prior = (double *)take(72); o->p2_prior = (double *)take(72);
  o->stream = (uint64_t *)take(8);
  o->p1_choices = take(9); o->p2_choices = take(9); o->m = take(1); o->n = take(1);
}
size_t outputs_bytes(size_t n) { return OUT_BYTES * n + 16 * 16; }
} // namespace

oakgpu_ctx *oakgpu_forest_ctx(const oakgpu_forest *f) { return f->ctx; }
void oakgpu_forest_limits(const oakgpu_forest *f, uint32_t *max_trees, uint32_t *max_iterations, int *contextual) {
  *max_trees = f->max_trees; *max_iterations = f->max_iterations; *contextual = f->contextual ? 1 : 0;
}
int oakgpu_forest_is_kept(const oakgpu_forest *f) { return f->kept ? 1 : 0; }
void oakgpu_forest_keep_arrays(const oakgpu_forest *f, const uint8_t **mismatch, const uint32_t **carried, const uint32_t **dropped) {
  *mismatch = f->mismatch; *carried = f->carried; *dropped = f->dropped;
}
void *oakgpu_forest_attachment(const oakgpu_forest *f) { return f->attachment; }
void oakgpu_forest_set_attachment(oakgpu_forest *f, void *p, void (*dtor)(void *)) { f->attachment = p; f->attachment_free = dtor; }
void *oakgpu_forest_match_attachment(const oakgpu_forest *f) { return f->match_attachment; }
void oakgpu_forest_set_match_attachment(oakgpu_forest *f, void *p, void (*dtor)(void *)) { f->match_attachment = p; f->match_attachment_free = dtor; }

extern "C" {

int oakgpu_forest_check(uint32_t max_trees, uint32_t max_iterations, int contextual, const oakgpu_search_params *prm, int has_net, uint32_t n,
                        const uint8_t *results, int has_trace, uint32_t trace_levels) {
  if (!prm) return oakgpu_fail_msg("oakgpu_forest_search: null argument");
  if (prm->duration_us != 0) return oakgpu_fail_msg("oakgpu_forest_search: time budgets are not supported (every tree runs the same number of iterations)");
  if (prm->matrix_ucb) return oakgpu_fail_msg("oakgpu_forest_search: matrix_ucb is not supported");
  if (prm->bandit < 0 || prm->bandit > 4 || prm->eval < 0 || prm->eval > 2) return oakgpu_fail_msg("oakgpu_forest_search: unknown bandit / eval");
  if (prm->bandit >= 2) {
    static const char *names[5] = {"UCB", "PUCB", "UCB1", "Exp3", "PExp3"};
    return oakgpu_fail_msg((std::string("oakgpu_forest_search: the ") + names[prm->bandit] + " bandit is not supported (UCB and PUCB are)").c_str());
  }
  const bool pucb = prm->bandit == B_PUCB;
  if ((prm->eval == 1 || pucb) && !has_net) return oakgpu_fail_msg("oakgpu_forest_search: network evaluation / PUCB priors need a network");
  if (pucb && prm->eval != 1) return oakgpu_fail_msg("oakgpu_forest_search: PUCB takes its priors from the network evaluator (eval = 1)");
  if (pucb && !contextual) return oakgpu_fail_msg("oakgpu_forest_search: PUCB needs a forest created contextual");
  auto rolls_ok = [](uint32_t r) { return r == 1 || r == 2 || r == 3 || r == 20 || r == 39; };
  if (!rolls_ok(prm->root_rolls) || !rolls_ok(prm->other_rolls)) return oakgpu_fail_msg("oakgpu_forest_search: rolls must be 1, 2, 3, 20 or 39");
  if (prm->iterations == 0) return oakgpu_fail_msg("oakgpu_forest_search: give an iteration budget");
  if (prm->iterations > max_iterations) return oakgpu_fail_msg("oakgpu_forest_search: iterations exceed the forest's max_iterations");
  if (n > max_trees) return oakgpu_fail_msg("oakgpu_forest_search: n exceeds the forest's max_trees");
  const uint32_t max_depth = prm->max_depth ? prm->max_depth : 100;
  if (has_trace && trace_levels < max_depth) return oakgpu_fail_msg("oakgpu_forest_search: trace_levels must be at least max_depth (0 = 100)");
  if (results)
    for (uint32_t g = 0; g < n; ++g)
      if ((results[g] & 15) != 0) return oakgpu_fail_msg(("oakgpu_forest_search: the root position of tree " + std::to_string(g) + " is terminal").c_str());
  return 0;
}

static uint32_t forest_slots(uint32_t arena) {
  uint32_t slots = 16;
  while (slots < 2 * arena) slots *= 2;
  return slots;
}

uint64_t oakgpu_forest_kept_tree_bytes(uint32_t max_iterations, uint32_t keep_arena) {
  if (max_iterations == 0 || max_iterations > (1u << 24)) return 0;
  if (keep_arena == 0) keep_arena = 4 * max_iterations + 1;
  if (keep_arena < max_iterations + 1 || keep_arena > (1u << 27)) return 0;
  return 2 * ((uint64_t)keep_arena * sizeof(FNode) + (uint64_t)forest_slots(keep_arena) * sizeof(FEdge));
}

// both creates: arena = 0 makes the plain forest (max_iterations + 1 nodes a tree, one copy), else a kept one of `arena` nodes a tree, two copies
static int forest_make(const char *who, oakgpu_ctx *ctx, uint32_t max_trees, uint32_t max_iterations, int contextual, uint32_t keep_arena, oakgpu_forest **out) {
  RC(oakgpu_ctx_enter(ctx));
  oakgpu_forest *f = new oakgpu_forest();
  f->ctx = ctx; f->device = oakgpu_ctx_device(ctx); f->max_trees = max_trees; f->max_iterations = max_iterations; f->contextual = contextual != 0;
  f->kept = keep_arena != 0;
  f->arena = f->kept ? keep_arena : max_iterations + 1;
  f->slots = forest_slots(f->arena);
  const size_t T = max_trees;
  auto trees = [&]() -> int { // the arenas and tables; a kept forest's failure names what was asked for
    if (!f->kept) { RC(f->get(f->nodes, T * f->arena)); RC(f->get(f->edges, T * f->slots)); return 0; }
    const int rc = [&]() -> int {
      RC(f->get(f->nodes, T * f->arena)); RC(f->get(f->edges, T * f->slots)); RC(f->get(f->nodes_back, T * f->arena)); RC(f->get(f->edges_back, T * f->slots));
      RC(f->get(f->map, T * f->arena));
      return 0;
    }();
    if (rc) {
      const unsigned long long per = oakgpu_forest_kept_tree_bytes(max_iterations, keep_arena) + (unsigned long long)f->arena * 4;
      char msg[320];
      snprintf(msg, sizeof msg, "%s: out of device memory: %u trees of %u nodes ask for %llu bytes (%llu a tree: two copies of %u x 224-byte nodes and %u x 32-byte slots, and the advance's map)",
               who, max_trees, f->arena, per * T, per, f->arena, f->slots);
      return oakgpu_fail_msg(msg);
    }
    RC(f->get(f->n_nodes_back, T)); RC(f->get(f->carried, T)); RC(f->get(f->dropped, 4)); RC(f->get(f->adv_src, T)); RC(f->get(f->mismatch, T)); RC(f->get(f->adv_in, T * 19));
    HIPCHK(hipMemset(f->edges_back, 0, T * f->slots * sizeof(FEdge)));
    HIPCHK(hipMemset(f->n_nodes_back, 0, T * 4)); HIPCHK(hipMemset(f->dropped, 0, 16)); HIPCHK(hipMemset(f->mismatch, 0, T));
    return 0;
  };
  auto all = [&]() -> int {
    RC(trees());
    RC(f->get(f->b, T * 384)); RC(f->get(f->d, T * 8)); RC(f->get(f->r, T)); RC(f->get(f->c1, T)); RC(f->get(f->c2, T)); RC(f->get(f->act, T * 16));
    RC(f->get(f->ch1, T * 9)); RC(f->get(f->cnt1, T)); RC(f->get(f->ch2, T * 9)); RC(f->get(f->cnt2, T)); RC(f->get(f->rout, T));
    RC(f->get(f->root_ch1, T * 9)); RC(f->get(f->root_cnt1, T)); RC(f->get(f->root_ch2, T * 9)); RC(f->get(f->root_cnt2, T)); RC(f->get(f->status, T));
    RC(f->get(f->prng, T)); RC(f->get(f->total_depth, T)); RC(f->get(f->steps, T)); RC(f->get(f->cur, T)); RC(f->get(f->leaf, T)); RC(f->get(f->levels, T));
    RC(f->get(f->n_nodes, T)); RC(f->get(f->values, T)); RC(f->get(f->pe_root, T)); RC(f->get(f->pe_score, T));
    if (f->contextual) { RC(f->get(f->l1, T * 9)); RC(f->get(f->l2, T * 9)); }
    HIPCHK(hipHostMalloc((void **)&f->h_live, 16, hipHostMallocDefault));
    HIPCHK(hipMemset(f->edges, 0, T * f->slots * sizeof(FEdge))); // stamp 0 = free; calls stamp from 1
    if (f->kept) HIPCHK(hipMemset(f->n_nodes, 0, T * 4));
    return 0;
  };
  if (int rc = all()) { f->release(); delete f; return rc; }
  *out = f;
  return 0;
}

int oakgpu_forest_create(oakgpu_ctx *ctx, uint32_t max_trees, uint32_t max_iterations, int contextual, oakgpu_forest **out) {
  if (!ctx || !out) return oakgpu_fail_msg("oakgpu_forest_create: null argument");
  if (max_trees == 0 || max_iterations == 0 || max_iterations > (1u << 24)) return oakgpu_fail_msg("oakgpu_forest_create: max_trees >= 1, max_iterations in 1..2^24");
  return forest_make("oakgpu_forest_create", ctx, max_trees, max_iterations, contextual, 0, out);
}

int oakgpu_forest_create_kept_check(uint32_t max_trees, uint32_t max_iterations, uint32_t keep_arena) {
  if (max_trees == 0 || max_iterations == 0 || max_iterations > (1u << 24)) return oakgpu_fail_msg("oakgpu_forest_create_kept: max_trees >= 1, max_iterations in 1..2^24");
  if (keep_arena != 0 && keep_arena < max_iterations + 1) return oakgpu_fail_msg("oakgpu_forest_create_kept: keep_arena must be at least max_iterations + 1 (0 = 4 * max_iterations + 1)");
  if (keep_arena > (1u << 27)) return oakgpu_fail_msg("oakgpu_forest_create_kept: keep_arena above 2^27");
  return 0;
}

int oakgpu_forest_create_kept(oakgpu_ctx *ctx, uint32_t max_trees, uint32_t max_iterations, int contextual, uint32_t keep_arena, oakgpu_forest **out) {
  if (!ctx || !out) return oakgpu_fail_msg("oakgpu_forest_create_kept: null argument");
  RC(oakgpu_forest_create_kept_check(max_trees, max_iterations, keep_arena));
  return forest_make("oakgpu_forest_create_kept", ctx, max_trees, max_iterations, contextual, keep_arena ? keep_arena : 4 * max_iterations + 1, out);
}

void oakgpu_forest_destroy(oakgpu_ctx *ctx, oakgpu_forest *f) {
  if (!f) return;
  // the forest's own context is not touched here: a caller that lost it (ctx == NULL) still frees the arenas, behind a device-wide wait
  (void)hipSetDevice(f->device);
  if (ctx) (void)hipStreamSynchronize((hipStream_t)oakgpu_ctx_stream(ctx));
  else (void)hipDeviceSynchronize();
  f->release();
  delete f;
}

int oakgpu_forest_last_stats(const oakgpu_forest *f, uint64_t out[4]) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_last_stats: null argument");
  for (int q = 0; q < 4; ++q) out[q] = f->stats[q];
  return 0;
}

int oakgpu_forest_last_rows(const oakgpu_forest *f, uint64_t out[2]) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_last_rows: null argument");
  out[0] = f->rows[0]; out[1] = f->rows[1];
  return 0;
}

int oakgpu_forest_budgets_check(const uint32_t *budgets, uint32_t n, uint64_t iterations) {
  if (!budgets && n) return oakgpu_fail_msg("oakgpu_forest_search_budgets: null argument");
  for (uint32_t g = 0; g < n; ++g) {
    if (budgets[g] == 0) return oakgpu_fail_msg(("oakgpu_forest_search_budgets: the budget of tree " + std::to_string(g) + " is 0 (a tree runs 1 .. params->iterations iterations)").c_str());
    if (budgets[g] > iterations)
      return oakgpu_fail_msg(("oakgpu_forest_search_budgets: the budget of tree " + std::to_string(g) + " (" + std::to_string(budgets[g]) + ") exceeds params->iterations (" +
                              std::to_string(iterations) + ")").c_str());
  }
  return 0;
}

// the body of the device searches: keep = the kept form (an initialised root goes on; the stamp is the one the advance wrote); budgets
// (device, n x u32; null = every tree runs params->iterations) = the budgets form
static int forest_search_body(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                              const uint8_t *results, const uint64_t *seeds, uint32_t n, const oakgpu_forest_outputs *o, void *trace, uint32_t trace_levels, bool keep,
                              const uint32_t *budgets = nullptr, bool with_budgets = false) {
  if (!f || !prm || !battles || !durations || !results || !seeds || !o) return oakgpu_fail_msg("oakgpu_forest_search: null argument");
  if (with_budgets && !budgets && n) return oakgpu_fail_msg("oakgpu_forest_search_budgets: null argument");
  if (keep && !f->kept) return oakgpu_fail_msg("oakgpu_forest_search_kept: the forest was created without keep (oakgpu_forest_create_kept makes one that keeps its trees)");
  if (!o->m || !o->n || !o->p1_choices || !o->p2_choices || !o->visit_matrix || !o->value_matrix || !o->iterations || !o->nodes || !o->total_depth ||
      !o->initial_value || !o->p1_logit || !o->p2_logit || !o->p1_prior || !o->p2_prior || !o->stream)
    return oakgpu_fail_msg("oakgpu_forest_search: every output array is required");
  RC(oakgpu_forest_check(f->max_trees, f->max_iterations, f->contextual, prm, net != nullptr, n, nullptr, trace != nullptr, trace_levels));
  if (n == 0) return 0;
  oakgpu_ctx *ctx = f->ctx;
  RC(oakgpu_ctx_enter(ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(ctx);
  std::vector<uint32_t> hb; // the budgets on the host: they ride with the result bytes
  { // a terminal root is refused before anything is launched: one copy of the n result bytes
    std::vector<uint8_t> h(n);
    HIPCHK(hipMemcpyAsync(h.data(), results, n, hipMemcpyDeviceToHost, stream));
    if (budgets) { hb.resize(n); HIPCHK(hipMemcpyAsync(hb.data(), budgets, (size_t)n * 4, hipMemcpyDeviceToHost, stream)); }
    HIPCHK(hipStreamSynchronize(stream));
    RC(oakgpu_forest_check(f->max_trees, f->max_iterations, f->contextual, prm, net != nullptr, n, h.data(), trace != nullptr, trace_levels));
    if (budgets) RC(oakgpu_forest_budgets_check(hb.data(), n, prm->iterations));
  }
  const bool pucb = prm->bandit == B_PUCB, use_net = prm->eval == 1, use_pe = prm->eval == 2;
  const uint32_t max_depth = prm->max_depth ? prm->max_depth : 100;
  // the loop runs max(budgets) iterations; iteration t covers rows [0, rows_at[t]): one past the last tree whose budget is above t
  uint32_t iterations = (uint32_t)prm->iterations;
  std::vector<uint32_t> rows_at;
  uint64_t rows_launched = (uint64_t)n * iterations, rows_run = rows_launched;
  if (budgets) {
    iterations = *std::max_element(hb.begin(), hb.end());
    rows_at.assign(iterations, 0);
    rows_run = 0;
    for (uint32_t g = 0; g < n; ++g) { rows_at[hb[g] - 1] = g + 1; rows_run += hb[g]; } // ascending g: the last writer is the highest row
    for (uint32_t t = iterations - 1; t > 0; --t) rows_at[t - 1] = std::max(rows_at[t - 1], rows_at[t]);
    rows_launched = 0;
    for (uint32_t t = 0; t < iterations; ++t) rows_launched += rows_at[t];
  }
  const BanditParams BP{prm->bandit, prm->ucb_c, 0.05f};
  if (f->path_levels < max_depth || !f->path_node) {
    HIPCHK(hipStreamSynchronize(stream));
    if (f->path_node) (void)hipFree(f->path_node);
    if (f->path_i) (void)hipFree(f->path_i);
    if (f->path_j) (void)hipFree(f->path_j);
    if (f->ctl) (void)hipFree(f->ctl);
    f->path_node = nullptr; f->path_i = f->path_j = nullptr; f->ctl = nullptr; f->path_levels = 0;
    RC(dev_alloc(f->ctl, (size_t)max_depth + 2));
    RC(dev_alloc(f->path_node, (size_t)f->max_trees * max_depth)); RC(dev_alloc(f->path_i, (size_t)f->max_trees * max_depth)); RC(dev_alloc(f->path_j, (size_t)f->max_trees * max_depth));
    f->path_levels = max_depth;
  }
  if (!keep || f->gen == 0) {
    if (++f->gen > 0xFFFFu) { // the stamp wrapped: one real clear, of both copies
      HIPCHK(hipMemsetAsync(f->edges, 0, (size_t)f->max_trees * f->slots * sizeof(FEdge), stream));
      if (f->edges_back) HIPCHK(hipMemsetAsync(f->edges_back, 0, (size_t)f->max_trees * f->slots * sizeof(FEdge), stream));
      f->gen = 1;
    }
    f->valid = 0; // every tree of the new stamp is empty
  }
  f->last_n = 0;
  const dim3 grid((n + FBLOCK - 1) / FBLOCK), block(FBLOCK);
  uint64_t launches = 0, levels_stepped = 0, polls = 0;

  // the roots: choices (mcts.h:160-166), PUCB priors from the policy heads (:196-209), PokeEngine root scores (:172-174)
  RC(oakgpu_choices_dev(ctx, battles, results, 0, f->root_ch1, f->root_cnt1, n));
  RC(oakgpu_choices_dev(ctx, battles, results, 1, f->root_ch2, f->root_cnt2, n));
  if (pucb) RC(oakgpu_leaf_eval_policy_dev(ctx, net, battles, durations, n, f->root_ch1, f->root_cnt1, f->root_ch2, f->root_cnt2, f->values, f->l1, f->l2));
  if (use_pe) RC(oakgpu_poke_engine_eval_dev(ctx, battles, n, 0.0f, nullptr, f->pe_root));
  {
    BeginArgs a{};
    a.nodes = f->nodes; a.arena = f->arena; a.n = n; a.pucb = pucb; a.seeds = seeds;
    a.root_cnt1 = f->root_cnt1; a.root_cnt2 = f->root_cnt2; a.root_ch1 = f->root_ch1; a.root_ch2 = f->root_ch2;
    a.values = f->values; a.l1 = f->l1; a.l2 = f->l2; a.prng = f->prng; a.n_nodes = f->n_nodes; a.status = f->status; a.total_depth = f->total_depth;
    a.P = BP; a.out = *o;
    a.keep = keep; a.valid = f->valid; a.slots = f->slots; a.gen = f->gen; a.edges = f->edges; a.mismatch = f->mismatch; a.carried = f->carried;
    hipLaunchKernelGGL(k_forest_begin, grid, block, 0, stream, a);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemsetAsync(f->ctl, 0, 4, stream));

  ForestArgs A{};
  A.nodes = f->nodes; A.edges = f->edges; A.arena = f->arena; A.slots = f->slots; A.gen = f->gen; A.n = n; A.stride = n;
  A.cur = f->cur; A.leaf = f->leaf; A.levels = f->levels; A.n_nodes = f->n_nodes; A.status = f->status;
  A.path_node = f->path_node; A.path_i = f->path_i; A.path_j = f->path_j;
  A.results = f->r; A.act = f->act; A.ch1 = f->ch1; A.cnt1 = f->cnt1; A.ch2 = f->ch2; A.cnt2 = f->cnt2; A.root_ch1 = f->root_ch1; A.root_ch2 = f->root_ch2;
  A.c1 = f->c1; A.c2 = f->c2; A.ctl = f->ctl; A.total_depth = f->total_depth; A.P = BP; A.max_depth = max_depth;
  BackupArgs K{};
  K.nodes = f->nodes; K.arena = f->arena; K.n = n; K.stride = n; K.pucb = pucb; K.eval = (uint32_t)prm->eval; K.iterations = (uint32_t)prm->iterations; K.trace_levels = trace_levels;
  K.budgets = budgets; K.prng = f->prng; K.stream_out = o->stream;
  K.leaf = f->leaf; K.levels = f->levels; K.path_node = f->path_node; K.status = f->status; K.path_i = f->path_i; K.path_j = f->path_j;
  K.results = f->r; K.cnt1 = f->cnt1; K.cnt2 = f->cnt2; K.values = f->values; K.pe_root = f->pe_root; K.pe_score = f->pe_score; K.l1 = f->l1; K.l2 = f->l2;
  K.visit_matrix = o->visit_matrix; K.value_matrix = o->value_matrix; K.trace = (uint8_t *)trace; K.P = BP;

  for (uint32_t it = 0; it < iterations; ++it) {
    // the iteration's rows (the outputs, the path stride and the finish cover the call's n); >= 1: some tree's budget is above `it`
    const uint32_t rows = budgets ? rows_at[it] : n;
    const dim3 row_grid((rows + FBLOCK - 1) / FBLOCK);
    A.n = rows; K.n = rows;
    // root prep on the device (mcts.h:254-259): the rollout kernel with max_steps = 0, as the host search's begin_batch
    RC(oakgpu_rollout_dev(ctx, battles, durations, results, (uint8_t *)f->prng, rows, 0, 1, f->rout, f->steps, f->values, f->b, f->d));
    HIPCHK(hipMemcpyAsync(f->r, results, rows, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemsetAsync(f->ctl + 1, 0, (size_t)(max_depth + 1) * 4, stream));
    hipLaunchKernelGGL(k_forest_level, row_grid, block, 0, stream, A, 0u);
    HIPCHK(hipGetLastError());
    launches += 2;
    for (uint32_t depth = 1; depth <= max_depth; ++depth) {
      RC(oakgpu_tree_step_dev(ctx, f->b, f->d, f->r, f->c1, f->c2, rows, depth == 1 ? prm->root_rolls : prm->other_rolls, f->act, f->ch1, f->cnt1, f->ch2, f->cnt2));
      hipLaunchKernelGGL(k_forest_level, row_grid, block, 0, stream, A, depth);
      HIPCHK(hipGetLastError());
      launches += 2; ++levels_stepped;
      if (depth == max_depth) break; // no lane goes on below the cap
      HIPCHK(hipMemcpyAsync(f->h_live, f->ctl + 1 + depth, 4, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      ++polls;
      if (f->h_live[0] == 0) break;
    }
    // the leaf evaluation, over every row, as the host search's launch_eval
    if (use_pe) RC(oakgpu_poke_engine_eval_dev(ctx, f->b, rows, 0.0f, nullptr, f->pe_score));
    else if (!use_net) RC(oakgpu_rollout_dev(ctx, f->b, f->d, f->r, (uint8_t *)f->prng, rows, 1000, 0, f->rout, f->steps, f->values, nullptr, nullptr));
    else if (pucb) RC(oakgpu_leaf_eval_policy_dev(ctx, net, f->b, f->d, rows, f->ch1, f->cnt1, f->ch2, f->cnt2, f->values, f->l1, f->l2));
    else RC(oakgpu_leaf_eval_dev(ctx, net, f->b, f->d, rows, f->values, nullptr));
    K.iteration = it;
    hipLaunchKernelGGL(k_forest_backup, row_grid, block, 0, stream, K);
    HIPCHK(hipGetLastError());
    launches += 2;
  }
  hipLaunchKernelGGL(k_forest_finish, grid, block, 0, stream, n, (uint64_t)iterations, f->n_nodes, f->total_depth, f->prng, budgets, *o);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(f->h_live + 1, f->ctl, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  f->stats[0] = iterations; f->stats[1] = levels_stepped; f->stats[2] = launches; f->stats[3] = polls;
  f->rows[0] = rows_launched; f->rows[1] = rows_run;
  f->last_n = n;
  f->valid = keep ? std::max(f->valid, n) : n;
  if (f->h_live[1] & ERR_ARENA_FULL) return oakgpu_fail_msg("oakgpu_forest_search: a tree's node arena is full");
  if (f->h_live[1] & ERR_TABLE_FULL) return oakgpu_fail_msg("oakgpu_forest_search: a tree's edge table is full");
  return 0;
}

int oakgpu_forest_search_dev(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                             const uint8_t *results, const uint64_t *seeds, uint32_t n, const oakgpu_forest_outputs *o, void *trace, uint32_t trace_levels) {
  return forest_search_body(f, net, prm, battles, durations, results, seeds, n, o, trace, trace_levels, false);
}

int oakgpu_forest_search_kept_dev(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                                  const uint8_t *results, const uint64_t *seeds, uint32_t n, const oakgpu_forest_outputs *o, void *trace, uint32_t trace_levels) {
  return forest_search_body(f, net, prm, battles, durations, results, seeds, n, o, trace, trace_levels, true);
}

// the body of both host-array searches
static int forest_search_host(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                              const uint8_t *results, const uint64_t *seeds, uint32_t n, oakgpu_search_output *out, int solve_nash, uint64_t *streams_out,
                              void *trace, uint32_t trace_levels, bool keep, const uint32_t *budgets = nullptr, bool with_budgets = false) {
  if (!f || !prm || !battles || !durations || !results || !seeds || !out) return oakgpu_fail_msg("oakgpu_forest_search: null argument");
  if (with_budgets && !budgets && n) return oakgpu_fail_msg("oakgpu_forest_search_budgets: null argument");
  if (keep && !f->kept) return oakgpu_fail_msg("oakgpu_forest_search_kept: the forest was created without keep (oakgpu_forest_create_kept makes one that keeps its trees)");
  RC(oakgpu_forest_check(f->max_trees, f->max_iterations, f->contextual, prm, net != nullptr, n, results, trace != nullptr, trace_levels));
  if (budgets) RC(oakgpu_forest_budgets_check(budgets, n, prm->iterations));
  if (n == 0) return 0;
  const auto t0 = std::chrono::high_resolution_clock::now();
  RC(oakgpu_ctx_enter(f->ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(f->ctx);
  const size_t T = f->max_trees;
  if (!f->stage) RC(dev_alloc(f->stage, IN_BYTES * T + 64 + outputs_bytes(T)));
  uint8_t *d_b = f->stage, *d_d = d_b + T * 384, *d_s = d_d + T * 8, *d_r = d_s + T * 8, *d_o = d_r + ((T + 15) / 16) * 16;
  const size_t rec = OAKGPU_FOREST_TRACE_BYTES(trace_levels), trace_bytes = trace ? (size_t)n * prm->iterations * rec : 0;
  if (trace_bytes > f->trace_stage_bytes) {
    HIPCHK(hipStreamSynchronize(stream));
    if (f->trace_stage) (void)hipFree(f->trace_stage);
    f->trace_stage = nullptr; f->trace_stage_bytes = 0;
    RC(dev_alloc(f->trace_stage, trace_bytes));
    f->trace_stage_bytes = trace_bytes;
  }
  HIPCHK(hipMemcpyAsync(d_b, battles, (size_t)n * 384, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_d, durations, (size_t)n * 8, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_s, seeds, (size_t)n * 8, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_r, results, n, hipMemcpyHostToDevice, stream));
  if (budgets) {
    if (!f->budget_stage) RC(dev_alloc(f->budget_stage, T));
    HIPCHK(hipMemcpyAsync(f->budget_stage, budgets, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    // records past a tree's budget are not written: the caller's bytes there go down and come back
    if (trace) HIPCHK(hipMemcpyAsync(f->trace_stage, trace, trace_bytes, hipMemcpyHostToDevice, stream));
  }
  HIPCHK(hipStreamSynchronize(stream));
  oakgpu_forest_outputs o;
  carve_outputs(d_o, n, &o);
  RC(forest_search_body(f, net, prm, d_b, d_d, d_r, (const uint64_t *)d_s, n, &o, trace ? f->trace_stage : nullptr, trace_levels, keep, budgets ? f->budget_stage : nullptr,
                        with_budgets));
  std::vector<uint8_t> h(outputs_bytes(n));
  HIPCHK(hipMemcpy(h.data(), d_o, h.size(), hipMemcpyDeviceToHost));
  if (trace) HIPCHK(hipMemcpy(trace, f->trace_stage, trace_bytes, hipMemcpyDeviceToHost));
  oakgpu_forest_outputs ho;
  carve_outputs(h.data(), n, &ho);
  const double us = std::chrono::duration<double, std::micro>(std::chrono::high_resolution_clock::now() - t0).count();
  std::vector<int32_t> pay(solve_nash == 2 ? (size_t)n * oak_nash::PAY_STRIDE : 0, 0);
  for (uint32_t g = 0; g < n; ++g) {
    oakgpu_search_output &x = out[g];
    memset(&x, 0, sizeof x);
    const int m = x.m = ho.m[g], nn = x.n = ho.n[g];
    memcpy(x.p1_choices, ho.p1_choices + (size_t)g * 9, 9); memcpy(x.p2_choices, ho.p2_choices + (size_t)g * 9, 9);
    memcpy(x.visit_matrix, ho.visit_matrix + (size_t)g * 81, sizeof x.visit_matrix); memcpy(x.value_matrix, ho.value_matrix + (size_t)g * 81, sizeof x.value_matrix);
    x.iterations = ho.iterations[g]; x.nodes = ho.nodes[g]; x.total_depth = ho.total_depth[g]; x.initial_value = ho.initial_value[g];
    memcpy(x.p1_logit, ho.p1_logit + (size_t)g * 9, 72); memcpy(x.p2_logit, ho.p2_logit + (size_t)g * 9, 72);
    memcpy(x.p1_prior, ho.p1_prior + (size_t)g * 9, 72); memcpy(x.p2_prior, ho.p2_prior + (size_t)g * 9, 72);
    x.duration_us = us;
    if (streams_out) streams_out[g] = ho.stream[g];
    // MCTS::Search::process_output (mcts.h:620-659), as oakgpu_search runs it (selfplay_pick.hpp, shared with the device game loop)
    int32_t M[81];
    oak_pick::process_output(x.visit_matrix, x.value_matrix, m, nn, x.iterations, &x.empirical_value, x.p1_empirical, x.p2_empirical, M);
    double nv = 0;
    if (solve_nash == 2) { // one device solve over all n trees, below
      memcpy(pay.data() + (size_t)g * oak_nash::PAY_STRIDE, M, sizeof M);
      pay[(size_t)g * oak_nash::PAY_STRIDE + 81] = m | nn << 8;
    } else if (solve_nash && oak_nash::solve(M, m, nn, x.p1_nash, x.p2_nash, &nv)) x.nash_value = nv / 256.0;
  }
  if (solve_nash == 2) {
    OakHostCall call(f->ctx);
    int32_t *d_pay = (int32_t *)call.get(pay.size() * 4);
    double *d_nash = (double *)call.get((size_t)n * 19 * 8);
    if (!d_pay || !d_nash) return -1;
    std::vector<double> nash((size_t)n * 19);
    HIPCHK(hipMemcpyAsync(d_pay, pay.data(), pay.size() * 4, hipMemcpyHostToDevice, stream));
    RC(oakgpu_nash_solve_dev(f->ctx, d_pay, n, d_nash));
    HIPCHK(hipMemcpyAsync(nash.data(), d_nash, nash.size() * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (uint32_t g = 0; g < n; ++g) {
      memcpy(out[g].p1_nash, nash.data() + (size_t)g * 9, 72);
      memcpy(out[g].p2_nash, nash.data() + ((size_t)n + g) * 9, 72);
      out[g].nash_value = nash[(size_t)n * 18 + g];
    }
  }
  return 0;
}

int oakgpu_forest_search(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                         const uint8_t *results, const uint64_t *seeds, uint32_t n, oakgpu_search_output *out, int solve_nash, uint64_t *streams_out,
                         void *trace, uint32_t trace_levels) {
  return forest_search_host(f, net, prm, battles, durations, results, seeds, n, out, solve_nash, streams_out, trace, trace_levels, false);
}

int oakgpu_forest_search_kept(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                              const uint8_t *results, const uint64_t *seeds, uint32_t n, oakgpu_search_output *out, int solve_nash, uint64_t *streams_out,
                              void *trace, uint32_t trace_levels) {
  return forest_search_host(f, net, prm, battles, durations, results, seeds, n, out, solve_nash, streams_out, trace, trace_levels, true);
}

// the budgets forms: tree g runs budgets[g] iterations (the contract is in include/oakgpu.h)
int oakgpu_forest_search_budgets_dev(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                                     const uint8_t *results, const uint64_t *seeds, const uint32_t *budgets, uint32_t n, const oakgpu_forest_outputs *o, void *trace,
                                     uint32_t trace_levels) {
  return forest_search_body(f, net, prm, battles, durations, results, seeds, n, o, trace, trace_levels, false, budgets, true);
}

int oakgpu_forest_search_budgets_kept_dev(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                                          const uint8_t *results, const uint64_t *seeds, const uint32_t *budgets, uint32_t n, const oakgpu_forest_outputs *o,
                                          void *trace, uint32_t trace_levels) {
  return forest_search_body(f, net, prm, battles, durations, results, seeds, n, o, trace, trace_levels, true, budgets, true);
}

int oakgpu_forest_search_budgets(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                                 const uint8_t *results, const uint64_t *seeds, const uint32_t *budgets, uint32_t n, oakgpu_search_output *out, int solve_nash,
                                 uint64_t *streams_out, void *trace, uint32_t trace_levels) {
  return forest_search_host(f, net, prm, battles, durations, results, seeds, n, out, solve_nash, streams_out, trace, trace_levels, false, budgets, true);
}

int oakgpu_forest_search_budgets_kept(oakgpu_forest *f, oakgpu_net *net, const oakgpu_search_params *prm, const uint8_t *battles, const uint8_t *durations,
                                      const uint8_t *results, const uint64_t *seeds, const uint32_t *budgets, uint32_t n, oakgpu_search_output *out, int solve_nash,
                                      uint64_t *streams_out, void *trace, uint32_t trace_levels) {
  return forest_search_host(f, net, prm, battles, durations, results, seeds, n, out, solve_nash, streams_out, trace, trace_levels, true, budgets, true);
}

// Heap::update of every tree, and the move to another row (k_forest_advance): reads the front copy, writes the back one, then the two swap
int oakgpu_forest_advance_dev(oakgpu_forest *f, const uint8_t *i, const uint8_t *j, const uint8_t *obs, const uint32_t *src_tree, uint32_t n_new, uint8_t *kept_out) {
  if (!f) return oakgpu_fail_msg("oakgpu_forest_advance: null argument");
  if (!f->kept) return oakgpu_fail_msg("oakgpu_forest_advance: the forest was created without keep (oakgpu_forest_create_kept makes one that keeps its trees)");
  if (n_new > f->max_trees) return oakgpu_fail_msg("oakgpu_forest_advance: n_new exceeds the forest's max_trees");
  if (n_new && (!i || !j || !obs || !kept_out)) return oakgpu_fail_msg("oakgpu_forest_advance: null argument");
  RC(oakgpu_ctx_enter(f->ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(f->ctx);
  const size_t table_bytes = (size_t)f->max_trees * f->slots * sizeof(FEdge);
  const uint32_t gen_old = f->gen;
  const bool wrapped = f->gen + 1 > 0xFFFFu; // the back copy is cleared before it is written, the front one once it has been read
  if (wrapped) HIPCHK(hipMemsetAsync(f->edges_back, 0, table_bytes, stream));
  f->gen = wrapped ? 1 : f->gen + 1;
  if (n_new) {
    AdvanceArgs a{};
    a.src_nodes = f->nodes; a.src_edges = f->edges; a.src_n_nodes = f->n_nodes; a.dst_nodes = f->nodes_back; a.dst_edges = f->edges_back; a.dst_n_nodes = f->n_nodes_back;
    a.map = f->map; a.i = i; a.j = j; a.obs = obs; a.src_tree = src_tree; a.kept_out = kept_out; a.dropped = f->dropped;
    a.arena = f->arena; a.slots = f->slots; a.gen_old = gen_old; a.gen_new = f->gen; a.n_new = n_new; a.valid = f->valid; a.max_iterations = f->max_iterations;
    hipLaunchKernelGGL(k_forest_advance, dim3(n_new), dim3(64), 0, stream, a);
    HIPCHK(hipGetLastError());
  }
  if (wrapped) HIPCHK(hipMemsetAsync(f->edges, 0, table_bytes, stream));
  std::swap(f->nodes, f->nodes_back); std::swap(f->edges, f->edges_back); std::swap(f->n_nodes, f->n_nodes_back);
  f->valid = n_new;
  f->last_n = n_new;
  ++f->advances;
  return 0;
}

int oakgpu_forest_advance(oakgpu_forest *f, const uint8_t *i, const uint8_t *j, const uint8_t *obs, const uint32_t *src_tree, uint32_t n_new, uint8_t *kept_out) {
  if (!f) return oakgpu_fail_msg("oakgpu_forest_advance: null argument");
  if (!f->kept) return oakgpu_fail_msg("oakgpu_forest_advance: the forest was created without keep (oakgpu_forest_create_kept makes one that keeps its trees)");
  if (n_new > f->max_trees) return oakgpu_fail_msg("oakgpu_forest_advance: n_new exceeds the forest's max_trees");
  if (n_new && (!i || !j || !obs || !kept_out)) return oakgpu_fail_msg("oakgpu_forest_advance: null argument");
  RC(oakgpu_ctx_enter(f->ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(f->ctx);
  const size_t T = f->max_trees;
  uint8_t *d_obs = f->adv_in, *d_i = d_obs + 16 * T, *d_j = d_i + T, *d_kept = d_j + T;
  if (n_new) {
    HIPCHK(hipMemcpyAsync(d_i, i, n_new, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_j, j, n_new, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_obs, obs, (size_t)n_new * 16, hipMemcpyHostToDevice, stream));
    if (src_tree) HIPCHK(hipMemcpyAsync(f->adv_src, src_tree, (size_t)n_new * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  RC(oakgpu_forest_advance_dev(f, d_i, d_j, d_obs, src_tree ? f->adv_src : nullptr, n_new, d_kept));
  if (n_new) HIPCHK(hipMemcpyAsync(kept_out, d_kept, n_new, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_forest_keep_stats(oakgpu_forest *f, uint64_t out[4]) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_keep_stats: null argument");
  if (!f->kept) return oakgpu_fail_msg("oakgpu_forest_keep_stats: the forest was created without keep (oakgpu_forest_create_kept makes one that keeps its trees)");
  RC(oakgpu_ctx_enter(f->ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(f->ctx);
  uint32_t dropped = 0;
  HIPCHK(hipMemcpyAsync(&dropped, f->dropped, 4, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  out[0] = f->arena; out[1] = f->slots; out[2] = f->advances; out[3] = dropped;
  return 0;
}

int oakgpu_forest_node_counts(oakgpu_forest *f, uint32_t *out, uint32_t n, int to_device) {
  if (!f || (n && !out)) return oakgpu_fail_msg("oakgpu_forest_node_counts: null argument");
  if (n > f->last_n) return oakgpu_fail_msg("oakgpu_forest_node_counts: more trees than the forest's last call left");
  RC(oakgpu_ctx_enter(f->ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(f->ctx);
  if (n) HIPCHK(hipMemcpyAsync(out, f->n_nodes, (size_t)n * 4, to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_forest_mismatch(oakgpu_forest *f, uint8_t *out, uint32_t n, int to_device) {
  if (!f || (n && !out)) return oakgpu_fail_msg("oakgpu_forest_mismatch: null argument");
  if (!f->kept) return oakgpu_fail_msg("oakgpu_forest_mismatch: the forest was created without keep (oakgpu_forest_create_kept makes one that keeps its trees)");
  if (n > f->max_trees) return oakgpu_fail_msg("oakgpu_forest_mismatch: n exceeds the forest's max_trees");
  RC(oakgpu_ctx_enter(f->ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(f->ctx);
  if (n) HIPCHK(hipMemcpyAsync(out, f->mismatch, n, to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

int oakgpu_forest_nodes(oakgpu_forest *f, uint32_t tree, uint32_t first, uint32_t count, oakgpu_forest_node *out) {
  if (!f || !out) return oakgpu_fail_msg("oakgpu_forest_nodes: null argument");
  if (tree >= f->last_n) return oakgpu_fail_msg("oakgpu_forest_nodes: no such tree in the forest's last call");
  RC(oakgpu_ctx_enter(f->ctx));
  hipStream_t stream = (hipStream_t)oakgpu_ctx_stream(f->ctx);
  HIPCHK(hipStreamSynchronize(stream));
  uint32_t have = 0;
  HIPCHK(hipMemcpy(&have, f->n_nodes + tree, 4, hipMemcpyDeviceToHost));
  if ((uint64_t)first + count > have) return oakgpu_fail_msg("oakgpu_forest_nodes: the tree has fewer nodes");
  if (count) HIPCHK(hipMemcpy(out, f->nodes + (size_t)tree * f->arena + first, (size_t)count * sizeof(FNode), hipMemcpyDeviceToHost));
  return 0;
}

} // extern "C"
