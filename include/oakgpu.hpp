// include/oakgpu.hpp -- thin C++ host layer over the C ABI (include/oakgpu.h), shaped like the
// reference's search-node surface so Oak's tree code can use it as an `eval` (cpp/include/search/mcts.h:25-57).
//
//   OakGPU::Context            <- per-thread owner of device state (reference: per-thread Agent/Heap, util/search.h:17-64)
//   OakGPU::Network            <- NN::Battle::Network (nn/battle/network.h:22-176): shape(), value_inference(batch), and the
//                                 reference's own per-leaf eval signatures value_inference(battle, durations) /
//                                 value_policy_inference(b, d, m, n, c1, c2, p1, p2) that MCTS::Search::run calls (mcts.h:196-209,401-422)
//   OakGPU::BatchedMonteCarlo  <- MCTS::MonteCarlo (mcts.h:21-23) + init_stats_and_rollout (mcts.h:448-496), batched
//   OakGPU::TreeSearch         <- MCTS::Search::run (mcts.h:154-247): Node heap + the five joint bandits, leaves batched on the GPU
//   OakGPU::SearchForest       <- MCTS::Search::run for many positions at once: one GPU lane per tree, the trees resident on the device
//   OakGPU::ForestSelfplay     <- the per-game loop of generate.cc:238-322 for a batch of games at once over the forest search, `.battle.data` out
//   OakGPU::ForestMatch        <- the per-game loop of vs.cc:230-345 with a budget: two search agents, a batch of games at once over the forest search
//   OakGPU::run                <- RuntimeSearch::run (util/search.h:66, search.cc:150-313): the Agent's strings pick everything
//   OakGPU::solve_matrix       <- LRSNash::solve_fast as called at mcts.h:643-649 / pyoak.cc:394-426 (exact)
//   OakGPU::solve_matrices     <- a batch of those on the device, the same bits
//   OakGPU::SharedDeviceRollout<- benchmark.cc:23-31: n playouts from one root driven by ONE sequential std::mt19937
//   OakGPU::Frames             <- Train::Battle::CompressedFrames (train/battle/compressed-frame.h:37-243)
//   OakGPU::replay_check       <- the replay self-check of py/battle/frames.h:52-67, for a whole file at once
//   OakGPU::FrameCorpus, EncodedFrames <- pyoak.sample + Py::Battle::EncodedFrames (pyoak.cc:111-245, py/battle/encoded-frames.h)
//   OakGPU::FrameCorpus::inference / evaluate <- pyoak.cpp_inference over a whole corpus (pyoak.cc:331-392) and battle.py's loss terms
//   OakGPU::PolicyGames        <- the per-game loop of `vs --budget=0 --bandit=pucb-1.0 --policy-mode=p` (vs.cc:107-408), a batch of games at once
//   OakGPU::Exchange           <- the path's one collective: per-root means on the device + RCCL all-gather (no reference analogue)
// Errors surface as std::runtime_error, like the reference's loaders (cpp/src/search.cc:81-146).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "oakgpu.h"
#include "pkmn.h"

namespace OakGPU {

inline void check(int rc) {
  if (rc != 0) throw std::runtime_error{std::string{"oakgpu: "} + oakgpu_last_error()};
}

class Context {
public:
  explicit Context(int device = 0) { check(oakgpu_create(&ctx_, device)); }
  ~Context() { oakgpu_destroy(ctx_); }
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  oakgpu_ctx *get() const noexcept { return ctx_; }
  void synchronize() { check(oakgpu_synchronize(ctx_)); }
  // tree searches of this context look bench-slot embeddings up in a table filled from the search's root (no result changes;
  // default off); returns the previous value
  bool set_search_party_table(bool on) { return oakgpu_set_search_party_table(ctx_, on ? 1 : 0) != 0; }
  // {searches of this context that filled such a table, leaf batches they evaluated through one}
  std::pair<uint64_t, uint64_t> search_party_table_stats() const {
    uint64_t fills = 0, evals = 0;
    check(oakgpu_search_party_table_stats(ctx_, &fills, &evals));
    return {fills, evals};
  }

private:
  oakgpu_ctx *ctx_{};
};

// One leaf of the batch: what MCTS::Input carries (mcts.h:62-66)
struct Leaf {
  uint8_t battle[OAKGPU_BATTLE_SIZE];
  uint8_t durations[OAKGPU_DURATIONS_SIZE];
  uint8_t result;
};

struct RolloutResult {
  std::vector<float> value;     // 1 / 0 / 0.5 (mcts.h:481-495)
  std::vector<uint32_t> steps;  // turn-steps played
  std::vector<uint8_t> result;  // final pkmn_result byte
};

class BatchedMonteCarlo {
public:
  explicit BatchedMonteCarlo(Context &ctx) : ctx_{ctx} {}
  // Several independent batches (e.g. the leaf batches of many roots) drained by ONE launch through one playout queue:
  // a group has one tail instead of one per batch.  Device pointers; asynchronous on the context's stream.
  void rollout_group_dev(const std::vector<oakgpu_rollout_batch> &batches, bool prep = false, uint32_t max_steps = 1000) {
    check(oakgpu_rollout_group_dev(ctx_.get(), batches.data(), static_cast<uint32_t>(batches.size()), max_steps, prep ? 1 : 0));
  }
  // device_rng: one fast_prng state (8 bytes, util/random.h:67-133) per leaf, advanced in place.
  // prep = true performs run_root_iteration's re-seed + randomize_hidden_variables per leaf (mcts.h:254-259).
  RolloutResult rollout(const std::vector<Leaf> &leaves, std::vector<uint64_t> &device_rng, bool prep = false,
                        uint32_t max_steps = 1000) {
    const uint32_t n = static_cast<uint32_t>(leaves.size());
    if (device_rng.size() != n) throw std::runtime_error{"oakgpu: one RNG state per leaf required"};
    std::vector<uint8_t> battles(size_t{n} * OAKGPU_BATTLE_SIZE), durations(size_t{n} * OAKGPU_DURATIONS_SIZE), results(n);
    for (uint32_t i = 0; i < n; ++i) {
      std::memcpy(&battles[size_t{i} * OAKGPU_BATTLE_SIZE], leaves[i].battle, OAKGPU_BATTLE_SIZE);
      std::memcpy(&durations[size_t{i} * OAKGPU_DURATIONS_SIZE], leaves[i].durations, OAKGPU_DURATIONS_SIZE);
      results[i] = leaves[i].result;
    }
    RolloutResult out{std::vector<float>(n), std::vector<uint32_t>(n), std::vector<uint8_t>(n)};
    check(oakgpu_rollout(ctx_.get(), battles.data(), durations.data(), results.data(), reinterpret_cast<uint8_t *>(device_rng.data()), n,
                         max_steps, prep ? 1 : 0, out.result.data(), out.steps.data(), out.value.data(), nullptr, nullptr));
    return out;
  }

private:
  Context &ctx_;
};

class PartyTable;

class Network {
public:
  Network(Context &ctx, const std::string &path) : ctx_{ctx} { check(oakgpu_net_load(ctx_.get(), path.c_str(), &net_)); }
  // discrete = the quantized int8 main net (Agent.discrete): oakgpu_net_load_discrete
  Network(Context &ctx, const std::string &path, bool discrete) : ctx_{ctx} {
    check(discrete ? oakgpu_net_load_discrete(ctx_.get(), path.c_str(), &net_) : oakgpu_net_load(ctx_.get(), path.c_str(), &net_));
  }
  bool discrete() const { return oakgpu_net_is_discrete(net_) != 0; }
  ~Network() { oakgpu_net_free(ctx_.get(), net_); }
  Network(const Network &) = delete;
  Network &operator=(const Network &) = delete;
  // MainNet::shape(): fc0.in, fc0.out, value_fc2.out, p1_policy_fc2.out (main-net.h:32-34)
  std::tuple<int, int, int, int> shape() const {
    int a = 0, b = 0, c = 0, d = 0;
    check(oakgpu_net_shape(net_, &a, &b, &c, &d));
    return {a, b, c, d};
  }
  // how the main net's dense layers are multiplied: OAKGPU_MAIN_PAIR (default: scaled fp16 pairs, fp32 results), OAKGPU_MAIN_SPLIT (bf16 triples) or OAKGPU_MAIN_FP32
  int set_main_precision(int mode) { return oakgpu_net_set_main_precision(net_, mode); }
  // value_inference(battle, durations) for every leaf (network.h:72-79)
  std::vector<float> value_inference(const std::vector<Leaf> &leaves) {
    const uint32_t n = static_cast<uint32_t>(leaves.size());
    std::vector<uint8_t> battles(size_t{n} * OAKGPU_BATTLE_SIZE), durations(size_t{n} * OAKGPU_DURATIONS_SIZE);
    for (uint32_t i = 0; i < n; ++i) {
      std::memcpy(&battles[size_t{i} * OAKGPU_BATTLE_SIZE], leaves[i].battle, OAKGPU_BATTLE_SIZE);
      std::memcpy(&durations[size_t{i} * OAKGPU_DURATIONS_SIZE], leaves[i].durations, OAKGPU_DURATIONS_SIZE);
    }
    std::vector<float> values(n);
    check(oakgpu_leaf_eval(ctx_.get(), net_, battles.data(), durations.data(), n, values.data(), nullptr));
    return values;
  }

  // ---- the reference's per-leaf `eval` signatures (nn/battle/network.h:72-79, 102-123), what an UNCHANGED MCTS::Search::run
  // calls at every new leaf (mcts.h:401-422) and at a fresh contextual root (mcts.h:196-209).  Each is a batch of ONE through the
  // same kernels as the batched forms (like include/pkmn.h's update / choices): correct and within the same 1e-5 / 2e-5 of
  // the oracle, but it costs three kernel launches and four small PCIe copies per leaf (~60-100 us against 15 ns per leaf in
  // a 65,536-leaf batch).  It exists so that the network drops into the reference's sequential search unchanged; throughput
  // comes from the batched forms above and from OakGPU::TreeSearch.
  float value_inference(const pkmn_gen1_battle &b, const pkmn_gen1_chance_durations &d) {
    float value = 0.0f;
    check(oakgpu_leaf_eval(ctx_.get(), net_, b.bytes, d.bytes, 1, &value, nullptr));
    return value;
  }
  // m / n legal choices of the two sides (as pkmn_gen1_battle_choices returned them); p1 / p2 receive their m / n logits
  template <class Count, class Choice>
  float value_policy_inference(const pkmn_gen1_battle &b, const pkmn_gen1_chance_durations &d, const Count m, const Count n,
                               const Choice *p1_choice, const Choice *p2_choice, float *p1, float *p2) {
    if (m > 9 || n > 9) throw std::runtime_error{"oakgpu: more than PKMN_GEN1_MAX_CHOICES choices"};
    uint8_t c1[9] = {}, c2[9] = {};
    const uint8_t k1 = static_cast<uint8_t>(m), k2 = static_cast<uint8_t>(n);
    for (uint8_t i = 0; i < k1; ++i) c1[i] = static_cast<uint8_t>(p1_choice[i]);
    for (uint8_t i = 0; i < k2; ++i) c2[i] = static_cast<uint8_t>(p2_choice[i]);
    float value = 0.0f, l1[9], l2[9];
    check(oakgpu_leaf_eval_policy(ctx_.get(), net_, b.bytes, d.bytes, 1, c1, &k1, c2, &k2, &value, l1, l2));
    for (uint8_t i = 0; i < k1; ++i) p1[i] = l1[i];
    for (uint8_t i = 0; i < k2; ++i) p2[i] = l2[i];
    return value;
  }
  // value_policy_inference for every leaf (network.h:102-123): choices / counts as pkmn_gen1_battle_choices fills them (n x 9
  // bytes, n bytes per side); returns the values, fills the n x 9 logit arrays (entries past a count are 0)
  std::vector<float> value_policy_inference(const std::vector<Leaf> &leaves, const std::vector<uint8_t> &p1_choices,
                                            const std::vector<uint8_t> &p1_counts, const std::vector<uint8_t> &p2_choices,
                                            const std::vector<uint8_t> &p2_counts, std::vector<float> &p1_logits, std::vector<float> &p2_logits) {
    const uint32_t n = static_cast<uint32_t>(leaves.size());
    if (p1_choices.size() != size_t{n} * 9 || p2_choices.size() != size_t{n} * 9 || p1_counts.size() != n || p2_counts.size() != n)
      throw std::runtime_error{"oakgpu: choices must be n x 9 bytes and counts n bytes per side"};
    std::vector<uint8_t> battles(size_t{n} * OAKGPU_BATTLE_SIZE), durations(size_t{n} * OAKGPU_DURATIONS_SIZE);
    for (uint32_t i = 0; i < n; ++i) {
      std::memcpy(&battles[size_t{i} * OAKGPU_BATTLE_SIZE], leaves[i].battle, OAKGPU_BATTLE_SIZE);
      std::memcpy(&durations[size_t{i} * OAKGPU_DURATIONS_SIZE], leaves[i].durations, OAKGPU_DURATIONS_SIZE);
    }
    std::vector<float> values(n);
    p1_logits.assign(size_t{n} * 9, 0.0f);
    p2_logits.assign(size_t{n} * 9, 0.0f);
    check(oakgpu_leaf_eval_policy(ctx_.get(), net_, battles.data(), durations.data(), n, p1_choices.data(), p1_counts.data(), p2_choices.data(),
                                  p2_counts.data(), values.data(), p1_logits.data(), p2_logits.data()));
    return values;
  }

  // A RESIDENT batch evaluated every turn (device pointers): party-slot embeddings cached by exact identity tags, the GPU
  // form of NN::Battle::PokemonCache (nn/battle/cache.h:18-131).  `embedding` (n x in_dim floats) and `slot_tags`
  // (n x 10 x OAKGPU_SLOT_TAG_WORDS u32, initialised to 0xFF bytes) are the caller's, kept between calls.
  void value_inference_cached_dev(const uint8_t *battles, const uint8_t *durations, uint32_t n, float *values, float *embedding,
                                  uint32_t *slot_tags) {
    check(oakgpu_leaf_eval_cached_dev(ctx_.get(), net_, battles, durations, n, values, embedding, slot_tags));
  }

  // The same two calls with the bench slots looked up in a filled PartyTable of this network (device pointers; root_of: n root
  // indices on the device, or nullptr = all root 0).  Results equal the plain calls'.
  inline void value_inference_table_dev(PartyTable &table, const uint32_t *root_of, const uint8_t *battles, const uint8_t *durations, uint32_t n,
                                        float *values, float *embedding_out = nullptr);
  inline void value_policy_inference_table_dev(PartyTable &table, const uint32_t *root_of, const uint8_t *battles, const uint8_t *durations, uint32_t n,
                                               const uint8_t *p1_choices, const uint8_t *p1_counts, const uint8_t *p2_choices,
                                               const uint8_t *p2_counts, float *values, float *p1_logits, float *p2_logits);

  oakgpu_net *get() const noexcept { return net_; }

private:
  Context &ctx_;
  oakgpu_net *net_{};
};

// NN::Battle::PokemonCache filled once per root (nn/battle/cache.h:18-131): the 240 embeddings of each of a root battle's 12
// stored Pokemon, after which a leaf's bench slots are row copies.  Fill per search, or once per game -- a team's stored identity
// never changes; a slot the table does not hold is embedded as usual.  The network must outlive the table.
class PartyTable {
public:
  PartyTable(Context &ctx, Network &net, uint32_t max_roots = 1) : ctx_{ctx} { check(oakgpu_party_table_create(ctx.get(), net.get(), max_roots, &t_)); }
  ~PartyTable() { oakgpu_party_table_destroy(ctx_.get(), t_); }
  PartyTable(const PartyTable &) = delete;
  PartyTable &operator=(const PartyTable &) = delete;
  // n_roots x OAKGPU_BATTLE_SIZE bytes on the host (returns with the table complete) / on the device (asynchronous on the context's stream)
  void fill(const uint8_t *root_battles, uint32_t n_roots = 1) { check(oakgpu_party_table_fill(ctx_.get(), t_, root_battles, n_roots)); }
  void fill_dev(const uint8_t *root_battles, uint32_t n_roots = 1) { check(oakgpu_party_table_fill_dev(ctx_.get(), t_, root_battles, n_roots)); }
  int width() const noexcept { return oakgpu_party_table_width(t_); }
  // diagnostics: the 240 x width() rows of one Pokemon; the bench slots the context's last table call had to embed
  std::vector<float> rows(uint32_t root, int side, int pokemon) {
    std::vector<float> out(size_t{240} * static_cast<size_t>(width()));
    check(oakgpu_party_table_rows(ctx_.get(), t_, root, side, pokemon, out.data()));
    return out;
  }
  uint32_t last_misses() {
    uint32_t slots = 0;
    check(oakgpu_party_table_last_misses(ctx_.get(), t_, &slots));
    return slots;
  }
  oakgpu_party_table *get() const noexcept { return t_; }

private:
  Context &ctx_;
  oakgpu_party_table *t_{};
};

inline void Network::value_inference_table_dev(PartyTable &table, const uint32_t *root_of, const uint8_t *battles, const uint8_t *durations, uint32_t n,
                                               float *values, float *embedding_out) {
  check(oakgpu_leaf_eval_table_dev(ctx_.get(), net_, table.get(), root_of, battles, durations, n, values, embedding_out));
}
inline void Network::value_policy_inference_table_dev(PartyTable &table, const uint32_t *root_of, const uint8_t *battles, const uint8_t *durations,
                                                      uint32_t n, const uint8_t *p1_choices, const uint8_t *p1_counts, const uint8_t *p2_choices,
                                                      const uint8_t *p2_counts, float *values, float *p1_logits, float *p2_logits) {
  check(oakgpu_leaf_eval_policy_table_dev(ctx_.get(), net_, table.get(), root_of, battles, durations, n, p1_choices, p1_counts, p2_choices, p2_counts,
                                          values, p1_logits, p2_logits));
}

// RuntimeSearch::Heap (util/search.h:17-32, search.cc:17-58): the tree of a search kept between searches.
class Heap {
public:
  Heap() { check(oakgpu_heap_create(&h_)); }
  ~Heap() { oakgpu_heap_destroy(h_); }
  Heap(const Heap &) = delete;
  Heap &operator=(const Heap &) = delete;
  bool empty() const noexcept { return oakgpu_heap_empty(h_) != 0; }
  // after the joint action (p1 index i, p2 index j) was played and produced `obs` (the 16-byte chance actions): the child
  // becomes the root (true), or nothing could be kept (false) -- search.cc:27-52
  bool update(uint8_t i, uint8_t j, const uint8_t *obs16) { return oakgpu_heap_update(h_, i, j, obs16) != 0; }
  uint64_t nodes() const noexcept { return oakgpu_heap_nodes(h_); }
  oakgpu_heap *get() const noexcept { return h_; }

private:
  oakgpu_heap *h_{};
};

// MCTS::Search::run(device, budget, params, heap, eval, input, output = {}) (mcts.h:154-155): `params.bandit` picks the
// joint bandit, eval = Monte-Carlo (net == nullptr) or the network; heap == nullptr is a fresh Node tree for this call,
// `previous` (nullable) is the Output to add to.  The result carries MCTS::Output's root matrices (mcts.h:68-90).
class TreeSearch {
public:
  explicit TreeSearch(Context &ctx) : ctx_{ctx} {}
  // Start from these, not from `oakgpu_search_params{}`: roll clamping {3, 1} (mcts.h:131) and the DEFAULT Exp3 mixing of an
  // absent agent-string field -- a zeroed struct asks for alpha = 0 (no uniform mixing), which the reference only does on request.
  static oakgpu_search_params default_params() { return oakgpu_search_params OAKGPU_SEARCH_PARAMS_INIT; }
  oakgpu_search_output run(const Leaf &input, oakgpu_search_params params, Network *net = nullptr, Heap *heap = nullptr,
                           const oakgpu_search_output *previous = nullptr) {
    params.eval = net ? 1 : 0;
    oakgpu_search_output out{};
    check(oakgpu_search_heap(ctx_.get(), net ? net->get() : nullptr, heap ? heap->get() : nullptr, input.battle, input.durations, input.result,
                             &params, previous, &out));
    return out;
  }

private:
  Context &ctx_;
};

// RuntimeSearch::Agent (util/search.h:34-64) and RuntimeSearch::run: budget "4096" | "100ms" | "8s", bandit "ucb-1.0" |
// "exp3-0.1-0.05" | ..., eval "mc" | "fp" | <.battle.net path>, matrix_ucb "" | "delay-interval-minimum-c".  Unparsable
// strings throw std::runtime_error with the reference's texts (search.cc:200-307).
struct Agent {
  std::string budget{"4096"}, bandit{"ucb-1.0"}, eval{"mc"}, matrix_ucb{};
  bool discrete{false}, table{false};
};
inline oakgpu_search_output run(Context &ctx, const Leaf &input, const Agent &agent, uint64_t seed, uint32_t batch = 0, Heap *heap = nullptr,
                                const oakgpu_search_output *previous = nullptr) {
  const oakgpu_agent a{agent.budget.c_str(), agent.bandit.c_str(), agent.eval.c_str(), agent.matrix_ucb.c_str(), agent.discrete, agent.table};
  oakgpu_search_output out{};
  check(oakgpu_search_agent_heap(ctx.get(), heap ? heap->get() : nullptr, input.battle, input.durations, input.result, &a, batch, seed, previous, &out));
  return out;
}

// solve_nash of the forest search and the loops over it (and oakgpu_forest_match_params::solve_nash): no solve, the exact solves on the
// host's threads, or on the device (oakgpu_nash_solve_dev: the same bits, nothing leaves the device).  `true` / `false` still mean 1 / 0.
constexpr int NASH_NONE = 0, NASH_HOST = 1, NASH_DEVICE = 2;

// The forest search (include/oakgpu.h: oakgpu_forest_*): up to max_trees searches at once, one GPU lane per tree, every tree resident
// on the device; tree g is TreeSearch::run(roots[g], {params, seed = seeds[g], batch = 1}) iteration for iteration.  params.bandit 0 / 1
// (1 needs contextual = true, eval = 1 and a network), params.eval 0 / 1 / 2; the Nash fields are solved only with solve_nash.
// keep_arena != NO_KEEP makes a kept forest (oakgpu_forest_create_kept: that many nodes a tree, 0 = 4 * max_iterations + 1): its trees go
// on from call to call -- advance() is Heap::update of every tree, search(..., keep = true) the search on the kept trees.
class SearchForest {
public:
  static constexpr uint32_t NO_KEEP = 0xFFFFFFFFu;
  SearchForest(Context &ctx, uint32_t max_trees, uint32_t max_iterations, bool contextual = false, uint32_t keep_arena = NO_KEEP) : ctx_{ctx} {
    if (keep_arena == NO_KEEP) check(oakgpu_forest_create(ctx.get(), max_trees, max_iterations, contextual ? 1 : 0, &f_));
    else check(oakgpu_forest_create_kept(ctx.get(), max_trees, max_iterations, contextual ? 1 : 0, keep_arena, &f_));
  }
  ~SearchForest() { oakgpu_forest_destroy(ctx_.get(), f_); }
  SearchForest(const SearchForest &) = delete;
  SearchForest &operator=(const SearchForest &) = delete;
  // budgets (empty, or one per root): tree g runs budgets[g] <= params.iterations iterations and is, bit for bit, the tree of a search with
  // iterations = budgets[g] (oakgpu_forest_search_budgets*); rows of non-increasing budgets cost no launch over a finished tree
  std::vector<oakgpu_search_output> search(const oakgpu_search_params &params, const std::vector<Leaf> &roots, const std::vector<uint64_t> &seeds,
                                           Network *net = nullptr, int solve_nash = NASH_NONE, std::vector<uint64_t> *streams = nullptr, bool keep = false,
                                           const std::vector<uint32_t> &budgets = {}) {
    if (seeds.size() != roots.size()) throw std::runtime_error{"oakgpu: SearchForest::search: one seed per root"};
    if (!budgets.empty() && budgets.size() != roots.size()) throw std::runtime_error{"oakgpu: SearchForest::search: one budget per root"};
    const uint32_t n = (uint32_t)roots.size();
    std::vector<uint8_t> b((size_t)n * OAKGPU_BATTLE_SIZE), d((size_t)n * OAKGPU_DURATIONS_SIZE), r(n);
    for (uint32_t g = 0; g < n; ++g) {
      std::memcpy(b.data() + (size_t)g * OAKGPU_BATTLE_SIZE, roots[g].battle, OAKGPU_BATTLE_SIZE);
      std::memcpy(d.data() + (size_t)g * OAKGPU_DURATIONS_SIZE, roots[g].durations, OAKGPU_DURATIONS_SIZE);
      r[g] = roots[g].result;
    }
    std::vector<oakgpu_search_output> out(n);
    if (streams) streams->assign(n, 0);
    if (!budgets.empty())
      check((keep ? oakgpu_forest_search_budgets_kept : oakgpu_forest_search_budgets)(f_, net ? net->get() : nullptr, &params, b.data(), d.data(), r.data(), seeds.data(),
                                                                                      budgets.data(), n, out.data(), solve_nash, streams ? streams->data() : nullptr,
                                                                                      nullptr, 0));
    else
      check((keep ? oakgpu_forest_search_kept : oakgpu_forest_search)(f_, net ? net->get() : nullptr, &params, b.data(), d.data(), r.data(), seeds.data(), n,
                                                                      out.data(), solve_nash, streams ? streams->data() : nullptr, nullptr, 0));
    return out;
  }
  // Heap::update of every tree and its move to another row (a kept forest): new tree t continues tree src[t] (src empty: tree t) along the
  // played cell (i[t], j[t]) and the update's 16-byte observation obs[16 t ..]; returns 1 per tree whose child is the root now, 0 = nothing kept
  std::vector<uint8_t> advance(const std::vector<uint8_t> &i, const std::vector<uint8_t> &j, const std::vector<uint8_t> &obs, const std::vector<uint32_t> &src = {}) {
    const uint32_t n = (uint32_t)i.size();
    if (j.size() != n || obs.size() != (size_t)n * 16 || (!src.empty() && src.size() != n)) throw std::runtime_error{"oakgpu: SearchForest::advance: i, j, src n each, obs n x 16"};
    std::vector<uint8_t> kept((size_t)n + 1, 0);
    check(oakgpu_forest_advance(f_, i.data(), j.data(), obs.data(), src.empty() ? nullptr : src.data(), n, kept.data()));
    kept.resize(n);
    return kept;
  }
  // the same over device arrays (src_tree nullable), kept_out on the device too
  void advance_dev(const uint8_t *i, const uint8_t *j, const uint8_t *obs, const uint32_t *src_tree, uint32_t n_new, uint8_t *kept_out) {
    check(oakgpu_forest_advance_dev(f_, i, j, obs, src_tree, n_new, kept_out));
  }
  void search_kept_dev(const oakgpu_search_params &params, const uint8_t *battles, const uint8_t *durations, const uint8_t *results, const uint64_t *seeds,
                       uint32_t n, const oakgpu_forest_outputs &dev_out, Network *net = nullptr) {
    check(oakgpu_forest_search_kept_dev(f_, net ? net->get() : nullptr, &params, battles, durations, results, seeds, n, &dev_out, nullptr, 0));
  }
  // the same over arrays the caller holds on the device (dev_out: device arrays too)
  void search_dev(const oakgpu_search_params &params, const uint8_t *battles, const uint8_t *durations, const uint8_t *results, const uint64_t *seeds,
                  uint32_t n, const oakgpu_forest_outputs &dev_out, Network *net = nullptr) {
    check(oakgpu_forest_search_dev(f_, net ? net->get() : nullptr, &params, battles, durations, results, seeds, n, &dev_out, nullptr, 0));
  }
  // the budgets forms over device arrays (budgets: n x u32 on the device)
  void search_budgets_dev(const oakgpu_search_params &params, const uint8_t *battles, const uint8_t *durations, const uint8_t *results, const uint64_t *seeds,
                          const uint32_t *budgets, uint32_t n, const oakgpu_forest_outputs &dev_out, Network *net = nullptr, bool keep = false) {
    check((keep ? oakgpu_forest_search_budgets_kept_dev : oakgpu_forest_search_budgets_dev)(f_, net ? net->get() : nullptr, &params, battles, durations, results, seeds,
                                                                                            budgets, n, &dev_out, nullptr, 0));
  }
  // tree-iterations of the last search: launched (the sum of the iterations' row counts), run (the sum of the budgets)
  std::array<uint64_t, 2> last_rows() const {
    std::array<uint64_t, 2> out{};
    check(oakgpu_forest_last_rows(f_, out.data()));
    return out;
  }
  // `count` node records of one tree of the last call, from node `first`, in creation order (the root is node 0)
  std::vector<oakgpu_forest_node> nodes(uint32_t tree, uint32_t first, uint32_t count) {
    std::vector<oakgpu_forest_node> out(count);
    oakgpu_forest_node none;
    check(oakgpu_forest_nodes(f_, tree, first, count, count ? out.data() : &none));
    return out;
  }
  oakgpu_forest *get() const noexcept { return f_; }

private:
  Context &ctx_;
  oakgpu_forest *f_{};
};

// Self-play over the forest search (include/oakgpu.h: oakgpu_forest_selfplay*): n games at once, resident on the device; game g is the
// per-game loop of generate.cc:238-322 with batch = 1 and seed = seeds[g].  The records come back as one `.battle.data` byte stream in game
// order (a dropped game -- status OAKGPU_FSP_MAX_LENGTH / _ZERO_POLICY -- has zero bytes), with offsets[n + 1] into it.
class ForestSelfplay {
public:
  struct Result {
    std::vector<uint8_t> stream;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> n_frames;
    std::vector<uint8_t> results, status;
    std::array<uint64_t, 4> stats{}; // turns looped, rows searched summed over turns, compactions, host reads
    std::vector<uint32_t> nodes_kept;      // params.keep_node: per game, the updates that found their child (oakgpu_selfplay_params::nodes_kept); else zeros
    std::array<uint64_t, 4> keep_stats{};  // params.keep_node: sum of nodes_kept, trees dropped for want of room, root mismatches, nodes carried in
    std::array<uint64_t, 4> fast_stats{};  // params.fast_search_prob: fast frames, full frames, tree-iterations launched, tree-iterations run
    std::vector<double> matchup;           // per game: the first search's empirical value (a built seat's trajectory value); NaN if never searched
  };
  explicit ForestSelfplay(SearchForest &forest) : forest_{forest} {}
  // teams: n x 60 bytes; params.search.seed / batch and params.seed are ignored; keep_node = 1 needs a forest made with keep_arena;
  // params.fast_budget / fast_search_prob / fast_policy_mode: generate's fast searches (the forest's max_iterations covers both budgets)
  // built (empty = no game is built; else one byte per game, bit 0 = p1's team was built, bit 1 = p2's) with skip.battle_skip_prob /
  // t1_budget: generate's skipped battles -- such a game has status OAKGPU_FSP_SKIPPED, no record and a matchup
  Result play(const oakgpu_selfplay_params &params, const std::vector<uint8_t> &teams, const std::vector<uint64_t> &battle_seeds,
              const std::vector<uint64_t> &seeds, Network *net = nullptr, int solve_nash = NASH_HOST, const std::vector<uint8_t> &built = {},
              const oakgpu_selfplay_skip &skip = {}) {
    const uint32_t n = (uint32_t)seeds.size();
    if (teams.size() != (size_t)n * 60 || battle_seeds.size() != n) throw std::runtime_error{"oakgpu: ForestSelfplay::play: teams n x 60, one battle seed and one seed per game"};
    if (!built.empty() && built.size() != n) throw std::runtime_error{"oakgpu: ForestSelfplay::play: built is empty or one byte per game"};
    check(oakgpu_forest_selfplay_build(forest_.get(), net ? net->get() : nullptr, &params, &skip, teams.data(), battle_seeds.data(), seeds.data(),
                                       built.empty() ? nullptr : built.data(), n, solve_nash));
    Result out;
    size_t bytes = 0;
    check(oakgpu_forest_selfplay_records(forest_.get(), nullptr, 0, &bytes, nullptr, nullptr, nullptr, nullptr, 0));
    out.stream.resize(bytes);
    out.offsets.assign((size_t)n + 1, 0); out.n_frames.assign(n, 0); out.results.assign(n, 0); out.status.assign(n, 0);
    uint8_t none = 0;
    check(oakgpu_forest_selfplay_records(forest_.get(), bytes ? out.stream.data() : &none, bytes, &bytes, out.offsets.data(), out.n_frames.data(),
                                         out.results.data(), out.status.data(), 0));
    check(oakgpu_forest_selfplay_last_stats(forest_.get(), out.stats.data()));
    out.nodes_kept.assign((size_t)n + 1, 0);
    check(oakgpu_forest_selfplay_nodes_kept(forest_.get(), out.nodes_kept.data(), 0));
    out.nodes_kept.resize(n);
    check(oakgpu_forest_selfplay_keep_stats(forest_.get(), out.keep_stats.data()));
    check(oakgpu_forest_selfplay_fast_stats(forest_.get(), out.fast_stats.data()));
    out.matchup.assign((size_t)n + 1, 0.0);
    check(oakgpu_forest_selfplay_matchup(forest_.get(), out.matchup.data(), 0));
    out.matchup.resize(n);
    return out;
  }

private:
  SearchForest &forest_;
};

// Matches between two search agents over the forest search (include/oakgpu.h: oakgpu_forest_match*): n games at once, resident on the
// device, from the caller's states; seat p1 and seat p2 each search with their own parameters and network and play their own side's
// move -- the per-game loop of vs.cc:230-345 with a budget.  status: OAKGPU_FM_*; log: n x params.log_turns records, game-major, 0xFF
// bytes where no game came.  play(..., records = true) also returns each seat's `.battle.data` byte stream of the games (vs.cc:380-395: what
// `vs` saves under p1/ and p2/), in game order with offsets[n + 1] into it; a game cut at max_turns or stopped by a zeroed policy has zero
// bytes, an unsearched seat's update has iterations 0 (include/oakgpu.h).
class ForestMatch {
public:
  struct Records {
    std::vector<uint8_t> stream;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> n_frames;
  };
  struct Result {
    std::vector<uint8_t> results, status;
    std::vector<uint32_t> turns;
    std::vector<oakgpu_match_turn> log;
    std::array<uint64_t, 4> counts{}; // wins, ties, losses of seat p1 (early stops included), stopped at max_turns
    std::array<uint64_t, 4> stats{};  // turns looped, p1 rows searched, p2 rows searched, host reads of the per-turn record
    std::array<Records, 2> records;   // seat p1's and seat p2's; empty without records
  };
  explicit ForestMatch(SearchForest &forest) : forest_{forest} {}
  // params.p1 / p2 .net: the seats' network handles (Network::get()) or null; one seed per start state
  Result play(const oakgpu_forest_match_params &params, const std::vector<Leaf> &starts, const std::vector<uint64_t> &seeds, bool records = false) {
    if (seeds.size() != starts.size()) throw std::runtime_error{"oakgpu: ForestMatch::play: one seed per start state"};
    const uint32_t n = (uint32_t)starts.size();
    std::vector<uint8_t> b((size_t)n * OAKGPU_BATTLE_SIZE), d((size_t)n * OAKGPU_DURATIONS_SIZE), r(n);
    for (uint32_t g = 0; g < n; ++g) {
      std::memcpy(b.data() + (size_t)g * OAKGPU_BATTLE_SIZE, starts[g].battle, OAKGPU_BATTLE_SIZE);
      std::memcpy(d.data() + (size_t)g * OAKGPU_DURATIONS_SIZE, starts[g].durations, OAKGPU_DURATIONS_SIZE);
      r[g] = starts[g].result;
    }
    Result out;
    out.results.assign(n, 0); out.status.assign(n, 0); out.turns.assign(n, 0);
    out.log.resize((size_t)n * params.log_turns);
    if (!out.log.empty()) std::memset(out.log.data(), 0xFF, out.log.size() * sizeof(oakgpu_match_turn));
    check(oakgpu_forest_match_set_records(forest_.get(), records ? 1 : 0));
    check(oakgpu_forest_match(forest_.get(), &params, b.data(), d.data(), r.data(), seeds.data(), n, out.results.data(), out.turns.data(), out.status.data(),
                              out.log.empty() ? nullptr : out.log.data(), out.counts.data()));
    check(oakgpu_forest_match_last_stats(forest_.get(), out.stats.data()));
    for (int seat = 0; seat < 2 && records; ++seat) {
      Records &rec = out.records[seat];
      size_t bytes = 0;
      check(oakgpu_forest_match_records(forest_.get(), seat, nullptr, 0, &bytes, nullptr, nullptr, nullptr, nullptr, 0));
      rec.stream.resize(bytes);
      rec.offsets.assign((size_t)n + 1, 0); rec.n_frames.assign(n, 0);
      uint8_t none = 0;
      check(oakgpu_forest_match_records(forest_.get(), seat, bytes ? rec.stream.data() : &none, bytes, &bytes, rec.offsets.data(), rec.n_frames.data(), nullptr,
                                        nullptr, 0));
    }
    return out;
  }

private:
  SearchForest &forest_;
};

// Exact Nash equilibrium of an integer m x n (<= 9 x 9) matrix game, row player maximising: {p1, p2, value / discretize}.
inline std::tuple<std::vector<double>, std::vector<double>, double> solve_matrix(const std::vector<int32_t> &payoffs, int m, int n,
                                                                                 int discretize_factor = 256) {
  if (m < 1 || n < 1 || payoffs.size() != static_cast<size_t>(m) * static_cast<size_t>(n)) throw std::runtime_error{"oakgpu: payoff matrix shape"};
  std::vector<double> p1(static_cast<size_t>(m)), p2(static_cast<size_t>(n));
  double value = 0;
  check(oakgpu_solve_matrix(payoffs.data(), m, n, discretize_factor, p1.data(), p2.data(), &value));
  return {p1, p2, value};
}

// A batch of solve_matrix calls on the device (oakgpu_solve_matrices): matrix k is the m[k] x n[k] row-major ints payoffs[k]; entry k of the
// result is solve_matrix(payoffs[k], m[k], n[k], discretize_factor) bit for bit, and what that call refuses fails the whole call.
inline std::vector<std::tuple<std::vector<double>, std::vector<double>, double>> solve_matrices(Context &ctx, const std::vector<std::vector<int32_t>> &payoffs,
                                                                                                const std::vector<int> &m, const std::vector<int> &n,
                                                                                                int discretize_factor = 256) {
  const size_t count = payoffs.size();
  if (m.size() != count || n.size() != count) throw std::runtime_error{"oakgpu: solve_matrices: one m and one n per matrix"};
  std::vector<int32_t> flat(count * 81 + 1, 0), ms(count + 1, 0), ns(count + 1, 0);
  for (size_t k = 0; k < count; ++k) {
    if (m[k] < 1 || n[k] < 1 || m[k] > 9 || n[k] > 9 || payoffs[k].size() != static_cast<size_t>(m[k]) * static_cast<size_t>(n[k]))
      throw std::runtime_error{"oakgpu: payoff matrix shape"};
    std::copy(payoffs[k].begin(), payoffs[k].end(), flat.begin() + static_cast<std::ptrdiff_t>(k * 81));
    ms[k] = m[k]; ns[k] = n[k];
  }
  std::vector<double> p1(count * 9 + 1), p2(count * 9 + 1), value(count + 1);
  check(oakgpu_solve_matrices(ctx.get(), flat.data(), ms.data(), ns.data(), static_cast<uint32_t>(count), discretize_factor, p1.data(), p2.data(), value.data()));
  std::vector<std::tuple<std::vector<double>, std::vector<double>, double>> out;
  for (size_t k = 0; k < count; ++k)
    out.emplace_back(std::vector<double>(p1.begin() + static_cast<std::ptrdiff_t>(k * 9), p1.begin() + static_cast<std::ptrdiff_t>(k * 9 + ms[k])),
                     std::vector<double>(p2.begin() + static_cast<std::ptrdiff_t>(k * 9), p2.begin() + static_cast<std::ptrdiff_t>(k * 9 + ns[k])), value[k]);
  return out;
}

// benchmark.cc:23-31 + mcts.h:250-263,448-496 on the device: `n` playouts from one root, every draw taken from ONE
// std::mt19937{seed} in the reference's sequential order (playout i starts where playout i - 1 stopped).
class SharedDeviceRollout {
public:
  explicit SharedDeviceRollout(Context &ctx) : ctx_{ctx} {}
  RolloutResult run(const Leaf &root, uint32_t seed, uint32_t n, uint32_t max_steps = 100000, std::vector<uint8_t> *final_battles = nullptr) {
    RolloutResult out{std::vector<float>(n), std::vector<uint32_t>(n), std::vector<uint8_t>(n)};
    if (final_battles) final_battles->assign(size_t{n} * OAKGPU_BATTLE_SIZE, 0);
    for (size_t draws = size_t{n} * 160 + 4096;; draws *= 2) { // grow the generator's output until n playouts fit
      if (draws > (size_t{1} << 30)) throw std::runtime_error{"oakgpu: the shared generator's stream would exceed 2^30 draws"}; // (before the cast below)
      std::vector<uint64_t> stream(draws);
      check(oakgpu_mt19937_fill(seed, 0, stream.data(), stream.size()));
      uint64_t used = 0;
      const int rc = oakgpu_rollout_shared_device(ctx_.get(), root.battle, root.durations, root.result, stream.data(), static_cast<uint32_t>(draws), n,
                                                  max_steps, 1, out.result.data(), out.steps.data(), out.value.data(),
                                                  final_battles ? final_battles->data() : nullptr, nullptr, nullptr, &used);
      if (rc == 0) return out;
      if (draws > (size_t{1} << 30) || std::string{oakgpu_last_error()}.find("too short") == std::string::npos) check(rc);
    }
  }

private:
  Context &ctx_;
};

// One game's `.battle.data` record under construction (CompressedFrames: battle after the opening update, one Update per
// turn, the final result byte); bytes() serialises it in the reference's on-disk layout.
class Frames {
public:
  explicit Frames(const uint8_t *first_battle) { std::memcpy(battle_, first_battle, OAKGPU_BATTLE_SIZE); }
  void push(const oakgpu_search_output &o, uint8_t c1, uint8_t c2) { // Update{search_output, c1, c2} (compressed-frame.h:66-75)
    oakgpu_frame_update u{};
    u.m = o.m; u.n = o.n; u.c1 = c1; u.c2 = c2;
    u.iterations = static_cast<uint32_t>(o.iterations);
    u.empirical_value = o.empirical_value;
    u.nash_value = o.nash_value;
    for (int k = 0; k < 9; ++k) { u.p1_empirical[k] = o.p1_empirical[k]; u.p1_nash[k] = o.p1_nash[k]; u.p2_empirical[k] = o.p2_empirical[k]; u.p2_nash[k] = o.p2_nash[k]; }
    updates_.push_back(u);
  }
  std::vector<uint8_t> bytes(uint8_t result) const {
    std::vector<uint8_t> out(oakgpu_frames_size(updates_.data(), static_cast<uint32_t>(updates_.size())));
    size_t written = 0;
    check(oakgpu_frames_write(battle_, result, updates_.data(), static_cast<uint32_t>(updates_.size()), out.data(), out.size(), &written));
    out.resize(written);
    return out;
  }

private:
  uint8_t battle_[OAKGPU_BATTLE_SIZE];
  std::vector<oakgpu_frame_update> updates_;
};

// The replay check of a `.battle.data` file's bytes on the GPU (oakgpu_replay_records; the rules are in oakgpu.h): one report per
// record, its byte offset, where indexing stopped, and with want_states the battle and durations at each verdict.
struct ReplayCheck {
  std::vector<oakgpu_replay_report> reports;
  std::vector<uint64_t> offsets;
  size_t stopped_at = 0;
  std::vector<uint8_t> battles, durations; // n x 384, n x 8 (want_states)
};
inline ReplayCheck replay_check(Context &ctx, const std::vector<uint8_t> &bytes, bool want_states = false) {
  ReplayCheck out;
  uint32_t n = 0;
  check(oakgpu_replay_index(bytes.data(), bytes.size(), nullptr, nullptr, nullptr, 0, &n, &out.stopped_at));
  if (n == 0) return out;
  out.offsets.resize(n);
  std::vector<uint16_t> frames(n);
  std::vector<uint8_t> malformed(n);
  check(oakgpu_replay_index(bytes.data(), bytes.size(), out.offsets.data(), frames.data(), malformed.data(), n, &n, nullptr));
  out.reports.resize(n);
  if (want_states) { out.battles.resize(size_t{n} * OAKGPU_BATTLE_SIZE); out.durations.resize(size_t{n} * 8); }
  check(oakgpu_replay_records(ctx.get(), bytes.data(), bytes.size(), out.reports.data(), n, &n, &out.stopped_at,
                              want_states ? out.battles.data() : nullptr, want_states ? out.durations.data() : nullptr));
  return out;
}

// A training batch in host memory: the reference's EncodedFrames + Target fields (py/battle/encoded-frames.h:23-41, py/battle/target.h:17-40)
// as flat row-major vectors, plus status / where / picks (the contract of a row is in oakgpu.h).
struct EncodedFrames {
  explicit EncodedFrames(size_t sz)
      : size{sz}, pokemon(sz * 2 * 6 * 198), active(sz * 2 * 229), hp(sz * 2 * 6), empirical_policies(sz * 18), nash_policies(sz * 18), empirical_value(sz),
        nash_value(sz), score(sz), choice_indices(sz * 18), k(sz * 2), choice(sz * 2), status(sz), iterations(sz), where(sz), picks(sz * 2) {}
  size_t size;
  std::vector<float> pokemon, active, hp, empirical_policies, nash_policies, empirical_value, nash_value, score;
  std::vector<int64_t> choice_indices;
  std::vector<uint8_t> k, choice, status;
  std::vector<uint32_t> iterations, where, picks;
  oakgpu_encoded_frames pointers() {
    return oakgpu_encoded_frames{pokemon.data(), active.data(), hp.data(), choice_indices.data(), k.data(), choice.data(), iterations.data(),
                                 empirical_policies.data(), nash_policies.data(), empirical_value.data(), nash_value.data(), score.data(), status.data(),
                                 where.data()};
  }
};

// `.battle.data` records on the device (oakgpu_corpus_*): uploaded and indexed once, then batches are drawn (pyoak.sample's rule, pyoak.cc:111-245)
// or picked, replayed and encoded on the GPU.  Must not outlive its Context.  Both calls return the number of OK rows.
class FrameCorpus {
public:
  FrameCorpus(Context &ctx, const std::vector<uint8_t> &bytes) : ctx_{ctx.get()} { check(oakgpu_corpus_create(ctx_, bytes.data(), bytes.size(), &corpus_)); }
  ~FrameCorpus() { oakgpu_corpus_destroy(corpus_); }
  FrameCorpus(const FrameCorpus &) = delete;
  FrameCorpus &operator=(const FrameCorpus &) = delete;
  oakgpu_corpus *get() const noexcept { return corpus_; }
  oakgpu_corpus_stats info() const {
    oakgpu_corpus_stats st{};
    check(oakgpu_corpus_info(corpus_, &st));
    return st;
  }
  // rows 0 .. n-1 of `out` from out.picks[0 .. 2n) = (record, frame) pairs
  uint32_t encode(EncodedFrames &out, uint32_t n) {
    if (n > out.size) throw std::runtime_error{"oakgpu: more picks than rows"};
    const oakgpu_encoded_frames p = out.pointers();
    uint32_t ok = 0;
    check(oakgpu_frames_encode(ctx_, corpus_, out.picks.data(), n, &p, &ok));
    return ok;
  }
  uint32_t sample(EncodedFrames &out, uint64_t seed, uint32_t max_battle_length = 0, uint32_t min_iterations = 1) {
    const oakgpu_encoded_frames p = out.pointers();
    uint32_t ok = 0;
    check(oakgpu_frames_sample(ctx_, corpus_, static_cast<uint32_t>(out.size), seed, max_battle_length, min_iterations, out.picks.data(), &p, &ok));
    return ok;
  }
  // ---- every frame of the corpus (oakgpu_corpus_inference / _evaluate): record r owns rows bases[r] .. bases[r+1]-1
  std::vector<uint64_t> frame_bases() const {
    std::vector<uint64_t> bases(static_cast<size_t>(info().records) + 1);
    check(oakgpu_corpus_frame_bases(corpus_, bases.data()));
    return bases;
  }
  // pyoak.cpp_inference's fields for every row, flat row-major: value [F], policy_logit / policy [F,2,9], k [F,2], status, where [F]
  struct Output {
    std::vector<float> value, policy_logit, policy;
    std::vector<uint8_t> k, choices, status;
    std::vector<uint32_t> where;
  };
  Output inference(Network &net, uint32_t chunk_rows = 0) {
    const size_t rows = static_cast<size_t>(info().frames);
    Output o;
    o.value.resize(rows); o.policy_logit.resize(rows * 18); o.policy.resize(rows * 18); o.k.resize(rows * 2); o.choices.resize(rows * 18);
    o.status.resize(rows); o.where.resize(rows);
    const oakgpu_corpus_eval p{o.value.data(), o.policy_logit.data(), o.policy.data(), o.k.data(), o.choices.data(), o.status.data(), o.where.data()};
    check(oakgpu_corpus_inference(ctx_, net.get(), corpus_, 0, info().records, chunk_rows, &p));
    return o;
  }
  // battle.py's loss terms over the corpus; per_record (nullable) receives one entry per record
  oakgpu_corpus_losses evaluate(Network &net, const oakgpu_loss_params &p, uint32_t chunk_rows = 0, std::vector<oakgpu_corpus_losses> *per_record = nullptr) {
    oakgpu_corpus_losses total{};
    if (per_record) per_record->assign(std::max<size_t>(info().records, 1), oakgpu_corpus_losses{});
    check(oakgpu_corpus_evaluate(ctx_, net.get(), corpus_, &p, chunk_rows, &total, per_record ? per_record->data() : nullptr));
    if (per_record) per_record->resize(info().records);
    return total;
  }

protected:
  explicit FrameCorpus(oakgpu_ctx *ctx) : ctx_{ctx} {} // (ReplayWindow makes its own corpus)
  oakgpu_ctx *ctx_{};
  oakgpu_corpus *corpus_{};
};

// A corpus that starts empty and keeps the newest records appended to it (oakgpu_corpus_create_window: the contract is in oakgpu.h): every
// FrameCorpus call on it returns what it returns on FrameCorpus{ctx, window.records()}.
class ReplayWindow : public FrameCorpus {
public:
  struct Stats { uint64_t records, bytes, appended, evicted, rejected, appends; };
  ReplayWindow(Context &ctx, uint32_t max_records, size_t max_bytes) : FrameCorpus{ctx.get()} {
    check(oakgpu_corpus_create_window(ctx_, max_records, max_bytes, &corpus_));
  }
  // device arrays as oakgpu_forest_selfplay_records leaves them with to_device = 1: record i = bytes offsets[i] .. offsets[i+1]
  Stats append_dev(const uint8_t *stream, const uint64_t *offsets, uint32_t n) {
    check(oakgpu_corpus_append_dev(ctx_, corpus_, stream, offsets, n));
    return stats();
  }
  // host bytes, cut into records by their length fields
  Stats append(const std::vector<uint8_t> &bytes) {
    check(oakgpu_corpus_append(ctx_, corpus_, bytes.data(), bytes.size()));
    return stats();
  }
  Stats stats() const {
    uint64_t v[6] = {};
    check(oakgpu_corpus_window_stats(corpus_, v));
    return Stats{v[0], v[1], v[2], v[3], v[4], v[5]};
  }
  // the surviving records back to back: a `.battle.data` file's bytes
  std::vector<uint8_t> records() {
    size_t size = 0;
    check(oakgpu_corpus_records(ctx_, corpus_, nullptr, 0, &size, 0));
    std::vector<uint8_t> out(size);
    if (size) check(oakgpu_corpus_records(ctx_, corpus_, out.data(), out.size(), &size, 0));
    return out;
  }
  void save(const std::string &path) {
    const std::vector<uint8_t> data = records();
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (data.size() && fwrite(data.data(), 1, data.size(), f) != data.size())) { if (f) fclose(f); throw std::runtime_error{"oakgpu: cannot write " + path}; }
    fclose(f);
  }
};

// The optimiser step of a battle network on the device (oakgpu_trainer_*): parameters, gradients and Adam's state of one `.battle.net`, trained on
// rows of an EncodedFrames (host rows, staged; the _dev calls of oakgpu.h take device rows).  Must not outlive its Context.
class Trainer {
public:
  Trainer(Context &ctx, const std::vector<uint8_t> &net_bytes, uint32_t max_rows) : ctx_{ctx.get()} {
    check(oakgpu_trainer_create(ctx_, net_bytes.data(), net_bytes.size(), max_rows, &trainer_));
    check(oakgpu_trainer_shape(trainer_, nullptr, &count_, nullptr));
  }
  ~Trainer() { oakgpu_trainer_destroy(trainer_); }
  Trainer(const Trainer &) = delete;
  Trainer &operator=(const Trainer &) = delete;
  oakgpu_trainer *get() const noexcept { return trainer_; }
  size_t count() const noexcept { return count_; }   // floats per block: the 24 tensors in file order
  // host only: throws naming what create, or a call of n rows with this loss, would refuse
  static void check_net(const std::vector<uint8_t> &net_bytes, uint32_t max_rows, uint32_t n = 0, const oakgpu_train_loss *loss = nullptr) {
    check(oakgpu_trainer_check(net_bytes.data(), net_bytes.size(), max_rows, n, loss));
  }
  // value [n], logits [n,2,9], sq_err [n], ce [n,2] of rows 0 .. n-1 (each vector nullable)
  void forward(EncodedFrames &rows, uint32_t n, const oakgpu_train_loss &loss, std::vector<float> *value = nullptr, std::vector<float> *logits = nullptr,
               std::vector<float> *sq_err = nullptr, std::vector<float> *ce = nullptr) {
    if (n > rows.size) throw std::runtime_error{"oakgpu: more rows than the batch holds"};
    if (value) value->assign(n, 0.0f);
    if (logits) logits->assign(static_cast<size_t>(n) * 18, 0.0f);
    if (sq_err) sq_err->assign(n, 0.0f);
    if (ce) ce->assign(static_cast<size_t>(n) * 2, 0.0f);
    const oakgpu_encoded_frames p = rows.pointers();
    const oakgpu_train_outputs out{value ? value->data() : nullptr, logits ? logits->data() : nullptr, sq_err ? sq_err->data() : nullptr, ce ? ce->data() : nullptr};
    check(oakgpu_trainer_forward(ctx_, trainer_, &p, n, &loss, &out));
  }
  void gradients(EncodedFrames &rows, uint32_t n, const oakgpu_train_loss &loss) {
    if (n > rows.size) throw std::runtime_error{"oakgpu: more rows than the batch holds"};
    const oakgpu_encoded_frames p = rows.pointers();
    check(oakgpu_trainer_gradients(ctx_, trainer_, &p, n, &loss));
  }
  void adam(float lr, bool clamp_weights = false, uint32_t groups = OAKGPU_GROUP_TRUNK | OAKGPU_GROUP_VALUE | OAKGPU_GROUP_POLICY) {
    check(oakgpu_trainer_adam_dev(ctx_, trainer_, lr, clamp_weights ? 1 : 0, groups));
  }
  void step(EncodedFrames &rows, uint32_t n, const oakgpu_train_loss &loss, float lr, bool clamp_weights = false) {
    if (n > rows.size) throw std::runtime_error{"oakgpu: more rows than the batch holds"};
    const oakgpu_encoded_frames p = rows.pointers();
    check(oakgpu_trainer_step(ctx_, trainer_, &p, n, &loss, lr, clamp_weights ? 1 : 0));
  }
  // waits for the device; steps (nullable): the three groups' step counts
  oakgpu_train_report report(uint64_t steps[3] = nullptr) {
    oakgpu_train_report r{};
    check(oakgpu_trainer_report(ctx_, trainer_, &r, steps));
    return r;
  }
  std::vector<float> read(int which = OAKGPU_TRAIN_PARAMETERS) {
    std::vector<float> block(count_);
    check(oakgpu_trainer_read(ctx_, trainer_, which, block.data(), count_));
    return block;
  }
  void set_gradients(const std::vector<float> &block) { check(oakgpu_trainer_set_gradients(ctx_, trainer_, block.data(), block.size())); }
  std::vector<uint8_t> net_bytes() {
    size_t size = 0;
    check(oakgpu_trainer_net_bytes(ctx_, trainer_, nullptr, 0, &size));
    std::vector<uint8_t> out(size);
    check(oakgpu_trainer_net_bytes(ctx_, trainer_, out.data(), out.size(), &size));
    return out;
  }

private:
  oakgpu_ctx *ctx_{};
  oakgpu_trainer *trainer_{};
  size_t count_{};
};

// The team-building network on the device (oakgpu_build_*): a `.build.net`'s policy net, the rollout that completes teams with it and the
// provider of `generate` (TeamBuilding::Provider::get_trajectory).  Host vectors in and out.  Must not outlive its Context.
class BuildNet {
public:
  // What one call leaves: per row the completed team, the number of steps, and per step the action's cell, its position in the legal list,
  // the list's length and the probability; provide also the team the rollout started from (what a record's initial cells are), its size
  // and the pool index of an unchanged team (-1 for a built one).
  struct Trajectories {
    uint32_t n{};
    std::vector<uint8_t> teams_out, n_updates, teams_init, sizes;
    std::vector<uint16_t> action, index, n_legal;
    std::vector<float> prob;
    std::vector<int32_t> team_index;
  };
  BuildNet(Context &ctx, const std::vector<uint8_t> &net_bytes) : ctx_{ctx.get()} {
    check(oakgpu_build_net_load(ctx_, net_bytes.data(), net_bytes.size(), &net_));
  }
  ~BuildNet() { oakgpu_build_net_destroy(net_); }
  BuildNet(const BuildNet &) = delete;
  BuildNet &operator=(const BuildNet &) = delete;
  oakgpu_build_net *get() const noexcept { return net_; }
  // host only: throws naming what load would refuse
  static void check_net(const std::vector<uint8_t> &net_bytes) { check(oakgpu_build_net_check(net_bytes.data(), net_bytes.size())); }
  // teams: n x 30 bytes; sizes: n bytes or empty (6); seeds: n
  Trajectories rollout(const std::vector<uint8_t> &teams, const std::vector<uint64_t> &seeds, const std::vector<uint8_t> &sizes = {}, int input_update = 0) {
    const uint32_t n = static_cast<uint32_t>(seeds.size());
    if (teams.size() != static_cast<size_t>(n) * 30 || (!sizes.empty() && sizes.size() != n)) throw std::runtime_error{"oakgpu: teams, sizes and seeds disagree"};
    Trajectories t = make(n, false);
    const oakgpu_build_outputs out = pointers(t, false);
    check(oakgpu_build_rollout(ctx_, net_, teams.data(), sizes.empty() ? nullptr : sizes.data(), seeds.data(), n, input_update, &out));
    t.teams_init = teams;
    t.sizes = sizes.empty() ? std::vector<uint8_t>(n, 6) : sizes;
    return t;
  }
  // pool: T x 30 bytes
  Trajectories provide(const std::vector<uint8_t> &pool, const std::vector<uint64_t> &seeds, const oakgpu_build_provider &prm) {
    const uint32_t n = static_cast<uint32_t>(seeds.size());
    if (pool.size() % 30) throw std::runtime_error{"oakgpu: a pool is whole teams of 30 bytes"};
    Trajectories t = make(n, true);
    const oakgpu_build_outputs out = pointers(t, true);
    check(oakgpu_build_provide(ctx_, net_, pool.data(), static_cast<uint32_t>(pool.size() / 30), seeds.data(), n, &prm, &out));
    return t;
  }
  // the `.build.data` records of the built rows, in row order; a negative score means none
  std::vector<uint8_t> records(const Trajectories &t, const std::vector<float> &value, const std::vector<float> &score) {
    if (value.size() != t.n || score.size() != t.n) throw std::runtime_error{"oakgpu: one value and one score per row"};
    std::vector<uint8_t> out(static_cast<size_t>(t.n) * OAKGPU_BUILD_RECORD_BYTES);
    uint32_t count = 0;
    check(oakgpu_build_records(ctx_, t.teams_init.data(), t.sizes.data(), t.n_updates.data(), t.action.data(), t.prob.data(), value.data(), score.data(), t.n,
                               out.data(), &count));
    out.resize(static_cast<size_t>(count) * OAKGPU_BUILD_RECORD_BYTES);
    return out;
  }

private:
  static Trajectories make(uint32_t n, bool provide) {
    Trajectories t;
    const size_t steps = static_cast<size_t>(n) * OAKGPU_BUILD_MAX_STEPS;
    t.n = n;
    t.teams_out.assign(static_cast<size_t>(n) * 30, 0);
    t.n_updates.assign(n, 0);
    t.action.assign(steps, 0);
    t.index.assign(steps, 0);
    t.n_legal.assign(steps, 0);
    t.prob.assign(steps, 0.0f);
    if (provide) {
      t.teams_init.assign(static_cast<size_t>(n) * 30, 0);
      t.sizes.assign(n, 0);
      t.team_index.assign(n, 0);
    }
    return t;
  }
  static oakgpu_build_outputs pointers(Trajectories &t, bool provide) {
    oakgpu_build_outputs o{};
    o.teams_out = t.teams_out.data();
    o.n_updates = t.n_updates.data();
    o.action = t.action.data();
    o.index = t.index.data();
    o.n_legal = t.n_legal.data();
    o.prob = t.prob.data();
    if (provide) {
      o.teams_init = t.teams_init.data();
      o.sizes_out = t.sizes.data();
      o.team_index = t.team_index.data();
    }
    return o;
  }
  oakgpu_ctx *ctx_{};
  oakgpu_build_net *net_{};
};

// `.build.data` files resident on the device and read back into training arrays (oakgpu_build_corpus_*, oakgpu_build_traj*,
// oakgpu_build_targets): the reference's read_build_trajectories and the network-free half of build.py's process_targets.  Host vectors in
// and out.  Must not outlive its Context.
class BuildTrajectories {
public:
  struct Rows { // what a decode leaves, row-major: [n, 31] per step, [n, 31, 339] the mask (empty when not asked for), [n] per row
    uint32_t n{}, t_max{};
    std::vector<int64_t> action, mask, start, end;
    std::vector<uint16_t> n_legal;
    std::vector<float> policy, value, score;
    std::vector<uint8_t> status;
    std::vector<uint32_t> picks;
  };
  struct Targets { // valid / rewards [n, 31]; rows [V, 2], state_cells [V, 31], state_n / old_logp [V]
    uint32_t n_valid{};
    std::vector<uint8_t> valid, state_n;
    std::vector<uint32_t> rows;
    std::vector<uint16_t> state_cells;
    std::vector<float> old_logp, rewards;
  };
  // files: the bytes of each `.build.data` file
  BuildTrajectories(Context &ctx, const std::vector<std::vector<uint8_t>> &files) : ctx_{ctx.get()} {
    std::vector<uint8_t> all;
    std::vector<size_t> sizes;
    for (const auto &f : files) {
      all.insert(all.end(), f.begin(), f.end());
      sizes.push_back(f.size());
    }
    check(oakgpu_build_corpus_create(ctx_, all.data(), all.size(), sizes.data(), static_cast<uint32_t>(sizes.size()), &corpus_));
  }
  ~BuildTrajectories() { if (owned_) oakgpu_build_corpus_destroy(corpus_); }
  BuildTrajectories(const BuildTrajectories &) = delete;
  BuildTrajectories &operator=(const BuildTrajectories &) = delete;
  oakgpu_build_corpus *get() const noexcept { return corpus_; }
  // host only: the status of every record (OAKGPU_BUILD_TRAJ_*)
  static std::vector<uint8_t> check_records(const std::vector<uint8_t> &bytes) {
    std::vector<uint8_t> status(bytes.size() / OAKGPU_BUILD_RECORD_BYTES);
    check(oakgpu_build_traj_check(bytes.data(), bytes.size(), status.data()));
    return status;
  }
  oakgpu_build_corpus_stats info() {
    oakgpu_build_corpus_stats st{};
    check(oakgpu_build_corpus_info(corpus_, &st));
    return st;
  }
  Rows decode(const std::vector<uint32_t> &picks, bool with_mask = true, bool no_score = false) {
    Rows r = make(static_cast<uint32_t>(picks.size()), with_mask);
    const oakgpu_build_trajectories out = pointers(r);
    const oakgpu_build_traj_params prm{OAKGPU_BUILD_MASK_INT64, no_score ? 1 : 0};
    check(oakgpu_build_traj(ctx_, corpus_, picks.data(), r.n, &prm, &out));
    r.picks = picks;
    return r;
  }
  Rows sample(uint32_t n, uint64_t seed, bool with_mask = true, bool no_score = false) {
    Rows r = make(n, with_mask);
    r.picks.assign(n, 0);
    const oakgpu_build_trajectories out = pointers(r);
    const oakgpu_build_traj_params prm{OAKGPU_BUILD_MASK_INT64, no_score ? 1 : 0};
    check(oakgpu_build_traj_sample(ctx_, corpus_, n, seed, &prm, r.picks.data(), &out));
    return r;
  }
  Targets targets(Rows &r, double value_weight) {
    const size_t steps = static_cast<size_t>(r.n) * OAKGPU_BUILD_MAX_STEPS;
    Targets t;
    t.valid.assign(steps, 0); t.state_n.assign(steps, 0); t.rows.assign(steps * 2, 0); t.state_cells.assign(steps * OAKGPU_BUILD_MAX_STEPS, 0);
    t.old_logp.assign(steps, 0.0f); t.rewards.assign(steps, 0.0f);
    const oakgpu_build_trajectories in = pointers(r);
    const oakgpu_build_target_outputs out{t.valid.data(), &t.n_valid, t.rows.data(), t.state_cells.data(), t.state_n.data(), t.old_logp.data(), t.rewards.data()};
    check(oakgpu_build_targets(ctx_, &in, r.n, value_weight, &out));
    t.state_n.resize(t.n_valid); t.rows.resize(static_cast<size_t>(t.n_valid) * 2); t.state_cells.resize(static_cast<size_t>(t.n_valid) * OAKGPU_BUILD_MAX_STEPS);
    t.old_logp.resize(t.n_valid);
    return t;
  }

protected:
  BuildTrajectories(Context &ctx, oakgpu_build_corpus *borrowed) : ctx_{ctx.get()}, corpus_{borrowed}, owned_{false} {} // (BuildWindow's corpus)

private:
  static Rows make(uint32_t n, bool with_mask) {
    Rows r;
    const size_t steps = static_cast<size_t>(n) * OAKGPU_BUILD_MAX_STEPS;
    r.n = n;
    r.action.assign(steps, 0); r.n_legal.assign(steps, 0); r.policy.assign(steps, 0.0f);
    if (with_mask) r.mask.assign(steps * OAKGPU_BUILD_MAX_ACTIONS, 0);
    r.start.assign(n, 0); r.end.assign(n, 0); r.value.assign(n, 0.0f); r.score.assign(n, 0.0f); r.status.assign(n, 0);
    return r;
  }
  static oakgpu_build_trajectories pointers(Rows &r) {
    return oakgpu_build_trajectories{r.action.data(), r.mask.empty() ? nullptr : r.mask.data(), r.n_legal.data(), r.policy.data(), r.value.data(), r.score.data(),
                                     r.start.data(), r.end.data(), r.status.data(), &r.t_max};
  }
  oakgpu_ctx *ctx_{};
  oakgpu_build_corpus *corpus_{};
  bool owned_{true};
};

// The newest max_records `.build.data` records resident on the device (oakgpu_build_window_*): self-play appends, the oldest leave first,
// and info / decode / sample / targets are BuildTrajectories' on the surviving records as one file, oldest first.  Must not outlive its Context.
class BuildWindow : public BuildTrajectories {
public:
  BuildWindow(Context &ctx, uint32_t max_records) : BuildWindow(ctx, make_window(ctx, max_records)) {}
  ~BuildWindow() { oakgpu_build_window_destroy(window_); }
  oakgpu_build_window *window() const noexcept { return window_; }
  void append(const std::vector<uint8_t> &bytes) { check(oakgpu_build_window_append(wctx_, window_, bytes.data(), bytes.size())); }
  // device records (16-byte aligned) and a device count word, as oakgpu_build_game_records_dev leaves them
  void append_dev(const uint8_t *records, const uint32_t *count, uint32_t max_count) { check(oakgpu_build_window_append_dev(wctx_, window_, records, count, max_count)); }
  std::vector<uint8_t> records() {
    size_t bytes = 0;
    check(oakgpu_build_window_records(window_, nullptr, 0, &bytes));
    std::vector<uint8_t> out(bytes + 1);
    check(oakgpu_build_window_records(window_, out.data(), bytes, &bytes));
    out.resize(bytes);
    return out;
  }
  std::array<uint64_t, 4> stats() const { // records held, appended, evicted, rejected
    std::array<uint64_t, 4> out{};
    check(oakgpu_build_window_stats(window_, out.data()));
    return out;
  }

private:
  static oakgpu_build_window *make_window(Context &ctx, uint32_t max_records) {
    oakgpu_build_window *w = nullptr;
    check(oakgpu_build_window_create(ctx.get(), max_records, &w));
    return w;
  }
  BuildWindow(Context &ctx, oakgpu_build_window *w) : BuildTrajectories(ctx, oakgpu_build_window_corpus(w)), wctx_{ctx.get()}, window_{w} {}
  oakgpu_ctx *wctx_{};
  oakgpu_build_window *window_{};
};

// The optimiser step of the reference's build.py on the device, for the three-layer nets of a `.build.net` (oakgpu_build_trainer_*; the
// rule is in oakgpu.h, "Training the build network").  A chunk's arrays are DEVICE arrays, as oakgpu_build_traj_dev and
// oakgpu_build_targets_dev write them; parameters, gradients and nets cross as host vectors in file order.  Must not outlive its Context.
class BuildTrainer {
public:
  BuildTrainer(Context &ctx, const std::vector<uint8_t> &net_bytes, uint32_t max_traj) : ctx_{ctx.get()} {
    check(oakgpu_build_trainer_create(ctx_, net_bytes.data(), net_bytes.size(), max_traj, &t_));
    check(oakgpu_build_trainer_shape(t_, dims_, &count_, &max_traj_));
  }
  ~BuildTrainer() { oakgpu_build_trainer_destroy(t_); }
  BuildTrainer(const BuildTrainer &) = delete;
  BuildTrainer &operator=(const BuildTrainer &) = delete;
  oakgpu_build_trainer *get() const noexcept { return t_; }
  // host only: the refusals of the constructor, by name
  static void check_net(const std::vector<uint8_t> &net_bytes, uint32_t max_traj) { check(oakgpu_build_trainer_check(net_bytes.data(), net_bytes.size(), max_traj)); }
  size_t count() const noexcept { return count_; }
  uint32_t max_traj() const noexcept { return max_traj_; }
  std::pair<uint32_t, uint32_t> layer(int k) const { return {dims_[2 * k], dims_[2 * k + 1]}; }   // (in, out) of layer k of six, file order
  void forward_dev(const oakgpu_build_chunk &chunk, const oakgpu_build_train_outputs *out = nullptr) { check(oakgpu_build_trainer_forward_dev(ctx_, t_, &chunk, out)); }
  void accumulate_dev(const oakgpu_build_chunk &chunk) { check(oakgpu_build_trainer_accumulate_dev(ctx_, t_, &chunk)); }
  void zero_gradients() { check(oakgpu_build_trainer_zero_gradients_dev(ctx_, t_)); }
  void adam(float lr) { check(oakgpu_build_trainer_adam_dev(ctx_, t_, lr)); }
  void average(double gamma) { check(oakgpu_build_trainer_average_dev(ctx_, t_, gamma)); }
  oakgpu_build_train_report report() {
    oakgpu_build_train_report r{};
    check(oakgpu_build_trainer_report(ctx_, t_, &r));
    return r;
  }
  std::vector<float> read(int which = OAKGPU_BUILD_TRAIN_PARAMETERS) {
    std::vector<float> out(count_);
    check(oakgpu_build_trainer_read(ctx_, t_, which, out.data(), out.size()));
    return out;
  }
  void set_gradients(const std::vector<float> &grads) { check(oakgpu_build_trainer_set_gradients(ctx_, t_, grads.data(), grads.size())); }
  std::vector<uint8_t> net_bytes(int which = OAKGPU_BUILD_TRAIN_PARAMETERS) {
    size_t size = 0;
    check(oakgpu_build_trainer_net_bytes(ctx_, t_, which, nullptr, 0, &size));
    std::vector<uint8_t> out(size);
    check(oakgpu_build_trainer_net_bytes(ctx_, t_, which, out.data(), out.size(), &size));
    return out;
  }

private:
  oakgpu_ctx *ctx_{};
  oakgpu_build_trainer *t_{};
  uint32_t dims_[12]{};
  size_t count_{};
  uint32_t max_traj_{};
};

// The path's one exchange step for root-parallel search sharded over the GPUs of a node (one process per GPU): reduce the
// rank's leaf values to one mean per root on the device, then ONE ncclAllGather (RCCL over xGMI) of those means.
class Exchange {
public:
  // id128: made by rank 0 with Exchange::unique_id() and handed to the other ranks out of band
  Exchange(Context &ctx, const uint8_t *id128, int rank, int world) : ctx_{ctx} { check(oakgpu_comm_create(ctx_.get(), id128, rank, world, &comm_)); }
  ~Exchange() { oakgpu_comm_destroy(comm_); }
  Exchange(const Exchange &) = delete;
  Exchange &operator=(const Exchange &) = delete;
  static std::vector<uint8_t> unique_id() {
    std::vector<uint8_t> id(128);
    check(oakgpu_comm_unique_id(id.data()));
    return id;
  }
  // device pointers, asynchronous on the context's stream: means[r] = mean(values[r * per_root ...]); all = world x roots
  void root_means_all_gather_dev(const float *values, uint32_t roots, uint32_t per_root, float *means, float *all) {
    check(oakgpu_segment_mean_dev(ctx_.get(), values, roots, per_root, means));
    check(oakgpu_all_gather_dev(ctx_.get(), comm_, means, all, roots));
  }

  // the sliced search steps' exchange: `count` 64-bit aggregates (count | 2 x value sum << 32, OakGPU::RootSteps) per rank
  void aggregates_all_gather_dev(const unsigned long long *mine, unsigned long long *all, size_t count) {
    check(oakgpu_all_gather_dev(ctx_.get(), comm_, reinterpret_cast<const float *>(mine), reinterpret_cast<float *>(all), 2 * count));
  }

private:
  Context &ctx_;
  oakgpu_comm *comm_{};
};

// BASELINE configs[3] as search steps that do not wait for their longest playout (oakgpu_root_steps_*, include/oakgpu.h): every launch
// advances each playout in flight by at most `slice` turn-steps; a playout of len turn-steps started in step k is credited to step
// k + (len - 1) / slice of its root and travels between launches on a carry list.  The reference's analogue: the generator's workers never
// wait for each other (cpp/src/generate.cc:527-536); per-playout prep = mcts.h:250-263, the playout = mcts.h:448-496.
class RootSteps {
public:
  RootSteps(Context &ctx, uint32_t roots, uint32_t replicas, uint32_t slice = 16, uint32_t max_steps = 1000) : roots_{roots} {
    check(oakgpu_root_steps_create(ctx.get(), roots, replicas, slice, max_steps, &rs_));
  }
  ~RootSteps() { oakgpu_root_steps_destroy(rs_); }
  RootSteps(const RootSteps &) = delete;
  RootSteps &operator=(const RootSteps &) = delete;
  // device pointers, asynchronous on the context's stream.  report: roots + 2 u64 -- [r] count | (2 x value sum) << 32 of the playouts
  // credited to this step, [roots] turn-steps executed, [roots + 1] carried playouts | error word << 32.  fresh = false: a drain step.
  void launch_dev(const uint8_t *root_battles, const uint8_t *root_durations, const uint8_t *root_results, uint8_t *lane_prng,
                  unsigned long long *report, bool fresh = true) {
    check(oakgpu_root_steps_launch_dev(rs_, root_battles, root_durations, root_results, lane_prng, fresh ? 1 : 0, report));
  }
  static uint32_t credited(unsigned long long a) { return static_cast<uint32_t>(a); }
  static double mean_value(unsigned long long a) { return credited(a) ? static_cast<double>(a >> 32) / (2.0 * credited(a)) : 0.5; }
  uint32_t roots() const { return roots_; }

private:
  oakgpu_root_steps *rs_{};
  uint32_t roots_;
};

// Whole games between two policies, a batch resident on the device (oakgpu_policy_games*, include/oakgpu.h): the reference's `vs`
// (cpp/src/vs.cc:107-408) with --budget=0 --bandit=pucb-1.0 --policy-mode=p, where each side samples its network's root prior.
class PolicyGames {
public:
  struct Params {
    const Network *p1 = nullptr, *p2 = nullptr; // nullptr: a RANDOM seat (the rollout's rule)
    double p1_temp = 1, p1_min = 0, p2_temp = 1, p2_min = 0; // RuntimePolicy::Options (util/policy.h:8-12)
    uint32_t max_turns = 1000, poll = 16;
    float compact_below = 0.5f;
    uint32_t log_turns = 0;
  };
  struct Result {
    std::vector<uint8_t> result;      // final pkmn_result byte (type 0: stopped at max_turns)
    std::vector<uint32_t> turns;      // updates made
    std::vector<float> value;         // 1 / 0 / 0.5 for seat p1
    std::vector<uint8_t> choice_log;  // n x log_turns x 2 (c1, c2); 0xFF where a game did not get
    uint64_t wins = 0, ties = 0, losses = 0, stopped = 0;
  };
  PolicyGames(Context &ctx, const Params &params) : ctx_{ctx}, log_turns_{params.log_turns} {
    p_.p1 = oakgpu_seat{params.p1 ? OAKGPU_SEAT_POLICY : OAKGPU_SEAT_RANDOM, params.p1 ? params.p1->get() : nullptr, params.p1_temp, params.p1_min};
    p_.p2 = oakgpu_seat{params.p2 ? OAKGPU_SEAT_POLICY : OAKGPU_SEAT_RANDOM, params.p2 ? params.p2->get() : nullptr, params.p2_temp, params.p2_min};
    p_.max_turns = params.max_turns;
    p_.poll = params.poll;
    p_.compact_below = params.compact_below;
    p_.log_turns = params.log_turns;
  }
  // device pointers (n games; the outputs by game index, battles_out / durations_out / choice_log nullable); returns {wins, ties, losses, stopped}
  std::array<uint64_t, 4> run_dev(const uint8_t *battles, const uint8_t *durations, const uint8_t *results_in, uint8_t *prng_state, uint32_t n,
                                  uint8_t *results_out, uint32_t *turns_out, float *values_out, uint8_t *battles_out = nullptr,
                                  uint8_t *durations_out = nullptr, uint8_t *choice_log = nullptr) {
    std::array<uint64_t, 4> counts{};
    check(oakgpu_policy_games_dev(ctx_.get(), &p_, battles, durations, results_in, prng_state, n, results_out, turns_out, values_out, battles_out,
                                  durations_out, choice_log, counts.data()));
    return counts;
  }
  // host form: the games start at `leaves`; device_rng holds one fast_prng state per game and is advanced; the leaves receive the final states
  Result run(std::vector<Leaf> &leaves, std::vector<uint64_t> &device_rng) {
    const uint32_t n = static_cast<uint32_t>(leaves.size());
    if (device_rng.size() != n) throw std::runtime_error{"oakgpu: one RNG state per game required"};
    std::vector<uint8_t> battles(size_t{n} * OAKGPU_BATTLE_SIZE), durations(size_t{n} * OAKGPU_DURATIONS_SIZE), results(n);
    for (uint32_t i = 0; i < n; ++i) {
      std::memcpy(&battles[size_t{i} * OAKGPU_BATTLE_SIZE], leaves[i].battle, OAKGPU_BATTLE_SIZE);
      std::memcpy(&durations[size_t{i} * OAKGPU_DURATIONS_SIZE], leaves[i].durations, OAKGPU_DURATIONS_SIZE);
      results[i] = leaves[i].result;
    }
    Result out{std::vector<uint8_t>(n), std::vector<uint32_t>(n), std::vector<float>(n), std::vector<uint8_t>(size_t{n} * log_turns_ * 2, 0xFF)};
    uint64_t counts[4] = {};
    check(oakgpu_policy_games(ctx_.get(), &p_, battles.data(), durations.data(), results.data(), reinterpret_cast<uint8_t *>(device_rng.data()), n,
                              out.result.data(), out.turns.data(), out.value.data(), battles.data(), durations.data(),
                              log_turns_ ? out.choice_log.data() : nullptr, counts));
    for (uint32_t i = 0; i < n; ++i) {
      std::memcpy(leaves[i].battle, &battles[size_t{i} * OAKGPU_BATTLE_SIZE], OAKGPU_BATTLE_SIZE);
      std::memcpy(leaves[i].durations, &durations[size_t{i} * OAKGPU_DURATIONS_SIZE], OAKGPU_DURATIONS_SIZE);
      leaves[i].result = out.result[i];
    }
    out.wins = counts[0]; out.ties = counts[1]; out.losses = counts[2]; out.stopped = counts[3];
    return out;
  }

private:
  Context &ctx_;
  oakgpu_policy_games_params p_{};
  uint32_t log_turns_;
};

} // namespace OakGPU
