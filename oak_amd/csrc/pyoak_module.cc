// oak_amd/csrc/pyoak_module.cc -- the Python face of the boundary: a pybind11 module with pyoak's names
// (cpp/src/pyoak.cc:428-716) over the C ABI of liboakgpu.so.  Import as `from oak_amd import pyoak`.
//
//   Heap(), Agent() {budget, bandit, eval, matrix_ucb, discrete, table}, Input()        pyoak.cc:442-454
//   parse_battle(battle_string, seed = 0x123456) -> Input                                 :456-466
//   update(input, c1, c2)                                                                 :468-478
//   Output {iterations, empirical_value, nash_value, duration_ms, visit_matrix[9,9], value_matrix[9,9],
//           p{1,2}_{prior,empirical,nash}[9]}                                             :494-574
//   search(input, heap, agent, output = Output()) -> Output                               :575-583
//   cpp_inference(record, network_path, discrete, budget) -> value / policy_logit / policy :331-392, 709
//   corpus_inference(paths_or_bytes, network_path, discrete) -> the same three fields for EVERY frame of many records at once
//           (+ k, status, where, picks): one walk per record and one evaluator call per chunk of rows (oakgpu_corpus_inference)
//   solve_matrix(row_payoff, discretize_factor) -> (p1, p2, value)                        :394-426, 711
//   read_battle_data(path) -> [(bytes, frame_count), ...]                                 :43-71, 713
//   policy_games(battles, durations, results, prng, p1_network, p2_network, ...) -> whole games between two networks' raw policies, the
//           per-game loop of `vs --budget=0 --bandit=pucb-1.0 --policy-mode=p` (vs.cc:107-408) for a batch at once (oakgpu_policy_games)
//   selfplay_forest(teams, battle_seeds, seeds, agent, policy_mode, ...) -> n self-play games at once over the forest search, the per-game
//           loop of `generate` (generate.cc:238-322) as one `.battle.data` byte stream (oakgpu_forest_selfplay)
//   match_forest(battles, durations, results, seeds, agent_p1, agent_p2, policy_p1, policy_p2, ..., records) -> n games between two SEARCH agents at
//           once over the forest search, the per-game loop of `vs` with a budget (vs.cc:230-345) (oakgpu_forest_match)
//   network hyper-parameter constants                                                    :586-596
//   EncodedBattleFrames(size) {the reference's numpy fields + status, where, picks}, clear(), from_bytes(bytes, size)  py/battle/encoded-frames.h
//   SampleIndexer() {get(path), prune(paths), size()}, sample(encoded_frames, indexer, threads, max_battle_length, min_iterations)  :73-245
// Every battle operation goes through the C ABI (GPU); this file holds no battle arithmetic.  The battle training-data loader
// (EncodedBattleFrames, SampleIndexer, sample) is the GPU loader of include/oakgpu.h behind the reference's names: the indexer's
// files are uploaded once as a corpus (again when a path joins or leaves, or a file's size or time of last write changes) and a call draws, replays and encodes `size` rows on
// the device, then copies them into the numpy fields; `threads` is accepted and ignored, the seed comes from std::random_device
// as in the reference.  oak_amd/train.py is the same loader on torch tensors, without the copy.  BuildTrajectories(size) and
// read_build_trajectories(trajectories, paths, threads) are the GPU reader of `.build.data` behind the reference's names (:247-329, :697-715).  Heap keeps the tree between searches (RuntimeSearch::Heap over oakgpu_heap; its C++
// `update(i, j, obs)` is exposed too, and `update(input, c1, c2)` returns the 16-byte observation that call needs), an
// `output` passed to search() is resumed like MCTS::Search::run's by-value Output (mcts.h:153-155), p{1,2}_prior are the
// softmax of the root's policy logits for contextual bandits (mcts.h:196-209).  cpp_inference takes a game record as
// read_battle_data returns it (the reference's BattleFrames loader is not carried over) and replays it exactly like
// pyoak.cc:331-392.  battle_string / parse_battle are served by the Python host mirror.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <memory>
#include <mutex>
#include <random>
#include <stdexcept>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/oakgpu.h"

namespace py = pybind11;

namespace {

struct Input { // MCTS::Input (search/mcts.h:62-66): battle + public durations + result
  uint8_t battle[OAKGPU_BATTLE_SIZE] = {};
  uint8_t durations[OAKGPU_DURATIONS_SIZE] = {};
  uint8_t result = 0;
};
struct Heap { // RuntimeSearch::Heap (util/search.h:17-32): the tree of the last search, kept (oakgpu_heap)
  oakgpu_heap *h = nullptr;
  Heap() { if (oakgpu_heap_create(&h) != 0) throw std::runtime_error(oakgpu_last_error()); }
  Heap(const Heap &) = delete;
  Heap &operator=(const Heap &) = delete;
  ~Heap() { oakgpu_heap_destroy(h); }
  bool empty() const { return oakgpu_heap_empty(h) != 0; }
  std::string type() const {
    static const char *names[5] = {"UCB", "PUCB", "UCB1", "Exp3", "PExp3"};
    const int k = oakgpu_heap_kind(h);
    return k < 0 ? "std::monostate" : std::string("MCTS::Node<") + names[k] + "::JointBandit>";
  }
};
struct Agent { // RuntimeSearch::AgentParams (util/search.h:34-43)
  std::string budget = "4096", bandit = "ucb-1.0", eval = "mc", matrix_ucb;
  bool discrete = false, table = false;
};
struct Output { // MCTS::Output (search/mcts.h:68-90) as pyoak exposes it
  oakgpu_search_output raw{};
};

void check(int rc) {
  if (rc != 0) throw std::runtime_error(oakgpu_last_error());
}

// solve_nash of the forest calls: False / True, "host" / "device", or the C ABI's 0 / 1 / 2 (2: the root matrices are solved on the GPU)
int nash_mode(const py::object &v) {
  if (py::isinstance<py::str>(v)) {
    const std::string s = v.cast<std::string>();
    if (s == "device") return 2;
    if (s == "host") return 1;
    throw std::runtime_error("solve_nash: True / False, \"host\", \"device\" or 0 / 1 / 2");
  }
  if (!py::isinstance<py::bool_>(v) && py::isinstance<py::int_>(v) && v.cast<long>() == 2) return 2;
  return v.cast<bool>() ? 1 : 0;
}

std::mutex g_ctx_mu; // a context serves one caller at a time; search() drops the GIL, so two Python threads could meet here
oakgpu_ctx *context() { // one context per process, created on first use (device from OAKGPU_DEVICE, default 0)
  static oakgpu_ctx *ctx = nullptr;
  if (!ctx) {
    const char *env = std::getenv("OAKGPU_DEVICE");
    check(oakgpu_create(&ctx, env ? std::atoi(env) : 0));
  }
  return ctx;
}

// Py::Battle::EncodedFrames + Target (py/battle/encoded-frames.h:23-50, py/battle/target.h:17-53): the same numpy fields, plus the
// loader's status / where per row (include/oakgpu.h)
struct EncodedBattleFrames {
  size_t size;
  py::array_t<float> pokemon, active, hp;
  py::array_t<int64_t> choice_indices;
  py::array_t<uint8_t> k, choice;
  py::array_t<uint32_t> iterations;
  py::array_t<float> empirical_policies, nash_policies, empirical_value, nash_value, score;
  py::array_t<uint8_t> status;
  py::array_t<uint32_t> where, picks; // picks: the (record, frame) behind each row, records counted over the indexer's files in path order
  explicit EncodedBattleFrames(size_t sz)
      : size{sz}, pokemon(std::vector<size_t>{sz, 2, 6, 198}), active(std::vector<size_t>{sz, 2, 1, 229}), hp(std::vector<size_t>{sz, 2, 6, 1}),
        choice_indices(std::vector<size_t>{sz, 2, 9}), k(std::vector<size_t>{sz, 2, 1}), choice(std::vector<size_t>{sz, 2, 1}),
        iterations(std::vector<size_t>{sz, 1}), empirical_policies(std::vector<size_t>{sz, 2, 9}), nash_policies(std::vector<size_t>{sz, 2, 9}),
        empirical_value(std::vector<size_t>{sz, 1}), nash_value(std::vector<size_t>{sz, 1}), score(std::vector<size_t>{sz, 1}),
        status(std::vector<size_t>{sz}), where(std::vector<size_t>{sz}), picks(std::vector<size_t>{sz, 2}) {
    clear();
  }
  template <class T> static void zero(py::array_t<T> &a) { std::fill_n(a.mutable_data(), a.size(), T{}); }
  void clear() {
    zero(pokemon); zero(active); zero(hp); zero(choice_indices); zero(k); zero(choice); zero(iterations); zero(empirical_policies);
    zero(nash_policies); zero(empirical_value); zero(nash_value); zero(score); zero(status); zero(where); zero(picks);
  }
  oakgpu_encoded_frames pointers() {
    return oakgpu_encoded_frames{pokemon.mutable_data(), active.mutable_data(), hp.mutable_data(), choice_indices.mutable_data(), k.mutable_data(),
                                 choice.mutable_data(), iterations.mutable_data(), empirical_policies.mutable_data(), nash_policies.mutable_data(),
                                 empirical_value.mutable_data(), nash_value.mutable_data(), score.mutable_data(), status.mutable_data(),
                                 where.mutable_data()};
  }
};

std::vector<char> read_file(const std::string &path, const char *who) {
  std::ifstream file(path, std::ios::binary);
  if (!file) throw std::runtime_error(std::string(who) + ": Failed to open file: " + path);
  return std::vector<char>((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
}

// SampleIndexer (pyoak.cc:73-109): path -> [(byte offset, frame count), ...]; here it also owns the device corpus of its files
struct SampleIndexer {
  std::map<std::string, py::list> data;
  oakgpu_corpus *corpus = nullptr;
  struct FileKey { // a file as uploaded: a file that grew or was rewritten under its name is read again
    std::string path;
    uintmax_t size;
    std::filesystem::file_time_type written;
    bool operator==(const FileKey &o) const { return path == o.path && size == o.size && written == o.written; }
  };
  std::vector<FileKey> corpus_files;
  SampleIndexer() = default;
  SampleIndexer(const SampleIndexer &) = delete;
  SampleIndexer &operator=(const SampleIndexer &) = delete;
  ~SampleIndexer() {
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    drop();
  }
  void drop() { // (under g_ctx_mu)
    if (corpus) oakgpu_corpus_destroy(corpus);
    corpus = nullptr;
    corpus_files.clear();
  }
  size_t size() const { return data.size(); }
  py::list get(const std::string &path) {
    auto it = data.find(path);
    if (it != data.end()) return it->second;
    const std::vector<char> bytes = read_file(path, "SampleIndexer.get");
    uint32_t n = 0;
    size_t stop = 0;
    check(oakgpu_replay_index((const uint8_t *)bytes.data(), bytes.size(), nullptr, nullptr, nullptr, 0, &n, &stop));
    std::vector<uint64_t> offs(n ? n : 1);
    std::vector<uint16_t> frames(n ? n : 1);
    std::vector<uint8_t> malformed(n ? n : 1);
    if (n) check(oakgpu_replay_index((const uint8_t *)bytes.data(), stop, offs.data(), frames.data(), malformed.data(), n, &n, nullptr));
    py::list out;
    for (uint32_t i = 0; i < n; ++i) out.append(py::make_tuple((int)offs[i], (int)frames[i]));
    data[path] = out;
    return out;
  }
  void prune(const std::vector<std::string> &paths) { // keeps the listed paths only
    for (auto it = data.begin(); it != data.end();)
      it = std::find(paths.begin(), paths.end(), it->first) == paths.end() ? data.erase(it) : std::next(it);
  }
  // The files of `data`, in path order, uploaded once per set of (path, size, time of last write); under g_ctx_mu.  A changed set is
  // read and concatenated in host memory again as a whole.  The lists get() returned are not refreshed (the reference's are not).
  oakgpu_corpus *device_corpus() {
    std::vector<FileKey> files;
    for (const auto &kv : data) {
      std::error_code ec1, ec2;
      const uintmax_t size = std::filesystem::file_size(kv.first, ec1);
      const auto written = std::filesystem::last_write_time(kv.first, ec2);
      if (ec1 || ec2) throw std::runtime_error("sample: Failed to open file: " + kv.first);
      files.push_back(FileKey{kv.first, size, written});
    }
    if (corpus && files == corpus_files) return corpus;
    drop();
    std::vector<uint8_t> all;
    for (const auto &file : files) {
      const std::string &path = file.path;
      const std::vector<char> bytes = read_file(path, "sample");
      uint32_t n = 0;
      size_t stop = 0; // (bytes behind a record whose length cannot be trusted are left out, so that the next file's records follow)
      check(oakgpu_replay_index((const uint8_t *)bytes.data(), bytes.size(), nullptr, nullptr, nullptr, 0, &n, &stop));
      all.insert(all.end(), bytes.begin(), bytes.begin() + (std::ptrdiff_t)stop);
    }
    check(oakgpu_corpus_create(context(), all.data(), all.size(), &corpus));
    corpus_files = files;
    return corpus;
  }
};

// Py::Build::Trajectories (py/build/trajectories.h:105-134): the reference's seven numpy fields in its shapes, plus the reader's status
struct BuildTrajectories {
  size_t size;
  py::array_t<int64_t> action, mask, start, end;
  py::array_t<float> policy, value, score;
  py::array_t<uint8_t> status;
  explicit BuildTrajectories(size_t sz)
      : size{sz}, action(std::vector<size_t>{sz, 31, 1}), mask(std::vector<size_t>{sz, 31, OAKGPU_BUILD_MAX_ACTIONS}), start(std::vector<size_t>{sz, 1}),
        end(std::vector<size_t>{sz, 1}), policy(std::vector<size_t>{sz, 31, 1}), value(std::vector<size_t>{sz, 1}), score(std::vector<size_t>{sz, 1}),
        status(std::vector<size_t>{sz}) {
    clear();
  }
  void clear() {
    using E = EncodedBattleFrames;
    E::zero(action); E::zero(mask); E::zero(start); E::zero(end); E::zero(policy); E::zero(value); E::zero(score); E::zero(status);
  }
};

// The corpus behind read_build_trajectories: the listed files, uploaded once per list of (path, size, time of last write); under g_ctx_mu
struct BuildCorpusCache {
  std::vector<SampleIndexer::FileKey> files;
  oakgpu_build_corpus *corpus = nullptr;
  oakgpu_build_corpus *get(const std::vector<std::string> &paths) {
    std::vector<SampleIndexer::FileKey> now;
    for (const auto &path : paths) {
      std::error_code ec1, ec2;
      const uintmax_t size = std::filesystem::file_size(path, ec1);
      const auto written = std::filesystem::last_write_time(path, ec2);
      if (ec1 || ec2) throw std::runtime_error("read_build_trajectories: Failed to open file: " + path);
      now.push_back(SampleIndexer::FileKey{path, size, written});
    }
    if (corpus && now == files) return corpus;
    if (corpus) oakgpu_build_corpus_destroy(corpus);
    corpus = nullptr;
    files.clear();
    std::vector<uint8_t> all;
    std::vector<size_t> sizes;
    for (const auto &path : paths) {
      const std::vector<char> bytes = read_file(path, "read_build_trajectories");
      all.insert(all.end(), bytes.begin(), bytes.end());
      sizes.push_back(bytes.size());
    }
    check(oakgpu_build_corpus_create(context(), all.data(), all.size(), sizes.data(), (uint32_t)sizes.size(), &corpus));
    files = now;
    return corpus;
  }
};
BuildCorpusCache g_build_corpus;

template <class T, class F> py::array_t<T> vec9(F f) {
  py::array_t<T> arr(9);
  auto r = arr.template mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < 9; ++i) r(i) = f((int)i);
  return arr;
}

} // namespace

PYBIND11_MODULE(pyoak, m) {
  m.doc() = "pyoak-compatible bindings over liboakgpu.so (MI355X)";

  py::class_<Heap>(m, "Heap")
      .def(py::init<>())
      .def("empty", &Heap::empty)
      .def("type", &Heap::type)
      // RuntimeSearch::Heap::update(i, j, obs) (search.cc:27-52; not bound by pyoak, used by its C++ callers vs.cc / chall.cc)
      .def("update", [](Heap &hp, int i, int j, py::bytes obs) {
             const std::string o = obs;
             if (o.size() != 16) throw std::runtime_error("Heap.update: obs must be 16 bytes");
             return oakgpu_heap_update(hp.h, (uint8_t)i, (uint8_t)j, (const uint8_t *)o.data()) != 0;
           }, py::arg("i"), py::arg("j"), py::arg("obs"))
      .def("nodes", [](const Heap &hp) { return (size_t)oakgpu_heap_nodes(hp.h); });

  py::class_<Agent>(m, "Agent")
      .def(py::init<>())
      .def_readwrite("budget", &Agent::budget)
      .def_readwrite("bandit", &Agent::bandit)
      .def_readwrite("eval", &Agent::eval)
      .def_readwrite("matrix_ucb", &Agent::matrix_ucb)
      .def_readwrite("discrete", &Agent::discrete)
      .def_readwrite("table", &Agent::table);

  py::class_<Input>(m, "Input")
      .def(py::init<>())
      // not in pyoak (its Input is opaque): raw views for tests and for feeding the batched C ABI
      .def_property_readonly("battle", [](const Input &i) { return py::bytes((const char *)i.battle, sizeof i.battle); })
      .def_property_readonly("durations", [](const Input &i) { return py::bytes((const char *)i.durations, sizeof i.durations); })
      .def_property_readonly("result", [](const Input &i) { return (int)i.result; });

  m.def(
      "parse_battle",
      [](const std::string &battle_string, uint64_t seed) {
        // Parse::parse_battle (util/parse.h:14-282) lives in the Python host mirror (oak_amd/parse.py)
        py::object mod = py::module_::import("oak_amd.parse");
        py::tuple bd = mod.attr("parse_battle")(battle_string, seed).cast<py::tuple>();
        auto b = bd[0].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
        auto d = bd[1].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
        if (b.size() != OAKGPU_BATTLE_SIZE || d.size() != OAKGPU_DURATIONS_SIZE) throw std::runtime_error("parse_battle: bad array sizes");
        Input in;
        std::memcpy(in.battle, b.data(), sizeof in.battle);
        std::memcpy(in.durations, d.data(), sizeof in.durations);
        in.result = mod.attr("result_from_state")(bd[0]).cast<uint8_t>(); // PKMN::result(battle), pkmn.h:235-272
        return in;
      },
      py::arg("battle_string"), py::arg("seed") = 0x123456);

  m.def(
      "update",
      [](Input &input, uint8_t c1, uint8_t c2) { // options <- durations; PKMN::update; durations <- options (pyoak.cc:468-478)
        uint8_t actions[16];
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        check(oakgpu_update(context(), input.battle, &c1, &c2, input.durations, actions, nullptr, 1, &input.result));
        return py::bytes((const char *)actions, 16); // the observation of this update (pyoak returns None): Heap.update's obs
      },
      py::arg("input"), py::arg("c1"), py::arg("c2"));

  m.def(
      "choices",
      [](const Input &input) { // not in pyoak: PKMN::choices(battle, result) (pkmn.h:141-156) for both players
        uint8_t c1[9], c2[9], n1 = 0, n2 = 0;
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        check(oakgpu_choices(context(), input.battle, &input.result, 0, c1, &n1, 1));
        check(oakgpu_choices(context(), input.battle, &input.result, 1, c2, &n2, 1));
        return py::make_tuple(std::vector<int>(c1, c1 + n1), std::vector<int>(c2, c2 + n2));
      },
      py::arg("input"));

  m.def(
      "battle_string",
      [](const Input &input) {
        py::object mod = py::module_::import("oak_amd.parse");
        return mod.attr("battle_string")(py::bytes((const char *)input.battle, 384), py::bytes((const char *)input.durations, 8)).cast<std::string>();
      },
      py::arg("input"));

  py::class_<Output>(m, "Output")
      .def(py::init<>())
      .def_property_readonly("iterations", [](const Output &o) { return o.raw.iterations; })
      .def_property_readonly("empirical_value", [](const Output &o) { return o.raw.empirical_value; })
      .def_property_readonly("nash_value", [](const Output &o) { return o.raw.nash_value; })
      .def_property_readonly("duration_ms", [](const Output &o) { return o.raw.duration_us / 1e3; })
      .def_property_readonly("m", [](const Output &o) { return (int)o.raw.m; })
      .def_property_readonly("n", [](const Output &o) { return (int)o.raw.n; })
      .def_property_readonly("p1_choices", [](const Output &o) { return std::vector<int>(o.raw.p1_choices, o.raw.p1_choices + o.raw.m); })
      .def_property_readonly("p2_choices", [](const Output &o) { return std::vector<int>(o.raw.p2_choices, o.raw.p2_choices + o.raw.n); })
      .def_property_readonly("visit_matrix",
                             [](const Output &o) {
                               py::array_t<size_t> arr({9, 9});
                               auto r = arr.mutable_unchecked<2>();
                               for (int i = 0; i < 9; ++i)
                                 for (int j = 0; j < 9; ++j) r(i, j) = (i < o.raw.m && j < o.raw.n) ? o.raw.visit_matrix[i * 9 + j] : 0;
                               return arr;
                             })
      .def_property_readonly("value_matrix",
                             [](const Output &o) {
                               py::array_t<double> arr({9, 9});
                               auto r = arr.mutable_unchecked<2>();
                               for (int i = 0; i < 9; ++i)
                                 for (int j = 0; j < 9; ++j) r(i, j) = (i < o.raw.m && j < o.raw.n) ? o.raw.value_matrix[i * 9 + j] : 0.0;
                               return arr;
                             })
      .def_property_readonly("initial_value", [](const Output &o) { return o.raw.initial_value; })
      .def_property_readonly("p1_logit", [](const Output &o) { return vec9<double>([&](int i) { return o.raw.p1_logit[i]; }); })
      .def_property_readonly("p2_logit", [](const Output &o) { return vec9<double>([&](int i) { return o.raw.p2_logit[i]; }); })
      .def_property_readonly("p1_prior", [](const Output &o) { return vec9<double>([&](int i) { return o.raw.p1_prior[i]; }); })
      .def_property_readonly("p2_prior", [](const Output &o) { return vec9<double>([&](int i) { return o.raw.p2_prior[i]; }); })
      .def_property_readonly("p1_empirical", [](const Output &o) { return vec9<double>([&](int i) { return o.raw.p1_empirical[i]; }); })
      .def_property_readonly("p2_empirical", [](const Output &o) { return vec9<double>([&](int i) { return o.raw.p2_empirical[i]; }); })
      .def_property_readonly("p1_nash", [](const Output &o) { return vec9<double>([&](int i) { return o.raw.p1_nash[i]; }); })
      .def_property_readonly("p2_nash", [](const Output &o) { return vec9<double>([&](int i) { return o.raw.p2_nash[i]; }); });

  m.def(
      "format",
      [](const Input &input, const Output &o) { // MCTS::output_string(output, input), pyoak.cc:487-492
        py::object mod = py::module_::import("oak_amd.parse");
        py::dict d;
        const int mm = o.raw.m, nn = o.raw.n;
        d["m"] = mm; d["n"] = nn;
        d["iterations"] = (uint64_t)o.raw.iterations;
        d["duration_ms"] = o.raw.duration_us / 1e3;
        d["empirical_value"] = o.raw.empirical_value;
        d["p1_choices"] = std::vector<int>(o.raw.p1_choices, o.raw.p1_choices + mm);
        d["p2_choices"] = std::vector<int>(o.raw.p2_choices, o.raw.p2_choices + nn);
        d["p1_empirical"] = std::vector<double>(o.raw.p1_empirical, o.raw.p1_empirical + 9);
        d["p2_empirical"] = std::vector<double>(o.raw.p2_empirical, o.raw.p2_empirical + 9);
        d["p1_nash"] = std::vector<double>(o.raw.p1_nash, o.raw.p1_nash + 9);
        d["p2_nash"] = std::vector<double>(o.raw.p2_nash, o.raw.p2_nash + 9);
        d["p1_prior"] = std::vector<double>(o.raw.p1_prior, o.raw.p1_prior + 9);
        d["p2_prior"] = std::vector<double>(o.raw.p2_prior, o.raw.p2_prior + 9);
        py::array_t<double> vis({9, 9}), val({9, 9});
        auto rv = vis.mutable_unchecked<2>(); auto rw = val.mutable_unchecked<2>();
        for (int i = 0; i < 9; ++i)
          for (int j = 0; j < 9; ++j) { rv(i, j) = (double)o.raw.visit_matrix[i * 9 + j]; rw(i, j) = o.raw.value_matrix[i * 9 + j]; }
        d["visit_matrix"] = vis; d["value_matrix"] = val;
        return mod.attr("format_output")(py::bytes((const char *)input.battle, 384), d).cast<std::string>();
      },
      py::arg("input"), py::arg("output"));

  m.def(
      "search",
      [](const Input &input, Heap &heap, Agent &agent, Output previous, uint32_t batch, py::object seed) {
        const oakgpu_agent a{agent.budget.c_str(), agent.bandit.c_str(), agent.eval.c_str(), agent.matrix_ucb.c_str(), agent.discrete, agent.table};
        // pyoak seeds its device from std::random_device on every call (pyoak.cc:579); a seed may be given for reproducibility
        const uint64_t s = seed.is_none() ? ((uint64_t)std::random_device{}() << 32) ^ std::random_device{}() : seed.cast<uint64_t>();
        Output out;
        int rc;
        {
          py::gil_scoped_release release; // the search is long and touches no Python state
          std::lock_guard<std::mutex> lock(g_ctx_mu);
          // RuntimeSearch::run(device, input, heap, agent, output) (pyoak.cc:575-583): the heap's tree and `output` are resumed
          rc = oakgpu_search_agent_heap(context(), heap.h, input.battle, input.durations, input.result, &a, batch, s, &previous.raw, &out.raw);
        }
        check(rc);
        return out;
      },
      py::arg("input"), py::arg("heap"), py::arg("agent"), py::arg("output") = Output{}, py::arg("batch") = 0, py::arg("seed") = py::none());

  m.def(
      "search_forest",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> battles, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> durations,
         py::array_t<uint8_t, py::array::c_style | py::array::forcecast> results, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> seeds,
         Agent &agent, py::object solve_nash_arg, py::object budgets_arg) {
        const int solve_nash = nash_mode(solve_nash_arg);
        // budgets (None, or n x uint32): tree g runs budgets[g] <= the agent's budget iterations (oakgpu_forest_search_budgets)
        std::vector<uint32_t> budgets;
        const bool with_budgets = !budgets_arg.is_none();
        if (with_budgets) {
          auto arr = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(budgets_arg);
          if (!arr || (size_t)arr.size() != (size_t)results.size()) throw std::runtime_error("search_forest: budgets: one uint32 per tree");
          budgets.assign(arr.data(), arr.data() + arr.size());
        }
        // not in pyoak: n positions searched at once, one GPU lane per tree (include/oakgpu.h: oakgpu_forest_search); output g is
        // search(input g, Heap(), agent, batch = 1, seed = seeds[g]).  The Agent's strings go through search's own parser; what the
        // forest does not run (time budgets, matrix_ucb, UCB1 / Exp3 / PExp3) is refused by name.
        const size_t n = (size_t)results.size();
        if ((size_t)battles.size() != n * OAKGPU_BATTLE_SIZE || (size_t)durations.size() != n * OAKGPU_DURATIONS_SIZE || (size_t)seeds.size() != n)
          throw std::runtime_error("search_forest: battles n x 384, durations n x 8, results n, seeds n");
        const oakgpu_agent a{agent.budget.c_str(), agent.bandit.c_str(), agent.eval.c_str(), agent.matrix_ucb.c_str(), agent.discrete, agent.table};
        std::vector<Output> out(n);
        std::vector<oakgpu_search_output> raw(n);
        int rc = 0;
        std::string err;
        {
          py::gil_scoped_release release;
          std::lock_guard<std::mutex> lock(g_ctx_mu);
          oakgpu_search_params P{};
          oakgpu_net *net = nullptr;
          oakgpu_forest *forest = nullptr;
          rc = oakgpu_agent_params(context(), &a, 1, 0, &P, &net);
          if (!rc) rc = oakgpu_forest_check((uint32_t)n, (uint32_t)std::min<uint64_t>(P.iterations, 0xFFFFFFFFu), P.bandit == 1, &P, net != nullptr, (uint32_t)n, results.data(), 0, 0);
          if (!rc && n) rc = oakgpu_forest_create(context(), (uint32_t)n, (uint32_t)P.iterations, P.bandit == 1, &forest);
          if (!rc && with_budgets) rc = oakgpu_forest_budgets_check(budgets.data(), (uint32_t)n, P.iterations);
          if (!rc && n && with_budgets)
            rc = oakgpu_forest_search_budgets(forest, net, &P, battles.data(), durations.data(), results.data(), seeds.data(), budgets.data(), (uint32_t)n, raw.data(), solve_nash,
                                              nullptr, nullptr, 0);
          else if (!rc && n) rc = oakgpu_forest_search(forest, net, &P, battles.data(), durations.data(), results.data(), seeds.data(), (uint32_t)n, raw.data(), solve_nash, nullptr, nullptr, 0);
          if (rc) err = oakgpu_last_error();
          oakgpu_forest_destroy(context(), forest);
        }
        if (rc) throw std::runtime_error(err);
        for (size_t g = 0; g < n; ++g) out[g].raw = raw[g];
        return out;
      },
      py::arg("battles"), py::arg("durations"), py::arg("results"), py::arg("seeds"), py::arg("agent"), py::arg("solve_nash") = true, py::arg("budgets") = py::none());

  m.def(
      "selfplay_forest",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> teams, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> battle_seeds,
         py::array_t<uint64_t, py::array::c_style | py::array::forcecast> seeds, Agent &agent, const std::string &policy_mode, double policy_temp,
         double policy_min, uint32_t max_battle_length, py::object solve_nash_arg, bool keep_node, uint32_t keep_arena, uint32_t fast_budget,
         double fast_search_prob, const std::string &fast_policy_mode, py::object built_arg, double battle_skip_prob, uint32_t t1_budget, bool matchup) {
        const int solve_nash = nash_mode(solve_nash_arg);
        // not in pyoak: the reference's `generate` loop for n games at once over the forest search (include/oakgpu.h:
        // oakgpu_forest_selfplay); game g is the per-game loop with batch = 1 and seed = seeds[g].  Returns (stream bytes, offsets, n_frames,
        // results, status); with keep_node (generate's --keep-node, on a kept forest of keep_arena nodes a tree, 0 = 4 * budget + 1) a sixth
        // value, nodes_kept per game.  fast_budget / fast_search_prob / fast_policy_mode: generate's fast searches (oakgpu_selfplay_params).
        // built (None, or one byte per game: bit 0 = p1's team was built, bit 1 = p2's) / battle_skip_prob / t1_budget: generate's skipped
        // battles (status 3, no record); matchup = True appends the games' first-search values (float64 per game) to the tuple.
        const size_t n = (size_t)seeds.size();
        py::array_t<uint8_t, py::array::c_style | py::array::forcecast> built;
        const bool has_built = !built_arg.is_none();
        if (has_built) {
          built = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(built_arg);
          if (!built || (size_t)built.size() != n) throw std::runtime_error("selfplay_forest: built: one byte per game");
        }
        py::array_t<double> matchup_out(n);
        if ((size_t)teams.size() != n * 60 || (size_t)battle_seeds.size() != n) throw std::runtime_error("selfplay_forest: teams n x 60, battle_seeds n, seeds n");
        if (policy_mode.size() > 15) throw std::runtime_error("selfplay_forest: policy_mode: at most 15 characters");
        if (fast_policy_mode.size() > 15) throw std::runtime_error("selfplay_forest: fast_policy_mode: at most 15 characters");
        const oakgpu_agent a{agent.budget.c_str(), agent.bandit.c_str(), agent.eval.c_str(), agent.matrix_ucb.c_str(), agent.discrete, agent.table};
        std::string stream;
        py::array_t<uint64_t> offsets(n + 1);
        py::array_t<uint32_t> n_frames(n);
        py::array_t<uint8_t> results(n), status(n);
        py::array_t<uint32_t> nodes_kept(n);
        int rc = 0;
        std::string err;
        {
          py::gil_scoped_release release;
          std::lock_guard<std::mutex> lock(g_ctx_mu);
          oakgpu_selfplay_params P{};
          P.keep_node = keep_node ? 1 : 0;
          oakgpu_net *net = nullptr;
          oakgpu_forest *forest = nullptr;
          rc = oakgpu_agent_params(context(), &a, 1, 0, &P.search, &net);
          std::memcpy(P.policy_mode, policy_mode.c_str(), policy_mode.size() + 1);
          P.policy_temp = policy_temp; P.policy_min = policy_min; P.max_battle_length = max_battle_length;
          std::memcpy(P.fast_policy_mode, fast_policy_mode.c_str(), fast_policy_mode.size() + 1);
          P.fast_budget = fast_budget; P.fast_search_prob = fast_search_prob;
          const oakgpu_selfplay_skip skip{t1_budget, battle_skip_prob};
          const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(P.search.iterations, std::max(fast_budget, t1_budget)), 0xFFFFFFFFu);
          if (!rc && keep_node) rc = oakgpu_forest_create_kept_check((uint32_t)std::max<size_t>(n, 1), cap, keep_arena);
          if (!rc) rc = oakgpu_forest_selfplay_check((uint32_t)n, cap, (P.search.bandit == 1 ? 1 : 0) | (keep_node ? OAKGPU_FOREST_KEPT : 0), &P, net != nullptr, (uint32_t)n,
                                                     teams.data(), solve_nash);
          if (!rc) rc = oakgpu_forest_selfplay_skip_check(cap, &skip);
          if (!rc && n) rc = keep_node ? oakgpu_forest_create_kept(context(), (uint32_t)n, cap, P.search.bandit == 1, keep_arena, &forest)
                                       : oakgpu_forest_create(context(), (uint32_t)n, cap, P.search.bandit == 1, &forest);
          if (!rc && n) rc = oakgpu_forest_selfplay_build(forest, net, &P, &skip, teams.data(), battle_seeds.data(), seeds.data(), has_built ? built.data() : nullptr, (uint32_t)n,
                                                          solve_nash);
          size_t bytes = 0;
          if (!rc && n) rc = oakgpu_forest_selfplay_records(forest, nullptr, 0, &bytes, nullptr, nullptr, nullptr, nullptr, 0);
          if (!rc && n) {
            stream.resize(bytes);
            rc = oakgpu_forest_selfplay_records(forest, (uint8_t *)stream.data(), bytes, &bytes, offsets.mutable_data(), n_frames.mutable_data(),
                                                results.mutable_data(), status.mutable_data(), 0);
          }
          if (!rc && n && keep_node) rc = oakgpu_forest_selfplay_nodes_kept(forest, nodes_kept.mutable_data(), 0);
          if (!rc && n && matchup) rc = oakgpu_forest_selfplay_matchup(forest, matchup_out.mutable_data(), 0);
          if (rc) err = oakgpu_last_error();
          oakgpu_forest_destroy(context(), forest);
        }
        if (rc) throw std::runtime_error(err);
        if (!n) offsets.mutable_data()[0] = 0;
        py::tuple out = keep_node ? py::tuple(py::make_tuple(py::bytes(stream), offsets, n_frames, results, status, nodes_kept))
                                  : py::tuple(py::make_tuple(py::bytes(stream), offsets, n_frames, results, status));
        return matchup ? py::tuple(out + py::make_tuple(matchup_out)) : out;
      },
      py::arg("teams"), py::arg("battle_seeds"), py::arg("seeds"), py::arg("agent"), py::arg("policy_mode") = "e", py::arg("policy_temp") = 1.0,
      py::arg("policy_min") = 0.0, py::arg("max_battle_length") = 0, py::arg("solve_nash") = true, py::arg("keep_node") = false, py::arg("keep_arena") = 0,
      py::arg("fast_budget") = 0, py::arg("fast_search_prob") = 0.0, py::arg("fast_policy_mode") = "", py::arg("built") = py::none(),
      py::arg("battle_skip_prob") = 0.0, py::arg("t1_budget") = 0, py::arg("matchup") = false);

  m.def(
      "match_forest",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> battles, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> durations,
         py::array_t<uint8_t, py::array::c_style | py::array::forcecast> results, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> seeds,
         Agent &agent_p1, Agent &agent_p2, const std::string &policy_p1, const std::string &policy_p2, double temp_p1, double temp_p2, double min_p1,
         double min_p2, uint32_t max_turns, double early_stop, uint32_t log_turns, py::object solve_nash_arg, bool records) {
        const int solve_nash = nash_mode(solve_nash_arg);
        // not in pyoak: the reference's `vs` loop with a budget for n games at once over the forest search (include/oakgpu.h:
        // oakgpu_forest_match); each seat's Agent strings go through search's own parser.  Returns a dict: results, turns, status, log
        // (uint8 [n, log_turns, 24], 0xFF where no game came), counts (wins, ties, losses of seat p1, stopped at max_turns).  records: the
        // dict gains records = (p1, p2), each seat's `.battle.data` of the games as a dict: stream (bytes), offsets, n_frames.
        const size_t n = (size_t)results.size();
        if ((size_t)battles.size() != n * OAKGPU_BATTLE_SIZE || (size_t)durations.size() != n * OAKGPU_DURATIONS_SIZE || (size_t)seeds.size() != n)
          throw std::runtime_error("match_forest: battles n x 384, durations n x 8, results n, seeds n");
        if (policy_p1.size() > 15 || policy_p2.size() > 15) throw std::runtime_error("match_forest: policy mode: at most 15 characters");
        const oakgpu_agent a1{agent_p1.budget.c_str(), agent_p1.bandit.c_str(), agent_p1.eval.c_str(), agent_p1.matrix_ucb.c_str(), agent_p1.discrete, agent_p1.table};
        const oakgpu_agent a2{agent_p2.budget.c_str(), agent_p2.bandit.c_str(), agent_p2.eval.c_str(), agent_p2.matrix_ucb.c_str(), agent_p2.discrete, agent_p2.table};
        py::array_t<uint8_t> res(n), status(n);
        py::array_t<uint32_t> turns(n);
        py::array_t<uint8_t> log(std::vector<py::ssize_t>{(py::ssize_t)n, (py::ssize_t)log_turns, (py::ssize_t)sizeof(oakgpu_match_turn)});
        std::memset(log.mutable_data(), 0xFF, (size_t)log.size());
        uint64_t counts[4] = {0, 0, 0, 0};
        std::string stream[2];
        std::vector<uint64_t> offsets[2] = {std::vector<uint64_t>(n + 1, 0), std::vector<uint64_t>(n + 1, 0)};
        std::vector<uint32_t> n_frames[2] = {std::vector<uint32_t>(n, 0), std::vector<uint32_t>(n, 0)};
        int rc = 0;
        std::string err;
        {
          py::gil_scoped_release release;
          std::lock_guard<std::mutex> lock(g_ctx_mu);
          oakgpu_forest_match_params P{};
          oakgpu_forest *forest = nullptr;
          rc = oakgpu_agent_params(context(), &a1, 1, 0, &P.p1.search, &P.p1.net);
          if (!rc) rc = oakgpu_agent_params(context(), &a2, 1, 0, &P.p2.search, &P.p2.net);
          std::memcpy(P.p1.policy_mode, policy_p1.c_str(), policy_p1.size() + 1);
          std::memcpy(P.p2.policy_mode, policy_p2.c_str(), policy_p2.size() + 1);
          P.p1.policy_temp = temp_p1; P.p2.policy_temp = temp_p2; P.p1.policy_min = min_p1; P.p2.policy_min = min_p2;
          P.max_turns = max_turns; P.early_stop = early_stop; P.log_turns = log_turns; P.solve_nash = solve_nash;
          const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max(P.p1.search.iterations, P.p2.search.iterations), 0xFFFFFFFFu);
          const int contextual = P.p1.search.bandit == 1 || P.p2.search.bandit == 1;
          if (!rc) rc = oakgpu_forest_match_check((uint32_t)n, cap, contextual, &P, (uint32_t)n);
          if (!rc && n) rc = oakgpu_forest_create(context(), (uint32_t)n, cap, contextual, &forest);
          if (!rc && n && records) rc = oakgpu_forest_match_set_records(forest, 1);
          if (!rc && n)
            rc = oakgpu_forest_match(forest, &P, battles.data(), durations.data(), results.data(), seeds.data(), (uint32_t)n, res.mutable_data(), turns.mutable_data(),
                                     status.mutable_data(), log_turns ? (oakgpu_match_turn *)log.mutable_data() : nullptr, counts);
          for (int seat = 0; seat < 2 && !rc && n && records; ++seat) {
            size_t bytes = 0;
            rc = oakgpu_forest_match_records(forest, seat, nullptr, 0, &bytes, nullptr, nullptr, nullptr, nullptr, 0);
            if (rc) break;
            stream[seat].resize(bytes);
            uint8_t none = 0;
            rc = oakgpu_forest_match_records(forest, seat, bytes ? (uint8_t *)stream[seat].data() : &none, bytes, &bytes, offsets[seat].data(), n_frames[seat].data(),
                                             nullptr, nullptr, 0);
          }
          if (rc) err = oakgpu_last_error();
          oakgpu_forest_destroy(context(), forest);
        }
        if (rc) throw std::runtime_error(err);
        py::dict out;
        out["results"] = res; out["turns"] = turns; out["status"] = status; out["log"] = log;
        out["counts"] = py::make_tuple(counts[0], counts[1], counts[2], counts[3]);
        if (records) {
          py::dict seat[2];
          for (int q = 0; q < 2; ++q) {
            seat[q]["stream"] = py::bytes(stream[q]);
            seat[q]["offsets"] = py::array_t<uint64_t>((py::ssize_t)offsets[q].size(), offsets[q].data());
            seat[q]["n_frames"] = py::array_t<uint32_t>((py::ssize_t)n_frames[q].size(), n_frames[q].data());
          }
          out["records"] = py::make_tuple(seat[0], seat[1]);
        }
        return out;
      },
      py::arg("battles"), py::arg("durations"), py::arg("results"), py::arg("seeds"), py::arg("agent_p1"), py::arg("agent_p2"), py::arg("policy_p1") = "e",
      py::arg("policy_p2") = "e", py::arg("temp_p1") = 1.0, py::arg("temp_p2") = 1.0, py::arg("min_p1") = 0.0, py::arg("min_p2") = 0.0,
      py::arg("max_turns") = 1000, py::arg("early_stop") = 0.0, py::arg("log_turns") = 0, py::arg("solve_nash") = true, py::arg("records") = false);

  m.def(
      "value_policy_inference",
      [](const Input &input, const std::string &network_path) {
        // NetworkImpl::value_policy_inference at one position (network.h:102-123), the way Search::run calls it for a fresh
        // root of a contextual bandit (mcts.h:196-209): a zero-iteration "pucb" search leaves value + legal logits in the output
        const oakgpu_agent a{"0", "pucb-1.0", network_path.c_str(), "", 0, 0};
        oakgpu_search_output out{};
        {
          std::lock_guard<std::mutex> lock(g_ctx_mu);
          check(oakgpu_search_agent_heap(context(), nullptr, input.battle, input.durations, input.result, &a, 1, 0, nullptr, &out));
        }
        py::array_t<float> l1(out.m), l2(out.n);
        for (int i = 0; i < out.m; ++i) l1.mutable_unchecked<1>()(i) = (float)out.p1_logit[i];
        for (int j = 0; j < out.n; ++j) l2.mutable_unchecked<1>()(j) = (float)out.p2_logit[j];
        return py::make_tuple((float)out.initial_value, l1, l2);
      },
      py::arg("input"), py::arg("network_path"));
  m.def(
      "value_inference",
      [](const Input &input, const std::string &network_path) { // NetworkImpl::value_inference (network.h:72-79)
        const oakgpu_agent a{"0", "pucb-1.0", network_path.c_str(), "", 0, 0};
        oakgpu_search_output out{};
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        check(oakgpu_search_agent_heap(context(), nullptr, input.battle, input.durations, input.result, &a, 1, 0, nullptr, &out));
        return (float)out.initial_value;
      },
      py::arg("input"), py::arg("network_path"));

  m.def(
      "cpp_inference",
      [](py::bytes record, const std::string &network_path, bool discrete, const std::string &budget) {
        // pyoak.cc:331-392 (the C++ side of the reference's torch == C++ check, src/oak/lab.py:21-79): replay one game record;
        // at every frame run RuntimeSearch::run with agent {eval = network, bandit = "pucb-1.0", budget} on a fresh heap and
        // keep initial_value, the legal logits and their softmax; then play the stored choices.  Like the reference, the
        // first frame starts from the record's battle with zero durations and result None|Move|Move.
        const std::string rec = record;
        uint8_t battle[384], final_result = 0;
        uint32_t count = 0;
        check(oakgpu_frames_read((const uint8_t *)rec.data(), rec.size(), battle, &final_result, nullptr, 0, &count, nullptr));
        std::vector<oakgpu_frame_update> ups(count ? count : 1);
        check(oakgpu_frames_read((const uint8_t *)rec.data(), rec.size(), nullptr, nullptr, ups.data(), count, &count, nullptr));
        py::array_t<float> value(count), logit({(py::ssize_t)count, (py::ssize_t)2, (py::ssize_t)9}), policy({(py::ssize_t)count, (py::ssize_t)2, (py::ssize_t)9});
        auto v = value.mutable_unchecked<1>();
        auto lg = logit.mutable_unchecked<3>();
        auto po = policy.mutable_unchecked<3>();
        uint8_t durations[8] = {}, result = 0x50; // PKMN::result(): None, p1 Move, p2 Move (pkmn.h:228-233)
        const oakgpu_agent a{budget.c_str(), "pucb-1.0", network_path.c_str(), "", discrete ? 1 : 0, 0};
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        for (uint32_t f = 0; f < count; ++f) {
          oakgpu_search_output out{};
          check(oakgpu_search_agent_heap(context(), nullptr, battle, durations, result, &a, 0, std::random_device{}(), nullptr, &out));
          v(f) = (float)out.initial_value;
          for (int q = 0; q < 9; ++q) {
            lg(f, 0, q) = q < out.m ? (float)out.p1_logit[q] : 0.0f;
            lg(f, 1, q) = q < out.n ? (float)out.p2_logit[q] : 0.0f;
            po(f, 0, q) = q < out.m ? (float)out.p1_prior[q] : 0.0f;
            po(f, 1, q) = q < out.n ? (float)out.p2_prior[q] : 0.0f;
          }
          check(oakgpu_update(context(), battle, &ups[f].c1, &ups[f].c2, durations, nullptr, nullptr, 1, &result));
        }
        py::dict d;
        d["value"] = value;
        d["policy_logit"] = logit;
        d["policy"] = policy;
        return d;
      },
      py::arg("record"), py::arg("network_path"), py::arg("discrete") = false, py::arg("budget") = "0");

  m.def(
      "corpus_inference",
      [](py::object paths_or_bytes, const std::string &network_path, bool discrete) {
        // cpp_inference's value / policy_logit / policy for every frame of every record, through the corpus calls of include/oakgpu.h:
        // row bases[r] + f is frame f of record r (picks lists them); status / where as in EncodedBattleFrames
        std::vector<uint8_t> all;
        if (py::isinstance<py::bytes>(paths_or_bytes)) {
          const std::string b = paths_or_bytes.cast<std::string>();
          all.assign(b.begin(), b.end());
        } else {
          for (const std::string &path : paths_or_bytes.cast<std::vector<std::string>>()) {
            const std::vector<char> bytes = read_file(path, "corpus_inference");
            uint32_t n = 0;
            size_t stop = 0; // (bytes behind a record whose length cannot be trusted are left out, so that the next file's records follow)
            check(oakgpu_replay_index((const uint8_t *)bytes.data(), bytes.size(), nullptr, nullptr, nullptr, 0, &n, &stop));
            all.insert(all.end(), bytes.begin(), bytes.begin() + (std::ptrdiff_t)stop);
          }
        }
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        oakgpu_corpus *corpus = nullptr;
        oakgpu_net *net = nullptr;
        check(oakgpu_corpus_create(context(), all.data(), all.size(), &corpus));
        oakgpu_corpus_stats st{};
        int rc = oakgpu_corpus_info(corpus, &st);
        const py::ssize_t rows = rc ? 0 : (py::ssize_t)st.frames;
        py::array_t<float> value({rows, (py::ssize_t)1}), logit({rows, (py::ssize_t)2, (py::ssize_t)9}), policy({rows, (py::ssize_t)2, (py::ssize_t)9});
        py::array_t<uint8_t> k({rows, (py::ssize_t)2}), status(rows);
        py::array_t<uint32_t> where(rows), picks({rows, (py::ssize_t)2});
        if (!rc) rc = discrete ? oakgpu_net_load_discrete(context(), network_path.c_str(), &net) : oakgpu_net_load(context(), network_path.c_str(), &net);
        if (!rc) {
          const oakgpu_corpus_eval out{value.mutable_data(), logit.mutable_data(), policy.mutable_data(), k.mutable_data(), nullptr, status.mutable_data(),
                                       where.mutable_data()};
          rc = oakgpu_corpus_inference(context(), net, corpus, 0, st.records, 0, &out);
        }
        std::vector<uint64_t> bases((size_t)st.records + 1);
        if (!rc) rc = oakgpu_corpus_frame_bases(corpus, bases.data());
        if (net) oakgpu_net_free(context(), net);
        oakgpu_corpus_destroy(corpus);
        check(rc);
        uint32_t *pk = picks.mutable_data();
        for (uint32_t r = 0; r < st.records; ++r)
          for (uint64_t row = bases[r]; row < bases[r + 1]; ++row) { pk[2 * row] = r; pk[2 * row + 1] = (uint32_t)(row - bases[r]); }
        py::dict d;
        d["value"] = value;
        d["policy_logit"] = logit;
        d["policy"] = policy;
        d["k"] = k;
        d["status"] = status;
        d["where"] = where;
        d["picks"] = picks;
        return d;
      },
      py::arg("paths_or_bytes"), py::arg("network_path"), py::arg("discrete") = false);

  m.def(
      "solve_matrix",
      [](py::array_t<float> p1_payoffs, int discretize_factor) { // pyoak.cc:394-426: float payoffs, discretised here
        if (p1_payoffs.ndim() != 2) throw std::runtime_error{"Expecting 2d array"};
        const auto mm = p1_payoffs.shape(0), nn = p1_payoffs.shape(1);
        auto r = p1_payoffs.unchecked<2>();
        std::vector<int32_t> disc((size_t)(mm * nn));
        for (py::ssize_t i = 0; i < mm; ++i)
          for (py::ssize_t j = 0; j < nn; ++j) disc[(size_t)(i * nn + j)] = static_cast<int>(r(i, j) * discretize_factor);
        std::vector<double> a((size_t)std::max<py::ssize_t>(mm, 1)), b((size_t)std::max<py::ssize_t>(nn, 1));
        double value = 0;
        check(oakgpu_solve_matrix(disc.data(), (int)mm, (int)nn, discretize_factor, a.data(), b.data(), &value));
        py::array_t<float> p1(mm), p2(nn);
        for (py::ssize_t i = 0; i < mm; ++i) p1.mutable_unchecked<1>()(i) = (float)a[(size_t)i];
        for (py::ssize_t j = 0; j < nn; ++j) p2.mutable_unchecked<1>()(j) = (float)b[(size_t)j];
        return py::make_tuple(p1, p2, (float)value);
      },
      py::arg("row_payoff"), py::arg("discretize_factor") = 256);

  m.def(
      "solve_matrices",
      [](const std::vector<py::array_t<float>> &matrices, int discretize_factor) {
        // not in pyoak: a batch of solve_matrix calls on the GPU (oakgpu_solve_matrices); entry k is solve_matrix(matrices[k], discretize_factor)
        const size_t count = matrices.size();
        std::vector<int32_t> disc(count * 81 + 1, 0), ms(count + 1, 0), ns(count + 1, 0);
        for (size_t k = 0; k < count; ++k) {
          if (matrices[k].ndim() != 2) throw std::runtime_error{"Expecting 2d array"};
          const auto mm = matrices[k].shape(0), nn = matrices[k].shape(1);
          if (mm < 1 || nn < 1 || mm > 9 || nn > 9) throw std::runtime_error("oakgpu_solve_matrices: matrix " + std::to_string(k) + ": payoff matrix must be between 1x1 and 9x9");
          auto r = matrices[k].unchecked<2>();
          for (py::ssize_t i = 0; i < mm; ++i)
            for (py::ssize_t j = 0; j < nn; ++j) disc[k * 81 + (size_t)(i * nn + j)] = static_cast<int>(r(i, j) * discretize_factor);
          ms[k] = (int32_t)mm; ns[k] = (int32_t)nn;
        }
        std::vector<double> a(count * 9 + 1), b(count * 9 + 1), value(count + 1);
        int rc = 0;
        std::string err;
        {
          py::gil_scoped_release release;
          std::lock_guard<std::mutex> lock(g_ctx_mu);
          rc = oakgpu_solve_matrices(context(), disc.data(), ms.data(), ns.data(), (uint32_t)count, discretize_factor, a.data(), b.data(), value.data());
          if (rc) err = oakgpu_last_error();
        }
        if (rc) throw std::runtime_error(err);
        py::list out;
        for (size_t k = 0; k < count; ++k) {
          py::array_t<float> p1(ms[k]), p2(ns[k]);
          for (int i = 0; i < ms[k]; ++i) p1.mutable_unchecked<1>()(i) = (float)a[k * 9 + (size_t)i];
          for (int j = 0; j < ns[k]; ++j) p2.mutable_unchecked<1>()(j) = (float)b[k * 9 + (size_t)j];
          out.append(py::make_tuple(p1, p2, (float)value[k]));
        }
        return out;
      },
      py::arg("row_payoffs"), py::arg("discretize_factor") = 256);

  m.def(
      "read_battle_data",
      [](const std::string &path) { // pyoak.cc:43-71: [(record bytes, frame count), ...]
        std::ifstream file(path, std::ios::binary);
        if (!file) throw std::runtime_error("read_battle_data: Failed to open file: " + path);
        std::vector<char> data((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
        py::list result;
        size_t pos = 0;
        while (pos < data.size()) {
          uint32_t count = 0;
          size_t used = 0;
          if (oakgpu_frames_read((const uint8_t *)data.data() + pos, data.size() - pos, nullptr, nullptr, nullptr, 0, &count, &used) != 0)
            throw std::runtime_error(std::string("read_battle_data: ") + oakgpu_last_error());
          result.append(py::make_tuple(py::bytes(data.data() + pos, used), (int)count));
          pos += used;
        }
        return result;
      },
      py::arg("path"));

  m.def(
      "policy_games",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> battles, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> durations,
         py::array_t<uint8_t, py::array::c_style | py::array::forcecast> results, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> prng,
         const std::string &p1_network, const std::string &p2_network, bool p1_discrete, bool p2_discrete, double p1_temp, double p1_min, double p2_temp,
         double p2_min, uint32_t max_turns, uint32_t poll, float compact_below, uint32_t log_turns) {
        // n games from the given states, seat p1 against seat p2; an empty network path is a RANDOM seat (include/oakgpu.h)
        const py::ssize_t n = results.size();
        if (battles.size() != n * OAKGPU_BATTLE_SIZE || durations.size() != n * OAKGPU_DURATIONS_SIZE || prng.size() != n * 8)
          throw std::runtime_error("policy_games: expecting battles [n, 384], durations [n, 8], results [n], prng [n, 8]");
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        oakgpu_net *nets[2] = {nullptr, nullptr};
        const std::string *paths[2] = {&p1_network, &p2_network};
        const bool disc[2] = {p1_discrete, p2_discrete};
        int rc = 0;
        for (int s = 0; s < 2 && !rc; ++s) {
          if (paths[s]->empty()) continue;
          if (s == 1 && *paths[0] == *paths[1] && disc[0] == disc[1]) { nets[1] = nets[0]; continue; } // (one handle: one evaluator call per turn)
          rc = disc[s] ? oakgpu_net_load_discrete(context(), paths[s]->c_str(), &nets[s]) : oakgpu_net_load(context(), paths[s]->c_str(), &nets[s]);
        }
        oakgpu_policy_games_params p{};
        p.p1 = oakgpu_seat{nets[0] ? OAKGPU_SEAT_POLICY : OAKGPU_SEAT_RANDOM, nets[0], p1_temp, p1_min};
        p.p2 = oakgpu_seat{nets[1] ? OAKGPU_SEAT_POLICY : OAKGPU_SEAT_RANDOM, nets[1], p2_temp, p2_min};
        p.max_turns = max_turns; p.poll = poll; p.compact_below = compact_below; p.log_turns = log_turns;
        py::array_t<uint8_t> results_out(n), prng_out({n, (py::ssize_t)8}), battles_out({n, (py::ssize_t)OAKGPU_BATTLE_SIZE}),
            durations_out({n, (py::ssize_t)OAKGPU_DURATIONS_SIZE}), log({n, (py::ssize_t)log_turns, (py::ssize_t)2});
        py::array_t<uint32_t> turns(n);
        py::array_t<float> values(n);
        std::memcpy(prng_out.mutable_data(), prng.data(), (size_t)n * 8);
        std::fill_n(log.mutable_data(), log.size(), (uint8_t)0xFF);
        uint64_t counts[4] = {0, 0, 0, 0};
        if (!rc)
          rc = oakgpu_policy_games(context(), &p, battles.data(), durations.data(), results.data(), prng_out.mutable_data(), (uint32_t)n, results_out.mutable_data(),
                                   turns.mutable_data(), values.mutable_data(), battles_out.mutable_data(), durations_out.mutable_data(),
                                   log_turns ? log.mutable_data() : nullptr, counts);
        const std::string err = rc ? oakgpu_last_error() : "";
        if (nets[1] && nets[1] != nets[0]) oakgpu_net_free(context(), nets[1]);
        if (nets[0]) oakgpu_net_free(context(), nets[0]);
        if (rc) throw std::runtime_error(err);
        py::dict d;
        d["results"] = results_out;
        d["turns"] = turns;
        d["values"] = values;
        d["prng"] = prng_out;
        d["battles"] = battles_out;
        d["durations"] = durations_out;
        d["log"] = log;
        d["counts"] = py::make_tuple(counts[0], counts[1], counts[2], counts[3]);
        return d;
      },
      py::arg("battles"), py::arg("durations"), py::arg("results"), py::arg("prng"), py::arg("p1_network") = "", py::arg("p2_network") = "",
      py::arg("p1_discrete") = false, py::arg("p2_discrete") = false, py::arg("p1_temp") = 1.0, py::arg("p1_min") = 0.0, py::arg("p2_temp") = 1.0,
      py::arg("p2_min") = 0.0, py::arg("max_turns") = 1000, py::arg("poll") = 16, py::arg("compact_below") = 0.0f, py::arg("log_turns") = 0);

  py::class_<EncodedBattleFrames>(m, "EncodedBattleFrames")
      .def(py::init<size_t>(), py::arg("size"))
      .def_readonly("size", &EncodedBattleFrames::size)
      .def_readonly("pokemon", &EncodedBattleFrames::pokemon)
      .def_readonly("active", &EncodedBattleFrames::active)
      .def_readonly("hp", &EncodedBattleFrames::hp)
      .def_readonly("choice_indices", &EncodedBattleFrames::choice_indices)
      .def_readonly("k", &EncodedBattleFrames::k)
      .def_readonly("choice", &EncodedBattleFrames::choice)
      .def_readonly("iterations", &EncodedBattleFrames::iterations)
      .def_readonly("empirical_policies", &EncodedBattleFrames::empirical_policies)
      .def_readonly("nash_policies", &EncodedBattleFrames::nash_policies)
      .def_readonly("empirical_value", &EncodedBattleFrames::empirical_value)
      .def_readonly("nash_value", &EncodedBattleFrames::nash_value)
      .def_readonly("score", &EncodedBattleFrames::score)
      .def_readonly("status", &EncodedBattleFrames::status)
      .def_readonly("where", &EncodedBattleFrames::where)
      .def_readonly("picks", &EncodedBattleFrames::picks)
      .def("clear", &EncodedBattleFrames::clear)
      .def_static(
          "from_bytes",
          [](const py::bytes &record, size_t size) { // encoded-frames.h:111-133: every frame of one game record, rows 0 .. frames-1
            const std::string bytes = record;
            auto out = std::make_unique<EncodedBattleFrames>(size);
            std::lock_guard<std::mutex> lock(g_ctx_mu);
            oakgpu_corpus *corpus = nullptr;
            check(oakgpu_corpus_create(context(), (const uint8_t *)bytes.data(), bytes.size(), &corpus));
            oakgpu_corpus_stats st{};
            int rc = oakgpu_corpus_info(corpus, &st);
            if (!rc && (st.records != 1 || st.malformed)) rc = -2;
            if (!rc && st.frames > size) rc = -3;
            if (!rc) {
              uint32_t *picks = out->picks.mutable_data();
              for (uint32_t f = 0; f < st.frames; ++f) picks[2 * f + 1] = f;
              const oakgpu_encoded_frames p = out->pointers();
              rc = oakgpu_frames_encode(context(), corpus, picks, (uint32_t)st.frames, &p, nullptr);
            }
            oakgpu_corpus_destroy(corpus);
            if (rc == -2) throw std::runtime_error("EncodedBattleFrames.from_bytes: expected exactly one well-formed game record");
            if (rc == -3) throw std::runtime_error("EncodedBattleFrames.from_bytes: the record has more frames than `size`");
            check(rc);
            return out;
          },
          py::arg("data"), py::arg("size"));

  py::class_<SampleIndexer>(m, "SampleIndexer")
      .def(py::init<>())
      .def("get", &SampleIndexer::get, py::arg("path"))
      .def("prune", &SampleIndexer::prune, py::arg("paths"))
      .def("size", &SampleIndexer::size);

  m.def(
      "sample",
      [](EncodedBattleFrames &frames, SampleIndexer &indexer, size_t /*threads*/, size_t max_battle_length, size_t min_iterations) -> size_t {
        // pyoak.cc:111-245.  Returns the rows written with status OK (all `size` of them on records that pass the replay check).
        if (frames.size == 0) return 0;
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        oakgpu_corpus *corpus = indexer.device_corpus();
        std::random_device rd;
        const uint64_t seed = ((uint64_t)rd() << 32) | rd();
        const oakgpu_encoded_frames p = frames.pointers();
        uint32_t ok = 0;
        const uint32_t max_len = max_battle_length > 65535 ? 0u : (uint32_t)max_battle_length; // (a record holds at most 65,535 frames: no limit)
        const uint32_t min_it = (uint32_t)std::min<size_t>(min_iterations, 0xFFFFFFFFu);
        check(oakgpu_frames_sample(context(), corpus, (uint32_t)frames.size, seed, max_len, min_it, frames.picks.mutable_data(), &p, &ok));
        return ok;
      },
      py::arg("encoded_frames"), py::arg("indexer"), py::arg("threads"), py::arg("max_battle_length"), py::arg("min_iterations"));

  // Battle net hyper-parameters (pyoak.cc:586-596; nn/default-hyperparameters.h:10-18, encode/battle/*.h dims)
  m.attr("pokemon_in_dim") = 198;
  m.attr("active_in_dim") = 427;
  m.attr("pokemon_hidden_dim") = 128;
  m.attr("pokemon_out_dim") = 59;
  m.attr("active_hidden_dim") = 128;
  m.attr("active_out_dim") = 83;
  m.attr("side_out_dim") = 384;
  m.attr("hidden_dim") = 64;
  m.attr("value_hidden_dim") = 32;
  m.attr("policy_hidden_dim") = 64;
  m.attr("policy_out_dim") = 315;

  // Build net hyper-parameters and index tables (pyoak.cc:598-620; nn/default-hyperparameters.h:22-23, encode/build/tensorizer.h)
  m.attr("build_policy_hidden_dim") = 128;
  m.attr("build_value_hidden_dim") = 128;
  m.attr("build_max_actions") = (int)OAKGPU_BUILD_MAX_ACTIONS;
  {
    std::vector<uint8_t> cells((size_t)OAKGPU_BUILD_N_DIM * 2);
    std::vector<int32_t> table(152 * 166);
    check(oakgpu_build_tables(nullptr, cells.data(), table.data()));
    std::vector<std::pair<int, int>> species_move_list;
    for (int c = 0; c < (int)OAKGPU_BUILD_N_DIM; ++c) species_move_list.emplace_back(cells[2 * c], cells[2 * c + 1]);
    m.attr("species_move_list") = std::move(species_move_list);
    std::vector<std::vector<int>> species_move_table;
    for (int s = 0; s < 152; ++s) species_move_table.emplace_back(table.begin() + s * 166, table.begin() + (s + 1) * 166);
    m.attr("species_move_table") = std::move(species_move_table);
  }

  py::class_<BuildTrajectories>(m, "BuildTrajectories")
      .def(py::init<size_t>())
      .def_readonly("size", &BuildTrajectories::size)
      .def_readwrite("action", &BuildTrajectories::action)
      .def_readwrite("mask", &BuildTrajectories::mask)
      .def_readwrite("policy", &BuildTrajectories::policy)
      .def_readwrite("value", &BuildTrajectories::value)
      .def_readwrite("score", &BuildTrajectories::score)
      .def_readwrite("start", &BuildTrajectories::start)
      .def_readwrite("end", &BuildTrajectories::end)
      .def_readwrite("status", &BuildTrajectories::status)
      .def("clear", &BuildTrajectories::clear);

  m.def(
      "read_build_trajectories",
      [](BuildTrajectories &t, const std::vector<std::string> &paths, size_t /*threads*/, int no_score) -> size_t {
        // pyoak.cc:247-329: `size` draws of a random file and a random record of it, each written by Py::Build::Trajectories::write -- here
        // one decode call on the device over the files' corpus (include/oakgpu.h), the seed from std::random_device as the reference's
        // threads seed theirs.  Returns the count read, or 0 on a refusal (the message goes to stderr, as the reference's does).
        if (t.size == 0 || paths.empty()) return 0;
        const uint64_t seed = ((uint64_t)std::random_device{}() << 32) | std::random_device{}();
        oakgpu_build_trajectories out{};
        out.action = t.action.mutable_data(); out.mask = t.mask.mutable_data(); out.policy = t.policy.mutable_data(); out.value = t.value.mutable_data();
        out.score = t.score.mutable_data(); out.start = t.start.mutable_data(); out.end = t.end.mutable_data(); out.status = t.status.mutable_data();
        const oakgpu_build_traj_params prm{OAKGPU_BUILD_MASK_INT64, no_score};
        try {
          py::gil_scoped_release release;
          std::lock_guard<std::mutex> lock(g_ctx_mu);
          oakgpu_build_corpus *corpus = g_build_corpus.get(paths);
          check(oakgpu_build_traj_sample(context(), corpus, (uint32_t)t.size, seed, &prm, nullptr, &out));
        } catch (const std::exception &e) {
          fprintf(stderr, "%s\n", e.what());
          return 0;
        }
        return t.size;
      },
      py::arg("trajectories"), py::arg("paths"), py::arg("threads") = 1, py::arg("no_score") = 0);

  m.def(
      "build_teams",
      [](py::bytes net_bytes, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> pool, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> seeds,
         int max_pokemon, double pokemon_delete_prob, double move_delete_prob, double team_modify_prob, int input_update) {
        // not in pyoak: TeamBuilding::Provider::get_trajectory for len(seeds) rows at once (include/oakgpu.h: oakgpu_build_provide) over a
        // pool of teams (n x 30 bytes, 6 x {species, 4 moves}) with the `.build.net` in net_bytes.  Returns a dict: teams [n, 30], team_index
        // (-1: built), n_updates, teams_init, sizes, and per step [n, 31] action, index, n_legal, prob.
        const std::string net = net_bytes;
        const size_t n = (size_t)seeds.size();
        if (pool.size() % 30) throw std::runtime_error("build_teams: a pool is whole teams of 30 bytes");
        const size_t steps = n * OAKGPU_BUILD_MAX_STEPS;
        py::array_t<uint8_t> teams_out(std::vector<size_t>{n, 30}), teams_init(std::vector<size_t>{n, 30}), n_updates(n), sizes(n);
        py::array_t<int32_t> team_index(n);
        py::array_t<uint16_t> action(std::vector<size_t>{n, OAKGPU_BUILD_MAX_STEPS}), index(std::vector<size_t>{n, OAKGPU_BUILD_MAX_STEPS}),
            n_legal(std::vector<size_t>{n, OAKGPU_BUILD_MAX_STEPS});
        py::array_t<float> prob(std::vector<size_t>{n, OAKGPU_BUILD_MAX_STEPS});
        std::memset(action.mutable_data(), 0, steps * 2);
        std::memset(index.mutable_data(), 0, steps * 2);
        std::memset(n_legal.mutable_data(), 0, steps * 2);
        std::memset(prob.mutable_data(), 0, steps * 4);
        oakgpu_build_outputs out{};
        out.teams_out = teams_out.mutable_data(); out.n_updates = n_updates.mutable_data(); out.action = action.mutable_data(); out.index = index.mutable_data();
        out.n_legal = n_legal.mutable_data(); out.prob = prob.mutable_data(); out.teams_init = teams_init.mutable_data(); out.sizes_out = sizes.mutable_data();
        out.team_index = team_index.mutable_data();
        const oakgpu_build_provider prm{max_pokemon, input_update, pokemon_delete_prob, move_delete_prob, team_modify_prob};
        int rc = 0;
        std::string err;
        {
          py::gil_scoped_release release;
          std::lock_guard<std::mutex> lock(g_ctx_mu);
          oakgpu_build_net *bn = nullptr;
          rc = oakgpu_build_provide_check(pool.data(), (uint32_t)(pool.size() / 30), (uint32_t)n, max_pokemon, pokemon_delete_prob, move_delete_prob, team_modify_prob);
          if (!rc) rc = oakgpu_build_net_load(context(), (const uint8_t *)net.data(), net.size(), &bn);
          if (!rc) rc = oakgpu_build_provide(context(), bn, pool.data(), (uint32_t)(pool.size() / 30), seeds.data(), (uint32_t)n, &prm, &out);
          if (rc) err = oakgpu_last_error();
          oakgpu_build_net_destroy(bn);
        }
        if (rc) throw std::runtime_error(err);
        py::dict d;
        d["teams"] = teams_out; d["team_index"] = team_index; d["n_updates"] = n_updates; d["teams_init"] = teams_init; d["sizes"] = sizes;
        d["action"] = action; d["index"] = index; d["n_legal"] = n_legal; d["prob"] = prob;
        return d;
      },
      py::arg("net_bytes"), py::arg("pool"), py::arg("seeds"), py::arg("max_pokemon") = 6, py::arg("pokemon_delete_prob") = 0.0, py::arg("move_delete_prob") = 0.0,
      py::arg("team_modify_prob") = 0.0, py::arg("input_update") = 0);
}
