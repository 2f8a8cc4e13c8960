// oak_amd/csrc/selfplay_pick.hpp -- the pick rule of a self-play turn, one text for the host loop (selfplay.hip), the forest search's
// host output path (forest.hip) and the device game loop (forestplay.hip): the game's random stream, MCTS::Search::process_output's
// empirical fields (mcts.h:620-659), RuntimePolicy::get_policy (util/policy.h:22-98), device.sample_pdf (util/random.h:40-49) and the
// bytes of one CompressedFrames Update (compressed-frame.h:77-113).
//
// Everything is double arithmetic in a fixed order; every function switches contraction off, so a * b + c is two roundings on the
// device as on the host (bandit.hpp's rule).  The one operation that is NOT the same number on both sides is pow (policy_temp != 1).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OAK_PICK_HD __host__ __device__
#else
#define OAK_PICK_HD
#endif

namespace oak_pick {

constexpr uint64_t GAME_STREAM_XOR = 0x9FB21C651E98DF25ull; // rng = seed ^ this (the game loop's own stream)
constexpr int MAX_WORDS = 8;                                // words of a policy mode string ("e0.9-x0.1" has two)
constexpr uint32_t MAX_UPDATE_BYTES = 83;                   // update_bytes(9, 9)
enum : int32_t { W_EMPIRICAL = 0, W_NASH = 1, W_ARGMAX = 2, W_PRIOR = 3 };

OAK_PICK_HD inline uint64_t splitmix64(uint64_t &x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
OAK_PICK_HD inline double uniform01(uint64_t &rng) { return (double)(splitmix64(rng) >> 11) * (1.0 / 9007199254740992.0); }

// The start of a turn, for the host loop and the device loop alike (generate.cc:292-299, playout-cap randomisation): with
// fast_search_prob > 0 the game's stream first gives one uniform draw, and the turn is a fast one -- searched with fast_budget
// iterations, picked with fast_policy_mode -- when the draw is below the probability; then, as ever, the next splitmix64 output is the
// seed of the turn's search.  With fast_search_prob == 0 (or below, or NaN) no draw is made: the stream is the one of a game without
// fast searches.  The reference draws from its worker thread's device; a game here owns its stream, so the draw comes from it.
struct TurnPrelude { uint64_t search_seed; bool fast; };
OAK_PICK_HD inline bool turn_is_fast(uint64_t &rng, double fast_search_prob) { return fast_search_prob > 0 && uniform01(rng) < fast_search_prob; }
OAK_PICK_HD inline TurnPrelude turn_prelude(uint64_t &rng, double fast_search_prob) {
  TurnPrelude t;
  t.fast = turn_is_fast(rng, fast_search_prob);
  t.search_seed = splitmix64(rng);
  return t;
}
// the iterations of a turn's search: fast_budget == 0 means the full budget
OAK_PICK_HD inline uint32_t turn_budget(bool fast, uint32_t iterations, uint32_t fast_budget) { return fast && fast_budget ? fast_budget : iterations; }

// Skipped battles (generate's --battle-skip-prob, generate.cc:233-236): a game with at least one built seat (`built` != 0) is skipped with
// probability `prob` -- searched once, on turn 1, for its matchup value, then dropped.  The draw is the first uniform of a stream of its
// own, seeds[g] ^ SKIP_STREAM_XOR (the reference: the worker thread's device), so the game's stream is untouched: a game that is not
// skipped is the game of a call without the fields, whatever `built` says.  No draw is made at probability 0 or for a game without a built
// seat.
constexpr uint64_t SKIP_STREAM_XOR = 0x5B1D7C83A46E20F9ull;
OAK_PICK_HD inline bool game_is_skipped(uint64_t seed, double prob, int built) {
  if (!built || !(prob > 0)) return false;
  uint64_t x = seed ^ SKIP_STREAM_XOR;
  return uniform01(x) < prob;
}

OAK_PICK_HD inline uint16_t compress_prob(double x) { // compress_probs<double, uint16_t> (compressed-frame.h:11-25)
#pragma clang fp contract(off)
  const double v = x * 65535.0;
  return v <= 0 ? 0 : v >= 65535.0 ? 65535 : (uint16_t)v;
}
OAK_PICK_HD inline size_t update_bytes(uint32_t m, uint32_t n) { return 1 + 2 + 4 + 2 * 2 + 2 * (m + n) * 2; } // Update::n_bytes_static (:77-82)

// A policy mode string, parsed once: words 'e' (empirical), 'n' (nash), 'x' (argmax of empirical), 'p' (prior AND empirical, the
// reference's fall-through), each optionally followed by a weight, joined by '-'.
struct PolicyWord { int32_t kind, pad; double weight; };
struct PolicyMode { uint32_t count, pad; PolicyWord word[MAX_WORDS]; };

// 0, or the offending letter ('b' and unknown letters alike), or -1 for more than MAX_WORDS words.  NULL / "" is "e".  `len` bounds a
// field that may lack its terminator.
inline int parse_policy_mode(const char *mode, size_t len, PolicyMode *out) {
  out->count = 0; out->pad = 0;
  char s[64];
  size_t k = 0;
  if (mode) while (k < len && k < sizeof s - 1 && mode[k]) { s[k] = mode[k]; ++k; }
  s[k] = 0;
  if (!k) { s[0] = 'e'; s[1] = 0; k = 1; }
  size_t pos = 0;
  while (pos <= k) {
    size_t end = pos;
    while (end < k && s[end] != '-') ++end;
    if (end > pos) {
      const char c = s[pos];
      const int32_t kind = c == 'e' ? W_EMPIRICAL : c == 'n' ? W_NASH : c == 'x' ? W_ARGMAX : c == 'p' ? W_PRIOR : -1;
      if (kind < 0) return (int)(unsigned char)c;
      if (out->count == MAX_WORDS) return -1;
      char num[64];
      memcpy(num, s + pos + 1, end - pos - 1);
      num[end - pos - 1] = 0;
      out->word[out->count++] = PolicyWord{kind, 0, end - pos > 1 ? atof(num) : 1.0};
    }
    pos = end + 1;
  }
  return 0;
}

// RuntimePolicy::get_policy's arithmetic over parsed words: the weighted sum, then temperature, the minimum-probability cut and
// renormalisation, all over 9 entries.  false: the cut zeroed the whole policy.
OAK_PICK_HD inline bool get_policy(const double *prior, const double *empirical, const double *nash, int k, const PolicyMode &mode, double temp, double minp,
                                   double *policy) {
#pragma clang fp contract(off)
  for (int i = 0; i < 9; ++i) policy[i] = 0;
  for (uint32_t q = 0; q < mode.count; ++q) {
    const double w = mode.word[q].weight;
    switch (mode.word[q].kind) {
      case W_PRIOR: for (int i = 0; i < k; ++i) policy[i] += w * prior[i] + w * empirical[i]; break;
      case W_EMPIRICAL: for (int i = 0; i < k; ++i) policy[i] += w * empirical[i]; break;
      case W_NASH: for (int i = 0; i < k; ++i) policy[i] += w * nash[i]; break;
      default: { // std::max_element: the first of the largest
        int best = 0;
        for (int i = 1; i < k; ++i) if (empirical[best] < empirical[i]) best = i;
        policy[best] += w;
      }
    }
  }
  if (temp != 1) {
    double sum = 0;
    for (int i = 0; i < 9; ++i) { policy[i] = std::pow(policy[i], temp); sum += policy[i]; }
    for (int i = 0; i < 9; ++i) policy[i] /= sum;
  }
  double sum = 0;
  for (int i = 0; i < 9; ++i) { if (policy[i] < minp) policy[i] = 0; sum += policy[i]; }
  if (!(sum > 0)) return false;
  for (int i = 0; i < 9; ++i) policy[i] /= sum;
  return true;
}

OAK_PICK_HD inline int sample_pdf(const double *p, int k, uint64_t &rng) { // device.sample_pdf (util/random.h:40-49)
#pragma clang fp contract(off)
  double u = uniform01(rng);
  for (int i = 0; i < k; ++i) { u -= p[i]; if (u <= 0) return i; }
  return 0;
}

// MCTS::Search::process_output (mcts.h:620-659) over root matrices of row stride 9: the empirical value and strategies, and (M nullable)
// the integer payoffs of the exact Nash solve, M[i * n + j].  p1_empirical / p2_empirical: 9 entries each, zeroed here.
OAK_PICK_HD inline void process_output(const uint64_t *visit_matrix, const double *value_matrix, int m, int n, uint64_t iterations, double *empirical_value,
                                       double *p1_empirical, double *p2_empirical, int32_t *M) {
#pragma clang fp contract(off)
  for (int q = 0; q < 9; ++q) p1_empirical[q] = p2_empirical[q] = 0;
  double tv = 0;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      tv += value_matrix[i * 9 + j];
      uint64_t v = visit_matrix[i * 9 + j];
      p1_empirical[i] += (double)v;
      p2_empirical[j] += (double)v;
      v += !v;
      if (M) M[i * n + j] = (int32_t)(value_matrix[i * 9 + j] / (double)v * 256.0);
    }
  *empirical_value = tv / (double)iterations;
  for (int i = 0; i < m; ++i) p1_empirical[i] /= (double)(float)iterations;
  for (int j = 0; j < n; ++j) p2_empirical[j] /= (double)(float)iterations;
}

// Update::write (compressed-frame.h:89-113) into `p` (update_bytes(m, n) bytes, any alignment); returns the length.
OAK_PICK_HD inline uint32_t encode_update(uint8_t *p, uint32_t m, uint32_t n, uint8_t c1, uint8_t c2, uint32_t iterations, double empirical_value, double nash_value,
                                          const double *p1_empirical, const double *p1_nash, const double *p2_empirical, const double *p2_nash) {
  uint8_t *q = p;
  auto put16 = [&](uint16_t v) { *q++ = (uint8_t)v; *q++ = (uint8_t)(v >> 8); };
  *q++ = (uint8_t)((m - 1) | ((n - 1) << 4));
  *q++ = c1;
  *q++ = c2;
  for (int b = 0; b < 4; ++b) *q++ = (uint8_t)(iterations >> (8 * b));
  put16(compress_prob(empirical_value));
  put16(compress_prob(nash_value));
  for (uint32_t k = 0; k < m; ++k) put16(compress_prob(p1_empirical[k]));
  for (uint32_t k = 0; k < m; ++k) put16(compress_prob(p1_nash[k]));
  for (uint32_t k = 0; k < n; ++k) put16(compress_prob(p2_empirical[k]));
  for (uint32_t k = 0; k < n; ++k) put16(compress_prob(p2_nash[k]));
  return (uint32_t)(q - p);
}

} // namespace oak_pick
