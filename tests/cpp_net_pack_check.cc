// tests/cpp_net_pack_check.cc -- oak_amd/csrc/net_pack.hpp stand-alone: no HIP, no Python, its own main.
//
//   cpp_net_pack_check GOLDEN_DIR              packs a list of networks and prints a JSON array, one document per network and line:
//                                              dims, T0 / NB / PB / PH, the four flags, scalars, and for every image in upload order its
//                                              name, byte count and 64-bit FNV-1a digest -- or the refusal text.  tests/test_net_pack.py
//                                              holds this output to tests/golden/net_pack_digests.json, also under sanitizers.
//   cpp_net_pack_check GOLDEN_DIR --dump DIR   also writes every network's file bytes to DIR/NN_name[.discrete].net
//   cpp_net_pack_check --time FILE             packs FILE twice and prints the second call's milliseconds
//
// The networks: the three golden files; net_default re-headed for the int8 path; synthetic ones at the smallest shapes where each
// layout can still go wrong (block counts 3 -> 4 and 5 -> 8, PB 2 and 4, q*b_img present and absent); one edit each for the four
// flags; one file for every refusal text of the packer, and two files with two faults each that pin the order of the checks.
// Synthetic weights are k / 2^m from a fixed integer recurrence, |w| <= 1 / sqrt(in) like the reference's initialiser.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../oak_amd/csrc/net_pack.hpp"

namespace {
using oak::pack::PackedNet;

struct Layer { uint32_t in, out; std::vector<float> b, w; };
enum { P0, P1, A0, A1, FC0, FC1, V2, V3, Q1A, Q1B, Q2A, Q2B };
struct NetFile {
  uint8_t header[8] = {0};
  Layer L[12];
  std::vector<uint8_t> bytes() const {
    std::vector<uint8_t> out(header, header + 8);
    for (const Layer &l : L) {
      const uint32_t dims[2] = {l.in, l.out};
      out.insert(out.end(), (const uint8_t *)dims, (const uint8_t *)dims + 8);
      oak::pack::append(out, l.b);
      oak::pack::append(out, l.w);
    }
    return out;
  }
};
struct Shape { uint32_t hidden, value_hidden, policy_hidden, p_out = 27, a_out = 19, p_hidden = 128, a_hidden = 128; int activation = 2; };

NetFile synth(const Shape &s) {
  NetFile f;
  f.header[0] = (uint8_t)(s.activation - 1);
  const uint32_t emb = 2 * ((1 + s.a_out) + 5 * (1 + s.p_out));
  const uint32_t dims[12][2] = {{198, s.p_hidden}, {s.p_hidden, s.p_out}, {427, s.a_hidden}, {s.a_hidden, s.a_out}, {emb, s.hidden}, {s.hidden, s.hidden},
                                {s.hidden, s.value_hidden}, {s.value_hidden, 1}, {s.hidden, s.policy_hidden}, {s.policy_hidden, 315}, {s.hidden, s.policy_hidden}, {s.policy_hidden, 315}};
  uint64_t state = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 12; ++i) {
    Layer &l = f.L[i];
    l.in = dims[i][0]; l.out = dims[i][1];
    int m = 15; // |k| <= 2^15, so |k / 2^m| <= 2^-(m - 15) <= 1 / sqrt(in)
    while ((1u << (2 * (m - 15))) < l.in) ++m;
    auto next = [&]() {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      return std::ldexp((float)((int)((state >> 40) & 0xFFFF) - 32768), -m);
    };
    l.b.resize(l.out);
    l.w.resize((size_t)l.out * l.in);
    for (float &v : l.b) v = next();
    for (float &v : l.w) v = next();
  }
  return f;
}
void set_dims(Layer &l, uint32_t in, uint32_t out) { // keeps the file well-formed: the parameters follow the dims
  l.in = in; l.out = out;
  l.b.assign(out, 0.0078125f);
  l.w.assign((size_t)out * in, -0.00390625f);
}

struct Case { std::string name; std::vector<uint8_t> bytes; bool discrete; };

std::vector<uint8_t> read_file(const std::string &path) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
  std::vector<uint8_t> buf;
  uint8_t tmp[1 << 16];
  size_t r;
  while ((r = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + r);
  fclose(f);
  return buf;
}

std::vector<Case> cases(const std::string &golden) {
  std::vector<Case> c;
  auto add = [&](const char *name, const NetFile &f, bool discrete = false) { c.push_back({name, f.bytes(), discrete}); };
  for (const char *g : {"net_tiny", "net_default", "net_256"}) c.push_back({g, read_file(golden + "/" + g + ".battle.net"), false});
  {
    std::vector<uint8_t> b = read_file(golden + "/net_default.battle.net");
    b[0] = 1;
    c.push_back({"net_default_discrete", b, true});
  }
  const Shape s1{96, 160, 40}, s2{96, 160, 72};
  Shape sq{32, 32, 32};
  sq.p_out = 59; sq.a_out = 83; // the 768-wide embedding
  add("synth_96_160_40", synth(s1));
  add("synth_96_160_72", synth(s2));
  add("synth_discrete_32", synth(sq), true);
  // the flags: the second synthetic net with one edit
  { NetFile f = synth(s2); f.L[FC1].w[5] = 0x1p21f; add("flag_main_weight_2p21", f); }
  { NetFile f = synth(s2); f.L[Q1B].w[7] = 0x1p21f; add("flag_policy_fc3_weight_2p21", f); }
  { NetFile f = synth(s2); Layer &l = f.L[FC0]; for (uint32_t n = 0; n < l.out; ++n) l.w[(size_t)n * l.in + 3] *= 0x1p-20f; add("flag_fc0_column_2m20", f); }
  { NetFile f = synth(s2); Layer &l = f.L[P1]; for (uint32_t k = 0; k < l.in; ++k) l.w[(size_t)2 * l.in + k] *= 0x1p-30f; add("flag_embed_row_2m30", f); }
  // the refusals, on the smallest shape (one block everywhere)
  const Shape sb{32, 32, 32};
  { Case k{"refuse_short_header", synth(sb).bytes(), false}; k.bytes.resize(7); c.push_back(k); }
  { NetFile f = synth(sb); f.header[0] = 2; add("refuse_activation_byte", f); }
  { Shape s = sq; s.activation = 1; add("refuse_discrete_relu", synth(s), true); }
  { Case k{"refuse_truncated_layer", synth(sb).bytes(), false}; k.bytes.resize(k.bytes.size() - 4); c.push_back(k); }
  { Case k{"refuse_trailing_byte", synth(sb).bytes(), false}; k.bytes.push_back(0); c.push_back(k); }
  { NetFile f = synth(sb); f.L[A0].w[0] = std::numeric_limits<float>::quiet_NaN(); add("refuse_nan_active_fc0", f); }
  { NetFile f = synth(sb); f.L[V2].b[1] = std::numeric_limits<float>::infinity(); add("refuse_inf_value_fc2", f); }
  { NetFile f = synth(sb); set_dims(f.L[P0], 199, 128); add("refuse_embedding_input_dims", f); }
  { NetFile f = synth(sb); set_dims(f.L[V3], 33, 1); add("refuse_inconsistent_dims", f); }
  { NetFile f = synth(sb); set_dims(f.L[P0], 198, 129); set_dims(f.L[P1], 129, 27); add("refuse_embedding_width_129", f); }
  { NetFile f = synth(sb); set_dims(f.L[FC0], f.L[FC0].in + 4, 32); add("refuse_fc0_input", f); }
  { NetFile f = synth(sb); set_dims(f.L[FC1], 32, 33); set_dims(f.L[V2], 33, 32); add("refuse_fc0_fc1_widths", f); }
  add("refuse_width_288", synth(Shape{288, 32, 32}));
  { Shape s = sb; s.p_out = 26; add("refuse_multiple_of_4", synth(s)); } // side 155: fc0 input 310
  { NetFile f = synth(sb); set_dims(f.L[Q2B], 32, 314); add("refuse_policy_heads", f); }
  add("refuse_policy_width_288", synth(Shape{32, 32, 288}));
  add("refuse_quant_side_dim", synth(sb), true);
  { Shape s = sq; s.hidden = 96; add("refuse_quant_hidden", synth(s), true); }
  { Shape s = sq; s.hidden = 64; s.value_hidden = 48; add("refuse_quant_value_hidden", synth(s), true); }
  { Shape s = sq; s.policy_hidden = 40; add("refuse_quant_policy_hidden", synth(s), true); }
  { Shape s = sq; s.value_hidden = 64; add("refuse_quant_value_above_hidden", synth(s), true); }
  { Shape s = sq; s.policy_hidden = 64; add("refuse_quant_policy_above_hidden", synth(s), true); }
  { NetFile f = synth(sq); set_dims(f.L[FC1], 64, 32); add("refuse_quant_bad_in_dim", f, true); }
  { NetFile f = synth(sq); set_dims(f.L[Q1B], 32, 300); add("refuse_quant_bad_out_dim", f, true); }
  { NetFile f = synth(sq); f.L[FC1].w[3] = 2.0f; add("refuse_quant_weight_2", f, true); }
  { NetFile f = synth(sq); f.L[FC0].b[1] = 1e6f; add("refuse_quant_bias_int32", f, true); }
  // two faults each: the first check in the loader's order wins
  { NetFile f = synth(Shape{288, 32, 32}); f.L[FC1].w[0] = std::numeric_limits<float>::quiet_NaN(); add("order_nan_then_width_288", f); }
  { Shape s = sb; s.p_out = 26; NetFile f = synth(s); set_dims(f.L[Q2B], 32, 314); add("order_multiple_of_4_then_policy_heads", f); }
  return c;
}

uint64_t fnv1a(const void *data, size_t bytes) {
  uint64_t h = 14695981039346656037ull;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const uint8_t *)data)[i]) * 1099511628211ull;
  return h;
}
std::string json_text(const std::string &s) {
  std::string o = "\"";
  for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; }
  return o + "\"";
}
void print_case(const Case &k) {
  PackedNet n;
  const std::string refusal = oak::pack::pack_net(k.bytes.data(), k.bytes.size(), k.discrete, n);
  printf("{\"net\": %s, \"discrete\": %s, \"file_bytes\": %zu, ", json_text(k.name).c_str(), k.discrete ? "true" : "false", k.bytes.size());
  if (!refusal.empty()) { printf("\"refused\": %s}", json_text(refusal).c_str()); return; }
  uint32_t b3;
  memcpy(&b3, &n.b3, 4);
  printf("\"activation\": %d, \"dims\": {\"in_dim\": %d, \"hidden\": %d, \"value_hidden\": %d, \"policy_hidden\": %d, \"p_hidden\": %d, \"p_out\": %d, "
         "\"a_hidden\": %d, \"a_out\": %d, \"side_dim\": %d, \"H\": %d, \"VH\": %d}, \"T0\": %d, \"NB\": %d, \"PB\": %d, \"PH\": %d, \"b3_bits\": %" PRIu32 ", ",
         n.activation, n.in_dim, n.hidden, n.value_hidden, n.policy_hidden, n.p_hidden, n.p_out, n.a_hidden, n.a_out, n.side_dim, n.H, n.VH, n.T0, n.NB, n.PB, n.PH, b3);
  printf("\"split_safe\": %s, \"embed_safe\": %s, \"pair_safe\": %s, \"policy_safe\": %s, ", n.split_safe ? "true" : "false", n.embed_safe ? "true" : "false",
         n.pair_safe ? "true" : "false", n.policy_safe ? "true" : "false");
  if (n.discrete) printf("\"q\": {\"H\": %d, \"VH\": %d, \"PH\": %d, \"img_bytes\": %d, \"b3\": %d}, ", n.q_H, n.q_VH, n.q_PH, n.q_img_bytes, (int)n.q_b3);
  printf("\"images\": [");
  for (size_t i = 0; i < n.images.size(); ++i)
    printf("%s{\"name\": \"%s\", \"bytes\": %zu, \"fnv1a\": \"%016" PRIx64 "\"}", i ? ", " : "", n.images[i].name, n.images[i].bytes(), fnv1a(n.images[i].data(), n.images[i].bytes()));
  printf("]}");
}
} // namespace

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "--time")) {
    const std::vector<uint8_t> b = read_file(argv[2]);
    double ms = 0;
    for (int i = 0; i < 2; ++i) {
      PackedNet n;
      const auto t0 = std::chrono::steady_clock::now();
      const std::string refusal = oak::pack::pack_net(b.data(), b.size(), false, n);
      ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (!refusal.empty() || n.images.empty()) { fprintf(stderr, "refused: %s\n", refusal.c_str()); return 1; }
    }
    printf("%.3f\n", ms);
    return 0;
  }
  if (argc != 2 && !(argc == 4 && !strcmp(argv[2], "--dump"))) { fprintf(stderr, "usage: %s GOLDEN_DIR [--dump DIR] | --time FILE\n", argv[0]); return 2; }
  const std::vector<Case> all = cases(argv[1]);
  printf("[\n");
  for (size_t i = 0; i < all.size(); ++i) {
    print_case(all[i]);
    printf(i + 1 < all.size() ? ",\n" : "\n");
    if (argc == 4) {
      char path[4096];
      snprintf(path, sizeof path, "%s/%02zu_%s%s.net", argv[3], i, all[i].name.c_str(), all[i].discrete ? ".discrete" : "");
      FILE *f = fopen(path, "wb");
      if (!f || fwrite(all[i].bytes.data(), 1, all[i].bytes.size(), f) != all[i].bytes.size()) { fprintf(stderr, "cannot write %s\n", path); return 2; }
      fclose(f);
    }
  }
  printf("]\n");
  return 0;
}
