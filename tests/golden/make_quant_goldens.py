"""Generator of tests/golden/quant_goldens.npz: the reference's quantized layers (cpp/include/nn/battle/quantized/{common,simd,
affine,clipped_relu}.h) run on fixed weights and inputs, compiled the way the reference's g++ builds compile them
(g++ -O3 -mavx2).  Run by hand where the reference tree exists:

    python tests/golden/make_quant_goldens.py /path/to/reference

It writes a small harness of its own into a temporary directory (nothing of the reference is copied or kept), feeds it the
inputs below and stores inputs and outputs -- data only -- in the .npz.  tests/test_quant_oracle.py holds tests/quant_oracle.py
to every int32 in it.  The cases:
  * weights at +-(2 - 2^-23) (the largest floats inside the bound), on k / 64 and just beside it, tiny ones of either sign;
  * biases whose (b * 64) * 127 rounds onto / beside an integer in fp32, and biases near the int32 limit;
  * input bytes 0..255 with rows of 128-255 bytes, so that _mm256_maddubs_epi16 pairs saturate in both directions;
  * ClippedReLU of those outputs, a one-output layer (value_fc3's form) and propagate_single (the policy rows);
  * static_cast<uint8_t>(127 f) over a sweep of floats: truncation, the wrap of 127 f >= 256, values beyond int32.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

F = np.float32
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "quant_goldens.npz")

HARNESS = r'''
#include <nn/battle/quantized/affine.h>
#include <nn/battle/quantized/clipped_relu.h>
#include <algorithm>
#include <cstdio>
#include <vector>
using namespace NN::Battle::Quantized;
struct Layer { uint32_t in_dim, out_dim; std::vector<float> weights, biases; };
static Layer read_layer(FILE *f, uint32_t in, uint32_t out) {
  Layer l{in, out, std::vector<float>(in * out), std::vector<float>(out)};
  if (fread(l.weights.data(), 4, in * out, f) != in * out || fread(l.biases.data(), 4, out, f) != out) std::exit(2);
  return l;
}
static AffineTransform<64, 32> fc;
static AffineTransform<32, 1> fc3;
static AffineTransform<32, 64> rows;
static ClippedReLU<32> ac;
int main(int argc, char **argv) {
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  uint32_t n_x, n_cast;
  if (fread(&n_x, 4, 1, in) != 1 || fread(&n_cast, 4, 1, in) != 1) return 2;
  Layer a = read_layer(in, 64, 32), c = read_layer(in, 32, 1), r = read_layer(in, 32, 64);
  fc.try_copy_parameters(a);
  fc3.try_copy_parameters(c);
  rows.try_copy_parameters(r);
  for (int i = 0; i < 64 * 32; ++i) { const int8_t w = fc.weights[fc.get_weight_index(i)]; fwrite(&w, 1, 1, out); }
  fwrite(fc.biases, 4, 32, out);
  for (int i = 0; i < 32; ++i) { const int8_t w = fc3.weights[fc3.get_weight_index(i)]; fwrite(&w, 1, 1, out); }
  fwrite(fc3.biases, 4, 1, out);
  for (int i = 0; i < 32 * 64; ++i) { const int8_t w = rows.weights[rows.get_weight_index(i)]; fwrite(&w, 1, 1, out); }
  fwrite(rows.biases, 4, 64, out);
  alignas(64) uint8_t x[64];
  alignas(64) int32_t y[32];
  alignas(64) uint8_t h[32];
  alignas(64) int32_t v[32];
  for (uint32_t k = 0; k < n_x; ++k) {
    if (fread(x, 1, 64, in) != 64) return 2;
    fc.propagate(x, y);
    ac.propagate(y, h);
    fc3.propagate(h, v);
    fwrite(y, 4, 32, out);
    fwrite(h, 1, 32, out);
    fwrite(v, 4, 1, out);
    for (int o = 0; o < 64; ++o) { const int32_t s = rows.propagate_single(h, o); fwrite(&s, 4, 1, out); }
  }
  std::vector<float> f(n_cast);
  std::vector<uint8_t> b(n_cast);
  if (fread(f.data(), 4, n_cast, in) != n_cast) return 2;
  std::transform(f.begin(), f.end(), b.begin(), [](const auto v) { return static_cast<uint8_t>(127 * v); }); // cache.h:98-99, 204-205
  fwrite(b.data(), 1, n_cast, out);
  fclose(out);
  return 0;
}
'''


def inputs():
    rng = np.random.default_rng(20261016)
    top = np.nextafter(F(2), F(0))
    W = (rng.random((32, 64)) * 4 - 2).astype(F) * F(0.999)
    W[0, :8] = [top, -top, F(1.984375), -F(1.984375), np.nextafter(F(1.984375), F(0)), -np.nextafter(F(1.984375), F(0)), F(0.015625), -F(0.015625)]
    W[1, :8] = [F(0.0156), -F(0.0156), F(1e-30), -F(1e-30), F(0), -F(0.0), F(0.5), F(-1.5)]
    W[2:6] = np.sign(W[2:6]) * top                             # rows of extreme weights: the saturating pairs
    W[6:8, :] = np.round(W[6:8, :] * 64) / 64                  # exactly on the grid
    b = (rng.random(32) * 2 - 1).astype(F)
    edges = [(k + 0.5) / 8128.0 for k in (0, 1, 7, 1000)] + [k / 8128.0 for k in (1, 3, -5)] + [264000.0, -264000.0, 1e-9, -1e-9]
    b[:len(edges)] = np.array(edges, dtype=np.float64).astype(F)
    b[len(edges):len(edges) + 4] = np.nextafter(b[:4], F(1))
    c_w = (rng.random((1, 32)) * 4 - 2).astype(F) * F(0.999)
    c_b = np.array([0.37], F)
    r_w = (rng.random((64, 32)) * 4 - 2).astype(F) * F(0.999)
    r_b = (rng.random(64) * 0.4 - 0.2).astype(F)
    X = rng.integers(0, 256, (96, 64)).astype(np.uint8)
    X[:16] = rng.integers(128, 256, (16, 64))
    X[16:24] = 255
    X[24:32] = rng.integers(0, 128, (8, 64))
    X[32] = 0
    k = np.arange(0, 400, dtype=np.float64)
    cast = np.concatenate([
        np.linspace(0, 3, 4001).astype(F),
        (k / 127).astype(F), np.nextafter((k / 127).astype(F), F(0)), np.nextafter((k / 127).astype(F), F(10)),
        np.array([266.7 / 127, 1.0, 2.0, 2.0159, 1e6, 1.6e7, 1.69e7, 1.7e7, 3e7, 1e9, 1e30, -0.0, -1e-8], F),
    ]).astype(F)
    return W, b, c_w, c_b, r_w, r_b, X, cast


def main(ref):
    W, b, c_w, c_b, r_w, r_b, X, cast = inputs()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        open(src, "w").write(HARNESS)
        subprocess.check_call(["g++", "-std=c++20", "-O3", "-mavx2", "-I", os.path.join(ref, "cpp", "include"), src, "-o", exe])
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([X.shape[0], cast.size], "<u4").tobytes())
            for w_, b_ in ((W, b), (c_w, c_b), (r_w, r_b)):
                f.write(w_.astype("<f4").tobytes() + b_.astype("<f4").tobytes())
            f.write(X.tobytes())
            f.write(cast.astype("<f4").tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    off = 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(raw, dtype, count, off)
        off += a.nbytes
        return a.copy()
    wq, bq = take("i1", 64 * 32).reshape(32, 64), take("<i4", 32)
    wq3, bq3 = take("i1", 32).reshape(1, 32), take("<i4", 1)
    wqr, bqr = take("i1", 32 * 64).reshape(64, 32), take("<i4", 64)
    fc_out, crelu_out, fc3_out, single_out = [], [], [], []
    for _ in range(X.shape[0]):
        fc_out.append(take("<i4", 32))
        crelu_out.append(take("u1", 32))
        fc3_out.append(take("<i4", 1))
        single_out.append(take("<i4", 64))
    cast_out = take("u1", cast.size)
    assert off == len(raw)
    np.savez_compressed(OUT, w=W, b=b, wq=wq, bq=bq, w3=c_w, b3=c_b, wq3=wq3, bq3=bq3, wr=r_w, br=r_b, wqr=wqr, bqr=bqr, x=X,
                        fc_out=np.array(fc_out), crelu_out=np.array(crelu_out), fc3_out=np.array(fc3_out)[:, 0],
                        single_out=np.array(single_out), cast_in=cast, cast_out=cast_out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OAK_REFERENCE", "../oak"))
