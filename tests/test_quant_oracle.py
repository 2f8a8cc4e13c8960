"""CPU: tests/quant_oracle.py against tests/golden/quant_goldens.npz -- the reference's quantized layers (nn/battle/quantized/
{affine,clipped_relu,simd}.h) compiled with g++ -O3 -mavx2 on fixed weights and inputs (tests/golden/make_quant_goldens.py).
Every int32 and byte must be reproduced."""
import os
import struct

import numpy as np
import pytest

import quant_oracle as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "quant_goldens.npz"))
F = np.float32


def test_quantized_weights_and_biases():
    assert (Q.quantize_weights(G["w"]) == G["wq"]).all()
    assert (Q.quantize_biases(G["b"]) == G["bq"]).all()
    assert (Q.quantize_weights(G["w3"]) == G["wq3"]).all() and (Q.quantize_biases(G["b3"]) == G["bq3"]).all()
    assert (Q.quantize_weights(G["wr"]) == G["wqr"]).all() and (Q.quantize_biases(G["br"]) == G["bqr"]).all()
    assert G["wq"].min() == -127 and G["wq"].max() == 127      # +-(2 - 2^-23) -> +-127


def test_fc_outputs_saturating_pairs_and_crelu():
    stats = {}
    y = Q.affine(G["wq"], G["bq"], G["x"], stats)
    assert (y == G["fc_out"]).all()
    assert stats["saturated"] > 0                                # the goldens exercise _mm256_maddubs_epi16's saturation
    # ... and the unsaturated dot product would be wrong on them
    assert (G["x"].astype(np.int64) @ G["wq"].T.astype(np.int64) + G["bq"] != G["fc_out"]).any()
    h = Q.crelu(y)
    assert (h == G["crelu_out"]).all()
    assert (Q.affine(G["wq3"], G["bq3"], h)[:, 0] == G["fc3_out"]).all()
    single = h.astype(np.int64) @ G["wqr"].T.astype(np.int64) + G["bqr"]      # propagate_single: no pairs, plain int32
    assert (single == G["single_out"]).all() and (Q.affine(G["wqr"], G["bqr"], h) == G["single_out"]).all()


def test_byte_cast_sweep():
    got = Q.cast_u8(G["cast_in"])
    assert (got == G["cast_out"]).all(), np.flatnonzero(got != G["cast_out"])[:8]
    v = F(127) * G["cast_in"]
    assert ((v >= 256) & (G["cast_out"] != 255)).any()           # the sweep covers the wrap


def test_refusals():
    with pytest.raises(Q.NotClamped, match="^5non clamped2.000000$"):
        Q.quantize_weights(np.array([[0, 0, 0, 0, 0, 2.0]], F))
    with pytest.raises(Q.NotClamped, match="^0non clamped-?nan$"):
        Q.quantize_weights(np.array([np.nan], F))
    with pytest.raises(ValueError):
        Q.quantize_biases(np.array([265000.0], F))
    assert Q.quantize_weights(np.array([np.nextafter(F(2), F(0)), -np.nextafter(F(2), F(0))], F)).tolist() == [127, -127]


def test_quant_net_refuses_a_relu_header(tmp_path):
    src = open(os.path.join(ROOT, "tests", "golden", "net_default.battle.net"), "rb").read()
    assert src[0] == 0
    with pytest.raises(ValueError, match="does not encode clamped activations"):
        Q.QuantNet(os.path.join(ROOT, "tests", "golden", "net_default.battle.net"))
    p = tmp_path / "clamp.net"
    p.write_bytes(bytes([1]) + src[1:])
    qn = Q.QuantNet(str(p))
    assert (qn.H, qn.VH, qn.PH) == (64, 32, 64) and qn.relu.activation == 1 and qn.clamp.activation == 2
    assert struct.unpack_from("<II", src, 8) == (198, 128)
