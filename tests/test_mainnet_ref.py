"""CPU: the yardstick of tests/test_gpu_mainnet.py, tested on its own -- the batched float64 value path against
test_gpu_leafnet._main_value_f64, the premises of the net table (block counts, padded widths, ring parity, the span of the
pre-sigmoid sums), the fp32 oracle's own distance from float64 (E_ref, what the bound is made of), and the proof that the bound sees
a layer whose operands lost their low part.  The embeddings are nn_oracle.battle_embedding's of 128 leaves of policy_ref.batch_of."""
import json
import os

import numpy as np
import pytest

import mainnet_ref as M
import policy_ref as P
from policy_ref import NN

N_LEAVES = 128
FACTORS = {}
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _discrimination_records():
    """OAK_MAINNET_DISCRIMINATION_JSON=<file>: write the measured factors (the "discrimination" part of profiles/r11_mainnet_accuracy.json)."""
    yield
    out = os.environ.get("OAK_MAINNET_DISCRIMINATION_JSON")
    if out and FACTORS:
        with open(out, "w") as f:
            json.dump(FACTORS, f, indent=1, sort_keys=True)


def _case(name, tmp_path_factory):
    """(oracle net, fp32 embeddings of N_LEAVES leaves) of a net of the table, computed once per process."""
    if name not in _CASES:
        onet = NN.Net(M.write_net(name, tmp_path_factory.mktemp(name)))
        b, d, _ = P.batch_of(N_LEAVES, seed=M.SEED)
        _CASES[name] = (onet, M.oracle_embeddings(onet, b, d))
    return _CASES[name]


def test_value_f64_equals_the_row_by_row_evaluation(tmp_path_factory):
    from test_gpu_leafnet import _main_value_f64
    onet, emb = _case("256", tmp_path_factory)
    got, y = M.value_f64(onet, emb)
    want = np.array([_main_value_f64(onet, emb[i]) for i in range(emb.shape[0])])
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-15
    assert np.abs(1.0 / (1.0 + np.exp(-y)) - got).max() == 0.0
    # operand: the identity only rounds the layer's input to fp32 (fc0's is fp32 already), a cut changes more
    for layer in M.LAYERS:
        same = np.abs(M.value_f64(onet, emb, operand=(layer, lambda x: x))[0] - got).max()
        assert same == 0.0 if layer == "fc0" else same <= 1e-8
        assert np.abs(M.value_f64(onet, emb, operand=(layer, P.trunc16))[0] - got).max() > 1e-7
    assert np.array_equal(M.oracle_values(onet, emb), np.array([onet.main_value(e) for e in emb], dtype=np.float32))


def test_premises_of_the_net_table(tmp_path_factory):
    """What each net of the table is there to reach, computed from the written files' dims the way the loader does
    (nbr = max(H, VH) / 32, NB = nbr > 4 ? 8 : nbr > 2 ? 4 : nbr, T0 = 4 ceil(K / 64); a group takes (T0 + 4 NB) / G phases of
    k_mainnet_pair's ring, G = 4 at NB >= 2)."""
    want = {                      # K, H, VH, NB, chunks, pair_phases
        "h32_k60": (60, 32, 32, 1, 1, 4),
        "h33_v1_k320": (320, 64, 32, 2, 5, 7),
        "h100_v40_k320": (320, 128, 64, 4, 5, 9),
        "h96_v160_k536": (536, 96, 160, 8, 9, 17),
        "h200_v72_k536": (536, 224, 96, 8, 9, 17),
        "h255_v255": (768, 256, 256, 8, 12, 20),
        "h64_v64_k1256": (1256, 64, 64, 2, 20, 22),
        "h128_v128": (768, 128, 128, 4, 12, 16),
        "256": (768, 256, 256, 8, 12, 20),
    }
    for name in M.ALL_NETS:
        onet, emb = _case(name, tmp_path_factory)
        t = M.NETS[name]
        assert (t["K"], t["hidden"], t["value_hidden"]) == (onet.fc0.in_dim, onet.fc0.out_dim, onet.v2.out_dim) and emb.shape == (N_LEAVES, t["K"])
        assert t["K"] % 4 == 0 and t["chunks"] == -(-t["K"] // 64) and t["H"] % 32 == 0 and 0 <= t["H"] - t["hidden"] < 32
        assert name in M.GOLDEN_NETS or (1 <= onet.pod <= 99 and 19 <= onet.aod <= 128)    # inside what tests/test_gpu_embedding.py covers
        if name in want:
            assert tuple(t[k] for k in ("K", "H", "VH", "NB", "chunks", "pair_phases")) == want[name], name
        if t["NB"] >= 2:
            assert t["pair_phases"] == t["chunks"] + t["NB"]
        assert t["split_phases"] % 2 == 0                                # k_mainnet_split's groups always start on buffer 0
    for name in M.ODD_PAIR_PHASES:
        assert M.NETS[name]["pair_phases"] % 2 == 1, name
    assert sorted(M.NETS[n]["NB"] for n in M.ODD_PAIR_PHASES) == [2, 4, 8, 8]
    assert {M.NETS[n]["NB"] for n in M.ALL_NETS} == {1, 2, 4, 8}
    # padded block counts: 5 and 7 blocks run as 8; K below one chunk and above 768
    assert max(M.NETS["h96_v160_k536"]["H"], M.NETS["h96_v160_k536"]["VH"]) // 32 == 5 and M.NETS["h200_v72_k536"]["H"] // 32 == 7
    assert M.NETS["h32_k60"]["K"] < 64 and M.NETS["h64_v64_k1256"]["K"] > 768 and M.NETS["h64_v64_k1256"]["K"] % 64 == 40


@pytest.mark.parametrize("name", sorted(M.RANDOM_NETS))
def test_pre_sigmoid_sums_span_the_sigmoid(tmp_path_factory, name):
    """Every random net's value_fc3 is scaled so that y covers at least [-4, 4] (values 0.018 ... 0.982) -- unscaled they are all
    0.5 +- 0.03 and the sigmoid is never checked away from its middle."""
    onet, emb = _case(name, tmp_path_factory)
    y = M.value_f64(onet, emb)[1]
    print("%s: y %.3f ... %.3f" % (name, y.min(), y.max()))
    assert y.min() <= -4.0 and y.max() >= 4.0, (y.min(), y.max())


def test_sigmoid_net_saturates_both_ways(tmp_path_factory):
    """net_256 with value_fc3 x 2^10 over the 700 leaves test_gpu_mainnet.py's sigmoid test runs: rows beyond +-90, where fp32's
    exp overflows (88.7) and the value is exactly 0 or 1."""
    onet = NN.Net(M.write_net(M.SIGMOID_NET, tmp_path_factory.mktemp("sig")))
    b, d, _ = P.batch_of(700, seed=M.SIGMOID_SEED)
    v, y = M.value_f64(onet, M.oracle_embeddings(onet, b, d))
    print("y %.2f ... %.2f, %d rows below -90, %d above 90" % (y.min(), y.max(), (y < -90).sum(), (y > 90).sum()))
    assert (y < -90).any() and (y > 90).any()
    assert (v[y < -90] < 1e-38).all() and (v[y > 90] > 1 - 1e-8).all()


@pytest.mark.parametrize("name", M.ALL_NETS)
def test_the_bound_sees_a_layer_that_lost_its_low_part(tmp_path_factory, name):
    """E_ref is positive on every net (the bound is never just its floor) and the fp32 oracle meets its own bound; an evaluation
    whose fc0, fc1 or value_fc2 multiplies operands cut to 16 significant bits -- a bf16 triple without its l part, an fp16 pair
    whose l part is lost -- lies outside the bound, for every net and every layer.  The factors (worst error / bound) of the
    16-bit cut and of a 22-bit cut are recorded, not asserted (profiles/r11_mainnet_accuracy.json: 1.6 to 32 bounds at 16 bits; 0.03 to
    0.29 at 22 bits, which the bound does not see)."""
    onet, emb = _case(name, tmp_path_factory)
    ref = M.value_f64(onet, emb)[0]
    worst, e_ref, lim = M.hold(M.oracle_values(onet, emb), onet, emb)
    assert 0 < e_ref and worst == e_ref and e_ref <= lim == 4 * e_ref + 2e-7
    assert M.hold(ref, onet, emb)[0] == 0.0
    for layer in M.LAYERS:
        lost = {bits: float(np.abs(M.value_f64(onet, emb, operand=(layer, M.trunc(bits)))[0] - ref).max()) for bits in (16, 22)}
        FACTORS["%s|%s" % (name, layer)] = dict(E_ref=e_ref, bound=lim, cut16=lost[16] / lim, cut22=lost[22] / lim)
        print("%s %s: E_ref %.3g, bound %.3g, 16-bit cut %.1f bounds, 22-bit cut %.2f bounds" % (name, layer, e_ref, lim, lost[16] / lim, lost[22] / lim))
        assert lost[16] > lim, (name, layer, lost[16], lim)
