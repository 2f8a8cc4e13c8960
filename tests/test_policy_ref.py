"""CPU: the yardstick of tests/test_gpu_policy.py, tested on its own -- the vectorised policy index against nn_oracle.policy_index,
the fp32 numpy oracle's heads against the float64 evaluation (its worst distance E_ref is what the kernels' bound is made of), the
proof that the bound sees an fc2 that lost its low bf16 part, and the choice forms the mid-game states contain."""
import numpy as np
import pytest

import policy_ref as P
from policy_ref import NN

_CHOICES = {}


def _oracle_choices():
    if not _CHOICES:
        b, d, r = P.form_states()
        _CHOICES["v"] = (b, d, r, [P.oracle_choices(b, r, pl) for pl in range(2)])
    return _CHOICES["v"]


def test_policy_rows_equal_policy_index_on_every_entry():
    b, d, r, ch = _oracle_choices()
    assert b.shape[0] > 10000
    pairs = set()
    for head, (c, cnt) in enumerate(ch):
        rows = P.policy_rows(b, c, cnt, head)
        want = np.full(rows.shape, -1, dtype=np.int64)
        for i in range(b.shape[0]):
            side = b[i, 184 * head:184 * head + 184]
            want[i, :cnt[i]] = [NN.policy_index(side, int(x)) for x in c[i, :cnt[i]]]
        assert np.array_equal(rows, want), np.argwhere(rows != want)[:4]
        assert rows.max() < 315
        pairs |= {(head, int(x)) for x in np.unique(rows[rows >= 0])}
    assert len(pairs) >= 600, len(pairs)


def test_mid_game_states_contain_every_choice_form():
    """The condition test_gpu_policy.py asserts on the GPU's choices, here on the oracle's: at least 20 leaves of every form and head."""
    b, d, r, ch = _oracle_choices()
    for head, (c, cnt) in enumerate(ch):
        forms = P.choice_forms(b, c, cnt, head)
        print("head %d: %s" % (head, forms))
        assert min(forms.values()) >= P.MIN_PER_FORM, (head, forms)


def _golden_case(tag, n=700):
    onet = NN.Net(P.GOLDEN[tag])
    b, d, r = P.batch_of(n, seed=7)
    emb = np.stack([NN.battle_embedding(onet, b[i], d[i]) for i in range(n)])
    rows = [P.policy_rows(b, *P.oracle_choices(b, r, pl), head=pl) for pl in range(2)]
    return onet, emb, rows


@pytest.mark.parametrize("tag", ["default", "tiny", "256"])
def test_fp32_oracle_heads_against_float64_and_the_bound_sees_a_lost_part(tag):
    """E_ref: the fp32 numpy oracle's worst distance from the float64 heads (measured over these 700 leaves: 1.1e-7 to 1.5e-7).  An fc2
    whose operands keep 16 significant bits (a bf16 triple without its l part) is 1.1e-5 to 1.7e-5 away -- it must break the bound
    4 E_ref + 2e-7 S that the kernels are held to (0.64e-6 to 0.89e-6 here; the older 2e-5 bar lets it pass on all three nets)."""
    onet, emb, rows = _golden_case(tag)
    ref = P.logits_f64(onet, emb)
    e_ref, s, cnt = P.yardstick(ref, P.oracle_logits(onet, emb), rows)
    lim = P.bound(e_ref, s)
    lost = P.worst_error([P.gather(x, r_) for x, r_ in zip(P.logits_f64(onet, emb, fc2_operand=P.trunc16), rows)], ref, rows)
    print("net_%s: E_ref %.3g, S %.3g, bound %.3g, 16-bit fc2 %.3g over %d logits" % (tag, e_ref, s, lim, lost, cnt))
    assert 0 < e_ref <= 1e-6 and cnt > 5000
    assert lim < 2.0 ** -17 * s / 2          # the bound stays clear of where a dropped low part sits
    assert lost > lim, (lost, lim)
    assert P.worst_error([P.gather(x, r_) for x, r_ in zip(ref, rows)], ref, rows) == 0.0
