"""EngineR::scale_boost is one multiply: x * num / den == umulhi(x << 3, M[stage + 6]) with M = ceil(2^29 * num / den).  The constants
are read from the file the build compiles (oak_amd/csrc/gen1_tables.inc, tools/gen_tables.py's output) and held to the 13 ratios of
oak_amd/data/gen1_data.json for every x below 2^16 -- the engine scales accuracies (at most 255 * 4) and unmodified stats (below 1,000)."""
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _multipliers():
    text = open(os.path.join(ROOT, "oak_amd", "csrc", "gen1_tables.inc")).read()
    m = re.search(r"const\s+uint32_t\s+OAK_BOOSTS\[13\]\s*=\s*\{([^}]*)\}", text)
    assert m, "OAK_BOOSTS is no longer a table of 13 32-bit multipliers"
    vals = [int(v.rstrip("uU")) for v in m.group(1).replace("\n", " ").split(",") if v.strip()]
    assert len(vals) == 13
    return vals


def _ratios():
    ratios = json.load(open(os.path.join(ROOT, "oak_amd", "data", "gen1_data.json")))["boosts"]
    assert len(ratios) == 13 and ratios[6][0] == ratios[6][1]     # index = stage + 6: stage 0 is the identity
    return [(int(n), int(d)) for n, d in ratios]


def test_the_multipliers_fit_32_bits_and_are_the_rounded_up_ratios():
    for m, (num, den) in zip(_multipliers(), _ratios()):
        assert 0 < m < 1 << 32
        assert m == -((-(num << 29)) // den), (m, num, den)


def test_one_multiply_equals_the_division_for_every_stage_and_every_16_bit_value():
    x = np.arange(1 << 16, dtype=np.uint64)
    for stage, (m, (num, den)) in enumerate(zip(_multipliers(), _ratios())):
        got = ((x << np.uint64(3)) * np.uint64(m)) >> np.uint64(32)      # (x << 3) * m < 2^19 * 2^32: no overflow in 64 bits
        assert (x << np.uint64(3)).max() < 1 << 32                        # ... and x << 3 fits the 32-bit operand
        want = x * np.uint64(num) // np.uint64(den)
        bad = np.where(got != want)[0]
        assert bad.size == 0, (stage - 6, num, den, bad[:8])
