"""A numpy / Python float64 restatement of one self-play turn's pick (oak_amd/csrc/selfplay_pick.hpp): the game's random stream,
MCTS::Search::process_output's empirical fields, RuntimePolicy::get_policy, device.sample_pdf and the bytes of a CompressedFrames Update.
Written from the rule's description in include/oakgpu.h, not from the header's text; tests/test_forestplay_ref.py holds it bit for bit to
oakgpu_selfplay_pick_host, tests/test_gpu_forest_selfplay.py uses it to say what the device game loop must have picked.

Python floats are IEEE doubles and every sum below runs in the stated order, so with policy_temp = 1 every number here is the library's."""
import struct

import numpy as np

MASK = (1 << 64) - 1
GAME_STREAM_XOR = 0x9FB21C651E98DF25
HEAD_BYTES = 4 + 2 + 384 + 1


def splitmix64(state):
    """(new state, output)"""
    state = (state + 0x9E3779B97F4A7C15) & MASK
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return state, z ^ (z >> 31)


def uniform01(state):
    state, z = splitmix64(state)
    return state, float(z >> 11) * (1.0 / 9007199254740992.0)


def game_stream(seed):
    return (int(seed) ^ GAME_STREAM_XOR) & MASK


def process_output(visits, values, m, n, iterations):
    """visits / values: [9, 9].  Returns (empirical_value, p1_empirical[9], p2_empirical[9], payoffs [m][n] ints)."""
    e1, e2 = [0.0] * 9, [0.0] * 9
    tv, M = 0.0, [[0] * n for _ in range(m)]
    for i in range(m):
        for j in range(n):
            tv += float(values[i][j])
            v = int(visits[i][j])
            e1[i] += float(v)
            e2[j] += float(v)
            v = v or 1
            M[i][j] = int(float(values[i][j]) / float(v) * 256.0)
    den = float(np.float32(iterations))
    ev = tv / float(iterations)
    for i in range(m):
        e1[i] /= den
    for j in range(n):
        e2[j] /= den
    return ev, e1, e2, M


def parse_mode(mode):
    """[(letter, weight)] of a mode string such as "e0.9-x0.1"; ValueError for a letter outside e / n / x / p."""
    words = []
    for word in (mode or "e").split("-"):
        if not word:
            continue
        if word[0] not in "enxp":
            raise ValueError("policy mode letter %r" % word[0])
        words.append((word[0], float(word[1:]) if len(word) > 1 else 1.0))
    return words


def get_policy(prior, empirical, nash, k, words, temp=1.0, minp=0.0):
    """The 9-entry policy, or None when the minimum cut zeroes all of it."""
    pol = [0.0] * 9
    for letter, w in words:
        if letter == "p":
            for i in range(k):
                pol[i] += w * prior[i] + w * empirical[i]
        elif letter == "e":
            for i in range(k):
                pol[i] += w * empirical[i]
        elif letter == "n":
            for i in range(k):
                pol[i] += w * nash[i]
        else:
            best = 0
            for i in range(1, k):
                if empirical[best] < empirical[i]:
                    best = i
            pol[best] += w
    if temp != 1:
        pol = [x ** temp for x in pol]
        s = 0.0
        for x in pol:
            s += x
        pol = [x / s for x in pol]
    s = 0.0
    for i in range(9):
        if pol[i] < minp:
            pol[i] = 0.0
        s += pol[i]
    if not s > 0:
        return None
    return [x / s for x in pol]


def sample_pdf(p, k, state):
    """(new state, index, the uniform drawn)"""
    state, u0 = uniform01(state)
    u = u0
    for i in range(k):
        u -= p[i]
        if u <= 0:
            return state, i, u0
    return state, 0, u0


def compress_prob(x):
    v = float(x) * 65535.0
    return 0 if v <= 0 else 65535 if v >= 65535.0 else int(v)


def encode_update(m, n, c1, c2, iterations, ev, nv, e1, n1, e2, n2):
    out = struct.pack("<BBBIHH", (m - 1) | ((n - 1) << 4), c1, c2, iterations & 0xFFFFFFFF, compress_prob(ev), compress_prob(nv))
    for arr, k in ((e1, m), (n1, m), (e2, n), (n2, n)):
        out += struct.pack("<%dH" % k, *[compress_prob(arr[q]) for q in range(k)])
    return out


def pick(m, n, visits, values, iterations, state, p1_nash=None, p2_nash=None, nash_value=0.0, p1_prior=None, p2_prior=None, p1_choices=None,
         p2_choices=None, mode="e", temp=1.0, minp=0.0):
    """One turn.  Returns a dict like oak_amd.frames.selfplay_pick_host's plus "u1" / "u2" (the uniforms drawn), or None for a zeroed policy."""
    pad = lambda a: [0.0] * 9 if a is None else ([float(x) for x in a] + [0.0] * 9)[:9]
    n1, n2, r1, r2 = pad(p1_nash), pad(p2_nash), pad(p1_prior), pad(p2_prior)
    ev, e1, e2, M = process_output(visits, values, m, n, iterations)
    words = parse_mode(mode)
    temp = temp if temp > 0 else 1.0
    pol1 = get_policy(r1, e1, n1, m, words, temp, minp)
    pol2 = get_policy(r2, e2, n2, n, words, temp, minp)
    if pol1 is None or pol2 is None:
        return None
    state, i, u1 = sample_pdf(pol1, m, state)
    state, j, u2 = sample_pdf(pol2, n, state)
    c1 = i if p1_choices is None else int(p1_choices[i])
    c2 = j if p2_choices is None else int(p2_choices[j])
    return {"empirical_value": ev, "p1_empirical": e1, "p2_empirical": e2, "p1_policy": pol1, "p2_policy": pol2, "i": i, "j": j, "rng": state,
            "u1": u1, "u2": u2, "payoffs": M, "update": encode_update(m, n, c1, c2, iterations, ev, nash_value, e1, n1, e2, n2)}


def assemble_record(battle, result, updates):
    """One CompressedFrames record from the stored battle (384 bytes), the result byte and the updates' bytes."""
    body = b"".join(updates)
    return struct.pack("<IH", HEAD_BYTES + len(body), len(updates)) + bytes(bytearray(battle)) + bytes([result]) + body


def split_updates(record):
    """The updates' byte strings of one record."""
    total, frames = struct.unpack_from("<IH", record, 0)
    out, pos = [], HEAD_BYTES
    while pos < total:
        m, n = (record[pos] & 15) + 1, (record[pos] >> 4) + 1
        size = 11 + 4 * (m + n)
        out.append(record[pos:pos + size])
        pos += size
    assert len(out) == frames and pos == total
    return out


def decode_update(u):
    """The stored fields of one update's bytes, probabilities as their stored u16."""
    mn, c1, c2, iterations, ev, nv = struct.unpack_from("<BBBIHH", u, 0)
    m, n = (mn & 15) + 1, (mn >> 4) + 1
    f = struct.unpack_from("<%dH" % (2 * (m + n)), u, 11)
    return {"m": m, "n": n, "c1": c1, "c2": c2, "iterations": iterations, "empirical_value": ev, "nash_value": nv, "p1_empirical": f[:m],
            "p1_nash": f[m:2 * m], "p2_empirical": f[2 * m:2 * m + n], "p2_nash": f[2 * m + n:]}
