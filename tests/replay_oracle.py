"""The replay check of `.battle.data` records (include/oakgpu.h, oakgpu_replay_records) restated on the CPU oracle: the checker the
GPU replay is held to in tests/test_gpu_replay.py and tools/verify_battle_data.py --oracle.  TEST INFRASTRUCTURE ONLY."""
import struct

import numpy as np

import oracle_lib as O

OK, COUNT, ILLEGAL, EARLY_END, RESULT, MALFORMED = range(6)
STATUS = ("OK", "COUNT", "ILLEGAL", "EARLY_END", "RESULT", "MALFORMED")


def update_bytes(m, n):
    return 11 + 4 * (m + n)


def check_record(rec):
    """The checks of CompressedFrames::read on one record (bytes): "ok", "malformed" (damaged inside its own length) or "stop" (its
    length field cannot be trusted)."""
    if len(rec) < 391:
        return "stop"
    total, frames = struct.unpack_from("<IH", rec, 0)
    if total > len(rec) or total < 391:
        return "stop"
    p, k = 391, 0
    while p < total:
        if total - p < 3:
            return "malformed"
        m, n = (rec[p] & 15) + 1, (rec[p] >> 4) + 1
        if m > 9 or n > 9 or total - p < update_bytes(m, n):
            return "malformed"
        p += update_bytes(m, n)
        k += 1
    return "ok" if k == frames else "malformed"


def replay(rec):
    """One record (bytes, exactly its own length or more) -> (status, player, frame, expected, got, battle uint8[384] at the verdict,
    durations uint8[8] at the verdict)."""
    if check_record(rec) != "ok":
        return MALFORMED, 0, 0, 0, 0, np.zeros(384, np.uint8), np.zeros(8, np.uint8)
    total, frames = struct.unpack_from("<IH", rec, 0)
    battle = np.frombuffer(rec, np.uint8, 384, 6).copy()
    stored = rec[390]
    opt = O.Options()                                                   # zero durations, no damage-roll clamp (frames.h:57-59)
    r = int(O.LIB.oracle_result_from_state(O.ptr(battle)))
    p = 391
    for k in range(frames):
        m, n, c1, c2 = (rec[p] & 15) + 1, (rec[p] >> 4) + 1, rec[p + 1], rec[p + 2]
        verdict = None
        if r & 15:
            verdict = (EARLY_END, 0, k, stored, r)
        else:
            l1, l2 = O.choices(battle, 0, (r >> 4) & 3), O.choices(battle, 1, (r >> 6) & 3)
            if len(l1) != m:
                verdict = (COUNT, 1, k, m, len(l1))
            elif len(l2) != n:
                verdict = (COUNT, 2, k, n, len(l2))
            elif c1 not in l1:
                verdict = (ILLEGAL, 1, k, c1, len(l1))
            elif c2 not in l2:
                verdict = (ILLEGAL, 2, k, c2, len(l2))
        if verdict:
            return verdict + (battle, opt.durations.copy())
        opt.set()
        r = int(O.update(battle, c1, c2, opt))
        p += update_bytes(m, n)
    return (OK if r == stored else RESULT), 0, frames, stored, r, battle, opt.durations.copy()


def replay_buffer(data):
    """Every record of a buffer, indexed like oakgpu_replay_index -> (list of (offset, replay(...)), stopped_at)."""
    out, pos = [], 0
    while pos < len(data):
        if check_record(data[pos:]) == "stop":
            break
        total = struct.unpack_from("<I", data, pos)[0]
        out.append((pos, replay(data[pos:pos + total])))
        pos += total
    return out, pos


def play_random_game(battle, seed, max_frames=2000):
    """A random-play game on the oracle from a battle after its opening update: (record fields) = (first battle, result byte,
    [(m, n, c1, c2)]) with legal choices drawn uniformly."""
    rng = np.random.default_rng(seed)
    b = np.array(battle, dtype=np.uint8).copy()
    first = b.copy()
    opt = O.Options()
    r = int(O.LIB.oracle_result_from_state(O.ptr(b)))
    frames = []
    while not (r & 15) and len(frames) < max_frames:
        l1, l2 = O.choices(b, 0, (r >> 4) & 3), O.choices(b, 1, (r >> 6) & 3)
        c1, c2 = int(l1[rng.integers(len(l1))]), int(l2[rng.integers(len(l2))])
        frames.append((len(l1), len(l2), c1, c2))
        opt.set()
        r = int(O.update(b, c1, c2, opt))
    return first, r, frames, b, opt.durations.copy()


def make_record(battle, result, frames):
    """A record in the on-disk layout with the given (m, n, c1, c2) per frame; iterations, values and probabilities are zero."""
    body = b"".join(struct.pack("<BBB", (m - 1) | ((n - 1) << 4), c1, c2) + bytes(8 + 4 * (m + n)) for m, n, c1, c2 in frames)
    return struct.pack("<IH", 391 + len(body), len(frames)) + bytes(np.asarray(battle, np.uint8)) + bytes([result]) + body
