"""The referee of the replay window (include/oakgpu.h: oakgpu_corpus_create_window), in numpy and plain Python: the slice rule of an
append, the eviction rule, and the damage every test of the window builds its batches from.  Nothing here calls the library."""
import struct

import numpy as np

FIXED = 4 + 2 + 384 + 1
DROPPED, OK, MALFORMED, REJECTED = 0, 1, 2, 3
MALFORMED_KINDS = ("m", "n", "past_end", "count", "short_update")
REJECTED_KINDS = ("length_small", "length_short", "length_long", "header_cut")


def update_bytes(m, n):
    return 11 + 4 * (m + n)


def classify(piece):
    """(kind, frames) of one slice by oakgpu_frames_read's rules: the frame count is the header's for a record, 0 otherwise."""
    piece = bytes(piece)
    if len(piece) == 0:
        return DROPPED, 0
    if len(piece) < FIXED:
        return REJECTED, 0
    total, frames = struct.unpack_from("<IH", piece, 0)
    if total != len(piece):
        return REJECTED, 0
    p, n_read = FIXED, 0
    while p < total:
        if total - p < 3:
            return MALFORMED, frames
        m, n = (piece[p] & 15) + 1, (piece[p] >> 4) + 1
        if m > 9 or n > 9 or total - p < update_bytes(m, n):
            return MALFORMED, frames
        p += update_bytes(m, n)
        n_read += 1
    return (OK if n_read == frames else MALFORMED), frames


def damage(rec, kind, rng):
    """A damaged copy of a well-formed record with at least one frame.  MALFORMED_KINDS stay inside the record's own length (the first
    four are tests/test_replay_index.py's); REJECTED_KINDS make the length field disagree with the slice."""
    rec = bytearray(rec)
    frames = struct.unpack_from("<H", rec, 4)[0]
    offs, p = [], FIXED
    for _ in range(frames):
        offs.append(p)
        p += update_bytes((rec[p] & 15) + 1, (rec[p] >> 4) + 1)
    k = offs[int(rng.integers(len(offs)))]
    if kind == "m":
        rec[k] = (rec[k] & 0xF0) | int(rng.integers(9, 16))
    elif kind == "n":
        rec[k] = (rec[k] & 0x0F) | (int(rng.integers(9, 16)) << 4)
    elif kind == "past_end":
        rec = rec[:-2]
        struct.pack_into("<I", rec, 0, len(rec))
    elif kind == "count":
        struct.pack_into("<H", rec, 4, frames + 1)
    elif kind == "short_update":                     # two bytes of an update at the end: fewer than its three header bytes
        rec = rec[:offs[-1] + 2]
        struct.pack_into("<I", rec, 0, len(rec))
    elif kind == "length_small":
        struct.pack_into("<I", rec, 0, FIXED - 1)
    elif kind == "length_short":                     # a length inside the slice: the host's walk would find another boundary
        struct.pack_into("<I", rec, 0, len(rec) - 1)
    elif kind == "length_long":
        struct.pack_into("<I", rec, 0, len(rec) + 7)
    elif kind == "header_cut":
        rec = rec[:200]
    else:
        raise ValueError(kind)
    return bytes(rec)


def slices(pieces):
    """stream bytes and offsets uint64[n + 1] of a batch of slices"""
    return b"".join(pieces), np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)


class Window:
    """The window's rule on lists: after each append the survivors are the longest suffix of (survivors + accepted slices) with at most
    max_records records in at most max_bytes bytes."""

    def __init__(self, max_records, max_bytes):
        assert max_records >= 1 and max_bytes >= FIXED
        self.max_records, self.max_bytes = int(max_records), int(max_bytes)
        self.items = []          # (tag, bytes, malformed, frames) in arrival order
        self.appended = self.evicted = self.rejected = self.appends = 0

    def append(self, pieces, tags=None):
        self.appends += 1
        joined = list(self.items)
        for i, piece in enumerate(pieces):
            kind, frames = classify(piece)
            if kind == REJECTED:
                self.rejected += 1
            elif kind != DROPPED:
                self.appended += 1
                joined.append((None if tags is None else tags[i], bytes(piece), kind == MALFORMED, frames))
        keep, size = 0, 0
        for item in reversed(joined):
            if keep + 1 > self.max_records or size + len(item[1]) > self.max_bytes:
                break
            keep, size = keep + 1, size + len(item[1])
        self.evicted += len(joined) - keep
        self.items = joined[len(joined) - keep:]
        return self.stats()

    def stats(self):
        return {"records": len(self.items), "bytes": sum(len(i[1]) for i in self.items), "appended": self.appended, "evicted": self.evicted,
                "rejected": self.rejected, "appends": self.appends}

    def bytes(self):
        return b"".join(i[1] for i in self.items)

    def tags(self):
        return [i[0] for i in self.items]

    def info(self):
        return {"records": len(self.items), "malformed": sum(1 for i in self.items if i[2]), "frames": sum(i[3] for i in self.items if not i[2]),
                "stopped_at": len(self.bytes())}


def evict(batches, max_records, max_bytes):
    """The rule on sizes and classes alone: batches = [(sizes, kinds), ...] -> (survivors as (batch, index) pairs, stats).  The numpy form
    (a reversed cumulative sum) of what Window does item by item."""
    where = np.array([(b, i) for b, (sizes, kinds) in enumerate(batches) for i in range(len(sizes))], dtype=np.int64).reshape(-1, 2)
    sizes = np.concatenate([np.asarray(s, dtype=np.int64) for s, _ in batches] + [np.zeros(0, np.int64)])
    kinds = np.concatenate([np.asarray(k, dtype=np.int64) for _, k in batches] + [np.zeros(0, np.int64)])
    stats = {"appended": int(((kinds == OK) | (kinds == MALFORMED)).sum()), "rejected": int((kinds == REJECTED).sum()), "appends": len(batches)}
    alive = np.zeros(len(sizes), dtype=bool)
    for b in range(len(batches)):
        alive |= (where[:, 0] == b) & ((kinds == OK) | (kinds == MALFORMED))
        idx = np.flatnonzero(alive)[::-1]                                    # newest first
        fits = (np.arange(1, len(idx) + 1) <= max_records) & (np.cumsum(sizes[idx]) <= max_bytes)
        keep = int(fits.argmin()) if not fits.all() else len(idx)            # the first that does not fit ends the window
        alive[idx[keep:]] = False
    stats.update(records=int(alive.sum()), bytes=int(sizes[alive].sum()), evicted=stats["appended"] - int(alive.sum()))
    return [tuple(int(x) for x in w) for w in where[alive]], stats
