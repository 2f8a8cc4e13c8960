"""CPU: the replay window without a device -- the eviction rule's two referees against each other (tests/window_ref.py), the shared scan
header (oak_amd/csrc/record_scan.hpp) through its host-only entry point against oakgpu_replay_index and the referee on every damage
class, the refusals of oakgpu_corpus_window_check by message, the ABI, and the stand-alone tests/cpp_window_check.cc plain and under
sanitizers (the host form of the scan rule and the window's host bookkeeping)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import window_ref as W
from oak_amd import _lib
from oak_amd.frames import replay_index, write_frames
from oak_amd.train import window_check, window_scan_host
from test_frames import _hand_record, _updates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("oakgpu_corpus_window_check", "oakgpu_corpus_create_window", "oakgpu_corpus_append_dev", "oakgpu_corpus_append", "oakgpu_corpus_window_stats",
         "oakgpu_corpus_records", "oakgpu_window_scan_host")


def _records(rng, counts):
    out = []
    for i, k in enumerate(counts):
        b, ups = rng.integers(0, 256, 384, dtype=np.uint8), _updates(rng, k)
        out.append(write_frames(b, int(rng.integers(0, 256)), ups) if i % 2 else _hand_record(b, int(rng.integers(0, 256)), ups))
    return out


def _batch(rng, n):
    """n slices: whole records, every damage class, dropped games"""
    recs = _records(rng, [int(x) for x in rng.integers(1, 40, n)])
    kinds = W.MALFORMED_KINDS + W.REJECTED_KINDS
    for i in range(n):
        roll = rng.random()
        if roll < 0.15:
            recs[i] = b""
        elif roll < 0.6:
            recs[i] = W.damage(recs[i], kinds[i % len(kinds)], rng)
    return recs


def test_library_exports_the_window_calls():
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    for name in CALLS:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None, name


def test_struct_sizes_the_window_relies_on(tmp_path):
    """oakgpu_corpus_stats as the mirror has it (info() of a window goes through it), and the summary an append reads once"""
    src, exe = str(tmp_path / "probe.cc"), str(tmp_path / "probe")
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "oakgpu.h"\n#include "../oak_amd/csrc/record_scan.hpp"\n'
                         'int main() { printf("%zu %zu %zu %zu %zu\\n", sizeof(oakgpu_corpus_stats), offsetof(oakgpu_corpus_stats, frames), '
                         "offsetof(oakgpu_corpus_stats, stopped_at), sizeof(oak_scan::AppendSummary), offsetof(oak_scan::AppendSummary, bytes)); return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.CorpusStats
    assert got == [C.sizeof(S), S.frames.offset, S.stopped_at.offset, 40, 24]


def test_window_check_refuses_by_message():
    window_check(1, 391)
    window_check(2 ** 32 - 1, 1 << 40)
    for args, text in (((0, 1 << 20), "max_records must be at least 1"), ((8, 390), "max_bytes is below one minimal record"), ((8, 0), "max_bytes")):
        with pytest.raises(_lib.OakGpuError) as e:
            window_check(*args)
        assert text in str(e.value) and "oakgpu_corpus_create_window:" in str(e.value)


def test_calls_refuse_null_arguments_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.oakgpu_corpus_create_window(None, 4, 1 << 20, C.byref(h)) != 0 and "oakgpu_corpus_create_window: null ctx" in lib.oakgpu_last_error().decode()
    assert lib.oakgpu_corpus_append_dev(None, None, None, None, 1) != 0 and "oakgpu_corpus_append_dev: null ctx or corpus" in lib.oakgpu_last_error().decode()
    assert lib.oakgpu_corpus_append(None, None, None, 0) != 0 and "oakgpu_corpus_append: null ctx or corpus" in lib.oakgpu_last_error().decode()
    assert lib.oakgpu_corpus_records(None, None, None, 0, None, 0) != 0 and "oakgpu_corpus_records:" in lib.oakgpu_last_error().decode()
    out = (C.c_uint64 * 6)()
    assert lib.oakgpu_corpus_window_stats(None, C.byref(out)) != 0 and "oakgpu_corpus_window_stats:" in lib.oakgpu_last_error().decode()


@pytest.mark.parametrize("kind", W.MALFORMED_KINDS + W.REJECTED_KINDS)
def test_scan_header_on_every_damage_class(kind):
    rng = np.random.default_rng(31)
    recs = _records(rng, [4, 9, 6, 12, 1])
    recs[2] = W.damage(recs[2], kind, rng)
    recs.insert(1, b"")
    stream, offsets = W.slices(recs)
    kinds, frames = window_scan_host(stream, offsets)
    want = [W.classify(r) for r in recs]
    assert [(int(k), int(f)) for k, f in zip(kinds, frames)] == want
    assert want[3][0] == (W.MALFORMED if kind in W.MALFORMED_KINDS else W.REJECTED) and want[1] == (W.DROPPED, 0)
    # against the host indexer on the same bytes: a malformed record is indexed with its flag and the header's frame count; where a slice is
    # rejected the indexer stops, or goes on at another boundary than the slice's
    idx = replay_index(stream)
    if kind in W.MALFORMED_KINDS:
        assert len(idx["offsets"]) == 5 and list(idx["malformed"]) == [k == W.MALFORMED for k in kinds if k != W.DROPPED]
        assert list(idx["frames"]) == [int(f) for k, f in zip(kinds, frames) if k != W.DROPPED] and idx["stopped_at"] == len(stream)
    else:
        assert list(idx["offsets"][:2]) == [int(offsets[0]), int(offsets[2])]
        assert idx["stopped_at"] != len(stream) or [int(o) for o in idx["offsets"]] != [int(o) for o, k in zip(offsets, kinds) if k in (W.OK, W.MALFORMED)]


def test_scan_header_equals_the_indexer_on_a_fuzzed_corpus():
    rng = np.random.default_rng(32)
    recs = _records(rng, [int(x) for x in rng.integers(0, 30, 300)])
    for i in range(len(recs)):
        if rng.random() < 0.4:
            r = bytearray(recs[i])
            for _ in range(int(rng.integers(1, 4))):
                j = int(rng.integers(391, len(r))) if len(r) > 391 and rng.random() < 0.8 else 4 + int(rng.integers(0, 2))
                r[j] = int(rng.integers(0, 256))
            recs[i] = bytes(r)
    stream, offsets = W.slices(recs)
    kinds, frames = window_scan_host(stream, offsets)
    idx = replay_index(stream)
    assert [int(o) for o in idx["offsets"]] == [int(o) for o in offsets[:-1]]
    assert list(idx["malformed"]) == [k == W.MALFORMED for k in kinds] and list(idx["frames"]) == list(frames) and 10 < (kinds == W.MALFORMED).sum() < len(recs)
    assert [(int(k), int(f)) for k, f in zip(kinds, frames)] == [W.classify(r) for r in recs]


def test_offsets_that_run_backwards_are_rejected():
    rec = _records(np.random.default_rng(33), [3])[0]
    kinds, frames = window_scan_host(rec + rec, np.array([len(rec), 0, len(rec)], dtype=np.uint64))
    assert list(kinds) == [W.REJECTED, W.OK] and list(frames) == [0, 3]


@pytest.mark.parametrize("max_records,max_bytes", [(1, 1 << 30), (7, 1 << 30), (1 << 20, 5000), (5, 3000), (1 << 20, 391), (1 << 20, 1 << 30)])
def test_the_two_referees_of_the_eviction_rule_agree(max_records, max_bytes):
    rng = np.random.default_rng(34)
    win, batches = W.Window(max_records, max_bytes), []
    for b, n in enumerate((5, 1, 0, 12, 3, 30, 2)):
        pieces = _batch(rng, n)
        got = win.append(pieces, tags=[(b, i) for i in range(n)])
        classes = [W.classify(p) for p in pieces]
        batches.append(([len(p) for p in pieces], [k for k, _ in classes]))
        survivors, stats = W.evict(batches, max_records, max_bytes)
        assert win.tags() == survivors and got == stats
        assert got["records"] <= max_records and got["bytes"] <= max_bytes and got["appended"] - got["evicted"] == got["records"]
    assert win.stats()["rejected"] > 0 and win.stats()["appends"] == 7


def test_eviction_rule_on_hand_cases():
    rec = lambda size: struct.pack("<IH", size, 0) + bytes(size - 6)
    win = W.Window(3, 2000)
    assert win.append([rec(500), rec(600), rec(700)])["records"] == 3                        # 1,800 bytes
    assert win.append([rec(400)]) == {"records": 3, "bytes": 1700, "appended": 4, "evicted": 1, "rejected": 0, "appends": 2}
    assert win.append([rec(1500)])["records"] == 2 and win.stats()["bytes"] == 1900          # the byte cap cuts: 400 + 1500
    assert win.append([rec(2001)]) == {"records": 0, "bytes": 0, "appended": 6, "evicted": 6, "rejected": 0, "appends": 4}   # larger than the window
    assert win.append([rec(391)] * 5)["records"] == 3 and win.stats()["evicted"] == 8        # a batch larger than the window leaves its tail
    assert win.append([b"", b""])["records"] == 3 and win.stats()["appends"] == 6            # an all-dropped batch changes nothing else
    assert win.append([rec(600), rec(2001), rec(391)])["records"] == 1                      # nothing older than a record that does not fit survives


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ids=("plain", "sanitizers"))
def test_standalone_program(tmp_path, flags):
    rng = np.random.default_rng(35)
    pieces = _batch(rng, 120)
    pieces[-1] = W.damage(_records(rng, [5])[0], "header_cut", rng)          # the stream's last slice is a cut record
    stream, offsets = W.slices(pieces)
    exe, data = str(tmp_path / "check"), str(tmp_path / "slices.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp_window_check.cc"), "-o", exe], check=True)
    open(data, "wb").write(struct.pack("<I", len(pieces)) + offsets.tobytes() + stream)
    for max_records, max_bytes, batch in ((1 << 20, 1 << 30, 16), (10, 1 << 30, 7), (1 << 20, 6000, 16), (1, 391, 1)):
        run = subprocess.run([exe, data, str(max_records), str(max_bytes), str(batch)], capture_output=True, text=True)
        assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
        lines = run.stdout.splitlines()
        assert [tuple(int(x) for x in l.split()) for l in lines[:len(pieces)]] == [W.classify(p) for p in pieces]
        win = W.Window(max_records, max_bytes)
        for lo in range(0, len(pieces), batch):
            win.append(pieces[lo:lo + batch])
        st, info = win.stats(), win.info()
        assert [int(x) for x in lines[len(pieces)].split()] == [info["records"], info["malformed"], info["frames"], st["bytes"], st["appended"], st["evicted"],
                                                                 st["rejected"], st["appends"]]
        assert lines[len(pieces) + 1] == "refused %d" % (2 * st["appends"])
