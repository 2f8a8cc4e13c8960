"""CPU: the host half of the replay check of `.battle.data` records -- oakgpu_replay_index (record boundaries, MALFORMED records, the
stop offset), oakgpu_engine_switches, the CLI's --index-only mode and the C++ face.  The rules: include/oakgpu.h."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import replay_oracle as R
from oak_amd.frames import read_frames, replay_index, write_frames
from test_frames import _hand_record, _updates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _corpus(rng, counts):
    recs = []
    for i, k in enumerate(counts):
        b, ups = rng.integers(0, 256, 384, dtype=np.uint8), _updates(rng, k)
        recs.append(write_frames(b, int(rng.integers(0, 256)), ups) if i % 2 else _hand_record(b, int(rng.integers(0, 256)), ups))
    return recs


def test_index_finds_every_record_and_its_frame_count():
    rng = np.random.default_rng(11)
    counts = [3, 0, 17, 1, 80, 5]
    recs = _corpus(rng, counts)
    blob = b"".join(recs)
    idx = replay_index(blob)
    assert list(idx["offsets"]) == list(np.cumsum([0] + [len(r) for r in recs[:-1]]))
    assert list(idx["frames"]) == counts and not idx["malformed"].any() and idx["stopped_at"] == len(blob)
    empty = replay_index(b"")
    assert len(empty["offsets"]) == 0 and empty["stopped_at"] == 0


def _damage(rec, kind, rng):
    rec = bytearray(rec)
    frames = struct.unpack_from("<H", rec, 4)[0]
    offs, p = [], 391
    for _ in range(frames):
        offs.append(p)
        p += R.update_bytes((rec[p] & 15) + 1, (rec[p] >> 4) + 1)
    k = offs[int(rng.integers(len(offs)))]
    if kind == "m":
        rec[k] = (rec[k] & 0xF0) | int(rng.integers(9, 16))
    elif kind == "n":
        rec[k] = (rec[k] & 0x0F) | (int(rng.integers(9, 16)) << 4)
    elif kind == "past_end":                       # the last update runs past the record's end: the length field is cut short
        rec = rec[:-2]
        struct.pack_into("<I", rec, 0, len(rec))
    elif kind == "count":
        struct.pack_into("<H", rec, 4, frames + 1)
    return bytes(rec)


@pytest.mark.parametrize("kind", ["m", "n", "past_end", "count"])
def test_internal_damage_marks_only_that_record_malformed(kind):
    rng = np.random.default_rng(12)
    recs = _corpus(rng, [4, 9, 6, 12])
    recs[2] = _damage(recs[2], kind, rng)
    blob = b"".join(recs)
    idx = replay_index(blob)
    assert len(idx["offsets"]) == 4 and idx["stopped_at"] == len(blob)
    assert list(idx["malformed"]) == [False, False, True, False]
    with pytest.raises(RuntimeError):
        read_frames(recs[2])


def test_malformed_set_equals_what_frames_read_refuses_on_a_fuzzed_corpus():
    rng = np.random.default_rng(13)
    recs = _corpus(rng, [int(x) for x in rng.integers(0, 30, 200)])
    for i in range(len(recs)):
        if rng.random() < 0.4:
            r = bytearray(recs[i])
            for _ in range(int(rng.integers(1, 4))):
                j = int(rng.integers(391, len(r))) if len(r) > 391 and rng.random() < 0.8 else 4 + int(rng.integers(0, 2))
                r[j] = int(rng.integers(0, 256))
            recs[i] = bytes(r)
    blob = b"".join(recs)
    idx = replay_index(blob)
    assert len(idx["offsets"]) == len(recs) and idx["stopped_at"] == len(blob)
    refused = []
    for off, rec in zip(idx["offsets"], recs):
        try:
            read_frames(blob[int(off):int(off) + len(rec)])
            refused.append(False)
        except RuntimeError:
            refused.append(True)
    assert refused == list(idx["malformed"]) and 10 < sum(refused) < len(recs)
    assert refused == [R.check_record(r) == "malformed" for r in recs]


@pytest.mark.parametrize("cut", ["length_small", "length_past_end", "header", "mid_record"])
def test_untrustworthy_length_stops_indexing_and_keeps_the_records_before(cut):
    rng = np.random.default_rng(14)
    recs = _corpus(rng, [2, 7, 3])
    head = b"".join(recs[:2])
    bad = bytearray(recs[2])
    tail = recs[0]                                 # (a cut record can only be the buffer's last)
    if cut == "length_small":
        struct.pack_into("<I", bad, 0, 390)
    elif cut == "length_past_end":
        struct.pack_into("<I", bad, 0, len(bad) + len(tail) + 1)
    elif cut == "header":
        bad, tail = bad[:200], b""
    else:
        bad, tail = bad[:len(bad) - 5], b""
    blob = head + bytes(bad) + tail
    idx = replay_index(blob)
    assert idx["stopped_at"] == len(head) and len(idx["offsets"]) == 2 and not idx["malformed"].any()


def test_engine_switches_of_the_default_build():
    lib = os.environ.get("OAKGPU_LIB", "")
    if lib and "liboakgpu_v" in os.path.basename(lib):
        pytest.skip("a variant build (tools/engine_variants.sh): its switches are its name")
    from oak_amd.frames import engine_switches
    assert engine_switches() == {"MULTIHIT_ROLL_FIRST": 1, "PSYWAVE_SHOWDOWN": 1, "COUNTER_SHOWDOWN": 0, "ACCURACY_LAST": 0}


def test_cli_index_only(tmp_path):
    rng = np.random.default_rng(15)
    recs = _corpus(rng, [3, 5, 2, 8])
    (tmp_path / "a").mkdir()
    (tmp_path / "a" / "x.battle.data").write_bytes(b"".join(recs[:2]))
    bad = _damage(recs[3], "m", rng)
    (tmp_path / "y.battle.data").write_bytes(recs[2] + bad + recs[0][:100])
    (tmp_path / "ignored.txt").write_bytes(b"no")
    out = tmp_path / "summary.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "verify_battle_data.py"), str(tmp_path), "--index-only", "--json", str(out)],
                       capture_output=True, text=True)
    assert p.returncode == 1, p.stdout + p.stderr         # one MALFORMED record, one stopped file
    s = json.loads(out.read_text())
    assert s["files"] == 2 and s["records"] == 4 and s["frames"] == 3 + 5 + 2 + 8
    assert s["malformed"] == [{"file": str(tmp_path / "y.battle.data"), "offset": len(recs[2])}]
    assert s["stopped"] == [{"file": str(tmp_path / "y.battle.data"), "offset": len(recs[2]) + len(bad)}]
    (tmp_path / "y.battle.data").unlink()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "verify_battle_data.py"), str(tmp_path), "--index-only"], capture_output=True, text=True)
    assert p.returncode == 0 and json.loads(p.stdout)["records"] == 2, p.stdout + p.stderr
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "verify_battle_data.py"), str(tmp_path / "missing"), "--index-only"],
                          capture_output=True).returncode == 2


def test_cpp_replay_check_compiles_against_the_header(tmp_path):
    src = tmp_path / "replay_check.cc"
    src.write_text('#include "oakgpu.hpp"\n#include <cstdio>\n'
                   'int main(int argc, char **argv) {\n'
                   '  std::vector<uint8_t> bytes;\n'
                   '  if (argc > 1) return 0;\n'
                   '  OakGPU::Context ctx(0);\n'
                   '  OakGPU::ReplayCheck rc = OakGPU::replay_check(ctx, bytes, true);\n'
                   '  for (const auto &r : rc.reports) std::printf("%u %u\\n", r.status, r.frame);\n'
                   '  return (int)rc.stopped_at + (int)rc.battles.size() + (int)rc.durations.size() + (int)rc.offsets.size();\n'
                   '}\n')
    exe = str(tmp_path / "replay_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", os.path.join(ROOT, "oak_amd"),
                           "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert subprocess.run([exe, "x"]).returncode == 0
