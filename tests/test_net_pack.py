"""CPU: the battle-net loader's host half (oak_amd/csrc/net_pack.hpp) stand-alone.  tests/cpp_net_pack_check.cc packs a list of
networks -- the golden files, synthetic shapes at the block-count edges, one edit per safety flag, one file per refusal text -- and
prints dims, flags and the FNV-1a digest of every image in upload order.  tests/golden/net_pack_digests.json holds that output as
recorded from the loader's text before it was simplified (the bytes oakgpu_net_load* uploaded then); it does not change with the
packer.  The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, a process of its own."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_net_pack_check.cc")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "net_pack_digests.json")

QUANT = "Invalid layer size for quantized net %s (check code for valid sizes)."
REFUSALS = {
    "refuse_short_header": "network file: truncated header",
    "refuse_activation_byte": "network file: unknown activation byte",
    "refuse_discrete_relu": "Agent: .discrete was specified but the parsed header does not encode clamped activations.",
    "refuse_truncated_layer": "network file: truncated or malformed layer",
    "refuse_trailing_byte": "network file: trailing bytes (network.h:60-63)",
    "refuse_nan_active_fc0": "network file: non-finite parameter (NaN / inf) in active_net.fc0",
    "refuse_inf_value_fc2": "network file: non-finite parameter (NaN / inf) in main_net.value_fc2",
    "refuse_embedding_input_dims": "network file: embedding input dims must be 198 / 427",
    "refuse_inconsistent_dims": "network file: inconsistent layer dims",
    "refuse_embedding_width_129": "embedding widths above 128 unsupported",
    "refuse_fc0_input": "network file: fc0 input != 2 * side embedding",
    "refuse_fc0_fc1_widths": "network file: fc0/fc1 widths differ",
    "refuse_width_288": "main-net widths above 256 unsupported",
    "refuse_multiple_of_4": "embedding dim must be a multiple of 4",
    "refuse_policy_heads": "network file: inconsistent policy-head dims",
    "refuse_policy_width_288": "policy hidden width above 256 unsupported",
    "refuse_quant_side_dim": QUANT % "Side dim: 320",
    "refuse_quant_hidden": QUANT % "Hidden: 96",
    "refuse_quant_value_hidden": QUANT % "Value hidden: 48",
    "refuse_quant_policy_hidden": QUANT % "Policy hidden: 40",
    "refuse_quant_value_above_hidden": QUANT % "Value hidden cannot be larger than hidden.",
    "refuse_quant_policy_above_hidden": QUANT % "Policy hidden cannot be larger than hidden.",
    "refuse_quant_bad_in_dim": "bad in dim",
    "refuse_quant_bad_out_dim": "bad out dim",
    "refuse_quant_weight_2": "3non clamped2.000000",
    "refuse_quant_bias_int32": "quantized net: bias 1 of main_net.fc0 is outside int32 (1000000.000000)",
    # two faults in one file: the loader's first check wins
    "order_nan_then_width_288": "network file: non-finite parameter (NaN / inf) in main_net.fc1",
    "order_multiple_of_4_then_policy_heads": "embedding dim must be a multiple of 4",
}
# (split_safe, embed_safe, pair_safe, policy_safe) and the images that must be absent
FLAGS = {
    "synth_96_160_40": ((True, True, True, True), []),
    "synth_96_160_72": ((True, True, True, True), ["q1b_img", "q2b_img"]),
    "flag_main_weight_2p21": ((False, False, False, True), ["q1b_img", "q2b_img"]),
    "flag_policy_fc3_weight_2p21": ((True, True, True, False), ["q1b_img", "q2b_img", "q1a_t", "q2a_t"]),
    "flag_fc0_column_2m20": ((True, True, False, True), ["q1b_img", "q2b_img"]),
    "flag_embed_row_2m30": ((True, True, True, True), ["q1b_img", "q2b_img"]),
}


def host_compiler():
    """ROCm's clang++, found from hipcc the way build() finds hipcc (g++ 11 has no _Float16 on x86-64; this is the compiler that
    builds the library's host code)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found: the packer's check program needs ROCm's clang++"
    bindir = os.path.dirname(os.path.realpath(hipcc))
    for cand in (os.path.join(bindir, "..", "lib", "llvm", "bin", "clang++"), os.path.join(bindir, "amdclang++"), os.path.join(bindir, "clang++")):
        if os.path.exists(cand):
            return os.path.normpath(cand)
    raise AssertionError("no clang++ beside " + hipcc)


def build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run([host_compiler(), "-std=c++17"] + flags + [SRC, "-o", exe], check=True)
    run = subprocess.run([exe, GOLDEN_DIR], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("net_pack"), "net_pack_check", ["-O2"])


def first_difference(got, want):
    if got.get("net") != want.get("net"):
        return "network %r where %r was recorded" % (got.get("net"), want.get("net"))
    for key in sorted(set(got) | set(want)):
        if key != "images" and got.get(key) != want.get(key):
            return "%s: %s is %r, recorded %r" % (want["net"], key, got.get(key), want.get(key))
    gi, wi = got.get("images", []), want.get("images", [])
    for k in range(max(len(gi), len(wi))):
        g, w = gi[k] if k < len(gi) else None, wi[k] if k < len(wi) else None
        if g != w:
            return "%s: image %d is %r, recorded %r" % (want["net"], k, g, w)
    return None


def test_digests_match_the_recorded_bytes(output):
    got, want = json.loads(output), json.load(open(GOLDEN))
    for g, w in zip(got, want):
        diff = first_difference(g, w)
        assert diff is None, diff
    assert len(got) == len(want)
    assert output == open(GOLDEN).read()


def test_refusal_texts(output):
    docs = {d["net"]: d for d in json.loads(output)}
    assert {n: docs[n].get("refused") for n in REFUSALS} == REFUSALS
    assert sorted(n for n, d in docs.items() if "refused" in d) == sorted(REFUSALS)


def test_flags_and_absent_images(output):
    docs = {d["net"]: d for d in json.loads(output)}
    full = [i["name"] for i in docs["synth_96_160_40"]["images"]]
    for net, (flags, absent) in FLAGS.items():
        d = docs[net]
        assert (d["split_safe"], d["embed_safe"], d["pair_safe"], d["policy_safe"]) == flags, net
        assert [i["name"] for i in d["images"]] == [n for n in full if n not in absent], net
    # the shapes the cases are there for
    assert (docs["net_tiny"]["T0"], docs["net_tiny"]["PB"], docs["net_tiny"]["dims"]["VH"]) == (8, 1, 32)
    assert (docs["net_default"]["PH"], docs["net_256"]["NB"]) == (64, 8)
    assert (docs["synth_96_160_40"]["NB"], docs["synth_96_160_40"]["PB"], docs["synth_96_160_72"]["PB"]) == (8, 2, 4)
    for net in ("net_default_discrete", "synth_discrete_32"):
        names = [i["name"] for i in docs[net]["images"]]
        assert names[:len(full)] == full and names[len(full):] == ["q.img", "q.b0", "q.b1", "q.b2", "q.w3"] + [
            "q.%s[%d]" % (f, h) for h in (0, 1) for f in ("pw2", "pb2", "pw3", "pb3")], net
    assert docs["net_default_discrete"]["q"]["img_bytes"] == docs["net_default_discrete"]["images"][len(full)]["bytes"]


def test_standalone_program_under_sanitizers(tmp_path, output):
    """a process of its own, nothing preloaded: every layout walk and the file reader under AddressSanitizer and
    UndefinedBehaviorSanitizer, with the same output"""
    san = build_and_run(tmp_path, "net_pack_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert san == output
