"""Manual GPU tool: the quantized (discrete) leaf evaluator against the fp32 one on the same file.

65,536 device-resident mid-game leaves; a clamp-header network of the default shape (768-64-64-32, policy 64, main-net weights
stretched over (-1.9, 1.9)), evaluated (1) as fp32 (k_mainnet_pair, fp16 pairs), (2) as discrete (k_mainnet_i8), and (3) a "hot"
variant whose pokemon-net second layer is scaled by 12, so that many bench bytes are above 127 (the split MFMAs and the saturation
correction run).  Wall time per oakgpu_leaf_eval_dev call (median of 30), then the same calls once under
`rocprofv3 --kernel-trace --stats` for the kernel split, and a roofline of k_mainnet_i8 against the i8 MFMA peak and HBM.
Writes profiles/r06_discrete_leaf.json.

usage: python tools/discrete_leaf_bench.py            (driver: timing, then the traced child, then the JSON)
       python tools/discrete_leaf_bench.py --child    (one pass of each configuration; what rocprofv3 traces)"""
import csv
import ctypes as C
import glob
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oak_amd import _lib  # noqa: E402
from oak_amd.engine import Context, Network  # noqa: E402

N = 65536
REPS = 30
I8_PEAK_OPS = 5.0e15   # 2 x the bf16 dense peak (an i8 32x32x32 MFMA takes the cycles of the bf16 32x32x16)
HBM_BPS = 6.3e12       # achievable HBM3E bandwidth (float4 copy)
OUT = os.path.join(ROOT, "profiles", "r06_discrete_leaf.json")
TMP = os.environ.get("TMPDIR", "/tmp")


def rewrite(src, dst, edit):
    raw = open(src, "rb").read()
    out, off = [bytes([1]) + raw[1:8]], 8
    for i in range(12):
        n_in, n_out = struct.unpack_from("<II", raw, off)
        off += 8
        b = np.frombuffer(raw, "<f4", n_out, off).copy()
        off += 4 * n_out
        W = np.frombuffer(raw, "<f4", n_out * n_in, off).copy().reshape(n_out, n_in)
        off += 4 * n_out * n_in
        b, W = edit(i, b, W)
        out += [struct.pack("<II", n_in, n_out), np.asarray(b, "<f4").tobytes(), np.asarray(W, "<f4").tobytes()]
    open(dst, "wb").write(b"".join(out))
    return dst


def spread(i, b, W):
    if i < 4:
        return b, W
    return (b / np.abs(b).max() * np.float32(0.6)).astype(np.float32), (W / np.abs(W).max() * np.float32(1.9)).astype(np.float32)


def nets():
    src = os.path.join(ROOT, "tests", "golden", "net_default.battle.net")
    normal = rewrite(src, os.path.join(TMP, "discrete_bench.battle.net"), spread)
    hot = rewrite(src, os.path.join(TMP, "discrete_bench_hot.battle.net"),
                  lambda i, b, W: (b * np.float32(12), W * np.float32(12)) if i == 1 else spread(i, b, W))
    return normal, hot


def setup():
    ctx = Context(0)
    ctx.ensure_ou_pools()
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    T = lambda *s, dt=torch.uint8: torch.empty(s, dtype=dt, device=dev)  # noqa: E731
    battles, durations, prng, rin, rout, mid, dmid = T(N, 384), T(N, 8), T(N, 8), T(N), T(N), T(N, 384), T(N, 8)
    steps, values = T(N, dt=torch.int32), T(N, dt=torch.float32)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lib, h = ctx.lib, ctx.handle
    _lib.check(lib.oakgpu_random_ou_battles_dev(h, C.c_uint64(0x0D15C8E7E), N, P(battles), P(durations), P(prng), P(rin)))
    _lib.check(lib.oakgpu_rollout_dev(h, P(battles), P(durations), P(rin), P(prng), N, 20, 0, P(rout), P(steps), P(values), P(mid), P(dmid)))
    torch.cuda.synchronize()
    return ctx, P, mid, dmid, values, T


def configs(ctx):
    normal, hot = nets()
    return [("fp32_pair", Network(ctx, path=normal)), ("discrete", Network(ctx, path=normal, discrete=True)),
            ("discrete_hot", Network(ctx, path=hot, discrete=True))]


def call(ctx, P, net, mid, dmid, values):
    _lib.check(ctx.lib.oakgpu_leaf_eval_dev(ctx.handle, net.handle, P(mid), P(dmid), N, P(values), None))


def child():
    ctx, P, mid, dmid, values, _ = setup()
    for _, net in configs(ctx):
        for _ in range(5):
            call(ctx, P, net, mid, dmid, values)
        torch.cuda.synchronize()


def timed(ctx, P, net, mid, dmid, values):
    for _ in range(5):
        call(ctx, P, net, mid, dmid, values)
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(ctx, P, net, mid, dmid, values)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def kernel_split():
    d = os.path.join(TMP, "discrete_leaf_prof")
    shutil.rmtree(d, ignore_errors=True)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                        sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        return {"error": "rocprofv3 rc %d" % r.returncode, "tail": (r.stdout + r.stderr)[-2000:]}
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda x: int(x["Start_Timestamp"]))
    # the child runs 5 calls of each configuration in order: fp32_pair, discrete, discrete_hot; the leaf kernels of each call are
    # the embedding launch and the main-net launch, so the trace splits into three equal runs of the leaf kernels
    leaf = [r for r in rows if any(k in r["Kernel_Name"] for k in ("k_embed", "k_mainnet", "k_party"))]
    per = len(leaf) // 3
    out = {}
    for c, name in enumerate(("fp32_pair", "discrete", "discrete_hot")):
        agg = {}
        for r in leaf[c * per:(c + 1) * per]:
            k = r["Kernel_Name"].split("(")[0]
            agg.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        out[name] = {k: {"calls": len(v), "avg_us": round(float(np.mean(v)), 2)} for k, v in agg.items()}
    return out


def main():
    ctx, P, mid, dmid, values, T = setup()
    res = {"leaves": N, "reps": REPS, "net": "768-64-64-32, policy 64 (clamp header, main-net weights over (-1.9, 1.9))", "wall_us": {}}
    for name, net in configs(ctx):
        med, best = timed(ctx, P, net, mid, dmid, values)
        res["wall_us"][name] = {"median": round(med, 2), "min": round(best, 2)}
        print(name, res["wall_us"][name], flush=True)
    split = kernel_split()
    res["kernels"] = split
    ops = 2 * (768 * 64 + 64 * 64 + 64 * 32 + 32) * N
    bytes_min = N * 768 * 4 + N * 4   # the fp32 embedding in, the value out
    res["roofline_k_mainnet_i8"] = {"int_ops": ops, "ops_floor_us": round(ops / I8_PEAK_OPS * 1e6, 3),
                                    "hbm_bytes": bytes_min, "hbm_floor_us": round(bytes_min / HBM_BPS * 1e6, 2)}
    for name in ("discrete", "discrete_hot"):
        k = split.get(name, {}) if isinstance(split, dict) else {}
        for kn, v in k.items():
            if "k_mainnet_i8" in kn:
                res["roofline_k_mainnet_i8"][name + "_us"] = v["avg_us"]
                res["roofline_k_mainnet_i8"][name + "_of_i8_peak"] = round(ops / (v["avg_us"] * 1e-6) / I8_PEAK_OPS, 5)
                res["roofline_k_mainnet_i8"][name + "_of_hbm"] = round(bytes_min / (v["avg_us"] * 1e-6) / HBM_BPS, 3)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
