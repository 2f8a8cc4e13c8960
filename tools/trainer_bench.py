"""Time the trainer's optimiser step (oak_amd.train.Trainer.step: k_gemm, k_loss, k_adam, ... of oak_amd/csrc/trainer.hip) on an MI355X
against the same step as plain torch-ROCm autograd + torch.optim.Adam in fp32 on the same device -- the referee module of
tests/trainer_ref.py moved to the GPU, fed the same device tensors -- and the end-to-end loop (sample + symmetries + step) in rows/s.

Corpus: tools/replay_bench.py's seeded random-play corpus played on the device (its records carry no search targets: the policies are
zero, which changes no launch and no operand shape).  Per network (`default`, `256`: tests/golden) and batch size (4,096 and 65,536 rows):
HIP-event time of one step after warm-up, fused and baseline alternated inside every round, medians over --repeats rounds; then --loop
steps of sample + symmetries + step timed as a whole.

  python tools/trainer_bench.py [--games 512] [--repeats 3] [--loop 10] [--batches 4096,65536] [--nets default,256] [--out profiles/r24_trainer.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOSS = (0.0, 0.5, 0.5, 0.5, 1.0, 1.0)


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    med = float(np.median(ms))
    return {"ms": [float(x) for x in ms], "median_ms": med, "spread_pct": 100 * (max(ms) - min(ms)) / med}


def flops_per_row(dims):
    """Forward + backward multiply-adds x 2 of the dense layers per batch row (the embedding nets run 10 and 2 rows per batch row; the
    first layers have no input gradient; fc3 of the policy heads counted dense, as the backward runs it)."""
    total = 0
    for i, (n_in, n_out) in enumerate(dims):
        rows = 10 if i < 2 else 2 if i < 4 else 1
        passes = 2 if i in (0, 2) else 3
        total += 2 * rows * passes * n_in * n_out
    return total


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop", type=int, default=10)
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--nets", default="default,256")
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.cuda.init()   # torch initialises the GPU before the library does
    from oak_amd.engine import Context
    from oak_amd.train import EncodedBattleFrames, FrameCorpus, Trainer, apply_symmetries, train_loss
    import policy_ref as P
    import replay_bench as RB
    import trainer_ref as TR
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    first, results, frames, lengths = RB.play_corpus(ctx, a.games)
    buf, _ = RB.assemble(first, results, frames, lengths)
    corpus = FrameCorpus(ctx, buf.tobytes())
    stream = torch.cuda.ExternalStream(ctx.lib.oakgpu_get_stream(ctx.handle))
    loss = train_loss(*LOSS)
    res = {"corpus": corpus.info(), "loss": LOSS, "repeats": a.repeats, "loop_steps": a.loop,
           "timing": "HIP events on the context's stream around one step, one warm-up round, fused and baseline alternated inside every round",
           "baseline": "tests/trainer_ref.Ref in fp32 on the device: torch autograd + torch.optim.Adam on the same device tensors", "cases": []}
    for tag in a.nets.split(","):
        data = open(P.GOLDEN[tag], "rb").read()
        for n in (int(x) for x in a.batches.split(",")):
            enc = EncodedBattleFrames(n, dev)
            assert corpus.sample(enc, 1, 0, 0) == n
            trainer = Trainer(ctx, data, n)
            ref = TR.Ref(data, torch.float32).to(dev)
            ref.keep = False
            opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
            idx, k = enc.choice_indices, enc.k.to(torch.int64).reshape(n, 2)

            def baseline():
                with torch.cuda.stream(stream):
                    opt.zero_grad(set_to_none=True)
                    total, _ = ref.loss_of(enc.pokemon, enc.active, enc.hp, idx, k, enc.empirical_policies, enc.nash_policies, enc.empirical_value[:, 0],
                                           enc.nash_value[:, 0], enc.score[:, 0], float(n), LOSS)
                    total.backward()
                    opt.step()

            def fused():
                trainer.step(enc, n, loss, 1e-3)

            ms = {"fused": [], "baseline": []}
            for rep in range(a.repeats + 1):                          # round 0 is warm-up
                for name, fn in (("fused", fused), ("baseline", baseline)):
                    t = timed(stream, fn)
                    if rep:
                        ms[name].append(t)
            f, b = stats(ms["fused"]), stats(ms["baseline"])

            def loop():
                for step in range(a.loop):
                    corpus.sample(enc, 1000 + step * n, 0, 0, count_ok=False)
                    apply_symmetries(ctx, enc, 1000 + step * n)
                    trainer.step(enc, n, loss, 1e-3)
            loop()
            torch.cuda.synchronize()
            loop_ms = timed(stream, loop)
            rep_ = trainer.report()
            gf = flops_per_row(trainer.dims) * n / 1e9
            res["cases"].append({"net": tag, "rows": n, "gflop_per_step": gf, "fused": f, "baseline": b, "baseline_over_fused": b["median_ms"] / f["median_ms"],
                                 "fused_tflops": gf / f["median_ms"], "loop_ms_per_step": loop_ms / a.loop, "loop_rows_per_s": n * a.loop / (loop_ms * 1e-3),
                                 "last_report": rep_})
            print(json.dumps(res["cases"][-1]), flush=True)
            trainer.close()
            del ref, opt, enc
            torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
