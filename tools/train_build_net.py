"""Train a team-building network on `.build.data` trajectories on the GPU: build.py's loop (src/oak/build.py:281-342) over
oak_amd.build.TrajectoryCorpus.sample, oak_amd.build.targets and oak_amd.build.Trainer -- sampling, decoding, forward, GAE, loss, gradients,
Adam and the rolling average all on the device (include/oakgpu.h: "Reading `.build.data` back", "Training the build network").  The network
is the three-layer `.build.net` this project's rollout reads, not build.py's two-layer EmbeddingNets.

  python tools/train_build_net.py --data-dir DIR --batch-size N --lr LR --trajectories-per-step N --keep-prob P [--network-path X |
         --policy-hidden-dim H --value-hidden-dim H] [--dir OUT] [--steps N] [--checkpoint N] [--lr-decay F] [--lr-decay-start N]
         [--lr-decay-interval N] [--value-weight W] [--policy-loss-weight W] [--value-loss-weight W] [--entropy-loss-weight W] [--gamma G]
         [--lam L] [--avg-gamma G] [--clip-eps E] [--print-window N] [--seed N]

The options carry build.py's names and defaults (--clip-eps is accepted and unused, as it is there: the ratio is commented out).  --data-dir
is scanned recursively for `*.build.data` files, which are uploaded once.  Writes OUT/initial.build.net, and OUT/{step}.build.net and
OUT/{step}.avg.build.net every --checkpoint steps; prints one JSON line per --print-window steps (the only read of the trainer that waits)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", default=".")
    ap.add_argument("--dir")
    ap.add_argument("--network-path")
    ap.add_argument("--batch-size", type=int, required=True)
    ap.add_argument("--lr", type=float, required=True)
    ap.add_argument("--lr-decay", type=float, default=1.0)
    ap.add_argument("--lr-decay-start", type=int, default=0)
    ap.add_argument("--lr-decay-interval", type=int, default=1)
    ap.add_argument("--steps", type=int, default=-1)
    ap.add_argument("--checkpoint", type=int, default=50)
    ap.add_argument("--seed", type=int)
    ap.add_argument("--avg-gamma", type=float, default=0.995)
    ap.add_argument("--trajectories-per-step", type=int, required=True)
    ap.add_argument("--keep-prob", type=float, required=True)
    ap.add_argument("--value-weight", type=float, default=1.0)
    ap.add_argument("--policy-loss-weight", type=float, default=1.0)
    ap.add_argument("--value-loss-weight", type=float, default=0.5)
    ap.add_argument("--entropy-loss-weight", type=float, default=0.01)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.90)
    ap.add_argument("--clip-eps", type=float, default=0.10, help="accepted and unused, as in build.py")
    ap.add_argument("--policy-hidden-dim", type=int, default=128)
    ap.add_argument("--value-hidden-dim", type=int, default=128)
    ap.add_argument("--print-window", type=int, default=5)
    a = ap.parse_args(argv)
    import torch
    from oak_amd import build, netfile
    from oak_amd.engine import Context

    paths = sorted(os.path.join(d, f) for d, _, files in os.walk(a.data_dir) for f in files if f.endswith(".build.data"))
    if not paths:
        print(json.dumps({"error": "no .build.data files under %s" % a.data_dir}))
        return 2
    out_dir = a.dir or time.strftime("build-%Y-%m-%d-%H:%M:%S")
    os.makedirs(out_dir, exist_ok=True)
    initial = os.path.join(out_dir, "initial.build.net")
    if a.network_path:
        with open(a.network_path, "rb") as f:
            data = f.read()
        with open(initial, "wb") as f:
            f.write(data)
    else:
        netfile.write_random_build_net(initial, a.seed if a.seed is not None else 7, policy_hidden=a.policy_hidden_dim, value_hidden=a.value_hidden_dim)
    device = torch.device("cuda:0")
    torch.zeros(1, device=device)                                        # (torch initialises the GPU before the library does)
    if a.seed is not None:
        torch.manual_seed(a.seed)
    ctx = Context(0)
    corpus = build.TrajectoryCorpus(ctx, paths)
    trainer = build.Trainer(ctx, initial, a.trajectories_per_step)
    seed0 = a.seed if a.seed is not None else int(time.time())
    hyper = dict(gamma=a.gamma, lam=a.lam, policy_loss_weight=a.policy_loss_weight, value_loss_weight=a.value_loss_weight, entropy_loss_weight=a.entropy_loss_weight)
    lr, step, chunks, rows, t0 = a.lr, 0, 0, 0, time.perf_counter()
    print(json.dumps({"files": len(paths), "corpus": corpus.info(), "parameters": trainer.count, "dir": out_dir}), flush=True)
    while a.steps < 0 or step < a.steps:
        try:                                                             # build.py:295-332: backward() per chunk until the batch is full
            chunks, rows = build.accumulate_batch(ctx, corpus, trainer, a.batch_size, a.trajectories_per_step, a.keep_prob, a.value_weight, seed0, chunks, rows,
                                                  device, hyper)
        except build.NoValidStep as e:
            print(json.dumps({"error": str(e)}))
            return 2
        trainer.adam(lr)
        # save_and_decay (src/oak/common_args.py:134-153), then the rolling average and its checkpoint
        if step >= a.lr_decay_start and step % a.lr_decay_interval == 0:
            lr *= a.lr_decay
        if (step + 1) % a.checkpoint == 0:
            trainer.save(os.path.join(out_dir, "%d.build.net" % (step + 1)))
        trainer.average(a.avg_gamma)
        if (step + 1) % a.checkpoint == 0:
            trainer.save(os.path.join(out_dir, "%d.avg.build.net" % (step + 1)), "average")
        if (step + 1) % a.print_window == 0 or step + 1 == a.steps:
            rep = trainer.report()                                       # (of the step's last chunk)
            rep.update(step=step + 1, lr=lr, chunks=chunks, rows_per_s=rows / (time.perf_counter() - t0))
            print(json.dumps(rep), flush=True)
        step += 1
    trainer.close()
    corpus.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
