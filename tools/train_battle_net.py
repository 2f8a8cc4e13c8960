"""Train a battle network on `.battle.data` games on the GPU: battle.py's loop (src/oak/battle.py) over oak_amd.train.FrameCorpus.sample
and oak_amd.train.Trainer.step -- sampling, replay, encoding, forward, loss, gradients and Adam all on the device (include/oakgpu.h:
"Training batches", "Training the battle network").

  python tools/train_battle_net.py --data-dir DIR --batch-size N --lr LR [--network-path X | widths] [--dir OUT] [--steps N]
         [--checkpoint N] [--lr-decay F] [--lr-decay-start N] [--lr-decay-interval N] [--value-nash-weight W] [--value-empirical-weight W]
         [--value-score-weight W] [--p-nash-weight W] [--policy-loss-weight W] [--no-value-loss] [--no-policy-loss] [--clamp-parameters]
         [--discrete] [--no-apply-symmetries] [--max-battle-length N] [--min-iterations N] [--print-window N] [--seed N]

The options carry battle.py's names and defaults.  --data-dir is scanned recursively for `*.battle.data` files, which are uploaded once.
Without --network-path a network of the given widths is drawn with the reference's initialiser.  Writes OUT/initial.battle.net and
OUT/{step}.battle.net every --checkpoint steps; prints one JSON line per --print-window steps (the only reads that wait for the device)."""
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
    ap.add_argument("--max-battle-length", type=int, default=10000)
    ap.add_argument("--min-iterations", type=int, default=1)
    ap.add_argument("--discrete", action="store_true")
    ap.add_argument("--clamp-parameters", action="store_true")
    ap.add_argument("--value-nash-weight", type=float, default=0.0)
    ap.add_argument("--value-empirical-weight", type=float, default=0.0)
    ap.add_argument("--value-score-weight", type=float, default=1.0)
    ap.add_argument("--p-nash-weight", type=float, default=0.0)
    ap.add_argument("--policy-loss-weight", type=float, default=1.0)
    ap.add_argument("--no-value-loss", action="store_true")
    ap.add_argument("--no-policy-loss", action="store_true")
    ap.add_argument("--no-apply-symmetries", action="store_true", help="Whether to skip permuting Bench/Sides")
    ap.add_argument("--print-window", type=int, default=5)
    for name, default in (("pokemon-hidden", 128), ("pokemon-out", 59), ("active-hidden", 128), ("active-out", 83), ("hidden", 64),
                          ("value-hidden", 32), ("policy-hidden", 64)):
        ap.add_argument("--%s-dim" % name, type=int, default=default)
    a = ap.parse_args(argv)
    from oak_amd import netfile
    from oak_amd.engine import Context
    from oak_amd.train import EncodedBattleFrames, FrameCorpus, Trainer, apply_symmetries, train_loss

    paths = sorted(os.path.join(d, f) for d, _, files in os.walk(a.data_dir) for f in files if f.endswith(".battle.data"))
    if not paths:
        print(json.dumps({"error": "no .battle.data files under %s" % a.data_dir}))
        return 2
    out_dir = a.dir or time.strftime("%Y-%m-%d-%H-%M-%S")
    os.makedirs(out_dir, exist_ok=True)
    initial = os.path.join(out_dir, "initial.battle.net")
    if a.network_path:
        with open(a.network_path, "rb") as f:
            data = f.read()
        with open(initial, "wb") as f:
            f.write(data)
    else:
        netfile.write_random_net(initial, seed=a.seed if a.seed is not None else 7, activation=2 if a.discrete else 1, pokemon_hidden=a.pokemon_hidden_dim,
                                 pokemon_out=a.pokemon_out_dim, active_hidden=a.active_hidden_dim, active_out=a.active_out_dim, hidden=a.hidden_dim,
                                 value_hidden=a.value_hidden_dim, policy_hidden=a.policy_hidden_dim)
    loss = train_loss(a.value_nash_weight, a.value_empirical_weight, a.value_score_weight, a.p_nash_weight, 0.0 if a.no_value_loss else 1.0,
                      0.0 if a.no_policy_loss else a.policy_loss_weight)
    enc = EncodedBattleFrames(a.batch_size, "cuda:0")                    # (torch initialises the GPU before the library does)
    ctx = Context(0)
    corpus = FrameCorpus(ctx, paths)
    trainer = Trainer(ctx, initial, a.batch_size)
    seed0 = a.seed if a.seed is not None else int(time.time())
    clamp = a.discrete or a.clamp_parameters
    lr, step, t0 = a.lr, 0, time.perf_counter()
    print(json.dumps({"files": len(paths), "corpus": corpus.info(), "parameters": trainer.count, "dir": out_dir}), flush=True)
    while a.steps < 0 or step < a.steps:
        lib_seed = (seed0 + step * a.batch_size) & (2 ** 64 - 1)          # draw i of a step is seeded seed + i: no stream is used twice
        corpus.sample(enc, lib_seed, a.max_battle_length, a.min_iterations, count_ok=False)
        if not a.no_apply_symmetries:
            apply_symmetries(ctx, enc, lib_seed)
        trainer.step(enc, a.batch_size, loss, lr, clamp_parameters=clamp)
        # save_and_decay (src/oak/common_args.py:134-153)
        if step >= a.lr_decay_start and step % a.lr_decay_interval == 0:
            lr *= a.lr_decay
        if (step + 1) % a.checkpoint == 0:
            trainer.save(os.path.join(out_dir, "%d.battle.net" % (step + 1)))
        if (step + 1) % a.print_window == 0 or step + 1 == a.steps:
            rep = trainer.report()
            rep.update(step=step + 1, lr=lr, rows_per_s=(step + 1) * a.batch_size / (time.perf_counter() - t0))
            print(json.dumps(rep), flush=True)
        step += 1
    trainer.close()
    corpus.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
