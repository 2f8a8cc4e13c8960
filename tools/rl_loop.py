"""The battle network's reinforcement loop on one device (oak_amd/rl.py; the reference's src/oak/rl.py without a file between its stages):
self-play on the forest search -> a replay window on the device -> sample, symmetries, optimiser step -> the new evaluator.

  python tools/rl_loop.py --dir runs/a --network-path tests/golden/net_tiny.battle.net --rounds 3 --games 64 --budget 8 --steps 2 \\
         --batch-size 256 --lr 1e-3 --data-window 96 --checkpoint 2 --seed 1

One JSON line per round: games, frames, window records, evicted, the last step's losses, and wall time split into generate / append / train.
--dir receives `{step}.battle.net` every --checkpoint steps and `final.battle.net`.  The arguments carry the reference's names where it has
them (src/oak/rl.py, src/oak/common_args.py); --data-window counts RECORDS here (files there), --min-records stands for --min-files, and the
rounds alternate: there is no concurrent generate, no --sleep and one GPU.
  --build-network-path X.build.net with --team-modify-prob > 0 turns the build network's side on (the reference's use_build): both seats'
                    teams are built, games with a built seat are skipped with --battle-skip-prob (searched once with --t1-budget iterations
                    for their matchup value), the seats' records go to a build window of --build-data-window records, and --build-steps
                    build steps follow each round under the --build-* options (tools/train_build_net.py's names).  --dir also receives
                    `{step}.build.net` and `final.build.net`.
  --save-data DIR   each round's records as DIR/{round}.battle.data
  --gate-games N    after each round that trained, N matches (both seatings) of the new network against the one before it (arena.match)
  --eval fp | mc    self-play with the PokeEngine evaluator or Monte-Carlo leaves instead of the network being trained (then --bandit ucb-C)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", required=True)
    ap.add_argument("--network-path", required=True)
    ap.add_argument("--teams", default=os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json"))
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--games", type=int, default=4096, help="self-play games per round")
    ap.add_argument("--steps", type=int, default=16, help="optimiser steps per round")
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--fast-budget", type=int, default=0)
    ap.add_argument("--fast-search-prob", type=float, default=0.0)
    ap.add_argument("--bandit", default="pucb-1.0")
    ap.add_argument("--eval", default="", help="\"\" = the network being trained; fp = PokeEngine; mc = Monte Carlo")
    ap.add_argument("--policy-mode", default="e")
    ap.add_argument("--fast-policy-mode", default="")
    ap.add_argument("--policy-temp", type=float, default=1.0)
    ap.add_argument("--policy-min", type=float, default=0.0)
    ap.add_argument("--max-battle-length", type=int, default=0)
    ap.add_argument("--batch-size", type=int, required=True)
    ap.add_argument("--lr", type=float, required=True)
    ap.add_argument("--lr-decay", type=float, default=1.0)
    ap.add_argument("--lr-decay-start", type=int, default=0)
    ap.add_argument("--lr-decay-interval", type=int, default=1)
    ap.add_argument("--value-nash-weight", type=float, default=0.0)
    ap.add_argument("--value-empirical-weight", type=float, default=0.0)
    ap.add_argument("--value-score-weight", type=float, default=1.0)
    ap.add_argument("--p-nash-weight", type=float, default=0.0)
    ap.add_argument("--policy-loss-weight", type=float, default=1.0)
    ap.add_argument("--data-window", type=int, default=65536, help="records the window keeps")
    ap.add_argument("--window-mb", type=float, default=1024.0, help="bytes the window keeps")
    ap.add_argument("--min-records", type=int, default=1, help="records the window must hold before training starts")
    ap.add_argument("--checkpoint", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--discrete", action="store_true")
    ap.add_argument("--clamp-parameters", action="store_true")
    ap.add_argument("--no-apply-symmetries", action="store_true")
    ap.add_argument("--save-data")
    ap.add_argument("--gate-games", type=int, default=0)
    ap.add_argument("--build-network-path", default="")
    ap.add_argument("--team-modify-prob", type=float, default=0.0)
    ap.add_argument("--pokemon-delete-prob", type=float, default=0.0)
    ap.add_argument("--move-delete-prob", type=float, default=0.0)
    ap.add_argument("--max-pokemon", type=int, default=6)
    ap.add_argument("--battle-skip-prob", type=float, default=0.0)
    ap.add_argument("--t1-budget", type=int, default=0)
    ap.add_argument("--build-data-window", type=int, default=65536, help="records the build window keeps")
    ap.add_argument("--build-steps", type=int, default=1, help="build optimiser steps per round")
    ap.add_argument("--build-batch-size", type=int, default=0)
    ap.add_argument("--build-lr", type=float, default=0.0)
    ap.add_argument("--build-lr-decay", type=float, default=1.0)
    ap.add_argument("--build-lr-decay-start", type=int, default=0)
    ap.add_argument("--build-lr-decay-interval", type=int, default=1)
    ap.add_argument("--build-trajectories-per-step", type=int, default=0)
    ap.add_argument("--build-keep-prob", type=float, default=1.0)
    ap.add_argument("--build-value-weight", type=float, default=1.0)
    ap.add_argument("--build-policy-loss-weight", type=float, default=1.0)
    ap.add_argument("--build-value-loss-weight", type=float, default=0.5)
    ap.add_argument("--build-entropy-loss-weight", type=float, default=0.01)
    ap.add_argument("--build-gamma", type=float, default=0.99)
    ap.add_argument("--build-lam", type=float, default=0.90)
    ap.add_argument("--build-avg-gamma", type=float, default=0.995)
    a = ap.parse_args(argv)
    import torch
    torch.zeros(1, device="cuda:0")                                      # (torch initialises the GPU before the library does)
    from oak_amd import rl
    from oak_amd.engine import Context
    from oak_amd.train import train_loss
    from policy_match import team_bytes
    with open(a.network_path, "rb") as f:
        net = f.read()
    os.makedirs(a.dir, exist_ok=True)
    ctx = Context(0)
    loss = train_loss(a.value_nash_weight, a.value_empirical_weight, a.value_score_weight, a.p_nash_weight, 1.0, a.policy_loss_weight)
    evaluator = {"": None, "fp": "poke-engine", "mc": "mc"}[a.eval]
    build_kw = {}
    if a.build_network_path:
        with open(a.build_network_path, "rb") as f:
            build_kw = dict(build_net_bytes=f.read(), team_modify_prob=a.team_modify_prob, pokemon_delete_prob=a.pokemon_delete_prob,
                            move_delete_prob=a.move_delete_prob, max_pokemon=a.max_pokemon, battle_skip_prob=a.battle_skip_prob, t1_budget=a.t1_budget,
                            build_data_window=a.build_data_window, build_steps=a.build_steps, build_batch_size=a.build_batch_size, build_lr=a.build_lr,
                            build_lr_decay=a.build_lr_decay, build_lr_decay_start=a.build_lr_decay_start, build_lr_decay_interval=a.build_lr_decay_interval,
                            build_trajectories_per_step=a.build_trajectories_per_step, build_keep_prob=a.build_keep_prob, build_value_weight=a.build_value_weight,
                            build_policy_loss_weight=a.build_policy_loss_weight, build_value_loss_weight=a.build_value_loss_weight,
                            build_entropy_loss_weight=a.build_entropy_loss_weight, build_gamma=a.build_gamma, build_lam=a.build_lam,
                            build_avg_gamma=a.build_avg_gamma)
    res = rl.run(ctx, net, team_bytes(a.teams), a.rounds, a.games, a.budget, a.steps, a.batch_size, a.lr, a.data_window, max_bytes=int(a.window_mb * (1 << 20)),
                 min_records=a.min_records, bandit=a.bandit, policy_mode=a.policy_mode, fast_policy_mode=a.fast_policy_mode, policy_temp=a.policy_temp,
                 policy_min=a.policy_min, max_battle_length=a.max_battle_length, fast_budget=a.fast_budget, fast_search_prob=a.fast_search_prob,
                 lr_decay=a.lr_decay, lr_decay_start=a.lr_decay_start, lr_decay_interval=a.lr_decay_interval, loss=loss, checkpoint=a.checkpoint, seed=a.seed,
                 discrete=a.discrete, clamp_parameters=a.clamp_parameters, apply_symmetry=not a.no_apply_symmetries, out_dir=a.dir, save_data=a.save_data,
                 gate_games=a.gate_games, evaluator=evaluator, log=rl.print_json, **build_kw)
    with open(os.path.join(a.dir, "final.battle.net"), "wb") as f:
        f.write(res["net"])
    summary = {"window": res["window"], "checkpoints": sorted(res["checkpoints"]), "dir": a.dir}
    if "build_net" in res:
        with open(os.path.join(a.dir, "final.build.net"), "wb") as f:
            f.write(res["build_net"])
        summary.update(build_window=res["build_window"], build_checkpoints=sorted(res["build_checkpoints"]))
    print(json.dumps(summary), flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
