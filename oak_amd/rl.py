"""The reference's reinforcement loop for the battle network (src/oak/rl.py: generate and battle.py side by side on one directory) on one
device, with no file between its stages: self-play on a reused forest -> ReplayWindow.append on the device -> sample -> apply_symmetries
-> Trainer.step -> the evaluator replaced from the trainer's parameters (oakgpu_net_load_memory).  tools/rl_loop.py is its command line.

A round:
  1. `games` self-play games with the current evaluator (forest_selfplay on torch tensors: the records stay on the device);
  2. window.append(stream, offsets): the append's one wait and one small read;
  3. once the window holds min_records records (the reference's --min-files), `steps` optimiser steps on batches drawn from the window with
     min_iterations = fast_budget + 1 (rl.py:279), so that only full searches are trained on;
  4. the evaluator is made again from trainer.net_bytes();
  5. every `checkpoint` steps the parameters are kept as `{step}.battle.net`.
The build network's side (rl.py:161-166's use_build: a build network and team_modify_prob > 0) rides along in the same round, as resident:
  1b. both seats' teams come from build.provide_pairs with the current build network, seeds from (seed, round) (build_round_games);
  1c. self-play gets the seats' built bits, battle_skip_prob and t1_budget: a game with a built seat may be searched once for its matchup
      value and not played (frames.forest_selfplay); a skipped game is a zero-byte slice, which the battle window's append passes over;
  2b. build.game_records -> BuildWindow.append on the device: both seats' records, value = the game's matchup, of the played and the
      skipped games;
  3b. once the build window holds a record, `build_steps` steps of build.accumulate_batch + adam + the rolling average
      (tools/train_build_net.py's step); the keep mask draws from a torch.Generator seeded from (seed, step);
  4b. the build network is made again from its trainer's bytes; 5b. `{step}.build.net` beside the battle checkpoints.
Departures from the reference, which runs its two halves concurrently as processes: the rounds alternate (no generate || train), the windows
are counted in records rather than files (--data-window, --build-data-window) and there is no --sleep.

Every seed is derived from `seed` by round and step (round_games, sample_seed), so a run is a function of its arguments."""
import json
import os
import time

import numpy as np

from .train import EncodedBattleFrames, ReplayWindow, Trainer, apply_symmetries, train_loss

MASK = 2 ** 64 - 1


def round_games(pool, games, seed, rnd):
    """The games of round `rnd`: teams uint8[games, 60] drawn from pool (uint8 [T, 30]; a pair the endless battle check refuses is drawn
    again), battle seeds and policy seeds uint64[games] -- from a generator seeded with (seed, rnd) alone."""
    import ctypes as C
    from . import _lib
    lib = _lib.load()
    rng = np.random.default_rng([int(seed) & MASK, int(rnd)])
    pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1, 30)
    teams = np.zeros((games, 60), np.uint8)
    for g in range(games):
        while True:
            i, j = rng.integers(0, len(pool), 2)
            pair = np.ascontiguousarray(np.concatenate([pool[i], pool[j]]))
            if not lib.oakgpu_endless_battle_check(pair.ctypes.data_as(C.c_void_p)):
                break
        teams[g] = pair
    return teams, rng.integers(0, 1 << 63, games, dtype=np.uint64), rng.integers(0, 1 << 63, games, dtype=np.uint64)


def build_round_games(ctx, build_net, pool, games, seed, rnd, **provide_kw):
    """Round rnd's games with the build side: (teams uint8[games, 60], (p1, p2) provide's dict per seat, battle seeds, policy seeds), all
    from a generator seeded with (seed, rnd, 1) alone -- build.provide_pairs draws a refused pair again from the seeds' own successors."""
    from . import build
    rng = np.random.default_rng([int(seed) & MASK, int(rnd), 1])
    provide_seeds = rng.integers(0, 1 << 63, (games, 2), dtype=np.uint64)
    teams, seats = build.provide_pairs(ctx, build_net, np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1, 30), provide_seeds, **provide_kw)
    return teams, seats, rng.integers(0, 1 << 63, games, dtype=np.uint64), rng.integers(0, 1 << 63, games, dtype=np.uint64)


def build_step_seed(seed, step):
    """The seed of build step `step`'s keep mask (a torch.Generator's)."""
    return ((int(seed) & MASK) * 0xD1342543DE82EF95 + int(step) + 1) & (2 ** 63 - 1)


def sample_seed(seed, step, batch_size):
    """The seed of step `step`'s draws and symmetries: row i of a step uses stream seed + i, so steps are batch_size apart."""
    return ((int(seed) & MASK) * 0x9E3779B97F4A7C15 + int(step) * int(batch_size)) & MASK


def parse_bandit(text):
    """"ucb-2.0" / "pucb-1.0" -> (name, c)"""
    name, _, c = text.partition("-")
    if name not in ("ucb", "pucb"):
        raise ValueError("--bandit: ucb-C or pucb-C (the forest search's bandits)")
    return name, float(c) if c else 2.0


def selfplay_round(ctx, forest, evaluator, pool, games, seed, rnd, budget, bandit="pucb-1.0", policy_mode="e", policy_temp=1.0, policy_min=0.0,
                   max_battle_length=0, fast_budget=0, fast_search_prob=0.0, fast_policy_mode="", device="cuda:0", drawn=None, built=None,
                   battle_skip_prob=0.0, t1_budget=0, stats=None):
    """Round rnd's self-play call on device tensors: forest_selfplay's five tensors.  drawn: the round's (teams, battle seeds, seeds) when
    the build side made them (built: its uint8[games] bits; stats then receives the games' matchup tensor), else round_games draws them."""
    import torch
    from .frames import forest_selfplay
    name, c = parse_bandit(bandit)
    teams, battle_seeds, seeds = round_games(pool, games, seed, rnd) if drawn is None else drawn
    dev = torch.device(device)
    if built is not None:
        return forest_selfplay(ctx, torch.from_numpy(teams).to(dev), torch.from_numpy(battle_seeds.view(np.int64)).to(dev),
                               torch.from_numpy(seeds.view(np.int64)).to(dev), budget, c=c, bandit=name, evaluator=evaluator, policy_mode=policy_mode,
                               policy_temp=policy_temp, policy_min=policy_min, max_battle_length=max_battle_length, forest=forest, solve_nash="device",
                               fast_budget=fast_budget, fast_search_prob=fast_search_prob, fast_policy_mode=fast_policy_mode, stats=stats,
                               built=torch.from_numpy(np.ascontiguousarray(built, np.uint8)).to(dev), battle_skip_prob=battle_skip_prob, t1_budget=t1_budget)
    return forest_selfplay(ctx, torch.from_numpy(teams).to(dev), torch.from_numpy(battle_seeds.view(np.int64)).to(dev),
                           torch.from_numpy(seeds.view(np.int64)).to(dev), budget, c=c, bandit=name, evaluator=evaluator, policy_mode=policy_mode,
                           policy_temp=policy_temp, policy_min=policy_min, max_battle_length=max_battle_length, forest=forest, solve_nash="device",
                           fast_budget=fast_budget, fast_search_prob=fast_search_prob, fast_policy_mode=fast_policy_mode)


def run(ctx, net_bytes, pool, rounds, games, budget, steps, batch_size, lr, data_window, max_bytes=1 << 30, min_records=1, bandit="pucb-1.0",
        policy_mode="e", fast_policy_mode="", policy_temp=1.0, policy_min=0.0, max_battle_length=0, fast_budget=0, fast_search_prob=0.0,
        lr_decay=1.0, lr_decay_start=0, lr_decay_interval=1, loss=None, checkpoint=0, seed=0, discrete=False, clamp_parameters=False,
        apply_symmetry=True, out_dir=None, save_data=None, gate_games=0, evaluator=None, log=None, device="cuda:0", keep_records=False,
        build_net_bytes=None, team_modify_prob=0.0, pokemon_delete_prob=0.0, move_delete_prob=0.0, max_pokemon=6, battle_skip_prob=0.0, t1_budget=0,
        build_data_window=0, build_steps=1, build_batch_size=0, build_lr=0.0, build_lr_decay=1.0, build_lr_decay_start=0, build_lr_decay_interval=1,
        build_trajectories_per_step=0, build_keep_prob=1.0, build_value_weight=1.0, build_policy_loss_weight=1.0, build_value_loss_weight=0.5,
        build_entropy_loss_weight=0.01, build_gamma=0.99, build_lam=0.90, build_avg_gamma=0.995):
    """The loop.  net_bytes: the initial `.battle.net`; pool: uint8 [T, 6, 5] teams; evaluator: None (the network being trained, with
    PUCB or UCB) or "poke-engine" / "mc" for self-play that does not use it; log: a callable that receives each round's dict (tools/rl_loop.py
    prints it as JSON).  Returns {"net": the final parameters as `.battle.net` bytes, "checkpoints": {step: bytes}, "rounds": [dict],
    "window": the window's stats, and with keep_records "records": the window's bytes at the end}; with out_dir the checkpoints are also written
    there, with save_data each round's records.
    The build side (the module's 1b - 5b) is on when build_net_bytes is given and team_modify_prob > 0; it needs build_data_window,
    build_batch_size, build_lr and build_trajectories_per_step; the build_* names are the reference's --build-* options and
    tools/train_build_net.py's.  The result then also holds "build_net" (the final `.build.net` bytes), "build_avg_net", "build_checkpoints"
    {step: bytes}, "build_window" (its stats), and with keep_records "build_records" (the build window's bytes at the end) and
    "build_rounds": per round {"status", "results", "matchup", "built", "records"} -- the games' outputs and the round's build records as
    numpy arrays and bytes.  Without the build arguments the loop is the battle loop alone, byte for byte."""
    from .engine import Network
    from .search import Forest
    name, _ = parse_bandit(bandit)
    use_build = build_net_bytes is not None and team_modify_prob > 0
    if use_build and not (build_data_window > 0 and build_batch_size > 0 and build_trajectories_per_step > 0 and build_lr > 0):
        raise ValueError("rl.run: the build side needs build_data_window, build_batch_size, build_trajectories_per_step and build_lr")
    loss = train_loss() if loss is None else loss
    enc = EncodedBattleFrames(batch_size, device)
    window = ReplayWindow(ctx, data_window, max_bytes)
    trainer = Trainer(ctx, net_bytes, batch_size)
    forest = Forest(ctx, games, max(int(budget), int(fast_budget), int(t1_budget) if use_build else 0, 1), contextual=name == "pucb")
    current, previous = bytes(net_bytes), None
    bwindow = btrainer = generator = None
    build_current, build_checkpoints, build_rounds, bstep, bchunks, brows = None, {}, [], 0, 0, 0
    if use_build:
        import torch
        from . import build
        build_current = bytes(build_net_bytes)
        bwindow, btrainer = build.BuildWindow(ctx, build_data_window), build.Trainer(ctx, build_current, build_trajectories_per_step)
        generator = torch.Generator(device=torch.device(device))
        hyper = dict(gamma=build_gamma, lam=build_lam, policy_loss_weight=build_policy_loss_weight, value_loss_weight=build_value_loss_weight,
                     entropy_loss_weight=build_entropy_loss_weight)
    clamp = bool(discrete or clamp_parameters)
    checkpoints, history, step = {}, [], 0
    for d in (out_dir, save_data):
        if d:
            os.makedirs(d, exist_ok=True)
    try:
        for rnd in range(rounds):
            t0 = time.perf_counter()
            net = Network(ctx, data=current, discrete=discrete) if evaluator is None else None
            try:
                extra, sp_stats, seats = {}, {}, None
                if use_build:
                    with build.BuildNetwork(ctx, build_current) as bnet:
                        teams, seats, battle_seeds, seeds = build_round_games(ctx, bnet, pool, games, seed, rnd, max_pokemon=max_pokemon,
                                                                              pokemon_delete_prob=pokemon_delete_prob, move_delete_prob=move_delete_prob,
                                                                              team_modify_prob=team_modify_prob)
                    built = ((seats[0]["n_updates"] > 0) | ((seats[1]["n_updates"] > 0) << 1)).astype(np.uint8)
                    extra = dict(drawn=(teams, battle_seeds, seeds), built=built, battle_skip_prob=battle_skip_prob, t1_budget=t1_budget, stats=sp_stats)
                out = selfplay_round(ctx, forest, net if evaluator is None else evaluator, pool, games, seed, rnd, budget, bandit, policy_mode, policy_temp,
                                     policy_min, max_battle_length, fast_budget, fast_search_prob, fast_policy_mode, device, **extra)
                t1 = time.perf_counter()
                before = window.stats()
                st = window.append(out[0], out[1])
                t2 = time.perf_counter()
            finally:
                if net is not None:
                    net.close()
            if save_data:
                with open(os.path.join(save_data, "%d.battle.data" % rnd), "wb") as f:
                    f.write(bytes(out[0].cpu().numpy().tobytes()))
            trained = 0
            if st["records"] >= min_records:
                for _ in range(steps):
                    s = sample_seed(seed, step, batch_size)
                    window.sample(enc, s, max_battle_length, fast_budget + 1, count_ok=False)
                    if apply_symmetry:
                        apply_symmetries(ctx, enc, s)
                    trainer.step(enc, batch_size, loss, lr, clamp_parameters=clamp)
                    if step >= lr_decay_start and step % lr_decay_interval == 0:       # save_and_decay (src/oak/common_args.py:134-153)
                        lr *= lr_decay
                    step += 1
                    trained += 1
                    if checkpoint and step % checkpoint == 0:
                        checkpoints[step] = trainer.net_bytes()
                        if out_dir:
                            with open(os.path.join(out_dir, "%d.battle.net" % step), "wb") as f:
                                f.write(checkpoints[step])
            build_row = {}
            if use_build:
                tb = time.perf_counter()
                records, count = build.game_records(ctx, seats, out[4], out[3], sp_stats["matchup"])
                bbefore = bwindow.stats()
                bwindow.append(records, count)
                bst = bwindow.stats()
                tb1 = time.perf_counter()
                if keep_records:
                    build_rounds.append({"status": out[4].cpu().numpy(), "results": out[3].cpu().numpy(), "matchup": sp_stats["matchup"].cpu().numpy(), "built": built,
                                         "records": records.reshape(-1)[:int(count.item()) * build.RECORD_BYTES].cpu().numpy().tobytes()})
                btrained = 0
                if bst["records"] > 0:
                    for _ in range(build_steps):
                        generator.manual_seed(build_step_seed(seed, bstep))
                        bchunks, brows = build.accumulate_batch(ctx, bwindow, btrainer, build_batch_size, build_trajectories_per_step, build_keep_prob,
                                                                build_value_weight, sample_seed(seed, 0, 1), bchunks, brows, torch.device(device), hyper,
                                                                generator=generator)
                        btrainer.adam(build_lr)
                        if bstep >= build_lr_decay_start and bstep % build_lr_decay_interval == 0:
                            build_lr *= build_lr_decay
                        btrainer.average(build_avg_gamma)
                        bstep += 1
                        btrained += 1
                        if checkpoint and bstep % checkpoint == 0:
                            build_checkpoints[bstep] = btrainer.net_bytes()
                            if out_dir:
                                with open(os.path.join(out_dir, "%d.build.net" % bstep), "wb") as f:
                                    f.write(build_checkpoints[bstep])
                if btrained:
                    build_current = btrainer.net_bytes()
                build_row = {"skipped": int((out[4] == 3).sum().item()), "build_records": int(bst["appended"] - bbefore["appended"]), "build_window": bst["records"],
                             "build_step": bstep, "build_lr": build_lr, "build_append_s": tb1 - tb, "build_train_s": time.perf_counter() - tb1}
                if btrained:
                    build_row.update({"build_" + k: v for k, v in btrainer.report().items() if k != "steps"})
            row = {"round": rnd, "games": int(st["appended"] - before["appended"]), "frames": int(out[2].sum().item()), "window": st["records"],
                   "evicted": st["evicted"], "rejected": st["rejected"], "step": step, "lr": lr}
            if trained:
                previous, current = current, trainer.net_bytes()
                row.update({k: v for k, v in trainer.report().items() if k != "steps"})
            t3 = time.perf_counter()
            row.update(generate_s=t1 - t0, append_s=t2 - t1, train_s=t3 - t2)
            row.update(build_row)
            if gate_games and trained and previous is not None:
                from . import arena
                a, b = Network(ctx, data=current, discrete=discrete), Network(ctx, data=previous, discrete=discrete)
                try:
                    res = arena.match(ctx, a, b, np.asarray(pool, np.uint8).reshape(-1, 6, 5), gate_games, seed=sample_seed(seed, rnd, 1))
                finally:
                    a.close()
                    b.close()
                row["gate"] = {k: res[k] for k in ("W", "D", "L", "score", "elo")}
            history.append(row)
            if log:
                log(row)
        res = {"net": current, "checkpoints": checkpoints, "rounds": history, "window": window.stats()}
        if keep_records:
            res["records"] = window.records()
        if use_build:
            res.update(build_net=build_current, build_avg_net=btrainer.net_bytes("average"), build_checkpoints=build_checkpoints, build_window=bwindow.stats())
            if keep_records:
                res.update(build_records=bwindow.records(), build_rounds=build_rounds)
        return res
    finally:
        forest.close()
        trainer.close()
        window.close()
        if btrainer is not None:
            btrainer.close()
        if bwindow is not None:
            bwindow.close()


def print_json(row):
    print(json.dumps(row), flush=True)
