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
Departures from the reference, which runs its two halves concurrently as processes: the rounds alternate (no generate || train), the window
is counted in records rather than files (--data-window), there is no --sleep, and only the battle network is trained (no .build.data side).

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
                   max_battle_length=0, fast_budget=0, fast_search_prob=0.0, fast_policy_mode="", device="cuda:0"):
    """Round rnd's self-play call on device tensors: forest_selfplay's five tensors."""
    import torch
    from .frames import forest_selfplay
    name, c = parse_bandit(bandit)
    teams, battle_seeds, seeds = round_games(pool, games, seed, rnd)
    dev = torch.device(device)
    return forest_selfplay(ctx, torch.from_numpy(teams).to(dev), torch.from_numpy(battle_seeds.view(np.int64)).to(dev),
                           torch.from_numpy(seeds.view(np.int64)).to(dev), budget, c=c, bandit=name, evaluator=evaluator, policy_mode=policy_mode,
                           policy_temp=policy_temp, policy_min=policy_min, max_battle_length=max_battle_length, forest=forest, solve_nash="device",
                           fast_budget=fast_budget, fast_search_prob=fast_search_prob, fast_policy_mode=fast_policy_mode)


def run(ctx, net_bytes, pool, rounds, games, budget, steps, batch_size, lr, data_window, max_bytes=1 << 30, min_records=1, bandit="pucb-1.0",
        policy_mode="e", fast_policy_mode="", policy_temp=1.0, policy_min=0.0, max_battle_length=0, fast_budget=0, fast_search_prob=0.0,
        lr_decay=1.0, lr_decay_start=0, lr_decay_interval=1, loss=None, checkpoint=0, seed=0, discrete=False, clamp_parameters=False,
        apply_symmetry=True, out_dir=None, save_data=None, gate_games=0, evaluator=None, log=None, device="cuda:0", keep_records=False):
    """The loop.  net_bytes: the initial `.battle.net`; pool: uint8 [T, 6, 5] teams; evaluator: None (the network being trained, with
    PUCB or UCB) or "poke-engine" / "mc" for self-play that does not use it; log: a callable that receives each round's dict (tools/rl_loop.py
    prints it as JSON).  Returns {"net": the final parameters as `.battle.net` bytes, "checkpoints": {step: bytes}, "rounds": [dict],
    "window": the window's stats, and with keep_records "records": the window's bytes at the end}; with out_dir the checkpoints are also written
    there, with save_data each round's records."""
    from .engine import Network
    from .search import Forest
    name, _ = parse_bandit(bandit)
    loss = train_loss() if loss is None else loss
    enc = EncodedBattleFrames(batch_size, device)
    window = ReplayWindow(ctx, data_window, max_bytes)
    trainer = Trainer(ctx, net_bytes, batch_size)
    forest = Forest(ctx, games, max(int(budget), int(fast_budget), 1), contextual=name == "pucb")
    current, previous = bytes(net_bytes), None
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
                out = selfplay_round(ctx, forest, net if evaluator is None else evaluator, pool, games, seed, rnd, budget, bandit, policy_mode, policy_temp,
                                     policy_min, max_battle_length, fast_budget, fast_search_prob, fast_policy_mode, device)
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
            row = {"round": rnd, "games": int(st["appended"] - before["appended"]), "frames": int(out[2].sum().item()), "window": st["records"],
                   "evicted": st["evicted"], "rejected": st["rejected"], "step": step, "lr": lr}
            if trained:
                previous, current = current, trainer.net_bytes()
                row.update({k: v for k, v in trainer.report().items() if k != "steps"})
            t3 = time.perf_counter()
            row.update(generate_s=t1 - t0, append_s=t2 - t1, train_s=t3 - t2)
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
        return res
    finally:
        forest.close()
        trainer.close()
        window.close()


def print_json(row):
    print(json.dumps(row), flush=True)
