"""Measure the whole-game loop (oakgpu_policy_games_dev through oak_amd.arena.policy_games on device tensors) against the loop a user could
write from the public calls that existed before it: per turn oakgpu_tree_step_dev, oakgpu_leaf_eval_policy_dev on all n rows, and the
pick on the host.

Workload: --games (65,536) random OU battles built on the device (oakgpu_random_ou_battles_dev), RANDOM against RANDOM and, for each
network, POLICY against POLICY with one handle in both seats.  Per workload: three runs of the device loop with compaction on, three of
the baseline, alternating, the order of each pair swapped from round to round, after one warm-up of each; then one run of the device loop
with compaction off.  Times are a host clock around calls that end with the stream idle.  Reported: games/s, turn-steps/s (the games' own
updates, sum of turns_out), the share of rows the evaluator and the tree step ran over for games already over (1 - turn-steps / rows
looped), the compactions, and whether the device loop's median is no slower than the baseline's fastest run.

  python tools/policy_games_bench.py [--games 65536] [--max-turns 1000] [--workloads random,tiny,default,256] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from oak_amd import _lib, arena
    from oak_amd.engine import Context, Network
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--max-turns", type=int, default=1000)
    ap.add_argument("--workloads", default="random,tiny,default,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.cuda.init()   # torch initialises the GPU before the library does
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    ctx.ensure_ou_pools()
    lib, h, n = ctx.lib, ctx.handle, a.games
    P = lambda t: C.c_void_p(t.data_ptr())
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
    b0, d0, p0, r0 = u8(n, 384), u8(n, 8), u8(n, 8), u8(n)
    _lib.check(lib.oakgpu_random_ou_battles_dev(h, 0x0A4B00000000, n, P(b0), P(d0), P(p0), P(r0)))
    ctx.synchronize()

    def device_loop(net, compact_below):
        ctx.synchronize()
        t = time.perf_counter()
        out = arena.policy_games(ctx, (net, net), b0, d0, r0, p0, max_turns=a.max_turns, compact_below=compact_below)
        s = time.perf_counter() - t
        st = arena.last_stats(ctx)
        steps = int(out["turns"].to(torch.int64).sum())
        return dict(s=s, turn_steps=steps, games_per_s=n / s, turn_steps_per_s=steps / s, rows_looped=st["row_turns"], turns_looped=st["turns"],
                    compactions=st["compactions"], polls=st["polls"], dead_row_share=1.0 - steps / max(st["row_turns"], 1), counts=list(out["counts"]))

    def baseline(net, seed=7):
        """tree step, evaluator on all n rows, pick on the host: one round trip per turn"""
        rng = np.random.default_rng(seed)
        b, d, r = b0.clone(), d0.clone(), r0.clone()
        ch1, ch2, n1, n2, c1, c2, act = u8(n, 9), u8(n, 9), u8(n), u8(n), u8(n), u8(n), u8(n, 16)
        val = torch.empty(n, dtype=torch.float32, device=dev)
        l1, l2 = torch.empty((n, 9), dtype=torch.float32, device=dev), torch.empty((n, 9), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(lib.oakgpu_choices_dev(h, P(b), P(r), 0, P(ch1), P(n1), n))
        _lib.check(lib.oakgpu_choices_dev(h, P(b), P(r), 1, P(ch2), P(n2), n))
        turns = np.zeros(n, np.int64)
        lane = np.arange(n)

        def host_pick(logits, counts):
            k = np.maximum(counts.astype(np.int64), 1)
            if logits is None:
                return rng.integers(0, 1 << 32, n) % k
            ex = np.where(np.arange(9)[None, :] < k[:, None], np.exp(logits), np.float32(0))
            cum = np.cumsum(ex.astype(np.float64), axis=1)
            u = rng.random(n) * cum[:, -1]
            return np.minimum((cum < u[:, None]).sum(axis=1), k - 1)

        for _ in range(a.max_turns):
            if net is not None:
                _lib.check(lib.oakgpu_leaf_eval_policy_dev(h, net.handle, P(b), P(d), n, P(ch1), P(n1), P(ch2), P(n2), P(val), P(l1), P(l2)))
            ctx.synchronize()
            res = r.cpu().numpy()
            live = (res & 15) == 0
            if not live.any():
                break
            i1 = host_pick(None if net is None else l1.cpu().numpy(), n1.cpu().numpy())
            i2 = host_pick(None if net is None else l2.cpu().numpy(), n2.cpu().numpy())
            h1 = np.where(live, ch1.cpu().numpy()[lane, i1], 0xFF).astype(np.uint8)
            h2 = np.where(live, ch2.cpu().numpy()[lane, i2], 0xFF).astype(np.uint8)
            c1.copy_(torch.from_numpy(h1))
            c2.copy_(torch.from_numpy(h2))
            torch.cuda.synchronize()
            _lib.check(lib.oakgpu_tree_step_dev(h, P(b), P(d), P(r), P(c1), P(c2), n, 39, P(act), P(ch1), P(n1), P(ch2), P(n2)))
            turns += live
        ctx.synchronize()
        s = time.perf_counter() - t0
        steps = int(turns.sum())
        return dict(s=s, turn_steps=steps, games_per_s=n / s, turn_steps_per_s=steps / s, rows_looped=n * int(turns.max()), dead_row_share=1.0 - steps / max(n * int(turns.max()), 1))

    nets = {"tiny": "net_tiny.battle.net", "default": "net_default.battle.net", "256": "net_256.battle.net"}
    res = {"what": "tools/policy_games_bench.py on one MI355X", "games": n, "max_turns": a.max_turns,
           "timing": "host clock around each whole call, the stream idle before and after; one warm-up of each form first",
           "baseline": "per turn: oakgpu_tree_step_dev, oakgpu_leaf_eval_policy_dev on all n rows, the pick on the host (numpy), choices copied back",
           "workloads": {}}
    for name in a.workloads.split(","):
        net = None if name == "random" else Network(ctx, path=os.path.join(ROOT, "tests", "golden", nets[name]))
        device_loop(net, 0.0)
        warm = a.max_turns
        a.max_turns = min(a.max_turns, 8)       # (the baseline's warm-up: its kernels and shapes, not its thousand turns)
        baseline(net)
        a.max_turns = warm
        dl, bl = [], []
        for k in range(a.rounds):
            for which in (("device", "baseline") if k % 2 == 0 else ("baseline", "device")):
                (dl if which == "device" else bl).append(device_loop(net, 0.0) if which == "device" else baseline(net))
            print("  %s round %d: device %.3f s, baseline %.3f s" % (name, k, dl[-1]["s"], bl[-1]["s"]), file=sys.stderr, flush=True)
        off = device_loop(net, -1.0)
        med = float(np.median([x["s"] for x in dl]))
        best_base = min(x["s"] for x in bl)
        res["workloads"][name] = {
            "seats": "RANDOM vs RANDOM" if net is None else "POLICY vs POLICY, %s, one handle" % nets[name],
            "device_loop": dl, "baseline_loop": bl, "device_loop_compaction_off": off,
            "device_median_s": med, "baseline_fastest_s": best_base, "device_no_slower_than_baseline": bool(med <= best_base),
            "games_per_s_median": n / med, "turn_steps_per_s_median": dl[0]["turn_steps"] / med,
            "dead_row_share_compaction_on": dl[0]["dead_row_share"], "dead_row_share_compaction_off": off["dead_row_share"],
            "compactions": dl[0]["compactions"]}
        if net is not None:
            net.close()
        if a.out:       # (written after every workload: a run cut short keeps what it measured)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
