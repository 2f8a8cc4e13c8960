"""One optimiser step of the build network, oak_amd.build.Trainer against the SAME step as a torch loop on the same device: build.py's
process_targets verbatim on dense states (oak_amd.build.dense_state), three-layer torch.nn.Linear nets, autograd, torch.optim.Adam and
the rolling average.  The baseline is that torch loop, never this code; no ratio is promised.

  python tools/build_trainer_bench.py [--trajectories 4096] [--batches 61000,1000000] [--hidden 128] [--rounds 3] [--records 20000] [--out X.json]

The trajectories are made on the device (provide -> records with a seeded random net), decoded once (int64 masks, what torch's gather
reads) and handed to both sides: a step is timed from zero_grad to the rolling average, without sampling and decoding.  The two sides
alternate in one process; the figures are medians of the rounds after one warm-up step of each.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HYPER = dict(gamma=0.99, lam=0.90, policy_loss_weight=1.0, value_loss_weight=0.5, entropy_loss_weight=0.01)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trajectories", type=int, default=4096)
    ap.add_argument("--batches", default="61000,1000000")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import build_ref as B
    from oak_amd import build, netfile
    from oak_amd.engine import Context
    assert torch.cuda.is_available(), "build_trainer_bench needs a GPU"
    device = torch.device("cuda:0")
    torch.zeros(1, device=device)
    ctx = Context(0)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bench.build.net")
        netfile.write_random_build_net(path, 3, policy_hidden=a.hidden, value_hidden=a.hidden)
        net_bytes = open(path, "rb").read()
    seeds = np.arange(a.records, dtype=np.uint64) + np.uint64(7)
    with build.BuildNetwork(ctx, net_bytes) as net:
        rolled = build.provide(ctx, net, B.sample_teams(), seeds, team_modify_prob=0.9, pokemon_delete_prob=0.3, move_delete_prob=0.3)
    data = build.records(ctx, rolled, np.linspace(0, 1, a.records).astype(np.float32), 0.5)
    corpus = build.TrajectoryCorpus(ctx, data)
    result = {"trajectories_per_chunk": a.trajectories, "hidden": a.hidden, "records": corpus.records, "rounds": a.rounds, "hyper": HYPER, "steps": []}

    # ---- the torch side: three-layer nets, process_targets on dense states, autograd, Adam ------------------------------------------------
    def layers(blob):
        import struct
        out, pos = [], 0
        for _ in range(6):
            i, o = struct.unpack_from("<II", blob, pos)
            b = np.frombuffer(blob, "<f4", o, pos + 8).copy()
            w = np.frombuffer(blob, "<f4", o * i, pos + 8 + 4 * o).reshape(o, i).copy()
            out.append((b, w))
            pos += 8 + 4 * o * (i + 1)
        return out

    def torch_net(k):
        seq = []
        for q, (b, w) in enumerate(layers(net_bytes)[3 * k:3 * k + 3]):
            lin = torch.nn.Linear(w.shape[1], w.shape[0], device=device)
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(w))
                lin.bias.copy_(torch.from_numpy(b))
            seq += [lin] + ([torch.nn.ReLU()] if q < 2 else [])
        return torch.nn.Sequential(*seq)

    def apply_force_with_threshold(decision_outputs, force, threshold, threshold_center):
        can_decrease = decision_outputs - threshold_center > -threshold
        can_increase = decision_outputs - threshold_center < threshold
        force_negative = torch.clamp(force, max=0.0)
        force_positive = torch.clamp(force, min=0.0)
        clipped_force = can_decrease * force_negative + can_increase * force_positive
        return decision_outputs * clipped_force.detach()

    def process_targets(policy_net, value_net, traj, tg):
        mask, policy = traj["mask"], traj["policy"].unsqueeze(-1)
        b, T, _ = mask.shape
        valid = tg["valid"]
        valid_state = build.dense_state(ctx, tg, 0, tg["n_valid"])
        logits, v = policy_net(valid_state), value_net(valid_state)
        value = torch.sigmoid(v)
        valid_mask = mask[valid]
        mask_logits = torch.where(valid_mask >= 0, torch.gather(logits, 1, torch.clamp(valid_mask, min=0)), -torch.inf)
        logits = mask_logits[:, 0]
        mask_weights = torch.exp(mask_logits)
        mask_probs = torch.nn.functional.normalize(mask_weights, dim=1, p=1)
        valid_logp = torch.log(mask_probs[:, 0]).unsqueeze(-1)
        rewards = tg["rewards"].unsqueeze(-1)
        value_full = torch.zeros_like(policy)
        value_full[valid] = value
        next_value_full = torch.cat([value_full[:, 1:], torch.zeros_like(value_full[:, -1:])], dim=1)
        deltas = rewards + HYPER["gamma"] * next_value_full - value_full
        advantages = []
        advantage = torch.zeros((b, 1), device=device)
        for t in reversed(range(T)):
            advantage = deltas[:, t, :] * valid[:, t].unsqueeze(-1) + HYPER["gamma"] * HYPER["lam"] * advantage
            advantages.insert(0, advantage)
        gae = torch.stack(advantages, dim=1)
        returns = gae + value_full
        threshold_center = torch.zeros_like(logits)
        forced = apply_force_with_threshold(logits, gae[valid].squeeze(-1), 2, threshold_center)
        logp = torch.ones_like(policy)
        logp[valid] = valid_logp
        return (forced,) + tuple(x[valid] for x in (returns, value_full, logp))

    def compute_loss_from_targets(surr, returns, values, logp_actions, total, remaining):
        b = surr.shape[0]
        n = min(b, remaining)
        policy_loss = -(surr[:n]).mean()
        value_loss = (((returns - values)) ** 2)[:n].mean()
        entropy = -(logp_actions * logp_actions.exp()).sum(dim=-1, keepdim=True)[:n].mean()
        return (n / total) * (HYPER["policy_loss_weight"] * policy_loss + HYPER["value_loss_weight"] * value_loss - HYPER["entropy_loss_weight"] * entropy)

    for batch in [int(x) for x in a.batches.split(",")]:
        chunks, rows = [], 0
        while rows < batch:                                   # decoded once, shared by both sides
            traj = corpus.sample(a.trajectories, 1000 + len(chunks) * a.trajectories, mask_dtype="int64", device=device)
            tg = build.targets(ctx, traj, 1.0)
            chunks.append((traj, tg))
            rows += tg["n_valid"]
        policy_net, value_net = torch_net(0), torch_net(1)
        average = [p.detach().clone() for net in (policy_net, value_net) for p in net.parameters()]
        optimizer = torch.optim.Adam(list(policy_net.parameters()) + list(value_net.parameters()), lr=1e-4)
        trainer = build.Trainer(ctx, net_bytes, a.trajectories)

        def ours():
            trainer.zero_gradients()
            b = 0
            for traj, tg in chunks:
                trainer.accumulate(traj, tg, total=batch, remaining=batch - b, **HYPER)
                b += tg["n_valid"]
            trainer.adam(1e-4)
            trainer.average(0.995)
            return trainer.report()["loss"]                   # waits for the context's stream

        def theirs():
            optimizer.zero_grad()
            b = 0
            for traj, tg in chunks:
                loss = compute_loss_from_targets(*process_targets(policy_net, value_net, traj, tg), batch, batch - b)
                loss.backward()
                b += tg["n_valid"]
            optimizer.step()
            with torch.no_grad():
                for avg_p, p in zip(average, [p for net in (policy_net, value_net) for p in net.parameters()]):
                    avg_p.mul_(0.995).add_(p, alpha=1 - 0.995)
            torch.cuda.synchronize()
            return float(loss)

        times = {"hip": [], "torch": []}
        for name, fn in (("hip", ours), ("torch", theirs)):   # warm-up: code objects, allocator, algorithm choices
            fn()
        last = {}
        for _ in range(a.rounds):
            for name, fn in (("hip", ours), ("torch", theirs)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = fn()
                times[name].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in times.items()}
        result["steps"].append({"batch": batch, "chunks": len(chunks), "valid_rows": rows, "hip_s": med["hip"], "torch_s": med["torch"], "hip_all_s": times["hip"],
                                "torch_all_s": times["torch"], "hip_rows_per_s": min(rows, batch) / med["hip"], "torch_rows_per_s": min(rows, batch) / med["torch"],
                                "last_chunk_loss": last})
        trainer.close()
        del chunks, policy_net, value_net, optimizer, average
        torch.cuda.empty_cache()
    corpus.close()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
