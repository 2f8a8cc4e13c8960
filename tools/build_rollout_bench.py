"""Measure the team-building rollout (oak_amd.build.rollout, one launch of oak_amd/csrc/buildnet.hip) against the same rollout as a
torch loop on the same device.

  python tools/build_rollout_bench.py [--rows 4096 65536] [--hidden 128] [--repeats 3] [--out profiles/r25_build_rollout.json]

Two kinds of input: empty teams (31 steps each) and the 16 sample teams with random deletions (Omitter::delete_info with both
probabilities 0.3).  Both sides use input_update = 1 (x at the action's cell): with it x is exactly the set of held cells, which is what
lets the torch loop build its legal mask from x; the kernel's work does not depend on the rule.

The baseline, per step: a batched dense forward x[n, 3749] -> h -> h -> 3749 (torch.addmm / relu), a masked softmax over the legal cells
(the mask from the team state by scatter and gather), torch.multinomial, and the team update by tensor operations; 30 addition steps and
the lead-swap step.  It draws from torch's generator, not the rows' streams, and sums in fp32: it is the same work, not the same bits.

Timing: wall clock around torch.cuda.synchronize, one warm-up of each side, then the two sides alternated --repeats times; medians.
Teams/s and steps/s (the kernel's own count of steps; the loop's masked steps are counted the same way)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sample_pool():
    from oak_amd import gamedata as G
    teams = json.load(open(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json")))["teams"]
    pool = np.zeros((len(teams), 6, 5), np.uint8)
    for t, team in enumerate(teams):
        for i, row in enumerate(team):
            pool[t, i] = [G.species_id(row[0])] + [G.move_id(m) for m in row[1:]]
    return pool.reshape(-1, 30)


def deleted_teams(pool, n, rng):
    teams = pool[rng.integers(0, len(pool), n)].reshape(n, 6, 5).copy()
    gone = rng.random((n, 6)) < 0.3
    teams[gone] = 0
    moves = teams[:, :, 1:]
    moves[rng.random((n, 6, 4)) < 0.3] = 0
    moves[gone] = 0
    return teams.reshape(n, 30)


class TorchLoop:
    """The baseline: the rollout as batched tensor operations."""

    def __init__(self, net_bytes, device):
        import torch
        from oak_amd import build
        self.torch, self.device = torch, device
        pos, self.layers = 0, []
        for _ in range(3):
            i, o = np.frombuffer(net_bytes, "<u4", 2, pos)
            b = np.frombuffer(net_bytes, "<f4", o, pos + 8)
            w = np.frombuffer(net_bytes, "<f4", int(o) * int(i), pos + 8 + 4 * int(o)).reshape(o, i)
            self.layers.append((torch.tensor(w.T.copy(), device=device), torch.tensor(b.copy(), device=device)))
            pos += 8 + 4 * int(o) + 4 * int(o) * int(i)
        _, cells, table = build.tables()
        self.cell_species = torch.tensor(cells[:, 0].astype(np.int64), device=device)
        self.cell_move = torch.tensor(cells[:, 1].astype(np.int64), device=device)
        self.table = torch.tensor(table.astype(np.int64), device=device)

    def run(self, teams):
        torch = self.torch
        n = teams.shape[0]
        t = teams.view(n, 6, 5).long()
        species, moves = t[:, :, 0].clone(), t[:, :, 1:].clone()
        rows = torch.arange(n, device=self.device)
        x = torch.zeros((n, 3749), device=self.device)
        cells = self.table[species[:, :, None].expand(-1, -1, 5), torch.cat([torch.zeros_like(species)[:, :, None], moves], 2)]   # [n, 6, 5]
        held = (species[:, :, None] > 0) & (cells >= 0)
        x[rows[:, None, None].expand_as(cells)[held], cells[held]] = 1.0
        steps = torch.zeros(n, dtype=torch.long, device=self.device)
        for step in range(31):
            h = x
            for k, (w, b) in enumerate(self.layers):
                h = torch.addmm(b, h, w)
                h = torch.relu(h) if k < 2 else h
            if step < 30:
                on_team = torch.zeros((n, 152), dtype=torch.bool, device=self.device)
                on_team.scatter_(1, species, True)
                room = torch.zeros((n, 152), dtype=torch.bool, device=self.device)
                room.scatter_(1, species, (moves == 0).any(2))
                room[:, 0] = False
                gap = (species == 0).any(1)
                is_species = self.cell_move == 0
                mask = torch.where(is_species[None, :], gap[:, None] & ~on_team[:, self.cell_species], room[:, self.cell_species] & (x == 0))
            else:                                             # the lead swaps: the species of slots 1 .. 5
                mask = torch.zeros((n, 3749), dtype=torch.bool, device=self.device)
                mask[rows[:, None].expand(-1, 5), self.table[species[:, 1:], 0]] = True
            live = mask.any(1)
            p = torch.softmax(h.masked_fill(~mask, float("-inf")), 1)
            p = torch.where(live[:, None], p, torch.full_like(p, 1.0 / 3749))
            c = torch.multinomial(p, 1).squeeze(1)
            s, m = self.cell_species[c], self.cell_move[c]
            if step < 30:
                add_species = live & (m == 0)
                slot = (species == 0).long().argmax(1)
                species[rows[add_species], slot[add_species]] = s[add_species]
                add_move = live & (m != 0)
                slot = (species == s[:, None]).long().argmax(1)
                free = (moves[rows, slot] == 0).long().argmax(1)
                moves[rows[add_move], slot[add_move], free[add_move]] = m[add_move]
                x[rows[live], c[live]] = 1.0
            else:
                lead = (species == s[:, None]).long().argmax(1)
                first_s, first_m = species[:, 0].clone(), moves[:, 0].clone()
                species[rows, 0], moves[rows, 0] = species[rows, lead], moves[rows, lead]
                species[rows, lead], moves[rows, lead] = first_s, first_m
            steps += live
        return torch.cat([species[:, :, None], moves], 2).to(torch.uint8).view(n, 30), steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from oak_amd import build, netfile
    from oak_amd.engine import Context
    ctx = Context(0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bench.build.net")
        netfile.write_random_build_net(path, 25, policy_hidden=a.hidden, value_hidden=a.hidden)
        net_bytes = open(path, "rb").read()
    net = build.BuildNetwork(ctx, net_bytes)
    loop = TorchLoop(net_bytes, "cuda")
    rng = np.random.default_rng(25)
    pool = sample_pool()
    res = {"device": torch.cuda.get_device_name(0), "hidden": a.hidden, "repeats": a.repeats, "input_update": 1,
           "timing": "wall clock around torch.cuda.synchronize, one warm-up of each side, sides alternated, medians", "cases": []}
    for n in a.rows:
        for kind in ("empty", "deleted"):
            teams = np.zeros((n, 30), np.uint8) if kind == "empty" else deleted_teams(pool, n, rng)
            build.check_teams(teams, None, 1)
            t = torch.from_numpy(teams).cuda()
            seeds = torch.from_numpy(rng.integers(0, 1 << 62, n).astype(np.int64)).cuda()

            def kernel():
                return build.rollout(ctx, net, t, seeds, input_update=1)

            def baseline():
                return loop.run(t)
            times = {"kernel": [], "torch_loop": []}
            out = kernel()
            done, _ = baseline()
            torch.cuda.synchronize()
            steps = int(out["n_updates"].long().sum().item())
            complete = bool((done.view(n, 6, 5)[:, :, 0] != 0).all().item()) and bool((out["teams_out"].view(n, 6, 5)[:, :, 0] != 0).all().item())
            for _ in range(a.repeats):
                for name, fn in (("kernel", kernel), ("torch_loop", baseline)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
            k, b = float(np.median(times["kernel"])), float(np.median(times["torch_loop"]))
            case = {"rows": n, "teams": kind, "steps": steps, "all_teams_complete": complete, "kernel_s": times["kernel"], "torch_loop_s": times["torch_loop"],
                    "kernel_teams_per_s": n / k, "kernel_steps_per_s": steps / k, "torch_loop_teams_per_s": n / b, "torch_loop_steps_per_s": steps / b,
                    "torch_loop_over_kernel": b / k}
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    net.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
