"""The reference's `generate` as a command over the device game loop (oak_amd.frames.forest_selfplay: whole batches of self-play games
resident on the GPU, one forest search per turn, oak_amd/csrc/forestplay.hip): play --games games and write their records as `.battle.data`
files under --out.

  python tools/generate_battle_data.py --out DIR [--games N] [--batch B] [--teams FILE] [--budget K] [--bandit ucb-2.0 | pucb-1.5]
         [--eval mc | fp | NET.battle.net] [--discrete] [--policy-mode e] [--policy-temp 1] [--policy-min 0] [--max-battle-length L]
         [--no-nash | --device-nash] [--seed S] [--file-mb 8] [--keep-node [--keep-arena NODES]]
         [--fast-budget K --fast-search-prob P [--fast-policy-mode MODE]]
         [--build-network NET.build.net [--team-modify-prob P] [--pokemon-delete-prob P] [--move-delete-prob P] [--max-pokemon K]
          [--battle-skip-prob P] [--t1-budget N]]

--teams FILE: JSON {"teams": [[[species, move, move, move, move] x 6] ...]} by name, the layout of tests/golden/ou_sample_teams.json (the
default: the reference's 16 sample teams); each game draws its two teams from the file with --seed's generator, a pair that fails the
endless battle check is drawn again (generate.cc:222-225).  --batch games are resident at a time (one forest of that many trees).  A file
is closed once it holds --file-mb MiB of whole records; names are <seed>_<index>.battle.data.  A game that reaches --max-battle-length
frames is dropped, as generate drops it.  --keep-node: each game's tree goes on into the next turn (generate.cc:324-333) on a kept forest
of --keep-arena nodes per tree (0 = 4 * budget + 1); then the keep-node ratio is printed as generate prints it (updates that found their
child / updates), with the trees dropped for want of room.  Prints games, frames, dropped games and seconds.

--fast-budget / --fast-search-prob / --fast-policy-mode (generate.cc:292-299; rl.py passes all of --budget, --fast-budget and
--fast-search-prob): each turn is, with probability --fast-search-prob, searched with --fast-budget iterations and picked with
--fast-policy-mode (default: --policy-mode) instead of --budget and --policy-mode; every frame is written with the iterations that ran.
Training then wants --min-iterations = fast_budget + 1 (tools/train_battle_net.py), as rl.py sets it, so that only the full-budget
frames reach the loss.  The fast and full frame counts and the tree-iterations launched and run are printed.

--build-network: the other half of generate (TeamBuilding::Provider::get_trajectory): both seats' teams come from oak_amd.build.provide on
the device -- a team of the pool, truncated to --max-pokemon, with probability --team-modify-prob thinned by --pokemon-delete-prob /
--move-delete-prob and completed by the build network -- pairs that fail the endless battle check are provided again with fresh seeds
before the games start, and every batch also writes <seed>_<batch>.build.data beside the `.battle.data`: one 128-byte record per built
seat of a kept or skipped game, game-major, p1 before p2 (oak_amd.build.game_records, one launch): the value is the game's matchup -- the
empirical value of its first search, 1 - it for p2 -- the p1 rows carry the game's score and the p2 rows 1 - score.  --battle-skip-prob: a
game with a built seat is skipped with this probability: searched once with --t1-budget iterations (0 = --budget) for its matchup, written
to `.build.data` without a score and to no `.battle.data`.  The engine takes teams with empty
slots and empty move slots (init_side skips them as the reference's does), so --max-pokemon below 6 and species whose pools hold fewer
than four moves are played as they are.  The seconds spent in team building are printed beside the total."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def draw_games(team_bytes, n, rng):
    """teams uint8[n, 60], battle seeds and policy seeds of n games; pairs the endless battle check refuses are drawn again."""
    import ctypes as C
    from oak_amd import _lib
    lib = _lib.load()
    teams = np.zeros((n, 60), np.uint8)
    for g in range(n):
        while True:
            i, j = rng.integers(0, len(team_bytes), 2)
            pair = np.ascontiguousarray(np.concatenate([team_bytes[i].reshape(30), team_bytes[j].reshape(30)]))
            if not lib.oakgpu_endless_battle_check(pair.ctypes.data_as(C.c_void_p)):
                break
        teams[g] = pair
    return teams, rng.integers(0, 1 << 63, n, dtype=np.uint64), rng.integers(0, 1 << 63, n, dtype=np.uint64)


def main():
    from policy_match import team_bytes
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--teams", default=os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json"))
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--bandit", default="ucb-2.0")
    ap.add_argument("--eval", default="fp")
    ap.add_argument("--discrete", action="store_true")
    ap.add_argument("--policy-mode", default="e")
    ap.add_argument("--policy-temp", type=float, default=1.0)
    ap.add_argument("--policy-min", type=float, default=0.0)
    ap.add_argument("--max-battle-length", type=int, default=0)
    ap.add_argument("--no-nash", action="store_true")
    ap.add_argument("--device-nash", action="store_true", help="solve the root matrices on the GPU (the same bits, no host round trip)")
    ap.add_argument("--seed", type=int, default=0x0A4B)
    ap.add_argument("--file-mb", type=float, default=8.0)
    ap.add_argument("--keep-node", action="store_true")
    ap.add_argument("--keep-arena", type=int, default=0)
    ap.add_argument("--fast-budget", type=int, default=0, help="iterations for non-training frames (0 = --budget); train with --min-iterations = fast_budget + 1")
    ap.add_argument("--fast-search-prob", type=float, default=0.0, help="probability that a turn is a fast search (0 = off)")
    ap.add_argument("--fast-policy-mode", default="", help="policy mode of a fast turn's pick (default: --policy-mode)")
    ap.add_argument("--build-network", default="", help="a .build.net: build both seats' teams on the device and write .build.data")
    ap.add_argument("--team-modify-prob", type=float, default=0.0)
    ap.add_argument("--pokemon-delete-prob", type=float, default=0.0)
    ap.add_argument("--move-delete-prob", type=float, default=0.0)
    ap.add_argument("--max-pokemon", type=int, default=6)
    ap.add_argument("--battle-skip-prob", type=float, default=0.0, help="probability that a game with a built seat is searched once and not played")
    ap.add_argument("--t1-budget", type=int, default=0, help="iterations of a skipped game's one search (0 = --budget)")
    a = ap.parse_args()
    name, _, c = a.bandit.partition("-")
    if name not in ("ucb", "pucb"):
        sys.exit("--bandit: ucb-<c> or pucb-<c> (the forest search runs no other)")
    from oak_amd.engine import Context, Network
    from oak_amd.frames import forest_selfplay
    from oak_amd.search import Forest
    if a.build_network:
        import torch
        torch.zeros(1, device="cuda:0")                                  # (build.game_records stages through torch, which initialises the GPU before the library does)
    ctx = Context(0)
    evaluator = {"mc": "mc", "": "mc", "fp": "poke-engine"}.get(a.eval)
    net = None
    if evaluator is None:
        evaluator = net = Network(ctx, path=a.eval, discrete=a.discrete)
    pool = team_bytes(a.teams)
    build_net = None
    if a.build_network:
        from oak_amd import build
        build.check_provide(np.asarray(pool, np.uint8).reshape(-1, 30), 1, a.max_pokemon, a.pokemon_delete_prob, a.move_delete_prob, a.team_modify_prob)
        build_net = build.BuildNetwork(ctx, a.build_network)
    elif a.max_pokemon != 6 or a.team_modify_prob or a.pokemon_delete_prob or a.move_delete_prob or a.battle_skip_prob or a.t1_budget:
        sys.exit("--max-pokemon / --team-modify-prob / --pokemon-delete-prob / --move-delete-prob / --battle-skip-prob / --t1-budget need --build-network")
    build_seconds, build_records, batches = 0.0, 0, 0
    rng = np.random.default_rng(a.seed)
    os.makedirs(a.out, exist_ok=True)
    batch = max(1, min(a.batch, a.games))
    forest = Forest(ctx, batch, max(a.budget, a.fast_budget, a.t1_budget), contextual=name == "pucb", keep_arena=a.keep_arena if a.keep_node else None)
    limit = int(a.file_mb * (1 << 20))
    played = frames = dropped = files = skipped = 0
    updates = updates_with_node = trees_dropped = 0
    fast_frames = full_frames = launched = run = 0
    pending = []
    t0 = time.perf_counter()

    def flush(everything):
        nonlocal files, pending
        while pending and (everything or sum(map(len, pending)) >= limit):
            size, k = 0, 0
            while k < len(pending) and (k == 0 or size + len(pending[k]) <= limit):
                size += len(pending[k])
                k += 1
            with open(os.path.join(a.out, "%d_%d.battle.data" % (a.seed, files)), "wb") as f:
                f.write(b"".join(pending[:k]))
            files += 1
            pending = pending[k:]

    while played < a.games:
        n = min(batch, a.games - played)
        if build_net is None:
            teams, battle_seeds, seeds = draw_games(pool, n, rng)
        else:
            tb = time.perf_counter()
            teams, seats = build.provide_pairs(ctx, build_net, np.asarray(pool, np.uint8).reshape(-1, 30), rng.integers(0, 1 << 63, (n, 2), dtype=np.uint64),
                                               max_pokemon=a.max_pokemon, pokemon_delete_prob=a.pokemon_delete_prob, move_delete_prob=a.move_delete_prob,
                                               team_modify_prob=a.team_modify_prob)
            build_seconds += time.perf_counter() - tb
            battle_seeds, seeds = rng.integers(0, 1 << 63, n, dtype=np.uint64), rng.integers(0, 1 << 63, n, dtype=np.uint64)
        built = None if build_net is None else ((seats[0]["n_updates"] > 0) | ((seats[1]["n_updates"] > 0) << 1)).astype(np.uint8)
        stats = {}
        stream, offsets, n_frames, results, status = forest_selfplay(
            ctx, teams, battle_seeds, seeds, a.budget, c=float(c or 2.0), bandit=name, evaluator=evaluator, policy_mode=a.policy_mode,
            policy_temp=a.policy_temp, policy_min=a.policy_min, max_battle_length=a.max_battle_length, forest=forest, solve_nash=False if a.no_nash else ("device" if a.device_nash else True),
            keep_node=a.keep_node, stats=stats, fast_budget=a.fast_budget, fast_search_prob=a.fast_search_prob, fast_policy_mode=a.fast_policy_mode,
            built=built, battle_skip_prob=a.battle_skip_prob, t1_budget=a.t1_budget)[:5]
        fast_frames, full_frames, launched, run = fast_frames + stats["fast_frames"], full_frames + stats["full_frames"], launched + stats["launched"], run + stats["run"]
        if a.keep_node:   # RuntimeData::update_with_node_counter / update_counter (generate.cc:412-416)
            updates, updates_with_node, trees_dropped = updates + int(n_frames.sum()), updates_with_node + stats["nodes_kept"], trees_dropped + stats["dropped"]
        kept = status == 0
        if build_net is not None:   # generate.cc:190-213, 361-386: the trajectories of the kept and the skipped games, matchup and score
            tb = time.perf_counter()
            data = build.game_records(ctx, seats, status, results, stats["matchup"])
            with open(os.path.join(a.out, "%d_%d.build.data" % (a.seed, batches)), "wb") as f:
                f.write(data)
            build_records += len(data) // 128
            build_seconds += time.perf_counter() - tb
        batches += 1
        pending += [stream[int(offsets[g]):int(offsets[g + 1])] for g in range(n) if kept[g]]
        skipped += int((status == 3).sum())
        played, frames, dropped = played + n, frames + int(n_frames[kept].sum()), dropped + int((~kept).sum())
        flush(False)
    flush(True)
    s = time.perf_counter() - t0
    print("games: %d, frames: %d, dropped: %d, files: %d, seconds: %.2f (%.1f games/s, %.0f frames/s)" % (played - dropped, frames, dropped, files, s,
                                                                                                       (played - dropped) / s, frames / s))
    if a.battle_skip_prob > 0:
        print("skipped battles: %d of the %d dropped (searched once with %d iterations for their matchup)" % (skipped, dropped, a.t1_budget or a.budget))
    if build_net is not None:
        print("team building: %d records, %.2f seconds (%.1f %% of the call)" % (build_records, build_seconds, 100 * build_seconds / s))
        build_net.close()
    if a.fast_search_prob > 0:
        print("fast frames: %d, full frames: %d (the frames --min-iterations %d keeps), tree-iterations launched: %d, run: %d" % (
            fast_frames, full_frames, (a.fast_budget or a.budget) + 1, launched, run))
    if a.keep_node:
        print("keep node ratio: %g" % (updates_with_node / max(updates, 1)))
        print("trees dropped for want of room: %d" % trees_dropped)
    forest.close()
    if net is not None:
        net.close()
    ctx.close()


if __name__ == "__main__":
    main()
