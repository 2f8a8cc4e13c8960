"""Measure the replay check of `.battle.data` records (oakgpu_replay_records_dev) on a seeded random-play corpus built on the GPU.

Corpus: random OU pairs (oakgpu_random_ou_battles_dev) with a few percent Ghost-vs-Ghost stalemates that run to turn 1,000
(tests/test_frames.py's endless-battle teams), played with uniformly drawn legal choices through the choices / update ABI on the
device, assembled into records with vectorised numpy, then TILED in device memory (the same games repeated) until one call holds at
least --min-frames frames.  Reported: device-resident replay (device events, after warm-up, several repeats), the only path that
existed before (a batched host loop of choices_dev x 2 + update_dev per turn over all live games, on the untiled corpus), the
configs[1]-style rollout rate in the same process for scale, and end to end from files (read + index + upload + replay: disk- and
PCIe-bound at ~60 B per frame).

  python tools/replay_bench.py [--games 65536] [--min-frames 100e6] [--repeats 5] [--out profiles/r06_replay.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oak_amd import _lib, gamedata as G  # noqa: E402


def P(t):
    return C.c_void_p(t.data_ptr())


def ghost_teams():
    blunt = [94, G.match_move("hypnosis"), G.match_move("bodyslam"), G.match_move("leer"), G.match_move("growl")]
    return np.array([[blunt] * 6, [blunt] * 6], dtype=np.uint8)


def play_corpus(ctx, n_games, seed=1, ghost_frac=0.02, record_choices=True):
    """n_games random-play games on the device.  Returns (first battles uint8[n, 384], final results uint8[n], frames
    uint8[T, n, 4] = (m, n, c1, c2) per turn, lengths int[n])."""
    import torch
    dev = torch.device("cuda", 0)
    u8 = torch.uint8
    lib, h = ctx.lib, ctx.handle
    ctx.ensure_ou_pools()
    b = torch.empty((n_games, 384), dtype=u8, device=dev)
    d = torch.empty((n_games, 8), dtype=u8, device=dev)
    pr = torch.empty((n_games, 8), dtype=u8, device=dev)
    r = torch.empty((n_games,), dtype=u8, device=dev)
    _lib.check(lib.oakgpu_random_ou_battles_dev(h, C.c_uint64(0x0A4B00000000 + seed * n_games), n_games, P(b), P(d), P(pr), P(r)))
    ctx.synchronize()
    n_ghost = int(n_games * ghost_frac)
    if n_ghost:
        gb, gd, gr = ctx.battle(np.stack([ghost_teams()] * n_ghost), np.arange(n_ghost, dtype=np.uint64) + seed * 7919)
        sel = torch.from_numpy(np.random.default_rng(seed).choice(n_games, n_ghost, replace=False)).to(dev)
        b[sel] = torch.from_numpy(gb).to(dev)
        r[sel] = torch.from_numpy(gr).to(dev)
    d.zero_()
    first = b.clone()
    gen = torch.Generator(device=dev).manual_seed(seed)
    live = torch.nonzero((r & 15) == 0).flatten()
    rows, lengths = [], torch.zeros(n_games, dtype=torch.int64, device=dev)
    while live.numel():
        lb, ld, lr = b[live].contiguous(), d[live].contiguous(), r[live].contiguous()
        m = live.numel()
        ch = [torch.empty((m, 9), dtype=u8, device=dev) for _ in range(2)]
        cn = [torch.empty((m,), dtype=u8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()   # (the context's stream does not wait for torch's: the gathers above must have landed)
        for pl in range(2):
            _lib.check(lib.oakgpu_choices_dev(h, P(lb), P(lr), pl, P(ch[pl]), P(cn[pl]), m))
        ctx.synchronize()
        pick = [(torch.randint(0, 1 << 30, (m,), device=dev, generator=gen) % cn[pl].long()) for pl in range(2)]
        c = [ch[pl].gather(1, pick[pl][:, None]).flatten().contiguous() for pl in range(2)]
        if record_choices:
            row = torch.zeros((n_games, 4), dtype=u8, device=dev)
            row[live] = torch.stack([cn[0], cn[1], c[0], c[1]], 1)
            rows.append(row)
        lengths[live] += 1
        torch.cuda.synchronize()
        _lib.check(lib.oakgpu_update_dev(h, P(lb), P(c[0]), P(c[1]), P(ld), None, None, m, P(lr)))
        ctx.synchronize()
        b[live], d[live], r[live] = lb, ld, lr
        live = live[(lr & 15) == 0]
    frames = torch.stack(rows).cpu().numpy() if rows else np.zeros((0, n_games, 4), np.uint8)
    return first.cpu().numpy(), r.cpu().numpy(), frames, lengths.cpu().numpy()


def assemble(first, results, frames, lengths):
    """Records (one bytes object, numpy-assembled) + their offsets, from play_corpus's arrays."""
    n = len(lengths)
    T = frames.shape[0]
    valid = np.arange(T)[:, None] < lengths[None, :]                     # [T, n]
    fsz = np.where(valid, 11 + 4 * (frames[..., 0].astype(np.int64) + frames[..., 1]), 0)
    rsz = 391 + fsz.sum(0)
    offs = np.concatenate([[0], np.cumsum(rsz)[:-1]])
    out = np.zeros(int(rsz.sum()), np.uint8)
    hdr = np.zeros((n, 6), np.uint8)
    hdr[:, :4] = rsz.astype("<u4").view(np.uint8).reshape(n, 4)
    hdr[:, 4:6] = lengths.astype("<u2").view(np.uint8).reshape(n, 2)
    pos = offs[:, None] + np.arange(6)[None, :]
    out[pos] = hdr
    out[offs[:, None] + 6 + np.arange(384)[None, :]] = first
    out[offs + 390] = results
    fpos = offs[None, :] + 391 + np.concatenate([np.zeros((1, n), np.int64), np.cumsum(fsz, 0)[:-1]], 0)   # [T, n]
    fp, fr = fpos[valid], frames[valid]
    out[fp] = ((fr[:, 0] - 1) | ((fr[:, 1] - 1) << 4)).astype(np.uint8)
    out[fp + 1] = fr[:, 2]
    out[fp + 2] = fr[:, 3]
    return out, offs


def main():
    import torch
    from oak_amd.engine import Context
    from oak_amd.frames import engine_switches
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--min-frames", type=float, default=100e6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()   # torch initialises the GPU before the library does
    ctx = Context(0)
    t0 = time.perf_counter()
    first, results, frames, lengths = play_corpus(ctx, a.games)
    t_play = time.perf_counter() - t0
    buf, offs = assemble(first, results, frames, lengths)
    n, total_frames = len(offs), int(lengths.sum())
    tiles = max(1, int(np.ceil(a.min_frames / total_frames)))
    res = {"engine_switches": engine_switches(), "games": n, "frames": total_frames, "bytes": int(buf.size),
           "bytes_per_frame": buf.size / total_frames, "max_frames": int(lengths.max()), "ghost_games": int(a.games * 0.02),
           "corpus_build_s": t_play, "tiles": tiles, "tiled_games": n * tiles, "tiled_frames": total_frames * tiles,
           "note": "the device-resident corpus is the same %d games repeated %d times (tiled in device memory)" % (n, tiles)}
    # device-resident: tile records + index in device memory
    rec_d = torch.from_numpy(buf).to(dev).repeat(tiles)
    offs_t = (torch.from_numpy(offs.astype(np.int64)).to(dev)[None, :] + torch.arange(tiles, device=dev)[:, None] * buf.size).flatten().contiguous()
    fr_d = torch.from_numpy(lengths.astype(np.int16)).to(dev).repeat(tiles)
    mal_d = torch.zeros(n * tiles, dtype=torch.uint8, device=dev)
    rep_d = torch.zeros((n * tiles, 8), dtype=torch.uint8, device=dev)
    N = n * tiles
    lib, h = ctx.lib, ctx.handle
    torch.cuda.synchronize()

    def replay():
        _lib.check(lib.oakgpu_replay_records_dev(h, P(rec_d), P(offs_t), P(fr_d), P(mal_d), N, P(rep_d), None, None))
    replay()
    ctx.synchronize()
    rep = rep_d.cpu().numpy()
    status = rep[:, 4]
    res["replay_status_counts"] = {int(s): int((status == s).sum()) for s in np.unique(status)}
    assert (status == 0).all(), res["replay_status_counts"]
    stream = torch.cuda.ExternalStream(lib.oakgpu_get_stream(h))
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        t = time.perf_counter()
        e0.record(stream)
        replay()
        e1.record(stream)
        e1.synchronize()
        ms.append((e0.elapsed_time(e1), (time.perf_counter() - t) * 1e3))
    dev_ms = [x[0] for x in ms]
    res["replay_device"] = {"ms_per_call": dev_ms, "host_wall_ms": [x[1] for x in ms], "median_ms": float(np.median(dev_ms)),
                            "frames_per_s_median": total_frames * tiles / (np.median(dev_ms) / 1e3),
                            "spread_pct": 100 * (max(dev_ms) - min(dev_ms)) / float(np.median(dev_ms)),
                            "timing": "device events around the call on the context's stream; the call includes a D2H copy of the "
                                      "frame counts and a host sort, both in front of the events' kernels"}
    del rec_d, offs_t, fr_d, mal_d, rep_d
    torch.cuda.empty_cache()
    # the rollout rate in the same process, for scale (random OU, 65,536 playouts to terminal)
    nr = 65536
    bb = torch.empty((nr, 384), dtype=torch.uint8, device=dev)
    dd = torch.empty((nr, 8), dtype=torch.uint8, device=dev)
    pp = torch.empty((nr, 8), dtype=torch.uint8, device=dev)
    rr = torch.empty((nr,), dtype=torch.uint8, device=dev)
    ro = torch.empty((nr,), dtype=torch.uint8, device=dev)
    so = torch.empty((nr,), dtype=torch.int32, device=dev)
    vo = torch.empty((nr,), dtype=torch.float32, device=dev)
    _lib.check(lib.oakgpu_random_ou_battles_dev(h, C.c_uint64(0x0A4B00000000), nr, P(bb), P(dd), P(pp), P(rr)))
    ctx.synchronize()
    b0, d0, p0 = bb.clone(), dd.clone(), pp.clone()
    rms, steps = [], 0
    for it in range(4):
        bb.copy_(b0); dd.copy_(d0); pp.copy_(p0)
        torch.cuda.synchronize()
        ctx.synchronize()
        t = time.perf_counter()
        _lib.check(lib.oakgpu_rollout_dev(h, P(bb), P(dd), P(rr), P(pp), nr, 1000, 0, P(ro), P(so), P(vo), None, None))
        ctx.synchronize()
        if it:
            rms.append(time.perf_counter() - t)
        steps = int(so.sum().item())
    res["rollout_same_process"] = {"playouts": nr, "turn_steps": steps, "median_s": float(np.median(rms)),
                                   "turn_steps_per_s": steps / float(np.median(rms))}
    res["replay_vs_rollout"] = res["replay_device"]["frames_per_s_median"] / res["rollout_same_process"]["turn_steps_per_s"]
    # baseline: the batched host loop over the untiled corpus -- choices_dev x 2 + update_dev per turn over all live games
    if not a.skip_baseline:
        bq = torch.from_numpy(first).to(dev)
        dq = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
        rq = torch.from_numpy(np.array([__import__("oak_amd.parse", fromlist=["x"]).result_from_state(x) for x in first], np.uint8)).to(dev)
        fq = torch.from_numpy(frames).to(dev)
        torch.cuda.synchronize()
        t = time.perf_counter()
        live = torch.arange(n, device=dev)
        k = 0
        while live.numel() and k < fq.shape[0]:
            live = live[torch.from_numpy(lengths).to(dev)[live] > k]
            if not live.numel():
                break
            m = live.numel()
            lb, ld, lr = bq[live].contiguous(), dq[live].contiguous(), rq[live].contiguous()
            ch, cn = torch.empty((m, 9), dtype=torch.uint8, device=dev), torch.empty((m,), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            for pl in range(2):
                _lib.check(lib.oakgpu_choices_dev(h, P(lb), P(lr), pl, P(ch), P(cn), m))
            c1, c2 = fq[k, live, 2].contiguous(), fq[k, live, 3].contiguous()
            _lib.check(lib.oakgpu_update_dev(h, P(lb), P(c1), P(c2), P(ld), None, None, m, P(lr)))
            ctx.synchronize()
            bq[live], dq[live], rq[live] = lb, ld, lr
            k += 1
        torch.cuda.synchronize()
        tb = time.perf_counter() - t
        ok = bool((rq.cpu().numpy() == results).all())
        res["baseline_host_loop"] = {"games": n, "frames": total_frames, "s": tb, "frames_per_s": total_frames / tb, "results_match": ok,
                                     "what": "per turn: gather the live games, oakgpu_choices_dev x 2, oakgpu_update_dev with the recorded "
                                             "choices, scatter back (untiled corpus)"}
        res["replay_vs_baseline"] = res["replay_device"]["frames_per_s_median"] / res["baseline_host_loop"]["frames_per_s"]
    # end to end from files: write the untiled corpus as 8 files, then read + index + upload + replay
    from oak_amd.frames import replay_check_files
    with tempfile.TemporaryDirectory() as td:
        cut = np.linspace(0, n, 9).astype(int)
        paths = []
        for i in range(8):
            lo = int(offs[cut[i]])
            hi = int(offs[cut[i + 1]]) if cut[i + 1] < n else buf.size
            p = os.path.join(td, "part%d.battle.data" % i)
            buf[lo:hi].tofile(p)
            paths.append(p)
        replay_check_files(ctx, paths[:1])
        t = time.perf_counter()
        out = replay_check_files(ctx, paths, chunk_bytes=64 << 20)
        te = time.perf_counter() - t
        assert (out["reports"]["status"] == 0).all() and len(out["reports"]) == n
    res["end_to_end_files"] = {"files": 8, "bytes": int(buf.size), "s": te, "MB_per_s": buf.size / te / 1e6, "frames_per_s": total_frames / te,
                               "bound": "disk (page cache here) + host indexing + PCIe upload at ~%.0f B per frame" % (buf.size / total_frames)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
