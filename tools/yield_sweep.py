"""Manual GPU tool: the default command's timed region -- eight group launches of 20 x 65,536 playouts alternating over two contexts,
each followed by the caller's reduction on its stream -- in one process, for a list of schedule settings.

  python tools/yield_sweep.py [REPS] SETTING ...      SETTING = off | tail:BELOW:WAVES:LANES | yield:BELOW:R:LANES

`off` is the single dispatch with migration, `tail` oakgpu_set_tail_pack (a full grid, then WAVES follow-up waves), `yield`
oakgpu_set_yield_schedule mode 1 (R waves fewer, then at most R).  Every launch starts from the same choice streams, so every setting
does the same work; the outputs' sums must not change.  Prints one JSON line per setting: G turn-steps/s of every repetition, ms per
launch period, the parked playouts of each context's last launch and the error word."""
import ctypes as C
import json
import sys
import time

import torch

sys.path.insert(0, ".")
from oak_amd import _lib
from oak_amd.engine import Context

G, n, LAUNCHES = 20, 65536, 8
dev = torch.device("cuda", 0)
P = lambda t: C.c_void_p(t.data_ptr())


class Slot:
    def __init__(self, idx):
        self.ctx = Context(0)
        self.stream = torch.cuda.ExternalStream(self.ctx.stream_ptr(), device=dev)
        self.ctx.ensure_ou_pools()
        T = lambda *s, dt=torch.uint8: torch.empty(s, dtype=dt, device=dev)
        self.battles, self.durations, self.prng, self.prng0 = T(G, n, 384), T(G, n, 8), T(G, n, 8), T(G, n, 8)
        self.rin, self.rout = T(G, n), T(G, n)
        self.steps, self.values = torch.zeros((G, n), dtype=torch.int32, device=dev), T(G, n, dt=torch.float32)
        self.total = torch.zeros((), dtype=torch.int64, device=dev)
        self.descs = (_lib.RolloutBatch * G)()
        for k in range(G):
            _lib.check(self.ctx.lib.oakgpu_random_ou_battles_dev(self.ctx.handle, C.c_uint64(0x0A4B00000000 + (idx * G + k) * n), n, P(self.battles[k]),
                                                                 P(self.durations[k]), P(self.prng0[k]), P(self.rin[k])))
            self.descs[k] = _lib.RolloutBatch(self.battles[k].data_ptr(), self.durations[k].data_ptr(), self.rin[k].data_ptr(), self.prng[k].data_ptr(), n,
                                              self.rout[k].data_ptr(), self.steps[k].data_ptr(), self.values[k].data_ptr(), None, None)
        self.ctx.synchronize()

    def run(self):
        with torch.cuda.stream(self.stream):
            self.prng.copy_(self.prng0, non_blocking=True)   # (a 10 MB copy per launch, the same for every setting)
        _lib.check(self.ctx.lib.oakgpu_rollout_group_dev(self.ctx.handle, self.descs, G, 1000, 0))
        with torch.cuda.stream(self.stream):
            self.total += self.steps.sum(dtype=torch.int64)


def apply(slots, setting):
    f = setting.split(":")
    below, waves, lanes = (int(x) for x in f[1:4]) if len(f) == 4 else (0, 0, 0)
    for sl in slots:
        _lib.check(sl.ctx.lib.oakgpu_set_tail_pack(sl.ctx.handle, below if f[0] == "tail" else 0, waves, lanes))
        _lib.check(sl.ctx.lib.oakgpu_set_yield_schedule(sl.ctx.handle, 1 if f[0] == "yield" else 0, below if f[0] == "yield" else 16, waves, lanes))


def main():
    args = sys.argv[1:]
    reps = int(args.pop(0)) if args and args[0].isdigit() else 3
    slots = [Slot(0), Slot(1)]
    ref = None
    for setting in args or ["off"]:
        apply(slots, setting)
        rates, periods = [], []
        for _ in range(reps + 1):   # the first repetition warms the setting up (and is the registry's first alternation)
            for sl in slots:
                sl.total.zero_()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for k in range(LAUNCHES):
                slots[k % 2].run()
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            tot = sum(int(sl.total.item()) for sl in slots)
            rates.append(round(tot / dt / 1e9, 3))
            periods.append(round(dt / LAUNCHES * 1e3, 3))
        sig = [tot] + [int(x.sum(dtype=torch.int64).item()) for sl in slots for x in (sl.rout, sl.prng, sl.values.view(torch.int32))]
        ref = ref or sig
        assert sig == ref, "results changed with the schedule: %r vs %r" % (sig, ref)
        qc = [sl.ctx.queue_counters() for sl in slots]
        print(json.dumps({"setting": setting, "g_turn_steps_per_s": rates[1:], "ms_per_launch": periods[1:], "warm_rep": rates[0],
                          "yielded": [sl.ctx.last_launch_yield() for sl in slots], "parked_last_launch": [sl.ctx.last_launch_parked() for sl in slots],
                          "error_word_63": [int(c[63]) for c in qc]}), flush=True)


if __name__ == "__main__":
    main()
