"""Training batches from `.battle.data` records on the GPU: the reference's loader (pyoak.sample + EncodedBattleFrames,
cpp/src/pyoak.cc:111-245, py/battle/encoded-frames.h, py/battle/target.h) over the C ABI of include/oakgpu.h, where the contract of a
row is written down.  The records are uploaded once (FrameCorpus); a batch is replayed, encoded and written on the device
(k_frames_pick, k_frames_encode in oak_amd/csrc/trainframes.hip).  This module only holds buffers and marshals pointers.

    corpus = FrameCorpus(ctx, paths)
    enc = EncodedBattleFrames(4096, "cuda:0")          # torch tensors with the reference's attribute names and shapes
    ok = corpus.sample(enc, seed=step, max_battle_length=0, min_iterations=1)

With device=None the tensors are numpy arrays and the calls go through the staged host-pointer entry points.

Scoring a network on every frame of a corpus (k_frames_expand, k_corpus_terms, k_corpus_record_sums in oak_amd/csrc/corpuseval.hip):

    out = corpus.inference(net)                        # value [F,1], policy_logit [F,2,9], policy [F,2,9], k, status, where, picks
    losses = corpus.evaluate(net, 0.0, 0.5, 0.5, 0.5)  # mse, ce_p1, ce_p2, rows, excluded, failed

The optimiser step on such batches (oak_amd/csrc/trainer.hip): Trainer, apply_symmetries, train_loss, trainer_check below."""
import ctypes as C

import numpy as np

from . import _lib

PICK_STATUS = ("OK", "COUNT", "ILLEGAL", "EARLY_END", "RESULT", "MALFORMED", "RANGE")
POKEMON_IN, ACTIVE_IN, POLICY_DIM = 198, 229, 315
# name -> (shape behind the batch axis, dtype): the reference's fields, then status / where
FIELDS = {
    "pokemon": ((2, 6, POKEMON_IN), "float32"), "active": ((2, 1, ACTIVE_IN), "float32"), "hp": ((2, 6, 1), "float32"),
    "choice_indices": ((2, 9), "int64"), "k": ((2, 1), "uint8"), "choice": ((2, 1), "uint8"), "iterations": ((1,), "uint32"),
    "empirical_policies": ((2, 9), "float32"), "nash_policies": ((2, 9), "float32"), "empirical_value": ((1,), "float32"),
    "nash_value": ((1,), "float32"), "score": ((1,), "float32"), "status": ((), "uint8"), "where": ((), "uint32"),
}


class EncodedBattleFrames:
    """`size` rows of every tensor of a training batch, plus `picks` (size x 2 uint32: record, frame).  device: a torch device on the
    GPU, or None for numpy arrays on the host."""

    def __init__(self, size, device=None):
        self.size, self.device = int(size), device
        if device is None:
            for name, (tail, dtype) in FIELDS.items():
                setattr(self, name, np.zeros((self.size,) + tail, dtype=dtype))
            self.picks = np.zeros((self.size, 2), dtype=np.uint32)
        else:
            import torch
            def zeros(shape, dtype):   # (uint32 tensors are made as int32 and viewed: torch's uint32 has few operators)
                if dtype == "uint32":
                    return torch.zeros(shape, dtype=torch.int32, device=device).view(torch.uint32)
                return torch.zeros(shape, dtype=getattr(torch, dtype), device=device)
            for name, (tail, dtype) in FIELDS.items():
                setattr(self, name, zeros((self.size,) + tail, dtype))
            self.picks = zeros((self.size, 2), "uint32")

    def _ptr(self, t):
        return t.ctypes.data if self.device is None else t.data_ptr()

    def pointers(self):
        """The oakgpu_encoded_frames of these tensors."""
        return _lib.EncodedFrames(**{name: self._ptr(getattr(self, name)) for name in FIELDS})

    def clear(self):
        if self.device is not None:
            import torch
        for name in FIELDS:
            t = getattr(self, name)
            if self.device is None:
                t.fill(0)
            else:
                (t.view(torch.int32) if t.dtype == torch.uint32 else t).zero_()


# name -> (shape behind the row axis, dtype): the reference's OutputBuffer fields (py/battle/output.h), then k / choices / status / where
EVAL_FIELDS = {"value": ((1,), "float32"), "policy_logit": ((2, 9), "float32"), "policy": ((2, 9), "float32"), "k": ((2,), "uint8"),
               "choices": ((2, 9), "uint8"), "status": ((), "uint8"), "where": ((), "uint32")}
STATE_FIELDS = {"battles": ((384,), "uint8"), "durations": ((8,), "uint8"), "results": ((), "uint8"), "p1_choices": ((9,), "uint8"),
                "p1_counts": ((), "uint8"), "p2_choices": ((9,), "uint8"), "p2_counts": ((), "uint8"), "status": ((), "uint8"), "where": ((), "uint32")}


class CorpusOutput:
    """`size` rows of a corpus evaluation: value [F,1], policy_logit [F,2,9], policy [F,2,9] (the reference's OutputBuffer names and
    shapes), k [F,2], choices [F,2,9], status [F], where [F], and picks [F,2] (record, frame) filled on the host."""

    def __init__(self, size, device=None):
        self.size, self.device = int(size), device
        if device is None:
            for name, (tail, dtype) in EVAL_FIELDS.items():
                setattr(self, name, np.zeros((self.size,) + tail, dtype=dtype))
        else:
            import torch
            for name, (tail, dtype) in EVAL_FIELDS.items():
                if dtype == "uint32":
                    t = torch.zeros((self.size,) + tail, dtype=torch.int32, device=device).view(torch.uint32)
                else:
                    t = torch.zeros((self.size,) + tail, dtype=getattr(torch, dtype), device=device)
                setattr(self, name, t)
        self.picks = np.zeros((self.size, 2), dtype=np.uint32)

    def _ptr(self, t):
        return t.ctypes.data if self.device is None else t.data_ptr()

    def pointers(self, row=0):
        """The oakgpu_corpus_eval of these tensors from row `row` on."""
        def at(name):
            t = getattr(self, name)
            tail, dtype = EVAL_FIELDS[name]
            return self._ptr(t) + row * int(np.prod(tail, dtype=np.int64)) * np.dtype(dtype).itemsize
        return _lib.CorpusEval(**{name: at(name) for name in EVAL_FIELDS})


class _Bracket:
    """The context's stream ordered behind torch's current stream for the call, and torch's behind it afterwards."""

    def __init__(self, ctx, enc):
        self.ctx, self.enc = ctx, enc

    def __enter__(self):
        if self.enc.device is not None:
            import torch
            self.mine = torch.cuda.ExternalStream(self.ctx.stream_ptr(), device=self.enc.device)
            self.theirs = torch.cuda.current_stream(self.enc.device)
            self.mine.wait_stream(self.theirs)

    def __exit__(self, *exc):
        if self.enc.device is not None:
            self.theirs.wait_stream(self.mine)


class FrameCorpus:
    """`.battle.data` records on the device.  data_or_paths: a bytes-like of records, or a list of file paths (read in pieces that end on
    record boundaries; a file's bytes behind a record whose length cannot be trusted are left out).  info(): records, malformed, frames,
    stopped_at."""

    def __init__(self, ctx, data_or_paths, chunk_bytes=64 << 20):
        if isinstance(data_or_paths, (bytes, bytearray, memoryview)):
            data = bytes(data_or_paths)
        else:
            from .frames import _whole_records
            pieces = []
            for path in data_or_paths:
                with open(path, "rb") as f:
                    pieces += [piece for _, piece in _whole_records(f, chunk_bytes) if piece]
            data = b"".join(pieces)
        self.ctx = ctx
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
        h = C.c_void_p()
        _lib.check(ctx.lib.oakgpu_corpus_create(ctx.handle, buf.ctypes.data_as(C.c_void_p), len(data), C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.oakgpu_corpus_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        st = _lib.CorpusStats()
        _lib.check(self.ctx.lib.oakgpu_corpus_info(self.handle, C.byref(st)))
        return {"records": int(st.records), "malformed": int(st.malformed), "frames": int(st.frames), "stopped_at": int(st.stopped_at)}

    def encode(self, enc, picks):
        """Rows 0 .. len(picks)-1 of enc from picks (n x 2: record, frame).  Returns the number of OK rows."""
        lib, n = self.ctx.lib, len(picks)
        assert n <= enc.size
        ptrs = enc.pointers()
        if enc.device is None:
            enc.picks[:n] = np.asarray(picks, dtype=np.uint32).reshape(n, 2)
            ok = C.c_uint32(0)
            _lib.check(lib.oakgpu_frames_encode(self.ctx.handle, self.handle, enc.picks.ctypes.data, n, C.byref(ptrs), C.byref(ok)))
            return int(ok.value)
        import torch
        if not torch.is_tensor(picks):   # (copied as int32 bit patterns: torch's uint32 has few operators)
            picks = torch.from_numpy(np.ascontiguousarray(np.asarray(picks, dtype=np.uint32).reshape(n, 2)).view(np.int32))
        elif picks.dtype == torch.uint32:
            picks = picks.view(torch.int32)
        enc.picks.view(torch.int32)[:n].copy_(picks.reshape(n, 2))
        with _Bracket(self.ctx, enc):
            _lib.check(lib.oakgpu_frames_encode_dev(self.ctx.handle, self.handle, enc.picks.data_ptr(), n, C.byref(ptrs)))
        return int((enc.status[:n] == 0).sum())

    def sample(self, enc, seed, max_battle_length=0, min_iterations=1, n=None, count_ok=True):
        """n (default: enc.size) draws of pyoak.sample's rule into enc (and enc.picks); draw i depends on seed + i alone.  Returns the
        number of OK rows (all of them on a corpus that passes the replay check); count_ok=False on device tensors returns None and
        does not wait for the device (a training loop: the trainer leaves out the rows that are not OK itself)."""
        lib, n = self.ctx.lib, enc.size if n is None else int(n)
        assert n <= enc.size
        ptrs = enc.pointers()
        args = (n, int(seed) & (2 ** 64 - 1), int(max_battle_length), int(min_iterations), enc._ptr(enc.picks), C.byref(ptrs))
        if enc.device is None:
            ok = C.c_uint32(0)
            _lib.check(lib.oakgpu_frames_sample(self.ctx.handle, self.handle, *args, C.byref(ok)))
            return int(ok.value)
        with _Bracket(self.ctx, enc):
            _lib.check(lib.oakgpu_frames_sample_dev(self.ctx.handle, self.handle, *args))
        return int((enc.status[:n] == 0).sum()) if count_ok else None


    # ---- every frame of the corpus --------------------------------------------------------------------------------------------
    def frame_bases(self):
        """uint64[records + 1]: record r owns rows bases[r] .. bases[r+1]-1 (a malformed record owns none)."""
        bases = np.zeros(self.info()["records"] + 1, dtype=np.uint64)
        _lib.check(self.ctx.lib.oakgpu_corpus_frame_bases(self.handle, bases.ctypes.data))
        return bases

    def chunks(self, chunk_rows=0, first=0, n=None):
        """The record ranges an evaluation with chunk_rows walks: list of (first record, records) covering records first .. first+n-1."""
        bases = self.frame_bases()
        n = len(bases) - 1 - first if n is None else int(n)
        frames = np.diff(bases)[first:first + n]
        if len(frames) and int(frames.max()) > 0xFFFF:
            raise _lib.OakGpuError("a record holds at most 65,535 frames")
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        count = C.c_uint32(0)
        lib = self.ctx.lib
        _lib.check(lib.oakgpu_corpus_chunks(frames.ctypes.data, None, n, int(chunk_rows), None, 0, C.byref(count)))
        firsts = np.zeros(count.value + 1, dtype=np.uint32)
        _lib.check(lib.oakgpu_corpus_chunks(frames.ctypes.data, None, n, int(chunk_rows), firsts.ctypes.data, len(firsts), C.byref(count)))
        return [(first + int(firsts[i]), int(firsts[i + 1] - firsts[i])) for i in range(count.value)]

    def states(self, first, n, rows_capacity=None):
        """The state in front of every frame of records first .. first+n-1 (numpy, by name: STATE_FIELDS).  rows_capacity: what the
        arrays may hold (default: exactly the rows of the range)."""
        bases = self.frame_bases()
        rows = int(bases[first + n] - bases[first]) if first + n < len(bases) else 0
        cap = rows if rows_capacity is None else int(rows_capacity)
        out = {name: np.zeros((min(rows, cap),) + tail, dtype=dtype) for name, (tail, dtype) in STATE_FIELDS.items()}
        _lib.check(self.ctx.lib.oakgpu_corpus_states(self.ctx.handle, self.handle, int(first), int(n), cap, *[out[name].ctypes.data for name in STATE_FIELDS]))
        return out

    def inference(self, net, records=None, chunk_rows=0, device=None):
        """The network on every frame of the corpus, or of records = (first, n): a CorpusOutput (numpy, or torch tensors on `device`)."""
        bases = self.frame_bases()
        first, n = (0, len(bases) - 1) if records is None else (int(records[0]), int(records[1]))
        if first + n > len(bases) - 1:
            raise _lib.OakGpuError("inference: records %d .. %d are not all in the corpus" % (first, first + n))
        rows = int(bases[first + n] - bases[first])
        out = CorpusOutput(rows, device)
        frames = np.diff(bases)[first:first + n].astype(np.int64)
        out.picks[:, 0] = np.repeat(np.arange(first, first + n, dtype=np.int64), frames)
        out.picks[:, 1] = np.arange(rows, dtype=np.int64) - np.repeat(bases[first:first + n].astype(np.int64) - int(bases[first]), frames)
        lib = self.ctx.lib
        if device is None:
            ptrs = out.pointers()
            _lib.check(lib.oakgpu_corpus_inference(self.ctx.handle, net.handle, self.handle, first, n, int(chunk_rows), C.byref(ptrs)))
            return out
        with _Bracket(self.ctx, out):
            for f, k in self.chunks(chunk_rows, first, n):
                row, crows = int(bases[f] - bases[first]), int(bases[f + k] - bases[f])
                ptrs = out.pointers(row)
                _lib.check(lib.oakgpu_corpus_inference_dev(self.ctx.handle, net.handle, self.handle, f, k, crows, C.byref(ptrs)))
        return out

    def evaluate(self, net, value_nash_weight, value_empirical_weight, value_score_weight, p_nash_weight, min_iterations=1, chunk_rows=0,
                 per_record=False):
        """battle.py's loss terms over the whole corpus: {"mse", "ce_p1", "ce_p2", "sq_err", "ce1", "ce2" (the sums), "rows", "excluded"
        (for their iterations), "failed" (rows that are not OK)}; per_record=True adds "records": the same per record."""
        p = _lib.LossParams(float(value_nash_weight), float(value_empirical_weight), float(value_score_weight), float(p_nash_weight), int(min_iterations))
        total = _lib.CorpusLosses()
        per = (_lib.CorpusLosses * max(self.info()["records"], 1))() if per_record else None
        _lib.check(self.ctx.lib.oakgpu_corpus_evaluate(self.ctx.handle, net.handle, self.handle, C.byref(p), int(chunk_rows), C.byref(total), per))
        as_dict = lambda l: {name: getattr(l, name) for name, _ in _lib.CorpusLosses._fields_}
        out = as_dict(total)
        if per_record:
            out["records"] = [as_dict(per[r]) for r in range(self.info()["records"])]
        return out


def window_check(max_records, max_bytes):
    """The host-only check (no GPU): raises OakGpuError naming what ReplayWindow would refuse."""
    _lib.check(_lib.load().oakgpu_corpus_window_check(int(max_records), int(max_bytes)))


def window_scan_host(stream, offsets):
    """The slice rule of ReplayWindow.append on host bytes (no GPU): (kinds uint8[n], frames uint16[n]); kinds: 0 dropped, 1 record,
    2 record with its malformed flag, 3 rejected."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    data = bytes(stream)
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    kinds, frames = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint16)
    _lib.check(_lib.load().oakgpu_window_scan_host(buf.ctypes.data, offsets.ctypes.data, n, kinds.ctypes.data, frames.ctypes.data))
    return kinds[:n], frames[:n]


class ReplayWindow(FrameCorpus):
    """A corpus that starts empty and keeps the newest records appended to it: at most max_records of them in at most max_bytes, the oldest
    leaving first (include/oakgpu.h: the contract).  Every FrameCorpus call on it returns what it returns on FrameCorpus(ctx, records()).

        window = ReplayWindow(ctx, 65536, 1 << 30)
        stream, offsets, *_ = forest_selfplay(ctx, teams_gpu, battle_seeds_gpu, seeds_gpu, ...)    # torch tensors on the device
        window.append(stream, offsets)                                                             # nothing goes through the host
        window.sample(enc, seed=step)"""

    def __init__(self, ctx, max_records, max_bytes):
        self.ctx, self.handle = ctx, None
        h = C.c_void_p()
        _lib.check(ctx.lib.oakgpu_corpus_create_window(ctx.handle, int(max_records), int(max_bytes), C.byref(h)))
        self.handle = h

    def append(self, data, offsets=None, chunk_bytes=64 << 20):
        """append(stream, offsets): torch uint8 / int64 GPU tensors as forest_selfplay returns them (record i = bytes offsets[i] ..
        offsets[i+1]; a slice of zero bytes is skipped).  append(bytes) or append([paths]): host bytes, cut into records by their length
        fields.  Returns stats()."""
        lib = self.ctx.lib
        if offsets is not None:
            import torch
            assert data.is_cuda and offsets.is_cuda and data.dtype == torch.uint8 and offsets.dtype in (torch.int64, torch.uint64)
            data, offsets = data.contiguous(), offsets.contiguous()
            n = int(offsets.numel()) - 1
            dev = data.device
            mine, theirs = torch.cuda.ExternalStream(self.ctx.stream_ptr(), device=dev), torch.cuda.current_stream(dev)
            mine.wait_stream(theirs)
            _lib.check(lib.oakgpu_corpus_append_dev(self.ctx.handle, self.handle, data.data_ptr(), offsets.data_ptr(), max(n, 0)))
            theirs.wait_stream(mine)   # (the tensors may be freed or rewritten once torch's stream has passed the move)
            return self.stats()
        if isinstance(data, (bytes, bytearray, memoryview)):
            pieces = [bytes(data)]
        else:
            from .frames import _whole_records
            pieces = []
            for path in data:
                with open(path, "rb") as f:
                    pieces += [piece for _, piece in _whole_records(f, chunk_bytes) if piece]
        for piece in pieces:
            buf = np.frombuffer(piece, dtype=np.uint8) if piece else np.zeros(1, np.uint8)
            _lib.check(lib.oakgpu_corpus_append(self.ctx.handle, self.handle, buf.ctypes.data, len(piece)))
        return self.stats()

    def stats(self):
        out = (C.c_uint64 * 6)()
        _lib.check(self.ctx.lib.oakgpu_corpus_window_stats(self.handle, C.byref(out)))
        return dict(zip(("records", "bytes", "appended", "evicted", "rejected", "appends"), (int(v) for v in out)))

    def records(self, device=None):
        """The surviving records back to back, as a `.battle.data` file holds them: bytes, or a torch uint8 tensor on `device`."""
        lib, size = self.ctx.lib, C.c_size_t(0)
        _lib.check(lib.oakgpu_corpus_records(self.ctx.handle, self.handle, None, 0, C.byref(size), 0))
        if device is None:
            buf = np.zeros(max(size.value, 1), np.uint8)
            _lib.check(lib.oakgpu_corpus_records(self.ctx.handle, self.handle, buf.ctypes.data, size.value, C.byref(size), 0))
            return buf[:size.value].tobytes()
        import torch
        out = torch.zeros(max(size.value, 1), dtype=torch.uint8, device=device)
        mine, theirs = torch.cuda.ExternalStream(self.ctx.stream_ptr(), device=out.device), torch.cuda.current_stream(out.device)
        mine.wait_stream(theirs)
        _lib.check(lib.oakgpu_corpus_records(self.ctx.handle, self.handle, out.data_ptr(), size.value, C.byref(size), 1))
        theirs.wait_stream(mine)
        return out[:size.value]

    def save(self, path):
        data = self.records()
        with open(path, "wb") as f:
            f.write(data)
        return len(data)


def encode_battles(ctx, battles, durations, results, enc):
    """The position encoder alone on states the caller holds on the device: torch uint8 tensors battles [n, 384], durations [n, 8],
    results [n] -> enc.pokemon, active, hp, choice_indices, k (rows 0 .. n-1; enc on the same device)."""
    assert enc.device is not None, "encode_battles works on device tensors"
    n = int(battles.shape[0])
    assert n <= enc.size and battles.is_contiguous() and durations.is_contiguous() and results.is_contiguous()
    with _Bracket(ctx, enc):
        _lib.check(ctx.lib.oakgpu_encode_battles_dev(ctx.handle, battles.data_ptr(), durations.data_ptr(), results.data_ptr(), n, enc.pokemon.data_ptr(),
                                                     enc.active.data_ptr(), enc.hp.data_ptr(), enc.choice_indices.data_ptr(), enc.k.data_ptr()))


# ---- the optimiser step ----------------------------------------------------------------------------------------------------------------
WHICH = {"parameters": 0, "gradients": 1, "m": 2, "v": 3}
GROUPS = {"trunk": 1, "value": 2, "policy": 4}
LAYERS = ("pokemon_net.fc0", "pokemon_net.fc1", "active_net.fc0", "active_net.fc1", "main_net.fc0", "main_net.fc1", "value_fc2", "value_fc3",
          "p1_policy_fc2", "p1_policy_fc3", "p2_policy_fc2", "p2_policy_fc3")
# name -> (shape behind the row axis): Trainer.forward's per-row outputs
TRAIN_OUTPUTS = {"value": (), "logits": (2, 9), "sq_err": (), "ce": (2,)}


def train_loss(value_nash_weight=0.0, value_empirical_weight=0.0, value_score_weight=1.0, p_nash_weight=0.0, value_weight=1.0, policy_weight=1.0):
    """battle.py's loss options (its defaults) as an oakgpu_train_loss; --no-value-loss / --no-policy-loss are a zero weight."""
    return _lib.TrainLoss(float(value_nash_weight), float(value_empirical_weight), float(value_score_weight), float(p_nash_weight), float(value_weight),
                          float(policy_weight))


def apply_symmetries(ctx, enc, seed, n=None, flip_sides=True, permute_bench=True):
    """battle.py's permute_sides / permute_pokemon on rows 0 .. n-1 of device tensors, in place; row i is drawn from seed + i alone.  hp moves
    with its Pokemon (the reference leaves it in place): include/oakgpu.h, oakgpu_frames_symmetries_dev."""
    assert enc.device is not None, "apply_symmetries works on device tensors"
    n = enc.size if n is None else int(n)
    assert n <= enc.size
    ptrs = enc.pointers()
    with _Bracket(ctx, enc):
        _lib.check(ctx.lib.oakgpu_frames_symmetries_dev(ctx.handle, C.byref(ptrs), n, int(seed) & (2 ** 64 - 1), int(bool(flip_sides)), int(bool(permute_bench))))


def trainer_check(net_bytes, max_rows, n=0, loss=None):
    """The host-only check (no GPU): raises OakGpuError naming what create or a call of n rows would refuse."""
    data = bytes(net_bytes)
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    _lib.check(_lib.load().oakgpu_trainer_check(buf.ctypes.data, len(data), int(max_rows), int(n), C.byref(loss) if loss is not None else None))


class Trainer:
    """Parameters, gradients and Adam state of one `.battle.net` on the device, and the optimiser step on training rows (k_gemm, k_loss, k_adam
    in oak_amd/csrc/trainer.hip; the contract is in include/oakgpu.h).  net_bytes_or_path: the bytes of a `.battle.net` or its path.

        trainer = Trainer(ctx, "initial.battle.net", max_rows=4096)
        corpus.sample(enc, seed=step)
        trainer.step(enc, enc.size, loss=train_loss(policy_weight=1.0), lr=1e-3)      # asynchronous for device rows
        trainer.report()                                                                # waits: loss, mse, ce_p1, ce_p2, rows, steps

    frames: an EncodedBattleFrames, torch tensors on the context's device (ordered against torch's current stream) or numpy (staged)."""

    def __init__(self, ctx, net_bytes_or_path, max_rows):
        if isinstance(net_bytes_or_path, (bytes, bytearray, memoryview)):
            data = bytes(net_bytes_or_path)
        else:
            with open(net_bytes_or_path, "rb") as f:
                data = f.read()
        self.ctx, self.max_rows, self.handle = ctx, int(max_rows), None
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
        h = C.c_void_p()
        _lib.check(ctx.lib.oakgpu_trainer_create(ctx.handle, buf.ctypes.data, len(data), self.max_rows, C.byref(h)))
        self.handle = h
        dims, count = (C.c_uint32 * 24)(), C.c_size_t(0)
        _lib.check(ctx.lib.oakgpu_trainer_shape(h, C.byref(dims), C.byref(count), None))
        self.dims = [(int(dims[2 * i]), int(dims[2 * i + 1])) for i in range(12)]
        self.count = int(count.value)
        self.last_groups = 0

    def close(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.oakgpu_trainer_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, frames, *args):
        lib = self.ctx.lib
        ptrs = frames.pointers()
        if frames.device is None:
            _lib.check(getattr(lib, name)(self.ctx.handle, self.handle, C.byref(ptrs), *args))
        else:
            with _Bracket(self.ctx, frames):
                _lib.check(getattr(lib, name + "_dev")(self.ctx.handle, self.handle, C.byref(ptrs), *args))

    def forward(self, frames, n, loss, want=("value", "logits", "sq_err", "ce"), out=None):
        """Forward and loss terms of rows 0 .. n-1: {name: array [n, ...]} for the names in `want` (torch on the rows' device, or numpy), and the
        report.  out: tensors to write into, by name, each of at least n rows."""
        n = int(n)
        res = {}
        for name in want:
            if out is not None and name in out:
                res[name] = out[name]
            elif frames.device is None:
                res[name] = np.zeros((n,) + TRAIN_OUTPUTS[name], dtype=np.float32)
            else:
                import torch
                res[name] = torch.zeros((n,) + TRAIN_OUTPUTS[name], dtype=torch.float32, device=frames.device)
        outs = _lib.TrainOutputs(**{name: frames._ptr(t) for name, t in res.items()})
        self._call("oakgpu_trainer_forward", frames, n, C.byref(loss), C.byref(outs))
        return res

    def gradients(self, frames, n, loss):
        """Forward and backward of rows 0 .. n-1 into the gradient block."""
        self._call("oakgpu_trainer_gradients", frames, int(n), C.byref(loss))
        self.last_groups = 1 | (2 if loss.value_weight != 0 else 0) | (4 if loss.policy_weight != 0 else 0)

    def adam(self, lr, clamp_parameters=False, groups=None):
        """The Adam update alone, from the gradient block: of `groups` (names of GROUPS or their bits; default: the groups the last gradients
        call gave a gradient)."""
        if groups is None:
            groups = self.last_groups
        elif not isinstance(groups, int):
            groups = sum(GROUPS[g] for g in groups)
        _lib.check(self.ctx.lib.oakgpu_trainer_adam_dev(self.ctx.handle, self.handle, float(lr), int(bool(clamp_parameters)), int(groups)))

    def step(self, frames, n, loss, lr, clamp_parameters=False):
        """gradients, then adam: one optimiser step on rows 0 .. n-1."""
        self._call("oakgpu_trainer_step", frames, int(n), C.byref(loss), float(lr), int(bool(clamp_parameters)))
        self.last_groups = 1 | (2 if loss.value_weight != 0 else 0) | (4 if loss.policy_weight != 0 else 0)

    def report(self):
        """Waits for the device: the last call's loss, mse, ce_p1, ce_p2, rows, and the groups' step counts."""
        rep, steps = _lib.TrainReport(), (C.c_uint64 * 3)()
        _lib.check(self.ctx.lib.oakgpu_trainer_report(self.ctx.handle, self.handle, C.byref(rep), C.byref(steps)))
        out = {name: getattr(rep, name) for name, _ in _lib.TrainReport._fields_}
        out["rows"] = int(out["rows"])
        out["steps"] = {"trunk": int(steps[0]), "value": int(steps[1]), "policy": int(steps[2])}
        return out

    def read(self, which="parameters", flat=False):
        """The parameters, "gradients", "m" or "v": a list of 12 (bias [out], weight [out, in]) pairs in file order, or the flat block."""
        block = np.zeros(self.count, dtype=np.float32)
        _lib.check(self.ctx.lib.oakgpu_trainer_read(self.ctx.handle, self.handle, WHICH[which], block.ctypes.data, self.count))
        return block if flat else self.split(block)

    def split(self, block):
        out, p = [], 0
        for i, o in self.dims:
            out.append((block[p:p + o], block[p + o:p + o + o * i].reshape(o, i)))
            p += o * (i + 1)
        return out

    def set_gradients(self, block):
        block = np.ascontiguousarray(block, dtype=np.float32).reshape(-1)
        _lib.check(self.ctx.lib.oakgpu_trainer_set_gradients(self.ctx.handle, self.handle, block.ctypes.data, block.size))

    def net_bytes(self):
        size = C.c_size_t(0)
        _lib.check(self.ctx.lib.oakgpu_trainer_net_bytes(self.ctx.handle, self.handle, None, 0, C.byref(size)))
        buf = np.zeros(size.value, dtype=np.uint8)
        _lib.check(self.ctx.lib.oakgpu_trainer_net_bytes(self.ctx.handle, self.handle, buf.ctypes.data, buf.size, C.byref(size)))
        return buf.tobytes()

    def save(self, path):
        data = self.net_bytes()
        with open(path, "wb") as f:
            f.write(data)
