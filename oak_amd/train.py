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
    losses = corpus.evaluate(net, 0.0, 0.5, 0.5, 0.5)  # mse, ce_p1, ce_p2, rows, excluded, failed"""
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

    def sample(self, enc, seed, max_battle_length=0, min_iterations=1, n=None):
        """n (default: enc.size) draws of pyoak.sample's rule into enc (and enc.picks); draw i depends on seed + i alone.  Returns the
        number of OK rows (all of them on a corpus that passes the replay check)."""
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
        return int((enc.status[:n] == 0).sum())


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


def encode_battles(ctx, battles, durations, results, enc):
    """The position encoder alone on states the caller holds on the device: torch uint8 tensors battles [n, 384], durations [n, 8],
    results [n] -> enc.pokemon, active, hp, choice_indices, k (rows 0 .. n-1; enc on the same device)."""
    assert enc.device is not None, "encode_battles works on device tensors"
    n = int(battles.shape[0])
    assert n <= enc.size and battles.is_contiguous() and durations.is_contiguous() and results.is_contiguous()
    with _Bracket(ctx, enc):
        _lib.check(ctx.lib.oakgpu_encode_battles_dev(ctx.handle, battles.data_ptr(), durations.data_ptr(), results.data_ptr(), n, enc.pokemon.data_ptr(),
                                                     enc.active.data_ptr(), enc.hp.data_ptr(), enc.choice_indices.data_ptr(), enc.k.data_ptr()))
