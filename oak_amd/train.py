"""Training batches from `.battle.data` records on the GPU: the reference's loader (pyoak.sample + EncodedBattleFrames,
cpp/src/pyoak.cc:111-245, py/battle/encoded-frames.h, py/battle/target.h) over the C ABI of include/oakgpu.h, where the contract of a
row is written down.  The records are uploaded once (FrameCorpus); a batch is replayed, encoded and written on the device
(k_frames_pick, k_frames_encode in oak_amd/csrc/trainframes.hip).  This module only holds buffers and marshals pointers.

    corpus = FrameCorpus(ctx, paths)
    enc = EncodedBattleFrames(4096, "cuda:0")          # torch tensors with the reference's attribute names and shapes
    ok = corpus.sample(enc, seed=step, max_battle_length=0, min_iterations=1)

With device=None the tensors are numpy arrays and the calls go through the staged host-pointer entry points."""
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


def encode_battles(ctx, battles, durations, results, enc):
    """The position encoder alone on states the caller holds on the device: torch uint8 tensors battles [n, 384], durations [n, 8],
    results [n] -> enc.pokemon, active, hp, choice_indices, k (rows 0 .. n-1; enc on the same device)."""
    assert enc.device is not None, "encode_battles works on device tensors"
    n = int(battles.shape[0])
    assert n <= enc.size and battles.is_contiguous() and durations.is_contiguous() and results.is_contiguous()
    with _Bracket(ctx, enc):
        _lib.check(ctx.lib.oakgpu_encode_battles_dev(ctx.handle, battles.data_ptr(), durations.data_ptr(), results.data_ptr(), n, enc.pokemon.data_ptr(),
                                                     enc.active.data_ptr(), enc.hp.data_ptr(), enc.choice_indices.data_ptr(), enc.k.data_ptr()))
