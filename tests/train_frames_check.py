"""Child process of tests/test_gpu_train_frames.py: oak_amd.train on torch tensors (torch initialises the GPU first).  sample and encode
into EncodedBattleFrames(size, "cuda:0") equal the staged host-pointer path bit for bit; encode_battles on device states equals the
numpy restatement.  Prints "train frames ok"."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    import oracle_lib as O
    import policy_ref as P
    import replay_oracle as R
    import train_ref as T
    from oak_amd.engine import Context
    from oak_amd.train import FIELDS, EncodedBattleFrames, FrameCorpus, encode_battles
    b, _, _, _ = O.make_random_ou_batch(6, seed0=0x5EED0000)
    games = [R.play_random_game(b[i], seed=i) for i in range(6)]
    recs = [R.make_record(g[0], g[1], g[2]) for g in games]
    tref = T.Corpus(recs)
    ctx = Context(0)
    corpus = FrameCorpus(ctx, b"".join(recs))
    n = 300
    host, gpu = EncodedBattleFrames(n), EncodedBattleFrames(n, dev)
    for name in FIELDS:
        getattr(gpu, name).fill_(1) if getattr(gpu, name).dtype != torch.uint32 else getattr(gpu, name).view(torch.int32).fill_(1)
    assert corpus.sample(host, 9, 0, 0) == n and corpus.sample(gpu, 9, 0, 0) == n
    torch.cuda.synchronize()
    assert (gpu.picks.cpu().numpy() == host.picks).all() and (host.picks == tref.draws(n, 9, 0, 0)).all()
    for name in FIELDS:
        assert getattr(gpu, name).cpu().numpy().tobytes() == getattr(host, name).tobytes(), name
    picks = np.array([(r, f) for r in range(2) for f in range(tref.frames(r))][:n], dtype=np.uint32)
    m = len(picks)
    assert corpus.encode(gpu, picks) == m and corpus.encode(host, picks) == m
    assert corpus.encode(gpu, torch.from_numpy(picks.astype(np.int64)).to(dev)) == m
    exp = tref.expected(picks)
    for name in FIELDS:
        assert getattr(gpu, name)[:m].cpu().numpy().tobytes() == exp[name].tobytes(), name
    sb, sd, sr = P.batch_of(500, seed=3)
    enc = EncodedBattleFrames(500, dev)
    encode_battles(ctx, torch.from_numpy(sb).to(dev), torch.from_numpy(sd).to(dev), torch.from_numpy(sr).to(dev), enc)
    want = T.encode_states(sb, sd, sr)
    for name in T.POSITION_FIELDS:
        assert getattr(enc, name).cpu().numpy().tobytes() == want[name].tobytes(), name
    corpus.close()
    ctx.close()
    print("train frames ok")


if __name__ == "__main__":
    main()
