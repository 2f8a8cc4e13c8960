"""Child process of tests/test_gpu_corpus_eval.py: FrameCorpus.inference on torch tensors (torch initialises the GPU first).  The
tensors on "cuda:0" equal the staged host-pointer path bit for bit, at the default chunk size and at one that cuts the corpus into
several chunks.  Prints "corpus eval ok"."""
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
    import corpus_eval_ref as CE
    import policy_ref as P
    from oak_amd.engine import Context, Network
    from oak_amd.train import EVAL_FIELDS, FrameCorpus
    games, recs = CE.world()
    ctx = Context(0)
    corpus = FrameCorpus(ctx, b"".join(recs))
    net = Network(ctx, path=P.GOLDEN["default"])
    host = corpus.inference(net)
    longest = int(np.diff(corpus.frame_bases()).max())
    for chunk_rows in (0, longest):
        gpu = corpus.inference(net, chunk_rows=chunk_rows, device=dev)
        torch.cuda.synchronize()
        assert gpu.value.is_cuda and tuple(gpu.value.shape) == host.value.shape and tuple(gpu.policy.shape) == host.policy.shape
        for name in EVAL_FIELDS:
            t = getattr(gpu, name)
            t = t.view(torch.int32) if t.dtype == torch.uint32 else t
            assert t.cpu().numpy().tobytes() == getattr(host, name).tobytes(), (chunk_rows, name)
        assert (gpu.picks == host.picks).all()
    losses = corpus.evaluate(net, 0.25, 0.25, 0.5, 0.25)
    assert losses["rows"] > 0 and np.isfinite(losses["mse"]) and losses["failed"] > 0
    print("corpus eval ok")


if __name__ == "__main__":
    main()
