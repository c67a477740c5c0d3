"""Golden eval-mode score blocks of the REFERENCE's MLP / NeuMF (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ncf_scores_golden.py [/root/reference]

Imports spotlight/dnn_models/mlp.py and neuMF.py read-only from the reference checkout, seeds
torch, builds a small model with the reference's own init (N(0, 1) embeddings, Xavier weights),
calls .eval() and records named_parameters() (in order, as p0, p1, ...) and net(u, i) for every
(user, item) pair: ncf_scores_<kind>_e<E>[_m<M>].npz (arrays only).  Layer sizes as
ncf_spotlight.py:53-56 / neuMF_spotlight.py: [2E, E, ..., 8].  This script and the reference
never run on the GPU box; the fixtures are what travels (tests/test_ncf_score_gpu.py).
"""
import os
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

CASES = [("mlp", 64, 0), ("mlp", 16, 0), ("neumf", 16, 50), ("neumf", 8, 5)]
U, I = 9, 97


def tower(E):
    sizes = [2 * E]
    while sizes[-1] > 8:
        sizes.append(sizes[-1] // 2)
    return sizes


def main():
    from spotlight.dnn_models.mlp import MLP
    from spotlight.dnn_models.neuMF import NeuMF
    for n, (kind, E, M) in enumerate(CASES):
        torch.manual_seed(100 + n)
        if kind == "mlp":
            net = MLP(tower(E), U, I, embedding_dim=E)
        else:
            net = NeuMF(tower(E), U, I, mf_embedding_dim=M, mlp_embedding_dim=E)
        net.eval()
        u = torch.arange(U).repeat_interleave(I)
        i = torch.arange(I).repeat(U)
        with torch.no_grad():
            s = net(u, i).reshape(U, I)
        arrays = {f"p{k}": p.detach().numpy() for k, (_, p) in enumerate(net.named_parameters())}
        names = np.array([nm for nm, _ in net.named_parameters()])
        name = f"ncf_scores_{kind}_e{E}" + (f"_m{M}" if M else "") + ".npz"
        np.savez(os.path.join(OUT, name), scores=s.numpy(), names=names, dim=np.int64(E), mf_dim=np.int64(M), **arrays)
        print(name, s.shape, float(s.min()), float(s.max()))


if __name__ == "__main__":
    main()
