"""Golden representations and scores of the REFERENCE's PoolNet (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_seq_pool_golden.py <reference checkout>

Imports spotlight/sequence/representations.py read-only from the reference checkout, seeds torch,
builds PoolNet(num_items = 23, embedding_dim = 8) with the reference's own init, gives the biases
random values (its ZeroEmbedding starts them at zero, which would leave the bias term untested;
the padding row stays zero) and records, float32 on the CPU: E, b, left-padded sequences (full
length, leading padding, a single item, a repeated item), targets of the same shape, both results
of user_representation (every position [n, d, L] and the final one [n, d]) and forward(all
representations, targets) [n, L]: seq_pool_d8.npz (arrays only).  This script and the reference
never run on the GPU box; the fixture is what travels (tests/test_seq_cpu.py, test_seq_gpu.py).
"""
import os
import sys

import numpy as np
import torch

REF = sys.argv[1]
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

NUM_ITEMS, DIM, L = 23, 8, 6


def main():
    from spotlight.sequence.representations import PoolNet
    torch.manual_seed(2016)
    net = PoolNet(NUM_ITEMS, embedding_dim=DIM)
    net.eval()
    with torch.no_grad():
        net.item_biases.weight[1:].normal_(0, 0.3)
    rs = np.random.RandomState(7)
    seq = rs.randint(1, NUM_ITEMS, (7, L)).astype(np.int64)
    seq[1, :2] = 0                   # leading padding
    seq[2, :L - 1] = 0               # a single item
    seq[3, 4] = seq[3, 2]            # a repeated item
    seq[4, :3] = 0
    seq[4, 4] = seq[4, 3]            # padding and a repeat
    targets = rs.randint(1, NUM_ITEMS, (7, L)).astype(np.int64)
    targets[5] = seq[5]              # the training step's own targets: the sequence itself
    with torch.no_grad():
        every, final = net.user_representation(torch.from_numpy(seq))
        scores = net(every, torch.from_numpy(targets))
    np.savez(os.path.join(OUT, "seq_pool_d8.npz"), E=net.item_embeddings.weight.detach().numpy(),
             b=net.item_biases.weight.detach().numpy().reshape(-1), sequences=seq, targets=targets,
             representations=every.numpy(), final=final.numpy(), scores=scores.numpy())
    print("wrote seq_pool_d8.npz", every.shape, final.shape, scores.shape)


if __name__ == "__main__":
    main()
