"""Golden representations and scores of the REFERENCE's CNNNet (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_seq_cnn_golden.py <reference checkout>

Imports spotlight/sequence/representations.py read-only from the reference checkout and, for three
configurations at num_items = 23, embedding_dim = 16, L = 6 --
    A  kernel_width 3,         dilation 1,         1 layer,  tanh, residual
    B  kernel_width (3, 2),    dilation (1, 2),    2 layers, relu, residual
    C  kernel_width (2, 3, 3), dilation (1, 2, 4), 3 layers, tanh, no residual
-- seeds torch, builds CNNNet with the reference's own init, gives the item biases and the
convolutions' biases random values (the padding row stays zero) and records, float32 on the CPU,
on the pooling fixture's sequences and targets (seq_pool_d8.npz): the parameters (E, b and per
layer the Conv2d weight [d, d, w, 1] and bias [d]), both results of user_representation (every
position [n, d, L] and the final one [n, d]) and forward(all representations, targets) [n, L]:
seq_cnn_d16.npz (arrays only, keys prefixed by the configuration's letter).  This script and the
reference never run on the GPU box; the fixture is what travels (tests/test_seq_cnn_cpu.py,
test_seq_cnn_gpu.py).
"""
import os
import sys

import numpy as np
import torch

REF = sys.argv[1]
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

NUM_ITEMS, DIM = 23, 16
CONFIGS = {"A": dict(kernel_width=3, dilation=1, num_layers=1, nonlinearity="tanh", residual_connections=True),
           "B": dict(kernel_width=(3, 2), dilation=(1, 2), num_layers=2, nonlinearity="relu",
                     residual_connections=True),
           "C": dict(kernel_width=(2, 3, 3), dilation=(1, 2, 4), num_layers=3, nonlinearity="tanh",
                     residual_connections=False)}


def main():
    from spotlight.sequence.representations import CNNNet
    pool = np.load(os.path.join(OUT, "seq_pool_d8.npz"))
    seq, targets = pool["sequences"], pool["targets"]
    out = dict(sequences=seq, targets=targets)
    for i, (name, kw) in enumerate(sorted(CONFIGS.items())):
        torch.manual_seed(2016 + i)
        net = CNNNet(NUM_ITEMS, embedding_dim=DIM, **kw)
        net.eval()
        with torch.no_grad():
            net.item_biases.weight[1:].normal_(0, 0.3)
            for layer in net.cnn_layers:
                layer.bias.normal_(0, 0.1)
            every, final = net.user_representation(torch.from_numpy(seq))
            scores = net(every, torch.from_numpy(targets))
        out[name + "_E"] = net.item_embeddings.weight.detach().numpy()
        out[name + "_b"] = net.item_biases.weight.detach().numpy().reshape(-1)
        for l, layer in enumerate(net.cnn_layers):
            out["%s_cnn_%d_weight" % (name, l)] = layer.weight.detach().numpy()
            out["%s_cnn_%d_bias" % (name, l)] = layer.bias.detach().numpy()
        out[name + "_representations"] = every.numpy()
        out[name + "_final"] = final.numpy()
        out[name + "_scores"] = scores.numpy()
        print(name, every.shape, final.shape, scores.shape)
    np.savez(os.path.join(OUT, "seq_cnn_d16.npz"), **out)
    print("wrote seq_cnn_d16.npz")


if __name__ == "__main__":
    main()
