"""Sequence representations as torch modules: the CPU statement of what the device kernels
compute, and what ``ImplicitSequenceModel(representation=<net>)`` takes its configuration and
initial parameters from.

``CNNNet`` is the stacked causal dilated convolution (WaveNet / ByteNet style) of the reference's
spotlight/sequence/representations.py: parameter names and shapes are the reference's
(``item_embeddings``, ``item_biases``, ``cnn_i`` as ``nn.Conv2d(d, d, (w, 1), dilation=(D, 1))``), so
one of its ``state_dict``s loads here.  include/rg_hip.h (rg_seq_cnn_grads) states the same model
position by position."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..layers import ScaledEmbedding, ZeroEmbedding

PADDING_IDX = 0
NONLINEARITIES = ("tanh", "relu")


def _per_layer(val, num):
    """An int stands for every layer; a sequence is taken as given."""
    try:
        return tuple(int(v) for v in val)
    except TypeError:
        return (int(val),) * num


class CNNNet(nn.Module):
    """x_t of the top layer represents the items before position t; ``kernel_width`` and
    ``dilation`` are one int for every layer or one per layer."""

    def __init__(self, num_items, embedding_dim=32, kernel_width=3, dilation=1, num_layers=1, nonlinearity="tanh",
                 residual_connections=True, item_embedding_layer=None):
        super().__init__()
        if nonlinearity not in NONLINEARITIES:
            raise ValueError("Nonlinearity must be one of (tanh, relu)")
        if int(num_layers) < 1:
            raise ValueError("num_layers must be at least 1")
        self.num_items = int(num_items)
        self.embedding_dim = int(embedding_dim)
        self.num_layers = int(num_layers)
        self.kernel_width = _per_layer(kernel_width, self.num_layers)
        self.dilation = _per_layer(dilation, self.num_layers)
        if len(self.kernel_width) != self.num_layers or len(self.dilation) != self.num_layers:
            raise ValueError("kernel_width and dilation need one value per layer")
        if min(self.kernel_width) < 1 or min(self.dilation) < 1:
            raise ValueError("kernel widths and dilations must be at least 1")
        self.nonlinearity_name = nonlinearity
        self.nonlinearity = torch.tanh if nonlinearity == "tanh" else F.relu
        self.residual_connections = bool(residual_connections)
        if item_embedding_layer is not None:
            self.item_embeddings = item_embedding_layer
        else:
            self.item_embeddings = ScaledEmbedding(self.num_items, self.embedding_dim, padding_idx=PADDING_IDX)
        self.item_biases = ZeroEmbedding(self.num_items, 1, padding_idx=PADDING_IDX)
        for i, (w, dil) in enumerate(zip(self.kernel_width, self.dilation)):
            self.add_module("cnn_{}".format(i), nn.Conv2d(self.embedding_dim, self.embedding_dim, (w, 1),
                                                          dilation=(dil, 1)))

    @property
    def cnn_layers(self):
        return [getattr(self, "cnn_{}".format(i)) for i in range(self.num_layers)]

    def user_representation(self, item_sequences):
        """(x_0 .. x_{L-1} as [n, d, L], x_L as [n, d]) of left-padded sequences [n, L]."""
        emb = self.item_embeddings(item_sequences).permute(0, 2, 1).unsqueeze(3)    # [n, d, L, 1]
        layers = self.cnn_layers
        # one zero row for "nothing seen yet" and the taps' reach in front of it
        x = F.pad(emb, (0, 0, 1 + (self.kernel_width[0] - 1) * self.dilation[0], 0))
        x = self.nonlinearity(layers[0](x))
        if self.residual_connections:
            x = x + F.pad(emb, (0, 0, 1, 0))
        for layer, w, dil in zip(layers[1:], self.kernel_width[1:], self.dilation[1:]):
            residual = x
            x = self.nonlinearity(layer(F.pad(x, (0, 0, (w - 1) * dil, 0))))
            if self.residual_connections:
                x = x + residual
        x = x.squeeze(3)
        return x[:, :, :-1], x[:, :, -1]

    def forward(self, user_representations, targets):
        """Scores [n, L] of ``targets`` [n, L] under representations [n, d, L]."""
        target_embedding = self.item_embeddings(targets).permute(0, 2, 1)
        target_bias = self.item_biases(targets).squeeze(-1)
        return target_bias + (user_representations * target_embedding).sum(1)
