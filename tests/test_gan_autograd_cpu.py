"""oracle/gan.py's hand-derived backward against float64 autograd, at the kinds of shape the
goldens do not have: E > 8, a batch that is no multiple of anything (37) and a tiny one (5),
histories with an all-padding row, a full row, a repeated item and an item in every row.

The forward is restated here with plain float64 torch ops from the module definitions
(cGAN_models.py generator / discriminator; CGANs.py D and G iterations): padded embedding
sum, cat, LeakyReLU(0.2), Linear, train-mode BatchNorm by its formula, the recorded dropout
masks times the scale, tanh heads; D's three Linear + Dropout + LeakyReLU layers and its output
layer; the clamp before a D step.  Autograd differentiates it.  Both sides are float64 and each
quantity is a sum of fewer than 1e4 terms through at most eight layers, so every tensor agrees
within 1e-10 of its largest magnitude.

The two Linear biases feeding a BatchNorm are the one place where "the tensor's largest
magnitude" is not a scale: their exact gradient is 0 (the batch mean removes the bias), so both
sides hold only the rounding residue of sum_b dy[b] (1e-20 here) and the ratio of two residues
means nothing.  They are held to 1e-10 of what a sum that cancels is measured against, the sum
of its terms' magnitudes max_c sum_b |dy[b, c]| (autograd's own dy), on each side separately:
a wrong bias gradient is of that order, not 1e-10 of it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gan as og
from tests.gan_common import (DROP_SCALES, d_step_widths, edge_histories, f64, g_step_widths, noise, random_gan,
                              scale_d)

N, S, H, E, Z, L = 20, 3, 16, 12, 10, 6
RTOL = 1e-10


def t64(x, grad=False):
    return torch.tensor(np.asarray(x, np.float64), dtype=torch.float64, requires_grad=grad)


def emb_sum(W, hist):
    return F.embedding(torch.from_numpy(hist), W, padding_idx=N).sum(1)


def g_forward(G, z, hist, masks, scale, keep):
    """Train-mode generator; returns (fake (B, S*N), new running stats); the pre-BatchNorm
    Linear outputs are kept in ``keep`` (with their gradients) for the bias bound."""
    a = F.leaky_relu(torch.cat([z, emb_sum(G["embedding_layer.weight"], hist)], 1), og.LRELU)
    B, stats = z.shape[0], {}
    for k, (lin, bn) in enumerate((("layers.0", "layers.1"), ("layers.4", "layers.5"))):
        y = a @ G[lin + ".weight"].t() + G[lin + ".bias"]
        if y.requires_grad:
            y.retain_grad()
            keep[lin + ".bias"] = y
        mu = y.mean(0)
        var = ((y - mu) ** 2).mean(0)
        with torch.no_grad():
            stats[bn + ".running_mean"] = (1 - og.BN_MOMENTUM) * G[bn + ".running_mean"] + og.BN_MOMENTUM * mu
            stats[bn + ".running_var"] = (1 - og.BN_MOMENTUM) * G[bn + ".running_var"] + \
                og.BN_MOMENTUM * var * B / (B - 1)
        o = (y - mu) / torch.sqrt(var + og.BN_EPS) * G[bn + ".weight"] + G[bn + ".bias"]
        a = F.leaky_relu(o * masks[k] * scale, og.LRELU)
    heads = [torch.tanh(a @ G[f"mult_heads.head_{s}.weight"].t() + G[f"mult_heads.head_{s}.bias"]) for s in range(S)]
    return torch.cat(heads, 1), stats


def d_forward(D, slate, hist, masks, scale):
    h = torch.cat([emb_sum(D["embedding_layer.weight"], hist), slate], 1)
    for k, lin in enumerate(("layers.0", "layers.3", "layers.6")):
        h = F.leaky_relu((h @ D[lin + ".weight"].t() + D[lin + ".bias"]) * masks[k] * scale, og.LRELU)
    return h @ D["layers.9.weight"].t() + D["layers.9.bias"]


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    assert err <= RTOL * scale, f"{what}: max |oracle - autograd| {err:.3e}, scale {scale:.3e}"


def grads_close(oracle_grads, params, keep, what):
    for k, p in params.items():
        ref = p.grad.numpy()
        if k in keep:       # pre-BatchNorm bias: exact gradient 0, see the module docstring
            bound = RTOL * float(keep[k].grad.abs().sum(0).max())
            a, b = np.abs(ref).max(), np.abs(oracle_grads[k]).max()
            assert bound > 0 and a <= bound and b <= bound, \
                f"{what} {k}: autograd {a:.3e}, oracle {b:.3e}, bound {bound:.3e}"
        else:
            close(oracle_grads[k], ref, f"{what} grad {k}")


def params_of(sd, grad):
    return {k: t64(v, grad) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


@pytest.mark.parametrize("B", [37, 5])
def test_gan_oracle_matches_autograd(B):
    gs, ds = random_gan(N, S, H, E, Z, 21)
    # D scaled to max |x| = 0.02: about half of every tensor lies beyond the +-0.01 clamp, so the
    # clamp is part of what is compared (the gradient is taken at the clamped values)
    ds = scale_d(ds, 0.02)
    o = og.GANOracle({k: v.numpy() for k, v in gs.items()}, {k: v.numpy() for k, v in ds.items()}, N, S, H, E, Z,
                     opt="rms", lr=1e-4)
    rs = np.random.RandomState(100 + B)
    hist = edge_histories(rs, B, N, L)
    assert (hist[0] == N).all() and (hist[1] != N).all() and len(set(hist[2, :3])) == 2 and (hist[1:] == 3).any(1).all()
    slates = np.stack([rs.choice(N, S, replace=False) for _ in range(B)])
    sg, sd = DROP_SCALES
    buffers = ("layers.1.running_mean", "layers.1.running_var", "layers.5.running_mean", "layers.5.running_var")

    # ---- D iteration: clamp, D(real one-hot), G(z) in train mode, D(fake.detach())
    z, mk = noise(rs, B, Z, d_step_widths(H))
    assert (np.abs(o.D["layers.3.weight"]) > og.CLAMP).mean() > 0.3
    Gt = params_of(o.G, False)
    Dt = {k: t64(np.clip(v, -og.CLAMP, og.CLAMP), True) for k, v in o.D.items()}
    loss, d_real, d_fake, fake = o.d_step(hist, slates, z.astype(np.float64), f64(mk), DROP_SCALES)
    tm = [t64(m) for m in mk]
    one_hot = torch.zeros(B, S * N, dtype=torch.float64)
    for s in range(S):
        one_hot[torch.arange(B), s * N + torch.from_numpy(slates[:, s])] = 1.0
    t_fake, stats = g_forward(Gt, t64(z), hist, tm[3:5], sg, {})
    t_real = d_forward(Dt, one_hot, hist, tm[0:3], sd)
    t_dfake = d_forward(Dt, t_fake.detach(), hist, tm[5:8], sd)
    t_loss = t_dfake.mean() - t_real.mean()
    t_loss.backward()
    close(loss, t_loss.item(), "d_loss")
    close(d_real, t_real.detach().numpy(), "D(real)")
    close(d_fake, t_dfake.detach().numpy(), "D(fake)")
    close(fake, t_fake.detach().numpy(), "G(z)")
    grads_close(o.last_grads, Dt, {}, "D step")
    assert not o.last_grads["embedding_layer.weight"][N].any() and not Dt["embedding_layer.weight"].grad[N].any()
    for k in buffers:
        close(o.G[k], stats[k].numpy(), f"D step {k}")
    assert int(o.G["layers.1.num_batches_tracked"]) == 1 and int(o.G["layers.5.num_batches_tracked"]) == 1

    # ---- G iteration on the stepped D: G(z) -> D (frozen, train-mode dropout) -> -mean
    z, mk = noise(rs, B, Z, g_step_widths(H))
    Gt = params_of(o.G, True)
    for k in buffers:
        Gt[k].requires_grad_(False)
    Dt = params_of(o.D, False)
    gloss, gd_fake, _ = o.g_step(hist, z.astype(np.float64), f64(mk), DROP_SCALES)
    tm = [t64(m) for m in mk]
    keep = {}
    t_fake, stats = g_forward(Gt, t64(z), hist, tm[0:2], sg, keep)
    t_dfake = d_forward(Dt, t_fake, hist, tm[2:5], sd)
    t_loss = -t_dfake.mean()
    t_loss.backward()
    close(gloss, t_loss.item(), "g_loss")
    close(gd_fake, t_dfake.detach().numpy(), "D(G(z))")
    grads_close(o.last_grads, {k: v for k, v in Gt.items() if k not in buffers}, keep, "G step")
    assert set(o.last_grads) == set(o.g_params)
    assert not o.last_grads["embedding_layer.weight"][N].any() and not Gt["embedding_layer.weight"].grad[N].any()
    for k in buffers:
        close(o.G[k], stats[k].numpy(), f"G step {k}")
    assert int(o.G["layers.1.num_batches_tracked"]) == 2 and int(o.G["layers.5.num_batches_tracked"]) == 2
