"""Shared by the rg_gan_score_slates tests: a seeded discriminator state with weights of order 0.1
(well outside the D iteration's +-0.01 clamp), slates, and the expected scores from the repo's own
``discriminator`` module on the CPU (histories: tests/gan_recommend_common.histories).

``discriminator.forward`` itself refuses CPU tensors and casts its input to float32, so
``module_forward`` runs the module's own submodules in forward's order (embedding sum, concat,
every entry of ``layers``) at the module's dtype: the same computation without the gate and the
cast, which is what a float64 reference needs."""
import numpy as np
import torch


def seeded_d(N, S, H, E, seed, scale=0.1):
    """A discriminator state dict (reference names and shapes), every tensor N(0, scale^2) from a
    seeded generator, the embedding's padding row zero."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: scale * torch.randn(*shape, generator=g)  # noqa: E731
    ds = {"embedding_layer.weight": rn(N + 1, E)}
    ds["embedding_layer.weight"][N] = 0
    for pre, (o, i) in (("layers.0", (2 * H, S * N + E)), ("layers.3", (H, 2 * H)), ("layers.6", (H // 2, H)),
                        ("layers.9", (1, H // 2))):
        ds[pre + ".weight"], ds[pre + ".bias"] = rn(o, i), rn(o)
    return ds


def d_module(ds, N, S, H, E, dtype):
    from recommendation_gans_amd.spotlight.dnn_models.cGAN_models import discriminator
    D = discriminator(num_items=N, embedding_dim=E, hidden_layers=[2 * H, H, H // 2], input_dim=S)
    D.load_state_dict(ds)
    return D.to(dtype).eval()


def one_hot(slates, N, dtype):
    """CGAN.one_hot_encoding with an all-zero block for an id outside [0, N)."""
    sl = np.asarray(slates, np.int64)
    rows, S = sl.shape
    x = torch.zeros(rows, S * N, dtype=dtype)
    for s in range(S):
        ok = np.flatnonzero((sl[:, s] >= 0) & (sl[:, s] < N))
        x[ok, s * N + sl[ok, s]] = 1
    return x


def module_forward(D, x, hist, N):
    """(scores (rows,), h3 (rows, H/2)) of the module in eval mode; history ids outside [0, N) are
    the padding id."""
    h = np.asarray(hist, np.int64)
    h = torch.from_numpy(np.where((h >= 0) & (h < N), h, N))
    with torch.no_grad():
        v = torch.cat([D.embedding_layer(h).sum(1), x], dim=1)
        for layer in list(D.layers)[:-1]:
            v = layer(v)
        return D.layers[-1](v)[:, 0], v


def expected(ds, N, S, H, E, hist, slates):
    """The float64 scores, the error measure's per-row denominator sum_k |h3_k w4_k| + |b4| from the
    float64 forward, and e0: the largest error by that measure of torch's float32 CPU forward of
    the same module on the same inputs."""
    D64 = d_module(ds, N, S, H, E, torch.float64)
    want, h3 = module_forward(D64, one_hot(slates, N, torch.float64), hist, N)
    last = D64.layers[-1]
    den = (h3.abs() @ last.weight.detach()[0].abs() + last.bias.detach().abs()).numpy()
    f32, _ = module_forward(d_module(ds, N, S, H, E, torch.float32), one_hot(slates, N, torch.float32), hist, N)
    want = want.numpy()
    e0 = float(np.max(np.abs(f32.numpy().astype(np.float64) - want) / den))
    return want, den, e0


def tolerance(e0):
    """4 e0 (another summation order in four chained layers), at least that factor times four
    layers' half-ulp."""
    return max(4 * e0, 16 * 2.0 ** -24)


def measure(got, want, den):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / den))


def slates_of(rs, rows, N, S):
    """(rows, S) int32 ids in [0, N); row 0 holds the first and the last item."""
    sl = rs.randint(0, N, (rows, S)).astype(np.int32)
    sl[0, 0], sl[0, S - 1] = 0, N - 1
    return sl
