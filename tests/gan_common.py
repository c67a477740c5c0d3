"""Input builders shared by the cGAN tests (CPU and GPU): reference-shaped random state
dicts, histories and real slates with the edge rows the kernels take their own paths for,
recorded noise (z and dropout masks) and the float32-rounded dropout scales."""
import numpy as np
import torch

from oracle import gan as og

# torch's noise.div_(1 - p) in float32, as make_golden.gan_case records them (G 0.1, D 0.3)
DROP_SCALES = (float(np.float32(1) / np.float32(0.9)), float(np.float32(1) / np.float32(0.7)))
# learning rates of make_golden.gan_case per optimizer
GOLDEN_LR = {"rms": 1e-4, "adam": 1e-4, "sgd": 1e-2}


def random_gan(N, S, H, E, Z, seed):
    """Reference-shaped G / D state dicts (cGAN_models.py init: xavier weights, bias 0.01,
    N(0,1) embeddings with a zero padding row, BatchNorm gamma 1 / beta 0)."""
    g = torch.Generator().manual_seed(seed)
    H1 = H // 2

    def lin(o, i):
        b = (6.0 / (i + o)) ** 0.5
        return (torch.rand(o, i, generator=g) * 2 - 1) * b, torch.full((o,), 0.01)

    def emb():
        e = torch.randn(N + 1, E, generator=g)
        e[N] = 0
        return e

    gs = {"embedding_layer.weight": emb()}
    for pre, (o, i) in (("layers.0", (H1, Z + E)), ("layers.4", (H, H1))):
        gs[pre + ".weight"], gs[pre + ".bias"] = lin(o, i)
    for pre, w in (("layers.1", H1), ("layers.5", H)):
        gs.update({pre + ".weight": torch.ones(w), pre + ".bias": torch.zeros(w), pre + ".running_mean": torch.zeros(w),
                   pre + ".running_var": torch.ones(w), pre + ".num_batches_tracked": torch.tensor(0)})
    for s in range(S):
        gs[f"mult_heads.head_{s}.weight"], gs[f"mult_heads.head_{s}.bias"] = lin(N, H)
    ds = {"embedding_layer.weight": emb()}
    for pre, (o, i) in (("layers.0", (2 * H, S * N + E)), ("layers.3", (H, 2 * H)), ("layers.6", (H1, H)),
                        ("layers.9", (1, H1))):
        ds[pre + ".weight"], ds[pre + ".bias"] = lin(o, i)
    return gs, ds


def scale_d(ds, peak=0.004):
    """Every D tensor rescaled to max |x| = peak (make_golden.gan_case, C4's scaled_d): at 0.004
    the +-0.01 clamp does not bind and no pre-activation sits on the LeakyReLU kink."""
    return {k: v * (peak / max(float(v.abs().max()), 1e-30)) for k, v in ds.items()}


def hist_and_slates(rs, rows, N, S, L):
    hist = np.full((rows, L), N, np.int64)
    for r in range(rows):
        ln = rs.randint(0, L + 1)
        hist[r, :ln] = rs.choice(N, ln, replace=False)
    slates = np.stack([rs.choice(N, S, replace=False) for _ in range(rows)])
    return hist, slates


def edge_histories(rs, rows, N, L, common=3, full_rows=(1,)):
    """(rows, L) histories padded with N.  Row 0 is all padding; the rows of ``full_rows`` have no
    padding; row 2 (when there is one) holds one item twice; every row but row 0 holds
    ``common``, so that item's group in the embedding backward has rows - 1 entries.  A row
    longer than the catalogue necessarily repeats items."""
    hist = np.full((rows, L), N, np.int64)
    others = np.setdiff1d(np.arange(N), [common])
    for r in range(1, rows):
        ln = L if r in full_rows else rs.randint(1, L)
        row = np.concatenate([[common], rs.choice(others, ln - 1, replace=ln - 1 > len(others))])
        rs.shuffle(row)
        hist[r, :ln] = row
    if rows > 2:
        twice = int(others[rs.randint(len(others))])
        hist[2] = N
        hist[2, :3] = [twice, common, twice]
    return hist


def edge_slates(rs, rows, N, S, shared=17):
    """(rows, S) real slates, S >= 3 and N > 128, whose one-hot columns sit where the sorted hits
    are cut: head 0 holds items 127 and 128 in rows 0 and 1 (either side of the first
    128-column tile edge); row 0 holds item N - 1 in the last head (the last real column, next
    to the ks padding); row 1 holds item 0 in head 1 and row 2 item N - 1 in head 0 (either
    side of a head boundary); rows 3..110 share ``shared`` at position 1 (one column hit by
    more rows than a wave has lanes, once the batch has that many rows)."""
    sl = np.stack([rs.choice(N, S, replace=False) for _ in range(rows)]).astype(np.int64)
    sl[0, 0], sl[0, S - 1] = 127, N - 1
    sl[1, 0], sl[1, 1] = 128, 0
    if rows > 2:
        sl[2, 0] = N - 1
    sl[3:110, 1] = shared
    return sl


def noise(rs, rows, Z, widths):
    """z (rows, Z) float32 and one uint8 keep-mask per (width, drop probability)."""
    z = rs.rand(rows, Z).astype(np.float32)
    return z, [(rs.rand(rows, w) >= p).astype(np.uint8) for w, p in widths]


def d_step_widths(H):
    """The D iteration's dropout draws in the reference's call order: D(real) x3, G x2, D(fake) x3."""
    d, g = [(w, 0.3) for w in og.d_hidden(H)], [(w, 0.1) for w in og.g_hidden(H)]
    return d + g + d


def g_step_widths(H):
    """The G iteration's: G x2, D(fake) x3."""
    return [(w, 0.1) for w in og.g_hidden(H)] + [(w, 0.3) for w in og.d_hidden(H)]


def f64(arrays):
    return [np.asarray(a, np.float64) for a in arrays]
