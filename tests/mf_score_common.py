"""What the MF all-item scoring tests share (no tests here): the random tables of the float64
comparison, the float64 block, its float32 restatement, the tolerance, the exact-logit tables."""
import numpy as np

RTOL, ATOL = 1e-5, 1e-7         # the project's tolerance for a score block (tests/test_ncf_score_gpu.py)
DIMS = [1, 3, 4, 5, 8, 32, 64, 100, 128, 256]
GRID_DIMS = [16, 64]            # the dims that run the full shape grid


def random_tables(U, I, dim, seed):
    """(user_w, item_w, user_b, item_b) float32: entries N(0, 1) / sqrt(dim), biases N(0, 0.1), so
    the logits are O(1)."""
    rs = np.random.RandomState(seed)
    f = np.float32
    return ((rs.randn(U, dim) / np.sqrt(dim)).astype(f), (rs.randn(I, dim) / np.sqrt(dim)).astype(f),
            (0.1 * rs.randn(U)).astype(f), (0.1 * rs.randn(I)).astype(f))


def logits64(tabs, users, n_items=None):
    uw, iw, ub, ib = (np.asarray(t, dtype=np.float64) for t in tabs)
    return (uw[users] @ iw[:n_items].T + ub[users][:, None]) + ib[None, :n_items]


def block64(tabs, users, n_items=None):
    """float64 scores of `users` against items [0, n_items)."""
    return 1.0 / (1.0 + np.exp(-logits64(tabs, users, n_items)))


def block32_sequential(tabs, users, n_items=None):
    """The kernel's arithmetic restated in float32 on the host: one accumulator per score, k
    ascending, a fused multiply-add per k (the float64 product of two floats is exact, the sum is
    rounded to float32), then (dot + user bias) + item bias and 1 / (1 + exp(-z)) in float32."""
    uw, iw, ub, ib = tabs
    a, b = uw[users].astype(np.float64), iw[:n_items].astype(np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, k, None] * b[None, :, k]).astype(np.float32)
    z = (acc + ub[users][:, None]) + ib[None, :n_items]
    assert z.dtype == np.float32
    one = np.float32(1.0)
    return one / (one + np.exp(-z))


def exact_tables(U, I, dim=16, seed=0, equal_items=((3, 40), (3, 7), (100, 101))):
    """Entries and biases that are multiples of 1/8 in [-1/2, 1/2]: every product is a multiple of
    1/64 and every logit (|z| <= dim / 4 + 1) is exact in float32 in any summation order.  The item
    pairs of `equal_items` (those inside the table) get equal rows and biases, so their scores tie
    for every user."""
    rs = np.random.RandomState(seed)
    f = np.float32
    uw, iw = rs.randint(-4, 5, (U, dim)).astype(f) / 8, rs.randint(-4, 5, (I, dim)).astype(f) / 8
    ub, ib = rs.randint(-4, 5, U).astype(f) / 8, rs.randint(-4, 5, I).astype(f) / 8
    for x, y in equal_items:
        if x < I and y < I:
            iw[y], ib[y] = iw[x], ib[x]
    return uw, iw, ub, ib
