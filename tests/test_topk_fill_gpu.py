"""rg_topk_rows on rows with fewer than k finite scores: the -inf (excluded) and NaN entries fill the
rest of the top-k by ascending item id, so every row still gets k distinct ids inside the table.
recommend relies on it for a user with fewer than k items left.  (A -inf entry enters a list on its
id alone, against the filler the lists start from; that path lost the entry and the filler's id,
INT_MAX, came out.)  Reference: numpy's stable argsort with NaN as -inf, no tolerance."""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib

pytestmark = pytest.mark.gpu


def device_topk(x, k):
    s = torch.as_tensor(x, device="cuda:0").contiguous()
    out = torch.full((s.shape[0], k), -7, dtype=torch.int32, device="cuda:0")
    _lib.check(_lib.load().rg_topk_rows(_lib.stream_handle(), _lib.ptr(s), s.shape[0], s.shape[1], s.shape[1], k,
                                        _lib.ptr(out)), "rg_topk_rows")
    return out.cpu().numpy()


# k on both sides of the kernel's list lengths (8, 16, 32); cols below, at and above one pass of its
# 256 threads, and k == cols
@pytest.mark.parametrize("cols,k", [(1, 1), (3, 3), (40, 1), (40, 8), (40, 10), (40, 32), (255, 9), (256, 16),
                                    (257, 17), (818, 5), (818, 32), (32, 32)])
def test_rows_short_of_k_finite_scores_are_filled_by_id(cols, k):
    rs = np.random.RandomState(cols * 37 + k)
    counts = sorted({0, 1, max(k - 2, 0), k - 1, k, min(k + 1, cols)})     # finite scores per row
    x = np.full((2 * len(counts), cols), -np.inf, dtype=np.float32)
    for r, n in enumerate(counts * 2):
        at = rs.choice(cols, n, replace=False)
        x[r, at] = rs.rand(n).astype(np.float32)
        if r >= len(counts) and cols > n:                                    # second half: a NaN among the rest
            x[r, rs.choice(np.setdiff1d(np.arange(cols), at))] = np.nan
    got = device_topk(x, k)
    key = np.where(np.isnan(x), -np.inf, x)
    ref = np.argsort(-key, axis=1, kind="stable")[:, :k]
    assert got.min() >= 0 and got.max() < cols
    assert (got == ref).all()
    assert all(len(set(row)) == k for row in got.tolist())
