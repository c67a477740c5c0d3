"""rg_topk_rows_wide on the GPU (radix select, 1 <= k <= 1024) through the C-ABI, the model's
topk_users above k = 32, and the @k metrics routed through it.  The reference for ids is always
numpy's stable argsort of -key, key = the score with NaN replaced by -inf: the total order of
rg_topk_lists.h (key descending, column ascending), so nothing here needs a tolerance.  Values are
compared bit for bit with the block's own entries.  Padding columns hold a value above every score:
a kernel that read them would return their ids."""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib
from tests.ncf_infer_common import HostOnly, make_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 7.0e30


def wide(x, k, ld=None, values=True):
    """(ids, values) of rg_topk_rows_wide on the host block x [rows][cols], stored with row stride ld."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, cols = x.shape
    ld = cols if ld is None else ld
    buf = torch.full((rows, ld), PAD, dtype=torch.float32, device=DEV)
    buf[:, :cols] = torch.from_numpy(x).to(DEV)
    before = buf.clone()
    out = torch.full((rows, k), -7, dtype=torch.int32, device=DEV)
    val = torch.full((rows, k), -7.0, dtype=torch.float32, device=DEV) if values else None
    _lib.check(_lib.load().rg_topk_rows_wide(_lib.stream_handle(), _lib.ptr(buf), rows, cols, ld, k, _lib.ptr(out),
                                             _lib.ptr(val)), "rg_topk_rows_wide")
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the score block was written"
    return out.cpu().numpy(), (val.cpu().numpy() if values else None)


def narrow(x, k):
    s = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    out = torch.full((s.shape[0], k), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().rg_topk_rows(_lib.stream_handle(), _lib.ptr(s), s.shape[0], s.shape[1], s.shape[1], k,
                                        _lib.ptr(out)), "rg_topk_rows")
    return out.cpu().numpy()


def reference(x, k):
    key = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    return np.argsort(-key, axis=1, kind="stable")[:, :k]


def check(x, k, ld=None):
    """ids equal the reference, are distinct and inside the table; values are the block's bits."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ids, val = wide(x, k, ld)
    ref = reference(x, k)
    assert ids.min() >= 0 and ids.max() < x.shape[1]
    assert (ids == ref).all(), np.argwhere(ids != ref)[:5]
    assert all(len(set(row)) == k for row in ids.tolist())
    assert val.view(np.int32).tobytes() == np.take_along_axis(x, ref, axis=1).view(np.int32).tobytes()
    return ids


# k = 33 just past the narrow kernel; cols around one pass of 256 threads and of the 4 x 64-column
# wave segments; k == cols at the limit; k = 1024 of 1025; padded strides; more than one pass per thread
@pytest.mark.parametrize("rows,cols,k,ld", [(1, 33, 33, None), (3, 257, 33, None), (64, 777, 100, 800),
                                            (5, 1024, 1024, None), (5, 1025, 1024, 1100), (40, 5000, 50, None),
                                            (8, 20108, 1024, None)])
def test_continuous_scores_match_argsort(rows, cols, k, ld):
    rs = np.random.RandomState(rows * 7 + k)
    check(rs.randn(rows, cols).astype(np.float32), k, ld)


@pytest.mark.parametrize("k", [1, 8, 17, 32])
def test_same_ids_as_rg_topk_rows(k):
    rs = np.random.RandomState(k)
    x = rs.randn(6, 818).astype(np.float32)
    assert (wide(x, k)[0] == narrow(x, k)).all()
    # fill rows: all but a few columns -inf, a NaN among them (tests/test_topk_fill_gpu.py)
    counts = sorted({0, 1, max(k - 2, 0), k - 1, k, k + 1})
    f = np.full((len(counts), 818), -np.inf, dtype=np.float32)
    for r, n in enumerate(counts):
        at = rs.choice(818, n, replace=False)
        f[r, at] = rs.rand(n).astype(np.float32)
        f[r, rs.choice(np.setdiff1d(np.arange(818), at))] = np.nan
    got = check(f, k)
    assert (got == narrow(f, k)).all()


@pytest.mark.parametrize("k", [100, 1024])
def test_ties_at_the_threshold_take_the_lowest_columns(k):
    rs = np.random.RandomState(k)
    x = (rs.randint(0, 8, (6, 3000)) / 8.0).astype(np.float32)      # 8 levels: ~375 columns per level
    x[1] = 0.25                                                      # one value: ids 0 .. k - 1
    x[2] = np.where(rs.rand(3000) < 0.5, 1.0, rs.rand(3000) * 0.999).astype(np.float32)   # saturated at 1.0
    x[3] = -np.inf
    ids = check(x, k)
    assert (ids[1] == np.arange(k)).all() and (ids[3] == np.arange(k)).all()
    assert (np.diff(ids[2][x[2][ids[2]] == 1.0]) > 0).all()


def test_a_row_of_excluded_columns_is_filled_by_column():
    rs = np.random.RandomState(5)
    x = np.full((3, 3000), -np.inf, dtype=np.float32)
    for r in range(3):
        at = rs.choice(3000, 100, replace=False)
        x[r, at] = rs.rand(100).astype(np.float32)
    x[1, rs.choice(np.flatnonzero(np.isneginf(x[1])), 5, replace=False)] = np.nan
    ids = check(x, 500)
    for r in range(3):
        assert np.isfinite(x[r, ids[r, :100]]).all()
        rest = np.flatnonzero(~np.isfinite(x[r]))
        assert (ids[r, 100:] == rest[:400]).all()


def test_signed_zeros_are_one_key():
    rs = np.random.RandomState(9)
    x = np.zeros((2, 600), dtype=np.float32)
    x[:, 0::2] = -0.0
    at = 10 + rs.choice(580, 20, replace=False)
    x[:, at[:10]] = rs.rand(10).astype(np.float32) + 0.5
    x[:, at[10:]] = -rs.rand(10).astype(np.float32) - 0.5
    x[1] = x[1, ::-1]
    assert np.signbit(x[0, 2]) and not np.signbit(x[0, 1])
    ids = check(x, 200)                                               # 10 positives, then zeros by column
    zeros = np.flatnonzero(x[0] == 0)
    assert (ids[0, 10:] == zeros[:190]).all()
    check(x, 595)                                                     # into the negatives


def test_nan_payloads_rank_with_minus_inf():
    rs = np.random.RandomState(2)
    x = rs.rand(2, 400).astype(np.float32)
    x[:, 100:] = -np.inf
    bits = x.view(np.int32)
    for c, b in zip((3, 50, 120, 121, 250, 399),
                    (0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff)):
        bits[:, c] = np.uint32(b).astype(np.int32)
    assert np.isnan(x[:, [3, 50, 120, 121, 250, 399]]).all()
    ids, val = wide(x, 150)
    assert (ids == reference(x, 150)).all()
    assert (ids[0, :98] != 3).all() and (ids[0, 98:100] == [3, 50]).all()
    assert (ids[0, 100:104] == [100, 101, 102, 103]).all()
    assert val.view(np.int32).tobytes() == np.take_along_axis(x, ids.astype(np.int64), axis=1).view(np.int32).tobytes()
    # columns 3, 50, then 100, 101, ...: columns 120 and 121 stand at ranks 120 and 121
    assert np.isnan(val[:, [98, 99, 120, 121]]).all() and np.isneginf(val[:, 100]).all()


def test_refusals_and_the_empty_call():
    lib = _lib.load()
    s = torch.rand(4, 2000, device=DEV)
    out = torch.full((4, 1100), -7, dtype=torch.int32, device=DEV)
    st, sp, op = _lib.stream_handle(), _lib.ptr(s), _lib.ptr(out)
    assert lib.rg_topk_rows_wide(st, sp, 4, 2000, 2000, 50, None, None) != 0
    assert lib.rg_topk_rows_wide(st, None, 4, 2000, 2000, 50, op, None) != 0
    for k in (0, 1025):
        assert lib.rg_topk_rows_wide(st, sp, 4, 2000, 2000, k, op, None) != 0 and b"k must be" in lib.rg_last_error()
    assert lib.rg_topk_rows_wide(st, sp, 4, 40, 2000, 41, op, None) != 0 and b"k must be" in lib.rg_last_error()
    assert lib.rg_topk_rows_wide(st, sp, 4, 2000, 1999, 50, op, None) != 0
    assert lib.rg_topk_rows_wide(st, sp, 0, 2000, 2000, 50, op, None) == _lib.RG_OK
    torch.cuda.synchronize()
    assert (out == -7).all()                                          # nothing was launched


@pytest.mark.parametrize("kind", ["mf", "ncf"])
def test_topk_users_above_32_equals_the_stable_argsort_of_the_models_block(kind, tmp_path, monkeypatch):
    model, train, _ = make_model(kind, tmp_path, monkeypatch, U=75, I=391, n_test=10)
    users = np.array([7, 3, 70, 3, 0, 74, 12])
    csr = train.tocsr()
    blk = model.score_users(users)
    assert (model.topk_users(users, 100) == np.argsort(-blk, axis=1, kind="stable")[:, :100]).all()
    for r, u in enumerate(users):
        blk[r, csr[u].indices] = -np.inf
    got = model.topk_users(users, 100, csr)
    assert got.dtype == np.int64 and (got == np.argsort(-blk, axis=1, kind="stable")[:, :100]).all()
    assert model.topk_users(users, 391).shape == (7, 391)
    assert model.topk_users_max == 1024
    for k in (1025, 392):
        with pytest.raises(RuntimeError, match="k must be"):
            model.topk_users(users, k)


class _DeviceModel:
    """A model over fixed scores on the device whose ranking is rg_topk_rows_wide; score_users counts
    its calls (the metrics must not need it)."""
    topk_users_max = 1024

    def __init__(self, scores):
        self.s = scores.to(DEV)
        self.score_calls = 0

    def score_users(self, users):
        self.score_calls += 1
        return self.s[torch.as_tensor(np.asarray(users), device=DEV)].cpu().numpy()

    def topk_users(self, users, k, exclude_csr=None):
        sub = self.s[torch.as_tensor(np.asarray(users), device=DEV)].cpu().numpy()
        if exclude_csr is not None:
            for r, u in enumerate(users):
                sub[r, exclude_csr[u].indices] = -np.inf
        return wide(sub, k, values=False)[0].astype(np.int64)


def test_metrics_above_32_match_the_host_ranking():
    from recommendation_gans_amd.spotlight import evaluation
    from recommendation_gans_amd.spotlight.interactions import Interactions
    rs = np.random.RandomState(0)
    U, I = 300, 2000
    scores = torch.rand(U, I, generator=torch.Generator().manual_seed(1))
    m = _DeviceModel(scores)
    h = HostOnly(_DeviceModel(scores))
    test = Interactions(rs.randint(0, U, 3000), rs.randint(0, I, 3000), num_users=U, num_items=I)
    # at most 30 train items per user: k = 100 never reaches the excluded tail, whose order the host
    # path's argsort leaves unspecified
    tu = np.repeat(np.arange(U), 30)
    train = Interactions(tu, rs.randint(0, I, len(tu)), num_users=U, num_items=I)
    one = np.unique(test.user_ids, return_index=True)[1]             # hit_ratio reads one target per user
    single = Interactions(test.user_ids[one], test.item_ids[one], num_users=U, num_items=I)
    for k in (50, 100, [10, 50, 100]):
        kk = max(k) if isinstance(k, list) else k
        assert evaluation.precision_recall_score(m, test, k=k) == evaluation.precision_recall_score(h, test, k=k)
        assert evaluation.precision_recall_score(m, test, train, k=k) == \
            evaluation.precision_recall_score(h, test, train, k=k)
        assert evaluation.map_at_k(m, test, k=kk) == evaluation.map_at_k(h, test, k=kk)
        assert evaluation.hit_ratio(m, single, k=kk) == evaluation.hit_ratio(h, single, k=kk)
    assert m.score_calls == 0
