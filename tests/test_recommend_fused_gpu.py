"""The fused kernel (rg_mf_topk_users) on a model's tables.  recommend keeps the score-block path
wherever the block fits the device (README: the block path measured faster at 4096 users), so the
assertion of tests/test_recommend_gpu.py -- ids equal topk_users', scores are score_users' bits at
those ids -- is made on mf_engine.topk_users_fused with the model's tables, and on recommend itself
with the block declared not to fit, which is when recommend takes the kernel: with and without
`exclude`, for an exclusion matrix whose rows are stored unsorted, for 4,100 users in one call (no
score block is allocated on the way) and for a user with fewer than k items left.  Every such test
checks that the kernel was called; left alone, recommend does not call it at these sizes."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from recommendation_gans_amd import _lib, implicit, mf_engine
from tests.ncf_infer_common import make_model

pytestmark = pytest.mark.gpu

TILE = _lib.RG_MF_SCORE_ITEM_TILE


def count_calls(monkeypatch, fits=False):
    """Record the block sizes recommend hands to the kernel; fits=False: no score block fits."""
    calls, real = [], mf_engine.topk_users_fused
    if not fits:
        monkeypatch.setattr(implicit, "_score_block_fits", lambda n, num_items, device: False)

    def spy(*a, **kw):
        calls.append(len(a[4]))
        return real(*a, **kw)
    monkeypatch.setattr(mf_engine, "topk_users_fused", spy)
    return calls


def test_fused_equals_topk_users_and_score_users_on_the_models_tables(tmp_path, monkeypatch):
    model, train, _ = make_model("mf", tmp_path, monkeypatch, U=75, I=3 * TILE + 7, n_test=10)
    users = np.array([7, 3, 70, 3, 0, 74, 12])
    block, csr = model.score_users(users), train.tocsr()
    e_ptr, e_idx = implicit._csr_rows(csr, users)
    for k in (1, 10, 32):
        ids, sc = mf_engine.topk_users_fused(*model._tables(), users, k, e_ptr, e_idx)
        ids, sc = ids.cpu().numpy().astype(np.int64), sc.cpu().numpy()
        assert (ids == model.topk_users(users, k, csr)).all()
        assert sc.tobytes() == np.take_along_axis(block, ids, axis=1).tobytes()
        ids, sc = mf_engine.topk_users_fused(*model._tables(), users, k)
        ids, sc = ids.cpu().numpy().astype(np.int64), sc.cpu().numpy()
        assert (ids == model.topk_users(users, k)).all()
        assert sc.tobytes() == np.take_along_axis(block, ids, axis=1).tobytes()
    # left alone, recommend keeps the score block at this size
    calls = count_calls(monkeypatch, fits=True)
    assert (model.recommend(users, 10, exclude=train) == model.topk_users(users, 10, csr)).all() and calls == []


def test_recommend_equals_topk_users_and_score_users(tmp_path, monkeypatch):
    model, train, _ = make_model("mf", tmp_path, monkeypatch, U=75, I=3 * TILE + 7, n_test=10)
    calls = count_calls(monkeypatch)
    U, I = model._num_users, model._num_items
    users = np.array([7, 3, 70, 3, 0, 74, 12])
    before = model.score_users(users)
    csr = train.tocsr()
    for k in (1, 10, 32):
        ids, sc = model.recommend(users, k, exclude=train, return_scores=True)
        assert ids.dtype == np.int64 and sc.dtype == np.float32 and ids.shape == sc.shape == (len(users), k)
        assert (ids == model.topk_users(users, k, csr)).all()
        assert sc.tobytes() == np.take_along_axis(before, ids, axis=1).tobytes()
        for r, u in enumerate(users):
            assert not np.isin(ids[r], csr[u].indices).any()
        plain, psc = model.recommend(users, k, return_scores=True)
        assert (plain == model.topk_users(users, k)).all()
        assert (plain == np.argsort(-before, axis=1, kind="stable")[:, :k]).all()
        assert psc.tobytes() == np.take_along_axis(before, plain, axis=1).tobytes()
    assert calls == [len(users)] * 6                                    # every block went through the kernel
    # a scipy matrix, its rows stored unsorted, is the same exclusion
    coo = train.tocoo()
    perm = np.random.RandomState(1).permutation(coo.nnz)
    order = perm[np.argsort(coo.row[perm], kind="stable")]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(coo.row, minlength=U))])
    messy = sp.csr_matrix((coo.data[order], coo.col[order], ptr), shape=(U, I))
    assert not messy.has_sorted_indices
    a, asc = model.recommend(users, 10, exclude=messy, return_scores=True)
    b, bsc = model.recommend(users, 10, exclude=train, return_scores=True)
    assert (a == b).all() and asc.tobytes() == bsc.tobytes()
    assert model.score_users(users).tobytes() == before.tobytes()       # the model was only read


def test_a_user_with_fewer_than_k_items_left(tmp_path, monkeypatch):
    """With 32 of 40 items excluded and k = 10 the kernel's ranking continues into the excluded ids in
    id order with the score -inf: through recommend, and on the engine function itself."""
    model, _, _ = make_model("mf", tmp_path, monkeypatch, U=20, I=40, n_test=10)
    k, keep = 10, np.array([31, 4, 17, 22, 9, 38, 2, 13])               # k - 2 items stay for user 5
    gone = np.setdiff1d(np.arange(40), keep)
    exc = sp.csr_matrix((np.ones(len(gone), np.float32), (np.full(len(gone), 5), gone)), shape=(20, 40))
    block = model.score_users(np.array([5, 6]))
    want = model.topk_users(np.array([5, 6]), k, exc)
    e_ptr, e_idx = implicit._csr_rows(exc, np.array([5, 6]))
    direct = mf_engine.topk_users_fused(*model._tables(), np.array([5, 6]), k, e_ptr, e_idx)
    calls = count_calls(monkeypatch)
    routed = model.recommend([5, 6], k, exclude=exc, return_scores=True)
    assert calls == [2]                                                 # recommend went through the kernel
    for ids, sc in (routed, (direct[0].cpu().numpy().astype(np.int64), direct[1].cpu().numpy())):
        assert set(ids[0, :8]) == set(keep) and (ids[0, 8:] == gone[:2]).all()
        assert np.isneginf(sc[0, 8:]).all() and np.isfinite(sc[0, :8]).all() and np.isfinite(sc[1]).all()
        assert (ids == want).all()
        assert sc[0, :8].tobytes() == block[0][ids[0, :8]].tobytes()
        assert sc[1].tobytes() == block[1][ids[1]].tobytes()


def test_4100_users_in_one_call_without_a_score_block(tmp_path, monkeypatch):
    model, train, _ = make_model("mf", tmp_path, monkeypatch, U=75, I=TILE + 3, n_test=10)
    calls = count_calls(monkeypatch)
    users = np.random.RandomState(3).randint(0, 75, 4100)
    model.recommend(users[:8], 5, exclude=train)                        # load the code objects first
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ids, sc = model.recommend(users, 5, exclude=train, return_scores=True)
    peak = torch.cuda.max_memory_allocated() - base
    one_block = 4096 * (TILE + 3) * 4
    print(f"peak device memory during recommend: {peak} B; one 4096-user score block: {one_block} B")
    assert peak < one_block
    assert calls == [8, 4096, 4]
    uniq, first = np.unique(users, return_index=True)
    rows = first[np.searchsorted(uniq, users)]                          # every occurrence of a user: the same row
    assert (ids == ids[rows]).all() and sc.tobytes() == sc[rows].tobytes()
    assert (ids[first] == model.topk_users(uniq, 5, train.tocsr())).all()
    assert sc[first].tobytes() == np.take_along_axis(model.score_users(uniq), ids[first], axis=1).tobytes()
