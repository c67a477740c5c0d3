"""ImplicitFactorizationModel.recommend on the GPU, for MF, NCF and NeuMF: its ids are topk_users'
ids (the same score block, -inf over the excluded entries, rg_topk_rows), its scores are score_users'
bits at those ids, the excluded items stay out, the storage order of the exclusion rows does not
matter, more than 4096 users go in one call, and the model is only read.  No tolerance: both sides
read the same block."""
import numpy as np
import pytest
import scipy.sparse as sp

from recommendation_gans_amd import _lib
from tests.ncf_infer_common import make_model

pytestmark = pytest.mark.gpu

TILE = _lib.RG_MF_SCORE_ITEM_TILE


@pytest.mark.parametrize("kind", ["mf", "ncf", "neumf"])
def test_recommend_equals_topk_users_and_score_users(kind, tmp_path, monkeypatch):
    model, train, test = make_model(kind, tmp_path, monkeypatch, U=75, I=3 * TILE + 7, n_test=300)
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
        plain = model.recommend(users, k)
        assert isinstance(plain, np.ndarray) and (plain == model.topk_users(users, k)).all()
        assert (plain == np.argsort(-before, axis=1, kind="stable")[:, :k]).all()
    # a scipy matrix, its rows stored unsorted, is the same exclusion
    coo = train.tocoo()
    perm = np.random.RandomState(1).permutation(coo.nnz)
    order = perm[np.argsort(coo.row[perm], kind="stable")]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(coo.row, minlength=U))])
    messy = sp.csr_matrix((coo.data[order], coo.col[order], ptr), shape=(U, I))
    assert not (np.diff(messy.indices) >= 0).all()
    assert (model.recommend(users, 10, exclude=messy) == model.recommend(users, 10, exclude=train)).all()
    for bad in (dict(user_ids=[0, U]), dict(user_ids=[-1]), dict(user_ids=users, k=0), dict(user_ids=users, k=33),
                dict(user_ids=users, exclude=sp.csr_matrix((U, I + 1)))):
        with pytest.raises(ValueError):
            model.recommend(**bad)
    assert model.score_users(users).tobytes() == before.tobytes()       # the model was only read


def test_a_user_with_fewer_than_k_items_left_gets_excluded_ids_in_id_order(tmp_path, monkeypatch):
    """With 32 of 40 items excluded and k = 10 the ranking continues into the excluded ids in id order,
    with the score -inf, and equals topk_users (rg_topk_rows used to write INT_MAX at these positions;
    tests/test_topk_fill_gpu.py checks the kernel alone)."""
    model, _, _ = make_model("mf", tmp_path, monkeypatch, U=20, I=40, n_test=10)
    k, keep = 10, np.array([31, 4, 17, 22, 9, 38, 2, 13])               # k - 2 items stay for user 5
    gone = np.setdiff1d(np.arange(40), keep)
    exc = sp.csr_matrix((np.ones(len(gone), np.float32), (np.full(len(gone), 5), gone)), shape=(20, 40))
    ids, sc = model.recommend([5, 6], k, exclude=exc, return_scores=True)
    assert set(ids[0, :8]) == set(keep) and (ids[0, 8:] == gone[:2]).all()
    assert np.isneginf(sc[0, 8:]).all() and np.isfinite(sc[0, :8]).all() and np.isfinite(sc[1]).all()
    assert (ids == model.topk_users(np.array([5, 6]), k, exc)).all()
    assert model.recommend([1, 2], 32).shape == (2, 32)
    with pytest.raises(ValueError):
        model.recommend([1, 2], 33)


@pytest.mark.parametrize("kind", ["mf", "ncf"])
def test_recommend_takes_more_than_4096_users_in_one_call(kind, tmp_path, monkeypatch):
    model, train, _ = make_model(kind, tmp_path, monkeypatch, U=75, I=TILE + 3, n_test=10)
    users = np.random.RandomState(3).randint(0, 75, 4100)
    ids, sc = model.recommend(users, 5, exclude=train, return_scores=True)
    first = {}
    for r, u in enumerate(users):                       # every occurrence of a user gets the same row
        first.setdefault(u, r)
    rows = np.array([first[u] for u in users])
    assert (ids == ids[rows]).all() and sc.tobytes() == sc[rows].tobytes()
    uniq = np.unique(users)
    assert (ids[[first[u] for u in uniq]] == model.topk_users(uniq, 5, train.tocsr())).all()
