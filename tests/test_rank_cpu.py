"""mrr_score's device path on the CPU: a model with ``rank_users`` is asked for the ranks of
the test items (and never for the score block's ranking on the host), and the result is the
reference's per-user loop (spotlight/evaluation.py:13-60, scipy rankdata with ties averaged)
written out; a model without ``rank_users`` keeps the host path.  Scores quantised to eighths
so that ties occur.  The ranks are exact; the per-user means may differ in the float64
summation order only (rtol 1e-12)."""
import numpy as np
import pytest
import scipy.stats as st

from recommendation_gans_amd.spotlight import evaluation
from recommendation_gans_amd.spotlight.interactions import Interactions


class _HostModel:
    def __init__(self, scores):
        self.s = scores

    def score_users(self, users):
        return self.s[np.asarray(users)]


class _RankModel(_HostModel):
    """rank_users in NumPy by the counting identity, recording its calls."""

    def __init__(self, scores):
        super().__init__(scores)
        self.calls = []

    def rank_users(self, users, targets_csr, exclude_csr=None):
        self.calls.append((np.asarray(users).copy(), exclude_csr is not None))
        out = []
        for u in users:
            key = self.s[u].astype(np.float32).copy()
            if exclude_csr is not None:
                key[exclude_csr.indices[exclude_csr.indptr[u]:exclude_csr.indptr[u + 1]]] = -evaluation.FLOAT_MAX
            for t in targets_csr.indices[targets_csr.indptr[u]:targets_csr.indptr[u + 1]]:
                out.append((key > key[t]).sum() + ((key == key[t]).sum() + 1) / 2)
        return np.array(out, dtype=np.float64)


def _reference_loop(scores, test, train):
    """evaluation.py:13-60 written out, one rankdata per test user with items."""
    ref = []
    for u, row in enumerate(test.tocsr()):
        if not len(row.indices):
            continue
        pred = -scores[u].copy()
        if train is not None:
            pred[train.tocsr()[u].indices] = evaluation.FLOAT_MAX
        ref.append((1.0 / st.rankdata(pred)[row.indices]).mean())
    return np.array(ref)


@pytest.fixture(scope="module")
def data():
    rs = np.random.RandomState(2)
    U, I = 60, 45
    scores = (rs.rand(U, I) * 8).round().astype(np.float32) / 8
    test = Interactions(rs.randint(0, U - 5, 240), rs.randint(0, I, 240), ratings=np.ones(240), num_users=U,
                        num_items=I)                                   # the last users have no test items
    train = Interactions(rs.randint(0, U, 500), rs.randint(0, I, 500), ratings=np.ones(500), num_users=U,
                         num_items=I)
    return scores, test, train, {None: _reference_loop(scores, test, None), "train": _reference_loop(scores, test, train)}


@pytest.mark.parametrize("with_train", [False, True])
def test_mrr_takes_the_rank_path_and_matches_the_loop(data, with_train):
    scores, test, train, ref = data
    m = _RankModel(scores)
    got = evaluation.mrr_score(m, test, train if with_train else None)
    assert m.calls, "mrr_score must ask the model for the ranks (rank_users)"
    users = np.flatnonzero(np.diff(test.tocsr().indptr) > 0)
    assert (np.concatenate([c[0] for c in m.calls]) == users).all()      # same users, same order
    assert all(c[1] == with_train for c in m.calls)
    want = ref["train" if with_train else None]
    assert got.shape == want.shape and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("with_train", [False, True])
def test_model_without_rank_users_keeps_the_host_path(data, with_train):
    scores, test, train, ref = data
    got = evaluation.mrr_score(_HostModel(scores), test, train if with_train else None)
    np.testing.assert_allclose(got, ref["train" if with_train else None], rtol=0, atol=0)


def test_blocks_are_stitched_in_user_order(data):
    """More than one block: the blocks' users and results are concatenated in order."""
    scores, test, train, ref = data
    m = _RankModel(scores)
    got = evaluation._mrr_from_ranks(m, test.tocsr(), train.tocsr(), block=7)
    assert len(m.calls) > 1 and all(len(c[0]) <= 7 for c in m.calls)
    np.testing.assert_allclose(got, ref["train"], rtol=1e-12, atol=0)


def test_csr_rows_slices_in_the_given_order():
    """The upload helper of ImplicitFactorizationModel.rank_users: rows in the order asked
    (repeats and empty rows included), each row's indices as stored."""
    from recommendation_gans_amd.implicit import _csr_rows
    rs = np.random.RandomState(3)
    csr = Interactions(rs.randint(0, 20, 80), rs.randint(0, 30, 80), num_users=21, num_items=30).tocsr()
    rows = np.array([5, 20, 0, 5, 19], dtype=np.int64)
    ptr, idx = _csr_rows(csr, rows)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and ptr[0] == 0 and len(ptr) == len(rows) + 1
    for r, u in enumerate(rows):
        assert (idx[ptr[r]:ptr[r + 1]] == csr.indices[csr.indptr[u]:csr.indptr[u + 1]]).all()
    assert ptr[-1] == len(idx)
