"""Candidate lists without a GPU: NDCG@k against a per-user restatement on both of its paths, the
sampled protocol's list builder, sampled HR / NDCG through the host path on hand-checked scores (ties
included), the seed conditions the GPU tests rely on, and the three entries' declarations and
refusals (decided before any HIP call)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from recommendation_gans_amd import _lib
from recommendation_gans_amd.spotlight import evaluation as ev
from tests import candidates_common as cc


def interactions(users, items, shape):
    return sp.coo_matrix((np.ones(len(users), np.float32), (users, items)), shape=shape)


def small_problem(seed=0, U=30, I=50):
    rs = np.random.RandomState(seed)
    scores = rs.permutation(U * I).reshape(U, I).astype(np.float32) / (U * I)     # no ties
    test = interactions(rs.randint(0, U - 3, 80), rs.randint(0, I, 80), (U, I))    # the last users: no test items
    train = interactions(rs.randint(0, U, 200), rs.randint(0, I, 200), (U, I))
    return scores, test, train


def ndcg_restated(scores, test, train, k):
    test, out = test.tocsr(), []
    train = train.tocsr() if train is not None else None
    for u in range(test.shape[0]):
        targets = set(test.indices[test.indptr[u]:test.indptr[u + 1]].tolist())
        if not targets:
            continue
        s = scores[u].astype(np.float64).copy()
        if train is not None:
            s[train.indices[train.indptr[u]:train.indptr[u + 1]]] = -np.inf
        ranking = sorted(range(len(s)), key=lambda i: (-s[i], i))[:k]
        dcg = sum(1.0 / math.log2(j + 2) for j, i in enumerate(ranking) if i in targets)
        idcg = sum(1.0 / math.log2(j + 2) for j in range(min(len(targets), k)))
        out.append(dcg / idcg)
    return float(np.mean(out))


@pytest.mark.parametrize("k", [1, 5, 10])
@pytest.mark.parametrize("with_train", [False, True])
def test_ndcg_at_k_matches_a_per_user_restatement_on_both_paths(k, with_train):
    scores, test, train = small_problem()
    train = train if with_train else None
    want = ndcg_restated(scores, test, train, k)
    assert 0.0 <= want < 1.0 and (k < 10 or want > 0.0)
    host = ev.ndcg_at_k(cc.PredictOnly(scores), test, train, k=k)
    stub = cc.TopkUsers(scores)
    dev = ev.ndcg_at_k(stub, test, train, k=k)
    assert stub.calls == 1, "a model with topk_users takes the device top-k path"
    assert abs(host - want) <= 1e-12 and abs(dev - want) <= 1e-12
    assert ev.ndcg_at_k(cc.ScoreUsersOnly(scores), test, train, k=k) == host


def test_ndcg_is_one_for_a_perfect_ranking_and_counts_every_test_item():
    scores = np.zeros((2, 6), np.float32)
    scores[0, [1, 4]] = [2.0, 1.0]          # user 0: both test items on top
    scores[1, [0, 3, 5]] = [3.0, 2.0, 1.0]  # user 1: test items at ranks 0 and 2 of its 2
    test = interactions([0, 0, 1, 1], [1, 4, 0, 5], (2, 6))
    want1 = (1.0 + 1.0 / math.log2(4)) / (1.0 + 1.0 / math.log2(3))
    assert ev.ndcg_at_k(cc.PredictOnly(scores), test, k=3) == pytest.approx((1.0 + want1) / 2, abs=1e-15)


def test_sampled_candidate_lists():
    _, test, train = small_problem()
    I = test.shape[1]
    users, ptr, idx = ev.sampled_candidate_lists(test, train, 20, np.random.RandomState(5))
    csr = test.tocsr()
    m = csr.nnz
    assert users.dtype == np.int64 and ptr.dtype == np.int64 and idx.dtype == np.int32
    assert len(users) == m and (np.diff(ptr) == 21).all() and ptr[0] == 0 and ptr[-1] == len(idx)
    lists = idx.reshape(m, 21)
    assert (users == np.repeat(np.arange(csr.shape[0]), np.diff(csr.indptr))).all()
    assert (lists[:, 0] == csr.indices).all(), "the target comes first"
    taken = set((test.tocsr() + train.tocsr()).tocoo().row.astype(np.int64) * I +
                (test.tocsr() + train.tocsr()).tocoo().col)
    for u, row in zip(users, lists):
        assert len(set(row[1:].tolist())) == 20, "negatives are distinct"
        assert not any(int(u) * I + int(i) in taken for i in row[1:]), "a negative is a test or train item"
        assert row[1:].min() >= 0 and row[1:].max() < I
    again = ev.sampled_candidate_lists(test, train, 20, np.random.RandomState(5))
    assert all((a == b).all() for a, b in zip((users, ptr, idx), again)), "an equal seed reproduces the draw"
    other = ev.sampled_candidate_lists(test, train, 20, np.random.RandomState(6))
    assert (other[2] != idx).any()
    default = ev.sampled_candidate_lists(test, train, 20)
    zero = ev.sampled_candidate_lists(test, train, 20, np.random.RandomState(0))
    assert (default[2] == zero[2]).all(), "the default is RandomState(0)"
    # every eligible item is drawn when n_negatives is all of them (the exact draw of the last resort)
    dense_train = interactions(np.repeat(np.arange(30), 40), np.tile(np.arange(40), 30), (30, 50))
    t1 = interactions([2], [45], (30, 50))
    _, _, full = ev.sampled_candidate_lists(t1, dense_train, 9, np.random.RandomState(1))
    assert full[0] == 45 and sorted(full[1:].tolist()) == [40, 41, 42, 43, 44, 46, 47, 48, 49]
    with pytest.raises(ValueError, match="fewer than"):
        ev.sampled_candidate_lists(t1, dense_train, 10)


def test_sampled_hit_ndcg_host_path_hand_checked():
    """3 users x 6 items, one test item each, every other item a negative (n_negatives = 5, so the
    lists do not depend on the draw's order).  User 0's target is beaten by 1 item; user 1's ties with
    two items of which one has a lower id (ahead = 1 + 1 higher = 2); user 2's is beaten by all."""
    scores = np.array([[0.9, 0.5, 0.1, 0.2, 0.3, 0.4],      # target 1: only item 0 is higher -> ahead 1
                       [0.7, 0.1, 0.7, 0.7, 0.9, 0.2],      # target 2: item 4 higher, item 0 ties ahead -> 2
                       [0.6, 0.5, 0.4, 0.3, 0.2, 0.1]],     # target 5: all five higher -> 5
                      dtype=np.float32)
    test = interactions([0, 1, 2], [1, 2, 5], (3, 6))
    hr, ndcg = ev.sampled_hit_ndcg(cc.PredictOnly(scores), test, n_negatives=5, k=3)
    assert hr == 2 / 3
    assert ndcg == pytest.approx((1 / math.log2(3) + 1 / math.log2(4) + 0.0) / 3, abs=1e-15)
    hr1, ndcg1 = ev.sampled_hit_ndcg(cc.PredictOnly(scores), test, n_negatives=5, k=2)
    assert hr1 == 1 / 3 and ndcg1 == pytest.approx((1 / math.log2(3)) / 3, abs=1e-15)
    hr6, _ = ev.sampled_hit_ndcg(cc.PredictOnly(scores), test, n_negatives=5, k=6)
    assert hr6 == 1.0
    nan = scores.copy()
    nan[0, 1] = np.nan                                        # a NaN target ranks behind every number
    assert ev.sampled_hit_ndcg(cc.PredictOnly(nan), test, n_negatives=5, k=5)[0] == 1 / 3
    with pytest.raises(ValueError):
        ev.sampled_hit_ndcg(cc.PredictOnly(scores), interactions([], [], (3, 6)), n_negatives=2)


def test_numpy_references_of_the_segmented_kernels_on_a_hand_case():
    scores = np.array([0.5, np.nan, 0.5, -0.0, 0.0, 0.5, 2.0], np.float32)
    idx = np.array([7, 1, 3, 9, 2, 7, 4], np.int32)
    ptr = np.array([0, 6, 6, 7], np.int64)
    top = cc.ref_topk(scores, ptr, idx, 8)
    assert top[0].tolist() == [2, 0, 5, 4, 3, 1, -1, -1]      # 0.5: id 3, then id 7 twice by position; 0.0 by id
    assert top[1].tolist() == [-1] * 8 and top[2].tolist() == [0] + [-1] * 7
    assert cc.ref_rank(scores, ptr, idx).tolist() == [[0, 1], [-1, -1], [0, 0]]


@pytest.mark.parametrize("kind", ["mf", "ncf", "neumf"])
def test_seed_of_the_model_level_gpu_test_separates_the_rankings(kind):
    """The comparison of rank_candidates over the whole catalogue with recommend holds on the rows
    whose first k + 1 float64 scores are further apart than twice the allowed error: at least 90 %."""
    rows = cc.separated_rows(kind)
    assert len(rows) == cc.MODEL_U and rows.mean() >= 0.9, rows.mean()


def test_sampled_protocol_tables_of_the_gpu_test():
    """The two models the GPU test compares the device and host paths on.  Untied: in every list of
    the default draw the target is further from every negative than twice the two scores' bounds, so
    any two float32 evaluations within the bound count the same entries ahead.  Quantised: sums on a
    grid of 1/16, exact in float32 in any order, and ties with the target in most lists."""
    train, test = cc.model_interactions()
    users, ptr, idx = ev.sampled_candidate_lists(test, train, cc.SAMPLED_NEG)
    assert len(users) > 100
    assert cc.target_margins(cc.untied_tables(), users, ptr, idx).min() > 0
    U, I, ub, ib = (t.astype(np.float64) for t in cc.quantised_tables())
    z = U @ I.T + ub[:, None] + ib[None, :]
    assert (z * 16 == np.round(z * 16)).all() and np.abs(z).max() < 16
    lists = idx.reshape(len(users), -1)
    zl = z[users[:, None], lists]
    assert ((zl[:, 1:] == zl[:, :1]).any(axis=1)).mean() > 0.5


@pytest.mark.parametrize("dim", cc.SCORE_DIMS)
def test_mf_reference_admits_a_float32_restatement(dim):
    """The float64 reference and the bound the GPU test holds rg_mf_score_lists to, on the GPU test's
    own tables and lists at every dim of SCORE_DIMS: a plain float32 numpy restatement of the formula
    (one summation chain of length dim, longer than any layout's) stays inside the bound."""
    tables = cc.mf_tables(dim)
    worst = 0.0
    for n_lists in cc.SCORE_USERS:
        users, ptr, idx = cc.score_case(n_lists, seed=n_lists)
        ref, bound = cc.mf_reference(tables, users, ptr, idx)
        got = cc.mf_scores_float32(tables, users, ptr, idx)
        assert got.shape == ref.shape and len(ref) > 0
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / bound).max()))
    print(f"\ndim {dim}: float32 restatement, largest share of the bound {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- the entries, without a GPU
def test_signatures_are_bound():
    sig = {n: a for n, _, a in _lib.SIGNATURES}
    assert len(sig["rg_mf_score_lists"]) == 11 and len(sig["rg_seg_topk"]) == 8 and len(sig["rg_seg_rank"]) == 6
    L = _lib.load()
    assert all(hasattr(L, n) for n in ("rg_mf_score_lists", "rg_seg_topk", "rg_seg_rank"))


def test_entries_refuse_before_any_hip_call():
    L = _lib.load()
    p = 64              # never dereferenced: every call below is refused (or has nothing to do) first

    def refused(rc, reason):
        assert rc == -1 and reason in L.rg_last_error(), (rc, L.rg_last_error())
    score = [None, p, p, p, p, 16, p, p, p, 4, p]
    for at in (1, 2, 3, 4, 6, 7, 8, 10):
        a = list(score)
        a[at] = None
        refused(L.rg_mf_score_lists(*a), b"null pointer")
    for dim in (0, 257, -1):
        refused(L.rg_mf_score_lists(None, p, p, p, p, dim, p, p, p, 4, p), b"dim must be in [1, 256]")
    refused(L.rg_mf_score_lists(None, p, p, p, p, 16, p, p, p, -1, p), b"n < 0")
    assert L.rg_mf_score_lists(None, p, p, p, p, 16, p, p, p, 0, p) == _lib.RG_OK
    for at in (1, 2, 3, 6):
        a = [None, p, p, p, 4, 10, p, p]
        a[at] = None
        refused(L.rg_seg_topk(*a), b"null pointer")
    for k in (0, 33, -1):
        refused(L.rg_seg_topk(None, p, p, p, 4, k, p, p), b"k must be in [1, 32]")
    refused(L.rg_seg_topk(None, p, p, p, -1, 10, p, None), b"n < 0")
    assert L.rg_seg_topk(None, p, p, p, 0, 10, p, None) == _lib.RG_OK
    for at in (1, 2, 3, 5):
        a = [None, p, p, p, 4, p]
        a[at] = None
        refused(L.rg_seg_rank(*a), b"null pointer")
    refused(L.rg_seg_rank(None, p, p, p, -1, p), b"n < 0")
    assert L.rg_seg_rank(None, p, p, p, 0, p) == _lib.RG_OK
