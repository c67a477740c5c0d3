"""Diversified re-ranking without a GPU: ``seg_mmr_torch`` in float64 against a plain-Python greedy
loop (ties, repeats, NaN and infinities included), the replay check on that reference, the two
entries' declarations and refusals (decided before any HIP call), and the ValueErrors of the
wrappers, the model methods (against stub models) and ``intra_list_similarity``."""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib, candidates as cand
from recommendation_gans_amd.spotlight import evaluation as ev
from tests import candidates_common as cc
from tests import diverse_common as dc

t = torch.from_numpy


def small_lists(scores, ptr, idx, longest=40):
    rows = np.flatnonzero(np.diff(ptr) <= longest)
    return cc.take_lists(scores, ptr, idx, rows)


@pytest.mark.parametrize("kind", cc.SEG_KINDS)
@pytest.mark.parametrize("cosine", [False, True])
def test_seg_mmr_torch_float64_equals_a_plain_python_greedy_loop(kind, cosine):
    scores, ptr, idx = small_lists(*cc.seg_case(kind))
    table = dc.grid_table(3, rows=cc.NUM_ITEMS) if kind != "random" else dc.sim_table(3, rows=cc.NUM_ITEMS)
    rn = dc.rnorms64(table) if cosine else None
    for k, lam in ((1, 0.5), (10, 0.5), (32, 0.75), (10, 1.0)):
        want_pos, want_pen = dc.py_greedy(scores, ptr, idx, table, k, lam, rn)
        pos, val, pen = dc.ref_mmr(scores, ptr, idx, table, k, lam, rn)
        assert pos.dtype == np.int32 and (pos == want_pos).all(), (kind, k, lam)
        assert np.abs(pen - want_pen).max() <= 1e-12
        lens = np.diff(ptr)
        short = np.arange(k)[None, :] >= lens[:, None]
        assert (pos[short] == -1).all() and np.isneginf(val[short]).all() and (pen[short] == 0).all()
        at = (ptr[:-1, None] + np.maximum(pos, 0))[~short]
        assert np.array_equal(val[~short], scores[at].astype(np.float64), equal_nan=True)
        if lam == 1.0:
            assert (pos == cc.ref_topk(scores, ptr, idx, k)).all(), "lam = 1 is the top-k"


def test_seg_mmr_torch_diversifies_a_hand_case():
    """Items 0 and 1 are the same direction, item 2 is orthogonal: by relevance the order is 0, 1, 2;
    with lam = 0.5 the twin's penalty (1.0) puts the orthogonal item ahead of it."""
    table = np.array([[1.0, 0.0], [2.0, 0.0], [0.0, 1.0]], np.float32)
    scores, ptr, idx = np.array([0.9, 0.8, 0.5], np.float32), np.array([0, 3], np.int64), np.array([0, 1, 2], np.int32)
    rn = dc.rnorms64(table)
    assert dc.ref_mmr(scores, ptr, idx, table, 3, 1.0, rn)[0].tolist() == [[0, 1, 2]]
    pos, val, pen = dc.ref_mmr(scores, ptr, idx, table, 3, 0.5, rn)
    assert pos.tolist() == [[0, 2, 1]] and pen.tolist() == [[0.0, 0.0, 1.0]]
    # the returned tuple follows the flags
    f = lambda a: t(np.asarray(a, np.float64))      # noqa: E731
    args = (f(scores), t(ptr), t(idx), f(table), 2, 0.5)
    assert torch.is_tensor(cand.seg_mmr_torch(*args))
    assert len(cand.seg_mmr_torch(*args, return_penalties=True)) == 2
    assert cand.seg_mmr_torch(f([]), t(np.zeros(3, np.int64)), t(np.zeros(0, np.int32)), f(table), 2, 0.5).tolist() == \
        [[-1, -1], [-1, -1]]


def test_replay_accepts_the_reference_and_refuses_a_wrong_pick():
    scores, ptr, idx = small_lists(*cc.seg_case("repeats"), longest=70)
    table = dc.sim_table(16)
    rn = dc.rnorms64(table)
    lam = dc.lam32(0.7)
    pos, _, pen = dc.ref_mmr(scores, ptr, idx, table, 10, lam, rn)
    worst = dc.replay(scores, ptr, idx, table, lam, pos, rn, pen_out=pen)
    assert worst[0] <= 1e-6 and worst[1] <= 1e-6, "the float64 reference uses none of the fp32 bound"
    r = int(np.argmax(np.diff(ptr)))
    bad = pos.copy()
    bad[r, [1, 2]] = bad[r, [2, 1]]
    with pytest.raises(AssertionError):
        dc.replay(scores, ptr, idx, table, lam, bad, rn)
    # the bounds are of the size of float32's roundoff at these sizes
    a = table[:50].astype(np.float64)
    assert dc.sim_bound(a, a[::-1], rn[:50], rn[:50][::-1]).max() < 1e-4


# ---------------------------------------------------------------- the entries, without a GPU
def test_signatures_are_bound():
    sig = {n: a for n, _, a in _lib.SIGNATURES}
    assert len(sig["rg_seg_mmr"]) == 13 and len(sig["rg_seg_mean_sim"]) == 8
    L = _lib.load()
    assert hasattr(L, "rg_seg_mmr") and hasattr(L, "rg_seg_mean_sim")
    assert cand.SEG_MMR_MAX == 32 and cand.SEG_MMR_MAX_LEN == 1024


def test_entries_refuse_before_any_hip_call():
    L = _lib.load()
    p = 64              # never dereferenced: every call below is refused (or has nothing to do) first

    def refused(rc, reason):
        assert rc == -1 and reason in L.rg_last_error(), (rc, L.rg_last_error())
    good = [None, p, p, p, 4, p, p, 16, 0.5, 10, p, p, p]
    for at in (1, 2, 3, 5, 10):
        a = list(good)
        a[at] = None
        refused(L.rg_seg_mmr(*a), b"null pointer")
    for dim in (0, 257, -1):
        a = list(good)
        a[7] = dim
        refused(L.rg_seg_mmr(*a), b"dim must be in [1, 256]")
    for k in (0, 33, -1):
        a = list(good)
        a[9] = k
        refused(L.rg_seg_mmr(*a), b"k must be in [1, 32]")
    for lam in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        a = list(good)
        a[8] = lam
        refused(L.rg_seg_mmr(*a), b"lam must be in (0, 1]")
    a = list(good)
    a[4] = -1
    refused(L.rg_seg_mmr(*a), b"n < 0")
    for opt in (6, 11, 12):                       # rnorm, out_val and out_pen may be null: nothing to do at n == 0
        a = list(good)
        a[4], a[opt] = 0, None
        assert L.rg_seg_mmr(*a) == _lib.RG_OK
    good = [None, p, p, 4, p, p, 16, p]
    for at in (1, 2, 4, 7):
        a = list(good)
        a[at] = None
        refused(L.rg_seg_mean_sim(*a), b"null pointer")
    for dim in (0, 257):
        a = list(good)
        a[6] = dim
        refused(L.rg_seg_mean_sim(*a), b"dim must be in [1, 256]")
    a = list(good)
    a[3] = -1
    refused(L.rg_seg_mean_sim(*a), b"n < 0")
    a = list(good)
    a[3], a[5] = 0, None
    assert L.rg_seg_mean_sim(*a) == _lib.RG_OK


# ---------------------------------------------------------------- ValueErrors without a device
def bad(fn, *a, **kw):
    with pytest.raises(ValueError):
        fn(*a, **kw)


def test_wrappers_refuse_what_is_decided_on_the_host():
    scores, ptr, idx = t(np.zeros(3, np.float32)), t(np.array([0, 3], np.int64)), t(np.zeros(3, np.int32))
    table = t(np.ones((4, 8), np.float32))
    for k in (0, 33, -1, 2.5):
        bad(cand.seg_mmr, scores, ptr, idx, table, k, 0.5)
        bad(cand.seg_mmr_torch, scores, ptr, idx, table, k, 0.5)
    for lam in (0.0, -1.0, 1.5, float("nan")):
        bad(cand.seg_mmr, scores, ptr, idx, table, 5, lam)
        bad(cand.seg_mmr_torch, scores, ptr, idx, table, 5, lam)
    bad(cand.seg_mmr, scores, ptr, idx, table, 5, 0.5)          # host tensors: there is no fall-back
    bad(cand.seg_mean_sim, ptr, idx, table)
    bad(cand.seg_mean_sim, None, idx, table)


@pytest.mark.parametrize("kind", ["mf", "ncf", "neumf"])
def test_model_methods_refuse_bad_arguments(kind):
    m = dc.stub_model(kind, num_users=6, num_items=20)
    ok_space = None
    for fn in (m.diversify_candidates, ):
        bad(fn, [0, 1], [[1, 2]])                               # a length mismatch
        bad(fn, [0, 6], [[1], [2]])
        bad(fn, [0, -1], [[1], [2]])
        bad(fn, [0, 1], [[1], [20]])
        bad(fn, [0, 1], np.array([[1, -1], [2, 3]]))
        bad(fn, [0, 1], np.array([[0.5, 1.0], [2.0, 3.0]]))
        bad(fn, [0], [np.zeros(1025, np.int64)])                # over the cap
        for k in (0, 33, 2.5):
            bad(fn, [0], [[1, 2]], k=k)
        for lam in (0.0, 1.5, float("nan")):
            bad(fn, [0], [[1, 2]], lam=lam)
        bad(fn, [0], [[1, 2]], metric="euclid")
        bad(fn, [0], [[1, 2]], space="mlp" if kind != "neumf" else "tower")
    fn = m.recommend_diverse
    bad(fn, [6])
    bad(fn, [-1])
    for k in (0, 33, 21):                                      # 21 > num_items
        bad(fn, [0], k=k, pool=20)
    for pool in (9, 21, 10.5):                                 # below k, above num_items
        bad(fn, [0], k=10, pool=pool)
    for lam in (0.0, 1.5, float("nan")):
        bad(fn, [0], k=5, pool=10, lam=lam)
    bad(fn, [0], k=5, pool=10, metric="euclid")
    bad(fn, [0], k=5, pool=10, space="mlp" if kind != "neumf" else "tower")
    import scipy.sparse as sp
    bad(fn, [0], k=5, pool=10, exclude=sp.csr_matrix((6, 19)))
    big = dc.stub_model(kind, num_users=6, num_items=5000)
    bad(big.recommend_diverse, [0], k=5, pool=1025)
    # nothing to do: no device is touched
    assert m.recommend_diverse([], k=3, pool=5, space=ok_space).shape == (0, 3)
    ids, sc = m.diversify_candidates([0, 1], [[], []], k=3, return_scores=True)
    assert (ids == -1).all() and ids.dtype == np.int64 and np.isneginf(sc).all() and sc.dtype == np.float32
    # intra_list_similarity
    bad(ev.intra_list_similarity, m, [])
    bad(ev.intra_list_similarity, m, [[0, 20]])
    bad(ev.intra_list_similarity, m, np.array([[0.5, 1.0]]))
    bad(ev.intra_list_similarity, m, [np.zeros(1025, np.int64)])
    bad(ev.intra_list_similarity, m, [[0, 1]], metric="euclid")
    bad(ev.intra_list_similarity, m, [[0, 1]], space="mlp" if kind != "neumf" else "tower")
    assert ev.intra_list_similarity(m, [[], []]) == 0.0
