"""Candidate lists on the GPU: rg_seg_topk / rg_seg_rank exactly against numpy on ragged lists where
ties are the rule, rg_mf_score_lists within the bound derived for its formula and bit-stable per pair,
the model-level calls for MF, NCF and NeuMF, the sampled protocol's device path against its host
path, and every refusal.  300 items; every case in a few seconds."""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib, candidates as cand
from recommendation_gans_amd.spotlight import evaluation as ev
from tests import candidates_common as cc
from tests.ncf_infer_common import make_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
t = torch.from_numpy


def dev(*arrays):
    return [t(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def topk(scores, ptr, idx, k):
    pos, val = cand.seg_topk(*dev(scores, ptr, idx), k, return_values=True)
    return pos.cpu().numpy(), val.cpu().numpy()


def rank(scores, ptr, idx):
    return cand.seg_rank(*dev(scores, ptr, idx)).cpu().numpy()


# ---------------------------------------------------------------- rg_seg_topk / rg_seg_rank
@pytest.mark.parametrize("kind", cc.SEG_KINDS)
def test_seg_topk_and_rank_equal_numpy_exactly(kind):
    scores, ptr, idx = cc.seg_case(kind)
    want_rank = cc.ref_rank(scores, ptr, idx)
    got_rank = rank(scores, ptr, idx)
    assert got_rank.dtype == np.int32 and (got_rank == want_rank).all()
    lens = np.diff(ptr)
    for k in cc.KS:
        pos, val = topk(scores, ptr, idx, k)
        want = cc.ref_topk(scores, ptr, idx, k)
        assert pos.dtype == np.int32 and (pos == want).all(), (kind, k)
        short = np.arange(k)[None, :] >= lens[:, None]
        assert (pos[short] == -1).all() and (pos[~short] >= 0).all()
        assert np.isneginf(val[short]).all()
        at = (ptr[:-1, None] + np.maximum(pos, 0))[~short]
        assert val[~short].tobytes() == scores[at].tobytes(), "the raw value at each position"
        # the rank agrees with the top-k: the target is among the first k iff fewer than k are ahead
        ahead = want_rank.sum(axis=1)
        in_top = (pos == 0).any(axis=1)
        assert (in_top == ((ahead < k) & (lens > 0))).all()


@pytest.mark.parametrize("kind", ["quantised", "special"])
def test_a_lists_output_depends_on_that_list_alone(kind):
    scores, ptr, idx = cc.seg_case(kind, seed=1)
    n, k = len(ptr) - 1, 10
    pos, val = topk(scores, ptr, idx, k)
    rk = rank(scores, ptr, idx)
    rev = np.arange(n)[::-1]
    p2, v2 = topk(*cc.take_lists(scores, ptr, idx, rev), k)
    assert p2.tobytes() == pos[rev].tobytes() and v2.tobytes() == val[rev].tobytes()
    assert rank(*cc.take_lists(scores, ptr, idx, rev)).tobytes() == rk[rev].tobytes()
    for r in (int(np.argmax(np.diff(ptr))), int(np.flatnonzero(np.diff(ptr) == 33)[0])):
        p1, v1 = topk(*cc.take_lists(scores, ptr, idx, [r]), k)               # standing alone
        assert p1.tobytes() == pos[r:r + 1].tobytes() and v1.tobytes() == val[r:r + 1].tobytes()
        assert rank(*cc.take_lists(scores, ptr, idx, [r])).tobytes() == rk[r:r + 1].tobytes()
        other = scores.copy()                                                    # the other lists change
        keep = np.zeros(len(scores), bool)
        keep[ptr[r]:ptr[r + 1]] = True
        other[~keep] = np.float32(7.0)
        p3, v3 = topk(other, ptr, idx, k)
        assert p3[r].tobytes() == pos[r].tobytes() and v3[r].tobytes() == val[r].tobytes()
        assert rank(other, ptr, idx)[r].tobytes() == rk[r].tobytes()


def test_every_list_empty_and_no_lists():
    ptr = np.zeros(4, np.int64)
    e_s, e_i = torch.zeros(0, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)
    pos, val = cand.seg_topk(e_s, t(ptr).to(DEV), e_i, 3, return_values=True)
    assert (pos.cpu().numpy() == -1).all() and pos.shape == (3, 3) and np.isneginf(val.cpu().numpy()).all()
    assert (cand.seg_rank(e_s, t(ptr).to(DEV), e_i).cpu().numpy() == -1).all()
    assert cand.seg_topk(e_s, t(ptr[:1]).to(DEV), e_i, 3).shape == (0, 3)
    # empty lists beside a full one go through the kernel
    scores, p, idx = np.array([1.0, 2.0], np.float32), np.array([0, 0, 2, 2], np.int64), np.array([5, 6], np.int32)
    assert topk(scores, p, idx, 3)[0].tolist() == [[-1, -1, -1], [1, 0, -1], [-1, -1, -1]]
    assert rank(scores, p, idx).tolist() == [[-1, -1], [1, 0], [-1, -1]]


# ---------------------------------------------------------------- rg_mf_score_lists
def run_scores(tables, users, ptr, idx, unaligned=False):
    tabs = dev(*tables)
    if unaligned:                     # a view one float into a larger buffer: 4-byte aligned only
        for j in (0, 1):
            buf = torch.empty(tabs[j].numel() + 1, dtype=torch.float32, device=DEV)
            view = buf[1:].view(tabs[j].shape)
            view.copy_(tabs[j])
            assert view.data_ptr() % 16 != 0 and view.is_contiguous()
            tabs[j] = view
    before = [x.clone() for x in tabs]
    out = cand.score_lists(*tabs, *dev(users, ptr, idx))
    torch.cuda.synchronize()
    for a, b in zip(tabs, before):
        assert torch.equal(a, b), "the tables are only read"
    return out.cpu().numpy()


@pytest.mark.parametrize("dim", cc.SCORE_DIMS)
def test_mf_score_lists_within_the_derived_bound(dim):
    tables = cc.mf_tables(dim)
    worst = 0.0
    for n_lists in cc.SCORE_USERS:
        for unaligned in ((False, True) if dim % 4 == 0 else (False,)):
            users, ptr, idx = cc.score_case(n_lists, seed=n_lists)
            got = run_scores(tables, users, ptr, idx, unaligned)
            ref, bound = cc.mf_reference(tables, users, ptr, idx)
            assert got.dtype == np.float32 and got.shape == ref.shape
            if len(ref):
                share = float((np.abs(got.astype(np.float64) - ref) / bound).max())
                worst = max(worst, share)
                print(f"\ndim {dim} lists {n_lists} unaligned {unaligned}: largest share of the bound {share:.3f}")
                assert share <= 1.0
    print(f"dim {dim}: largest share of the bound over all cases {worst:.3f}")


@pytest.mark.parametrize("dim", sorted(cc.VEC_LAYOUT_DIMS.values()))
def test_aligned_and_unaligned_calls_both_meet_the_float64_reference(dim):
    """One dim per VecLayout (24, 100, 160): the aligned call runs on the VecLayout, the call on views
    one float off on the scalar layout of the same range (<16,2>, <64,2>, <64,3>).  The two order the
    summation chain differently, so the bits may differ; each is held to the bound against float64,
    and so they lie within two bounds of each other."""
    tables = cc.mf_tables(dim, seed=2)
    users, ptr, idx = cc.score_case(130, seed=11)
    ref, bound = cc.mf_reference(tables, users, ptr, idx)
    got = [run_scores(tables, users, ptr, idx, unaligned).astype(np.float64) for unaligned in (False, True)]
    shares = [float((np.abs(g - ref) / bound).max()) for g in got]
    between = float((np.abs(got[0] - got[1]) / bound).max())
    print(f"\ndim {dim}: largest share of the bound, aligned {shares[0]:.3f}, unaligned {shares[1]:.3f}; "
          f"|aligned - unaligned| / bound {between:.3f}")
    assert shares[0] <= 1.0 and shares[1] <= 1.0
    assert between <= 2.0


@pytest.mark.parametrize("dim", [3, 16, 65, 100, 12, 132])
def test_a_pairs_score_is_the_same_bits_wherever_it_stands(dim):
    tables = cc.mf_tables(dim)
    users, ptr, idx = cc.score_case(130, seed=7)
    got = run_scores(tables, users, ptr, idx)
    rows = np.repeat(np.arange(len(users)), np.diff(ptr))
    pair = users[rows] * cc.NUM_ITEMS + idx
    order = np.argsort(pair, kind="stable")
    same = pair[order][1:] == pair[order][:-1]
    assert same.sum() > 100, "the case repeats pairs"
    bits = got.view(np.uint32)[order]
    assert (bits[1:][same] == bits[:-1][same]).all()
    # another call: the lists reversed, and every entry as a list of its own
    rev = np.arange(len(users))[::-1]
    _, p2, i2 = cc.take_lists(got, ptr, idx, rev)
    got2 = run_scores(tables, users[rev], p2, i2)
    assert got2.tobytes() == cc.take_lists(got, ptr, idx, rev)[0].tobytes()
    got3 = run_scores(tables, users[rows], np.arange(len(idx) + 1, dtype=np.int64), idx)
    assert got3.tobytes() == got.tobytes()


# ---------------------------------------------------------------- model level
@pytest.mark.parametrize("kind", ["mf", "ncf", "neumf"])
def test_model_rank_candidates(kind, tmp_path, monkeypatch):
    model, _, _ = make_model(kind, tmp_path, monkeypatch, cc.MODEL_U, cc.MODEL_I, 50, E=cc.MODEL_E, M=cc.MODEL_M)
    if kind == "mf":
        cc.load_tables(model, cc.untied_tables())
    rs = np.random.RandomState(2)
    users = rs.randint(0, cc.MODEL_U, 23)
    lists = [rs.randint(0, cc.MODEL_I, n) for n in np.resize([0, 1, 5, 33, 64, 65, 200], 23)]
    scores = model.score_candidates(users, lists)
    ptr = cc.list_ptr([len(x) for x in lists])
    flat = np.concatenate(lists).astype(np.int32)
    assert scores.dtype == np.float32 and scores.shape == (ptr[-1],)
    for k in (1, 10, 32):
        ids, sc = model.rank_candidates(users, lists, k=k, return_scores=True)
        pos = cc.ref_topk(scores, ptr, flat, k)
        want = np.where(pos >= 0, flat[np.minimum(ptr[:-1, None] + np.maximum(pos, 0), len(flat) - 1)], -1)
        assert ids.dtype == np.int64 and (ids == want).all()
        want_sc = np.where(pos >= 0, scores[np.minimum(ptr[:-1, None] + np.maximum(pos, 0), len(flat) - 1)], -np.inf)
        assert sc.dtype == np.float32 and sc.tobytes() == want_sc.astype(np.float32).tobytes()
        assert (model.rank_candidates(users, lists, k=k) == ids).all()
    if kind != "mf":        # the same kernel as predict(users, items)
        rep = np.repeat(users, np.diff(ptr))
        assert model.predict(rep, flat.astype(np.int64)).tobytes() == scores.tobytes()
    # the other forms of `candidates`
    block = rs.randint(0, cc.MODEL_I, (23, 12))
    assert model.score_candidates(users, block).tobytes() == model.score_candidates(users, list(block)).tobytes()
    import scipy.sparse as sp
    csr = sp.csr_matrix((np.ones(block.size), block.reshape(-1), np.arange(24) * 12), shape=(23, cc.MODEL_I))
    assert model.score_candidates(users, csr).tobytes() == model.score_candidates(users, block).tobytes()
    # the whole catalogue as the candidates: recommend's ids where the float64 scores are separated
    k = cc.MODEL_K
    everyone = np.arange(cc.MODEL_U)
    got = model.rank_candidates(everyone, np.tile(np.arange(cc.MODEL_I), (cc.MODEL_U, 1)), k=k)
    ok = cc.separated_rows(kind, k)
    assert ok.mean() >= 0.9
    assert (got[ok] == model.recommend(everyone, k=k)[ok]).all()
    blk, _ = cc.model_block64(kind)
    assert (got[ok] == np.argsort(-blk, axis=1, kind="stable")[:, :k][ok]).all()


@pytest.mark.parametrize("tables", ["untied", "quantised"])
def test_sampled_hit_ndcg_device_path_equals_host_path(tables, tmp_path, monkeypatch):
    model, _, _ = make_model("mf", tmp_path, monkeypatch, cc.MODEL_U, cc.MODEL_I, 50, E=cc.MODEL_E)
    tabs = cc.untied_tables() if tables == "untied" else cc.quantised_tables()
    cc.load_tables(model, tabs)
    train, test = cc.model_interactions()

    class HostPath:                  # without score_candidates: predict + numpy
        predict = staticmethod(model.predict)
    for k in (1, 10):
        got = ev.sampled_hit_ndcg(model, test, train, n_negatives=cc.SAMPLED_NEG, k=k)
        want = ev.sampled_hit_ndcg(HostPath(), test, train, n_negatives=cc.SAMPLED_NEG, k=k)
        print(f"\n{tables} k={k}: HR {got[0]:.4f} NDCG {got[1]:.4f}")
        assert got == want and 0.0 <= got[1] <= got[0] <= 1.0
        assert k == 1 or got[0] > 0.0      # a random model hits about k in 100 lists: at k = 1 maybe none
    users, ptr, idx = ev.sampled_candidate_lists(test, train, cc.SAMPLED_NEG)
    counts = model.candidate_target_ranks(users, idx.reshape(len(users), -1))
    ref = cc.mf_reference(tabs, users, ptr, idx)[0]
    assert (counts == cc.ref_rank(ref, ptr, idx)).all(), "the counts are those of the float64 scores"
    if tables == "quantised":
        assert (counts[:, 1] > 0).mean() > 0.2, "ties decide"


def test_ncf_sampled_hit_ndcg_runs_on_the_device(tmp_path, monkeypatch):
    model, train, test = make_model("neumf", tmp_path, monkeypatch, cc.MODEL_U, cc.MODEL_I, 50, E=cc.MODEL_E,
                                    M=cc.MODEL_M)

    class HostPath:
        predict = staticmethod(model.predict)
    got = ev.sampled_hit_ndcg(model, test, train, n_negatives=50, k=10)
    assert got == ev.sampled_hit_ndcg(HostPath(), test, train, n_negatives=50, k=10)   # the same kernel's bits


# ---------------------------------------------------------------- refusals
def test_python_refusals(tmp_path, monkeypatch):
    U, I, ub, ib = dev(*cc.mf_tables(16))
    users, ptr, idx = dev(*cc.score_case(5, seed=1))
    ok = cand.score_lists(U, I, ub, ib, users, ptr, idx)

    def bad(fn, *a, **kw):
        with pytest.raises(ValueError):
            fn(*a, **kw)
    bad(cand.score_lists, U.double(), I, ub, ib, users, ptr, idx)
    bad(cand.score_lists, U.cpu(), I, ub, ib, users, ptr, idx)
    bad(cand.score_lists, U[:, ::2], I, ub, ib, users, ptr, idx)
    bad(cand.score_lists, U, I[:, :8].contiguous(), ub, ib, users, ptr, idx)
    bad(cand.score_lists, U, I, ub[:-1], ib, users, ptr, idx)
    bad(cand.score_lists, U, I, ub, ib, users.int(), ptr, idx)
    bad(cand.score_lists, U, I, ub, ib, users[:-1], ptr, idx)
    bad(cand.score_lists, U, I, ub, ib, users, ptr.int(), idx)
    bad(cand.score_lists, U, I, ub, ib, users, ptr, idx.long())
    bad(cand.score_lists, U, I, ub, ib, users, ptr.cpu(), idx)
    bad(cand.score_lists, U, I, ub, ib, users, ptr + 1, idx)
    bad(cand.score_lists, U, I, ub, ib, users, ptr.flip(0).contiguous(), idx)
    bad(cand.score_lists, U, I, ub, ib, users, ptr, idx[:-1])
    bad(cand.score_lists, U, I, ub, ib, users + U.shape[0], ptr, idx)
    bad(cand.score_lists, U, I, ub, ib, users - U.shape[0], ptr, idx)
    bad(cand.score_lists, U, I, ub, ib, users, ptr, idx + I.shape[0])
    bad(cand.score_lists, U, I, ub, ib, users, ptr, -idx - 1)
    for fn in (lambda *a: cand.seg_topk(*a, 5), cand.seg_rank):
        bad(fn, ok.double(), ptr, idx)
        bad(fn, ok.cpu(), ptr, idx)
        bad(fn, ok[:-1], ptr, idx)
        bad(fn, ok[::2], ptr[:3].contiguous(), idx)
        bad(fn, ok, ptr.int(), idx)
        bad(fn, ok, ptr, idx.long())
        bad(fn, ok, ptr + 1, idx)
        bad(fn, ok.reshape(1, -1), ptr, idx)
    for k in (0, 33, -1, 2.5):
        bad(cand.seg_topk, ok, ptr, idx, k)
    model, _, _ = make_model("mf", tmp_path, monkeypatch, cc.MODEL_U, cc.MODEL_I, 50, E=cc.MODEL_E)
    for fn in (model.score_candidates, model.rank_candidates, model.candidate_target_ranks):
        bad(fn, [0, 1], [[1, 2]])                               # a length mismatch
        bad(fn, [0, cc.MODEL_U], [[1], [2]])
        bad(fn, [0, -1], [[1], [2]])
        bad(fn, [0, 1], [[1], [cc.MODEL_I]])
        bad(fn, [0, 1], np.array([[1, -1], [2, 3]]))
        bad(fn, [0, 1], np.array([[0.5, 1.0], [2.0, 3.0]]))
    for k in (0, 33):
        bad(model.rank_candidates, [0], [[1, 2]], k=k)
    assert model.rank_candidates([], [], k=3).shape == (0, 3) and model.score_candidates([], []).shape == (0,)


def test_raw_entries_return_rg_e_arg():
    L = _lib.load()
    U, I, ub, ib = dev(*cc.mf_tables(16))
    users, ptr, idx = dev(*cc.score_case(5, seed=1))
    out = torch.zeros(idx.numel(), dtype=torch.float32, device=DEV)
    pos = torch.zeros(5, 32, dtype=torch.int32, device=DEV)
    P, st = _lib.ptr, _lib.stream_handle()
    good = [st, P(U), P(I), P(ub), P(ib), 16, P(users), P(ptr), P(idx), 5, P(out)]
    assert L.rg_mf_score_lists(*good) == _lib.RG_OK
    for at in (1, 2, 3, 4, 6, 7, 8, 10):
        a = list(good)
        a[at] = None
        assert L.rg_mf_score_lists(*a) == -1 and b"null" in L.rg_last_error()
    for at, v in ((5, 0), (5, 257), (9, -1)):
        a = list(good)
        a[at] = v
        assert L.rg_mf_score_lists(*a) == -1
    good = [st, P(out), P(ptr), P(idx), 5, 10, P(pos), None]
    assert L.rg_seg_topk(*good) == _lib.RG_OK
    for at, v in ((1, None), (2, None), (3, None), (6, None), (5, 0), (5, 33), (4, -1)):
        a = list(good)
        a[at] = v
        assert L.rg_seg_topk(*a) == -1
    good = [st, P(out), P(ptr), P(idx), 5, P(pos)]
    assert L.rg_seg_rank(*good) == _lib.RG_OK
    for at, v in ((1, None), (2, None), (3, None), (5, None), (4, -1)):
        a = list(good)
        a[at] = v
        assert L.rg_seg_rank(*a) == -1
    torch.cuda.synchronize()
