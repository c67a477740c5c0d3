"""Diversified re-ranking on the GPU: rg_seg_mmr bit for bit against rg_seg_topk at lam = 1 and against
the float64 reference where the arithmetic is exact, replayed in float64 within the derived bound on
random tables, its penalties, values and fills, locality, the two staging paths, rg_seg_mean_sim, and
the model-level calls for MF, NCF and NeuMF.  Every case in a few seconds."""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import candidates as cand, mf_engine
from recommendation_gans_amd.spotlight import evaluation as ev
from tests import candidates_common as cc
from tests import diverse_common as dc
from tests.ncf_infer_common import make_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
t = torch.from_numpy


def dev(*arrays):
    return [t(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def rnorms(table_dev):
    return mf_engine.row_rnorms(table_dev)


def mmr(scores, ptr, idx, table, k, lam, cosine):
    """(pos, val, pen, the device's reciprocal norms as float64 or None) of one call."""
    s, p, i, T = dev(scores, ptr, idx, table)
    rn = rnorms(T) if cosine else None
    before = T.clone()
    pos, val, pen = cand.seg_mmr(s, p, i, T, k, lam, rnorm=rn, return_values=True, return_penalties=True)
    torch.cuda.synchronize()
    assert torch.equal(T, before), "the table is only read"
    assert pos.dtype == torch.int32 and val.dtype == torch.float32 and pen.dtype == torch.float32
    assert pos.shape == val.shape == pen.shape == (len(ptr) - 1, k)
    return pos.cpu().numpy(), val.cpu().numpy(), pen.cpu().numpy()


def check_values_and_fills(scores, ptr, pos, val, pen):
    lens = np.diff(ptr)
    k = pos.shape[1]
    short = np.arange(k)[None, :] >= lens[:, None]
    assert (pos[short] == -1).all() and (pos[~short] >= 0).all()
    assert np.isneginf(val[short]).all() and (pen[short] == 0).all() and (pen[:, 0] == 0).all()
    at = (ptr[:-1, None] + np.maximum(pos, 0))[~short]
    assert val[~short].tobytes() == scores[at].tobytes(), "the raw score at each position"


# ---------------------------------------------------------------- kernel level
@pytest.mark.parametrize("kind", cc.SEG_KINDS)
def test_lam_one_is_seg_topk_bit_for_bit(kind):
    scores, ptr, idx = cc.seg_case(kind)
    table = dc.sim_table(16)
    s, p, i = dev(scores, ptr, idx)
    for k in cc.KS:
        want_pos, want_val = (x.cpu().numpy() for x in cand.seg_topk(s, p, i, k, return_values=True))
        for cosine in (False, True):
            pos, val, pen = mmr(scores, ptr, idx, table, k, 1.0, cosine)
            assert pos.tobytes() == want_pos.tobytes(), (kind, k, cosine)
            assert val.tobytes() == want_val.tobytes(), (kind, k, cosine)
            assert (pos == cc.ref_topk(scores, ptr, idx, k)).all()


@pytest.mark.parametrize("dim", dc.EXACT_DIMS)
@pytest.mark.parametrize("lam", dc.EXACT_LAMS)
def test_exact_arithmetic_equals_the_float64_reference(dim, lam):
    scores, ptr, idx = cc.seg_case("quantised")
    table = dc.grid_table(dim)
    for k in (10, 32):
        want_pos, want_val, want_pen = dc.ref_mmr(scores, ptr, idx, table, k, lam)
        assert np.abs(want_pen).max() < 17 and (want_pen * 64 == np.round(want_pen * 64)).all()
        pos, val, pen = mmr(scores, ptr, idx, table, k, lam, cosine=False)
        assert (pos == want_pos).all(), (dim, lam, k)
        assert (pen.astype(np.float64) == want_pen).all() and (val.astype(np.float64) == want_val).all()
    ties = sum(len(np.unique(scores[ptr[r]:ptr[r + 1]])) < ptr[r + 1] - ptr[r] for r in range(len(ptr) - 1))
    assert ties > 10, "ties are the rule in this case"


@pytest.mark.parametrize("dim", dc.COS_DIMS)
@pytest.mark.parametrize("lam", [0.3, 0.7])
@pytest.mark.parametrize("kind", ["random", "repeats"])
def test_cosine_replayed_in_float64_within_the_derived_bound(dim, lam, kind):
    scores, ptr, idx = cc.seg_case(kind)
    table = dc.sim_table(dim)
    rn = dc.rnorms64(table)
    worst = (0.0, 0.0)
    for k in (10, 32):
        pos, val, pen = mmr(scores, ptr, idx, table, k, lam, cosine=True)
        check_values_and_fills(scores, ptr, pos, val, pen)
        got = dc.replay(scores, ptr, idx, table, dc.lam32(lam), pos, rn, pen_out=pen)
        worst = (max(worst[0], got[0]), max(worst[1], got[1]))
    print(f"\ndim {dim} lam {lam} {kind}: largest share of the bound used: objective {worst[0]:.3f}, "
          f"penalty {worst[1]:.3f}")


@pytest.mark.parametrize("cosine", [False, True])
def test_penalties_values_and_fills(cosine):
    scores, ptr, idx = cc.seg_case("repeats", seed=2)
    table = dc.sim_table(65)
    rn = dc.rnorms64(table) if cosine else None
    for k in cc.KS:
        pos, val, pen = mmr(scores, ptr, idx, table, k, 0.5, cosine)
        check_values_and_fills(scores, ptr, pos, val, pen)
        dc.replay(scores, ptr, idx, table, 0.5, pos, rn, pen_out=pen)
    # the optional outputs do not change the positions
    s, p, i, T = dev(scores, ptr, idx, table)
    only = cand.seg_mmr(s, p, i, T, 10, 0.5, rnorm=rnorms(T) if cosine else None)
    assert torch.is_tensor(only) and only.cpu().numpy().tobytes() == mmr(scores, ptr, idx, table, 10, 0.5, cosine)[0].tobytes()


def test_a_lists_output_depends_on_that_list_alone():
    scores, ptr, idx = cc.seg_case("repeats", seed=1)
    table = dc.sim_table(16)
    n, k = len(ptr) - 1, 10
    full = mmr(scores, ptr, idx, table, k, 0.6, True)
    rev = np.arange(n)[::-1]
    part = mmr(*cc.take_lists(scores, ptr, idx, rev), table, k, 0.6, True)
    for a, b in zip(full, part):
        assert b.tobytes() == a[rev].tobytes()
    for r in (int(np.argmax(np.diff(ptr))), int(np.flatnonzero(np.diff(ptr) == 33)[0])):
        alone = mmr(*cc.take_lists(scores, ptr, idx, [r]), table, k, 0.6, True)
        for a, b in zip(full, alone):
            assert b.tobytes() == a[r:r + 1].tobytes()


def test_staged_and_gathered_rows_give_the_same_bits():
    """dim 256: a list of up to 63 entries is staged in LDS (63 * 257 floats fit 64 KiB), a longer one
    reads its rows from the table at every step.  The first 60 entries of a 1000-entry list score 10
    above the rest, so every pick of the long list comes from them (a cosine penalty moves an
    objective by less than 2 (1 - lam) = 1): the prefix as a list of its own must give the same
    positions, values and penalty bits."""
    rs = np.random.RandomState(5)
    dim, k, lam = 256, 32, 0.5
    table = dc.sim_table(dim)
    for length in (1000, 1024, 64):
        idx = rs.randint(0, dc.TABLE_ROWS, length).astype(np.int32)
        scores = rs.rand(length).astype(np.float32)
        scores[:60] += 10
        ptr = np.array([0, length], np.int64)
        long_ = mmr(scores, ptr, idx, table, k, lam, True)
        short = mmr(scores[:60], np.array([0, 60], np.int64), idx[:60], table, k, lam, True)
        assert (long_[0] < 60).all()
        for a, b in zip(long_, short):
            assert a.tobytes() == b.tobytes(), length
        dc.replay(scores, ptr, idx, table, lam, long_[0], dc.rnorms64(table), pen_out=long_[2])
    # 1025 entries: the wrapper refuses
    s, p, i, T = dev(np.zeros(1025, np.float32), np.array([0, 1025], np.int64), np.zeros(1025, np.int32), table)
    with pytest.raises(ValueError, match="longer than 1024"):
        cand.seg_mmr(s, p, i, T, 5, 0.5)
    with pytest.raises(ValueError, match="longer than 1024"):
        cand.seg_mean_sim(p, i, T)


@pytest.mark.parametrize("dim", [3, 16, 65, 256])
def test_seg_mean_sim_within_the_similarity_bound(dim):
    rs = np.random.RandomState(dim)
    lengths = rs.permutation(np.minimum(cc.LENGTHS + [1024], 1024))
    ptr = cc.list_ptr(lengths)
    idx = rs.randint(0, dc.TABLE_ROWS, int(ptr[-1])).astype(np.int32)
    idx[rs.rand(len(idx)) < 0.2] = -1                      # skipped
    table = dc.sim_table(dim)
    p, i, T = dev(ptr, idx, table)
    for cosine in (True, False):
        rn = rnorms(T) if cosine else None
        got = cand.seg_mean_sim(p, i, T, rnorm=rn).cpu().numpy()
        want, bound = dc.mean_sim64(ptr, idx, table, dc.rnorms64(table) if cosine else None)
        assert got.dtype == np.float32 and got.shape == want.shape
        few = np.array([(idx[ptr[r]:ptr[r + 1]] >= 0).sum() < 2 for r in range(len(lengths))])
        assert few.any() and (got[few] == 0).all()
        share = np.abs(got.astype(np.float64) - want)[~few] / bound[~few]
        print(f"\ndim {dim} cosine {cosine}: largest share of the bound {share.max():.3f}")
        assert (share <= 1.0).all()
        # a list alone, and the lists reversed: the same bits
        rev = np.arange(len(lengths))[::-1]
        _, p2, i2 = cc.take_lists(idx.astype(np.float32), ptr, idx, rev)
        again = cand.seg_mean_sim(*dev(p2, i2), T, rnorm=rn).cpu().numpy()
        assert again.tobytes() == got[rev].tobytes()


def test_python_refusals_and_empty_calls():
    scores, ptr, idx = cc.seg_case("random")
    table = dc.sim_table(16)
    s, p, i, T = dev(scores, ptr, idx, table)
    rn = rnorms(T)

    def bad(fn, *a, **kw):
        with pytest.raises(ValueError):
            fn(*a, **kw)
    for args in ((s.double(), p, i, T), (s.cpu(), p, i, T), (s[:-1], p, i, T), (s, p.int(), i, T), (s, p, i.long(), T),
                 (s, p + 1, i, T), (s, p, i, T.double()), (s, p, i, T.cpu()), (s, p, i, T[:, ::2]), (s, p, i, T[0]),
                 (s, p, i + dc.TABLE_ROWS, T), (s, p, -i - 1, T), (s, p, i, torch.zeros(4, 257, device=DEV))):
        bad(cand.seg_mmr, *args, 5, 0.5)
    bad(cand.seg_mmr, s, p, i, T, 5, 0.5, rnorm=rn[:-1])
    bad(cand.seg_mmr, s, p, i, T, 5, 0.5, rnorm=rn.double())
    bad(cand.seg_mmr, s, p, i, T, 5, 0.5, rnorm=rn.cpu())
    for k in (0, 33, 2.5):
        bad(cand.seg_mmr, s, p, i, T, k, 0.5)
    for lam in (0.0, 1.5, float("nan")):
        bad(cand.seg_mmr, s, p, i, T, 5, lam)
    for args in ((p.int(), i, T), (p, i.long(), T), (p + 1, i, T), (p, i, T.double()), (p, i + dc.TABLE_ROWS, T),
                 (p.cpu(), i, T)):
        bad(cand.seg_mean_sim, *args)
    bad(cand.seg_mean_sim, p, i, T, rnorm=rn[:-1])
    # every list empty, and no lists: filled outputs, no launch
    z, e_s, e_i = t(np.zeros(4, np.int64)).to(DEV), torch.zeros(0, device=DEV), torch.zeros(0, dtype=torch.int32,
                                                                                         device=DEV)
    pos, val, pen = cand.seg_mmr(e_s, z, e_i, T, 3, 0.5, return_values=True, return_penalties=True)
    assert pos.shape == (3, 3) and (pos.cpu().numpy() == -1).all() and np.isneginf(val.cpu().numpy()).all()
    assert (pen.cpu().numpy() == 0).all()
    assert cand.seg_mmr(e_s, z[:1], e_i, T, 3, 0.5).shape == (0, 3)
    assert cand.seg_mean_sim(z, e_i, T).cpu().numpy().tolist() == [0.0, 0.0, 0.0]
    # empty lists beside a full one go through the kernel
    got = mmr(np.array([1.0, 2.0], np.float32), np.array([0, 0, 2, 2], np.int64), np.array([5, 6], np.int32), table, 3,
              0.5, True)
    assert got[0].tolist() == [[-1, -1, -1], [1, 0, -1], [-1, -1, -1]]


def test_seg_mmr_torch_on_the_device_agrees_where_float64_is_clear():
    """The timing baseline runs on the device in float32: its picks pass the same replay."""
    scores, ptr, idx = cc.seg_case("random", seed=3)
    table = dc.sim_table(16)
    s, p, i, T = dev(scores, ptr, idx, table)
    pos = cand.seg_mmr_torch(s, p, i, T, 10, 0.7, rnorm=rnorms(T)).cpu().numpy()
    dc.replay(scores, ptr, idx, table, dc.lam32(0.7), pos, dc.rnorms64(table))


# ---------------------------------------------------------------- model level
def model_of(kind, tmp_path, monkeypatch):
    model, train, _ = make_model(kind, tmp_path, monkeypatch, cc.MODEL_U, cc.MODEL_I, 50, E=cc.MODEL_E, M=cc.MODEL_M)
    if kind == "mf":
        cc.load_tables(model, cc.untied_tables())
    return model, train


def item_table64(model, space=None):
    return model._item_table(space).detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("kind", ["mf", "ncf", "neumf"])
def test_lam_one_is_recommend_and_rank_candidates(kind, tmp_path, monkeypatch):
    model, train = model_of(kind, tmp_path, monkeypatch)
    everyone = np.arange(cc.MODEL_U)
    for k, pool in ((10, 100), (32, 32), (1, 300), (5, 33)):
        for exclude in (None, train):
            ids, sc = model.recommend(everyone, k=k, exclude=exclude, return_scores=True)
            got, gsc = model.recommend_diverse(everyone, k=k, pool=pool, lam=1.0, exclude=exclude, return_scores=True)
            assert got.dtype == np.int64 and gsc.dtype == np.float32 and got.shape == (cc.MODEL_U, k)
            assert (got == ids).all() and gsc.tobytes() == sc.tobytes(), (kind, k, pool)
            assert (model.recommend_diverse(everyone, k=k, pool=pool, lam=1.0, exclude=exclude) == ids).all()
    rs = np.random.RandomState(2)
    users = rs.randint(0, cc.MODEL_U, 23)
    lists = [rs.randint(0, cc.MODEL_I, n) for n in np.resize([0, 1, 5, 33, 64, 65, 200], 23)]
    for k in (1, 10, 32):
        ids, sc = model.rank_candidates(users, lists, k=k, return_scores=True)
        got, gsc = model.diversify_candidates(users, lists, k=k, lam=1.0, return_scores=True)
        assert (got == ids).all() and gsc.tobytes() == sc.tobytes()
        assert (model.diversify_candidates(users, lists, k=k, lam=1.0, metric="dot") == ids).all()


@pytest.mark.parametrize("kind", ["mf", "ncf", "neumf"])
def test_model_methods_at_lam_half_replay_against_float64_scores(kind, tmp_path, monkeypatch):
    model, train = model_of(kind, tmp_path, monkeypatch)
    blk, bound = cc.model_block64(kind)
    bound = np.broadcast_to(bound, blk.shape)
    table = item_table64(model, "mf" if kind == "neumf" else None)        # NeuMF's default space
    rn = dc.rnorms64(table)
    k, pool = cc.MODEL_K, 100
    # diversify_candidates over lists with repeats
    rs = np.random.RandomState(3)
    users = rs.randint(0, cc.MODEL_U, 23)
    lists = [rs.randint(0, cc.MODEL_I, n) for n in np.resize([0, 1, 5, 33, 64, 65, 200], 23)]
    ptr = cc.list_ptr([len(x) for x in lists])
    flat = np.concatenate(lists).astype(np.int64)
    rows = np.repeat(users, np.diff(ptr))
    ids, sc = model.diversify_candidates(users, lists, k=k, lam=0.5, return_scores=True)
    scored = model.score_candidates(users, lists)
    pos = np.full(ids.shape, -1, np.int32)
    for r in range(len(users)):                 # ids back to positions: the entry of that id and score, first unused
        used = set()
        for j in range(k):
            if ids[r, j] < 0:
                continue
            c = [e for e in range(ptr[r], ptr[r + 1]) if flat[e] == ids[r, j] and e not in used and
                 scored[e].tobytes() == sc[r, j].tobytes()]
            used.add(c[0])
            pos[r, j] = c[0] - ptr[r]
    worst = dc.replay(blk[rows, flat], ptr, flat, table, 0.5, pos, rn, key_bound=bound[rows, flat])
    assert (np.abs(scored.astype(np.float64) - blk[rows, flat]) <= bound[rows, flat]).all()
    # recommend_diverse: the pool is the float64 block's top `pool` wherever the device retrieved the same set
    everyone = np.arange(cc.MODEL_U)
    got, gsc = model.recommend_diverse(everyone, k=k, pool=pool, lam=0.5, exclude=train, return_scores=True)
    cands = model.recommend_diverse(everyone, k=32, pool=pool, lam=1.0, exclude=train)      # in rank order
    wide = model.topk_users(everyone, pool, exclude_csr=train.tocsr())
    assert (wide[:, :32] == cands).all()
    p2 = cc.list_ptr([pool] * cc.MODEL_U)
    flat2 = wide.reshape(-1)
    rows2 = np.repeat(everyone, pool)
    s64 = blk[rows2, flat2].copy()
    tr = train.tocsr()
    s64[np.asarray(tr[rows2, flat2]).reshape(-1) > 0] = -np.inf
    pos2 = np.array([[int(np.flatnonzero(wide[r] == i)[0]) for i in got[r]] for r in everyone], np.int32)
    w2 = dc.replay(s64, p2, flat2, table, 0.5, pos2, rn, key_bound=bound[rows2, flat2])
    print(f"\n{kind}: largest share of the bound used: diversify_candidates {worst[0]:.3f}, recommend_diverse {w2[0]:.3f}")
    assert (got != model.recommend(everyone, k=k, exclude=train)).any(), "lam = 0.5 changes some list"
    assert (np.abs(gsc.astype(np.float64) - blk[everyone[:, None], got]) <= bound[everyone[:, None], got]).all()


def test_intra_list_similarity_and_the_spaces(tmp_path, monkeypatch):
    model, train = model_of("neumf", tmp_path, monkeypatch)
    everyone = np.arange(cc.MODEL_U)
    plain = model.recommend(everyone, k=10)
    for space in ("mf", "mlp"):
        table = item_table64(model, space)
        for metric in ("cosine", "dot"):
            rn = dc.rnorms64(table) if metric == "cosine" else None
            div = model.recommend_diverse(everyone, k=10, pool=100, lam=0.5, metric=metric, space=space)
            lists = np.concatenate([plain, div])
            lists[3, 4:] = -1                                   # a short list's fill
            lists[5, 1:] = -1                                   # one item: counts 0
            want, bound = dc.mean_sim64(cc.list_ptr([10] * len(lists)), lists.reshape(-1), table, rn)
            got = ev.intra_list_similarity(model, lists, metric=metric, space=space)
            assert abs(got - want.mean()) <= bound.mean() + 1e-7 * abs(want.mean())
            assert ev.intra_list_similarity(model, [list(r) for r in lists], metric=metric, space=space) == got
            a = ev.intra_list_similarity(model, plain, metric=metric, space=space)
            b = ev.intra_list_similarity(model, div, metric=metric, space=space)
            print(f"\nNeuMF {space} {metric}: intra-list similarity {a:.4f} (relevance) -> {b:.4f} (lam 0.5)")
            if metric == "cosine":      # 40 lists of 10 out of 100: greedy max-similarity avoidance lowers the mean
                assert b < a, "the re-ranking lowers the similarity it penalises"
    assert ev.intra_list_similarity(model, plain) == ev.intra_list_similarity(model, plain, space="mf")
    # the tower's table is the one used: the picks differ between the spaces, and those of "mlp" replay
    # in float64 against the tower's table
    d_mf = model.recommend_diverse(everyone, k=10, pool=100, lam=0.3, space="mf")
    d_mlp = model.recommend_diverse(everyone, k=10, pool=100, lam=0.3, space="mlp")
    assert (d_mf != d_mlp).any()
    assert model._item_table("mlp").shape[1] == cc.MODEL_E and model._item_table("mf").shape[1] == cc.MODEL_M
    blk, bound = cc.model_block64("neumf")
    rs = np.random.RandomState(6)
    users = everyone[:20]
    lists = np.stack([rs.permutation(cc.MODEL_I)[:80] for _ in users])          # no repeats: an id is a position
    ids = model.diversify_candidates(users, lists, k=10, lam=0.5, space="mlp")
    pos = np.array([[int(np.flatnonzero(lists[r] == i)[0]) for i in ids[r]] for r in range(len(users))], np.int32)
    rows, flat = np.repeat(users, 80), lists.reshape(-1)
    tower = item_table64(model, "mlp")
    dc.replay(blk[rows, flat], cc.list_ptr([80] * len(users)), flat, tower, 0.5, pos, dc.rnorms64(tower),
              key_bound=np.broadcast_to(bound, blk.shape)[rows, flat])
    mf, _ = model_of("mf", tmp_path, monkeypatch)
    with pytest.raises(ValueError, match="unknown space"):
        mf.recommend_diverse(everyone, space="mlp")
