"""MF all-item scoring on the GPU (rg_mf_score_users through the C-ABI, and through the model).

* Against float64 NumPy at rtol=1e-5, atol=1e-7 (the project's tolerance for a score block; checked
  for a sequential fp32 sum on the host in tests/test_mf_score_cpu.py) at the shapes where the
  kernel can go wrong: item counts around its tile, user counts around its group, every kind of
  dim (below 4, not a multiple of 4, one chunk, several chunks, the largest), unsorted ids with a
  duplicate, a padded row stride and spare rows that must stay untouched.
* Exact logits (multiples of 1/64): the block equals rg_mf_scores bit for bit, and topk_users
  equals the stable argsort of the float64 logits, ties included.
* The same bits on a repeated call, at any position of a block, in a block of one, and from
  tables that are not 16-byte aligned (the scalar loads).
* Through ImplicitFactorizationModel: score_users is the kernel's block, the rankings and the
  metrics follow, a bad id raises, and the stand-in bench.py builds works on CUDA tables.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from recommendation_gans_amd import _lib
from tests.mf_score_common import ATOL, DIMS, GRID_DIMS, RTOL, block64, exact_tables, logits64, random_tables
from tests.ncf_infer_common import DEV, HostOnly, make_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, GROUP = _lib.RG_MF_SCORE_ITEM_TILE, _lib.RG_MF_SCORE_USER_GROUP
ITEM_COUNTS = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7]
USER_COUNTS = [1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 2]
SENTINEL, LD_PAD, SPARE_ROWS = -7.0, 5, 3


def on_device(tabs, n_items=None):
    uw, iw, ub, ib = tabs
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (uw, iw[:n_items], ub, ib[:n_items])]


def score(dt, users, ld=None, spare_rows=0):
    """rg_mf_score_users on device tables `dt` into a (len(users) + spare_rows, ld) buffer filled with
    the sentinel beforehand; the whole buffer comes back."""
    U, I, ub, ib = dt
    n, num_items = len(users), int(I.shape[0])
    ld = num_items if ld is None else ld
    u = torch.as_tensor(np.asarray(users, dtype=np.int64), device=DEV)
    out = torch.full((n + spare_rows, ld), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().rg_mf_score_users(_lib.stream_handle(), _lib.ptr(U), _lib.ptr(I), _lib.ptr(ub), _lib.ptr(ib),
                                             int(U.shape[1]), num_items, _lib.ptr(u), n, _lib.ptr(out), ld),
               "rg_mf_score_users")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def user_ids(n, U, seed):
    """n ids out of U, unsorted, with a duplicate when n > 1."""
    u = np.random.RandomState(seed).randint(0, U, n)
    if n > 1:
        u[-1] = u[0]
    return u


@pytest.mark.parametrize("dim", sorted(set(DIMS + GRID_DIMS)))
def test_matches_float64_at_edge_shapes(dim):
    """The full item-count x user-count grid at dims 16 and 64; at every other dim the diagonal of
    the grid (every item count and every user count once)."""
    U, Imax = max(USER_COUNTS) + 9, max(ITEM_COUNTS)
    tabs = random_tables(U, Imax, dim, seed=1000 + dim)
    ref = block64(tabs, np.arange(U))                         # (U, Imax), once
    shapes = [(I, n) for I in ITEM_COUNTS for n in USER_COUNTS] if dim in GRID_DIMS else \
        list(zip(ITEM_COUNTS, USER_COUNTS))
    worst, dts = 0.0, {}
    for I, n in shapes:
        dt = dts.setdefault(I, on_device(tabs, n_items=I))
        u = user_ids(n, U, seed=I + n)
        got = score(dt, u, ld=I + LD_PAD, spare_rows=SPARE_ROWS)
        assert (got[:, I:] == SENTINEL).all(), (I, n, "padding columns written")
        assert (got[n:] == SENTINEL).all(), (I, n, "rows past n_users written")
        want = ref[u][:, :I]
        worst = max(worst, float(np.max(np.abs(got[:n, :I] - want) / np.abs(want))))
        np.testing.assert_allclose(got[:n, :I], want, rtol=RTOL, atol=ATOL, err_msg=f"dim={dim} I={I} n={n}")
    print(f"dim={dim} shapes={len(shapes)} max rel diff {worst:.3g}")


# ---------------------------------------------------------------- exact logits
EX_U, EX_I, EX_DIM = 70, 3 * TILE + 7, 16


@pytest.fixture(scope="module")
def exact():
    tabs = exact_tables(EX_U, EX_I, EX_DIM, seed=3)
    users = np.random.RandomState(5).permutation(EX_U)
    z = logits64(tabs, users)
    assert np.abs(z).max() <= 5 and (z * 64 == np.round(z * 64)).all()
    return tabs, on_device(tabs), users, z


def test_exact_block_equals_the_pair_kernel_bit_for_bit(exact):
    tabs, dt, users, z = exact
    got = score(dt, users)
    n, I = len(users), EX_I
    pu = torch.as_tensor(np.repeat(users, I).astype(np.int64), device=DEV)
    pi = torch.arange(I, device=DEV).repeat(n)
    out = torch.empty(n * I, dtype=torch.float32, device=DEV)
    U, It, ub, ib = dt
    _lib.check(_lib.load().rg_mf_scores(_lib.stream_handle(), _lib.ptr(U), _lib.ptr(It), _lib.ptr(ub), _lib.ptr(ib),
                                        EX_DIM, _lib.ptr(pu), _lib.ptr(pi), n * I, _lib.ptr(out)), "rg_mf_scores")
    torch.cuda.synchronize()
    assert got.tobytes() == out.cpu().numpy().reshape(n, I).tobytes()
    np.testing.assert_allclose(got, 1.0 / (1.0 + np.exp(-z)), rtol=RTOL, atol=ATOL)


def stand_in(dt, num_items):
    """The model stand-in of bench.py --model eval: the model's own evaluation methods over bare tables."""
    sys.path.insert(0, ROOT)
    import bench
    return bench.eval_model(dt, num_items, torch.device(DEV))


@pytest.mark.parametrize("exclude", [False, True])
def test_exact_topk_is_the_stable_argsort_of_the_float64_logits(exact, exclude):
    tabs, dt, users, z = exact
    k, z = 10, z.copy()
    first = np.argsort(-z, axis=1, kind="stable")
    # ties occur inside the first k and across its edge: the lower item id must come first
    zs = np.take_along_axis(z, first[:, :k + 1], axis=1)
    assert (zs[:, :-1] == zs[:, 1:]).any() and (zs[:, k - 1] == zs[:, k]).any()
    csr = None
    if exclude:
        # each user's three best items, a tie partner among them for some, and a few random ones
        rs = np.random.RandomState(9)
        cols =np.concatenate([np.concatenate([first[r, :3], rs.randint(0, EX_I, 3)]) for r in range(len(users))])
        rows = np.repeat(users, 6)
        csr = sp.csr_matrix((np.ones(len(cols), np.float32), (rows, cols)), shape=(EX_U, EX_I))
        for r, u in enumerate(users):
            z[r, csr[u].indices] = -np.inf
    got = stand_in(dt, EX_I).topk_users(users, k, csr)
    want = np.argsort(-z, axis=1, kind="stable")[:, :k]
    assert got.dtype == np.int64 and (got == want).all()


# ---------------------------------------------------------------- the same bits everywhere
@pytest.mark.parametrize("dim", [64, 100, 128])
def test_same_bits_on_any_call_at_any_position_in_any_block(dim):
    U, I = 40, 3 * TILE + 7
    dt = on_device(random_tables(U, I, dim, seed=dim))
    u = user_ids(2 * GROUP + 2, U, seed=2)
    for pos in (0, 17, GROUP - 1, GROUP + 3, 2 * GROUP + 1):      # other waves, other groups, the masked tail
        u[pos] = 5
    a, b = score(dt, u), score(dt, u)
    assert a.tobytes() == b.tobytes()
    one = score(dt, [5])
    for pos in np.flatnonzero(u == 5):
        assert a[pos].tobytes() == one[0].tobytes(), pos
    assert not (a == SENTINEL).any()


@pytest.mark.parametrize("dim", [8, 64])
def test_unaligned_tables_take_the_scalar_loads_and_give_the_same_bits(dim):
    """dim % 4 == 0 but tables that start 4 bytes past a 16-byte boundary: no 16-byte loads; the
    sums keep their order, so the block keeps its bits."""
    U, I = 20, TILE + 9
    tabs = random_tables(U, I, dim, seed=7)
    dt = on_device(tabs)
    shifted = []
    for t in dt[:2]:
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        shifted.append(v)
    u = user_ids(17, U, seed=3)
    a, b = score(dt, u), score(shifted + dt[2:], u)
    assert a.tobytes() == b.tobytes()
    np.testing.assert_allclose(a, block64(tabs, u), rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------- through the model
def test_model_paths_use_the_kernel(tmp_path, monkeypatch):
    from recommendation_gans_amd.spotlight import evaluation
    model, train, test = make_model("mf", tmp_path, monkeypatch, U=75, I=3 * TILE + 7, n_test=300)
    e, U, I = model._engine, model._num_users, model._num_items
    users = np.array([7, 3, 70, 3, 0, 74, 12])
    block = model.score_users(users)
    assert block.shape == (len(users), I) and block.dtype == np.float32
    # the kernel's block on the engine's own tables, bit for bit: the path is taken
    direct = score(list(e.params()), users)
    assert block.tobytes() == direct.tobytes()
    ut = torch.as_tensor(users, device=e.device)
    pair = e.scores(ut.repeat_interleave(I), torch.arange(I, device=e.device).repeat(len(users)))
    np.testing.assert_allclose(block, pair.reshape(len(users), I).cpu().numpy(), rtol=RTOL, atol=ATOL)
    with pytest.raises(ValueError):
        model.score_users(np.array([0, U]))
    with pytest.raises(ValueError):
        model.score_users(np.array([-1, 2]))
    # ranking: the stable argsort of the model's own block, excluded items at -inf
    k, csr = 10, train.tocsr()
    got = model.topk_users(users, k, csr)
    x = block.copy()
    for r, u in enumerate(users):
        x[r, csr[u].indices] = -np.inf
    assert (got == np.argsort(-x, axis=1, kind="stable")[:, :k]).all()
    h = HostOnly(model)
    for k in (1, 5):
        assert evaluation.precision_recall_score(model, test, k=k) == evaluation.precision_recall_score(h, test, k=k)
        assert evaluation.precision_recall_score(model, test, train, k=k) == \
            evaluation.precision_recall_score(h, test, train, k=k)
        assert evaluation.map_at_k(model, test, k=k) == evaluation.map_at_k(h, test, k=k)
    for tr in (None, train):    # the two paths sum the same ranks; the tolerance of tests/test_rank_gpu.py
        np.testing.assert_allclose(evaluation.mrr_score(model, test, tr), evaluation.mrr_score(h, test, tr),
                                   rtol=1e-12, atol=0)


def test_stand_in_model_works_on_cuda_tables():
    """bench.py --model eval binds the model's evaluation methods to a stand-in that holds only the
    tables: they must read nothing else, and take the kernel."""
    U, I, dim = 90, 2 * TILE + 3, 64
    tabs = random_tables(U, I, dim, seed=4)
    dt = on_device(tabs)
    m = stand_in(dt, I)
    users = user_ids(GROUP + 5, U, seed=6)
    block = m.score_users(users)
    assert block.dtype == np.float32 and block.tobytes() == score(dt, users).tobytes()
    top = m.topk_users(users, 5)
    assert (top == np.argsort(-block, axis=1, kind="stable")[:, :5]).all()
    with pytest.raises(ValueError):
        m.score_users([U])
