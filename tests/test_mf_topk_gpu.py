"""The fused MF top-k on the GPU (rg_mf_topk_users through mf_engine.topk_users_fused).

The oracle is computed on the host from the block rg_mf_score_users writes
(mf_engine.score_users_block, downloaded): NaN -> -inf for the key, -inf at the excluded entries,
the first k of a stable argsort of the negated key.  Ids are compared for equality, scores as bytes
against the block at those ids with -inf at the excluded ones: no tolerance, the kernel's contract
is bit equality.  Every axis is taken at its edges with the others at a mid value: item counts
around the tile, user counts around the group, the dims of the scalar-load path, of a second K
chunk and the largest, k at the boundaries of the three instantiations and k == num_items.  Every
call is made twice and must give the same bytes; every id must be in [0, num_items) and distinct
within its row.  No call passes a user id outside the table to the kernel."""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib, mf_engine
from tests.mf_score_common import random_tables
from tests.ncf_infer_common import DEV

pytestmark = pytest.mark.gpu

TILE, GROUP = _lib.RG_MF_SCORE_ITEM_TILE, _lib.RG_MF_SCORE_USER_GROUP
ITEM_COUNTS = [1, 33, TILE - 1, TILE, TILE + 1, 3 * TILE + 7]
USER_COUNTS = [1, 15, 17, 64, 65, 130]
DIMS = [1, 3, 4, 64, 68, 256]
KS = [1, 8, 9, 16, 17, 32]
NEG_INF = np.float32(-np.inf)


def on_device(tabs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in tabs]


def user_ids(n, U, seed):
    """n ids out of U, unsorted, with a repeated user when n > 1."""
    u = np.random.RandomState(seed).randint(0, U, n)
    if n > 1:
        u[-1] = u[0]
    return u


def csr(rows):
    """(ptr int64, idx int32) of a list of per-row id lists, as given."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([i for r in rows for i in r], dtype=np.int32)


def random_exclusions(n, num_items, seed, per_row=5):
    """Sorted ids per row, up to per_row of them, with an empty row among full ones."""
    rs = np.random.RandomState(seed)
    rows = [sorted(rs.choice(num_items, min(per_row, num_items - 1), replace=False).tolist()) for _ in range(n)]
    if n > 2:
        rows[1] = []
    return rows


def oracle(dt, users, k, exc):
    block = mf_engine.score_users_block(*dt, users).cpu().numpy()
    num_items = block.shape[1]
    gone = np.zeros(block.shape, dtype=bool)
    for r, ids in enumerate(exc or []):
        for i in ids:
            if 0 <= i < num_items:
                gone[r, i] = True
    key = np.where(np.isnan(block), NEG_INF, block)
    key[gone] = NEG_INF
    ids = np.argsort(-key, axis=1, kind="stable")[:, :k]
    scores = np.where(np.take_along_axis(gone, ids, 1), NEG_INF, np.take_along_axis(block, ids, 1))
    return ids, scores.astype(np.float32), block


def fused(dt, users, k, exc=None, splits=0):
    e_ptr, e_idx = csr(exc) if exc is not None else (None, None)
    ids, sc = mf_engine.topk_users_fused(*dt, users, k, e_ptr, e_idx, splits=splits)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def check(dt, users, k, exc=None, splits=0):
    """The kernel against the oracle, twice; returns (ids, scores, block)."""
    want_ids, want_sc, block = oracle(dt, users, k, exc)
    ids, sc = fused(dt, users, k, exc, splits)
    num_items = block.shape[1]
    assert ids.dtype == np.int32 and sc.dtype == np.float32 and ids.shape == sc.shape == (len(users), k)
    assert ids.min() >= 0 and ids.max() < num_items, "an id outside [0, num_items)"
    assert all(len(set(row)) == k for row in ids.tolist()), "a repeated id in a row"
    assert (ids == want_ids).all(), (np.argwhere(ids != want_ids)[:5], ids[ids != want_ids][:5])
    assert sc.tobytes() == want_sc.tobytes()
    again = fused(dt, users, k, exc, splits)
    assert again[0].tobytes() == ids.tobytes() and again[1].tobytes() == sc.tobytes()
    return ids, sc, block


def test_one_small_shape():
    """The narrowest case: one tile, one user group, one K chunk, K = 8, nothing excluded."""
    dt = on_device(random_tables(20, 33, 4, seed=1))
    check(dt, user_ids(15, 20, 2), 8, splits=1)


@pytest.mark.parametrize("num_items", ITEM_COUNTS)
def test_item_counts_around_the_tile(num_items):
    dt = on_device(random_tables(30, num_items, 64, seed=10 + num_items))
    users = user_ids(17, 30, 3)
    k = min(9, num_items)
    check(dt, users, k, random_exclusions(17, num_items, seed=num_items) if num_items > 1 else None)
    check(dt, users, k)


@pytest.mark.parametrize("n", USER_COUNTS)
def test_user_counts_around_the_group(n):
    dt = on_device(random_tables(140, TILE + 1, 64, seed=20 + n))
    check(dt, user_ids(n, 140, 4), 9, random_exclusions(n, TILE + 1, seed=n))


@pytest.mark.parametrize("dim", DIMS)
def test_dims(dim):
    dt = on_device(random_tables(30, TILE + 1, dim, seed=30 + dim))
    check(dt, user_ids(17, 30, 5), 9, random_exclusions(17, TILE + 1, seed=dim))


@pytest.mark.parametrize("k", KS)
def test_k_at_the_boundaries_of_the_instantiations(k):
    dt = on_device(random_tables(30, TILE + 1, 64, seed=40 + k))
    check(dt, user_ids(17, 30, 6), k, random_exclusions(17, TILE + 1, seed=k))


@pytest.mark.parametrize("num_items", [1, 9, 17, 32])
def test_k_equal_to_num_items(num_items):
    dt = on_device(random_tables(30, num_items, 64, seed=50 + num_items))
    ids, _, _ = check(dt, user_ids(17, 30, 7), num_items)
    assert (np.sort(ids, axis=1) == np.arange(num_items)).all()


def test_splits_do_not_change_a_byte():
    num_items = 3 * TILE + 7                            # 4 item tiles
    dt = on_device(random_tables(80, num_items, 64, seed=60))
    users = user_ids(65, 80, 8)
    exc = random_exclusions(65, num_items, seed=61, per_row=40)
    for k in (10, 32):
        got = [check(dt, users, k, exc, splits=s)[:2] for s in (0, 1, 2, 4)]
        for ids, sc in got[1:]:
            assert ids.tobytes() == got[0][0].tobytes() and sc.tobytes() == got[0][1].tobytes()
    with pytest.raises(ValueError, match="splits"):
        fused(dt, users, 10, exc, splits=5)


def test_ties_rank_by_item_id():
    num_items, k = 2 * TILE + 5, 12
    # every score equal
    zeros = on_device([np.zeros(s, np.float32) for s in ((20, 8), (num_items, 8), (20,), (num_items,))])
    ids, sc, _ = check(zeros, np.arange(20), k, splits=2)
    assert (ids == np.arange(k)).all() and (sc == 0.5).all()
    # duplicated item rows tie for every user: the lower id first
    uw, iw, ub, ib = random_tables(20, num_items, 16, seed=70)
    for x, y in ((3, 40), (TILE - 1, TILE), (7, 2 * TILE + 4), (100, 101)):
        iw[y], ib[y] = iw[x], ib[x]
    ids, _, block = check(on_device((uw, iw, ub, ib)), np.arange(20), 32, splits=0)
    assert (block[:, 3] == block[:, 40]).all()
    for row in ids.tolist():
        for x, y in ((3, 40), (TILE - 1, TILE), (7, 2 * TILE + 4), (100, 101)):
            if y in row:
                assert x in row and row.index(x) + 1 == row.index(y)
    # the sigmoid saturates to exactly 1.0 for many items
    uw, iw, ub, ib = random_tables(20, num_items, 16, seed=71)
    ids, sc, block = check(on_device((40 * uw, 40 * iw, ub, ib)), np.arange(20), k, splits=3)
    ones = (block == 1.0).sum(axis=1)
    assert (ones > k).any()
    for r in np.flatnonzero(ones > k):
        assert (ids[r] == np.flatnonzero(block[r] == 1.0)[:k]).all() and (sc[r] == 1.0).all()


def test_a_nan_item_ranks_behind_every_finite_score():
    num_items, lo, hi = TILE + 9, 1, TILE + 2                           # two items with a NaN row
    uw, iw, ub, ib = random_tables(10, num_items, 8, seed=80)
    iw[lo] = iw[hi] = np.nan
    dt = on_device((uw, iw, ub, ib))
    users = np.arange(10)
    for s in (0, 1, 2):
        ids, _, block = check(dt, users, 10, splits=s)
        assert np.isnan(block[:, [lo, hi]]).all() and not np.isin(ids, [lo, hi]).any()
        # row 0 keeps three finite items: the -inf keys (excluded or NaN) follow them in id order, so
        # the NaN item 1 is returned between the excluded 0 and 2, its score NaN, theirs -inf
        keep = [5, 17, TILE + 1]
        exc = [sorted(set(range(num_items)) - set(keep) - {lo, hi})] + [[] for _ in users[1:]]
        ids, sc, _ = check(dt, users, 6, exc, splits=s)
        assert set(ids[0, :3]) == set(keep) and np.isfinite(sc[0, :3]).all()
        assert (ids[0, 3:] == [0, 1, 2]).all()
        assert np.isneginf(sc[0, 3]) and np.isnan(sc[0, 4]) and np.isneginf(sc[0, 5])
        assert not np.isin(ids[1:], [lo, hi]).any()


def test_exclusions():
    num_items, n, k = 3 * TILE + 7, 20, 10
    dt = on_device(random_tables(30, num_items, 32, seed=90))
    users = user_ids(n, 30, 9)
    last = num_items - 1
    rows = [[] for _ in range(n)]
    rows[0] = [TILE - 1, TILE, last]                                    # tile and split boundaries
    rows[1] = [0, 0, 5, 5, 5, TILE, TILE, last, last]                   # repeated ids
    rows[2] = [-7, -1, 3, TILE + 1, num_items, num_items + 5, 2 ** 31 - 1]      # ids outside the table are ignored
    rows[4] = list(range(num_items))                                    # every item excluded
    keep = [2 * TILE + 1, 4, TILE, 77, last, 300, 131, 9]               # k - 2 items stay
    rows[5] = sorted(set(range(num_items)) - set(keep))
    rows[6] = list(range(TILE))                                         # a whole tile
    rows[7] = list(range(TILE, num_items))                              # all but the first tile
    for s in (0, 1, 2, 4):
        ids, sc, block = check(dt, users, k, rows, splits=s)
        assert not np.isin(ids[0], rows[0]).any() and not np.isin(ids[1], rows[1]).any()
        assert not np.isin(ids[2], [3, TILE + 1]).any()
        assert (ids[3] == np.argsort(-block[3], kind="stable")[:k]).all()       # the empty row among full ones
        assert (ids[4] == np.arange(k)).all() and np.isneginf(sc[4]).all()
        assert set(ids[5, :8]) == set(keep) and (ids[5, 8:] == rows[5][:2]).all()
        assert np.isfinite(sc[5, :8]).all() and np.isneginf(sc[5, 8:]).all()
        assert (ids[6] >= TILE).all() and (ids[7] < TILE).all()
    check(dt, users, k, None, splits=2)                                 # none: null pointers
    check(dt, users, k, [[] for _ in range(n)], splits=2)               # none: an empty CSR


def test_the_tables_are_only_read():
    tabs = random_tables(30, 2 * TILE + 3, 64, seed=100)
    dt = on_device(tabs)
    users = user_ids(65, 30, 10)
    check(dt, users, 16, random_exclusions(65, 2 * TILE + 3, seed=101), splits=2)
    for t, h in zip(dt, tabs):
        assert t.cpu().numpy().tobytes() == h.tobytes()


def test_bad_arguments_raise_before_any_launch():
    dt = on_device(random_tables(30, TILE + 1, 16, seed=110))
    for bad in ([0, 30], [-1, 2]):                                       # refused in Python: never launched
        with pytest.raises(ValueError, match="user ids"):
            mf_engine.topk_users_fused(*dt, np.array(bad), 5)
    for k in (0, 33):
        with pytest.raises(ValueError, match="k must be"):
            mf_engine.topk_users_fused(*dt, np.arange(4), k)
    with pytest.raises(ValueError):
        mf_engine.topk_users_fused(*dt, np.arange(4), 5, exc_ptr=np.zeros(5, np.int64))
    with pytest.raises(ValueError, match="exc_ptr"):
        mf_engine.topk_users_fused(*dt, np.arange(4), 5, np.array([0, 2, 1, 3, 3]), np.array([1, 2, 3], np.int32))
    with pytest.raises(ValueError, match="exc_ptr"):
        mf_engine.topk_users_fused(*dt, np.arange(4), 5, np.array([0, 1, 2, 3, 9]), np.array([1, 2, 3], np.int32))
    ids, sc = mf_engine.topk_users_fused(*dt, np.zeros(0, np.int64), 5)
    assert ids.shape == sc.shape == (0, 5)
