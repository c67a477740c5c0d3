"""NCF / NeuMF scores of arbitrary (user, item) pairs on the GPU (rg_ncf_score_pairs through the C-ABI).

* Against the reference's own eval-mode scores (tests/golden/ncf_scores_*.npz: its parameters and
  its 9 x 97 scores), all 873 pairs in a shuffled order with repeats, at rtol=1e-5, atol=1e-7 -- the
  project's tolerance for these fixtures.
* Against a float64 restatement of the forward on reference-style random parameters, the same
  tolerance, at every supported width and at pair counts around the kernel's tile; ids unsorted with
  repeats and always holding the last user and the last item; the 8 entries after out[n) stay
  untouched.
* Position independence: equal pairs give equal bits in a batch, in a permutation of it, alone, on a
  second call, and in a batch of more tiles than workgroups are launched (each workgroup then walks
  several tiles).
* Agreement with the all-item kernel (rg_ncf_score_users) on the same pairs.
* Every refusal returns non-zero and launches nothing; n == 0 is RG_OK.
* Through ImplicitFactorizationModel (MLP and NeuMF): predict(users, items) is NCFEngine.scores,
  within tolerance of NCFEngine.scores_torch; a scalar user broadcasts; an id past the table raises.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib
from tests.ncf_infer_common import DEV, PAD, SENTINEL, Device, make_model, random_params
from tests.ncf_infer_common import forward64_pairs as forward64

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-7
T = _lib.RG_NCF_SCORE_PAIR_TILE


def pair_ids(n, U, I, seed):
    """n pairs, unsorted, with repeats when n > 2, always holding user U - 1 and item I - 1."""
    rs = np.random.RandomState(seed)
    u, i = rs.randint(0, U, n), rs.randint(0, I, n)
    k = rs.randint(0, max(n - 1, 1))
    u[k], i[k] = U - 1, I - 1
    if n > 2:
        u[-1], i[-1] = u[0], i[0]
    return u, i


GOLDEN_CASES = ["mlp_e64", "mlp_e16", "neumf_e16_m50", "neumf_e8_m5"]


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_matches_reference_scores(golden_dir, case):
    z = np.load(os.path.join(golden_dir, f"ncf_scores_{case}.npz"))
    E, M = int(z["dim"]), int(z["mf_dim"])
    params = [z[f"p{k}"] for k in range(len(z["names"]))]
    ref = z["scores"]
    U, I = ref.shape
    assert (U, I) == (9, 97)
    rs = np.random.RandomState(7)
    order = np.concatenate([rs.permutation(U * I), rs.randint(0, U * I, 40)])     # every pair, shuffled, 40 repeated
    u, i = order // I, order % I
    got = Device(params, E, M).pairs(u, i)
    print(case, "max rel diff", float(np.max(np.abs(got - ref[u, i]) / np.abs(ref[u, i]))))
    np.testing.assert_allclose(got, ref[u, i], rtol=RTOL, atol=ATOL)


CONFIGS = [(8, 0), (16, 0), (32, 0), (64, 0), (8, 5), (16, 50), (32, 1), (64, 128)]
PAIR_COUNTS = [1, T - 1, T, T + 1, 3 * T + 7]


@pytest.mark.parametrize("E,M", CONFIGS)
def test_matches_float64_at_edge_counts(E, M):
    U, I = 75, 203
    params = random_params(E, M, U, I, seed=E * 1000 + M)
    dev = Device(params, E, M)
    worst = 0.0
    for n in PAIR_COUNTS:
        u, i = pair_ids(n, U, I, seed=n)
        assert (U - 1) in u and (I - 1) in i
        ref = forward64(params, M, u, i)
        got = dev.pairs(u, i)
        worst = max(worst, float(np.max(np.abs(got - ref) / np.abs(ref))))
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=f"n={n}")
    print(f"E={E} M={M} max rel diff {worst:.3g}")


@pytest.mark.parametrize("E,M", [(64, 0), (16, 50)])
def test_scores_do_not_depend_on_position(E, M):
    U, I, n = 75, 203, 3 * T + 7
    dev = Device(random_params(E, M, U, I, seed=5), E, M)
    u, i = pair_ids(n, U, I, seed=1)
    a = dev.pairs(u, i)
    assert a.tobytes() == dev.pairs(u, i).tobytes()                   # a second call
    perm = np.random.RandomState(2).permutation(n)
    assert dev.pairs(u[perm], i[perm]).tobytes() == a[perm].tobytes()  # a permutation
    assert dev.pairs(u[:1], i[:1]).tobytes() == a[:1].tobytes()        # the first pair alone
    first = {}                                                        # repeats within the batch
    for p in range(n):
        assert first.setdefault((u[p], i[p]), a[p].tobytes()) == a[p].tobytes()
    assert len(first) < n


@pytest.mark.parametrize("E,M", [(64, 0), (16, 50)])
def test_more_tiles_than_workgroups(E, M):
    """300,001 pairs are more tiles than a launch has workgroups, so each workgroup walks several;
    the batch repeats 1,000 pairs, and every repeat has the bits of the small batch, itself checked
    against float64."""
    U, I, base, n = 75, 203, 1000, 300001
    params = random_params(E, M, U, I, seed=9)
    dev = Device(params, E, M)
    u, i = pair_ids(base, U, I, seed=3)
    small = dev.pairs(u, i)
    np.testing.assert_allclose(small, forward64(params, M, u, i), rtol=RTOL, atol=ATOL)
    idx = np.arange(n) % base
    big = dev.pairs(u[idx], i[idx])
    assert big.tobytes() == small[idx].tobytes()


@pytest.mark.parametrize("E,M", [(64, 0), (16, 50), (8, 5)])
def test_agrees_with_the_all_item_kernel(E, M):
    U, I = 75, 203
    dev = Device(random_params(E, M, U, I, seed=6), E, M)
    users = np.array([74, 0, 33, 0])
    block = dev.users(users)
    got = dev.pairs(np.repeat(users, I), np.tile(np.arange(I), len(users))).reshape(len(users), I)
    print(f"E={E} M={M} max rel diff {float(np.max(np.abs(got - block) / np.abs(block))):.3g}")
    np.testing.assert_allclose(got, block, rtol=RTOL, atol=ATOL)


def test_bad_arguments_fail_loudly():
    lib = _lib.load()
    U, I, E, M, n = 12, 40, 16, 5, 4
    dev = Device(random_params(E, M, U, I, seed=2), E, M)
    u, i = torch.arange(n, device=DEV), torch.arange(n, device=DEV) + 3
    out = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    s, ref = _lib.stream_handle(), ctypes.byref

    def call(model=dev.model, users=u, items=i, n=n, o=out):
        return lib.rg_ncf_score_pairs(s, ref(model) if model is not None else None, _lib.ptr(users), _lib.ptr(items), n,
                                      _lib.ptr(o))

    def variant(**kw):
        m = _lib.NCFModel.from_buffer_copy(dev.model)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert call(model=None) != 0 and b"null" in lib.rg_last_error()
    assert call(model=variant(user_w=None)) != 0 and call(model=variant(item_w=None)) != 0
    assert call(model=variant(mlp=None)) != 0 and b"null" in lib.rg_last_error()
    assert call(users=None) != 0 and call(items=None) != 0 and call(o=None) != 0
    assert call(model=variant(mf_user_w=None)) != 0 and b"GMF" in lib.rg_last_error()
    assert call(model=variant(mf_item_w=None)) != 0 and b"GMF" in lib.rg_last_error()
    assert call(model=variant(dim=48)) != 0 and b"dim" in lib.rg_last_error()
    assert call(model=variant(mf_dim=129)) != 0 and b"mf_dim" in lib.rg_last_error()
    assert call(model=variant(mf_dim=-1)) != 0 and b"mf_dim" in lib.rg_last_error()
    assert call(n=-1) != 0 and b"n < 0" in lib.rg_last_error()
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()          # nothing was launched by any of the calls above
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out[:n] == SENTINEL).any() and (out[n:] == SENTINEL).all()


# ---------------------------------------------------------------- through the model
@pytest.mark.parametrize("kind", ["ncf", "neumf"])
def test_predict_takes_the_kernel(kind, tmp_path, monkeypatch):
    model, _, _ = make_model(kind, tmp_path, monkeypatch, U=75, I=199, n_test=300)
    e, U, I = model._engine, model._num_users, model._num_items
    rs = np.random.RandomState(8)
    users, items = rs.randint(0, U, 300), rs.randint(0, I, 300)
    users[0], items[0], users[-1], items[-1] = U - 1, I - 1, users[1], items[1]
    got = model.predict(users, items)
    assert got.shape == (300,) and got.dtype == np.float32
    np.testing.assert_array_equal(got, e.scores(torch.from_numpy(users), torch.from_numpy(items)).cpu().numpy())
    np.testing.assert_allclose(got, e.scores_torch(torch.from_numpy(users), torch.from_numpy(items)).cpu().numpy(),
                               rtol=RTOL, atol=ATOL)
    assert got[-1].tobytes() == got[1].tobytes()
    # a scalar user broadcasts over the items
    sub = np.array([5, 1, I - 1, 64])
    np.testing.assert_array_equal(model.predict(3, sub), model.predict(np.full(4, 3), sub))
    np.testing.assert_allclose(model.predict(3, sub), model.predict(3)[sub], rtol=RTOL, atol=ATOL)
    assert e.scores(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError):
        model.predict(np.array([0, 1]), np.array([0, I]))
    with pytest.raises(ValueError):
        e.scores(torch.tensor([0, 1]), torch.tensor([0, I]))
    with pytest.raises(ValueError):
        e.scores(torch.tensor([U, 1]), torch.tensor([0, 0]))
