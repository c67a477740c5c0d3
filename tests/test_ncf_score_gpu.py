"""NCF / NeuMF all-item scoring on the GPU (rg_ncf_score_users through the C-ABI).

* Against the reference's own eval-mode scores (tests/golden/ncf_scores_*.npz, made by
  tests/golden/make_ncf_scores_golden.py importing the reference's MLP / NeuMF) at
  rtol=1e-5, atol=1e-7 -- the tolerance of the predict(3) golden checks.  An fp32 evaluation
  with the split first layer differs from float64 by at most ~6e-7 relative at reference-style
  init (N(0, 1) embeddings, Xavier weights) over E in {8, 16, 32, 64}, M in {0, 5, 50, 128}.
* Against a float64 restatement of the forward on random parameters, the same tolerance, at
  the shapes where the kernel can go wrong: item counts around its tile, user counts around its
  group, unsorted user ids with a duplicate, a padded row stride whose padding stays untouched.
* Bit-identical repeat calls, loud failures on bad arguments, n_users = 0.
* Through ImplicitFactorizationModel (MLP and NeuMF): score_users / predict(3) equal the pairwise
  NCFEngine.scores path; topk_users equals the stable argsort of the model's own block; the
  metrics equal the host-only path's.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib
from tests.ncf_infer_common import DEV, Device, HostOnly, forward64, make_model, random_params

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-7
TILE, GROUP = _lib.RG_NCF_SCORE_ITEM_TILE, _lib.RG_NCF_SCORE_USER_GROUP


GOLDEN_CASES = ["mlp_e64", "mlp_e16", "neumf_e16_m50", "neumf_e8_m5"]


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_matches_reference_scores(golden_dir, case):
    z = np.load(os.path.join(golden_dir, f"ncf_scores_{case}.npz"))
    E, M = int(z["dim"]), int(z["mf_dim"])
    params = [z[f"p{k}"] for k in range(len(z["names"]))]
    ref = z["scores"]
    U, I = ref.shape
    assert (U, I) == (9, 97)
    got = Device(params, E, M).score(np.arange(U))
    print(case, "max rel diff", float(np.max(np.abs(got - ref) / np.abs(ref))))
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)


CONFIGS = [(8, 0), (16, 0), (32, 0), (64, 0), (8, 5), (16, 50), (32, 1), (64, 128)]
ITEM_COUNTS = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7]
USER_COUNTS = [1, GROUP - 1, GROUP + 1]


def user_ids(n, U, seed):
    """n ids out of U, unsorted, with a duplicate when n > 1."""
    u = np.random.RandomState(seed).randint(0, U, n)
    if n > 1:
        u[-1] = u[0]
    return u


@pytest.mark.parametrize("E,M", CONFIGS)
def test_matches_float64_at_edge_shapes(E, M):
    U, Imax = GROUP + 9, max(ITEM_COUNTS)
    params = random_params(E, M, U, Imax, seed=E * 1000 + M)
    worst = 0.0
    for I in ITEM_COUNTS:
        ref = forward64(params, M, n_items=I)             # (U, I), once per item count
        dev = Device(params, E, M, n_items=I)
        for n in USER_COUNTS:
            u = user_ids(n, U, seed=I + n)
            got = dev.score(u, ld=I + 5)
            assert (got[:, I:] == -7.0).all(), (I, n, "padding columns written")
            worst = max(worst, float(np.max(np.abs(got[:, :I] - ref[u]) / np.abs(ref[u]))))
            np.testing.assert_allclose(got[:, :I], ref[u], rtol=RTOL, atol=ATOL, err_msg=f"I={I} n={n}")
    print(f"E={E} M={M} max rel diff {worst:.3g}")


@pytest.mark.parametrize("E,M", [(64, 0), (16, 50)])
def test_repeat_calls_are_bit_identical(E, M):
    U, I = GROUP + 9, 3 * TILE + 7
    dev = Device(random_params(E, M, U, I, seed=5), E, M)
    u = user_ids(GROUP + 1, U, seed=1)
    a, b = dev.score(u), dev.score(u)
    assert a.tobytes() == b.tobytes()


def test_bad_arguments_fail_loudly():
    lib = _lib.load()
    U, I, E, M = 12, 40, 16, 5
    dev = Device(random_params(E, M, U, I, seed=2), E, M)
    u = torch.arange(4, device=DEV)
    ws = torch.empty(lib.rg_ncf_score_workspace_len(ctypes.byref(dev.model), 4), dtype=torch.float32, device=DEV)
    out = torch.full((4, I), -7.0, dtype=torch.float32, device=DEV)
    s, ref = _lib.stream_handle(), ctypes.byref

    def call(model=dev.model, users=u, n=4, w=ws, o=out, ld=I):
        return lib.rg_ncf_score_users(s, ref(model) if model is not None else None, _lib.ptr(users), n, _lib.ptr(w),
                                      _lib.ptr(o), ld)

    def variant(**kw):
        m = _lib.NCFModel.from_buffer_copy(dev.model)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert call(model=None) != 0 and b"null" in lib.rg_last_error()
    assert call(users=None) != 0 and call(w=None) != 0 and call(o=None) != 0
    assert call(model=variant(mlp=None)) != 0 and call(model=variant(mf_item_w=None)) != 0
    assert call(ld=I - 1) != 0 and b"ld" in lib.rg_last_error()
    assert call(model=variant(dim=48)) != 0 and b"dim" in lib.rg_last_error()
    assert call(model=variant(mf_dim=129)) != 0 and call(model=variant(mf_dim=-1)) != 0
    assert call(n=-1) != 0
    assert lib.rg_ncf_score_workspace_len(ref(variant(dim=48)), 4) < 0
    assert lib.rg_ncf_score_workspace_len(ref(dev.model), -1) < 0
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()              # nothing was launched by any of the calls above
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out == -7.0).any()


# ---------------------------------------------------------------- through the model
@pytest.mark.parametrize("kind", ["ncf", "neumf"])
def test_model_paths_use_the_kernel(kind, tmp_path, monkeypatch):
    from recommendation_gans_amd.spotlight import evaluation
    model, train, test = make_model(kind, tmp_path, monkeypatch, U=75, I=3 * TILE + 7, n_test=300)
    e, U, I = model._engine, model._num_users, model._num_items
    assert e.neumf == (kind == "neumf")
    users = np.array([7, 3, 70, 3, 0, 74, 12])
    block = model.score_users(users)
    assert block.shape == (len(users), I) and block.dtype == np.float32
    ut = torch.as_tensor(users, device=e.device)
    pair = e.scores(ut.repeat_interleave(I), torch.arange(I, device=e.device).repeat(len(users)))
    np.testing.assert_allclose(block, pair.reshape(len(users), I).cpu().numpy(), rtol=RTOL, atol=ATOL)
    p3 = model.predict(3)
    assert p3.shape == (I,)
    np.testing.assert_allclose(p3, e.scores(torch.full((I,), 3), torch.arange(I)).cpu().numpy(), rtol=RTOL, atol=ATOL)
    assert p3.tobytes() == block[1].tobytes()          # one user or a block: the same bits
    # explicit item_ids keep the pair path
    items = np.array([5, 1, 190, 64])
    np.testing.assert_array_equal(model.predict(np.array([3, 3, 7, 0]), items),
                                  e.scores(torch.tensor([3, 3, 7, 0]), torch.from_numpy(items)).cpu().numpy())
    with pytest.raises(ValueError):
        e.score_users(np.array([0, U]))
    # ranking: the stable argsort of the model's own block, excluded items last
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
