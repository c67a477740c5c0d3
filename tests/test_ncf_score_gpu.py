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

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-7
TILE, GROUP = _lib.RG_NCF_SCORE_ITEM_TILE, _lib.RG_NCF_SCORE_USER_GROUP
DEV = "cuda:0"


def tower(E):
    sizes = [2 * E]
    while sizes[-1] > 8:
        sizes.append(sizes[-1] // 2)
    return sizes


def random_params(E, M, U, I, seed):
    """Reference-style init in named_parameters() order: N(0, 1) embeddings, Xavier-uniform weights,
    small random biases."""
    rs = np.random.RandomState(seed)
    f = np.float32
    p = [rs.randn(U, E).astype(f), rs.randn(I, E).astype(f)]
    if M:
        p += [rs.randn(U, M).astype(f), rs.randn(I, M).astype(f)]
    sizes = tower(E)
    shapes = [(o, i) for i, o in zip(sizes[:-1], sizes[1:])] + [(1, 8 + M)]
    for o, i in shapes:
        lim = np.sqrt(6.0 / (i + o))
        p += [rs.uniform(-lim, lim, (o, i)).astype(f), rs.uniform(-0.1, 0.1, o).astype(f)]
    return p


def forward64(params, M, n_items=None):
    """float64 eval-mode forward (mlp.py:30-41 / neuMF.py:34-55) of every (user, item) pair."""
    p = [np.asarray(x, dtype=np.float64) for x in params]
    uw, iw = p[0], p[1][:n_items]
    mlp = p[4:] if M else p[2:]
    U, I = len(uw), len(iw)
    x = np.concatenate([np.repeat(uw[:, None, :], I, 1), np.repeat(iw[None, :, :], U, 0)], -1)
    slope = float(np.float32(0.1))
    for k in range(0, len(mlp) - 2, 2):
        z = x @ mlp[k].T + mlp[k + 1]
        x = np.where(z > 0, z, z * slope)
    if M:
        x = np.concatenate([x, p[2][:, None, :] * p[3][:n_items][None, :, :]], -1)
    z = (x @ mlp[-2].T + mlp[-1])[..., 0]
    return 1.0 / (1.0 + np.exp(-z))


class Device:
    """The model's tensors on the device and its rg_ncf_model_t (moments null: the model is read-only)."""

    def __init__(self, params, E, M, n_items=None):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in params]
        self.uw, self.iw = t[0], t[1][:n_items].contiguous()
        self.mf = [t[2], t[3][:n_items].contiguous()] if M else [None, None]
        self.mlp = torch.cat([x.reshape(-1) for x in (t[4:] if M else t[2:])]).contiguous()
        self.U, self.I, self.E, self.M = self.uw.shape[0], self.iw.shape[0], E, M
        self.model = _lib.NCFModel(_lib.ptr(self.uw), _lib.ptr(self.iw), None, None, None, None, _lib.ptr(self.mlp),
                                   None, None, self.U, self.I, E, M)
        self.model.mf_user_w, self.model.mf_item_w = _lib.ptr(self.mf[0]), _lib.ptr(self.mf[1])

    def score(self, users, ld=None, sentinel=-7.0):
        lib = _lib.load()
        n, ld = len(users), self.I if ld is None else ld
        u = torch.as_tensor(np.asarray(users, dtype=np.int64), device=DEV)
        need = lib.rg_ncf_score_workspace_len(ctypes.byref(self.model), n)
        assert need == (self.I + n) * self.E + n * ((self.M + 3) // 4 * 4)
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=DEV)
        out = torch.full((n, ld), sentinel, dtype=torch.float32, device=DEV)
        _lib.check(lib.rg_ncf_score_users(_lib.stream_handle(), ctypes.byref(self.model), _lib.ptr(u), n, _lib.ptr(ws),
                                          _lib.ptr(out), ld), "rg_ncf_score_users")
        torch.cuda.synchronize()
        return out.cpu().numpy()


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
def make_model(kind, tmp_path, monkeypatch):
    from recommendation_gans_amd.implicit import ImplicitFactorizationModel
    from recommendation_gans_amd.spotlight.dnn_models.mlp import MLP
    from recommendation_gans_amd.spotlight.dnn_models.neuMF import NeuMF
    from recommendation_gans_amd.spotlight.interactions import Interactions
    monkeypatch.chdir(tmp_path)
    U, I, E, M = 75, 3 * TILE + 7, 16, 5
    torch.manual_seed(11)
    if kind == "ncf":
        net = MLP(layers=tower(E), num_users=U, num_items=I, embedding_dim=E)
    else:
        net = NeuMF(tower(E), U, I, mf_embedding_dim=M, mlp_embedding_dim=E)
    rs = np.random.RandomState(4)
    train = Interactions(rs.randint(0, U, 600).astype(np.int32), rs.randint(0, I, 600).astype(np.int32),
                         ratings=np.ones(600, np.float32), num_users=U, num_items=I)
    test = Interactions(rs.randint(0, U, 300).astype(np.int32), rs.randint(0, I, 300).astype(np.int32),
                        ratings=np.ones(300, np.float32), num_users=U, num_items=I)
    pool = list(zip(rs.randint(0, U, 500).tolist(), rs.randint(0, I, 500).tolist()))
    model = ImplicitFactorizationModel(loss="pointwise", embedding_dim=E, n_iter=1, batch_size=64, representation=net,
                                       random_state=np.random.RandomState(0), neg_examples=pool,
                                       num_negative_samples=3, use_cuda=True)
    model._initialize(train)
    return model, train, test


class _HostOnly:
    def __init__(self, m):
        self.score_users = m.score_users


@pytest.mark.parametrize("kind", ["ncf", "neumf"])
def test_model_paths_use_the_kernel(kind, tmp_path, monkeypatch):
    from recommendation_gans_amd.spotlight import evaluation
    model, train, test = make_model(kind, tmp_path, monkeypatch)
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
    h = _HostOnly(model)
    for k in (1, 5):
        assert evaluation.precision_recall_score(model, test, k=k) == evaluation.precision_recall_score(h, test, k=k)
        assert evaluation.precision_recall_score(model, test, train, k=k) == \
            evaluation.precision_recall_score(h, test, train, k=k)
        assert evaluation.map_at_k(model, test, k=k) == evaluation.map_at_k(h, test, k=k)
