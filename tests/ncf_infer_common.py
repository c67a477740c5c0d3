"""What the NCF / NeuMF inference and evaluation GPU tests share (no tests here): reference-style
random parameters, the model on the device behind the three C-ABI entry points, the float64
forward, a small ImplicitFactorizationModel, and the wrapper that hides a model's device ranking."""
import ctypes

import numpy as np
import torch

from oracle.ncf import layer_sizes
from recommendation_gans_amd import _lib

DEV = "cuda:0"
SENTINEL, PAD = -7.0, 8


def random_params(E, M, U, I, seed):
    """Reference-style init in named_parameters() order: N(0, 1) embeddings, Xavier-uniform weights,
    small random biases."""
    rs = np.random.RandomState(seed)
    f = np.float32
    p = [rs.randn(U, E).astype(f), rs.randn(I, E).astype(f)]
    if M:
        p += [rs.randn(U, M).astype(f), rs.randn(I, M).astype(f)]
    sizes = layer_sizes(E)
    shapes = [(o, i) for i, o in zip(sizes[:-1], sizes[1:])] + [(1, 8 + M)]
    for o, i in shapes:
        lim = np.sqrt(6.0 / (i + o))
        p += [rs.uniform(-lim, lim, (o, i)).astype(f), rs.uniform(-0.1, 0.1, o).astype(f)]
    return p


def forward64_pairs(params, M, users, items):
    """float64 eval-mode forward (mlp.py:30-41 / neuMF.py:34-55) of the pairs (users[p], items[p])."""
    p = [np.asarray(x, dtype=np.float64) for x in params]
    mlp = p[4:] if M else p[2:]
    x = np.concatenate([p[0][users], p[1][items]], -1)
    slope = float(np.float32(0.1))
    for k in range(0, len(mlp) - 2, 2):
        z = x @ mlp[k].T + mlp[k + 1]
        x = np.where(z > 0, z, z * slope)
    if M:
        x = np.concatenate([x, p[2][users] * p[3][items]], -1)
    z = (x @ mlp[-2].T + mlp[-1])[..., 0]
    return 1.0 / (1.0 + np.exp(-z))


def forward64(params, M, n_items=None):
    """The same forward of every (user, item) pair, items [0, n_items): a (U, I) block."""
    U, I = len(params[0]), len(params[1][:n_items])
    return forward64_pairs(params, M, np.repeat(np.arange(U), I), np.tile(np.arange(I), U)).reshape(U, I)


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

    def score(self, users, ld=None, sentinel=SENTINEL):
        """rg_ncf_score_users into a block of row stride ld filled with the sentinel beforehand."""
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

    def users(self, users):
        """rg_ncf_score_users: the users against every item."""
        return self.score(users)

    def pairs(self, users, items):
        """Scores of the pairs; the PAD sentinel entries after them must come back untouched."""
        n = len(users)
        u = torch.as_tensor(np.asarray(users, dtype=np.int64), device=DEV)
        i = torch.as_tensor(np.asarray(items, dtype=np.int64), device=DEV)
        out = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
        _lib.check(_lib.load().rg_ncf_score_pairs(_lib.stream_handle(), ctypes.byref(self.model), _lib.ptr(u),
                                                  _lib.ptr(i), n, _lib.ptr(out)), "rg_ncf_score_pairs")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[n:] == SENTINEL).all(), "entries past out[n) written"
        return got[:n]


def make_model(kind, tmp_path, monkeypatch, U, I, n_test, test_users=None, E=16, M=5):
    """An initialised ImplicitFactorizationModel ("mf", "ncf" or "neumf") with 600 train and n_test test
    interactions, the test users drawn below test_users (default U)."""
    from recommendation_gans_amd.implicit import ImplicitFactorizationModel
    from recommendation_gans_amd.spotlight.dnn_models.mlp import MLP
    from recommendation_gans_amd.spotlight.dnn_models.neuMF import NeuMF
    from recommendation_gans_amd.spotlight.factorization.representations import BilinearNet
    from recommendation_gans_amd.spotlight.interactions import Interactions
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(11)
    if kind == "mf":
        net = BilinearNet(U, I, E)
        with torch.no_grad():                  # spread the scores: the default init leaves them all near 0.5
            net.user_embeddings.weight.normal_()
            net.item_embeddings.weight.normal_()
            net.item_biases.weight.normal_()
    elif kind == "ncf":
        net = MLP(layers=layer_sizes(E), num_users=U, num_items=I, embedding_dim=E)
    else:
        net = NeuMF(layer_sizes(E), U, I, mf_embedding_dim=M, mlp_embedding_dim=E)
    rs = np.random.RandomState(4)
    train = Interactions(rs.randint(0, U, 600).astype(np.int32), rs.randint(0, I, 600).astype(np.int32),
                         ratings=np.ones(600, np.float32), num_users=U, num_items=I)
    test = Interactions(rs.randint(0, U if test_users is None else test_users, n_test).astype(np.int32),
                        rs.randint(0, I, n_test).astype(np.int32), ratings=np.ones(n_test, np.float32),
                        num_users=U, num_items=I)
    pool = list(zip(rs.randint(0, U, 500).tolist(), rs.randint(0, I, 500).tolist()))
    model = ImplicitFactorizationModel(loss="pointwise", embedding_dim=E, n_iter=1, batch_size=64, representation=net,
                                       random_state=np.random.RandomState(0), neg_examples=pool,
                                       num_negative_samples=3, use_cuda=True)
    model._initialize(train)
    return model, train, test


class HostOnly:
    """A model's score block without its device ranking: the metrics then take the host path."""

    def __init__(self, m):
        self.score_users = m.score_users
