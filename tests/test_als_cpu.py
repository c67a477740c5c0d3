"""Implicit ALS without a GPU: the numpy restatement (tests/als_common.py) in float64 solves the
explicitly formed systems, ``als.solve_rows_torch`` in float64 agrees with it on every case, every
case is admitted by the conditioning rule, the closed-form objective equals a brute-force dense
evaluation, and the Python entry points and the C entries refuse bad arguments before any launch."""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib, als
from tests import als_common as ac

t = torch.from_numpy


@pytest.mark.parametrize("dim", [1, 3, 8])
def test_the_restatement_with_dim_steps_from_zero_solves_the_explicit_system(dim):
    case = ac.make_case(dim, 130, 1.0, 40.0, True, "zero")
    x, _ = ac.numpy_als_rows(case, dim)
    worst = 0.0
    for u in range(case["rows"]):
        if case["ptr"][u + 1] == case["ptr"][u]:
            assert not x[u].any()
            continue
        A, b = ac.explicit_system(case, u)
        worst = max(worst, float(np.abs(np.linalg.solve(A, b) - x[u]).max()))
    print(f"dim {dim}: largest deviation from np.linalg.solve {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("i", range(len(ac.CASES)), ids=ac.CASE_IDS)
def test_solve_rows_torch_in_float64_equals_the_restatement_and_the_case_is_admitted(i):
    d = ac.case_data(i)
    case, f8 = d["case"], np.float64
    x = t(case["X0"].astype(f8))
    got, loss = als.solve_rows_torch(t(case["Y"].astype(f8)), t(case["G"].astype(f8)), t(case["ptr"]), t(case["idx"]),
                                     None if case["val"] is None else t(case["val"].astype(f8)), case["alpha"], d["cg"],
                                     x, return_loss=True, checked=True)
    assert got is x
    np.testing.assert_allclose(got.numpy(), d["r64"][0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(loss.numpy(), d["r64"][1], rtol=1e-12, atol=1e-12)
    empty = np.diff(case["ptr"]) == 0
    assert not got.numpy()[empty].any() and not loss.numpy()[empty].any()          # exactly zero
    print(f"case {ac.CASE_IDS[i]}: E32 {d['e32']:.3e} E32(loss) {d['e32_loss']:.3e} max|x| {d['xmax']:.2f}")
    assert d["admitted"] and d["e32"] > 0


def test_solve_rows_torch_takes_rows_and_blocks_and_zero_steps():
    case = ac.make_case(8, 130, 0.1, 1.0, True, "random")
    f8 = np.float64
    args = (t(case["Y"].astype(f8)), t(case["G"].astype(f8)), t(case["ptr"]), t(case["idx"]), t(case["val"].astype(f8)),
            1.0, 3)
    full = als.solve_rows_torch(*args, t(case["X0"].astype(f8))).numpy()
    rows = np.argsort(np.diff(case["ptr"]), kind="stable")[::2].copy()
    part = als.solve_rows_torch(*args, t(case["X0"].astype(f8)), rows=t(rows), block_elems=2000).numpy()
    np.testing.assert_allclose(part[rows], full[rows], rtol=0, atol=1e-13)
    rest = np.setdiff1d(np.arange(130), rows)
    assert (part[rest] == case["X0"][rest].astype(f8)).all()
    zero = als.solve_rows_torch(*args[:6], 0, t(case["X0"].astype(f8))).numpy()
    empty = np.diff(case["ptr"]) == 0
    assert (zero[~empty] == case["X0"][~empty].astype(f8)).all() and not zero[empty].any()


def test_the_closed_form_objective_equals_the_dense_brute_force():
    rs = np.random.RandomState(3)
    U, I, d, alpha, lam = 30, 20, 5, 40.0, 0.1
    X, Y = rs.randn(U, d) * 0.3, rs.randn(I, d) * 0.3
    dense = (rs.rand(U, I) < 0.2)
    dense[4] = False                                     # a user without interactions, and a non-zero row
    users, items = np.nonzero(dense)
    vals = rs.rand(len(users)) * 2
    ptr, idx, val = als.interactions_csr(users, items, vals, U)
    # brute force over the dense block: c (p - x.y)^2 with p = 1 on the listed cells, c = 1 elsewhere
    C, P = np.ones((U, I)), dense.astype(np.float64)
    C[users, items] = 1.0 + alpha * vals.astype(np.float32).astype(np.float64)
    want = float((C * (P - X @ Y.T) ** 2).sum() + lam * ((X * X).sum() + (Y * Y).sum()))
    got = als.objective_torch(t(X), t(Y), (t(ptr), t(idx), t(val.astype(np.float64))), alpha, lam)
    assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(ac.objective64(X, Y, (ptr, idx, val), alpha, lam) - want) <= 1e-12 * abs(want)


def test_interactions_csr_keeps_order_and_duplicates_and_the_transpose_agrees():
    users, items, w = [2, 0, 2, 2, 0], [5, 1, 3, 5, 1], [1.0, 2.0, 3.0, 4.0, 5.0]
    ptr, idx, val = als.interactions_csr(users, items, w, 4)
    assert ptr.tolist() == [0, 2, 2, 5, 5] and idx.tolist() == [1, 1, 5, 3, 5] and val.tolist() == [2.0, 5.0, 1.0, 3.0, 4.0]
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == np.float32
    tp, ti, tv = als.interactions_csr(items, users, w, 6)
    ap, ai, av = ac.transpose_csr(ptr, idx, val, 6)
    assert (tp == ap).all() and sorted(zip(ti.tolist(), tv.tolist())) == sorted(zip(ai.tolist(), av.tolist()))
    assert als.interactions_csr(users, items, None, 4)[2] is None


# ---------------------------------------------------------------- refusals, before any launch
def _args(**over):
    case = ac.make_case(8, 3, 0.1, 1.0, True, "random", lens=[2, 0, 3])
    a = dict(other=t(case["Y"]), G=t(case["G"]), ptr_=case["ptr"].copy(), idx=case["idx"].copy(), val=case["val"].copy(),
             alpha=1.0, cg_steps=3, x=t(case["X0"].copy()))
    a.update(over)
    return a


@pytest.mark.parametrize("over, match", [
    (dict(other=torch.zeros(ac.NUM_ITEMS, 8, dtype=torch.float64)), "float32"),
    (dict(other=torch.zeros(ac.NUM_ITEMS, 129), G=torch.zeros(129, 129), x=torch.zeros(3, 129)), "dim must be in"),
    (dict(G=torch.zeros(8, 7)), r"G must be \(dim, dim\)"),
    (dict(x=torch.zeros(3, 7)), "x \\(n_rows, dim\\)"),
    (dict(alpha=-1.0), "alpha"),
    (dict(alpha=float("nan")), "alpha"),
    (dict(cg_steps=-1), "cg_steps must be in"),
    (dict(cg_steps=65), "cg_steps must be in"),
    (dict(idx=np.zeros(5, np.float32)), "int32 or int64"),
    (dict(ptr_=np.array([0, 2, 5])), "one entry per row"),
    (dict(val=np.zeros(4, np.float32)), "one floating-point value per entry"),
    (dict(rows=np.zeros(2, np.float32)), "rows must be int32 or int64"),
    (dict(checked=True, ptr_=np.array([0, 3, 2, 5])), "ascend"),
    (dict(checked=True, ptr_=np.array([0, 2, 2, 4])), "ascend"),
    (dict(checked=True, idx=np.array([0, 1, ac.NUM_ITEMS, 3, 4])), "outside"),
    (dict(checked=True, idx=np.array([0, 1, -1, 3, 4])), "outside"),
    (dict(checked=True, val=np.array([1, 1, -0.5, 1, 1], np.float32)), "finite and >= 0"),
    (dict(checked=True, rows=np.array([0, 3])), "row id outside"),
    (dict(checked=True, rows=np.array([1, 1])), "twice"),
    (dict(), "CUDA"),                         # host tensors: refused, never a torch fall-back
    (dict(checked=True), "CUDA"),
])
def test_solve_rows_refuses_before_any_gpu_call(over, match, monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(als._lib, "load", no_gpu)
    with pytest.raises(ValueError, match=match):
        als.solve_rows(**_args(**over))


def test_gram_and_objective_refuse_host_tensors_and_bad_lam(monkeypatch):
    monkeypatch.setattr(als._lib, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("loaded")))
    tab = torch.zeros(10, 8)
    for lam in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lam"):
            als.gram(tab, lam)
    with pytest.raises(ValueError, match="CUDA"):
        als.gram(tab, 0.1)
    with pytest.raises(ValueError, match="CUDA"):
        als.objective(tab, tab, (np.zeros(11, np.int64), np.zeros(0, np.int32), None), 1.0, 0.1)
    for kw in (dict(iterations=0), dict(lam=0.0), dict(lam=-1.0)):
        a = dict(iterations=1, lam=0.1, alpha=1.0, cg_steps=3)
        a.update(kw)
        with pytest.raises(ValueError):
            als.als_sweeps(tab, tab, (None, None, None), (None, None, None), **a)


def _stub(kind="mf", dim=16, world=1, initialized=True):
    """An ImplicitFactorizationModel that holds only what the refusals read (no device)."""
    from recommendation_gans_amd.implicit import ImplicitFactorizationModel
    m = ImplicitFactorizationModel.__new__(ImplicitFactorizationModel)
    m._world, m._kind, m._embedding_dim, m._representation = world, kind, dim, None
    m._net = object() if initialized else None
    m._num_users, m._num_items, m._als, m._use_cuda = 6, 20, None, False
    return m


@pytest.mark.parametrize("kw", [dict(regularization=0.0), dict(regularization=-1.0), dict(regularization=float("nan")),
                                dict(alpha=-1.0), dict(iterations=0), dict(cg_steps=0), dict(cg_steps=65)])
def test_fit_als_refuses_bad_arguments(kw):
    with pytest.raises(ValueError):
        _stub().fit_als(None, **kw)


def test_fit_als_refuses_what_it_does_not_implement():
    with pytest.raises(ValueError, match="embedding_dim"):
        _stub(dim=129).fit_als(None)
    with pytest.raises(ValueError, match="embedding_dim"):
        _stub(dim=129, initialized=False).fit_als(None)
    for kind in ("ncf",):
        with pytest.raises(NotImplementedError):
            _stub(kind=kind).fit_als(None)
    with pytest.raises(NotImplementedError):
        _stub(world=2).fit_als(None)
    with pytest.raises(RuntimeError, match="GPU only"):             # a fresh model without use_cuda: as fit
        from recommendation_gans_amd.spotlight.interactions import Interactions
        _stub(initialized=False).fit_als(Interactions(np.zeros(1, np.int32), np.zeros(1, np.int32), num_users=6,
                                                      num_items=20))


def test_fold_in_users_als_and_recommend_for_histories_refuse_bad_arguments():
    with pytest.raises(RuntimeError, match="fitted"):
        _stub(initialized=False).fold_in_users_als([[1]])
    with pytest.raises(NotImplementedError):
        _stub(kind="ncf").fold_in_users_als([[1]])
    m = _stub()
    for kw in (dict(regularization=0.0), dict(regularization=-1.0), dict(alpha=-0.5), dict(cg_steps=0), dict(cg_steps=65)):
        with pytest.raises(ValueError):
            m.fold_in_users_als([[1, 2]], **kw)
    with pytest.raises(ValueError, match="embedding_dim"):
        _stub(dim=129).fold_in_users_als([[1]])
    with pytest.raises(ValueError, match="outside"):
        m.fold_in_users_als([[1, 20]])
    with pytest.raises(ValueError, match="method"):
        m.recommend_for_histories([[1]], 5, method="sgd")
    with pytest.raises(TypeError):                                   # each method has its own keywords
        m.recommend_for_histories([[1]], 5, method="als", steps=3)
    with pytest.raises(TypeError):
        m.recommend_for_histories([[1]], 5, method="adam", cg_steps=3)
    with pytest.raises(TypeError):
        m.recommend_for_histories([[1]], 5, cg_steps=3)
    with pytest.raises(ValueError):
        m.recommend_for_histories([[1]], 33, method="als")
    with pytest.raises(ValueError):
        m.recommend_for_histories([[1]], 5, method="als", cg_steps=0)


# ---------------------------------------------------------------- the entries, without a GPU
def test_signatures_are_bound_and_the_threshold_is_exported():
    sig = {n: a for n, _, a in _lib.SIGNATURES}
    assert len(sig["rg_als_solve_rows"]) == 13 and len(sig["rg_als_gram"]) == 7
    L = _lib.load()
    assert L.rg_als_long_row_len() == ac.T == als.long_row_len()
    assert L.rg_als_gram_workspace_len(1, 1) == 1 and L.rg_als_gram_workspace_len(0, 8) == 64
    assert L.rg_als_gram_workspace_len(1024, 128) == 128 * 128 and L.rg_als_gram_workspace_len(1025, 128) == 2 * 128 * 128
    for n, d in ((-1, 8), (10, 0), (10, 129)):
        assert L.rg_als_gram_workspace_len(n, d) == -1 and b"rg_als_gram_workspace_len" in L.rg_last_error()


def test_entries_refuse_before_any_hip_call():
    L = _lib.load()
    p = 64              # never dereferenced: every call below is refused (or has nothing to do) first

    def refused(rc, reason):
        assert rc == -1 and reason in L.rg_last_error(), (rc, L.rg_last_error())
    # stream, other, G, dim, ptr, idx, val, alpha, rows, n_rows, cg_steps, x, loss
    good = [None, p, p, 16, p, p, p, 1.0, p, 4, 3, p, p]
    for at in (1, 2, 4, 11):
        a = list(good)
        a[at] = None
        refused(L.rg_als_solve_rows(*a), b"null pointer")
    for dim in (0, 129, -1):
        a = list(good)
        a[3] = dim
        refused(L.rg_als_solve_rows(*a), b"dim must be in [1, 128]")
    for cg in (-1, 65):
        a = list(good)
        a[10] = cg
        refused(L.rg_als_solve_rows(*a), b"cg_steps must be in [0, 64]")
    for alpha in (-0.5, float("nan"), float("inf")):
        a = list(good)
        a[7] = alpha
        refused(L.rg_als_solve_rows(*a), b"alpha")
    a = list(good)
    a[9] = -1
    refused(L.rg_als_solve_rows(*a), b"n_rows < 0")
    a = list(good)
    a[5] = None
    refused(L.rg_als_solve_rows(*a), b"row_idx is null")
    for opt in (5, 6, 8, 12):                     # nothing to do at n_rows == 0, whatever is null
        a = list(good)
        a[9], a[opt] = 0, None
        assert L.rg_als_solve_rows(*a) == _lib.RG_OK
    # stream, table, n_rows, dim, lam, workspace, out
    good = [None, p, 10, 16, 0.1, p, p]
    for at in (1, 5, 6):
        a = list(good)
        a[at] = None
        refused(L.rg_als_gram(*a), b"null pointer")
    for dim in (0, 129):
        a = list(good)
        a[3] = dim
        refused(L.rg_als_gram(*a), b"dim must be in [1, 128]")
    a = list(good)
    a[2] = -1
    refused(L.rg_als_gram(*a), b"n_rows < 0")
    for lam in (-0.1, float("nan"), float("inf")):
        a = list(good)
        a[4] = lam
        refused(L.rg_als_gram(*a), b"lam")
