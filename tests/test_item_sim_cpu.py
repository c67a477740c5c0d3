"""The item-similarity entry points (rg_row_rnorms, rg_item_sim_workspace_len, rg_item_sim_topk)
and the layers above them without a GPU: the header declares them, the ctypes table binds them, the
source is built, every documented refusal comes back as a non-zero status that names its reason
before any HIP call is made (the pointers here are made-up addresses: a call that got past the
checks with rows or queries > 0 would launch on them), the workspace length is the documented
8 * n_queries * k * splits bytes, and similar_rows / similar_items refuse what they cannot take."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS, LEN, NAME = "rg_row_rnorms", "rg_item_sim_workspace_len", "rg_item_sim_topk"
P = 4096        # a made-up, 16-byte aligned, non-null address
INT_MAX = 2 ** 31 - 1


def test_header_declares_the_three_functions():
    txt = open(os.path.join(ROOT, "include", "rg_hip.h")).read()
    assert re.search(r"^\s*int\s+" + NORMS + r"\s*\(", txt, flags=re.M)
    assert re.search(r"^\s*int64_t\s+" + LEN + r"\s*\(", txt, flags=re.M)
    assert re.search(r"^\s*int\s+" + NAME + r"\s*\(", txt, flags=re.M)
    assert re.search(r"^#define\s+RG_SIM_EXCLUDE_SELF\s+1\s*$", txt, flags=re.M)


def test_symbols_are_exported_and_bound():
    from recommendation_gans_amd import _lib, build
    assert "rg_item_sim.hip" in build.SOURCES and "rg_topk_lists.h" in build.HEADERS
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert len(sig[NORMS][1]) == 5 and len(sig[LEN][1]) == 4 and len(sig[NAME][1]) == 13
    assert all(hasattr(_lib.load(), n) for n in (NORMS, LEN, NAME))
    assert _lib.RG_SIM_EXCLUDE_SELF == 1


def call(stream=None, table=P, rnorm=P, dim=16, num_rows=300, queries=P, n_queries=4, flags=1, k=10, splits=1, ws=P,
         out_idx=P, out_sims=P):
    from recommendation_gans_amd import _lib
    return _lib.load().rg_item_sim_topk(stream, table, rnorm, dim, num_rows, queries, n_queries, flags, k, splits, ws,
                                        out_idx, out_sims)


REFUSALS = [
    (dict(table=None), b"null"), (dict(queries=None), b"null"), (dict(ws=None), b"null"), (dict(out_idx=None), b"null"),
    (dict(dim=0), b"dim"), (dict(dim=-4), b"dim"), (dict(dim=257), b"dim"),
    (dict(flags=2), b"flag"), (dict(flags=3), b"flag"), (dict(flags=-1), b"flag"), (dict(flags=1 << 30), b"flag"),
    (dict(num_rows=0), b"num_items < 1"), (dict(num_rows=-1), b"num_items < 1"),
    (dict(num_rows=INT_MAX + 1), b"int32"),
    (dict(n_queries=-1), b"n_users < 0"),
    (dict(k=0), b"k must be"), (dict(k=33), b"k must be"), (dict(k=-1), b"k must be"),
    (dict(k=10, num_rows=9), b"k must be"),
    (dict(k=10, num_rows=10, flags=1), b"k must be"),                   # the query's own row does not count
    (dict(k=1, num_rows=1, flags=1), b"k must be"),
    (dict(k=32, num_rows=32, flags=1, rnorm=None), b"k must be"),
    (dict(splits=-1), b"splits"), (dict(splits=4), b"splits"),          # 300 rows are 3 tiles
    # more (query group, split) workgroups than one launch holds
    (dict(num_rows=1 << 30, splits=1 << 23, n_queries=1 << 20), b"too many"),
    (dict(n_queries=1 << 27), b"too many"), (dict(n_queries=1 << 27, splits=0), b"too many"),
]


@pytest.mark.parametrize("kw,reason", REFUSALS)
def test_refusals_name_their_reason(kw, reason):
    from recommendation_gans_amd import _lib
    rc = call(**kw)
    msg = _lib.load().rg_last_error()
    assert rc != 0 and NAME.encode() in msg and reason in msg, (rc, msg)


def test_no_queries_is_ok_and_launches_nothing():
    assert call(n_queries=0) == 0
    assert call(n_queries=0, splits=0) == 0 and call(n_queries=0, splits=3, k=32, dim=256) == 0
    assert call(n_queries=0, rnorm=None, out_sims=None, flags=0) == 0
    assert call(n_queries=0, k=10, num_rows=10, flags=0) == 0           # with self in, k may reach num_rows
    assert call(n_queries=0, k=9, num_rows=10, flags=1) == 0


@pytest.mark.parametrize("kw,reason", [
    (dict(table=None), b"null"), (dict(out=None), b"null"), (dict(dim=0), b"dim < 1"), (dict(dim=-3), b"dim < 1"),
    (dict(rows=-1), b"rows < 0"), (dict(rows=16 * INT_MAX + 1), b"too many rows"),
])
def test_row_rnorms_refusals_name_their_reason(kw, reason):
    from recommendation_gans_amd import _lib
    a = dict(table=P, rows=5, dim=8, out=P)
    a.update(kw)
    L = _lib.load()
    rc = L.rg_row_rnorms(None, a["table"], a["rows"], a["dim"], a["out"])
    msg = L.rg_last_error()
    assert rc != 0 and NORMS.encode() in msg and reason in msg, (rc, msg)


def test_row_rnorms_of_no_rows_is_ok_and_launches_nothing():
    from recommendation_gans_amd import _lib
    assert _lib.load().rg_row_rnorms(None, P, 0, 8, P) == 0
    assert _lib.load().rg_row_rnorms(None, P + 4, 0, 1 << 20, P) == 0


def test_workspace_length():
    from recommendation_gans_amd import _lib
    L = _lib.load()
    ws = L.rg_item_sim_workspace_len
    assert ws(300, 100, 10, 1) == 8 * 100 * 10
    assert ws(300, 100, 10, 3) == 8 * 100 * 10 * 3
    assert ws(300, 0, 10, 3) == 0
    assert ws(300, 100, 10, 1) < ws(300, 101, 10, 1) < ws(300, 101, 11, 1) < ws(300, 101, 11, 2)
    # splits == 0: the library's pick, within [1, row tiles]; the formula of rg_mf_topk_workspace_len
    assert ws(300, 100, 10, 0) % (8 * 100 * 10) == 0 and 1 <= ws(300, 100, 10, 0) // (8 * 100 * 10) <= 3
    assert ws(100, 100, 10, 0) == 8 * 100 * 10                          # one tile: one split
    for args in [(300, 100, 10, 0), (300, 100, 10, 2), (5000, 7, 32, 0), (5000, 7, 32, 40), (129, 65, 1, 2)]:
        assert ws(*args) == L.rg_mf_topk_workspace_len(*args), args
    for args, reason in [((0, 4, 10, 1), b"num_items < 1"), ((INT_MAX + 1, 4, 10, 1), b"int32"),
                         ((300, -1, 10, 1), b"n_users < 0"), ((300, 4, 0, 1), b"k must be"),
                         ((300, 4, 33, 1), b"k must be"), ((9, 4, 10, 1), b"k must be"),
                         ((300, 4, 10, -1), b"splits"), ((300, 4, 10, 4), b"splits"),
                         ((300, 1 << 27, 10, 1), b"too many"), ((300, 1 << 27, 10, 0), b"too many"),
                         ((1 << 30, 1 << 20, 10, 1 << 23), b"too many")]:
        assert ws(*args) == -1, args
        msg = L.rg_last_error()
        assert LEN.encode() in msg and reason in msg, (args, msg)


def test_similar_rows_refuses_tables_it_cannot_take():
    """mf_engine.similar_rows and row_rnorms raise for a table that is not on a CUDA device: no fall-back."""
    import torch
    from recommendation_gans_amd import mf_engine
    t = torch.randn(7, 4)
    for table in (t, t.numpy(), t.double(), t.t()):
        with pytest.raises(ValueError):
            mf_engine.similar_rows(table, np.array([0, 1]), 3)
        with pytest.raises(ValueError):
            mf_engine.similar_rows(table, np.array([0, 1]), 3, metric="dot", exclude_self=False)
        with pytest.raises(ValueError):
            mf_engine.row_rnorms(table)


I = 9


def bare(kind="mf", neumf=False):
    """A model that holds only its shape (tests/test_recommend_cpu.py); NCF / NeuMF: and the flag
    similar_items asks its engine for."""
    from recommendation_gans_amd.implicit import ImplicitFactorizationModel
    m = ImplicitFactorizationModel.__new__(ImplicitFactorizationModel)
    m._num_users, m._num_items, m._kind = 20, I, kind
    if kind != "mf":
        m._engine = types.SimpleNamespace(neumf=neumf)
    return m


@pytest.mark.parametrize("kw", [
    dict(item_ids=[0, I]), dict(item_ids=[-1]), dict(item_ids=np.array([3, 2 ** 40])),
    dict(item_ids=[1], k=0), dict(item_ids=[1], k=-3), dict(item_ids=[1], k=I), dict(item_ids=[1], k=33),
    dict(item_ids=[1], k=I + 1, include_self=True),
    dict(item_ids=[1], metric="euclid"), dict(item_ids=[1], metric=None), dict(item_ids=[], metric="Cosine"),
    dict(item_ids=[1], space="mf"), dict(item_ids=[1], space="mlp"), dict(item_ids=[], space="gmf"),
])
def test_bad_arguments_raise_value_error(kw):
    with pytest.raises(ValueError):
        bare().similar_items(**kw)


def test_space_belongs_to_neumf():
    for space in ("mf", "mlp", "x"):
        with pytest.raises(ValueError):
            bare("ncf").similar_items([], space=space)
    for space in ("gmf", "MLP", 0):
        with pytest.raises(ValueError):
            bare("ncf", neumf=True).similar_items([], space=space)
    for space in (None, "mf", "mlp"):
        assert bare("ncf", neumf=True).similar_items([], k=3, space=space).shape == (0, 3)
    assert bare("ncf").similar_items([], k=3).shape == (0, 3)


def test_k_is_capped_at_32_whatever_the_item_count():
    m = bare()
    m._num_items = 1000
    with pytest.raises(ValueError):
        m.similar_items([1], k=33)
    with pytest.raises(ValueError):
        m.similar_items([1], k=33, include_self=True)


def test_no_ids_is_an_empty_result():
    ids = bare().similar_items(np.zeros(0, np.int64), k=5)
    assert ids.shape == (0, 5) and ids.dtype == np.int64
    ids, sc = bare().similar_items([], k=I - 1, metric="dot", return_scores=True)
    assert ids.shape == sc.shape == (0, I - 1) and sc.dtype == np.float32
    ids, sc = bare().similar_items([], k=I, include_self=True, return_scores=True)
    assert ids.shape == sc.shape == (0, I)
