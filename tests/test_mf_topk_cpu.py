"""The fused MF top-k entry points (rg_mf_topk_users, rg_mf_topk_workspace_len) without a GPU: the
header declares them, the ctypes table binds them, the source is built, every documented refusal
comes back as a non-zero status that names its reason before any HIP call is made (the pointers
here are made-up addresses: a call that got past the checks with n_users > 0 would launch on them),
and the workspace length is the documented 8 * n_users * k * splits bytes."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, LEN = "rg_mf_topk_users", "rg_mf_topk_workspace_len"
P = 4096        # a made-up, 16-byte aligned, non-null address
INT_MAX = 2 ** 31 - 1


def test_header_declares_both_functions():
    txt = open(os.path.join(ROOT, "include", "rg_hip.h")).read()
    assert re.search(r"^\s*int\s+" + NAME + r"\s*\(", txt, flags=re.M)
    assert re.search(r"^\s*int64_t\s+" + LEN + r"\s*\(", txt, flags=re.M)


def test_symbols_are_exported_and_bound():
    from recommendation_gans_amd import _lib, build
    assert "rg_mf_topk.hip" in build.SOURCES and "rg_mf_score_tile.h" in build.HEADERS
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert NAME in sig and len(sig[NAME][1]) == 16
    assert LEN in sig and len(sig[LEN][1]) == 4
    assert hasattr(_lib.load(), NAME) and hasattr(_lib.load(), LEN)


def call(stream=None, uw=P, iw=P, ub=P, ib=P, dim=16, num_items=300, users=P, n_users=4, exc_ptr=None, exc_idx=None,
         k=10, splits=1, ws=P, out_idx=P, out_scores=P):
    from recommendation_gans_amd import _lib
    return _lib.load().rg_mf_topk_users(stream, uw, iw, ub, ib, dim, num_items, users, n_users, exc_ptr, exc_idx, k,
                                        splits, ws, out_idx, out_scores)


REFUSALS = [
    (dict(uw=None), b"null"), (dict(iw=None), b"null"), (dict(ub=None), b"null"), (dict(ib=None), b"null"),
    (dict(users=None), b"null"), (dict(ws=None), b"null"), (dict(out_idx=None), b"null"),
    (dict(exc_ptr=P), b"exc_ptr and exc_idx"), (dict(exc_idx=P), b"exc_ptr and exc_idx"),
    (dict(dim=0), b"dim"), (dict(dim=-4), b"dim"), (dict(dim=257), b"dim"),
    (dict(num_items=0), b"num_items < 1"), (dict(num_items=-1), b"num_items < 1"),
    (dict(num_items=INT_MAX + 1), b"int32"),
    (dict(n_users=-1), b"n_users < 0"),
    (dict(k=0), b"k must be"), (dict(k=33), b"k must be"), (dict(k=-1), b"k must be"),
    (dict(k=10, num_items=9), b"k must be"),
    (dict(splits=-1), b"splits"), (dict(splits=4), b"splits"),          # 300 items are 3 tiles
    # more (user group, split) workgroups than one launch holds
    (dict(num_items=1 << 30, splits=1 << 23, n_users=1 << 20), b"too many"),
    (dict(n_users=1 << 27), b"too many"), (dict(n_users=1 << 27, splits=0), b"too many"),
]


@pytest.mark.parametrize("kw,reason", REFUSALS)
def test_refusals_name_their_reason(kw, reason):
    from recommendation_gans_amd import _lib
    rc = call(**kw)
    msg = _lib.load().rg_last_error()
    assert rc != 0 and NAME.encode() in msg and reason in msg, (rc, msg)


def test_no_users_is_ok_and_launches_nothing():
    assert call(n_users=0) == 0
    assert call(n_users=0, splits=0) == 0 and call(n_users=0, splits=3, k=32, dim=256) == 0
    assert call(n_users=0, exc_ptr=P, exc_idx=P, out_scores=None) == 0


def test_workspace_length():
    from recommendation_gans_amd import _lib
    L = _lib.load()
    ws = L.rg_mf_topk_workspace_len
    # the header: 8 * n_users * k * splits bytes, with one split too (where it is not touched)
    assert ws(300, 100, 10, 1) == 8 * 100 * 10
    assert ws(300, 100, 10, 3) == 8 * 100 * 10 * 3
    assert ws(300, 0, 10, 3) == 0
    assert ws(300, 100, 10, 1) < ws(300, 101, 10, 1) < ws(300, 101, 11, 1) < ws(300, 101, 11, 2)
    # splits == 0: the library's pick, within [1, item tiles]
    assert ws(300, 100, 10, 0) % (8 * 100 * 10) == 0 and 1 <= ws(300, 100, 10, 0) // (8 * 100 * 10) <= 3
    assert ws(100, 100, 10, 0) == 8 * 100 * 10                          # one tile: one split
    for args, reason in [((0, 4, 10, 1), b"num_items < 1"), ((INT_MAX + 1, 4, 10, 1), b"int32"),
                         ((300, -1, 10, 1), b"n_users < 0"), ((300, 4, 0, 1), b"k must be"),
                         ((300, 4, 33, 1), b"k must be"), ((9, 4, 10, 1), b"k must be"),
                         ((300, 4, 10, -1), b"splits"), ((300, 4, 10, 4), b"splits"),
                         ((300, 1 << 27, 10, 1), b"too many"), ((300, 1 << 27, 10, 0), b"too many"),
                         ((1 << 30, 1 << 20, 10, 1 << 23), b"too many")]:
        assert ws(*args) == -1, args
        msg = L.rg_last_error()
        assert LEN.encode() in msg and reason in msg, (args, msg)


def test_engine_function_refuses_tables_and_exclusions_it_cannot_take():
    """mf_engine.topk_users_fused raises for tables that are not on a CUDA device: no fall-back."""
    import numpy as np
    import torch
    from recommendation_gans_amd import mf_engine
    U, I = torch.zeros(5, 4), torch.zeros(7, 4)
    ub, ib = torch.zeros(5), torch.zeros(7)
    with pytest.raises(ValueError):
        mf_engine.topk_users_fused(U, I, ub, ib, np.array([0, 1]), 3)
