"""The all-item NCF / NeuMF scoring entry points without a GPU: the header declares them, the
ctypes table binds them, and rg_ncf_score_workspace_len (host code) returns the documented size
and refuses what rg_ncf_score_users refuses."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rg_ncf_score_workspace_len", "rg_ncf_score_users")


def test_header_declares_the_functions_and_tile_constants():
    txt = open(os.path.join(ROOT, "include", "rg_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^\s*(?:int64_t|int)\s+" + n + r"\s*\(", txt, flags=re.M), n
    from recommendation_gans_amd import _lib
    for c in ("RG_NCF_SCORE_ITEM_TILE", "RG_NCF_SCORE_USER_GROUP"):
        m = re.search(r"#define\s+" + c + r"\s+(\d+)", txt)
        assert m and int(m.group(1)) == getattr(_lib, c), c


def test_binding_has_the_functions():
    from recommendation_gans_amd import _lib
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert set(NAMES) <= bound
    L = _lib.load()
    for n in NAMES:
        assert hasattr(L, n)


def model(I, E, M, U=10):
    from recommendation_gans_amd import _lib
    return _lib.NCFModel(None, None, None, None, None, None, None, None, None, U, I, E, M)


@pytest.mark.parametrize("I,E,M,n", [(97, 64, 0, 9), (26744, 64, 0, 4096), (97, 16, 50, 9), (97, 8, 5, 1),
                                     (5, 32, 1, 0), (300, 64, 128, 65)])
def test_workspace_len_is_the_documented_size(I, E, M, n):
    """(num_items + n_users) * dim floats for the two halves of the first layer, plus n_users rows of
    mf_dim rounded up to a multiple of 4 for NeuMF's scaled GMF user rows."""
    from recommendation_gans_amd import _lib
    L = _lib.load()
    assert L.rg_ncf_score_workspace_len(ctypes.byref(model(I, E, M)), n) == (I + n) * E + n * ((M + 3) // 4 * 4)


def test_workspace_len_refuses_bad_models():
    from recommendation_gans_amd import _lib
    L = _lib.load()
    assert L.rg_ncf_score_workspace_len(None, 4) < 0 and b"null" in L.rg_last_error()
    assert L.rg_ncf_score_workspace_len(ctypes.byref(model(97, 48, 0)), 4) < 0 and b"dim" in L.rg_last_error()
    assert L.rg_ncf_score_workspace_len(ctypes.byref(model(97, 16, 129)), 4) < 0 and b"mf_dim" in L.rg_last_error()
    assert L.rg_ncf_score_workspace_len(ctypes.byref(model(97, 16, -1)), 4) < 0
    assert L.rg_ncf_score_workspace_len(ctypes.byref(model(97, 16, 0)), -1) < 0 and b"n_users" in L.rg_last_error()
