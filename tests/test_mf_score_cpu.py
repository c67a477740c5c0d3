"""The all-item MF scoring entry point (rg_mf_score_users) without a GPU: the header declares it
and its tile constants, the ctypes table binds it, and every documented refusal comes back as a
non-zero status that names its reason before any HIP call is made (the pointers here are made-up
addresses: a call that got past the checks with n_users > 0 would launch on them)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rg_mf_score_users"
P = 4096        # a made-up, 16-byte aligned, non-null address


def test_header_declares_the_function_and_tile_constants():
    txt = open(os.path.join(ROOT, "include", "rg_hip.h")).read()
    assert re.search(r"^\s*int\s+" + NAME + r"\s*\(", txt, flags=re.M)
    from recommendation_gans_amd import _lib
    for c in ("RG_MF_SCORE_ITEM_TILE", "RG_MF_SCORE_USER_GROUP"):
        m = re.search(r"#define\s+" + c + r"\s+(\d+)", txt)
        assert m and int(m.group(1)) == getattr(_lib, c), c
    assert _lib.RG_MF_SCORE_ITEM_TILE % 16 == 0 and _lib.RG_MF_SCORE_USER_GROUP % 16 == 0


def test_symbol_is_exported_and_bound():
    from recommendation_gans_amd import _lib, build
    assert "rg_mf_score.hip" in build.SOURCES
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert NAME in sig and len(sig[NAME][1]) == 11
    assert hasattr(_lib.load(), NAME)


def call(stream=None, uw=P, iw=P, ub=P, ib=P, dim=16, num_items=40, users=P, n_users=4, out=P, ld=40):
    from recommendation_gans_amd import _lib
    return _lib.load().rg_mf_score_users(stream, uw, iw, ub, ib, dim, num_items, users, n_users, out, ld)


@pytest.mark.parametrize("kw,reason", [
    (dict(uw=None), b"null"), (dict(iw=None), b"null"), (dict(ub=None), b"null"), (dict(ib=None), b"null"),
    (dict(users=None), b"null"), (dict(out=None), b"null"),
    (dict(dim=0), b"dim"), (dict(dim=-4), b"dim"), (dict(dim=257), b"dim"),
    (dict(num_items=0, ld=0), b"num_items < 1"), (dict(num_items=-1, ld=0), b"num_items < 1"),
    (dict(ld=39), b"ld < num_items"),
    (dict(n_users=-1), b"n_users < 0"),
    # more (item tile, user group) workgroups than one launch holds
    (dict(num_items=1 << 40, ld=1 << 40, n_users=1 << 20), b"too many"),
])
def test_refusals_name_their_reason(kw, reason):
    from recommendation_gans_amd import _lib
    rc = call(**kw)
    msg = _lib.load().rg_last_error()
    assert rc != 0 and b"rg_mf_score_users" in msg and reason in msg, (rc, msg)


def test_tolerance_holds_for_a_sequential_float32_sum():
    """The GPU test compares the kernel with float64 at rtol 1e-5, atol 1e-7 on these inputs.  That
    only makes sense if fp32 arithmetic of the kernel's shape (one accumulator per score, k
    ascending) stays inside it: checked here on the host, at every dim the GPU test runs."""
    import numpy as np
    from tests.mf_score_common import ATOL, DIMS, GRID_DIMS, RTOL, block32_sequential, block64, random_tables
    users = np.arange(40)
    for dim in DIMS + GRID_DIMS:
        tabs = random_tables(40, 150, dim, seed=dim)
        ref, got = block64(tabs, users), block32_sequential(tabs, users)
        worst = float(np.max(np.abs(got - ref) / np.abs(ref)))
        print(f"dim {dim}: float32 sequential vs float64, max rel diff {worst:.3g}")
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=f"dim {dim}")
        assert worst < RTOL / 4         # headroom: another fp32 order or exp may differ by as much again


def test_no_users_is_ok_and_launches_nothing():
    assert call(n_users=0) == 0
    assert call(n_users=0, dim=1) == 0 and call(n_users=0, dim=256) == 0
    assert call(n_users=0, ld=45) == 0
