"""rg_topk_rows_wide and the k > 32 routing of the ranking metrics without a GPU: every documented
refusal comes back as a non-zero status that names its reason before any HIP call is made (the
pointers here are made-up addresses: a call that got past the checks with rows > 0 would launch on
them), the Python constant is the header's, a model that names no ``topk_users_max`` keeps the host
path above k = 32, and one that names 1024 gives the host loop's metric values to the bit."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096        # a made-up, 16-byte aligned, non-null address
INT_MAX = 2 ** 31 - 1


def call(stream=None, scores=P, rows=4, cols=300, ld=None, k=50, out_idx=P, out_val=P):
    from recommendation_gans_amd import _lib
    return _lib.load().rg_topk_rows_wide(stream, scores, rows, cols, cols if ld is None else ld, k, out_idx, out_val)


REFUSALS = [
    (dict(scores=None), b"null"), (dict(out_idx=None), b"null"),
    (dict(rows=-1), b"bad shape"), (dict(cols=0), b"bad shape"), (dict(cols=-5), b"bad shape"),
    (dict(ld=299), b"bad shape"),
    (dict(cols=INT_MAX + 1), b"int32"), (dict(rows=INT_MAX + 1), b"too many rows"),
    (dict(k=0), b"k must be"), (dict(k=-1), b"k must be"), (dict(k=1025, cols=5000), b"k must be"),
    (dict(k=301), b"k must be"), (dict(k=1024, cols=1023), b"k must be"),
]


@pytest.mark.parametrize("kw,reason", REFUSALS)
def test_refusals_name_their_reason(kw, reason):
    from recommendation_gans_amd import _lib
    rc = call(**kw)
    msg = _lib.load().rg_last_error()
    assert rc != 0 and reason in msg, (kw, rc, msg)


def test_no_rows_is_ok_without_a_launch():
    from recommendation_gans_amd import _lib
    assert call(rows=0) == _lib.RG_OK
    assert call(rows=0, out_val=None) == _lib.RG_OK
    assert call(rows=0, k=0) != 0               # the arguments are still checked


def test_constant_and_binding_match_the_header():
    from recommendation_gans_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "rg_hip.h")).read()
    m = re.search(r"^#define\s+RG_TOPK_WIDE_MAX\s+(\d+)", txt, flags=re.M)
    assert m and int(m.group(1)) == _lib.RG_TOPK_WIDE_MAX == 1024
    assert re.search(r"^\s*int\s+rg_topk_rows_wide\s*\(", txt, flags=re.M)
    assert "rg_topk_wide.hip" in build.SOURCES
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert len(sig["rg_topk_rows_wide"][1]) == 8 and hasattr(_lib.load(), "rg_topk_rows_wide")
    from recommendation_gans_amd.implicit import ImplicitFactorizationModel
    from recommendation_gans_amd.spotlight import evaluation
    assert ImplicitFactorizationModel.topk_users_max == _lib.RG_TOPK_WIDE_MAX and evaluation.TOPK_MAX == 32


class _TopkModel:
    """tests/test_eval_cpu.py's model: scores on the host, topk_users the first k ids of the stable
    argsort with the excluded (train) items last; both methods count their calls."""

    def __init__(self, scores):
        self.s = scores
        self.calls = {"score_users": 0, "topk_users": 0}

    def score_users(self, users):
        self.calls["score_users"] += 1
        return self.s[np.asarray(users)].copy()

    def topk_users(self, users, k, exclude_csr=None):
        self.calls["topk_users"] += 1
        sub = -self.s[np.asarray(users)].astype(np.float32)
        if exclude_csr is not None:
            for r, u in enumerate(users):
                sub[r, exclude_csr.indices[exclude_csr.indptr[u]:exclude_csr.indptr[u + 1]]] = np.finfo(np.float32).max
        return np.argsort(sub, axis=1, kind="stable")[:, :k].astype(np.int64)


class _WideModel(_TopkModel):
    topk_users_max = 1024


class _HostOnly:
    def __init__(self, m):
        self.score_users = m.score_users


def _data():
    from recommendation_gans_amd.spotlight.interactions import Interactions
    rs = np.random.RandomState(0)
    U, I = 400, 700
    scores = rs.rand(U, I).astype(np.float32)
    tu, ti = rs.randint(0, U, 4000), rs.randint(0, I, 4000)
    tu, ti = np.append(tu, [U - 1]), np.append(ti, [0])              # a user whose only test item is 0
    keep = ~((tu == U - 1) & (ti != 0))
    test = Interactions(tu[keep], ti[keep], num_users=U, num_items=I)
    train = Interactions(rs.randint(0, U - 50, 9000), rs.randint(0, I, 9000), num_users=U, num_items=I)
    # hit_ratio reads `target in ranking[:k]` with a user's whole target array: one item per user
    one = np.unique(test.user_ids, return_index=True)[1]
    single = Interactions(test.user_ids[one], test.item_ids[one], num_users=U, num_items=I)
    return scores, test, train, single


def test_a_model_without_the_attribute_keeps_the_host_path_above_32():
    from recommendation_gans_amd.spotlight import evaluation
    scores, test, train, single = _data()
    m = _TopkModel(scores)
    evaluation.precision_recall_score(m, test, train, k=50)
    evaluation.precision_recall_score(m, test, k=[5, 50])
    evaluation.map_at_k(m, test, k=50)
    evaluation.hit_ratio(m, single, k=50)
    assert m.calls["topk_users"] == 0 and m.calls["score_users"] > 0
    evaluation.precision_recall_score(m, test, train, k=32)        # and the device path up to 32, as before
    assert m.calls["topk_users"] > 0


def test_a_model_with_the_attribute_gives_the_host_loops_values():
    from recommendation_gans_amd.spotlight import evaluation
    scores, test, train, single = _data()
    m = _WideModel(scores)
    h = _HostOnly(m)
    for k in (50, [5, 50]):
        kk = max(k) if isinstance(k, list) else k
        assert evaluation.precision_recall_score(m, test, k=k) == evaluation.precision_recall_score(h, test, k=k)
        assert evaluation.precision_recall_score(m, test, train, k=k) == \
            evaluation.precision_recall_score(h, test, train, k=k)
        assert evaluation.map_at_k(m, test, k=kk) == evaluation.map_at_k(h, test, k=kk)
    calls = m.calls["score_users"]
    got = evaluation.hit_ratio(m, single, k=50)
    assert m.calls["score_users"] == calls                          # the ranking came from topk_users
    assert got == evaluation.hit_ratio(h, single, k=50)
