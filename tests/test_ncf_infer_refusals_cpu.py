"""The model check shared by rg_ncf_score_workspace_len, rg_ncf_score_users and rg_ncf_score_pairs,
without a GPU: every refusal that comes before any HIP call returns non-zero and names its reason in
rg_last_error().

Refusals only: the non-null pointers are dummy integers, which a refused call never dereferences,
and no call here could pass validation (so nothing is launched and n == 0 is not exercised)."""
import ctypes

import pytest

from recommendation_gans_amd import _lib

U, I, E, M, N = 12, 40, 16, 5, 4
TABLE, IDS, IDS2, WS, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000     # 16-byte aligned, never read


def model(**kw):
    m = _lib.NCFModel(TABLE, TABLE + 0x1000, None, None, None, None, TABLE + 0x2000, None, None, U, I, E, M)
    m.mf_user_w, m.mf_item_w = TABLE + 0x3000, TABLE + 0x4000
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def workspace_len(model=model(), n=N, **_):
    return _lib.load().rg_ncf_score_workspace_len(ctypes.byref(model) if model is not None else None, n)


def users(model=model(), users=IDS, n=N, ws=WS, out=OUT, ld=I, **_):
    return _lib.load().rg_ncf_score_users(None, ctypes.byref(model) if model is not None else None, users, n, ws, out, ld)


def pairs(model=model(), users=IDS, items=IDS2, n=N, out=OUT, **_):
    return _lib.load().rg_ncf_score_pairs(None, ctypes.byref(model) if model is not None else None, users, items, n, out)


# what every entry point refuses on the model's shape alone ...
SHAPE = [(dict(model=None), b"null"), (dict(model=model(dim=48)), b"dim"), (dict(model=model(mf_dim=129)), b"mf_dim"),
         (dict(model=model(mf_dim=-1)), b"mf_dim")]
# ... and the two launching ones on the model's pointers
POINTERS = [(dict(model=model(user_w=None)), b"null"), (dict(model=model(item_w=None)), b"null"),
            (dict(model=model(mlp=None)), b"null"), (dict(users=None), b"null"), (dict(out=None), b"null"),
            (dict(model=model(mf_user_w=None)), b"GMF"), (dict(model=model(mf_item_w=None)), b"GMF")]
CASES = [(workspace_len, kw, msg) for kw, msg in SHAPE + [(dict(n=-1), b"n_users")]]
CASES += [(users, kw, msg) for kw, msg in SHAPE + POINTERS + [
    (dict(ws=None), b"null"), (dict(n=-1), b"n_users"), (dict(ld=I - 1), b"ld"), (dict(ws=WS + 4), b"16-byte aligned")]]
CASES += [(pairs, kw, msg) for kw, msg in SHAPE + POINTERS + [
    (dict(items=None), b"null"), (dict(n=-1), b"n < 0"), (dict(model=model(user_w=TABLE + 4)), b"16-byte aligned"),
    (dict(model=model(item_w=TABLE + 0x1008)), b"16-byte aligned")]]


def case_id(c):
    entry, kw, msg = c
    (k, v), = kw.items()
    if isinstance(v, _lib.NCFModel):
        k, v = next((f, getattr(v, f)) for f, _ in v._fields_ if getattr(v, f) != getattr(model(), f))
    return f"{entry.__name__}-{k}={v}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusal_names_its_reason(case):
    entry, kw, msg = case
    assert entry(**kw) != 0
    err = _lib.load().rg_last_error()
    assert msg in err and entry.__name__.encode() in err, err
