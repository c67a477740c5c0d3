"""rg_gan_score_slates and its Python callers without a GPU: every refusal that is decided before
any HIP call returns RG_E_ARG and names its reason in rg_last_error(); rows == 0 returns RG_OK
without a launch; the argument checks of GANEngine.score_slates, CGAN.recommend(samples=...) and
CGAN.score_slates that need no device.

The non-null pointers are dummy integers, which a refused call (and the launch-free rows == 0
call) never dereferences."""
import ctypes

import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib

RG_E_ARG = -1
N, S, H, E, Z, B, L = 37, 3, 8, 5, 4, 16, 7
D, HIST, SLATES, OUT = 0x10000, 0x20000, 0x30000, 0x40000          # 16-byte aligned, never read


def model(d=D, **dims):
    m = _lib.GANModel()
    m.dims = _lib.GANDims(N, S, H, E, Z, B)
    for k, v in dims.items():
        setattr(m.dims, k, v)
    m.d = d                                                          # g and every m / v stay NULL
    return m


def score(model=model(), hist=HIST, hist_len=L, slates=SLATES, ld=S, rows=5, out=OUT):
    return _lib.load().rg_gan_score_slates(None, ctypes.byref(model) if model is not None else None, hist, hist_len,
                                           slates, ld, rows, out)


REFUSALS = [
    (dict(model=None), b"null"), (dict(model=model(d=None)), b"null"), (dict(hist=None), b"null"),
    (dict(slates=None), b"null"), (dict(out=None), b"null"),
    (dict(model=model(num_items=0)), b"bad dims"), (dict(model=model(slate_size=0)), b"bad dims"),
    (dict(model=model(hidden=0)), b"bad dims"), (dict(model=model(hidden=12)), b"bad dims"),
    (dict(model=model(hidden=-8)), b"bad dims"), (dict(model=model(emb_dim=0)), b"bad dims"),
    (dict(model=model(z_dim=0)), b"bad dims"), (dict(model=model(batch_max=0)), b"bad dims"),
    (dict(model=model(num_items=2 ** 30, slate_size=2)), b"31 bits"),
    (dict(model=model(hidden=8192)), b"LDS"), (dict(model=model(emb_dim=2 ** 30)), b"LDS"),
    (dict(model=model(d=D + 4)), b"16-byte aligned"),
    (dict(hist_len=0), b"hist_len"), (dict(hist_len=-3), b"hist_len"),
    (dict(hist_len=2 ** 31 - 1), b"hist_len too large"), (dict(hist_len=2 ** 31 - 128), b"hist_len too large"),
    (dict(ld=S - 1), b"ld"), (dict(rows=-1), b"rows < 0"),
    (dict(rows=16 * (2 ** 31 - 1) + 1), b"too many rows"), (dict(rows=2 ** 62), b"too many rows"),
    (dict(rows=2 ** 63 - 1), b"too many rows"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[f"{i}-{m.decode().replace(' ', '_')}" for i, (_, m) in enumerate(REFUSALS)])
def test_refusal_names_its_reason(kw, msg):
    assert score(**kw) == RG_E_ARG
    err = _lib.load().rg_last_error()
    assert msg in err and b"rg_gan_score_slates" in err, err


def test_no_rows_is_ok_without_a_launch():
    assert score(rows=0) == _lib.RG_OK
    assert score(rows=0, ld=S + 3, model=model(batch_max=1)) == _lib.RG_OK
    assert score(rows=0, ld=S - 1) == RG_E_ARG                      # still checked


def bare_engine():
    """A GANEngine without its constructor (which needs a device): what score_slates' checks read."""
    from recommendation_gans_amd.gan_engine import GANEngine
    e = GANEngine.__new__(GANEngine)
    e.device, e.S = torch.device("cpu"), S
    return e


def test_engine_argument_checks():
    e = bare_engine()
    hist, sl = torch.zeros(4, L, dtype=torch.int32), torch.zeros(4, S, dtype=torch.int32)
    cases = [dict(hist=hist.to(torch.int64)), dict(slates=sl.to(torch.int64)), dict(slates=sl.float()),
             dict(hist=hist.numpy()), dict(hist=hist[0]), dict(slates=sl[:, 0]),
             dict(hist=torch.zeros(4, 2 * L, dtype=torch.int32)[:, ::2]),
             dict(slates=torch.zeros(4, S + 2, dtype=torch.int32)[:, :S]),
             dict(slates=sl[:3]), dict(slates=sl[:, :S - 1].contiguous()), dict(hist=hist[:, :0]),
             dict(out=torch.zeros(4, dtype=torch.float64)), dict(out=torch.zeros(5)), dict(out=torch.zeros(8)[::2]),
             dict(out=np.zeros(4, np.float32))]
    for kw in cases:
        with pytest.raises(ValueError):
            e.score_slates(**{"hist": hist, "slates": sl, **kw})
    # a device other than the engine's
    e.device = torch.device("cuda:0")
    with pytest.raises(ValueError, match="engine's device"):
        e.score_slates(hist, sl)


@pytest.fixture
def unfitted(tmp_path, monkeypatch):
    from recommendation_gans_amd.CGANs import CGAN
    monkeypatch.chdir(tmp_path)
    return CGAN(slate_size=S, experiment_name="unfitted")


@pytest.mark.parametrize("samples", [0, -2, 1.5, 2.0, "3", None, True])
def test_recommend_refuses_bad_samples(unfitted, samples):
    with pytest.raises(ValueError, match="samples"):
        unfitted.recommend(np.zeros((2, L)), samples=samples)


def test_pick_best_ties_and_nan():
    """recommend(samples=M)'s selection: the highest score, the lower sample on ties, a NaN below
    every number (-inf included), sample 0 when every score is NaN."""
    from recommendation_gans_amd.CGANs import CGAN
    nan, inf = float("nan"), float("inf")
    sc = torch.tensor([[1.0, 2.0, nan, nan, nan, -inf, 0.5, inf],
                       [3.0, 2.0, -inf, nan, 1.0, nan, nan, inf],
                       [3.0, 2.0, -inf, nan, nan, -inf, 0.5, nan],
                       [0.0, 1.0, nan, nan, 1.0, nan, 0.5, 1.0]])
    assert CGAN._pick_best(sc).tolist() == [1, 0, 1, 0, 1, 0, 0, 0]
    assert CGAN._pick_best(sc[:1]).tolist() == [0] * 8


def test_public_entries_need_a_fitted_model(unfitted):
    with pytest.raises(RuntimeError, match="call fit"):
        unfitted.score_slates(np.zeros((2, L)), np.zeros((2, S), np.int64))
    with pytest.raises(RuntimeError, match="call fit"):
        unfitted.recommend(np.zeros((2, L)), samples=4)
