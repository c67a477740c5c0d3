"""rg_gan_recommend and rg_gan_recommend_scratch_bytes without a GPU: the header declares them,
the ctypes table binds them, every documented refusal comes back as a non-zero status that names
its reason before any HIP call is made (the pointers here are made-up addresses: a call that got
past the checks would launch on them), the scratch length follows the documented formula,
CGAN.recommend needs a fitted model, and the host replay the GPU tests compare against does what
the contract says on hand-made blocks."""
import ctypes

import numpy as np
import pytest

from tests.gan_recommend_common import replay

NAME, LEN = "rg_gan_recommend", "rg_gan_recommend_scratch_bytes"
P = 4096        # a made-up, 16-byte aligned, non-null address


def model(N=300, S=3, H=64, E=8, Z=12, B=4, g=P, d=P):
    from recommendation_gans_amd import _lib
    m = _lib.GANModel()
    m.dims = _lib.GANDims(N, S, H, E, Z, B)
    m.g, m.d = g, d
    return m


def batch(rows=2, L=5, hist=P):
    from recommendation_gans_amd import _lib
    b = _lib.GANBatch()
    b.rows, b.hist_len, b.hist = rows, L, hist
    return b


def call(mdl="default", ws=P, bt="default", z=P, flags=3, path=0, scratch=P, slates=P):
    from recommendation_gans_amd import _lib
    mdl = model() if mdl == "default" else mdl
    bt = batch() if bt == "default" else bt
    return _lib.load().rg_gan_recommend(None, ctypes.byref(mdl) if mdl is not None else None, ws,
                                        ctypes.byref(bt) if bt is not None else None, z, flags, path, scratch, slates)


def test_symbols_are_declared_exported_and_bound():
    import os
    import re
    from recommendation_gans_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "rg_hip.h")).read()
    assert re.search(r"^\s*int\s+" + NAME + r"\s*\(", txt, flags=re.M)
    assert re.search(r"^\s*int64_t\s+" + LEN + r"\s*\(", txt, flags=re.M)
    assert re.search(r"#define\s+RG_GAN_REC_EXCLUDE_HISTORY\s+1\b", txt)
    assert re.search(r"#define\s+RG_GAN_REC_DISTINCT\s+2\b", txt)
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert len(sig[NAME][1]) == 9 and len(sig[LEN][1]) == 2
    assert hasattr(_lib.load(), NAME) and hasattr(_lib.load(), LEN)
    assert (_lib.GAN_REC_EXCLUDE_HISTORY, _lib.GAN_REC_DISTINCT) == (1, 2)


REFUSALS = [
    (dict(mdl=None), b"null"), (dict(ws=None), b"null"), (dict(bt=None), b"null"), (dict(z=None), b"null"),
    (dict(scratch=None), b"null"), (dict(slates=None), b"null"),
    # what check_common refuses for every rg_gan_* entry
    (dict(mdl=model(g=None)), b"null"), (dict(mdl=model(d=None)), b"null"),
    (dict(mdl=model(N=0)), b"bad dims"), (dict(mdl=model(S=0)), b"bad dims"), (dict(mdl=model(H=60)), b"bad dims"),
    (dict(mdl=model(E=0)), b"bad dims"), (dict(mdl=model(Z=0)), b"bad dims"), (dict(mdl=model(B=0)), b"bad dims"),
    (dict(bt=batch(rows=0)), b"rows must be"), (dict(bt=batch(rows=5)), b"rows must be"),
    (dict(bt=batch(L=0)), b"empty history"), (dict(bt=batch(hist=None)), b"empty history"),
    (dict(flags=-1), b"flags"), (dict(flags=4), b"flags"),
    (dict(path=-1), b"path must be"), (dict(path=3), b"path must be"),
    (dict(path=2, mdl=model(N=127)), b"fused path needs"), (dict(path=2, mdl=model(S=9)), b"fused path needs"),
    (dict(mdl=model(S=33)), b"slate_size above 32"), (dict(path=1, mdl=model(S=33, N=5)), b"slate_size above 32"),
    (dict(scratch=P + 8), b"16-byte aligned"),
]


@pytest.mark.parametrize("kw,reason", REFUSALS)
def test_refusals_name_their_reason(kw, reason):
    from recommendation_gans_amd import _lib
    rc = call(**kw)
    msg = _lib.load().rg_last_error()
    assert rc != 0 and reason in msg, (rc, msg)
    assert b"rg_gan" in msg


def test_scratch_length_formula():
    from recommendation_gans_amd import _lib
    fn = _lib.load().rg_gan_recommend_scratch_bytes

    def length(N, S, B, path=0):
        return fn(ctypes.byref(_lib.GANDims(N, S, 64, 8, 12, B)), path)

    def want(N, S, B, fused):
        bitmap = -(-(4 * B * -(-N // 32)) // 16) * 16
        T = 4 if S <= 4 else 8
        return bitmap + (8 * B * -(-(S * N) // 128) * 2 * T if fused else 0)

    for N, S, B in [(300, 3, 4), (130, 8, 129), (128, 1, 1), (26744, 5, 256), (1000, 4, 7), (1000, 5, 7)]:
        assert length(N, S, B) == length(N, S, B, 2) == want(N, S, B, True), (N, S, B)
        assert length(N, S, B, 1) == want(N, S, B, False)
        assert length(N, S, B) % 16 == 0
    # the fused path cannot apply: the bitmap alone
    for N, S, B in [(127, 3, 4), (5, 8, 2), (300, 9, 4), (300, 32, 3), (33, 1, 1)]:
        assert length(N, S, B) == length(N, S, B, 1) == want(N, S, B, False), (N, S, B)
        assert length(N, S, B, 2) == -1 and b"fused path needs" in _lib.load().rg_last_error()
    assert length(26744, 5, 256) == 4 * 256 * 836 + 8 * 256 * 1045 * 2 * 8
    for args, reason in [((0, 3, 4), b"bad dims"), ((300, 0, 4), b"bad dims"), ((300, 3, 0), b"bad dims"),
                         ((300, 33, 4), b"slate_size above 32"), ((300, 3, 4, 3), b"path must be"),
                         ((300, 3, 4, -1), b"path must be")]:
        assert length(*args) == -1, args
        msg = _lib.load().rg_last_error()
        assert LEN.encode() in msg and reason in msg, (args, msg)
    assert fn(None, 0) == -1 and b"null" in _lib.load().rg_last_error()


def test_recommend_before_fit_raises(tmp_path, monkeypatch):
    from recommendation_gans_amd.CGANs import CGAN
    monkeypatch.chdir(tmp_path)
    m = CGAN(slate_size=3, experiment_name="rec")
    with pytest.raises(RuntimeError, match=r"call fit\(\) first"):
        m.recommend(np.zeros((2, 4), np.float32))


# ---------------------------------------------------------------- the host replay
def block():
    """2 rows x 3 heads x 6 items, with ties, a saturated pair and a NaN."""
    f = np.array([
        # row 0: head 0 ties items 1 and 4 at 1.0; head 1 has its maximum at 1 too; head 2 is flat
        [[0.2, 1.0, -0.3, 0.5, 1.0, 0.1], [0.0, 0.9, 0.8, -1.0, 0.7, 0.9], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]],
        # row 1: head 0's largest number is item 2, a NaN sits at 0; head 1 is all NaN; head 2 plain
        [[np.nan, -0.5, 0.4, 0.4, -1.0, np.nan], [np.nan] * 6, [-0.1, -0.2, 0.3, 0.9, 0.8, 0.7]],
    ], dtype=np.float32)
    return f.reshape(2, 18)


def test_replay_first_maximum_and_ties():
    f = block()
    hist = np.full((2, 2), 6)
    got = replay(f, hist, 6, 3, False, False)
    # per-head first maximum; a NaN is below every number, all NaN: the lowest id
    assert got.tolist() == [[1, 1, 0], [2, 0, 3]]
    assert (got == np.nanargmax(np.where(np.isnan(f), -2, f).reshape(2, 3, 6), axis=2)).all()


def test_replay_distinct_walks_the_heads_in_order():
    f = block()
    hist = np.full((2, 2), 6)
    # row 0: head 0 takes 1 (the tie's lower id), head 1 then 5 (0.9, after 1 is gone), head 2 item 0
    # row 1: head 0 takes 2, head 1 (all NaN) the lowest id left, 0, head 2 item 3
    assert replay(f, hist, 6, 3, False, True).tolist() == [[1, 5, 0], [2, 0, 3]]


def test_replay_history_padding_and_out_of_range_ids():
    f = block()
    hist = np.array([[1, 6, 1, 4, -3, 99], [3, 6, 6, 6, 6, 6]])        # repeats, padding, ids to ignore
    assert replay(f, hist, 6, 3, True, False).tolist() == [[3, 5, 0], [2, 0, 4]]
    assert replay(f, hist, 6, 3, True, True).tolist() == [[3, 5, 0], [2, 0, 4]]
    hist = np.array([[1, 4, 3, 6, 6, 6], [2, 3, 6, 6, 6, 6]])
    # row 0: head 0 -> 0 (0.2), head 1 -> 5 (0.9), head 2 -> 2 (0 and 5 taken)
    # row 1: head 0 -> 1 (-0.5 beats -1.0 and the NaNs), head 1 -> 0, head 2 -> 4
    assert replay(f, hist, 6, 3, True, True).tolist() == [[0, 5, 2], [1, 0, 4]]


def test_replay_full_history_and_exhaustion():
    f = block()
    full = np.array([[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]])
    assert replay(f, full, 6, 3, True, True).tolist() == [[6, 6, 6], [6, 6, 6]]
    assert replay(f, full, 6, 3, True, False).tolist() == [[6, 6, 6], [6, 6, 6]]
    assert replay(f, full, 6, 3, False, True).tolist() == [[1, 5, 0], [2, 0, 3]]
    # two items left for three heads: they come in each head's value order, then the padding id
    two = np.array([[0, 1, 2, 3, 6, 6], [0, 1, 2, 5, 5, 5]])
    assert replay(f, two, 6, 3, True, True).tolist() == [[4, 5, 6], [3, 4, 6]]
