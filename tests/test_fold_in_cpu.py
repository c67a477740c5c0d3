"""Fold-in without a GPU: the two float64 references agree (the product's chain of torch ops and
the numpy restatement with hand-written gradients), the leave-out rule stays within its cap on every
case, ``mf_engine.fold_in_users`` refuses bad arguments before any GPU call, the three forms of
``histories`` give one CSR, and the negatives are NumPy's draws."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from recommendation_gans_amd import mf_engine
from recommendation_gans_amd.implicit import _fold_negatives, _histories_csr
from recommendation_gans_amd.spotlight.interactions import Interactions
from tests import fold_in_common as fc


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=fc.CASE_IDS)
def test_the_two_float64_references_agree_and_few_elements_are_left_out(i):
    d = fc.case_data(i)
    (W, b, lv), r64 = d["ref"], d["r64"]
    keep_W, keep_b = d["keep_W"], d["keep_b"]
    # kept elements: 1e-12 relative (an element whose gradient cancels to rounding level is one
    # Adam turns into +-lr either way: those are the left-out ones)
    np.testing.assert_allclose(r64["W"][keep_W], W[keep_W], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r64["b"][keep_b], b[keep_b], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r64["loss"][d["row_ok"]], lv[d["row_ok"]], rtol=1e-12, atol=1e-15)
    print(f"case {fc.CASE_IDS[i]}: E32 {d['e32']:.3e} E32(loss) {d['e32_loss']:.3e} left out {d['left_out']:.4f}")
    assert d["left_out"] <= fc.LEFT_OUT_CAP
    assert 0.0 < d["e32"] < 1e-4
    empty = np.diff(d["case"]["ptr"]) == 0          # an empty row is its start, bit for bit
    assert (W[empty] == d["case"]["W0"][empty]).all() and (b[empty] == d["case"]["b0"][empty]).all()
    assert (lv[empty] == 0).all()


def _args(**over):
    case = fc.make_case(8, 3, 2, lens=[2, 0, 3])
    a = dict(item_w=torch.from_numpy(case["Q"]), item_b=torch.from_numpy(case["c"]), hist_ptr=case["ptr"].copy(),
             hist_idx=case["idx"].copy(), neg_idx=case["neg"].copy(), n_neg=2, loss="hinge", steps=3, lr=0.05)
    a.update(over)
    return a


@pytest.mark.parametrize("over, match", [
    (dict(item_w=torch.zeros(fc.NUM_ITEMS, 8, dtype=torch.float64)), "float32"),
    (dict(hist_idx=np.zeros(5, np.float32)), "int32 or int64"),
    (dict(hist_ptr=np.array([0, 3, 2, 5])), "ascend"),
    (dict(hist_ptr=np.array([0, 2, 2, 4])), "ascend"),
    (dict(hist_idx=np.array([0, 1, fc.NUM_ITEMS, 3, 4])), "outside"),
    (dict(neg_idx=np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1])), "outside"),
    (dict(n_neg=0, neg_idx=None), "pairwise losses need n_neg"),
    (dict(n_neg=33, neg_idx=np.zeros(5 * 33, np.int32)), "n_neg must be in"),
    (dict(steps=-1), "steps must be in"),
    (dict(steps=1025), "steps must be in"),
    (dict(item_w=torch.zeros(fc.NUM_ITEMS, 257)), "dim must be in"),
    (dict(loss="pointwise_pos"), "unknown loss"),
    (dict(neg_idx=np.zeros(9, np.int32)), "n_neg ids per history entry"),
    (dict(init=(torch.zeros(3, 7), torch.zeros(3))), "init must be"),
    (dict(), "CUDA"),                         # host tables: refused, never a torch fall-back
])
def test_fold_in_users_refuses_before_any_gpu_call(over, match, monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(mf_engine._lib, "load", no_gpu)
    with pytest.raises(ValueError, match=match):
        mf_engine.fold_in_users(**_args(**over))


def test_the_three_forms_of_histories_give_one_csr():
    rows = [[3, 17, 250], [], [0, 5, 6, 299], [42]]
    I = fc.NUM_ITEMS
    ptr, idx = _histories_csr(rows, I)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32
    assert ptr.tolist() == [0, 3, 3, 7, 8] and idx.tolist() == [3, 17, 250, 0, 5, 6, 299, 42]
    u = np.repeat(np.arange(4), np.diff(ptr)).astype(np.int32)
    mat = sp.csr_matrix((np.ones(len(idx), np.float32), (u, idx)), shape=(4, I))
    inter = Interactions(u, idx.copy(), ratings=np.ones(len(idx), np.float32), num_users=4, num_items=I)
    for other in (mat, mat.tocoo(), inter):
        p2, i2 = _histories_csr(other, I)
        assert p2.dtype == np.int64 and i2.dtype == np.int32
        assert (p2 == ptr).all() and (i2 == idx).all()
    # a list keeps order and duplicates as given
    assert _histories_csr([[9, 2, 9]], I)[1].tolist() == [9, 2, 9]
    with pytest.raises(ValueError):
        _histories_csr(sp.csr_matrix((4, I + 1)), I)
    with pytest.raises(ValueError):
        _histories_csr([[0, I]], I)
    with pytest.raises(ValueError):
        _histories_csr([[-1]], I)


def test_the_negatives_are_numpys_draws_and_advance_the_random_state():
    a, b = np.random.RandomState(77), np.random.RandomState(77)
    got = _fold_negatives(41, 3, fc.NUM_ITEMS, a)
    assert (np.asarray(got) == b.randint(0, fc.NUM_ITEMS, 41 * 3)).all()
    assert a.randint(0, 1 << 30) == b.randint(0, 1 << 30)          # the same state afterwards


def test_adam_step_coef_is_torchs_double_arithmetic():
    c = mf_engine.adam_step_coef(5, 0.05, (0.9, 0.999))
    for t in range(1, 6):
        assert c[t - 1, 0] == 0.05 / (1 - 0.9 ** t) and c[t - 1, 1] == (1 - 0.999 ** t) ** 0.5
