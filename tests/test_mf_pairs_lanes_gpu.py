"""The MF pair pass with one lane per pair (csrc/rg_mf_kernels.h pairs_body): lane q % LPU of a
column's LPU lanes adds pair q's biases, takes its sigmoid and its loss term, in rounds of LPU
pairs, and the column's sums are formed from the broadcast terms.

Shapes: the smallest that reach each path.  U = 50, I = 40, B = 37 (no multiple of the 256 / LPU
columns of a workgroup; with n = 8 some rows overflow their lists); d = 16, 32, 64, 128 on 4, 8,
16 and 32 lanes and d = 160 on the masked scalar layout of 64; n = 1, 5 and RG_MF_MAX_NEG = 8, so
d = 16 runs 1, 2 and 3 rounds and d = 32 a second round holding one pair; every loss, the
positives-only form included; with a plan and without; two steps, the second with 30 positives
for the 37 columns (under pointwise its last 7 columns' negatives pair with no positive), so the
second prepare claims the list slots.  Criterion and tolerances: tests/test_mf_gpu.py check_step
against oracle/mf.py (the float32 oracle and its float64 twin)."""
import copy

import numpy as np
import pytest
import torch

from oracle import mf as omf
from oracle import rng as orng
import tests.test_mf_gpu as tm

pytestmark = pytest.mark.gpu

U, I, B, P = 50, 40, 37, 2000
LOSSES = ["bpr", "hinge", "pointwise", "adaptive_hinge", "pointwise_pos"]
NEGS = [1, 5, 8]
KW = dict(optimizer="adam", lr=1e-2, weight_decay=1e-5)


@pytest.fixture(scope="module")
def dev():
    from recommendation_gans_amd import _lib
    _lib.load()
    assert _lib.RG_MF_MAX_NEG == NEGS[-1]
    return torch.device("cuda:0")


def positives_only_step(o, pu, pi):
    """implicit.py:359-360 (no negative pool): the pointwise loss of the positives alone, no draw;
    oracle/mf.py's pointwise positive terms, its gradients and its optimizer."""
    Uw, Iw, ub, ib = o.params
    pu, pi = torch.as_tensor(pu).long(), torch.as_tensor(pi).long()
    p = omf.scores(Uw, Iw, ub, ib, pu, pi)
    loss = -torch.clamp(torch.log(p), min=-100.0).mean()
    dp = (1.0 / len(pu)) * (p - 1.0) / torch.clamp((1.0 - p) * p, min=1e-12)
    grads = omf.dense_grads(Uw, Iw, ub, ib, pu, pi, dp * (1.0 - p) * p)
    o.t += 1
    o.opt.step(o.params, grads)
    return float(loss)


def fp32_distance(snaps):
    """The largest relative distance (tensor norm) of the float32 oracle from its float64 twin over
    the steps' tables and Adam's m and v."""
    worst = 0.0
    for _, o, o64 in snaps:
        for k in range(4):
            for a, b in [(o.params[k], o64.params[k])] + [(o.opt.state[k][j], o64.opt.state[k][j]) for j in (0, 1)]:
                b = b.reshape(-1)
                worst = max(worst, float((a.double().reshape(-1) - b).norm() / b.norm()))
    return worst


WELL_CONDITIONED = 2e-6


def reference(d, n, loss):
    """(tables, pool, the two steps, MT state, per step: (loss, fp32 oracle, fp64 oracle) snapshots).

    The inputs are seeded, and a seed is taken only if the float32 oracle itself stays within
    WELL_CONDITIONED = 2e-6 (a fifth of check_step's 1e-5) of the float64 oracle: with 50 x d tables
    a single element whose gradient cancels to ~eps -- Adam's first steps turn its rounding into
    g / (|g| + eps) -- can carry the whole tensor's allowance, for any float32 arithmetic (the
    median case sits at 6e-7; the few seeds past 2e-6 are skipped for the next one)."""
    for seed in range(d + n, d + n + 8000, 1000):
        ref = reference_at(d, n, loss, seed)
        if fp32_distance(ref[5]) <= WELL_CONDITIONED:
            return ref
    raise AssertionError(f"no well-conditioned inputs for d{d} n{n} {loss}")


def reference_at(d, n, loss, seed):
    tabs, pool_u, pool_i, steps = tm.make_case(U, I, d, B, n, P, seed=seed)
    steps = [steps[0], steps[2]]            # a full batch, then B - 7 positives
    assert len(steps[0][0]) == B and len(steps[1][0]) == B - 7
    st = orng.py_seed_state(100 + seed)
    if loss == "pointwise_pos":
        pool_u, pool_i = np.zeros(1, np.int64), np.zeros(1, np.int64)
    okw = dict(loss="pointwise" if loss == "pointwise_pos" else loss, n_neg=n, batch_size=B, **KW)
    o = omf.MFOracle(*[t.clone() for t in tabs], pool_u, pool_i, st.copy(), **okw)
    o64 = omf.MFOracle(*[t.clone().double() for t in tabs], pool_u, pool_i, st.copy(), **okw)
    snaps = []
    for pu, pi in steps:
        if loss == "pointwise_pos":
            ref = positives_only_step(o, pu, pi)
            positives_only_step(o64, pu, pi)
        else:
            ref = o.step(pu, pi)
            o64.step(pu, pi)
        snaps.append((ref, copy.deepcopy(o), copy.deepcopy(o64)))
    return tabs, pool_u, pool_i, steps, st, snaps


@pytest.mark.parametrize("d", [16, 32, 64, 128, 160])
def test_pairs_one_lane_per_pair(dev, d):
    from recommendation_gans_amd.mf_engine import MFEngine
    shares = tm.Shares()
    for n in NEGS:
        for loss in LOSSES:
            tabs, pool_u, pool_i, steps, st, snaps = reference(d, n, loss)
            for plan in (False, True):
                e = MFEngine(tabs[0], tabs[1], tabs[2].reshape(-1), tabs[3].reshape(-1), pool_u, pool_i, st.copy(),
                             loss=loss, n_neg=n, batch_size=B, device=dev, **KW)
                tag = f"{loss}/d{d}/n{n}{'/plan' if plan else ''}"
                val = None
                if not plan:
                    # the validation pass (kLossOnly; adaptive: kAdaptFwd + kAdaptLoss) on the draw and
                    # the tables of step 0: the same terms summed in the same order as the training
                    # step's forward, so the same float
                    du, di = (torch.from_numpy(x).to(dev) for x in steps[0])
                    val = float(e.val_loss(du, di)[0])
                    e.set_mt_state(st.copy())
                for s, (pu, pi) in enumerate(steps):
                    du, di = torch.from_numpy(pu).to(dev), torch.from_numpy(pi).to(dev)
                    got = e.train_step(du, di, plan=e.make_plan(di) if plan else None)
                    torch.cuda.synchronize()
                    ref, o, o64 = snaps[s]
                    if s == 0 and val is not None:
                        assert val == float(got[0]), f"{tag}: validation loss {val!r}, step forward {float(got[0])!r}"
                    tm.check_step(f"{tag}/step{s}", "adam", got[0], e.params(), e.m, e.v, o, o64, ref, shares)
                    if loss != "pointwise_pos":
                        assert (e.mt_state() == o.state).all(), tag + " MT state"
                assert int(e.row_count.abs().sum()) == 0, tag
                assert float(e.hot_grad.abs().sum()) == 0.0, tag
    print(f"\npair lanes d{d}: {shares}")
