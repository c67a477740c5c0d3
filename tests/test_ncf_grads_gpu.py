"""The NCF / NeuMF training kernels' data gradients (NCFEngine.grads: rg_ncf_pairs, then
rg_ncf_mlp_grad and rg_ncf_grads with gmf 1 and 0) against the float64 oracle, element by element,
by the rule of tests/ncf_grad_common.py: |g - g64| <= C_RULE * T + FWD_BAND * F + K + q, no element exempted.

Every case is teacher-forced over three steps: before each step the engine takes the fp32
oracle's current parameters (which step with Adam, so the operands move), plan and no plan
alternate by step, and random 0/1 dropout masks go to both sides (the device-dropout cases: the
engine draws its own, the oracle gets the host restatement's).  Per step: every element of every
gradient tensor by the rule (the worst share per tensor is printed), the loss slot within 1e-5 of
the fp32 oracle's, the row slots as NCFEngine.grads documents them, the MT state bit-equal, the
per-row counts and the overflow accumulators zero.

The cases (ncf_grad_common.CASES; tests/test_ncf_grads_cpu.py runs the oracle side of each on the
CPU first): every loss on the wave kernel, the tile kernel and NeuMF, the other tile widths and
the GMF layouts under pointwise and bpr, batch sizes around the tile's column count, a partial
last batch with the full draw (hinge and bpr held to the documented pairing, as
tests/test_ncf_matrix_gpu.py explains), device dropout."""
import numpy as np
import pytest
import torch

from tests import ncf_common as nc
from tests import ncf_grad_common as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def make_engine(run, optimizer="adam", seed=None):
    from recommendation_gans_amd.ncf_engine import NCFEngine
    c, t = run.case, run.t
    ne = 4 if c.M else 2
    extra = dict(mf_user_w=t[2], mf_item_w=t[3]) if c.M else {}
    return NCFEngine(t[0], t[1], t[ne:], run.pool_u, run.pool_i, run.mt.copy(), loss=c.loss, optimizer=optimizer,
                     lr=1e-2, weight_decay=1e-5, n_neg=c.n, batch_size=c.B, device=torch.device(DEV),
                     seed=(c.drop_seed or 0) if seed is None else seed, **extra)


def expected_slots(case, st, planned):
    """min(examples that claimed a list slot of the row, RG_MF_LIST_CAP): every valid example for a
    user row, every valid one but the planned positives for an item row (a pairwise loss leaves the
    negatives of the columns past n_pos out)."""
    from recommendation_gans_amd._lib import RG_MF_LIST_CAP
    k = len(st.pu)
    nu, ni = st.out64["neg_u"].view(case.n, case.B), st.out64["neg_i"].view(case.n, case.B)
    if case.loss in ("bpr", "hinge"):
        nu, ni = nu[:, :k], ni[:, :k]
    u = torch.cat([torch.from_numpy(st.pu).long(), nu.reshape(-1)])
    i = ni.reshape(-1) if planned else torch.cat([torch.from_numpy(st.pi).long(), ni.reshape(-1)])
    cnt = torch.cat([torch.bincount(u, minlength=case.U), torch.bincount(i, minlength=case.I)])
    return cnt.clamp(max=RG_MF_LIST_CAP).float()


@pytest.mark.parametrize("case", gc.CASES, ids=[c.id for c in gc.CASES])
def test_ncf_gradients_elementwise(case):
    run = gc.run_oracles(case, restate=False)
    for why in run.reseeded:
        print(f"{case.id}: reseeded, {why}")
    case = run.case
    e = make_engine(run)
    assert e.tc == gc.tile_cols(case.n, case.E, case.M)
    dev = torch.device(DEV)
    fam = gc.families(case.E, case.M)
    worst = {}
    shapes = [tuple(x.shape) for x in run.t]
    for s, st in enumerate(run.steps):
        e.set_params(st.params)
        pu_d, pi_d = torch.from_numpy(st.pu).to(dev), torch.from_numpy(st.pi).to(dev)
        planned = s % 2 == 1
        plan = e.make_plan(pi_d) if planned else None
        masks = None if case.drop_seed is not None else (nc.pad_masks(st.mp, case.B, dev),
                                                         nc.pad_masks(st.mn, case.n * case.B, dev))
        emb, gmf, mlp = e.grads(pu_d, pi_d, plan=plan, masks=masks)
        torch.cuda.synchronize()
        got, slots, gslots, loss = gc.split_engine_grads(case, emb, gmf, mlp, shapes)
        sh = gc.shares(got, st)
        line = []
        for k, name in enumerate(run.names):
            w = float(sh[k].max())
            worst[fam[k]] = max(worst.get(fam[k], 0.0), w)
            line.append(f"{name} {w:.3g}")
        print(f"{case.id} step {s} plan={planned}: worst share per tensor: " + ", ".join(line))
        for k in range(len(got)):
            assert float(sh[k].max()) <= 1.0, f"{case.id} step {s} plan={planned} " + gc.describe_failure(run.names, sh, k)
        l32 = st.out32["loss"]
        assert abs(loss - l32) <= 1e-5 * abs(l32), (case.id, s, loss, l32)
        want = expected_slots(case, st, planned)
        assert torch.equal(slots[:-1], want) and float(slots[-1]) == 0.0, f"{case.id} step {s}: row slots"
        if gslots is not None:
            assert torch.equal(gslots[:-1], want) and float(gslots[-1]) == 0.0, f"{case.id} step {s}: GMF row slots"
        assert (e.mt_state() == st.mt_after).all(), f"{case.id}: MT state after step {s}"
        assert int(e.row_count.abs().sum()) == 0 and int(e.hot_grad.abs().sum()) == 0
        if case.M:
            assert int(e.mf_hot_grad.abs().sum()) == 0
    print(f"{case.id}: worst share of the rule per family {({k: float(f'{v:.3g}') for k, v in worst.items()})}")


def test_ncf_grads_then_train_step_equals_an_lr0_step():
    """grads() followed by train_step on the next batch equals, bit for bit, a second engine that
    took an lr = 0 step in its place: the MT state, the next step's loss and every parameter.  SGD
    (an lr = 0 step leaves no optimizer state behind) with device dropout, whose seed follows the
    step count, on NeuMF with a plan on the second step."""
    case = gc._case("then-step", 16, 20, "bpr", 5, 300, 60, 25, drop_seed=31)
    run = gc.run_oracles(case, restate=False, steps=2)
    dev = torch.device(DEV)
    a, b = make_engine(run, "sgd"), make_engine(run, "sgd")
    st0, st1 = run.steps
    d = lambda x: torch.from_numpy(x).to(dev)
    a.grads(d(st0.pu), d(st0.pi))
    opt_of = b._opt

    def lr0(t):
        o = opt_of(t)
        o.lr = 0.0
        o.step_size = 0.0
        return o
    b._opt = lr0
    b.train_step(d(st0.pu), d(st0.pi))
    b._opt = opt_of
    torch.cuda.synchronize()
    for pa, pb, p0 in zip(a.params(), b.params(), run.t):
        assert torch.equal(pa, pb) and torch.equal(pa.cpu().reshape(p0.shape), p0)
    assert (a.mt_state() == b.mt_state()).all() and a.t == b.t == 1
    pi1 = d(st1.pi)
    la = float(a.train_step(d(st1.pu), pi1, plan=a.make_plan(pi1))[0])
    lb = float(b.train_step(d(st1.pu), pi1, plan=b.make_plan(pi1))[0])
    torch.cuda.synchronize()
    assert la == lb and np.isfinite(la)
    assert (a.mt_state() == b.mt_state()).all()
    moved = False
    for pa, pb, p0 in zip(a.params(), b.params(), run.t):
        assert torch.equal(pa, pb)
        moved |= not torch.equal(pa.cpu().reshape(p0.shape), p0)
    assert moved
    assert int(a.row_count.abs().sum()) == 0 and int(a.hot_grad.abs().sum()) == 0 and int(a.mf_hot_grad.abs().sum()) == 0
