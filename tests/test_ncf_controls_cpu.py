"""Negative controls for the acceptance rule of the NCF / NeuMF parity tests: at the shapes those
tests use, oracle.mf.tensor_parity(got, ref32, ref64, before=...) with its defaults must reject a
step that is realistically wrong, and accept the same step summed in another fp32 order.

The fp32 and fp64 oracles (oracle/ncf.py) run two steps with shared masks; a mutated fp32 oracle
with ONE defect runs the same two steps from the same init and is judged as an engine would be.
A defect counts as rejected when some parameter fails the rule at step 0 or step 1.

A defect the rule accepts is kept as a strict xfail with the measured distances.  There is one:
plain SGD without its weight-decay term at weight_decay = 1e-5, lr = 1e-2 moves a tensor by
lr * wd = 1e-7 of its norm per step, a hundred times below the rule's 1e-5 relative, so two steps
cannot show it.  The same omission at weight_decay = 0.05 (5e-4 of the norm per step) is
rejected, which is why tests/test_ncf_matrix_gpu.py also runs its SGD cases at that decay."""
import numpy as np
import pytest
import torch

from oracle import mf as omf
from oracle import ncf as oncf
from oracle import rng as orng
from tests import ncf_common as nc

U, I, B, N_NEG = 300, 200, 300, 5


class Mutant(oncf.NCFOracle):
    """NCFOracle with one defect (``defect``):
    drop_example  the first positive's dL/dp is dropped from the backward pass
    lrelu         LeakyReLU slope 0.11 instead of 0.1 (forward and backward)
    drop_scale    hidden unit 3 of the first layer scales kept activations by 1.9 instead of 2
    step_count    the optimizer's step count starts one ahead (Adam's bias correction)
    no_wd         the weight-decay term is omitted
    rms_alpha     RMSprop with alpha 0.9 instead of 0.99"""

    def __init__(self, *a, defect, **k):
        if defect == "rms_alpha":
            k["alpha"] = 0.9
        super().__init__(*a, **k)
        self.defect, self._calls = defect, 0
        if defect == "step_count":
            self.opt.t = 1
        if defect == "no_wd":
            self.opt.wd = 0.0

    def _bwd(self, P, u, i, masks, cache, dp, xperm=None):
        self._calls += 1
        if self.defect == "drop_example" and self._calls % 2 == 1:      # the positives' call
            dp = dp.clone()
            dp[0] = 0
        return oncf.backward(P, u, i, masks, cache, dp, xperm)

    def step(self, pu, pi, mp, mn):
        if self.defect == "drop_scale":
            def scaled(ms):
                m0 = ms[0].float()
                m0[:, 3] *= 1.9 / oncf.DROP_SCALE
                return [m0] + list(ms[1:])
            mp, mn = scaled(mp), scaled(mn)
        slope = oncf.LRELU
        try:
            if self.defect == "lrelu":
                oncf.LRELU = 0.11
            return super().step(pu, pi, mp, mn)
        finally:
            oncf.LRELU = slope


def _run(E, loss, optimizer, make_other, wd=1e-5):
    """Two steps of o32 / o64 and of ``make_other(tensors, names, pool_u, pool_i, mt, **kw)``; per
    step the (name, ok, message, ratio) of every parameter of the other run."""
    t, names = nc.make_params(U, I, E, 0, seed=E)
    rs = np.random.RandomState(E + len(loss))
    pool_u, pool_i = rs.randint(0, U, 20000), rs.randint(0, I, 20000)
    mt = orng.py_seed_state(7)
    kw = dict(loss=loss, lr=1e-2, weight_decay=wd, n_neg=N_NEG, batch_size=B, optimizer=optimizer)
    o32 = oncf.NCFOracle([x.clone() for x in t], names, pool_u, pool_i, mt.copy(), **kw)
    o64 = oncf.NCFOracle([x.double() for x in t], names, pool_u, pool_i, mt.copy(), **kw)
    other = make_other([x.clone() for x in t], names, pool_u, pool_i, mt.copy(), **kw)
    units = sum(oncf.layer_sizes(E)[1:])
    out = []
    for s in range(2):
        pu, pi = nc.zipf_batch(rs, U, I, B)
        mp = nc.split_units((rs.rand(B, units) >= 0.5).astype(np.uint8), E)
        mn = nc.split_units((rs.rand(N_NEG * B, units) >= 0.5).astype(np.uint8), E)
        before = [x.clone() for x in o32.P.t]
        l32 = o32.step(pu, pi, mp, mn)
        o64.step(pu, pi, mp, mn)
        lo = other.step(pu, pi, mp, mn)
        assert (other.state == o32.state).all()
        rows = []
        for nm, p, r32, r64, b0 in zip(names, other.P.t, o32.P.t, o64.P.t, before):
            ok, msg = omf.tensor_parity(p, r32, r64, before=b0)
            rows.append((nm, ok, msg, nc.parity_ratio(p, r32, r64, before=b0)))
        out.append((rows, lo, l32))
    return out


_SGD_BLIND = ("tensor_parity accepts SGD without weight decay at wd = 1e-5, lr = 1e-2 (lr * wd = 1e-7 per step against "
              "the rule's 1e-5): no parameter rejected in two steps; measured worst ||mutant - ref32|| / (1e-5 "
              "||ref32||) = 0.027 (E=64 pointwise), 0.021 (E=64 bpr), 0.022 (E=16 pointwise), 0.021 (E=16 bpr)")
DEFECTS = [(d, o, 1e-5) for o in ("adam", "rms", "sgd") for d in ("drop_example", "lrelu", "drop_scale")]
DEFECTS += [("step_count", "adam", 1e-5), ("no_wd", "adam", 1e-5), ("no_wd", "rms", 1e-5), ("rms_alpha", "rms", 1e-5),
            ("no_wd", "sgd", 0.05),
            pytest.param("no_wd", "sgd", 1e-5, marks=pytest.mark.xfail(strict=True, reason=_SGD_BLIND))]


@pytest.mark.parametrize("defect,optimizer,wd", DEFECTS)
@pytest.mark.parametrize("loss", ["pointwise", "bpr"])
@pytest.mark.parametrize("E", [64, 16])
def test_tensor_parity_rejects_the_defect(E, loss, defect, optimizer, wd):
    out = _run(E, loss, optimizer, lambda *a, **k: Mutant(*a, defect=defect, **k), wd=wd)
    rejected = [(s, nm, msg) for s, (rows, _, _) in enumerate(out) for nm, ok, msg, _ in rows if not ok]
    worst = max(r for rows, _, _ in out for _, _, _, r in rows)
    first = f"first at step {rejected[0][0]} {rejected[0][1]} ({rejected[0][2]})" if rejected else "never"
    print(f"E={E} {loss} {optimizer} wd={wd:g} {defect}: {len(rejected)} rejections, {first}; worst parity ratio {worst:.3g}; "
          f"losses mutant / oracle {[(round(lo, 7), round(l32, 7)) for _, lo, l32 in out]}")
    assert rejected, f"{defect} under {optimizer} accepted on every parameter: worst parity ratio {worst:.3g}"


@pytest.mark.parametrize("optimizer", ["adam", "sgd", "rms"])
@pytest.mark.parametrize("E", [64, 16])
def test_tensor_parity_accepts_another_summation_order(E, optimizer):
    """The unmutated fp32 step over the examples, the input features and every hidden layer's
    units in seeded orders (order_seed: pointwise only) passes on every parameter."""
    out = _run(E, "pointwise", optimizer, lambda *a, **k: oncf.NCFOracle(*a, order_seed=5, **k))
    for s, (rows, lo, l32) in enumerate(out):
        assert abs(lo - l32) <= 1e-5 * abs(l32), (s, lo, l32)
        for nm, ok, msg, _ in rows:
            assert ok, f"E={E} {optimizer} step {s} {nm}: {msg}"
    print(f"E={E} {optimizer} reordered fp32 step: worst parity ratio {max(r for rows, _, _ in out for *_, r in rows):.3g}")
