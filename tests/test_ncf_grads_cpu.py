"""The elementwise gradient rule of tests/ncf_grad_common.py on the CPU, before a GPU sees it:

* the fp32 step and the two reordered ones pass the rule on every case of
  tests/test_ncf_grads_gpu.py with a worst share of at most 1/3 of the whole rule, so the GPU test
  cannot fail on rounding alone.  The kink-flipped step is held to (c T + FWD_BAND F + q) / 3 + K: it takes
  every decision inside the band the other way, so an element that one such decision feeds moves
  by exactly the K that decision contributes and no fraction of K could hold it;
* the preconditions of the non-smooth losses hold on every step of every case; a reseeded case
  prints the seeds it left and why;
* FWD_BAND is three times the measured maximum, rounded up to one significant digit;
* negative controls in the style of tests/test_ncf_controls_cpu.py: a mutated fp32 oracle
  gradient with ONE defect is rejected by the rule on a tensor the defect touches.  A defect the
  rule accepts would be kept as a strict xfail with its measured share; every one is rejected.

Run with ``-s`` for the per-family calibration table (profiles/ncf_grads/cpu_calibration.log)."""
import functools
import pathlib
import re

import numpy as np
import pytest
import torch

from oracle import ncf as oncf
from tests import ncf_common as nc
from tests import ncf_grad_common as gc


@functools.lru_cache(maxsize=None)
def oracle_run(k):
    return gc.run_oracles(gc.CASES[k])


IDS = [c.id for c in gc.CASES]


def test_kink_c_is_the_configured_one():
    src = (pathlib.Path(__file__).parent / "test_configs_gpu.py").read_text()
    assert float(re.search(r"^KINK_C = ([0-9.]+)", src, re.M).group(1)) == gc.KINK_C


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("k", range(len(gc.CASES)), ids=IDS)
def test_fp32_restatements_pass_the_rule(k):
    run = oracle_run(k)
    worst = flip = 0.0
    for s, st in enumerate(run.steps):
        bad = gc.hinge_precondition(run.case.loss, st.out64, run.case.n, run.case.B)
        assert bad is None, f"{run.case.id} step {s}: {bad}"
        for nm, g in [("fp32", st.out32["grads"])] + list(st.restated.items()):
            if nm == "kinkflip":
                ws = gc.worst_shares(g, st, rounding=1.0 / 3.0)
                flip = max(flip, max(ws))
                for name, w in zip(run.names, ws):
                    assert w <= 1.0, f"{run.case.id} step {s} {nm} {name}: {w:.3g} of (c T + FWD_BAND F + q) / 3 + K"
            else:
                ws = gc.worst_shares(g, st)
                worst = max(worst, max(ws))
                for name, w in zip(run.names, ws):
                    assert w <= 1.0 / 3.0, f"{run.case.id} step {s} {nm} {name}: share {w:.3g} of the rule"
    for why in run.reseeded:
        print(f"{run.case.id}: reseeded, {why}")
    print(f"{run.case.id} (seed {run.case.seed}): worst share of the whole rule, fp32 and reordered steps: {worst:.3g}; "
          f"kink-flipped step against (c T + FWD_BAND F + q) / 3 + K: {flip:.3g}")


def test_forward_band_is_three_times_the_measured_maximum():
    per = {f: (0.0, "") for f in gc.FAMILIES}
    plain = {f: (0.0, "") for f in gc.FAMILIES}
    for k, case in enumerate(gc.CASES):
        run = oracle_run(k)
        fam = gc.families(case.E, case.M)
        for s, st in enumerate(run.steps):
            for nm, g in [("fp32", st.out32["grads"])] + list(st.restated.items()):
                for f, x, y in zip(fam, gc.calibration_ratio(g, st), gc.plain_ratio(g, st)):
                    if y > plain[f][0]:
                        plain[f] = (y, f"{case.id} step {s} {nm}")
                    if x > per[f][0]:
                        per[f] = (x, f"{case.id} step {s} {nm}")
    print("\nfp32 restatements against float64 over the elements with K = 0, per kernel family:")
    for f in gc.FAMILIES:
        print(f"  {f:11s} max (|g - g64| - C_RULE / 3 T)+ / F = {per[f][0]:.3g}   ({per[f][1]})")
    for f in gc.FAMILIES:
        print(f"  {f:11s} max |g - g64| / T (what T alone would need) = {plain[f][0]:.3e}   ({plain[f][1]})")
    top = max(v for v, _ in per.values())
    band = gc.round_up_1sig(3.0 * top)
    print(f"  FWD_BAND = 3 * {top:.3g} = {3 * top:.3g} -> {band:g}; C_RULE = {gc.C_RULE:g} (derived)")
    assert abs(gc.FWD_BAND - band) <= 1e-9 * band, (gc.FWD_BAND, band)


# ----------------------------------------------------------------------------- negative controls
DEFECTS = {  # name: needs NeuMF
    "user_term_missing": False, "overflow_twice": False, "item_last_feature_zero": False, "lrelu": False,
    "drop_scale": False, "gmf_shifted_weight": True, "gmf_own_partner": True, "bias_missing_example": False}


def _slice_cache(cache, idx):
    out = {}
    for key, v in cache.items():
        if torch.is_tensor(v):
            out[key] = v[idx]
        elif isinstance(v, list):
            out[key] = [x[idx] for x in v]
        elif isinstance(v, dict):
            out[key] = {a: x[idx] for a, x in v.items()}
        else:
            out[key] = v
    return out


def mutant(base):
    """``base`` (NCFOracle / NeuMFOracle) with one defect in its data gradient (``defect``):
    user_term_missing     the first positive's term is missing from its user's MLP row
    overflow_twice        the terms past the first RG_MF_LIST_CAP = 8 of the positives' most
                          frequent user are counted twice in that row (the overflow accumulator)
    item_last_feature_zero  the last feature of the first positive's item row is 0
    lrelu                 LeakyReLU slope 0.11 (forward and backward)
    drop_scale            hidden unit 3 of the first layer scales kept activations by 1.9
    gmf_shifted_weight    the GMF gradient of column c takes w_aff[8 + c + 1]
    gmf_own_partner       the GMF user rows take the user's own row as the partner
    bias_missing_example  the last hidden layer's bias gradient misses the first positive"""
    fn = oncf.neumf_backward if base.N_EMB == 4 else oncf.backward

    class Mutant(base):
        def __init__(self, *a, defect, **k):
            super().__init__(*a, **k)
            self.defect, self._calls, self.touched = defect, 0, None

        def _bwd(self, P, u, i, masks, cache, dp, xperm=None):
            self._calls += 1
            out = fn(P, u, i, masks, cache, dp, xperm)
            if self._calls % 2 == 0:              # the negatives' call
                return out
            d, ne = self.defect, self.N_EMB

            def part(idx):
                idx = torch.as_tensor(idx).long()
                return fn(P, u[idx], i[idx], [m[idx] for m in masks], _slice_cache(cache, idx), dp[idx], xperm)
            if d == "user_term_missing":
                out[0][u[0]] -= part([0])[0][u[0]]
                self.touched = [0]
            elif d == "overflow_twice":
                hot = int(torch.bincount(u).argmax())
                idx = (u == hot).nonzero().flatten()
                assert len(idx) > 8
                out[0][hot] += part(idx[8:])[0][hot]
                self.touched = [0]
            elif d == "item_last_feature_zero":
                self.zero_item = int(i[0])
                self.touched = [1]
            elif d == "bias_missing_example":
                k = len(out) - 3
                out[k] = out[k] - part([0])[k]
                self.touched = [k]
            elif d in ("gmf_shifted_weight", "gmf_own_partner"):
                p = cache["p"]
                dz = dp * (1 - p) * p
                W = P.linears()[-1][0]
                wm = W[:, 8:]
                if d == "gmf_shifted_weight":
                    wm = torch.roll(wm, -1, 1)
                dg = dz.mm(wm)
                out[2] = torch.zeros_like(out[2]).index_add_(
                    0, u, dg * (cache["gmf_u"] if d == "gmf_own_partner" else cache["gmf_i"]))
                self.touched = [2]
                if d == "gmf_shifted_weight":
                    out[3] = torch.zeros_like(out[3]).index_add_(0, i, dg * cache["gmf_u"])
                    self.touched = [2, 3]
            return out

        def step(self, pu, pi, mp, mn, return_all=False):
            if self.defect == "drop_scale":
                def scaled(ms):
                    m0 = ms[0].float()
                    m0[:, 3] *= 1.9 / oncf.DROP_SCALE
                    return [m0] + list(ms[1:])
                mp, mn = scaled(mp), scaled(mn)
                self.touched = [self.N_EMB]                      # layers.0.weight, row 3
            slope = oncf.LRELU
            try:
                if self.defect == "lrelu":
                    oncf.LRELU = 0.11
                    self.touched = list(range(len(self.P.t) - 2))   # everything below a hidden layer
                out = super().step(pu, pi, mp, mn, return_all=True)
            finally:
                oncf.LRELU = slope
            if self.defect == "item_last_feature_zero":
                out["grads"][1][self.zero_item, -1] = 0
            return out
    return Mutant


CONTROL = dict(n=5, B=300, U=60, I=25)


@functools.lru_cache(maxsize=None)
def control_run(E, M, loss):
    case = gc._case("control", E, M, loss, **CONTROL)
    return gc.run_oracles(case, restate=False, steps=1)


def _control_cases():
    out = []
    for E in (64, 16):
        for M in (0, 5):
            for loss in ("pointwise", "bpr"):
                for d, needs in DEFECTS.items():
                    if needs and not M:
                        continue
                    out.append(pytest.param(E, M, loss, d, marks=XFAIL.get((E, M, loss, d), ())))
    return out


# Defects the rule accepts would be listed here with the measured worst share on the touched tensors
# and run as strict xfails (as tests/test_ncf_controls_cpu.py keeps its one).  There is none: the
# narrowest rejection of the 56 is 19.8 times the rule (one example missing from a bias, E = 16,
# pointwise); one term missing from a user row is rejected by 28 to 570 times.
ACCEPTED = {}
XFAIL = {k: pytest.mark.xfail(strict=True, reason=f"the rule accepts it: worst share {v} on the touched tensors")
         for k, v in ACCEPTED.items()}


@pytest.mark.parametrize("E,M,loss,defect", _control_cases())
def test_rule_rejects_the_defect(E, M, loss, defect):
    run = control_run(E, M, loss)
    st = run.steps[0]
    m = gc.make_oracle(run.case, run.t, run.names, run.pool_u, run.pool_i, run.mt, torch.float32,
                       cls=mutant(nc.oracle_for(M)), defect=defect)
    gc.force(m, st.params)
    got = m.step(st.pu, st.pi, nc.split_units(st.mp, E), nc.split_units(st.mn, E))["grads"]
    ws = gc.worst_shares(got, st)
    clean = gc.worst_shares(st.out32["grads"], st)
    assert max(clean) <= 1.0 / 3.0
    touched = {run.names[k]: ws[k] for k in m.touched}
    print(f"E={E} M={M} {loss} {defect}: shares on the touched tensors {({k: round(v, 3) for k, v in touched.items()})}, "
          f"unmutated worst {max(clean):.3g}")
    assert max(touched.values()) > 1.0, f"{defect} accepted: worst share {max(touched.values()):.3g} on {list(touched)}"
