"""The elementwise acceptance rule for the NCF / NeuMF data gradients and the cases it is run on
(test_ncf_grads_cpu.py, test_ncf_grads_gpu.py).  No test lives here and nothing here needs a GPU.

The rule.  An element g of a gradient tensor (NCFEngine.grads: the MLP tables' rows, the GMF
tables' rows, every MLP weight and bias) passes iff

    |g - g64| <= C_RULE * T + FWD_BAND * F + K + q

with g64 the float64 oracle's gradient of the same step from the same fp32 operands, and

* T   oracle.ncf.grad_terms: per element, the sum over the examples of the absolute value of
      every term of that element's sum (|dz| at the output pushed down through |W|, |a_prev|, the
      masks times 2 and the LeakyReLU slopes; GMF rows |dz| |w_aff[8 + c]| |partner row|) -- the
      scale on which the summation of the gradient itself errs in fp32;
* F   oracle.ncf.forward_error_terms: one standard error of the forward pass's rounding carried
      into the gradient to first order.  A pre-activation of K inputs gets the variance
      u^2 (K + 1) (sum of its squared terms) plus its inputs' variances through W^2 (independent
      roundings add in quadrature, as they do through signed weights); an activation that times
      its squared slope and mask; a score p^2 (1 - p)^2 of its logit's plus (u p)^2, the rounding
      of p itself, which is what fp32 loses of (1 - p) near 1; dz = dp (1 - p) p the standard
      error |dp| sp + (1 - p) p sdp (pointwise sdp = sp / p^2, sp / (1 - p)^2; bpr 0.1 g per score
      of the pair); a sum of dz * a gains vdz a^2 + dz^2 va per example, and examples add in
      quadrature.  T takes |a_prev| and |dz| at their computed values, so an element whose single
      term has an activation that cancelled to a few roundings, or whose example's score
      saturated, has an fp32 error no multiple of T describes; F is the size of that error;
* K   the kink envelope before the optimizer (NCFOracle.kink_grad_env at c = KINK_C, the value
      tests/test_configs_gpu.py uses): how far flipping any LeakyReLU decision within fp32
      rounding of the kink moves the element;
* q   the overflow accumulators' fixed-point quantum times the number of terms of the element.
      rg_common.h: to_fix(v) = round(v * 2^48) (kFixScale = 2^48, __double2ll_rn), and a row that
      overflowed its list sums ALL of its contributions that way -- the surplus where the pair kernel
      writes hot_grad / mf_hot_grad (fix_add), the listed ones in the pull (rg_mf_kernels.h
      gf += to_fix(dz * o)).  Each term is off by at most half a quantum, 2^-49; q = 2^-48 *
      (examples of the step that touch the row) bounds the sum with a factor two to spare (the
      final from_fix rounding to fp32 is relative to the sum and sits in C_RULE * T).  It applies
      to every row of the embedding and GMF tables (a row within its list has a smaller error
      than this bound) and is 0 for the MLP tensors, which never go through fixed point.

No element is exempted: an untouched row has T = F = K = q = 0 and must be exactly 0.

The two constants.  C_RULE = 1e-5 is derived, and it is the constant of the MF twin
(tests/test_mf_gpu.py check_grads): C_RULE * T covers the gradient sums' own rounding, n terms
summed in some fp32 order erring by about (2 sqrt(n) + 4) u of their sum of absolute values
(oracle.mf NOISE_C1, NOISE_C0), 6.4e-6 at the longest sum of the cases (2700 examples into one
MLP element).  FWD_BAND is measured as the issue prescribes for a constant of this rule: over
every case of the GPU file (CASES), the fp32 oracle, its reordered restatements (order_seed 5 and
11) and its kink_flip = KINK_C restatement are held against the float64 oracle, and the largest
(|g - g64| - C_RULE / 3 * T)+ / F over the elements with K = 0 is taken; FWD_BAND is three times
it (the project's ``band``, the margin over one sample of fp32 rounding) rounded up to one
significant digit.  Measured (tests/test_ncf_grads_cpu.py prints the table with the case behind
every figure; profiles/ncf_grads/cpu_calibration.log):

    wave (E = 64 tower: MLP tables and MLP tensors)      2.2
    tile (E in {8, 16, 32} and NeuMF towers)             3.1
    GMF vector layouts (M in {64, 128})                  0.0014  (C_RULE / 3 * T nearly covers it)
    GMF scalar layouts (M in {5, 20, 24, 50, 65, 100})   0.85

    FWD_BAND = 3 * 3.06 -> 10

The two towers and the scalar GMF rows agree within a factor of four, which is what says F has
the right shape at every width and depth.  A rule of T alone, as a first version of this file had, needs
max |g - g64| / T = 0.16 on the wave tower's tensors and 0.049 on the tile tower's (the table
prints the cases), a constant that rejects nothing; and a worst-case F (bands through |W|) sits
300 times above the fp32 oracle's own distance at E = 64.  The calibration test fails when a
change of the cases moves the measured maximum so that FWD_BAND is no longer three times it
rounded up.  Taking a third of C_RULE * T out makes every fp32 restatement use at most a third of
the rule where K = 0.

Preconditions (``hinge_precondition``) are the two of the non-smooth losses.  A seed that violates
one is replaced by the next (seed + 1000), never skipped, and the Run records which seeds were
left and why (``reseeded``; both test files print it).  Saturated scores are not excluded.

What the tensor-norm rule (oracle.mf.tensor_parity) cannot see and this one can: a defect
confined to a few table rows -- a lost overflow term, a row tail, one wrong column -- moves the
norm of a table by far less than 1e-5 of it under SGD or a warmed-up RMSprop, and no small MLP
tensor witnesses it (tests/test_ncf_grads_cpu.py: the negative controls, all rejected)."""
import collections
import functools
import math

import numpy as np
import torch

from oracle import ncf as oncf
from oracle import rng as orng
from tests import ncf_common as nc
from tests.mf_layout_common import layout_of

KINK_C = 4.0                      # tests/test_configs_gpu.py KINK_C
FIX_QUANTUM = 2.0 ** -48          # rg_common.h kFixScale = 2^48
C_RULE = 1e-5
FWD_BAND = 10.0                   # multiples of the forward pass's standard error (see the docstring)
ORDER_SEEDS = (5, 11)
STEPS = 3
FAMILIES = ("wave", "tile", "gmf-vector", "gmf-scalar")
LOSSES = ("pointwise", "bpr", "hinge", "adaptive_hinge")

Case = collections.namedtuple("Case", "id E M loss n B U I n_pos drop_seed seed")


def _case(group, E, M, loss, n, B, U, I, n_pos=None, drop_seed=None, extra=""):
    cid = f"{group}-E{E}-M{M}-{loss}-n{n}-B{B}{extra}"
    return Case(cid, E, M, loss, n, B, U, I, n_pos, drop_seed, seed=E + M + n + B)


def tile_cols(n, E, M):
    """rg_ncf_cols_per_tile restated (rows per tile // (1 + n): 48 rows for the E = 64 tower's wave
    kernel, 32 otherwise); the GPU file asserts it against the library."""
    return (48 if E == 64 and M == 0 else 32) // (1 + n)


def _cases():
    out = []
    ns = (1, 3, 5, 8)
    k = 0
    # kernel by loss: 60 x 25 tables at B = 300 (most rows overflow) or 300 x 200 (rows stay listed)
    grid = [((E, M), LOSSES) for E, M in ((64, 0), (16, 0), (8, 5), (32, 20))]
    grid += [((E, M), LOSSES[:2]) for E, M in ((8, 0), (32, 0), (16, 50), (64, 64), (32, 128))]
    grid += [((E, M), LOSSES[:2]) for E, M in ((16, 24), (16, 100), (8, 65))]
    for (E, M), losses in grid:
        for loss in losses:
            U, I = ((60, 25), (300, 200))[k % 2]
            out.append(_case("kernel", E, M, loss, ns[(k // 2 + k) % 4], 300, U, I))
            k += 1
    # batch edges around the tile's column count at n = 5
    for E, M in ((64, 0), (16, 0), (16, 50)):
        tc = tile_cols(5, E, M)
        for tag, B in (("1", 1), ("tc-1", tc - 1), ("tc+1", tc + 1), ("3tc+2", 3 * tc + 2)):
            for loss in LOSSES[:2]:
                out.append(_case("edge", E, M, loss, 5, B, 200, 150, extra=f"({tag})"))
    # partial last batch: n_pos of 256 with the full n * 256 draw
    for E in (64, 16):
        for n_pos in (1, 219):
            for loss in LOSSES:
                out.append(_case("partial", E, 0, loss, 5, 256, 400, 300, n_pos=n_pos, extra=f"-npos{n_pos}"))
    # device dropout: the engine draws its own masks, the oracle gets the host restatement's
    out.append(_case("devdrop", 64, 0, "pointwise", 5, 300, 60, 25, drop_seed=12345))
    out.append(_case("devdrop", 16, 50, "bpr", 5, 300, 300, 200, drop_seed=977))
    return out


CASES = _cases()


def families(E, M):
    """The kernel family of every gradient tensor of an (E, M) model, in parameter order."""
    tower = "wave" if E == 64 and M == 0 else "tile"
    n_lin = len(oncf.layer_sizes(E))          # hidden Linears + the output Linear
    out = [tower, tower]
    if M:
        out += ["gmf-vector" if layout_of(M) == "float4" else "gmf-scalar"] * 2
    return out + [tower] * (2 * n_lin)


# ----------------------------------------------------------------------------- preconditions
def hinge_precondition(loss, out, n, B):
    """The non-smooth losses away from their kinks on the float64 oracle (``out`` = its
    step(return_all=True)); returns None or what is violated.  hinge: no pair's margin
    neg - pos + 1 within 1e-5 (relative to |neg| + |pos| + 1) of 0.  adaptive hinge: the top two
    negative scores differ by more than 1e-5 relative, and no positive's margin against the
    maximum is within 1e-5 of 0."""
    pp, pn = out["p_pos"].reshape(-1), out["p_neg"].reshape(-1)
    if loss == "hinge":
        negm = pn.view(n, B)[:, :len(pp)]
        x = negm - pp[None, :] + 1.0
        if bool((x.abs() <= 1e-5 * (negm.abs() + pp[None, :].abs() + 1.0)).any()):
            return "a hinge margin within 1e-5 of 0"
    if loss == "adaptive_hinge":
        top = torch.topk(pn, 2).values
        if float(top[0] - top[1]) <= 1e-5 * float(top[0].abs()):
            return "the top two negatives within 1e-5"
        x = top[0] - pp + 1.0
        if bool((x.abs() <= 1e-5 * (top[0].abs() + pp.abs() + 1.0)).any()):
            return "an adaptive-hinge margin within 1e-5 of 0"
    return None


# ----------------------------------------------------------------------------- the oracle side
Step = collections.namedtuple("Step", "params pu pi mp mn out32 out64 T F K q restated mt_after")
Run = collections.namedtuple("Run", "case t names pool_u pool_i mt steps reseeded")


def make_oracle(case, t, names, pool_u, pool_i, mt, dtype, cls=None, **kw):
    Oracle = cls or nc.oracle_for(case.M)
    return Oracle([x.to(dtype).clone() for x in t], names, pool_u, pool_i, mt.copy(), loss=case.loss, lr=1e-2,
                  weight_decay=1e-5, n_neg=case.n, batch_size=case.B, optimizer="adam", **kw)


def force(o, params):
    """Teacher forcing: the oracle's parameters <- ``params`` (its optimizer state is not used)."""
    for dst, src in zip(o.P.t, params):
        dst.copy_(src)


def row_counts(case, pu, pi, out):
    """Examples of the step that touch each user / item row (every drawn negative counted)."""
    u = torch.cat([torch.as_tensor(pu).long(), out["neg_u"]])
    i = torch.cat([torch.as_tensor(pi).long(), out["neg_i"]])
    return torch.bincount(u, minlength=case.U).double(), torch.bincount(i, minlength=case.I).double()


def quanta(case, pu, pi, out, shapes):
    cu, ci = row_counts(case, pu, pi, out)
    q = [torch.zeros(s, dtype=torch.float64) for s in shapes]
    for k in range(4 if case.M else 2):
        q[k] += FIX_QUANTUM * (cu if k % 2 == 0 else ci)[:, None]
    return q


def case_inputs(case):
    t, names = nc.make_params(case.U, case.I, case.E, case.M, case.seed)
    rs = np.random.RandomState(case.seed * 7 + case.n)
    pool_u, pool_i = rs.randint(0, case.U, 20000), rs.randint(0, case.I, 20000)
    return t, names, rs, pool_u, pool_i, orng.py_seed_state(7)


def draw_step(case, rs, s):
    """Step s's positives (Zipf: a few hot rows overflow) and 0/1 dropout masks as uint8 arrays."""
    units = sum(oncf.layer_sizes(case.E)[1:])
    k = case.B if case.n_pos is None else case.n_pos
    pu, pi = nc.zipf_batch(rs, case.U, case.I, k)
    if case.drop_seed is None:
        mp = (rs.rand(k, units) >= 0.5).astype(np.uint8)
        mn = (rs.rand(case.n * case.B, units) >= 0.5).astype(np.uint8)
    else:
        mp, mn = nc.device_masks(case.drop_seed, s + 1, units, case.B, case.n)
        mp = mp[:k]
    return pu, pi, mp, mn


def run_oracles(case, restate=True, steps=STEPS):
    """The teacher-forced oracle side of a case, a ``Run`` (the case with the seed it ended on, the
    initial parameters, the pool, the MT state at the start): per step a ``Step`` with the fp32 operands
    (``params``, which the engine and every oracle are set to), the inputs, the fp32 and float64
    oracles' step(return_all=True), T, F, K, q per tensor, and (``restate``) the gradients of the
    reordered and kink-flipped fp32 restatements as {name: [tensor, ...]}.  The fp32 oracle steps
    with Adam, so the operands move from step to step.  A seed whose draw violates a precondition
    of a non-smooth loss is replaced by the next one (``hinge_precondition``)."""
    why = []
    for bump in range(24):
        got = _run_oracles(case._replace(seed=case.seed + 1000 * bump), restate, steps)
        if not isinstance(got, str):
            return got._replace(reseeded=tuple(why))
        why.append(f"seed {case.seed + 1000 * bump}: {got}")
    raise AssertionError(f"{case.id}: no seed satisfies the loss preconditions")


def _run_oracles(case, restate, steps):
    t, names, rs, pool_u, pool_i, mt = case_inputs(case)
    mk = functools.partial(make_oracle, case, t, names, pool_u, pool_i, mt)
    o32, o64 = mk(torch.float32), mk(torch.float64, kink_env=KINK_C, grad_bounds=True)
    others = {}
    if restate:
        others = {f"order{sd}": mk(torch.float32, order_seed=sd) for sd in ORDER_SEEDS}
        others["kinkflip"] = mk(torch.float32, kink_flip=KINK_C)
    result = []
    for s in range(steps):
        pu, pi, mp, mn = draw_step(case, rs, s)
        params = [x.clone() for x in o32.P.t]
        ms = lambda: (nc.split_units(mp, case.E), nc.split_units(mn, case.E))
        for o in [o64] + list(others.values()):
            force(o, params)
        out64 = o64.step(pu, pi, *ms(), return_all=True)
        bad = hinge_precondition(case.loss, out64, case.n, case.B)
        if bad is not None:
            return f"step {s}: {bad}"
        out32 = o32.step(pu, pi, *ms(), return_all=True)
        restated = {nm: o.step(pu, pi, *ms(), return_all=True)["grads"] for nm, o in others.items()}
        for o in others.values():
            assert (o.state == o32.state).all()
        assert (o64.state == o32.state).all()
        K = [e.clone() for e in o64.kink_grad_env]
        q = quanta(case, pu, pi, out64, [g.shape for g in out64["grads"]])
        result.append(Step(params, pu, pi, mp, mn, out32, out64, out64["terms"], out64["fwd"], K, q, restated, o32.state.copy()))
    return Run(case, t, names, pool_u, pool_i, mt, result, ())


# ----------------------------------------------------------------------------- the rule
def shares(got, step, rounding=1.0):
    """Per tensor, |g - g64| / (rounding * (c T + FWD_BAND F + q) + K) elementwise (float64; an element with
    a zero bound is 0 when it is exactly right and inf otherwise).  ``rounding`` < 1 holds a
    restatement to a fraction of the rounding allowance with the kink envelope at its full size."""
    c = C_RULE
    out = []
    for g, g64, T, F, K, q in zip(got, step.out64["grads"], step.T, step.F, step.K, step.q):
        err = (torch.as_tensor(g).double().cpu().reshape(g64.shape) - g64).abs()
        bound = rounding * (c * T + FWD_BAND * F + q) + K
        sh = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, math.inf, 0.0).double())
        out.append(sh)
    return out


def worst_shares(got, step, rounding=1.0):
    return [float(sh.max()) if sh.numel() else 0.0 for sh in shares(got, step, rounding)]


def describe_failure(names, sh, k):
    """The first elements of tensor k outside the rule, as (row, column) with their shares."""
    bad = (sh[k] > 1.0).nonzero()[:8].tolist()
    return f"{names[k]}: {int((sh[k] > 1.0).sum())} elements outside the rule, first " \
           f"{[(tuple(ix), float(sh[k][tuple(ix)])) for ix in bad]}"


def calibration_ratio(got, step):
    """Per tensor, the largest (|g - g64| - C_RULE / 3 * T)+ / F over the elements with K = 0 (and
    F > 0): how many standard errors of the forward pass's rounding an fp32 restatement lies from
    float64 once a third of the summation's allowance is taken out."""
    out = []
    for g, g64, T, F, K in zip(got, step.out64["grads"], step.T, step.F, step.K):
        err = ((torch.as_tensor(g).double().reshape(g64.shape) - g64).abs() - C_RULE / 3.0 * T).clamp(min=0)
        ok = (K == 0) & (F > 0)
        out.append(float((err[ok] / F[ok]).max()) if bool(ok.any()) else 0.0)
    return out


def plain_ratio(got, step):
    """Per tensor, the largest |g - g64| / T over the elements with K = 0 and T > 0 (reported: what
    a rule of T alone would have to allow)."""
    out = []
    for g, g64, T, K in zip(got, step.out64["grads"], step.T, step.K):
        err = (torch.as_tensor(g).double().reshape(g64.shape) - g64).abs()
        ok = (K == 0) & (T > 0)
        out.append(float((err[ok] / T[ok]).max()) if bool(ok.any()) else 0.0)
    return out


def round_up_1sig(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def split_engine_grads(case, emb, gmf, mlp, shapes):
    """NCFEngine.grads' three flat buffers as the oracle's tensors in parameter order, plus
    (row slots of emb, row slots of gmf or None, loss slot)."""
    U, I, E, M = case.U, case.I, case.E, case.M
    emb, mlp = emb.detach().cpu(), mlp.detach().cpu()
    rows = U + I
    out = [emb[:U * E].view(U, E), emb[U * E:rows * E].view(I, E)]
    gslots = None
    if M:
        gmf = gmf.detach().cpu()
        out += [gmf[:U * M].view(U, M), gmf[U * M:rows * M].view(I, M)]
        gslots = gmf[rows * M:]
    o = 0
    for shp in shapes[len(out):]:
        k = int(np.prod(shp))
        out.append(mlp[o:o + k].view(shp))
        o += k
    assert o + 1 == mlp.numel()
    return out, emb[rows * E:], gslots, float(mlp[-1])
