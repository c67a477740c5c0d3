"""What the fold-in tests share (no tests here): the case builder, the float64 CPU reference
(``mf_engine.fold_in_users_torch`` on float64 copies), and an independent numpy restatement of the
objective in include/rg_hip.h (rg_mf_fold_in_users) with hand-written gradients, which pins the
reference in float64 and, run in float32 with three summation orders, measures the error a float32
evaluation of the same formulas has (``E32``).

The cases cover every row layout the kernel is instantiated for (rg_common.h dispatch_dim; LPU
lanes x EPL elements per lane), by dim:
    8 / 16 / 32 / 64 / 128 / 256   the 16-byte layouts of 2 / 4 / 8 / 16 / 32 / 64 lanes x 4
    1, 3                           scalar, 16 lanes x 1        24         scalar, 16 lanes x 2
    48                             scalar, 16 lanes x 4        65, 96     scalar, 64 lanes x 2
    160                            scalar, 64 lanes x 3        200        scalar, 64 lanes x 4
with users {1, 5, 130}, history lengths {0, 1, 2, 63, 64, 65, 200} mixed in one call, n_neg {0, 1,
3, 5} (5 is past the kernel's chunk of 4 negatives, the odd lengths past its block of 2 positives),
steps {1, 2, 8}, the four losses, weight decay {0, 1e-3} and zero / random starts -- a covering
list, not the product.  Chosen before any GPU run by one rule: every case compares at least ~250
elements (a few users go with a large dim, the dims up to 48 with 130 users), because E32 and the
kernel's deviation are both maxima over the case's elements and the maximum over a dozen elements
is mostly chance.  ``UNALIGNED`` names the cases the tests run again on tables that start 4 bytes
off a 16-byte boundary, where every dim takes a scalar layout: the power-of-two dims then fill
every lane slot exactly (dim == LPU * EPL), and dim 24 keeps its layout.
"""
import functools

import numpy as np
import torch

from recommendation_gans_amd import mf_engine

NUM_ITEMS = 300
LR = 0.05
BETAS, EPS = (0.9, 0.999), 1e-8
CANCEL = 1e-5          # a gradient below this share of its sum of |terms| is rounding
TIE = 16 * 2.0 ** -24  # adaptive hinge: two highest negatives this close are equal to float32
LEFT_OUT_CAP = 0.01

# (dim, users, n_neg, steps, loss, weight_decay, init)
CASES = [
    (1, 130, 3, 2, "pointwise", 0.0, "zero"),
    (3, 130, 1, 8, "hinge", 1e-3, "random"),
    (16, 130, 3, 8, "pointwise", 1e-3, "zero"),
    (64, 130, 5, 2, "bpr", 0.0, "random"),
    (65, 5, 3, 8, "adaptive_hinge", 0.0, "zero"),
    (256, 130, 1, 1, "pointwise", 0.0, "random"),
    (256, 1, 0, 8, "pointwise", 1e-3, "random"),
    (64, 5, 5, 8, "adaptive_hinge", 1e-3, "random"),
    (256, 5, 3, 2, "hinge", 0.0, "zero"),
    (65, 130, 5, 1, "bpr", 1e-3, "zero"),
    (64, 1, 3, 8, "bpr", 0.0, "random"),
    (1, 130, 5, 8, "adaptive_hinge", 0.0, "random"),
    (16, 130, 1, 2, "hinge", 0.0, "zero"),
    (3, 130, 0, 2, "pointwise", 0.0, "zero"),
    # the layouts the list above never selected (every one admitted as first written)
    (8, 130, 5, 8, "bpr", 1e-3, "random"),
    (32, 130, 3, 2, "adaptive_hinge", 0.0, "zero"),
    (24, 130, 1, 8, "pointwise", 0.0, "random"),
    (48, 130, 5, 1, "hinge", 1e-3, "zero"),
    (128, 5, 3, 8, "bpr", 0.0, "zero"),
    (160, 5, 1, 2, "adaptive_hinge", 1e-3, "random"),
    (200, 5, 5, 8, "hinge", 0.0, "random"),
    (96, 5, 3, 2, "pointwise", 1e-3, "random"),
]
CASE_IDS = ["d%d-u%d-n%d-t%d-%s-wd%g-%s" % c for c in CASES]
# the cases run again on unaligned tables: the first case of dims 8, 16, 64, 128 and 24
UNALIGNED = [next(i for i, c in enumerate(CASES) if c[0] == dim) for dim in (8, 16, 64, 128, 24)]


def history_lengths(users):
    """Mixed lengths: the wave width and its neighbours, an empty row, 200 for a few rows."""
    if users == 1:
        return np.array([65])
    if users == 5:
        return np.array([0, 1, 64, 65, 200])
    pat = [0, 1, 2, 63, 64, 65, 3, 5, 2, 1]
    lens = np.array([pat[r % len(pat)] for r in range(users)])
    lens[[17, 101]] = 200
    return lens


def make_case(dim, users, n_neg, seed=0, init="zero", lens=None):
    """Item tables, a CSR of histories (duplicates allowed), fixed negatives and a start."""
    rs = np.random.RandomState(1000 * dim + 10 * users + n_neg + 7919 * seed)
    lens = history_lengths(users) if lens is None else np.asarray(lens)
    ptr = np.zeros(users + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    nnz = int(ptr[-1])
    case = dict(dim=dim, users=users, n_neg=n_neg, ptr=ptr,
                Q=(rs.randn(NUM_ITEMS, dim) * 0.7 / np.sqrt(dim)).astype(np.float32),
                c=(rs.randn(NUM_ITEMS) * 0.3).astype(np.float32),
                idx=rs.randint(0, NUM_ITEMS, nnz).astype(np.int32),
                neg=rs.randint(0, NUM_ITEMS, nnz * n_neg).astype(np.int32))
    if init == "random":
        case["W0"] = (rs.randn(users, dim) * 0.1).astype(np.float32)
        case["b0"] = (rs.randn(users) * 0.1).astype(np.float32)
    else:
        case["W0"] = np.zeros((users, dim), np.float32)
        case["b0"] = np.zeros(users, np.float32)
    return case


def reference64(case, loss, steps, wd, lr=LR):
    """The tests' reference: the product's chain of torch ops on float64 CPU copies."""
    t = torch.from_numpy
    W, b, lv = mf_engine.fold_in_users_torch(
        t(case["Q"].astype(np.float64)), t(case["c"].astype(np.float64)), t(case["ptr"]), t(case["idx"]),
        t(case["neg"]), case["n_neg"], loss=loss, steps=steps, lr=lr, weight_decay=wd, betas=BETAS, eps=EPS,
        init=(t(case["W0"].astype(np.float64)), t(case["b0"].astype(np.float64))), return_loss=True)
    return W.numpy(), b.numpy(), lv.numpy()


def _sum_rows(x, order):
    """Sum over axis 1 of (n, L, ...) in the dtype of x: sequentially ("forward"; "reversed" gets
    its rows already reversed) or as a balanced tree ("pairwise")."""
    if x.shape[1] == 0:
        return np.zeros(x.shape[:1] + x.shape[2:], x.dtype)
    if order != "pairwise":
        return np.cumsum(x, axis=1, dtype=x.dtype)[:, -1]
    while x.shape[1] > 1:
        if x.shape[1] % 2:
            x = np.concatenate([x, np.zeros_like(x[:, :1])], axis=1)
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def numpy_fold(case, loss, steps, wd, dtype=np.float64, order="forward", lr=LR):
    """The objective restated in numpy with hand-written gradients, every array in ``dtype``.
    Returns W, b, the last step's loss, and (float64 runs) what the leave-out rule reads: per element
    the smallest |gradient| / sum |terms| over the steps, and per row the smallest gap between an
    adaptive hinge's two highest negatives."""
    f = dtype
    n, k, dim, ptr = case["users"], case["n_neg"], case["dim"], case["ptr"]
    Q, c = case["Q"].astype(f), case["c"].astype(f)
    lens = np.diff(ptr)
    L = int(lens.max()) if n else 0
    col = np.arange(L)
    mask = col[None, :] < lens[:, None]
    within = (lens[:, None] - 1 - col[None, :]) if order == "reversed" else np.broadcast_to(col[None, :], (n, L))
    src = np.clip(ptr[:-1, None] + within, 0, max(len(case["idx"]) - 1, 0))
    pos = np.where(mask, case["idx"][src] if len(case["idx"]) else 0, 0)
    neg = np.where(mask[:, :, None], case["neg"].reshape(len(case["idx"]), k)[src] if len(case["idx"]) else 0, 0)
    Qp, cp, Qn, cn = Q[pos], c[pos], Q[neg], c[neg]
    mf_, mk = mask.astype(f), mask[:, :, None]
    W, b = case["W0"].astype(f), case["b0"].astype(f)
    mW, vW, mb, vb = np.zeros_like(W), np.zeros_like(W), np.zeros_like(b), np.zeros_like(b)
    live = lens > 0
    inv_p = (f(1.0) / np.maximum(lens, 1).astype(f))[:, None]
    inv_pn = (f(1.0) / np.maximum(lens * max(k, 1), 1).astype(f))[:, None, None]
    coef = mf_engine.adam_step_coef(steps, lr, BETAS).astype(f)
    b1, b2 = f(1.0 - BETAS[0]), f(1.0 - BETAS[1])
    ratio_W, ratio_b = np.full((n, dim), np.inf), np.full(n, np.inf)
    gap = np.full(n, np.inf)
    lv = np.zeros(n, f)
    for t in range(steps):
        sp = _sigmoid((W[:, None, :] * Qp).sum(-1) + b[:, None] + cp)                  # (n, L)
        sn = _sigmoid((W[:, None, None, :] * Qn).sum(-1) + b[:, None, None] + cn)      # (n, L, k)
        dzn = np.zeros_like(sn)
        if loss == "pointwise":
            lv = -_sum_rows(np.maximum(np.log(sp), f(-100.0)) * mf_, order) * inv_p[:, 0]
            dzp = (sp - f(1.0)) * inv_p
            if k:
                lneg = np.maximum(np.log(f(1.0) - sn), f(-100.0)) * mf_[:, :, None]
                lv = lv - _sum_rows(np.cumsum(lneg, axis=2, dtype=f)[:, :, -1], order) * inv_pn[:, 0, 0]
                dzn = sn * inv_pn
        elif loss == "bpr":
            sg = _sigmoid(sp[:, :, None] - sn)
            lv = _sum_rows(np.cumsum((f(1.0) - sg) * mf_[:, :, None], axis=2, dtype=f)[:, :, -1], order) * inv_pn[:, 0, 0]
            dx = -(((f(1.0) - sg) * sg) * inv_pn)
            dzp = np.cumsum(dx, axis=2, dtype=f)[:, :, -1] * (f(1.0) - sp) * sp
            dzn = (-dx) * (f(1.0) - sn) * sn
        elif loss == "hinge":
            x = (sn - sp[:, :, None]) + f(1.0)
            lv = _sum_rows(np.cumsum(np.maximum(x, f(0.0)) * mf_[:, :, None], axis=2, dtype=f)[:, :, -1], order) * \
                inv_pn[:, 0, 0]
            dx = np.where(x >= 0, inv_pn, f(0.0)).astype(f)
            dzp = -np.cumsum(dx, axis=2, dtype=f)[:, :, -1] * (f(1.0) - sp) * sp
            dzn = dx * (f(1.0) - sn) * sn
        else:
            jm = np.argmax(sn, axis=2)                                                  # the lowest j of equals
            best = np.take_along_axis(sn, jm[:, :, None], axis=2)[:, :, 0]
            if k > 1:    # the runner-up among OTHER items: a repeat of the winning item is the same row either way
                other = np.where(neg != np.take_along_axis(neg, jm[:, :, None], axis=2), sn, -np.inf).max(axis=2)
                gap = np.minimum(gap, np.where(mask, best - other, np.inf).min(axis=1, initial=np.inf))
            x = (best - sp) + f(1.0)
            lv = _sum_rows(np.maximum(x, f(0.0)) * mf_, order) * inv_p[:, 0]
            dx = np.where(x >= 0, inv_p, f(0.0)).astype(f)
            dzp = -dx * (f(1.0) - sp) * sp
            np.put_along_axis(dzn, jm[:, :, None], (dx * (f(1.0) - best) * best)[:, :, None], axis=2)
        dzp = dzp * mf_
        dzn = dzn * mf_[:, :, None]
        # a positive's term: its negatives in order, then itself; the positives by ``order``
        term = np.zeros((n, L, dim), f)
        tb = np.zeros((n, L), f)
        for j in range(k):
            term = term + dzn[:, :, j, None] * Qn[:, :, j]
            tb = tb + dzn[:, :, j]
        term = term + dzp[:, :, None] * Qp
        tb = tb + dzp
        gW, gb = _sum_rows(term, order), _sum_rows(tb, order)
        if f is np.float64:
            aW = (np.abs(dzn[:, :, :, None] * Qn).sum((1, 2)) + np.abs(dzp[:, :, None] * Qp).sum(1)) + np.abs(wd * W)
            ab = np.abs(dzn).sum((1, 2)) + np.abs(dzp).sum(1) + np.abs(wd * b)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio_W = np.minimum(ratio_W, np.where(aW > 0, np.abs(gW + wd * W) / aW, np.inf))
                ratio_b = np.minimum(ratio_b, np.where(ab > 0, np.abs(gb + wd * b) / ab, np.inf))
        ss, bc2 = coef[t]
        for p_, g_, m_, v_ in ((W, gW, mW, vW), (b, gb, mb, vb)):
            g_ = g_ + f(wd) * p_
            m_ += b1 * (g_ - m_)
            v_ *= f(BETAS[1])
            v_ += b2 * g_ * g_
            upd = (-ss) * m_ / (np.sqrt(v_) / bc2 + f(EPS))
            p_ += np.where(live.reshape((-1,) + (1,) * (p_.ndim - 1)), upd, f(0.0)).astype(f)
    return dict(W=W, b=b, loss=np.where(live, lv, f(0.0)).astype(f), ratio_W=ratio_W, ratio_b=ratio_b, gap=gap)


@functools.lru_cache(maxsize=None)
def case_data(i):
    """Case i, computed once per process and shared (treat as read-only): the case, the float64
    reference, the float64 restatement, the elements the comparison keeps, and E32 -- the largest
    deviation from the float64 restatement, over the kept elements, of the float32 restatement with
    the positives summed forward, reversed and pairwise (params and loss separately)."""
    dim, users, n_neg, steps, loss, wd, init = CASES[i]
    case = make_case(dim, users, n_neg, init=init)
    ref = reference64(case, loss, steps, wd)
    r64 = numpy_fold(case, loss, steps, wd)
    row_ok = r64["gap"] > TIE
    keep_W = (r64["ratio_W"] >= CANCEL) & row_ok[:, None]
    keep_b = (r64["ratio_b"] >= CANCEL) & row_ok
    e32 = e32_loss = 0.0
    for order in ("forward", "reversed", "pairwise"):
        r32 = numpy_fold(case, loss, steps, wd, dtype=np.float32, order=order)
        e32 = max(e32, deviation(r32["W"], r32["b"], (r64["W"], r64["b"]), keep_W, keep_b))
        e32_loss = max(e32_loss, float(np.abs(r32["loss"].astype(np.float64) - r64["loss"])[row_ok].max(initial=0.0)))
    return dict(case=case, loss=loss, steps=steps, wd=wd, ref=ref, r64=r64, keep_W=keep_W, keep_b=keep_b,
                row_ok=row_ok, e32=e32, e32_loss=e32_loss,
                left_out=1.0 - (keep_W.sum() + keep_b.sum()) / float(keep_W.size + keep_b.size))


def deviation(W, b, ref, keep_W, keep_b):
    """Largest kept elementwise |difference| of (W, b) from ref's (W, b), in float64."""
    dW = np.abs(np.asarray(W, np.float64) - ref[0])[keep_W].max(initial=0.0)
    db = np.abs(np.asarray(b, np.float64) - ref[1])[keep_b].max(initial=0.0)
    return float(max(dW, db))


def loss64(case, loss, W, b, wd=0.0):
    """float64 per-row loss of the rows (W, b) on the case's pairs (zero steps of the restatement)."""
    probe = dict(case, W0=np.asarray(W, np.float64), b0=np.asarray(b, np.float64))
    out = numpy_fold(probe, loss, 1, wd)      # the loss is taken before the step's update
    return out["loss"]
