"""Implicit ALS on the device: alternating least squares with confidence weights (Hu, Koren,
Volinsky 2008) over a pair of MF tables, each half-step a fused per-row conjugate-gradient solve
(rg_als_gram, rg_als_solve_rows; include/rg_hip.h has the maths and the kernel's layout).

Factors are ``X [num_users, d]`` and ``Y [num_items, d]``, no biases.  A list is a CSR row
``idx[ptr[u]:ptr[u + 1]]`` with values ``val`` (None: ones), duplicates counted as given;
``c = 1 + alpha * val``; ``G = Y^T Y + lam I``; a user half-step runs ``cg_steps`` CG iterations
on ``(G + sum (c - 1) y y^T) x = sum c y`` from the row's current value, and an empty row becomes
exactly zero.  The item half-step is the same call with the transposed CSR and the tables swapped.
The objective:

    L = sum_u [x_u^T (Y^T Y) x_u + sum_i ((c - 1)(x_u.y_i)^2 - 2 c (x_u.y_i) + c)] + lam (|X|^2 + |Y|^2)

``solve_rows_torch`` and ``objective_torch`` are the same formulas as chains of torch ops in the
tables' dtype: the timing baseline, and in float64 on the CPU a reference of the tests.  The kernel
calls take contiguous float32 CUDA tensors only -- there is no fall-back.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

MAX_DIM, MAX_CG_STEPS = 128, 64      # rg_als_solve_rows' ranges


def long_row_len():
    """Lists this long or longer take the workgroup-per-row path (rg_als_long_row_len)."""
    return int(_lib.load().rg_als_long_row_len())


def _device_table(t, what, name):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.dim() == 2):
        raise ValueError(f"{what} needs {name} as a contiguous float32 (rows, dim) tensor on a CUDA device")


def gram(table, lam):
    """``table^T table + lam I`` as a (dim, dim) float32 tensor on the table's device
    (rg_als_gram): per-block partials added in a fixed order, no atomics, so the bits repeat and
    the result is symmetric bit for bit.  ValueError for a table that is not contiguous float32
    (rows >= 1, 1 <= dim <= 128) on a CUDA device, or a ``lam`` that is negative or not finite."""
    lam = float(lam)
    if not (0.0 <= lam < float("inf")):
        raise ValueError("gram: lam must be finite and >= 0")
    _device_table(table, "gram", "the table")
    n, d = int(table.shape[0]), int(table.shape[1])
    if n < 1 or d < 1 or d > MAX_DIM:
        raise ValueError(f"gram: the table must be (rows >= 1, 1 <= dim <= {MAX_DIM})")
    lib = _lib.load()
    ws = torch.empty(int(lib.rg_als_gram_workspace_len(n, d)), dtype=torch.float32, device=table.device)
    G = torch.empty(d, d, dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        check(lib.rg_als_gram(_lib.stream_handle(), ptr(table), n, d, lam, ptr(ws), ptr(G)), "rg_als_gram")
    return G


def _solve_args(other, G, row_ptr, row_idx, row_val, alpha, cg_steps, x, rows, checked, what):
    """The argument checks both paths share (ValueError before anything touches a kernel).  Returns
    (ptr, idx, val or None, rows or None) as flat tensors, in the dtypes and on the devices they
    came in.  ``checked``: also the contents -- ``ptr`` ascends from 0 to len(idx), every id lies
    inside ``other``, every row id inside ``x`` and appears once (one download of a flag)."""
    if not (torch.is_tensor(other) and torch.is_tensor(G) and torch.is_tensor(x) and
            other.dtype == G.dtype == x.dtype and other.dtype in (torch.float32, torch.float64)):
        raise ValueError(f"{what}: other, G and x must be floating-point tensors of one dtype")
    if other.dim() != 2 or x.dim() != 2 or other.shape[1] != x.shape[1]:
        raise ValueError(f"{what}: other must be (n_other, dim) and x (n_rows, dim)")
    dim = int(other.shape[1])
    if dim < 1 or dim > MAX_DIM:
        raise ValueError(f"{what}: dim must be in [1, {MAX_DIM}]")
    if tuple(G.shape) != (dim, dim):
        raise ValueError(f"{what}: G must be (dim, dim)")
    alpha, cg_steps = float(alpha), int(cg_steps)
    if not (0.0 <= alpha < float("inf")):
        raise ValueError(f"{what}: alpha must be finite and >= 0")
    if cg_steps < 0 or cg_steps > MAX_CG_STEPS:
        raise ValueError(f"{what}: cg_steps must be in [0, {MAX_CG_STEPS}]")
    ints = (torch.int32, torch.int64)
    row_ptr, row_idx = torch.as_tensor(row_ptr), torch.as_tensor(row_idx)
    if row_ptr.dtype not in ints or row_idx.dtype not in ints:
        raise ValueError(f"{what}: ptr and idx must be int32 or int64")
    row_ptr, row_idx = row_ptr.reshape(-1), row_idx.reshape(-1)
    if row_ptr.numel() != x.shape[0] + 1:
        raise ValueError(f"{what}: ptr must have one entry per row of x and one more")
    if row_val is not None:
        row_val = torch.as_tensor(row_val).reshape(-1)
        if not row_val.dtype.is_floating_point or row_val.numel() != row_idx.numel():
            raise ValueError(f"{what}: val must hold one floating-point value per entry of idx")
    if rows is not None:
        rows = torch.as_tensor(rows)
        if rows.dtype not in ints:
            raise ValueError(f"{what}: rows must be int32 or int64")
        rows = rows.reshape(-1)
    if checked:
        nnz, n = int(row_idx.numel()), int(x.shape[0])
        bad = (row_ptr[0] != 0) | (row_ptr[-1] != nnz) | (row_ptr[1:] < row_ptr[:-1]).any()
        if bool(bad):
            raise ValueError(f"{what}: ptr must ascend from 0 to len(idx)")
        if nnz:
            lo, hi = torch.stack(row_idx.aminmax()).tolist()
            if lo < 0 or hi >= other.shape[0]:
                raise ValueError(f"{what}: idx holds an id outside [0, len(other))")
        if row_val is not None and nnz and not bool(torch.isfinite(row_val).all() & (row_val >= 0).all()):
            raise ValueError(f"{what}: val must be finite and >= 0")
        if rows is not None and rows.numel():
            lo, hi = torch.stack(rows.aminmax()).tolist()
            if lo < 0 or hi >= n:
                raise ValueError(f"{what}: rows holds a row id outside [0, len(x))")
            if int(torch.unique(rows).numel()) != int(rows.numel()):
                raise ValueError(f"{what}: rows holds a row id twice")
    return row_ptr, row_idx, row_val, rows


def solve_rows(other, G, ptr_, idx, val, alpha, cg_steps, x, rows=None, return_loss=False, checked=False):
    """One ALS half-step, in place on ``x`` (rg_als_solve_rows): row u of ``x`` takes ``cg_steps``
    CG iterations against the frozen table ``other`` and its Gram matrix ``G = gram(other, lam)``.
    ``rows``: the row ids to solve, in any order, each at most once (None: every row).  Returns
    ``x``, with ``return_loss`` also ``loss [len(x)]``: ``x^T G x + sum ((c - 1) s^2 - 2 c s + c)``
    with ``s = x.y`` at the returned row (rows outside ``rows`` hold 0).  ``cg_steps == 0``
    leaves the rows with a list as they are, zeroes the empty ones and still fills the loss.

    ValueError for tensors that are not contiguous float32 on one CUDA device (no fall-back), dim
    outside [1, 128], cg_steps outside [0, 64], a negative alpha, index arrays that are not
    integers or of the wrong length.  The contents of ``ptr_``, ``idx``, ``val`` and ``rows`` are
    trusted unless ``checked=True``, which validates them on the device before the launch (``ptr_``
    ascends from 0 to len(idx), ids inside ``other``, values finite and >= 0, row ids inside ``x``
    and distinct; one download of a flag)."""
    what = "solve_rows"
    if not (torch.is_tensor(other) and torch.is_tensor(G) and torch.is_tensor(x) and
            other.dtype == G.dtype == x.dtype == torch.float32):
        raise ValueError(f"{what}: other, G and x must be float32 tensors")
    rp, ri, rv, rows = _solve_args(other, G, ptr_, idx, val, alpha, cg_steps, x, rows, checked, what)
    if not (other.is_cuda and other.is_contiguous() and G.is_contiguous() and x.is_contiguous() and
            G.device == other.device and x.device == other.device):
        raise ValueError(f"{what} needs contiguous float32 tensors on one CUDA device")
    dev, n, dim = other.device, int(x.shape[0]), int(other.shape[1])
    loss = torch.zeros(n, dtype=torch.float32, device=dev) if return_loss else None
    n_rows = n if rows is None else int(rows.numel())
    if n_rows:
        rp = rp.to(dev, torch.int64).contiguous()
        ri = ri.to(dev, torch.int32).contiguous()
        if ri.numel() == 0:                       # every list is empty: the entry still wants a pointer
            ri = torch.zeros(1, dtype=torch.int32, device=dev)
        rv = rv.to(dev, torch.float32).contiguous() if rv is not None and rv.numel() else None
        rows_d = rows.to(dev, torch.int64).contiguous() if rows is not None else None
        with torch.cuda.device(dev):
            check(_lib.load().rg_als_solve_rows(_lib.stream_handle(), ptr(other), ptr(G), dim, ptr(rp), ptr(ri),
                                                ptr(rv), float(alpha), ptr(rows_d), n_rows, int(cg_steps), ptr(x),
                                                ptr(loss)), "rg_als_solve_rows")
    return (x, loss) if return_loss else x


def _row_blocks(lens, dim, block_elems):
    """Consecutive blocks [s, e) of the rows whose padded gather (rows x longest x dim) stays within
    ``block_elems`` elements (a single row may exceed it)."""
    n = len(lens)
    if block_elems is None:
        return [(0, n)] if n else []
    out, s = [], 0
    while s < n:
        e, longest = s + 1, max(int(lens[s]), 1)
        while e < n and (e + 1 - s) * max(longest, int(lens[e]), 1) * dim <= block_elems:
            longest = max(longest, int(lens[e]))
            e += 1
        out.append((s, e))
        s = e
    return out


def solve_rows_torch(other, G, ptr_, idx, val, alpha, cg_steps, x, rows=None, return_loss=False, checked=False,
                     block_elems=None):
    """``solve_rows`` as the chain of torch ops it replaces, on the tables' device and in their
    dtype, in place on ``x``: the lists padded to the longest row of a block, one (rows, longest,
    dim) gather, and the CG iteration batched over the rows with masks for the stopping rule.
    ``block_elems``: the rows (in the order of ``rows``) are taken in consecutive blocks whose padded
    gather stays within that many elements -- sort ``rows`` by length for it to help.  The timing
    baseline of the kernel, and in float64 on the CPU a reference of its tests."""
    rp, ri, rv, rows = _solve_args(other, G, ptr_, idx, val, alpha, cg_steps, x, rows, checked, "solve_rows_torch")
    dev, dt, dim = other.device, other.dtype, int(other.shape[1])
    Y, n = other.detach(), int(x.shape[0])
    alpha, cg_steps = float(alpha), int(cg_steps)
    rp, ri = rp.to(dev, torch.int64), ri.to(dev, torch.int64)
    rv = rv.to(dev, dt) if rv is not None else None
    rows = torch.arange(n, device=dev) if rows is None else rows.to(dev, torch.int64)
    loss = torch.zeros(n, dtype=dt, device=dev)
    all_lens = (rp[rows + 1] - rp[rows]) if rows.numel() else rp[:0]
    nnz = int(ri.numel())
    for s, e in _row_blocks(all_lens.tolist(), dim, block_elems):
        rb = rows[s:e]
        lo, lens = rp[rb], all_lens[s:e]
        Lmax = int(lens.max())
        live = lens > 0
        if Lmax == 0:
            x[rb] = 0
            continue
        col = torch.arange(Lmax, device=dev)
        mask = col[None, :] < lens[:, None]
        src = (lo[:, None] + col[None, :]).clamp(max=nnz - 1)
        ids = torch.where(mask, ri[src], torch.zeros((), dtype=torch.int64, device=dev))
        zero = torch.zeros((), dtype=dt, device=dev)
        c1 = torch.where(mask, alpha * rv[src] if rv is not None else torch.full((), alpha, dtype=dt, device=dev), zero)
        c = torch.where(mask, 1.0 + c1, zero)
        Yg = Y[ids]                                                   # (rows, Lmax, dim)

        def A(v):
            return v @ G.T + torch.einsum("nl,nld->nd", c1 * torch.einsum("nld,nd->nl", Yg, v), Yg)

        xs = x[rb].clone()
        if cg_steps:
            r = torch.einsum("nl,nld->nd", c, Yg) - A(xs)
            p = r.clone()
            rs = (r * r).sum(1)
            go = live.clone()
            for _ in range(cg_steps):
                go = go & (rs != 0)
                Ap = A(p)
                pAp = (p * Ap).sum(1)
                go = go & (pAp > 0)
                g = go[:, None]
                a = (rs / pAp)[:, None]
                xs = torch.where(g, xs + a * p, xs)
                r = torch.where(g, r - a * Ap, r)
                rn = (r * r).sum(1)
                p = torch.where(g, r + (rn / rs)[:, None] * p, p)
                rs = torch.where(go, rn, rs)
        xs[~live] = 0
        x[rb] = xs
        if return_loss:
            sc = torch.einsum("nld,nd->nl", Yg, xs)
            loss[rb] = (xs * (xs @ G.T)).sum(1) + (c1 * sc * sc - 2.0 * c * sc + c).sum(1)
    return (x, loss) if return_loss else x


def _csr(csr):
    if not (isinstance(csr, (tuple, list)) and len(csr) == 3):
        raise ValueError("a CSR is (ptr, idx, val or None)")
    return csr


def objective(X, Y, csr, alpha, lam):
    """The ALS objective L of (X, Y) on the user CSR ``(ptr, idx, val or None)`` as a float: the
    per-row terms from rg_als_solve_rows' ``loss_out`` at ``cg_steps = 0`` against ``gram(Y, 0)``
    (no dense block exists: sum_all (x.y)^2 = sum_u x_u^T (Y^T Y) x_u), summed in float64, plus
    ``lam`` times the two squared norms.  The pass runs on a copy of X (it zeroes rows with an empty
    list); such a row's term x^T (Y^T Y) x is added from the given X."""
    p_, i_, v_ = _csr(csr)
    _device_table(X, "objective", "X")
    _device_table(Y, "objective", "Y")
    G0 = gram(Y, 0.0)
    _, rows = solve_rows(Y, G0, p_, i_, v_, alpha, 0, X.clone(), return_loss=True)
    return _objective_total(X, Y, G0, p_, rows, lam)


def _objective_total(X, Y, G0, ptr_, rows, lam):
    lens = torch.as_tensor(ptr_).reshape(-1).to(X.device)
    E = X[lens[1:] == lens[:-1]].double()
    extra = ((E @ G0.double()) * E).sum()
    return float(rows.double().sum() + extra + float(lam) * (X.double().pow(2).sum() + Y.double().pow(2).sum()))


def objective_torch(X, Y, csr, alpha, lam):
    """``objective`` as a chain of torch ops in the tables' dtype (float64 on the CPU: a reference
    of the tests): the same closed form, with Y^T Y from one matmul."""
    p_, i_, v_ = _csr(csr)
    G0 = Y.T @ Y
    _, rows = solve_rows_torch(Y, G0, p_, i_, v_, alpha, 0, X.clone(), return_loss=True)
    return _objective_total(X, Y, G0, p_, rows, lam)


def rows_by_length(ptr_):
    """The row ids ordered by list length (stable), int64 on the host: neighbouring rows of a wave
    then loop equally long, and the workgroup-per-row lists sit together at the end."""
    p_ = np.asarray(torch.as_tensor(ptr_).cpu())
    return torch.from_numpy(np.argsort(np.diff(p_), kind="stable").astype(np.int64))


def als_sweeps(X, Y, csr_user, csr_item, *, iterations, lam, alpha, cg_steps, losses=None):
    """``iterations`` ALS sweeps in place on the device tables X and Y: ``gram(Y, lam)``, the user
    half-step, ``gram(X, lam)``, the item half-step.  ``csr_user`` is ``(ptr, idx, val or None)``
    over the users' items, ``csr_item`` its transpose.  ``losses``: a list that receives the
    objective after every sweep (one more Gram matrix and one loss pass per sweep).  Returns (X, Y)."""
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError("als_sweeps: iterations must be >= 1")
    if not (0.0 < float(lam) < float("inf")):
        raise ValueError("als_sweeps: lam must be finite and > 0")
    (pu, iu, vu), (pi, ii, vi) = _csr(csr_user), _csr(csr_item)
    dev = X.device
    dv = lambda t, dt: None if t is None else torch.as_tensor(t).to(dev, dt).contiguous()      # noqa: E731
    pu, pi, iu, ii = dv(pu, torch.int64), dv(pi, torch.int64), dv(iu, torch.int32), dv(ii, torch.int32)
    vu, vi = dv(vu, torch.float32), dv(vi, torch.float32)
    ru, ri = rows_by_length(pu).to(dev), rows_by_length(pi).to(dev)
    for _ in range(iterations):
        solve_rows(Y, gram(Y, lam), pu, iu, vu, alpha, cg_steps, X, rows=ru)
        solve_rows(X, gram(X, lam), pi, ii, vi, alpha, cg_steps, Y, rows=ri)
        if losses is not None:
            losses.append(objective(X, Y, (pu, iu, vu), alpha, lam))
    return X, Y


def interactions_csr(rows, cols, vals, n_rows):
    """(ptr int64 [n_rows + 1], idx int32, val float32 or None) of the pairs (rows[k], cols[k]) with
    values vals[k], on the host: a row's entries in the order given, duplicates kept as they are."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    order = np.argsort(rows, kind="stable")
    ptr_ = np.zeros(int(n_rows) + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=int(n_rows)), out=ptr_[1:])
    idx = np.asarray(cols).reshape(-1)[order].astype(np.int32)
    val = None if vals is None else np.asarray(vals, dtype=np.float32).reshape(-1)[order]
    return ptr_, idx, val
