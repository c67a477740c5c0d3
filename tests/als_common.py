"""What the ALS tests share (no tests here): the case builder, an independent numpy restatement of
the half-step in include/rg_hip.h (rg_als_solve_rows) -- written without ``als.py``, every array in
one dtype, the list summed forward, reversed or pairwise -- and ``E32``: the largest deviation of the
three float32 restatements from the float64 one over a case's elements, which is the error a float32
evaluation of the same formulas has.

The cases cover every row layout the kernels are instantiated for (rg_common.h dispatch_rows<128>; LPU
lanes x EPL elements per lane), by dim:
    8 / 16 / 32 / 64 / 128   the 16-byte layouts of 2 / 4 / 8 / 16 / 32 lanes x 4
    1, 3                     scalar, 16 lanes x 1        24    scalar, 16 lanes x 2
    48                       scalar, 16 lanes x 4        65    scalar, 64 lanes x 2
with rows {1, 5, 130}, list lengths {0, 1, 2, 63, 64, 65, 200} mixed in one call plus {T - 1, T,
T + 1, 3 T + 5} around the kernel's threshold T between its two paths, cg_steps {1, 3, 8}, alpha
{0, 1, 40}, values absent or random in (0, 2], zero and random starts, 300 items -- a covering
list, not the product; every case compares at least ~250 elements where its shape allows (dim 1
has 130, the single row 128).  ``UNALIGNED`` names the cases the tests run again on tables that
start 4 bytes off a 16-byte boundary, where every dim takes a scalar layout: the power-of-two dims
then fill every lane slot exactly (dim == LPU * EPL), and dim 24 keeps its layout.

Conditioning is a condition on the INPUTS, not a tolerance: truncated CG on an ill-conditioned row
amplifies rounding (dim 64, cg_steps 8, lam 0.01, alpha 40: E32 5e-3 at max|x| 4.5), so cg_steps 8 is
paired with lam in {0.1, 1} or alpha <= 1, lam 0.01 kept for cg_steps <= 3, and a case is admitted
only if its E32 <= 1e-4 max|x| (``admitted``; asserted without a GPU and again in the GPU tests).
"""
import functools

import numpy as np

NUM_ITEMS = 300
T = 256                  # rg_als_long_row_len(); the GPU and CPU tests assert that it is
TIE = 16 * 2.0 ** -24    # fold_in_common.TIE
ADMIT = 1e-4

# (dim, rows, cg_steps, lam, alpha, values, init, long)
CASES = [
    (1, 130, 1, 0.01, 40.0, False, "zero", False),
    (3, 130, 3, 0.01, 1.0, True, "random", False),
    (16, 130, 3, 0.01, 40.0, True, "zero", False),
    (64, 130, 3, 0.01, 40.0, False, "random", False),
    (65, 5, 8, 1.0, 1.0, True, "zero", False),
    (128, 5, 8, 1.0, 1.0, False, "random", False),
    (128, 130, 1, 0.01, 0.0, True, "zero", False),
    (64, 5, 8, 0.1, 1.0, True, "random", True),
    (16, 130, 8, 1.0, 40.0, False, "random", True),
    (128, 5, 3, 0.01, 40.0, True, "zero", True),
    (3, 130, 8, 0.1, 0.0, False, "zero", True),
    (65, 130, 3, 0.01, 1.0, False, "random", True),
    (128, 1, 3, 0.01, 40.0, True, "random", True),
    (1, 130, 3, 1.0, 1.0, True, "random", True),
    # the layouts the list above never selected.  Admitted as first written, but for dim 32: with
    # lam 0.1 it was first paired with alpha 40, where the two float64 statements of 8 CG steps
    # (test_als_cpu.py) part by 1.7e-11, past their 1e-12; alpha 1 is the other pairing the rule allows
    (8, 130, 3, 0.01, 40.0, True, "random", True),
    (32, 130, 8, 0.1, 1.0, False, "zero", False),
    (24, 130, 8, 1.0, 1.0, True, "zero", False),
    (48, 130, 3, 0.01, 1.0, False, "random", True),
]
CASE_IDS = ["d%d-r%d-cg%d-lam%g-a%g-%s-%s-%s" % (c[0], c[1], c[2], c[3], c[4], "val" if c[5] else "ones", c[6],
                                                "long" if c[7] else "short") for c in CASES]
# the cases run again on unaligned tables: the first case of dims 8, 16, 64, 128 and 24
UNALIGNED = [next(i for i, c in enumerate(CASES) if c[0] == dim) for dim in (8, 16, 64, 128, 24)]


def list_lengths(rows, long_):
    """Mixed lengths: the wave width and its neighbours, an empty row, 200 for a few rows; ``long_``
    puts T - 1, T, T + 1 and 3 T + 5 among them (the kernel's other path and both sides of T)."""
    if rows == 1:
        return np.array([3 * T + 5 if long_ else 65])
    if rows == 5:
        return np.array([0, T - 1, T, T + 1, 3 * T + 5] if long_ else [0, 1, 64, 65, 200])
    pat = [0, 1, 2, 63, 64, 65, 3, 5, 2, 1]
    lens = np.array([pat[r % len(pat)] for r in range(rows)])
    lens[[17, 101]] = 200
    if long_:
        lens[[7, 33, 64, 120]] = [T - 1, T, T + 1, 3 * T + 5]
    return lens


def make_case(dim, rows, lam, alpha, values, init, long_=False, seed=0, lens=None):
    """The other table Y, its Gram matrix G = Y^T Y + lam I (float64 product rounded to float32:
    symmetric), a CSR of lists (duplicates allowed), values and a start."""
    rs = np.random.RandomState(1000 * dim + 10 * rows + 7919 * seed + (1 if long_ else 0))
    lens = list_lengths(rows, long_) if lens is None else np.asarray(lens)
    ptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    nnz = int(ptr[-1])
    Y = (rs.randn(NUM_ITEMS, dim) * 0.7 / np.sqrt(dim)).astype(np.float32)
    Y64 = Y.astype(np.float64)
    G = (Y64.T @ Y64 + lam * np.eye(dim)).astype(np.float32)
    case = dict(dim=dim, rows=rows, lam=lam, alpha=alpha, ptr=ptr, Y=Y, G=G,
                idx=rs.randint(0, NUM_ITEMS, nnz).astype(np.int32),
                val=(2.0 - 2.0 * rs.rand(nnz)).astype(np.float32) if values else None)
    case["X0"] = (rs.randn(rows, dim) * 0.1).astype(np.float32) if init == "random" else np.zeros((rows, dim), np.float32)
    return case


def _sum_lists(x, order):
    """Sum over axis 1 of (n, L, ...) in the dtype of x: sequentially ("forward"; "reversed" gets its
    lists already reversed) or as a balanced tree ("pairwise")."""
    if x.shape[1] == 0:
        return np.zeros(x.shape[:1] + x.shape[2:], x.dtype)
    if order != "pairwise":
        return np.cumsum(x, axis=1, dtype=x.dtype)[:, -1]
    while x.shape[1] > 1:
        if x.shape[1] % 2:
            x = np.concatenate([x, np.zeros_like(x[:, :1])], axis=1)
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def numpy_als_rows(case, cg_steps, dtype=np.float64, order="forward", X0=None):
    """The half-step restated in numpy, every array in ``dtype``: returns (x [rows, dim], loss
    [rows]) -- the rows after ``cg_steps`` CG iterations from X0 (the case's start by default),
    empty rows zero, and x^T G x + sum ((c - 1) s^2 - 2 c s + c) at the returned rows."""
    f = dtype
    n, dim, ptr = case["rows"], case["dim"], case["ptr"]
    Y, G = case["Y"].astype(f), case["G"].astype(f)
    lens = np.diff(ptr)
    L = int(lens.max()) if n else 0
    col = np.arange(L)
    mask = col[None, :] < lens[:, None]
    within = (lens[:, None] - 1 - col[None, :]) if order == "reversed" else np.broadcast_to(col[None, :], (n, L))
    nnz = len(case["idx"])
    src = np.clip(ptr[:-1, None] + within, 0, max(nnz - 1, 0))
    ids = np.where(mask, case["idx"][src] if nnz else 0, 0)
    v = case["val"][src].astype(f) if case["val"] is not None and nnz else np.ones((n, L), f)
    c1 = np.where(mask, f(case["alpha"]) * v, f(0.0)).astype(f)
    c = np.where(mask, f(1.0) + c1, f(0.0)).astype(f)
    Yg = Y[ids]                                                     # (n, L, dim)

    def dots(vec):                                                  # y_i . vec per entry
        return (Yg * vec[:, None, :]).sum(-1, dtype=f)

    def A(vec):
        return (vec @ G.T).astype(f) + _sum_lists((c1 * dots(vec))[:, :, None] * Yg, order)

    def rowdot(a, b):
        return (a * b).sum(1, dtype=f)

    x = (case["X0"] if X0 is None else X0).astype(f).copy()
    live = lens > 0
    if cg_steps:
        r = _sum_lists(c[:, :, None] * Yg, order) - A(x)
        p = r.copy()
        rs = rowdot(r, r)
        go = live.copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            for _ in range(cg_steps):
                Ap = A(p)
                pAp = rowdot(p, Ap)
                go = go & (rs != 0) & (pAp > 0)
                g = go[:, None]
                a = (rs / pAp).astype(f)[:, None]
                x = np.where(g, x + a * p, x).astype(f)
                r = np.where(g, r - a * Ap, r).astype(f)
                rn = rowdot(r, r)
                p = np.where(g, r + (rn / rs).astype(f)[:, None] * p, p).astype(f)
                rs = np.where(go, rn, rs).astype(f)
    x[~live] = 0
    s = dots(x)
    loss = rowdot(x, (x @ G.T).astype(f)) + _sum_lists(c1 * s * s - f(2.0) * c * s + c, order)
    return x, np.where(live, loss, f(0.0)).astype(f)


def e32_of(run64, run32):
    """(E32 of x, E32 of the loss, max|x|) from the float64 result and the three float32 ones."""
    e_x = max(float(np.abs(x.astype(np.float64) - run64[0]).max(initial=0.0)) for x, _ in run32)
    e_l = max(float(np.abs(l.astype(np.float64) - run64[1]).max(initial=0.0)) for _, l in run32)
    return e_x, e_l, float(np.abs(run64[0]).max(initial=0.0))


ORDERS = ("forward", "reversed", "pairwise")


@functools.lru_cache(maxsize=None)
def case_data(i):
    """Case i, computed once per process and shared (treat as read-only): the case, the float64
    restatement (x, loss), E32 of both, max|x| and whether the case is admitted."""
    dim, rows, cg, lam, alpha, values, init, long_ = CASES[i]
    return measure(make_case(dim, rows, lam, alpha, values, init, long_), cg)


def measure(case, cg):
    """What ``case_data`` holds, of any case: the float64 restatement, E32 from the three float32
    ones, max|x| and the admission rule."""
    r64 = numpy_als_rows(case, cg)
    r32 = [numpy_als_rows(case, cg, np.float32, o) for o in ORDERS]
    e32, e32_loss, xmax = e32_of(r64, r32)
    return dict(case=case, cg=cg, r64=r64, e32=e32, e32_loss=e32_loss, xmax=xmax, admitted=e32 <= ADMIT * xmax)


def sub_case(case, rows):
    """The case of ``rows`` alone (their lists, values and starts, in that order; the same tables)."""
    rows = np.asarray(rows)
    ptr = case["ptr"]
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    new_ptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[rows])]).astype(np.int64)
    return dict(case, rows=len(rows), ptr=new_ptr, idx=case["idx"][take],
                val=None if case["val"] is None else case["val"][take], X0=case["X0"][rows])


# Launch geometry of rg_als_solve_rows, restated from rg_als.hip's AlsLaunch for the tests that make a
# workgroup take a second trip: both kernels run 8 waves per workgroup, a compute unit has 160 KB of
# LDS, and the grid is capped at CUs * min(4, 160 KB / LDS per workgroup) workgroups, which stride.
WAVES, WAVE, LDS_CU = 8, 64, 160 * 1024


def aligned_layout(dim):
    """(LPU, EPL) of an aligned call at ``dim`` (rg_common.h dispatch_rows, which rg_als.hip caps at
    dim 128)."""
    if dim in (8, 16, 32, 64, 128):
        return dim // 4, 4
    return (16, 1) if dim <= 16 else (16, 2) if dim <= 32 else (16, 4) if dim <= 64 else (64, 2)


def short_grid_cap(dim, cus):
    """(workgroups the short kernel launches at most, rows of one tile): a wave solves a tile of
    64 / LPU rows per trip; LDS per workgroup is G plus one p slot per lane group."""
    lpu, epl = aligned_layout(dim)
    lds = 4 * (((dim * dim + 3) & ~3) + WAVES * WAVE * epl)
    return cus * min(4, LDS_CU // lds), WAVE // lpu


def long_grid_cap(dim, cus):
    """Workgroups the long kernel launches at most (a workgroup per row per trip): LDS is G, the p
    slots, two vector scratch areas of the same size and one scalar per lane group."""
    lpu, epl = aligned_layout(dim)
    lds = 4 * (((dim * dim + 3) & ~3) + 3 * WAVES * WAVE * epl + WAVES * (WAVE // lpu))
    return cus * min(4, LDS_CU // lds)


def explicit_system(case, u):
    """A_u and b_u of row u, formed explicitly in float64."""
    Y, G = case["Y"].astype(np.float64), case["G"].astype(np.float64)
    lo, hi = case["ptr"][u], case["ptr"][u + 1]
    ids = case["idx"][lo:hi]
    v = case["val"][lo:hi].astype(np.float64) if case["val"] is not None else np.ones(hi - lo)
    c1 = float(case["alpha"]) * v
    Yn = Y[ids]
    return G + (Yn * c1[:, None]).T @ Yn, ((1.0 + c1)[:, None] * Yn).sum(0)


# ---------------------------------------------------------------- the whole procedure (fit_als)
def transpose_csr(ptr, idx, val, n_cols):
    """The transposed CSR, a column's entries in the order of the rows they came from."""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    tptr = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(idx, minlength=n_cols), out=tptr[1:])
    return tptr, rows[order].astype(np.int32), None if val is None else val[order]


def numpy_gram(table, lam, dtype):
    t = table.astype(dtype)
    return ((t.T @ t).astype(dtype) + dtype(lam) * np.eye(t.shape[1], dtype=dtype)).astype(dtype)


def numpy_sweeps(X0, Y0, csr_u, csr_i, sweeps, lam, alpha, cg, dtype=np.float64, order="forward"):
    """``sweeps`` ALS sweeps restated in numpy in ``dtype`` (Gram matrices too): the (X, Y) after
    every sweep."""
    X, Y = X0.astype(dtype), Y0.astype(dtype)
    out = []
    for _ in range(sweeps):
        cu = dict(dim=X.shape[1], rows=X.shape[0], alpha=alpha, ptr=csr_u[0], idx=csr_u[1], val=csr_u[2], Y=Y,
                  G=numpy_gram(Y, lam, dtype), X0=X)
        X = numpy_als_rows(cu, cg, dtype, order)[0]
        ci = dict(dim=X.shape[1], rows=Y.shape[0], alpha=alpha, ptr=csr_i[0], idx=csr_i[1], val=csr_i[2], Y=X,
                  G=numpy_gram(X, lam, dtype), X0=Y)
        Y = numpy_als_rows(ci, cg, dtype, order)[0]
        out.append((X.copy(), Y.copy()))
    return out


def objective64(X, Y, csr_u, alpha, lam):
    """The ALS objective by brute force in float64: every (user, item) cell of the dense block, then
    the listed entries' corrections (a duplicate counts once per occurrence)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    S = X @ Y.T
    total = float((S * S).sum())
    ptr, idx, val = csr_u
    for u in range(len(ptr) - 1):
        for e in range(ptr[u], ptr[u + 1]):
            c1 = float(alpha) * (float(val[e]) if val is not None else 1.0)
            s = S[u, idx[e]]
            total += c1 * s * s - 2.0 * (1.0 + c1) * s + (1.0 + c1)
    return total + float(lam) * float((X * X).sum() + (Y * Y).sum())


FIT = dict(users=130, items=NUM_ITEMS, dim=16, sweeps=3, cg=3, lam=0.1, alpha=40.0, nnz=4000, seed=1)


@functools.lru_cache(maxsize=None)
def fit_data():
    """The end-to-end case: 130 users x 300 items, 4000 interactions (duplicates as drawn), and the
    restatement of three sweeps from a fixed start in float64 and, for E32 of the whole procedure,
    in float32 with the three orders."""
    p = FIT
    rs = np.random.RandomState(p["seed"])
    users = rs.randint(0, p["users"], p["nnz"]).astype(np.int32)
    items = (rs.zipf(1.3, p["nnz"]) % p["items"]).astype(np.int32)
    X0 = (rs.randn(p["users"], p["dim"]) / p["dim"]).astype(np.float32)
    Y0 = (rs.randn(p["items"], p["dim"]) / p["dim"]).astype(np.float32)
    order = np.argsort(users, kind="stable")
    ptr = np.zeros(p["users"] + 1, dtype=np.int64)
    np.cumsum(np.bincount(users, minlength=p["users"]), out=ptr[1:])
    csr_u = (ptr, items[order], None)
    csr_i = transpose_csr(ptr, csr_u[1], None, p["items"])
    r64 = numpy_sweeps(X0, Y0, csr_u, csr_i, p["sweeps"], p["lam"], p["alpha"], p["cg"])
    e32 = 0.0
    for o in ORDERS:
        X, Y = numpy_sweeps(X0, Y0, csr_u, csr_i, p["sweeps"], p["lam"], p["alpha"], p["cg"], np.float32, o)[-1]
        e32 = max(e32, float(np.abs(X - r64[-1][0]).max()), float(np.abs(Y - r64[-1][1]).max()))
    return dict(users=users, items=items, X0=X0, Y0=Y0, csr_u=csr_u, csr_i=csr_i, r64=r64, e32=e32)
