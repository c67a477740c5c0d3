"""rg_als_gram and rg_als_solve_rows on the GPU: parity with the float64 numpy restatement inside
twice the error of a float32 evaluation of the same formulas (E32, tests/als_common.py), bit
invariance of a row against its place in the call on both sides of the kernel's path threshold, the
same parity on tables that start off a 16-byte boundary (the entry's scalar-layout dispatch), calls
large enough that a workgroup of either kernel takes a second trip over the rows (sized from the
device's compute-unit count), the Gram matrix, cg_steps = 0, guard elements, and ``fit_als`` /
``fold_in_users_als`` / ``recommend_for_histories(method=)`` end to end.  300 items; every case in a
few seconds.

The parity bound is measured, not picked: E32 is the largest deviation from float64 of the float32
restatement with the lists summed forward, reversed and pairwise; the kernel -- one more ordering of
the same sums, with fused multiply-adds -- must stay within 2 x E32 (the project's rule for
fold-in).  Both figures are printed per case.  A case is admitted only if E32 <= 1e-4 max|x|: the
conditioning of truncated CG is a condition on the inputs (als_common's docstring).
"""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib, als
from tests import als_common as ac

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
t = torch.from_numpy


def run(case, cg, rows=None, return_loss=True, X0=None):
    """The kernel on ``case`` (on its ``rows`` only when given): host arrays (x, loss).  x and the
    loss are followed by guard elements, which must come back untouched."""
    n, dim = case["rows"], case["dim"]
    buf = torch.full((n * dim + GUARD,), -7.0, dtype=torch.float32, device=DEV)
    x = buf[:n * dim].view(n, dim)
    x.copy_(t(case["X0"] if X0 is None else X0))
    out = als.solve_rows(t(case["Y"]).to(DEV), t(case["G"]).to(DEV), t(case["ptr"]), t(case["idx"]),
                         None if case["val"] is None else t(case["val"]), case["alpha"], cg, x,
                         rows=None if rows is None else t(np.asarray(rows, np.int64)), return_loss=return_loss)
    torch.cuda.synchronize()
    assert (buf[n * dim:].cpu().numpy() == -7.0).all(), "elements past x_inout written"
    if return_loss:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy(), None


def test_the_threshold_is_the_one_the_cases_were_built_for():
    assert als.long_row_len() == ac.T


@pytest.mark.parametrize("i", range(len(ac.CASES)), ids=ac.CASE_IDS)
def test_parity_with_the_float64_restatement_within_twice_the_float32_error(i):
    d = ac.case_data(i)
    assert d["admitted"], (d["e32"], d["xmax"])
    case = d["case"]
    x, lv = run(case, d["cg"])
    assert x.dtype == lv.dtype == np.float32
    dev = float(np.abs(x.astype(np.float64) - d["r64"][0]).max())
    dev_loss = float(np.abs(lv.astype(np.float64) - d["r64"][1]).max())
    print(f"\ncase {ac.CASE_IDS[i]}: kernel {dev:.3e} E32 {d['e32']:.3e} ratio {dev / d['e32']:.2f} | "
          f"loss kernel {dev_loss:.3e} E32 {d['e32_loss']:.3e} ratio {dev_loss / d['e32_loss']:.2f} | "
          f"max|x| {d['xmax']:.2f}")
    empty = np.diff(case["ptr"]) == 0
    assert not x[empty].any() and not lv[empty].any()
    assert np.isfinite(x).all() and np.isfinite(lv).all()
    assert dev <= 2 * d["e32"]
    assert dev_loss <= 2 * d["e32_loss"]


def _view(host, off):
    """``host`` as a contiguous device view ``off`` floats into a buffer of -7 (guards on both sides)."""
    host = np.ascontiguousarray(host)
    buf = torch.full((off + host.size + GUARD,), -7.0, dtype=torch.float32, device=DEV)
    view = buf[off:off + host.size].view(host.shape)
    view.copy_(t(host))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return buf, view


def run_views(case, cg, off_other, off_x):
    """The kernel with other_table / x_inout ``off_other`` / ``off_x`` floats into larger buffers
    (``solve_rows`` hands contiguous views through as they are): host (x, loss)."""
    ybuf, Y = _view(case["Y"], off_other)
    xbuf, x = _view(case["X0"], off_x)
    _, lv = als.solve_rows(Y, t(case["G"]).to(DEV), t(case["ptr"]), t(case["idx"]),
                           None if case["val"] is None else t(case["val"]), case["alpha"], cg, x, return_loss=True)
    torch.cuda.synchronize()
    yb, xb = ybuf.cpu().numpy(), xbuf.cpu().numpy()
    assert yb[off_other:off_other + Y.numel()].tobytes() == case["Y"].tobytes(), "other_table written"
    for buf, off, size in ((yb, off_other, Y.numel()), (xb, off_x, x.numel())):
        assert (buf[:off] == -7.0).all() and (buf[off + size:] == -7.0).all(), "elements outside a table written"
    return x.cpu().numpy(), lv.cpu().numpy()


@pytest.mark.parametrize("which", ["other_table and x_inout", "x_inout alone"])
@pytest.mark.parametrize("i", ac.UNALIGNED, ids=[ac.CASE_IDS[i] for i in ac.UNALIGNED])
def test_tables_off_a_16_byte_boundary_meet_the_float64_restatement(i, which):
    """The unaligned dispatch (dispatch_rows' scalar layouts), held to float64 by the parity test's
    own rule; at dim 24 the aligned call selects the same layout, so the bits are the aligned call's."""
    d = ac.case_data(i)
    assert d["admitted"], (d["e32"], d["xmax"])
    case = d["case"]
    x, lv = run_views(case, d["cg"], 1 if which == "other_table and x_inout" else 0, 1)
    dev = float(np.abs(x.astype(np.float64) - d["r64"][0]).max())
    dev_loss = float(np.abs(lv.astype(np.float64) - d["r64"][1]).max())
    print(f"\nunaligned {which}, case {ac.CASE_IDS[i]}: kernel {dev:.3e} E32 {d['e32']:.3e} ratio {dev / d['e32']:.2f} | "
          f"loss kernel {dev_loss:.3e} E32 {d['e32_loss']:.3e} ratio {dev_loss / d['e32_loss']:.2f}")
    empty = np.diff(case["ptr"]) == 0
    assert not x[empty].any() and not lv[empty].any()
    assert np.isfinite(x).all() and np.isfinite(lv).all()
    assert dev <= 2 * d["e32"]
    assert dev_loss <= 2 * d["e32_loss"]
    if case["dim"] == 24:
        x0, lv0 = run_views(case, d["cg"], 0, 0)
        assert x.tobytes() == x0.tobytes() and lv.tobytes() == lv0.tobytes()


class _Resident:
    """A case's arrays on the device once, for many calls of the entry itself on subsets of its rows."""

    def __init__(self, case):
        self.case, self.n, self.dim = case, case["rows"], case["dim"]
        self.Y, self.G = t(case["Y"]).to(DEV), t(case["G"]).to(DEV)
        self.ptr, self.idx = t(case["ptr"]).to(DEV), t(case["idx"]).to(DEV)
        self.val = None if case["val"] is None else t(case["val"]).to(DEV)

    def solve(self, cg, calls):
        """x and the loss (host) after one call per entry of ``calls`` (None: every row; else the
        row ids of that call) on a fresh copy of the start; guard elements follow both."""
        n, dim, p = self.n, self.dim, _lib.ptr
        xbuf = torch.full((n * dim + GUARD,), -7.0, dtype=torch.float32, device=DEV)
        lbuf = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device=DEV)
        xbuf[:n * dim].copy_(t(self.case["X0"]).reshape(-1))
        lib, stream = _lib.load(), _lib.stream_handle()
        held = []                                     # the row ids stay allocated until the last call has run
        for rows in calls:
            rows_d = None if rows is None else t(np.ascontiguousarray(rows, np.int64)).to(DEV)
            held.append(rows_d)
            rc = lib.rg_als_solve_rows(stream, p(self.Y), p(self.G), dim, p(self.ptr), p(self.idx), p(self.val),
                                       float(self.case["alpha"]), p(rows_d), n if rows is None else len(rows), cg,
                                       p(xbuf), p(lbuf))
            assert rc == 0, lib.rg_last_error()
        torch.cuda.synchronize()
        x, lv = xbuf.cpu().numpy(), lbuf.cpu().numpy()
        assert (x[n * dim:] == -7.0).all() and (lv[n:] == -7.0).all(), "elements past x_inout or loss_out written"
        return x[:n * dim].reshape(n, dim), lv[:n]


def _second_trip_check(case, cg, sample, what):
    """One call on all rows against calls of at most 130 rows each (the regime the parity cases hold
    to float64; a row's bits do not depend on its call), and ``sample`` against the restatement."""
    res = _Resident(case)
    n = case["rows"]
    x, lv = res.solve(cg, [None])
    xs, ls = res.solve(cg, [np.arange(s, min(s + 130, n)) for s in range(0, n, 130)])
    assert x.tobytes() == xs.tobytes() and lv.tobytes() == ls.tobytes()
    d = ac.measure(ac.sub_case(case, sample), cg)
    assert d["admitted"], (d["e32"], d["xmax"])
    dev = float(np.abs(x[sample].astype(np.float64) - d["r64"][0]).max())
    dev_loss = float(np.abs(lv[sample].astype(np.float64) - d["r64"][1]).max())
    print(f"\n{what}: kernel {dev:.3e} E32 {d['e32']:.3e} ratio {dev / d['e32']:.2f} | "
          f"loss kernel {dev_loss:.3e} E32 {d['e32_loss']:.3e} ratio {dev_loss / d['e32_loss']:.2f}")
    assert dev <= 2 * d["e32"]
    assert dev_loss <= 2 * d["e32_loss"]


@pytest.mark.parametrize("dim", [16, 128])
def test_short_rows_beyond_one_trip_of_the_grid_keep_their_bits(dim):
    """als_short_kernel's workgroups stride over the tiles: its grid is capped (als_common.
    short_grid_cap), every workgroup solves 8 tiles per trip (one per wave) and a tile is 64 / LPU
    rows, so a call of more than cap * 8 * tile rows sends workgroups on a second trip with the staged
    G and their p slots reused.  An eighth of them here, and the last tile is partial."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap, tile = ac.short_grid_cap(dim, cus)
    one_trip = cap * ac.WAVES * tile
    n = one_trip + one_trip // 8 + 5
    assert n > one_trip and -(-n // tile) > cap * ac.WAVES
    lens = np.random.RandomState(dim).randint(0, 6, n)
    case = ac.make_case(dim, n, 0.1, 40.0, True, "random", lens=lens)
    mid = n // 2
    sample = np.r_[0:86, mid:mid + 85, n - 85:n]
    assert len(sample) == 256
    _second_trip_check(case, 3, sample, f"short rows dim {dim}: {n} rows, one trip holds {one_trip}, sample of 256")


@pytest.mark.parametrize("dim", [16, 128])
def test_long_rows_beyond_one_trip_of_the_grid_keep_their_bits(dim):
    """als_long_kernel's workgroups stride over the call's rows and skip the short ones: its grid is
    min(rows, m * CUs) with m in 1 .. 4 by the LDS of the layout (als_common.long_grid_cap).  Rows j
    and j + 12 CUs fall to the same workgroup whatever m is (12 is a multiple of each), with 12 CUs
    / (m CUs) - 1 skipped short rows between its two solves; the pair's lists differ in length, so
    the reduction scratch of the first solve is overwritten by a different chunking."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = ac.long_grid_cap(dim, cus)
    firsts = [0, 1, 2, cus // 2, cus - 1, cus + 3]
    n = 12 * cus + max(firsts) + 1 + 7
    assert n > 4 * cus >= grid and all((j + 12 * cus) % (m * cus) == j % (m * cus) for j in firsts for m in (1, 2, 3, 4))
    lens = np.random.RandomState(dim + 1).randint(0, 2, n)
    T = ac.T
    pairs = [(T, T + 1), (T + 1, 3 * T + 5), (3 * T + 5, T), (T, 3 * T + 5), (T + 1, T), (3 * T + 5, T + 1)]
    long_rows = []
    for j, (a, b) in zip(firsts, pairs):
        lens[j], lens[j + 12 * cus] = a, b
        long_rows += [j, j + 12 * cus]
    assert len(long_rows) == 12 and (lens >= T).sum() == 12
    case = ac.make_case(dim, n, 0.1, 40.0, True, "random", True, lens=lens)
    sample = np.array(sorted(long_rows) + [r for r in range(3, 200) if r not in long_rows][:116])
    _second_trip_check(case, 3, sample, f"long rows dim {dim}: {n} rows on a grid of {grid}, 12 long rows and 116 others")


def test_loss_out_has_its_own_guard_and_is_optional():
    case = ac.make_case(16, 5, 0.1, 1.0, True, "random", True)
    n, dim = 5, 16
    lib = _lib.load()
    Y, G = t(case["Y"]).to(DEV), t(case["G"]).to(DEV)
    ptr, idx, val = t(case["ptr"]).to(DEV), t(case["idx"]).to(DEV), t(case["val"]).to(DEV)
    x = t(case["X0"]).to(DEV).clone()
    lbuf = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device=DEV)
    p = _lib.ptr
    assert lib.rg_als_solve_rows(_lib.stream_handle(), p(Y), p(G), dim, p(ptr), p(idx), p(val), 1.0, None, n, 3, p(x),
                                 p(lbuf)) == 0
    torch.cuda.synchronize()
    got = lbuf.cpu().numpy()
    assert (got[n:] == -7.0).all() and (got[:n] != -7.0).all()
    x2, _ = run(case, 3, return_loss=False)
    assert x2.tobytes() == x.cpu().numpy().tobytes()


@pytest.mark.parametrize("dim, values", [(16, True), (65, False), (128, True)])
def test_a_rows_bits_do_not_depend_on_its_place_in_the_call(dim, values):
    case = ac.make_case(dim, 130, 0.1, 40.0, values, "random", True, seed=3)
    cg, n = 3, 130
    lens = np.diff(case["ptr"])
    assert (lens >= ac.T).sum() >= 3 and (lens == ac.T - 1).any() and ((lens > 0) & (lens < ac.T)).sum() > 50
    full = run(case, cg)
    # every row alone: the other rows keep their start
    for r in range(n):
        x, lv = run(case, cg, rows=[r])
        assert x[r].tobytes() == full[0][r].tobytes() and lv[r].tobytes() == full[1][r].tobytes(), f"row {r} alone"
        others = np.arange(n) != r
        assert x[others].tobytes() == case["X0"][others].tobytes()
    # a shuffled permutation, and the rows sorted by length
    for perm in (np.random.RandomState(5).permutation(n), np.argsort(lens, kind="stable")):
        x, lv = run(case, cg, rows=perm)
        assert x.tobytes() == full[0].tobytes() and lv.tobytes() == full[1].tobytes()
    # every third row kept, the other rows' lists (and lengths) replaced
    keep = np.arange(0, n, 3)
    other = np.setdiff1d(np.arange(n), keep)
    lens2 = lens.copy()
    lens2[other] = np.random.RandomState(9).randint(0, 2 * ac.T, len(other))
    changed = ac.make_case(dim, n, 0.1, 40.0, values, "random", True, seed=4, lens=lens2)
    changed["Y"], changed["G"] = case["Y"], case["G"]
    for r in keep:
        a, b = changed["ptr"][r], changed["ptr"][r + 1]
        changed["idx"][a:b] = case["idx"][case["ptr"][r]:case["ptr"][r + 1]]
        if values:
            changed["val"][a:b] = case["val"][case["ptr"][r]:case["ptr"][r + 1]]
        changed["X0"][r] = case["X0"][r]
    x, lv = run(changed, cg)
    assert x[keep].tobytes() == full[0][keep].tobytes() and lv[keep].tobytes() == full[1][keep].tobytes()


@pytest.mark.parametrize("n, dim, lam", [(130, 128, 0.0), (1000, 16, 0.1), (1025, 65, 1.0), (2500, 128, 0.01),
                                         (3000, 64, 0.1)])
def test_gram_is_within_twice_a_float32_matmul_of_float64_and_repeats_bit_for_bit(n, dim, lam):
    rs = np.random.RandomState(n + dim)
    tab = (rs.randn(n, dim) * 0.7).astype(np.float32)
    ref = tab.astype(np.float64).T @ tab.astype(np.float64) + lam * np.eye(dim)
    e32 = float(np.abs((tab.T @ tab + np.float32(lam) * np.eye(dim, dtype=np.float32)).astype(np.float64) - ref).max())
    d = t(tab).to(DEV)
    a, b = als.gram(d, lam), als.gram(d, lam)
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    dev = float(np.abs(a.astype(np.float64) - ref).max())
    print(f"\ngram n {n} dim {dim}: kernel {dev:.3e} E32 {e32:.3e} ratio {dev / e32:.2f}")
    assert a.tobytes() == b.tobytes()
    assert (a == a.T).all()
    assert dev <= 2 * e32


@pytest.mark.parametrize("n, dim, lam", [(1, 1, 0.5), (5, 3, 0.01), (17, 8, 0.0)])
def test_gram_of_a_tiny_table(n, dim, lam):
    """Too few elements for a measured bound to mean anything: the textbook one instead, n + 1
    roundings of at most 2^-24 relative each on the sum of the terms' magnitudes."""
    rs = np.random.RandomState(n + dim)
    tab = (rs.randn(n, dim) * 0.7).astype(np.float32)
    t64 = tab.astype(np.float64)
    ref = t64.T @ t64 + lam * np.eye(dim)
    bound = (n + 1) * 2.0 ** -24 * (np.abs(t64).T @ np.abs(t64) + lam * np.eye(dim))
    a = als.gram(t(tab).to(DEV), lam).cpu().numpy()
    assert (np.abs(a.astype(np.float64) - ref) <= bound).all() and (a == a.T).all()


@pytest.mark.parametrize("dim", [16, 65])
def test_zero_cg_steps_leave_rows_zero_the_empty_ones_and_fill_the_loss(dim):
    case = ac.make_case(dim, 130, 0.1, 40.0, True, "random", True, seed=6)
    x, lv = run(case, 0)
    empty = np.diff(case["ptr"]) == 0
    assert empty.any() and case["X0"][empty].any()
    assert x[~empty].tobytes() == case["X0"][~empty].tobytes()
    assert not x[empty].any()
    r64 = ac.numpy_als_rows(case, 0)
    r32 = [ac.numpy_als_rows(case, 0, np.float32, o) for o in ac.ORDERS]
    _, e32_loss, _ = ac.e32_of(r64, r32)
    dev = float(np.abs(lv.astype(np.float64) - r64[1]).max())
    print(f"\ncg 0 dim {dim}: loss kernel {dev:.3e} E32 {e32_loss:.3e} ratio {dev / e32_loss:.2f}")
    assert dev <= 2 * e32_loss


def test_objective_on_the_device_equals_the_float64_brute_force():
    f = ac.fit_data()
    X, Y = f["r64"][0]
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    want = ac.objective64(X32, Y32, f["csr_u"], 40.0, 0.1)
    got = als.objective(t(X32).to(DEV), t(Y32).to(DEV), tuple(None if a is None else t(a) for a in f["csr_u"]), 40.0, 0.1)
    assert abs(got - want) <= 1e-5 * abs(want)


def _model(tmp_path, monkeypatch, f, dim=16):
    from recommendation_gans_amd.implicit import ImplicitFactorizationModel
    from recommendation_gans_amd.spotlight.interactions import Interactions
    monkeypatch.chdir(tmp_path)
    p = ac.FIT
    train = Interactions(f["users"], f["items"], ratings=np.ones(len(f["users"]), np.float32), num_users=p["users"],
                         num_items=p["items"])
    model = ImplicitFactorizationModel(embedding_dim=dim, use_cuda=True, random_state=np.random.RandomState(0))
    model._initialize(train)
    model._engine.set_params(t(f["X0"]), t(f["Y0"]), torch.ones(p["users"]), torch.ones(p["items"]))
    return model, train


def test_fit_als_end_to_end(tmp_path, monkeypatch):
    f, p = ac.fit_data(), ac.FIT
    model, train = _model(tmp_path, monkeypatch, f)
    # sweep by sweep first, for the descent check on the kernel's own tables
    objs = []
    for s in range(1, p["sweeps"] + 1):
        m2, _ = _model(tmp_path, monkeypatch, f)
        m2.fit_als(train, iterations=s, regularization=p["lam"], alpha=p["alpha"], cg_steps=p["cg"])
        X, Y, ub, ib = [a.cpu().numpy() for a in m2._engine.params()]
        objs.append(ac.objective64(X, Y, f["csr_u"], p["alpha"], p["lam"]))
        assert abs(m2.als_losses[-1] - objs[-1]) <= 1e-5 * objs[-1] and len(m2.als_losses) == s
    start = ac.objective64(f["X0"], f["Y0"], f["csr_u"], p["alpha"], p["lam"])
    print(f"\nfit_als float64 objective: start {start:.4f} then {objs}")
    for before, after in zip([start] + objs[:-1], objs):
        assert after <= before * (1 + 1e-5)
    assert not ub.any() and not ib.any()
    X64, Y64 = f["r64"][-1]
    dev = max(float(np.abs(X - X64).max()), float(np.abs(Y - Y64).max()))
    print(f"fit_als tables: kernel {dev:.3e} E32 {f['e32']:.3e} ratio {dev / f['e32']:.2f}")
    assert dev <= 2 * f["e32"]
    for prm, tab in zip(m2._params, (X, Y, ub, ib)):                     # the net holds the same tables
        assert prm.detach().cpu().numpy().reshape(tab.shape).tobytes() == tab.tobytes()

    # the serving layer on the fitted model
    k = 10
    users = np.arange(p["users"])
    ids = m2.recommend(users, k=k)
    S = X.astype(np.float64) @ Y.astype(np.float64).T
    order = np.argsort(-S, axis=1, kind="stable")
    top = np.take_along_axis(S, order[:, :k + 1], axis=1)
    gap = (top[:, :-1] - top[:, 1:]) / np.maximum(np.abs(top[:, :-1]), 1e-300)
    tied = (gap < ac.TIE).any(axis=1)
    print(f"recommend: {tied.sum()} of {len(users)} rows left out")
    assert tied.mean() <= 0.01
    assert (ids[~tied] == order[~tied, :k]).all()
    sim = m2.similar_items(np.arange(5), k=5)
    assert sim.shape == (5, 5)
    cand = np.random.RandomState(3).randint(0, p["items"], (p["users"], 20))
    ranked = m2.rank_candidates(users, cand, k=5)
    assert ranked.shape == (p["users"], 5)


def test_fold_in_users_als_is_solve_rows_from_zero_and_recommend_for_histories_takes_a_method(tmp_path, monkeypatch):
    f, p = ac.fit_data(), ac.FIT
    model, train = _model(tmp_path, monkeypatch, f)
    model.fit_als(train, iterations=2, regularization=p["lam"], alpha=p["alpha"], cg_steps=p["cg"])
    rs = np.random.RandomState(2)
    hist = [rs.choice(p["items"], size=rs.randint(0, 40), replace=False) for _ in range(37)]
    hist[5] = np.zeros(0, np.int64)
    hist[6] = rs.randint(0, p["items"], 2 * ac.T)                       # the workgroup path, duplicates
    W, b = model.fold_in_users_als(hist)
    assert W.shape == (37, 16) and W.dtype == np.float32 and b.shape == (37,) and not b.any() and not W[5].any()
    Y = model._engine.params()[1]
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in hist])]).astype(np.int64)
    idx = np.concatenate(hist).astype(np.int32)
    x = torch.zeros(37, 16, device=DEV)
    als.solve_rows(Y, als.gram(Y, p["lam"]), t(ptr), t(idx), None, p["alpha"], 16, x, checked=True)
    assert x.cpu().numpy().tobytes() == W.tobytes()
    W2, _ = model.fold_in_users_als(hist, regularization=1.0, alpha=1.0, cg_steps=2)
    assert W2.tobytes() != W.tobytes()
    ids = model.recommend_for_histories(hist, 5, method="als")
    S = W.astype(np.float64) @ Y.cpu().numpy().astype(np.float64).T
    for r in range(37):
        S[r, hist[r]] = -np.inf
        assert not np.isin(ids[r], hist[r]).any()
    assert (np.sort(np.take_along_axis(S, ids, 1), axis=1)[:, ::-1] >= np.sort(S, axis=1)[:, ::-1][:, :5] - 1e-5).all()
    # "adam" is the call without method, bit for bit
    a = model.recommend_for_histories(hist[:6], 5, return_scores=True, steps=4, random_state=np.random.RandomState(5))
    c = model.recommend_for_histories(hist[:6], 5, return_scores=True, method="adam", steps=4,
                                      random_state=np.random.RandomState(5))
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()
