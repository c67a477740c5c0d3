"""The pooling sequence model on the GPU: rg_seq_pool_grads against the float64 oracle under
fold_in_common's rule (tests/seq_common.py), rg_seq_adam_dense against torch's op sequence, five
free-running steps beside the float64 oracle, rg_seq_pool_repr / predict / recommend_next against
the fixture and the oracle, sequence_mrr_score's device path against its host loop, the entries'
refusals, and an end-to-end fit; the kernels again on tables that start off a 16-byte boundary, the
Adam pass on a table larger than one trip of its grid, and the entries' stated edges (padding
anywhere, ids outside the table, empty sequences, L = 1024 with K = 16).  Every case in a few seconds.
"""
import ctypes

import numpy as np
import pytest
import torch

from recommendation_gans_amd import _lib, seq_engine
from recommendation_gans_amd.spotlight import evaluation
from recommendation_gans_amd.spotlight.interactions import SequenceInteractions
from recommendation_gans_amd.spotlight.sequence import ImplicitSequenceModel
from recommendation_gans_amd.synthetic import generate_sequential
from tests import seq_common as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS32 = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=sc.CASE_IDS)
def test_pool_grads_against_the_float64_oracle(i):
    data = sc.case_data(i)
    case, loss = data["case"], data["loss"]
    lv, grad = seq_engine.pool_grads(_dev(case["E"]), _dev(case["b"]), _dev(case["seq"]), _dev(case["neg"]), loss)
    lv, grad = float(lv), grad.cpu().numpy()
    d = case["d"]
    assert grad.dtype == np.float32 and grad.shape == (case["num_items"], d + 1) and np.isfinite(grad).all()
    ref = data["r64"]
    rel_loss = abs(lv - ref["loss"]) / abs(ref["loss"])
    worst, plain = sc.gradient_excess(grad[:, :d], grad[:, d], data)
    print(f"\ncase {sc.CASE_IDS[i]}: loss rel {rel_loss:.2e} | gradient: E32 {data['e32']:.3e} "
          f"kernel / E32 {plain:.2f} kernel / bound {worst:.3f}")
    assert not grad[0].any()                                   # the padding row, bits
    assert rel_loss <= 1e-5
    assert worst <= 1.0


def test_the_loss_is_the_same_bits_on_every_run():
    case = sc.make_case(64, 33, 257, 5, 7)
    args = [_dev(case[k]) for k in ("E", "b", "seq", "neg")]
    a = [seq_engine.pool_grads(*args, "bpr") for _ in range(3)]
    assert len({float(x[0]) for x in a}) == 1
    # the gradients agree to rounding (float atomics: the order of a row's sums is not fixed)
    g0 = a[0][1].cpu().numpy().astype(np.float64)
    for _, g in a[1:]:
        assert np.abs(g.cpu().numpy() - g0).max() <= 1e-5 * np.abs(g0).max()


GUARD = 64


def _view(host, off, guard=GUARD):
    """``host`` as a contiguous device view ``off`` floats into a buffer of -7 (guards on both
    sides): returns (buffer, view)."""
    host = np.ascontiguousarray(host)
    buf = torch.full((off + host.size + guard,), -7.0, dtype=torch.float32, device=DEV)
    view = buf[off:off + host.size].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return buf, view


def _guards_hold(buf, off, size):
    got = buf.cpu().numpy()
    return (got[:off] == -7.0).all() and (got[off + size:] == -7.0).all()


@pytest.mark.parametrize("i", sc.UNALIGNED, ids=[sc.CASE_IDS[i] for i in sc.UNALIGNED])
def test_pool_grads_on_a_table_off_a_16_byte_boundary(i):
    """The unaligned dispatch (dispatch_rows' scalar layouts) under the oracle test's own rule; at
    d 24 the aligned call selects the same layout, so the loss (fixed-order sums) has its bits."""
    data = sc.case_data(i)
    case, loss, d = data["case"], data["loss"], data["case"]["d"]
    ebuf, E = _view(case["E"], 1)
    lv, grad = seq_engine.pool_grads(E, _dev(case["b"]), _dev(case["seq"]), _dev(case["neg"]), loss)
    lv32, lv, grad = lv.cpu().numpy(), float(lv), grad.cpu().numpy()
    assert ebuf.cpu().numpy()[1:1 + E.numel()].tobytes() == case["E"].tobytes() and _guards_hold(ebuf, 1, E.numel())
    ref = data["r64"]
    rel_loss = abs(lv - ref["loss"]) / abs(ref["loss"])
    worst, plain = sc.gradient_excess(grad[:, :d], grad[:, d], data)
    print(f"\nunaligned E, case {sc.CASE_IDS[i]}: loss rel {rel_loss:.2e} | gradient: E32 {data['e32']:.3e} "
          f"kernel / E32 {plain:.2f} kernel / bound {worst:.3f}")
    assert np.isfinite(grad).all() and not grad[0].any()
    assert rel_loss <= 1e-5
    assert worst <= 1.0
    if d == 24:
        lv0, _ = seq_engine.pool_grads(_dev(case["E"]), _dev(case["b"]), _dev(case["seq"]), _dev(case["neg"]), loss)
        assert lv0.cpu().numpy().tobytes() == lv32.tobytes()


def _adam_dense_against_torchs_op_sequence(N, d, step, l2, what):
    rs = np.random.RandomState(10 * step + int(l2 > 0))
    lr = 1e-2
    E, b = sc.make_tables(N, d, rs)
    g = (rs.randn(N, d + 1) * 1e-3).astype(np.float32)
    g[5] *= 1e-6                                              # |g| near eps
    g[0] = 0.0
    m = (rs.randn(N, d + 1) * 1e-3).astype(np.float32) if step > 1 else np.zeros((N, d + 1), np.float32)
    v = (rs.rand(N, d + 1) * 1e-6).astype(np.float32) if step > 1 else np.zeros((N, d + 1), np.float32)
    m[0] = v[0] = 0.0
    tens = dict(E=_dev(E), b=_dev(b), mE=_dev(m[:, :d]), vE=_dev(v[:, :d]), mb=_dev(m[:, d]), vb=_dev(v[:, d]),
                grad=_dev(g))
    seq_engine.adam_dense(tens["E"], tens["b"], tens["mE"], tens["vE"], tens["mb"], tens["vb"], tens["grad"], step, lr,
                          weight_decay=l2)
    got = {k: t.cpu().numpy() for k, t in tens.items()}
    assert not got["grad"].any()                               # zeroed for the next step
    t = torch.from_numpy
    for name, p0, g0, m0, v0, keys in (("E", E, g[:, :d], m[:, :d], v[:, :d], ("E", "mE", "vE")),
                                       ("b", b, g[:, d], m[:, d], v[:, d], ("b", "mb", "vb"))):
        refs = [sc.adam_formula_step(t(p0.copy()), t(np.ascontiguousarray(g0)), t(np.ascontiguousarray(m0)),
                                     t(np.ascontiguousarray(v0)), step, lr, l2, cr) for cr in (False, True)]
        up = np.minimum(sc.ulps(got[keys[0]][1:], refs[0][0].numpy()[1:]), sc.ulps(got[keys[0]][1:], refs[1][0].numpy()[1:]))
        um = sc.ulps(got[keys[1]][1:], refs[0][1].numpy()[1:])
        uv = sc.ulps(got[keys[2]][1:], refs[0][2].numpy()[1:])
        print(f"\nadam{what} step {step} l2 {l2} {name}: max ulp p {up.max()} m {um.max()} v {uv.max()}")
        assert up.max() <= 1 and um.max() <= 1 and uv.max() <= 1
        # row 0 is untouched, parameters and moments
        for k, start in zip(keys, (p0, m0, v0)):
            assert got[k][0].tobytes() == np.ascontiguousarray(start[0]).tobytes()
        assert (got[keys[0]][1:] != p0[1:]).any()
    return E, b, got


@pytest.mark.parametrize("l2", [0.0, 1e-3])
@pytest.mark.parametrize("step", [1, 7])
def test_adam_dense_is_torchs_op_sequence(step, l2):
    _adam_dense_against_torchs_op_sequence(301, 20, step, l2, "")


@pytest.mark.parametrize("step", [1, 7])
def test_adam_dense_beyond_one_trip_of_the_grid(step):
    """seq_adam_kernel launches at most 8 * CUs blocks of 256 threads, which stride over the
    num_items * (d + 1) elements: a table with more elements than that sends threads on a second
    trip (here 60 rows' worth of them), with element numbers past 2^19 split into row and column."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    d, one_trip = 256, 8 * cus * 256
    N = one_trip // (d + 1) + 60
    assert N * (d + 1) > one_trip
    E, b, got = _adam_dense_against_torchs_op_sequence(N, d, step, 1e-3, f" {N} x {d + 1} > {one_trip}")
    # the last row, and the last columns of every row behind the first trip, were updated (an update
    # below half an ulp of its parameter is possible, so nearly all of them rather than all)
    later = one_trip // (d + 1) + 1
    assert later * (d + 1) >= one_trip and N - later >= 50
    assert (got["E"][N - 1] != E[N - 1]).mean() > 0.99 and got["b"][N - 1] != b[N - 1]
    assert (got["E"][later:, d - 1] != E[later:, d - 1]).mean() > 0.9 and (got["b"][later:] != b[later:]).mean() > 0.9


def test_five_free_running_steps_beside_the_float64_oracle():
    d, L, B, N, lr = 32, 5, 64, 200, 1e-2
    rs = np.random.RandomState(11)
    E, b = sc.make_tables(N, d, rs)
    seqs = sc.make_sequences(5 * B, L, N, rs)
    model = ImplicitSequenceModel(loss="bpr", embedding_dim=d, batch_size=B, learning_rate=lr,
                                  random_state=np.random.RandomState(42))
    model.set_tables(E, b, device=DEV)
    host = np.random.RandomState(42)
    oracle = sc.Oracle(E, b, "bpr", lr)
    for s in range(5):
        batch = seqs[s * B:(s + 1) * B]
        got = float(model.train_batch(_dev(batch)))
        neg = host.randint(0, N, (B, L), dtype=np.int64).reshape(1, B, L)
        ref = oracle.step(batch, neg)
        print(f"\nstep {s}: kernel {got:.8f} float64 {ref:.8f} rel {abs(got - ref) / abs(ref):.2e}")
        assert abs(got - ref) <= 1e-5 * abs(ref)
    assert model._random_state.randint(0, 1 << 30) == host.randint(0, 1 << 30)
    assert not model.item_embeddings[0].any() and model.item_biases[0] == 0
    dE = np.abs(model.item_embeddings.cpu().numpy() - oracle.E.detach().numpy()).max()
    print(f"tables after 5 steps: max |kernel - float64| {dE:.3e}")


def test_fit_is_train_batch_over_shuffled_minibatches():
    inter = generate_sequential(40, 50, 600, 0.05, 1, np.random.RandomState(1)).to_sequence(5)
    a = ImplicitSequenceModel(loss="adaptive_hinge", embedding_dim=8, n_iter=2, batch_size=32,
                              random_state=np.random.RandomState(3), num_negative_samples=3)
    torch.manual_seed(0)
    a.fit(inter)
    assert a._step == 2 * -(-len(inter) // 32)
    host = np.random.RandomState(3)
    for _ in range(2):
        order = np.arange(len(inter))
        host.shuffle(order)
        for i in range(0, len(inter), 32):
            host.randint(0, 50, (3 * len(order[i:i + 32]), 5))
    assert a._random_state.randint(0, 1 << 30) == host.randint(0, 1 << 30)
    with pytest.raises(ValueError, match="number of items"):
        a.fit(SequenceInteractions(np.array([[1, 2, 3, 4, 50]]), num_items=51))


def _ragged(seq):
    lens = (seq != 0).sum(1)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), seq[seq != 0]


def test_pool_repr_and_predict_reproduce_the_reference_fixture():
    fx = sc.load_fixture()
    E = _dev(fx["E"])
    R = seq_engine.pool_repr(E, _dev(fx["sequences"])).cpu().numpy()
    assert np.abs(R - fx["final"]).max() <= 1e-6 * np.abs(fx["final"]).max()
    ptr, ids = _ragged(fx["sequences"])
    R2 = seq_engine.pool_repr(E, _dev(ids), seq_ptr=ptr).cpu().numpy()
    assert np.abs(R2 - fx["final"]).max() <= 1e-6 * np.abs(fx["final"]).max()
    model = ImplicitSequenceModel(embedding_dim=8)
    model.set_tables(fx["E"], fx["b"], device=DEV)
    ref = sc.final_scores(torch.from_numpy(fx["E"]).double(), torch.from_numpy(fx["b"]).double(),
                          torch.from_numpy(fx["sequences"])).numpy()
    for r in range(len(fx["sequences"])):
        p = model.predict(fx["sequences"][r])
        assert p.dtype == np.float32 and p.shape == (23,)
        assert np.abs(p - ref[r]).max() <= 1e-6 * np.abs(ref[r]).max()
        some = model.predict(fx["sequences"][r], item_ids=np.array([[3], [1], [22]]))
        assert some.tobytes() == p[[3, 1, 22]].tobytes()


def repr_entry(E, ids, ptr, L, n, out, num_items):
    """rg_seq_pool_repr itself (``pool_repr`` makes its own aligned ``out`` and checks the ids)."""
    lib, p = _lib.load(), _lib.ptr
    rc = lib.rg_seq_pool_repr(_lib.stream_handle(), p(E), int(E.shape[1]), num_items, p(ids), p(ptr), L, n, p(out))
    assert rc == 0, lib.rg_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["E and out", "out alone"])
@pytest.mark.parametrize("d", [8, 16, 64, 128, 24])
def test_pool_repr_on_tables_off_a_16_byte_boundary(d, which):
    """The unaligned dispatch (dispatch_rows' scalar layouts) inside the oracle test's own bound,
    padded and ragged; at d 24 the aligned call selects the same layout and gives the same bits."""
    n, L, N = 67, 33, 257
    rs = np.random.RandomState(n + L + d)
    E, _ = sc.make_tables(N, d, rs)
    seq = sc.make_sequences(n, L, N, rs)
    _, ref = sc.representations(torch.from_numpy(E).double(), torch.from_numpy(seq))
    ref = ref.numpy()
    bound = (L + 1) * EPS32 * np.abs(E).max() + 1e-30
    ptr, ids = _ragged(seq)
    off_e = 1 if which == "E and out" else 0
    ebuf, Ed = _view(E, off_e)
    for form, args in (("padded", (_dev(seq), None, L)), ("ragged", (_dev(ids), _dev(ptr), 0))):
        obuf, out = _view(np.zeros((n, d), np.float32), 1)
        repr_entry(Ed, *args, n, out, N)
        R = out.cpu().numpy()
        err = np.abs(R - ref).max()
        print(f"\nunaligned {which}, d {d} {form}: max err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert _guards_hold(obuf, 1, out.numel()) and _guards_hold(ebuf, off_e, Ed.numel())
        assert err <= bound
        if d == 24:
            aligned = torch.empty(n, d, device=DEV)
            repr_entry(_dev(E), *args, n, aligned, N)
            assert aligned.cpu().numpy().tobytes() == R.tobytes()
    assert ebuf.cpu().numpy()[off_e:off_e + Ed.numel()].tobytes() == E.tobytes()


@pytest.mark.parametrize("name, d, loss", sc.EDGE_CASES)
def test_pool_grads_at_the_entrys_edges_against_the_float64_oracle(name, d, loss):
    """Padding anywhere in a sequence (one row ends in it), zeros where the next test puts ids outside
    the table, rows of padding alone, and L = 1024 with K = 16 (the workspace's largest strides):
    each under the oracle test's own rule.  The longest case is followed by its representations."""
    data = sc.edge_data(name, d, loss)
    case = data["case"]
    N = case["num_items"]
    E = _dev(case["E"])
    lv, grad = seq_engine.pool_grads(E, _dev(case["b"]), _dev(case["seq"]), _dev(case["neg"]), loss)
    lv, grad = float(lv), grad.cpu().numpy()
    ref = data["r64"]
    rel_loss = abs(lv - ref["loss"]) / abs(ref["loss"])
    worst, plain = sc.gradient_excess(grad[:, :d], grad[:, d], data)
    print(f"\nedge {name} d {d} {loss}: loss rel {rel_loss:.2e} | gradient: E32 {data['e32']:.3e} "
          f"kernel / E32 {plain:.2f} kernel / bound {worst:.3f}")
    assert np.isfinite(grad).all() and not grad[0].any()
    assert rel_loss <= 1e-5
    assert worst <= 1.0
    seq = case["seq"]
    if name == "empty":
        # a row of padding alone adds no partial: without the last row (one of them) the partials
        # before it stand where they stood and the loss has the same bits
        a = seq_engine.pool_grads(E, _dev(case["b"]), _dev(seq), _dev(case["neg"]), loss)[0]
        b = seq_engine.pool_grads(E, _dev(case["b"]), _dev(seq[:-1]), _dev(case["neg"][:, :-1]), loss)
        assert a.cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
        g2 = b[1].cpu().numpy().astype(np.float64)
        assert np.abs(g2 - grad).max() <= 1e-5 * np.abs(grad).max()
    # the same sequences through rg_seq_pool_repr, padded and ragged
    L = seq.shape[1]
    _, r64 = sc.representations(torch.from_numpy(case["E"]).double(), torch.from_numpy(seq))
    bound = (L + 1) * EPS32 * np.abs(case["E"]).max() + 1e-30
    ptr, ids = _ragged(seq)
    for form, R in (("padded", seq_engine.pool_repr(E, _dev(seq))),
                    ("ragged", seq_engine.pool_repr(E, _dev(ids), seq_ptr=ptr))):
        err = np.abs(R.cpu().numpy() - r64.numpy()).max()
        print(f"edge {name} d {d} representations {form}: max err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert err <= bound
        assert not R.cpu().numpy()[(seq != 0).sum(1) == 0].any()


@pytest.mark.parametrize("d, loss", [(8, "hinge"), (64, "bpr")])
def test_ids_outside_the_table_are_read_as_padding(d, loss):
    """include/rg_hip.h: "an id outside [0, num_items) is read as padding".  The padding zeros of
    seq and a tenth of neg become num_items, num_items + 5, -1 and 2^40; inv_count stays the
    caller's count of the ids in range.  The fixed-order sums (loss, representations) have the bits
    of the call with zeros there, the atomic gradient agrees to rounding, and neither the guard
    rows behind grad nor E's buffer change."""
    out, ins = sc.edge_case("outside", d), sc.edge_case("inside", d)
    N, rows = out["num_items"], 3
    count = int((ins["seq"] != 0).sum())
    assert count == int(((out["seq"] > 0) & (out["seq"] < N)).sum())
    ebuf, E = _view(out["E"], 0, guard=rows * d)
    b = _dev(out["b"])
    got = []
    for case in (out, ins):
        gbuf = torch.full(((N + rows) * (d + 1),), -7.0, dtype=torch.float32, device=DEV)
        grad = gbuf[:N * (d + 1)].view(N, d + 1).zero_()
        lv, _ = seq_engine.pool_grads(E, b, _dev(case["seq"]), _dev(case["neg"]), loss, grad=grad, mask_count=count,
                                      checked=True)
        torch.cuda.synchronize()
        assert (gbuf[N * (d + 1):].cpu().numpy() == -7.0).all(), "rows behind grad written"
        got.append((lv.cpu().numpy(), grad.cpu().numpy()))
    assert got[0][0].tobytes() == got[1][0].tobytes()
    g_out, g_in = got[0][1].astype(np.float64), got[1][1].astype(np.float64)
    assert not g_out[0].any() and np.abs(g_out - g_in).max() <= 1e-5 * np.abs(g_in).max()
    # the call with zeros there is itself held to the oracle (the edge test above); so is this one
    data = sc.edge_data("inside", d, loss)
    worst, plain = sc.gradient_excess(got[0][1][:, :d], got[0][1][:, d], data)
    print(f"\nids outside d {d} {loss}: gradient: E32 {data['e32']:.3e} kernel / E32 {plain:.2f} "
          f"kernel / bound {worst:.3f}")
    assert worst <= 1.0
    ptr, _ = _ragged(ins["seq"])
    kept = out["seq"][ins["seq"] != 0]
    for a, z in ((seq_engine.pool_repr(E, _dev(out["seq"]), checked=True), seq_engine.pool_repr(E, _dev(ins["seq"]))),
                 (seq_engine.pool_repr(E, _dev(out["seq"].reshape(-1)), seq_ptr=np.arange(len(ptr)) * out["L"],
                                       checked=True),
                  seq_engine.pool_repr(E, _dev(kept), seq_ptr=ptr))):
        assert a.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()
    eb = ebuf.cpu().numpy()
    assert eb[:E.numel()].tobytes() == out["E"].tobytes() and (eb[E.numel():] == -7.0).all()


def test_pool_repr_gives_empty_sequences_the_zero_row():
    """include/rg_hip.h: "an empty sequence gives the zero row" -- ragged with the first, a middle
    and the last sequence empty, padded with rows of zeros, and a call of empty sequences alone."""
    d, N, n, L = 24, 40, 9, 5
    rs = np.random.RandomState(3)
    E, _ = sc.make_tables(N, d, rs)
    seq = sc.make_sequences(n, L, N, rs)
    seq[[0, 4, 8]] = 0
    _, ref = sc.representations(torch.from_numpy(E).double(), torch.from_numpy(seq))
    bound = (L + 1) * EPS32 * np.abs(E).max() + 1e-30
    ptr, ids = _ragged(seq)
    assert ptr[0] == ptr[1] and ptr[4] == ptr[5] and ptr[8] == ptr[9] == len(ids)
    Ed = _dev(E)
    for R in (seq_engine.pool_repr(Ed, _dev(seq)), seq_engine.pool_repr(Ed, _dev(ids), seq_ptr=ptr)):
        R = R.cpu().numpy()
        assert R[[0, 4, 8]].tobytes() == np.zeros((3, d), np.float32).tobytes()
        assert R[[1, 2, 3, 5, 6, 7]].any(axis=1).all() and np.abs(R - ref.numpy()).max() <= bound
    R = seq_engine.pool_repr(Ed, _dev(np.zeros(0, np.int64)), seq_ptr=np.zeros(4, np.int64)).cpu().numpy()
    assert R.tobytes() == np.zeros((3, d), np.float32).tobytes()


@pytest.mark.parametrize("n, L, d", [(1, 1, 8), (3, 33, 64), (300, 33, 12), (300, 1, 256), (3, 1, 4), (1, 33, 128),
                                     (3, 33, 16), (300, 5, 32), (3, 5, 24), (300, 33, 48), (3, 33, 96), (300, 2, 160),
                                     (3, 5, 200)])
def test_pool_repr_and_predict_batch_against_the_oracle(n, L, d):
    rs = np.random.RandomState(n + L + d)
    N = 257
    E, b = sc.make_tables(N, d, rs)
    seq = sc.make_sequences(n, L, N, rs)
    _, ref = sc.representations(torch.from_numpy(E).double(), torch.from_numpy(seq))
    ref = ref.numpy()
    # float32 error of a mean of at most L rows: the sum's L roundings and the division's one
    bound = (L + 1) * EPS32 * np.abs(E).max() + 1e-30
    ptr, ids = _ragged(seq)
    for R in (seq_engine.pool_repr(_dev(E), _dev(seq)), seq_engine.pool_repr(_dev(E), _dev(ids), seq_ptr=ptr)):
        R = R.cpu().numpy()
        assert R.shape == (n, d) and np.abs(R - ref).max() <= bound
    model = ImplicitSequenceModel(embedding_dim=d)
    model.set_tables(E, b, device=DEV)
    blk = model.predict_batch(seq)
    assert blk.is_cuda and blk.dtype == torch.float32 and tuple(blk.shape) == (n, N)
    ref_s = sc.final_scores(torch.from_numpy(E).double(), torch.from_numpy(b).double(), torch.from_numpy(seq)).numpy()
    # a dot of d products on top of the representation's error, and the bias add
    sbound = (d + L + 3) * EPS32 * (np.abs(ref).max() * np.abs(E).max() * d + np.abs(b).max())
    err = np.abs(blk.cpu().numpy() - ref_s).max()
    print(f"\nn {n} L {L} d {d}: scores max err {err:.3e} bound {sbound:.3e}")
    assert err <= sbound
    assert (blk.cpu().numpy()[:, 0] == 0).all()              # the padding item's row and bias are zero


@pytest.mark.parametrize("n, L, d, k", [(1, 1, 8, 5), (300, 33, 64, 10), (3, 33, 4, 32), (300, 1, 16, 1)])
def test_recommend_next_is_the_oracles_ranking(n, L, d, k):
    rs = np.random.RandomState(7 * n + L + d)
    N = 257
    E, b = sc.make_tables(N, d, rs)
    seq = sc.make_sequences(n, L, N, rs)
    model = ImplicitSequenceModel(embedding_dim=d)
    model.set_tables(E, b, device=DEV)
    s32 = sc.final_scores(torch.from_numpy(E), torch.from_numpy(b), torch.from_numpy(seq)).numpy()
    assert s32.dtype == np.float32
    s64 = sc.final_scores(torch.from_numpy(E).double(), torch.from_numpy(b).double(), torch.from_numpy(seq)).numpy()
    _, r64 = sc.representations(torch.from_numpy(E).double(), torch.from_numpy(seq))
    # the float32 error bound of a score (as in the predict test), for the oracle and the kernel alike
    bound = (d + L + 3) * EPS32 * (np.abs(r64.numpy()).max() * np.abs(E).max() * d + np.abs(b).max())
    assert np.abs(s32 - s64).max() <= bound
    for exclude in (True, False):
        ids = model.recommend_next(seq, k, exclude_preceding=exclude)
        assert ids.dtype == np.int64 and ids.shape == (n, k)
        masked = s32.copy()
        masked[:, 0] = -np.inf
        if exclude:
            np.put_along_axis(masked, seq, -np.inf, axis=1)
        want = np.argsort(-masked, axis=1, kind="stable")[:, :k + 1]
        checked = 0
        for r in range(n):
            assert (ids[r] != 0).all() and len(set(ids[r].tolist())) == k
            if exclude:
                assert not np.isin(ids[r], seq[r]).any()
            sv = masked[r, want[r]]
            # position j is pinned when its oracle score is more than twice the bound from both neighbours
            gaps = -np.diff(sv)
            clear = gaps > 2 * bound
            for j in range(k):
                if clear[j] and (j == 0 or clear[j - 1]):
                    assert ids[r, j] == want[r, j], (r, j)
                    checked += 1
        assert checked >= n * k // 2
    with pytest.raises(ValueError):
        model.recommend_next(seq, 0)
    with pytest.raises(ValueError):
        model.recommend_next(seq, N)


def test_sequence_mrr_score_on_the_device_equals_the_host_loop():
    rs = np.random.RandomState(5)
    N, d, L = 120, 16, 7
    E, b = sc.make_tables(N, d, rs)
    seqs = sc.make_sequences(50, L, N, rs)
    test = SequenceInteractions(seqs, num_items=N)
    model = ImplicitSequenceModel(embedding_dim=d)
    model.set_tables(E, b, device=DEV)

    class HostOnly:
        predict = staticmethod(model.predict)

    for exclude in (False, True):
        dev = evaluation.sequence_mrr_score(model, test, exclude_preceding=exclude)
        host = evaluation.sequence_mrr_score(HostOnly(), test, exclude_preceding=exclude)
        assert dev.shape == host.shape == (50,)
        assert np.abs(dev - host).max() <= 1e-12


def test_the_entries_refuse_out_of_range_arguments_without_a_launch():
    lib = _lib.load()
    case = sc.make_case(8, 5, 3, 1, 7)
    E, b, seq, neg = (_dev(case[k]) for k in ("E", "b", "seq", "neg"))
    grad = torch.full((7, 9), -7.0, device=DEV)
    ws = torch.full((int(lib.rg_seq_pool_workspace_len(3, 5, 1)),), -7.0, device=DEV)
    out = torch.full((1,), -7.0, device=DEV)
    p = _lib.ptr
    good = dict(seq=p(seq), neg=p(neg), E=p(E), b=p(b), dim=8, num_items=7, B=3, L=5, K=1, loss=1, inv=0.1,
                grad=p(grad), ws=p(ws), out=p(out))

    def call(**over):
        a = dict(good, **over)
        return lib.rg_seq_pool_grads(_lib.stream_handle(), *[a[k] for k in good])

    for over, word in ((dict(dim=6), "dim"), (dict(dim=0), "dim"), (dict(dim=260), "dim"), (dict(L=0), "L"),
                       (dict(L=1025), "L"), (dict(K=0), "K"), (dict(K=17), "K"), (dict(B=0), "B"),
                       (dict(loss=0), "pointwise"), (dict(loss=4), "loss"), (dict(inv=0.0), "inv_count"),
                       (dict(inv=2.0), "inv_count"), (dict(num_items=1), "num_items"), (dict(seq=None), "null"),
                       (dict(grad=None), "null"), (dict(ws=None), "null")):
        assert call(**over) == -1, over
        assert word in lib.rg_last_error().decode(), (over, lib.rg_last_error())
    assert lib.rg_seq_pool_workspace_len(3, 1025, 1) == -1 and lib.rg_seq_pool_workspace_len(3, 5, 17) == -1
    o = seq_engine.adam_opt(1, 1e-2)
    sgd = _lib.Opt()
    sgd.kind = 1
    z = torch.zeros(7, 8, device=DEV)
    zb = torch.zeros(7, device=DEV)
    for args, word in (((p(E), p(b), p(z), p(z), p(zb), p(zb), p(grad), 0, 7, ctypes.byref(o)), "dim"),
                       ((p(E), p(b), p(z), p(z), p(zb), p(zb), p(grad), 8, 0, ctypes.byref(o)), "num_items"),
                       ((p(E), p(b), p(z), p(z), p(zb), p(zb), p(grad), 8, 7, ctypes.byref(sgd)), "Adam"),
                       ((p(E), p(b), None, p(z), p(zb), p(zb), p(grad), 8, 7, ctypes.byref(o)), "null")):
        assert lib.rg_seq_adam_dense(_lib.stream_handle(), *args) == -1
        assert word in lib.rg_last_error().decode()
    R = torch.full((3, 8), -7.0, device=DEV)
    for args, word in (((p(E), 6, 7, p(seq), None, 5, 3, p(R)), "dim"), ((p(E), 8, 7, p(seq), None, 1025, 3, p(R)), "L"),
                       ((p(E), 8, 7, p(seq), None, 5, -1, p(R)), "n < 0"), ((p(E), 8, 7, None, None, 5, 3, p(R)), "ids"),
                       ((None, 8, 7, p(seq), None, 5, 3, p(R)), "null")):
        assert lib.rg_seq_pool_repr(_lib.stream_handle(), *args) == -1
        assert word in lib.rg_last_error().decode()
    assert lib.rg_seq_pool_repr(_lib.stream_handle(), p(E), 8, 7, p(seq), None, 5, 0, p(R)) == 0
    torch.cuda.synchronize()
    for t in (grad, ws, out, R):
        assert (t.cpu().numpy() == -7.0).all()
    assert E.cpu().numpy().tobytes() == case["E"].tobytes()


def test_an_end_to_end_fit_raises_the_sequence_mrr():
    inter = generate_sequential(500, 100, 10000, 0.01, 1, np.random.RandomState(0))
    seqs = inter.to_sequence(max_sequence_length=6, step_size=3)
    rs = np.random.RandomState(1)
    held = rs.rand(len(seqs)) < 0.2
    held &= (seqs.sequences[:, -2] != 0)
    train = SequenceInteractions(seqs.sequences[~held], num_items=100)
    test = SequenceInteractions(seqs.sequences[held], num_items=100)
    torch.manual_seed(0)
    model = ImplicitSequenceModel(loss="bpr", embedding_dim=32, n_iter=5, batch_size=256, learning_rate=5e-2,
                                  random_state=np.random.RandomState(2))
    model._n_iter = 0
    model.fit(train)                                            # tables initialised, no step taken
    before = evaluation.sequence_mrr_score(model, test).mean()
    model._n_iter = 5
    model.fit(train)
    after = evaluation.sequence_mrr_score(model, test).mean()
    print(f"\nsequence MRR on {len(test)} held-out sequences: {before:.4f} before fitting, {after:.4f} after 5 epochs")
    assert after > before
