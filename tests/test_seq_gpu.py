"""The pooling sequence model on the GPU: rg_seq_pool_grads against the float64 oracle under
fold_in_common's rule (tests/seq_common.py), rg_seq_adam_dense against torch's op sequence, five
free-running steps beside the float64 oracle, rg_seq_pool_repr / predict / recommend_next against
the fixture and the oracle, sequence_mrr_score's device path against its host loop, the entries'
refusals, and an end-to-end fit.  Every case in a few seconds.
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


@pytest.mark.parametrize("l2", [0.0, 1e-3])
@pytest.mark.parametrize("step", [1, 7])
def test_adam_dense_is_torchs_op_sequence(step, l2):
    rs = np.random.RandomState(10 * step + int(l2 > 0))
    N, d, lr = 301, 20, 1e-2
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
        print(f"\nadam step {step} l2 {l2} {name}: max ulp p {up.max()} m {um.max()} v {uv.max()}")
        assert up.max() <= 1 and um.max() <= 1 and uv.max() <= 1
        # row 0 is untouched, parameters and moments
        for k, start in zip(keys, (p0, m0, v0)):
            assert got[k][0].tobytes() == np.ascontiguousarray(start[0]).tobytes()
        assert (got[keys[0]][1:] != p0[1:]).any()


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


@pytest.mark.parametrize("n, L, d", [(1, 1, 8), (3, 33, 64), (300, 33, 12), (300, 1, 256), (3, 1, 4), (1, 33, 128)])
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
