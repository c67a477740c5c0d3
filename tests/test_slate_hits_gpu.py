"""Slate hits on the GPU (rg_slate_hits through the C-ABI) against the set arithmetic the
reference's precision_recall_score_slates does per user (spotlight/evaluation.py:355-382):
bit j of a row's word = slate position j is one of the row's targets and the item's first
occurrence in the slate, so popcount == len(set(pred[:k]) & set(targets)).  Masks are integers
and are compared for equality: every lane-stride boundary of the target lists, repeated slate
items, padding and negative ids, padded row strides, the widest k, bad arguments; then
precision_recall_score_slates on a device tensor, CGAN.test against the per-batch host
evaluation it replaces (the same floats, not close ones), and GANEngine.slate_hits under
torch's synchronisation check."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from recommendation_gans_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 3            # pad columns hold an item id that is in most target lists: reading one sets a bit


def csr_of(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    idx = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return ptr, idx.astype(np.int32)


def dev_i(a):
    """Device copy of an index array; an empty one still gets a non-null pointer."""
    t = torch.zeros(max(len(a), 1), dtype=torch.from_numpy(a).dtype, device=DEV)
    t[:len(a)] = torch.from_numpy(a).to(DEV)
    return t


def device_masks(slates, tgt, k, ld=None):
    """slates (rows, S) int numpy, tgt: one list of ids per row.  Returns the uint32 masks;
    checks that the slates were only read."""
    lib = _lib.load()
    rows, S = slates.shape
    ld = S if ld is None else ld
    buf = torch.full((rows, ld), JUNK, dtype=torch.int32, device=DEV)
    buf[:, :S] = torch.from_numpy(slates.astype(np.int32)).to(DEV)
    before = buf.clone()
    tp, ti = csr_of(tgt)
    tpd, tid = dev_i(tp), dev_i(ti)
    out = torch.full((rows,), -9, dtype=torch.int32, device=DEV)
    _lib.check(lib.rg_slate_hits(_lib.stream_handle(), _lib.ptr(buf), rows, S, ld, k, _lib.ptr(tpd), _lib.ptr(tid),
                                 _lib.ptr(out)), "rg_slate_hits")
    torch.cuda.synchronize()
    assert torch.equal(buf, before), "the slates were written"
    return out.cpu().numpy().view(np.uint32)


def host_masks(slates, tgt, k):
    """The issue's two conditions per bit, and the reference's set count as the popcount."""
    out = np.zeros(len(slates), dtype=np.uint32)
    for r, (pred, t) in enumerate(zip(slates, tgt)):
        m = 0
        for j in range(k):
            if pred[j] in set(t) and pred[j] not in list(pred[:j]):
                m |= 1 << j
        assert bin(m).count("1") == len(set(pred[:k].tolist()) & set(np.asarray(t).tolist()))
        out[r] = m
    return out


def draw_case(rows, S, N, seed):
    """Slates over [0, N) with repeats, ids 0 and N - 1, and the ids N (padding) and -1, which no
    target list holds; target lists cycling through the lane-stride boundaries, drawn with
    repeats from [0, N), unsorted."""
    rs = np.random.RandomState(seed)
    slates = rs.randint(0, N, (rows, S)).astype(np.int64)
    lens = [0, 1, 63, 64, 65, 130]
    tgt = [rs.randint(0, N, lens[r % len(lens)]).tolist() for r in range(rows)]
    for r in range(rows):
        if r % 4 == 1 and S >= 3:            # a repeated item (hit or miss as the targets fall)
            slates[r, S - 1] = slates[r, 0]
        if r % 7 == 2:
            slates[r, rs.randint(S)] = N
        if r % 7 == 3:
            slates[r, rs.randint(S)] = -1
        if r % 5 == 4:
            slates[r, 0], slates[r, S - 1] = 0, N - 1
    return slates, tgt


@pytest.mark.parametrize("k", [1, 3, 7])
def test_masks_match_set_arithmetic(k):
    N, rows, S, ld = 12, 257, 7, 9
    slates, tgt = draw_case(rows, S, N, seed=1)
    if S >= 3:
        # a repeated hit and a repeated miss, by construction (rows with 130 and 1 targets)
        slates[5, :3] = [tgt[5][0], 4, tgt[5][0]]
        miss = next(i for i in range(N) if i not in tgt[7])
        slates[7, :3] = [miss, miss, miss]
    got = device_masks(slates, tgt, k, ld)
    want = host_masks(slates, tgt, k)
    assert (got == want).all(), (np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    assert (got[[len(t) == 0 for t in tgt]] == 0).all()
    assert want.any() and (want >> k == 0).all()
    # the padding id and -1 never hit
    odd = (slates[:, :k] == N) | (slates[:, :k] == -1)
    assert odd.any()
    for j in range(k):
        assert ((got[odd[:, j]] >> j) & 1 == 0).all()
    if k >= 3:
        assert got[5] & 5 == 1 and got[7] & 7 == 0
    # a single row: fewer rows than one workgroup takes
    one = device_masks(slates[5:6], tgt[5:6], k, ld)
    assert one.shape == (1,) and one[0] == want[5]


def test_widest_k():
    """slate_size = k = 32: every bit of the word, hits at the first and the last position."""
    N, rows, S = 4000, 5, 32
    rs = np.random.RandomState(2)
    slates = np.stack([rs.permutation(N)[:S] for _ in range(rows)]).astype(np.int64)
    tgt = [rs.randint(0, N, 70).tolist() for _ in range(rows)]
    tgt[1] = [int(slates[1, 31]), int(slates[1, 0])] + [N + 5] * 64          # hits at positions 0 and 31 only
    tgt[2] = slates[2].tolist()                                               # every position hits
    tgt[3] = []
    slates[4, 31] = slates[4, 0]
    tgt[4] = [int(slates[4, 0])] * 3
    got = device_masks(slates, tgt, 32)
    assert (got == host_masks(slates, tgt, 32)).all()
    assert got[1] == 0x80000001 and got[2] == 0xffffffff and got[3] == 0 and got[4] == 1
    assert (device_masks(slates, tgt, 17) == host_masks(slates, tgt, 17)).all()      # the 32-wide kernel, k < 32


def test_bad_arguments_fail_loudly():
    lib = _lib.load()
    sl = torch.zeros(4, 9, dtype=torch.int32, device=DEV)
    tp, ti = dev_i(np.arange(5, dtype=np.int64)), dev_i(np.zeros(4, np.int32))
    out = torch.full((4,), -9, dtype=torch.int32, device=DEV)
    sh = _lib.stream_handle()

    def call(rows=4, S=7, ld=9, k=3, s=sl, tptr=tp, tidx=ti, o=out):
        return lib.rg_slate_hits(sh, _lib.ptr(s), rows, S, ld, k, _lib.ptr(tptr), _lib.ptr(tidx), _lib.ptr(o))

    def refused(**kw):
        rc = call(**kw)
        return rc != 0 and len(lib.rg_last_error()) > 0

    assert refused(s=None) and refused(tptr=None) and refused(tidx=None) and refused(o=None)
    assert refused(rows=-1)
    assert refused(S=0, ld=9, k=1)
    assert refused(ld=6)
    assert refused(k=0) and refused(k=8) and refused(S=40, ld=40, k=33)
    assert refused(rows=(2 ** 31 - 1) * _lib.RG_SLATE_HITS_ROWS_PER_BLOCK + 1)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -9).all()
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -9).all()                # rows = 0 launches nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 1).all()                 # item 0 at position 0 is each row's target


# ---------------------------------------------------------------- through the evaluation module
def ragged_csr(rs, rows, cols, empty_every=4, mean=6):
    """A CSR of held-out items; every ``empty_every``-th row has none."""
    lists = [[] if r % empty_every == 2 else rs.choice(cols, rs.randint(1, 2 * mean), replace=False).tolist()
             for r in range(rows)]
    ptr, idx = csr_of(lists)
    return sp.csr_matrix((np.ones(len(idx), np.float32), idx, ptr), shape=(rows, cols))


def test_precision_recall_score_slates_on_device():
    from recommendation_gans_amd.spotlight.evaluation import precision_recall_score_slates
    rs = np.random.RandomState(3)
    rows, S, N = 203, 5, 40
    test = ragged_csr(rs, rows, N)
    slates = torch.from_numpy(rs.randint(0, N, (rows, S)).astype(np.int64))
    slates[::9, 3] = slates[::9, 1]                       # repeated items
    for k in (5, 3):
        hp, hr = precision_recall_score_slates(slates, test, k=k)
        dp, dr = precision_recall_score_slates(slates.to(DEV), test, k=k)
        assert len(dp) == int((np.diff(test.indptr) > 0).sum()) and sum(dp) > 0
        assert dp == hp and dr == hr
        assert all(type(x) is float for x in dp + dr)


# ---------------------------------------------------------------- CGAN.test
def make_cgan(N, tmp_path, monkeypatch, S=5):
    from recommendation_gans_amd.CGANs import CGAN
    from recommendation_gans_amd.spotlight.dnn_models.cGAN_models import discriminator, generator
    monkeypatch.chdir(tmp_path)
    H, E, Z, B = 32, 5, 100, 64
    torch.manual_seed(5)
    G = generator(num_items=N, noise_dim=Z, embedding_dim=E, hidden_layer=[H // 2, H], output_dim=S)
    D = discriminator(num_items=N, embedding_dim=E, hidden_layers=[2 * H, H, H // 2], input_dim=S)
    model = CGAN(G=G, D=D, z_dim=Z, n_iter=1, batch_size=B, slate_size=S, embedding_dim=E, hidden_layer=H,
                 experiment_name=f"gan{N}_{S}", use_cuda=True, random_state=np.random.RandomState(0))
    model.num_users, model.num_items = 150, N
    model._initialize()                                   # what fit() does before its first epoch
    return model


@pytest.mark.parametrize("N", [300, 100])
def test_cgan_test_equals_the_per_batch_host_evaluation(N, tmp_path, monkeypatch):
    """N = 300: the generator GEMM's fused argmax epilogue; N = 100: heads narrower than a column
    tile.  Batches of 64, 64, 22 users and 64, 6 cold-start users; some users without targets."""
    from recommendation_gans_amd.gan_engine import GANBatch
    from recommendation_gans_amd.spotlight.evaluation import precision_recall_score_slates
    model = make_cgan(N, tmp_path, monkeypatch)
    S, B, Z, E = model.slate_size, 64, 100, 5
    rs = np.random.RandomState(N)
    U, C, L = 150, 70, 23
    hist = np.full((U, L), N, dtype=np.int64)
    for u in range(U):
        n = rs.randint(1, L + 1)
        hist[u, :n] = rs.randint(0, N, n)
    train_vec = torch.Tensor(hist.astype(np.float32))     # the data provider's float matrix
    test, cold = ragged_csr(rs, U, N, mean=12), ragged_csr(rs, C, N, empty_every=5, mean=12)

    # the evaluation as it was: one GANBatch + generate + download + host loop per batch
    seed = 11
    torch.manual_seed(seed)
    p, r = [], []
    cold_vec = np.full((C, E), N, dtype=np.int64)
    for vec, csr in ((hist, test), (cold_vec, cold)):
        for r0 in range(0, len(vec), B):
            rows = vec[r0:r0 + B]
            z = torch.rand(len(rows), Z, device=DEV)
            sl = model.engine.generate(GANBatch(rows, None, N, S, DEV), z=z).cpu().type(torch.int64)
            pb, rb = precision_recall_score_slates(sl, csr[r0:r0 + len(rows), :], k=S)
            p += pb
            r += rb
    want = {"precision": float(np.mean(p)), "recall": float(np.mean(r)), "at": S}
    assert 0.0 < want["precision"] < 1.0                  # some hits: the equality below says something

    torch.manual_seed(seed)
    got = model.test(train_vec, test, cold)
    assert got == want, (got, want)
    assert json.load(open(os.path.join(model.experiment_logs, "test_results.json"))) == want
    # without cold-start users, and with the history matrix going up in several chunks
    torch.manual_seed(seed)
    p0, r0_ = p[:int((np.diff(test.indptr) > 0).sum())], r[:int((np.diff(test.indptr) > 0).sum())]
    from recommendation_gans_amd import CGANs
    monkeypatch.setattr(CGANs, "HIST_UPLOAD_BYTES", 4 * L * B)        # one batch per chunk
    got = model.test(train_vec, test)
    assert got == {"precision": float(np.mean(p0)), "recall": float(np.mean(r0_)), "at": S}
    with pytest.raises(ValueError):
        bad = train_vec.clone()
        bad[140, 2] = N + 1
        model.test(bad, test)


def test_engine_slate_hits_does_not_synchronise(tmp_path, monkeypatch):
    from recommendation_gans_amd.gan_engine import csr_to_device
    model = make_cgan(300, tmp_path, monkeypatch)
    rs = np.random.RandomState(7)
    U, L, N = 150, 9, 300
    hist = torch.from_numpy(rs.randint(0, N + 1, (U, L)).astype(np.int32)).to(DEV)
    tp, ti = csr_to_device(ragged_csr(rs, U, N), U, DEV)
    out = torch.empty(U, dtype=torch.int32, device=DEV)
    model.engine.slate_hits(hist, tp, ti, 5)              # first call outside the check (lazy initialisation)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                # noqa: BLE001
        pytest.skip(f"torch.cuda.set_sync_debug_mode is not supported by this build: {e}")
    try:
        masks = model.engine.slate_hits(hist, tp, ti, 5, out=out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert masks is out and masks.dtype == torch.int32 and masks.shape == (U,)
    m = masks.cpu().numpy()
    assert (m >= 0).all() and (m < 32).all()


def test_cgan_test_with_a_slate_wider_than_a_mask_word(tmp_path, monkeypatch):
    """slate_size 33 > 32 bits: the slates are still generated from the device history matrix, the
    hits are counted by the host loop; the figures are the per-batch evaluation's."""
    from recommendation_gans_amd.gan_engine import GANBatch
    from recommendation_gans_amd.spotlight.evaluation import precision_recall_score_slates
    N, S, B, U, L = 100, 33, 64, 70, 6
    model = make_cgan(N, tmp_path, monkeypatch, S=S)
    rs = np.random.RandomState(1)
    hist = rs.randint(0, N + 1, (U, L)).astype(np.int64)
    test = ragged_csr(rs, U, N, mean=12)
    torch.manual_seed(2)
    p, r = [], []
    for r0 in range(0, U, B):
        rows = hist[r0:r0 + B]
        sl = model.engine.generate(GANBatch(rows, None, N, S, DEV), z=torch.rand(len(rows), 100, device=DEV))
        pb, rb = precision_recall_score_slates(sl.cpu().type(torch.int64), test[r0:r0 + len(rows), :], k=S)
        p += pb
        r += rb
    torch.manual_seed(2)
    assert model.test(hist, test) == {"precision": float(np.mean(p)), "recall": float(np.mean(r)), "at": S}
    assert np.mean(p) > 0
