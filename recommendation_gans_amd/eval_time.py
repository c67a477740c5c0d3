"""Stand-alone timing of the all-item NCF / NeuMF score block (outside tests and bench.py).

    python -m recommendation_gans_amd.eval_time [--users 256] [--items 26744] [--reps 20] [--big 4096]

Times, for the E = 64 NCF MLP and NeuMF (E = 16, M = 50) at the ML-20M item count, one block of
``--users`` users scored against every item by

  * ``NCFEngine.score_users``  -- rg_ncf_score_users (the split first layer's halves + the fused
    pair kernel), and
  * ``NCFEngine.scores_torch`` -- the pairwise torch path the evaluation used before (gather, cat,
    one GEMM per layer, where, sigmoid through global memory),

with device events around each call after a warm-up, the two paths alternating, and reports
min / median per path, their ratio, the largest difference between the two blocks, and the
kernel path's algorithmic flops and bytes against the fp32 MFMA and HBM peaks.  ``--big N``
also times the kernel path alone on a block of N users: the pairwise path is not run there, its
concatenated input alone is N x items x 2E floats (56 GB at 4096 x 26,744 x 128).  One JSON line
per model on stdout.

    python -m recommendation_gans_amd.eval_time --metric mrr [--test-users 4096] [--reps 20]

times ``evaluation.mrr_score`` instead, for an MF (d = 64) and an NCF (E = 64) model at 138,493
users x ``--items`` items: ``--test-users`` test users of about 20 test items each, 100 train
items each excluded.  The device path (``rank_users`` -> rg_rank_rows) and the host path (the
score block copied to the host, scipy rankdata per user; one repetition) run on the same model
object, wall time around calls that end on the host; the two results are compared.

    python -m recommendation_gans_amd.eval_time --metric slates [--users 136677] [--reps 5]

times one whole ``CGAN.test`` of ``--users`` users for the generator ``bench.py --model gan`` builds
(S = 5, H = 256, E = 5, Z = 100, the ML-20M item count, reference initialisation, batch 256):
synthetic padded histories of ``--hist-len`` columns and about 20 held-out items per user.  The
device path (``CGAN.test``: rg_gan_generate per batch, one rg_slate_hits launch, one download) and
the host path it replaced (per batch a GANBatch, ``generate``, ``.cpu()`` and the per-user set
loop, restated here) run in the same process on the same engine under the same torch seed, wall
time around calls that end on the host; the two results must be equal.

    python -m recommendation_gans_amd.eval_time --metric pairs [--users 256] [--batch 8192] [--reps 5]

times the scores of arbitrary (user, item) pairs, ``NCFEngine.scores`` (rg_ncf_score_pairs, one
fused launch) against ``NCFEngine.scores_torch`` (the chain of torch ops it replaced) on the same
engine and ids, for the same two models at two sizes: the ``--users`` x ``--items`` block as a flat
list of pairs, and one training batch of ``--batch`` random pairs.  Device events, the two paths
alternating; min / median, the largest relative difference of the two results, and the kernel's
time against max(flops at the fp32 MFMA peak, gathered bytes at the HBM peak).  One JSON line per
model and size.

    python -m recommendation_gans_amd.eval_time --metric mf_scores [--items 26744] [--reps 20]

times the MF score block, ``mf_engine.score_users_block`` (rg_mf_score_users, one fused launch)
against ``mf_engine.score_users_torch`` (the chain of torch ops it replaced: gather, library GEMM,
two broadcast adds, sigmoid) on the same tables and ids: 256 and 4096 users x ``--items`` items at
d in {32, 64, 128}.  Device events, the two paths alternating; min / median per path, their ratio,
the largest relative difference of the two blocks, and the kernel's time against max(flops at the
fp32 MFMA peak, output bytes at the HBM peak).  One JSON line per shape.

    python -m recommendation_gans_amd.eval_time --metric mf_topk [--items 26744] [--reps 20]

times one block of MF ``recommend``: ``mf_engine.topk_users_fused`` (rg_mf_topk_users: score,
exclude and rank in LDS) against the path it replaced, written out as one function -- the score
block, -inf scattered from host-built indices, rg_topk_rows, the scores gathered at the ids.  Both
start from host ids and a scipy CSR and end with ids and scores on the host, and must agree bit for
bit.  256 and 4096 users x ``--items`` items at d in {32, 64, 128}, k = 10, with 100 excluded items
per user and with none; the two paths alternating, device events and the host clock around the
whole call, min / median per path, and the peak device memory of one call of each.  One JSON line
per shape.

    python -m recommendation_gans_amd.eval_time --metric item_sim [--items 26744] [--reps 20]

times one block of ``similar_items``: ``mf_engine.row_rnorms`` + ``mf_engine.similar_rows``
(rg_row_rnorms, then rg_item_sim_topk: product, cosine and ranking in LDS) against the chain of
torch ops a user would write for it on the same device and table -- ``F.normalize``, ``mm``, -inf at
each query's own column, ``torch.topk``.  256 and 4096 query ids on an ``--items`` x d table at d in
{32, 64, 128}, k = 10, the query's own row excluded; ids on the device before and results on the
device after on both sides.  Device events, the two paths alternating; min / median per path, the
peak device memory of one call of each, the share of rows whose id sets agree (the chain's order of
tied items is torch.topk's) and the largest difference of the similarities.  One JSON line per shape.

    python -m recommendation_gans_amd.eval_time --metric gan_recommend [--users 256] [--reps 20]

times one batch of cGAN inference at the ``slates`` metric's shape (the ML-20M item count, S = 5,
H = 256, E = 5, Z = 100, ``--users`` = batch_max rows, histories ``--hist-len`` wide) three ways on
one engine and one z: rg_gan_generate (the per-head argmax, the baseline: not the code under
measurement), and rg_gan_recommend with both flags on its stored path (tanh block written to the
workspace, then one workgroup per row) and on its fused path (top-T candidates from the GEMM
epilogue, no block).  Device events, the three alternating; min / median per path, the peak device
memory torch saw during one call of each (the workspace and the scratch are allocated before), the
sizes of the tanh block and of the scratch, and whether the two paths agree.  One JSON line.

    python -m recommendation_gans_amd.eval_time --metric topk_wide [--items 26744] [--reps 20]

times rg_topk_rows_wide (radix select, k up to 1024) on one score block of 256 and of 4096 users x
``--items`` items that is already on the device, at k = 50, 100 and 1024: device events, the ids
left on the device.  Beside it, alternating on the same block: (a) the host path it replaces in
the @k metrics above k = 32 -- the block copied to the host, negated, one ``argsort`` per row in a
Python loop, the first k -- on the host clock, 2 repetitions at 256 users and 1 at 4096 (the line
says how many); (b) ``torch.topk(blk, k)``, for information only: its order of tied scores is
unspecified, so it is no replacement, and the line gives the share of rows whose id sets agree.
Each block size also gets a k = 32 line, the new entry against rg_topk_rows (reported only: the old
kernel keeps k <= 32).  One JSON line per block size and k.

    python -m recommendation_gans_amd.eval_time --metric gan_score [--reps 20]

times the cGAN critic at inference on 256 and on 4096 rows at the ``gan_recommend`` metric's shape
(histories ``--hist-len`` wide, ids already on the device, scores left there): GANEngine.score_slates
(rg_gan_score_slates) against the torch path it replaces -- ``d_state_dict()`` loaded into the
``discriminator`` module on the same GPU in eval mode, fed ``one_hot_encoding`` of the slates --
alternating in one process.  Device events, min / median per path, the peak device memory torch
saw during one call of each, the largest difference of the two results and, at 256 rows for
information, one batch of ``CGAN.recommend`` with ``samples=8`` (eight draws, one scoring call, the
selection) against ``samples=1``.  One JSON line per row count.

    python -m recommendation_gans_amd.eval_time --metric fold_in [--items 26744] [--reps 20]

times MF fold-in: ``mf_engine.fold_in_users`` (rg_mf_fold_in_users, one launch) against
``mf_engine.fold_in_users_torch`` (a padded gather, autograd and ``torch.optim.Adam`` per step) on the
same inputs, alternating in one process: 256 and 4096 new users against an ``--items`` x d item
table at d in {32, 64, 128}, 100 history items each, 3 negatives per positive, 20 steps, pointwise
loss; ids on the device going in, rows on the device coming out.  Device events, min / median per
path, the peak device memory of one call of each, the largest difference of the two results, and
the kernel's time against max(gathered bytes at 8 TB/s, flops at the fp32 vector peak).  One JSON
line per shape.

    python -m recommendation_gans_amd.eval_time --metric candidates [--items 26744] [--reps 20]

times candidate-list scoring and ranking, 100 candidates per user and k = 10 at 256 and 4096 users:
MF (d in {32, 64, 128}) through ``candidates.score_lists`` + ``seg_topk`` against the torch chain and
against the full score block + gather + rg_topk_rows, NCF (E = 64) through ``NCFEngine.scores`` +
``seg_topk`` against ``NCFEngine.scores_torch`` + ``torch.topk``; the paths alternate in one process,
device events, min / median and the peak device memory of one call of each.  One JSON line per model
and shape.

    python -m recommendation_gans_amd.eval_time --metric mmr [--items 26744] [--reps 20]

times diversified re-ranking (maximal marginal relevance) of 100 candidates per user, k = 10, lam = 0.7,
cosine, at 256 and 4096 users and d in {32, 64, 128}: ``candidates.seg_mmr`` (rg_seg_mmr) against
``candidates.seg_mmr_torch`` and beside ``seg_topk`` on the same lists; the paths alternate in one
process, device events, min / median, the peak device memory of one call of each, and the intra-list
similarity of the picks at lam = 1.0 and 0.7.  One JSON line per shape.

    python -m recommendation_gans_amd.eval_time --metric als [--users 138493] [--items 26744] [--reps 20]

times implicit ALS (``als.py``: rg_als_gram, rg_als_solve_rows) on a synthetic ML-20M-shaped matrix,
``--users`` x ``--items`` with 20 M interactions and Zipf-skewed item popularity (exponent 0.5: the
most popular item has ~60 k users, so the item half-step has workgroup-per-row lists beside a median
of a few hundred), at d in {32, 64, 128} and cg_steps = 3: one full sweep, and separately ``gram``,
the user half-step, the item half-step, and the item half-step's rows at or above
``rg_als_long_row_len()`` alone (the long path's share).  The half-steps alternate with
``als.solve_rows_torch`` on the same inputs in the same process (rows sorted by length, blocks of at
most ``block_elems`` padded elements; ``torch_reps`` repetitions).  Device events, min / median, the
largest difference of the two results, and the kernel's distance from its two bounds:
(cg_steps + 1) nnz d 4 gathered bytes at 8 TB/s, and its flops at the fp32 vector peak.  One JSON
line per d.

    python -m recommendation_gans_amd.eval_time --metric seq_pool [--items 26744] [--reps 20]

times the pooling sequence model (``seq_engine.py``: rg_seq_pool_grads + rg_seq_adam_dense, and one
``recommend_next`` block of 4096 sequences) against the chain of torch ops each replaces -- the
float32 formulas of ``seq_engine.pool_loss_torch`` with autograd and a hand-written dense Adam, and
gather / cumsum / GEMM / topk -- on the same GPU in the same process, the two alternating: training
steps at B in {256, 4096}, L in {10, 50}, d in {32, 64, 128}, bpr.  Device events, min / median, the
largest difference of the two results, and the step's distance from max(gathered bytes at 8 TB/s,
flops at the fp32 vector peak).  One JSON line per shape.

    python -m recommendation_gans_amd.eval_time --metric seq_cnn [--items 26744] [--reps 20]

times the causal-convolution sequence model the same way (rg_seq_cnn_grads + rg_seq_adam_dense +
rg_seq_adam_flat, and one ``recommend_next`` block, against ``seq_engine.cnn_loss_torch`` with
autograd and ``torch.optim.Adam``, and ``cnn_repr_torch`` / GEMM / topk), for the default net and a
3-layer net of dilations 1 / 2 / 4, with the GEMM stages' bound (``main_seq_cnn``).
"""
import argparse
import contextlib
import json
import os
import tempfile

import numpy as np
import torch

from .ncf_engine import NCFEngine
from .ncf_spotlight import mlp_layers

PEAK_FP32_MFMA = 157.3e12      # flop/s (spec)
PEAK_HBM = 8.0e12              # B/s (spec)
ML20M_USERS = 136677           # synthetic.ML20M["num_users"]


def stats(ts):
    return {"min": min(ts), "median": float(np.median(ts))}


@contextlib.contextmanager
def temp_cwd():
    """A temporary working directory: the models write their experiment folder under the cwd."""
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            yield
        finally:
            os.chdir(cwd)


def make_engine(E, M, U, I, dev):
    """Reference-style init: N(0, 1) embeddings, Xavier-uniform weights, bias 0.01."""
    g = torch.Generator().manual_seed(0)
    sizes = mlp_layers(E)
    mlp = []
    for i, o in list(zip(sizes[:-1], sizes[1:])) + [(8 + M, 1)]:
        lim = (6.0 / (i + o)) ** 0.5
        mlp += [(torch.rand(o, i, generator=g) * 2 - 1) * lim, torch.full((o,), 0.01)]
    tabs = dict(mf_user_w=torch.randn(U, M, generator=g), mf_item_w=torch.randn(I, M, generator=g)) if M else {}
    return NCFEngine(torch.randn(U, E, generator=g), torch.randn(I, E, generator=g), mlp, np.zeros(4, np.int64),
                     np.zeros(4, np.int64), np.zeros(625, np.uint32), device=dev, **tabs)


def algorithmic(E, M, n, I):
    """Flops and compulsory bytes of one block on the kernel path (2 flops per MAC)."""
    sizes = mlp_layers(E)
    narrow = sum(i * o for i, o in zip(sizes[1:-1], sizes[2:])) + 8      # per pair, after the split layer
    pair = narrow + M + E                                                 # + GMF dot + the halves' add
    halves = (I + n) * E * E + n * M
    flops = 2.0 * (n * I * pair + halves)
    bytes_ = 4.0 * (n * I + I * (E + M) + n * (E + M))                    # block written, tables read once
    return flops, bytes_


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


class _HostOnly:
    """The model's score block without its device ranking: mrr_score then takes the host path."""

    def __init__(self, m):
        self.score_users = m.score_users


def mrr_data(U, I, n_test, seed=3, test_mean=20, train_per_user=100):
    """``n_test`` random test users with about ``test_mean`` test items each (at least one) and
    ``train_per_user`` train interactions each (the exclusions)."""
    from .spotlight.interactions import Interactions
    rs = np.random.RandomState(seed)
    users = rs.choice(U, n_test, replace=False)
    n_t = np.maximum(rs.poisson(test_mean, n_test), 1)
    tu = np.repeat(users, n_t)
    test = Interactions(tu.astype(np.int32), rs.randint(0, I, len(tu)).astype(np.int32), num_users=U, num_items=I)
    ru = np.repeat(users, train_per_user)
    train = Interactions(ru.astype(np.int32), rs.randint(0, I, len(ru)).astype(np.int32), num_users=U, num_items=I)
    return test, train


def mrr_model(kind, U, I, train):
    """An initialised (untrained) ImplicitFactorizationModel: MF d = 64 or the NCF MLP E = 64."""
    from .implicit import ImplicitFactorizationModel
    from .spotlight.dnn_models.mlp import MLP
    from .spotlight.factorization.representations import BilinearNet
    torch.manual_seed(0)
    if kind == "mf_d64":
        net = BilinearNet(U, I, 64)
        with torch.no_grad():                  # spread the scores (the default init leaves them all near 0.5)
            net.user_embeddings.weight.normal_(0, 0.3)
            net.item_embeddings.weight.normal_(0, 0.3)
            net.item_biases.weight.normal_()
    else:
        net = MLP(layers=mlp_layers(64), num_users=U, num_items=I, embedding_dim=64)
    model = ImplicitFactorizationModel(loss="pointwise", embedding_dim=64, n_iter=1, batch_size=256,
                                       representation=net, random_state=np.random.RandomState(0),
                                       neg_examples=[(0, 0), (1, 1)], num_negative_samples=3, use_cuda=True)
    model._initialize(train)
    return model


def host_timed(fn, reps):
    """Wall time (ms) of calls that end on the host, the device drained before and after."""
    import time
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, out


def main_mrr(args):
    """``--metric mrr``: evaluation.mrr_score of the same model object on the device path
    (rank_users -> rg_rank_rows) and on the host path (score block to the host, scipy rankdata
    per user; one repetition), 4,096 test users with train exclusions."""
    from .spotlight import evaluation
    U, I = 138493, args.items
    test, train = mrr_data(U, I, args.test_users)
    out = []
    with temp_cwd():
        for kind in ("mf_d64", "ncf_e64"):
            model = mrr_model(kind, U, I, train)
            evaluation.mrr_score(model, test, train)                         # warm-up
            t_dev, got = host_timed(lambda: evaluation.mrr_score(model, test, train), args.reps)
            t_host, ref = host_timed(lambda: evaluation.mrr_score(_HostOnly(model), test, train), 1)
            # where the device path's time goes: the score block alone (device events), and
            # rank_users as a whole (score block + CSR upload + rg_rank_rows + counts download)
            tcsr, xcsr = test.tocsr(), train.tocsr()
            ub = np.flatnonzero(np.diff(tcsr.indptr) > 0)
            ud = torch.as_tensor(ub, device=model._engine.device)
            t_block = [timed(lambda: model._device_scores(ud), 1)[0] for _ in range(args.reps)]
            t_rank, _ = host_timed(lambda: model.rank_users(ub, tcsr, xcsr), args.reps)
            r = {"metric": "mrr", "model": kind, "users": U, "items": I, "test_users": int(len(got)),
                 "test_items": int(len(test)), "train_items": int(len(train)), "reps": args.reps,
                 "device_ms": stats(t_dev), "score_block_ms": stats(t_block), "rank_users_ms": stats(t_rank),
                 "host_ms": t_host[0], "speedup_min": t_host[0] / min(t_dev),
                 "speedup_median": float(t_host[0] / np.median(t_dev)),
                 "max_rel_diff": float((np.abs(got - ref) / ref).max()), "mean_mrr": float(got.mean())}
            print(json.dumps(r), flush=True)
            out.append(r)
            del model
            torch.cuda.empty_cache()
    return out


def slates_data(U, N, L, seed=4, test_mean=20):
    """Padded histories (U, L) as the data provider's float matrix (each user 1 .. L items, padding
    N) and a CSR of about ``test_mean`` held-out items per user (one user in 16 has none)."""
    import scipy.sparse as sp
    rs = np.random.RandomState(seed)
    hist = rs.randint(0, N, (U, L)).astype(np.float32)
    hist[np.arange(L)[None, :] >= rs.randint(1, L + 1, U)[:, None]] = N
    n_t = np.maximum(rs.poisson(test_mean, U), 1)
    n_t[::16] = 0
    ptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(n_t, out=ptr[1:])
    idx = rs.randint(0, N, ptr[-1]).astype(np.int32)
    return torch.from_numpy(hist), sp.csr_matrix((np.ones(len(idx), np.float32), idx, ptr), shape=(U, N))


def host_cgan_test(model, train_vec, test):
    """CGAN.test's regular-user loop as it stood before the device path: per batch a GANBatch
    (with the grouping only training needs), generate, a download, and the per-user set loop."""
    from .gan_engine import GANBatch
    from .spotlight.evaluation import precision_recall_score_slates
    from .spotlight.torch_utils import minibatch
    B, S = model._batch_size, model.slate_size
    total = {"precision": [], "recall": []}
    for n, user_batch in enumerate(minibatch(train_vec, batch_size=B)):
        z = torch.rand(user_batch.shape[0], model.z_dim, device=model.device)
        batch = GANBatch(user_batch.numpy().astype(np.int64), None, model.num_items, S, model.device)
        slates = model.engine.generate(batch, z=z).cpu().type(torch.int64)
        p, r = precision_recall_score_slates(slates, test[n * B:n * B + user_batch.shape[0], :], k=S)
        total["precision"] += p
        total["recall"] += r
    return {"precision": float(np.mean(total["precision"])), "recall": float(np.mean(total["recall"])), "at": S}


def main_slates(args):
    """``--metric slates``: one CGAN.test of ``--users`` users on the device path and on the host
    path it replaced, same engine, same seed."""
    from .CGANs import CGAN
    from .spotlight.dnn_models.cGAN_models import discriminator, generator
    from .synthetic import ML20M
    U, N, S, H, E, Z, B, L = args.users, ML20M["num_items"], 5, 256, 5, 100, 256, args.hist_len
    train_vec, test = slates_data(U, N, L)
    with temp_cwd():
        torch.manual_seed(0)
        G = generator(num_items=N, noise_dim=Z, embedding_dim=E, hidden_layer=[H // 2, H], output_dim=S)
        D = discriminator(num_items=N, embedding_dim=E, hidden_layers=[2 * H, H, H // 2], input_dim=S)
        model = CGAN(G=G, D=D, z_dim=Z, n_iter=1, batch_size=B, slate_size=S, embedding_dim=E, hidden_layer=H,
                     experiment_name="eval_time", use_cuda=True, random_state=np.random.RandomState(0))
        model.num_users, model.num_items = U, N
        model._initialize()

        def seeded(fn):
            def run():
                torch.manual_seed(1)
                return fn()
            return run

        dev = seeded(lambda: model.test(train_vec, test))
        host = seeded(lambda: host_cgan_test(model, train_vec, test))
        dev(), host()                                                        # warm-up
        host_reps = max(1, min(args.reps, 3))
        t_dev, got = host_timed(dev, args.reps)
        t_host, ref = host_timed(host, host_reps)
    if got != ref:
        raise SystemExit(f"the two paths disagree: device {got}, host {ref}")
    r = {"metric": "slates", "users": U, "items": N, "hist_len": L, "slate_size": S, "hidden": H, "emb": E, "z": Z,
         "batch": B, "test_items": int(test.nnz), "reps": args.reps, "host_reps": host_reps,
         "device_ms": stats(t_dev), "host_ms": stats(t_host),
         "speedup_min": min(t_host) / min(t_dev), "speedup_median": float(np.median(t_host) / np.median(t_dev)),
         "results_equal": True, "precision": got["precision"], "recall": got["recall"]}
    print(json.dumps(r), flush=True)
    return [r]


def pairs_algorithmic(E, M, n):
    """Flops (2 per MAC; the GMF term 3 per column) and compulsory bytes (ids in, gathered rows, one
    score out) of n pairs on rg_ncf_score_pairs."""
    sizes = mlp_layers(E)
    macs = sum(i * o for i, o in zip(sizes[:-1], sizes[1:])) + 8
    return n * (2.0 * macs + 3.0 * M), n * (4.0 * (2 * E + 2 * M) + 16 + 4)


def main_pairs(args):
    """``--metric pairs``: NCFEngine.scores (rg_ncf_score_pairs) against NCFEngine.scores_torch on the
    same engine and ids, at the users x items block and at one training batch of random pairs."""
    dev = torch.device("cuda:0")
    U, I = 138493, args.items
    out = []
    for name, E, M in (("ncf_e64", 64, 0), ("neumf_e16_m50", 16, 50)):
        e = make_engine(E, M, U, I, dev)
        rs = np.random.RandomState(1)
        users = torch.from_numpy(rs.randint(0, U, args.users)).to(dev)
        sizes = [("block", users.repeat_interleave(I), torch.arange(I, device=dev).repeat(args.users)),
                 ("batch", torch.from_numpy(rs.randint(0, U, args.batch)).to(dev),
                  torch.from_numpy(rs.randint(0, I, args.batch)).to(dev))]
        for kind, pu, pi in sizes:
            n = int(pu.numel())
            new = lambda: e.scores(pu, pi)
            old = lambda: e.scores_torch(pu, pi)
            for _ in range(3):                               # warm-up: code objects, GEMM algorithms, allocator
                a, b = new(), old()
            torch.cuda.synchronize()
            rel = float(((a - b).abs() / b.abs()).max())
            t_new, t_old = [], []
            for _ in range(args.reps):                       # alternate the two paths
                t_new += timed(new, 1)
                t_old += timed(old, 1)
            flops, bytes_ = pairs_algorithmic(E, M, n)
            bound = max(flops / PEAK_FP32_MFMA, bytes_ / PEAK_HBM)
            r = {"metric": "pairs", "model": name, "size": kind, "pairs": n, "reps": args.reps,
                 "kernel_ms": stats(t_new), "torch_ms": stats(t_old),
                 "speedup_min": min(t_old) / min(t_new), "speedup_median": float(np.median(t_old) / np.median(t_new)),
                 "max_rel_diff": rel, "gflop": flops / 1e9, "mbytes": bytes_ / 1e6,
                 "bound_ms": bound * 1e3,
                 "bound_by": "flops" if flops / PEAK_FP32_MFMA >= bytes_ / PEAK_HBM else "bytes",
                 "frac_of_bound": bound / (min(t_new) * 1e-3)}
            print(json.dumps(r), flush=True)
            out.append(r)
            del a, b
        del e, sizes, pu, pi
        torch.cuda.empty_cache()
    return out


def main_mf_scores(args):
    """``--metric mf_scores``: the MF score block, mf_engine.score_users_block (rg_mf_score_users)
    against mf_engine.score_users_torch (gather, library GEMM, two adds, sigmoid) on the same tables
    and ids: 256 and 4096 users x ``--items`` items at d in {32, 64, 128}."""
    from . import mf_engine
    dev = torch.device("cuda:0")
    U, I = 138493, args.items
    out = []
    for d in (32, 64, 128):
        g = torch.Generator().manual_seed(d)
        tabs = [(torch.randn(U, d, generator=g) / d ** 0.5).to(dev), (torch.randn(I, d, generator=g) / d ** 0.5).to(dev),
                (0.1 * torch.randn(U, generator=g)).to(dev), (0.1 * torch.randn(I, generator=g)).to(dev)]
        for n in (256, 4096):
            users = torch.from_numpy(np.random.RandomState(n).randint(0, U, n)).to(dev)
            # the launch alone (ids checked once, here), and the call as _device_scores makes it: the
            # ids' bounds come down to the host first, which the device waits for
            new = lambda: mf_engine.score_users_block(*tabs, users, checked=True)
            full = lambda: mf_engine.score_users_block(*tabs, users)
            old = lambda: mf_engine.score_users_torch(*tabs, users)
            for _ in range(3):                               # warm-up: code objects, GEMM algorithms, allocator
                a, b = full(), old()
                new()
            torch.cuda.synchronize()
            rel = float(((a - b).abs() / b.abs()).max())
            del a, b
            t_new, t_full, t_old = [], [], []
            for _ in range(args.reps):                       # alternate the paths
                t_new += timed(new, 1)
                t_full += timed(full, 1)
                t_old += timed(old, 1)
            flops, bytes_ = 2.0 * n * I * d, 4.0 * n * I     # the product; the block written once
            bound = max(flops / PEAK_FP32_MFMA, bytes_ / PEAK_HBM)
            r = {"metric": "mf_scores", "dim": d, "users": n, "items": I, "reps": args.reps,
                 "kernel_ms": stats(t_new), "with_id_check_ms": stats(t_full), "torch_ms": stats(t_old),
                 "speedup_min": min(t_old) / min(t_new), "speedup_median": float(np.median(t_old) / np.median(t_new)),
                 "speedup_with_id_check_median": float(np.median(t_old) / np.median(t_full)),
                 "max_rel_diff": rel, "gflop": flops / 1e9, "mbytes": bytes_ / 1e6, "bound_ms": bound * 1e3,
                 "bound_by": "flops" if flops / PEAK_FP32_MFMA >= bytes_ / PEAK_HBM else "bytes",
                 "frac_of_bound": bound / (min(t_new) * 1e-3)}
            print(json.dumps(r), flush=True)
            out.append(r)
        del tabs
        torch.cuda.empty_cache()
    return out


def main_mf_topk(args):
    """``--metric mf_topk``: one block of MF recommend, mf_engine.topk_users_fused against the path it
    replaced (score block, -inf scatter from host-built indices, rg_topk_rows, gather)."""
    import time

    import scipy.sparse as sp

    from . import mf_engine
    from .implicit import _csr_rows_sorted, _exclude_csr_rows, _topk_block
    dev = torch.device("cuda:0")
    U, I, k = 138493, args.items, 10
    out = []

    def replaced(tabs, ub, csr):
        u = torch.as_tensor(ub, device=dev)
        blk = mf_engine.score_users_block(*tabs, u)
        _exclude_csr_rows(blk, csr, ub)
        ids, got = _topk_block(blk, k)
        return got, torch.gather(blk, 1, ids.to(torch.int64)).cpu().numpy()

    def fused(tabs, ub, csr):
        e_ptr, e_idx = _csr_rows_sorted(csr, ub) if csr is not None else (None, None)
        ids, sc = mf_engine.topk_users_fused(*tabs, ub, k, e_ptr, e_idx, checked=True)
        got = ids.cpu().numpy()
        if got.min() < 0 or got.max() >= I:
            raise RuntimeError("rg_mf_topk_users returned an item id outside the table")
        return got, sc.cpu().numpy()

    def clocked(fn):
        """(device ms, host ms) of one call; the call ends with its results on the host."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    for d in (32, 64, 128):
        g = torch.Generator().manual_seed(d)
        tabs = [(torch.randn(U, d, generator=g) / d ** 0.5).to(dev), (torch.randn(I, d, generator=g) / d ** 0.5).to(dev),
                (0.1 * torch.randn(U, generator=g)).to(dev), (0.1 * torch.randn(I, generator=g)).to(dev)]
        for n in (256, 4096):
            rs = np.random.RandomState(n)
            ub = rs.choice(U, n, replace=False).astype(np.int64)
            cols = np.concatenate([rs.choice(I, 100, replace=False) for _ in range(n)])
            exc = sp.csr_matrix((np.ones(100 * n, np.float32), (np.repeat(ub, 100), cols)), shape=(U, I))
            exc.sort_indices()
            for csr, excluded in ((exc, 100), (None, 0)):
                new = lambda: fused(tabs, ub, csr)
                old = lambda: replaced(tabs, ub, csr)
                for _ in range(3):                           # warm-up: code objects, allocator
                    a, b = new(), old()
                equal = bool((a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes())
                del a, b
                t_new, t_old = [], []
                for _ in range(args.reps):                   # alternate the two paths
                    t_new.append(clocked(new))
                    t_old.append(clocked(old))
                dn, hn = zip(*t_new)
                do, ho = zip(*t_old)
                r = {"metric": "mf_topk", "dim": d, "users": n, "items": I, "k": k, "excluded_per_user": excluded,
                     "reps": args.reps, "equal": equal,
                     "fused_device_ms": stats(dn), "fused_host_ms": stats(hn),
                     "replaced_device_ms": stats(do), "replaced_host_ms": stats(ho),
                     "host_median_ratio_replaced_over_fused": float(np.median(ho) / np.median(hn)),
                     "device_median_ratio_replaced_over_fused": float(np.median(do) / np.median(dn)),
                     "fused_peak_bytes": peak(new), "replaced_peak_bytes": peak(old), "block_bytes": 4 * n * I}
                print(json.dumps(r), flush=True)
                out.append(r)
        del tabs
        torch.cuda.empty_cache()
    return out


def main_item_sim(args):
    """``--metric item_sim``: one block of similar_items, mf_engine.row_rnorms + similar_rows against
    the torch chain F.normalize, mm, -inf at the own column, torch.topk."""
    import torch.nn.functional as F

    from . import mf_engine
    dev = torch.device("cuda:0")
    I, k = args.items, 10
    out = []

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    for d in (32, 64, 128):
        g = torch.Generator().manual_seed(d)
        table = (torch.randn(I, d, generator=g) / d ** 0.5).to(dev)
        for n in (256, 4096):
            q = torch.from_numpy(np.random.RandomState(n).randint(0, I, n)).to(dev)
            rows = torch.arange(n, device=dev)

            def new():
                return mf_engine.similar_rows(table, q, k, rnorm=mf_engine.row_rnorms(table), checked=True)

            def old():
                unit = F.normalize(table, dim=1)
                sims = unit[q] @ unit.T
                sims[rows, q] = float("-inf")
                top = torch.topk(sims, k, dim=1)
                return top.indices, top.values

            for _ in range(3):                               # warm-up: code objects, GEMM algorithms, allocator
                a, b = new(), old()
            torch.cuda.synchronize()
            ia, ib = a[0].cpu().numpy().astype(np.int64), b[0].cpu().numpy()
            same = float(np.mean([set(x) == set(y) for x, y in zip(ia.tolist(), ib.tolist())]))
            diff = float((a[1] - b[1]).abs().max())
            del a, b
            t_new, t_old = [], []
            for _ in range(args.reps):                       # alternate the two paths
                t_new += timed(new, 1)
                t_old += timed(old, 1)
            r = {"metric": "item_sim", "dim": d, "queries": n, "items": I, "k": k, "reps": args.reps,
                 "kernel_ms": stats(t_new), "torch_ms": stats(t_old),
                 "median_ratio_torch_over_kernel": float(np.median(t_old) / np.median(t_new)),
                 "kernel_peak_bytes": peak(new), "torch_peak_bytes": peak(old), "block_bytes": 4 * n * I,
                 "rows_with_equal_id_sets": same, "max_abs_sim_diff": diff}
            print(json.dumps(r), flush=True)
            out.append(r)
        del table
        torch.cuda.empty_cache()
    return out


def main_fold_in(args):
    """``--metric fold_in``: mf_engine.fold_in_users (rg_mf_fold_in_users, one launch) against
    fold_in_users_torch (padded gather, autograd, torch.optim.Adam per step) on the same inputs: new
    users with 100 history items each, 3 negatives per positive, 20 steps, pointwise loss; ids on the
    device going in, rows on the device coming out.  ``bound_ms``: max(gathered bytes at 8 TB/s,
    flops at the 157.3 TFLOP/s fp32 vector peak) -- every step gathers users * 100 * 4 rows of
    (dim + 1) floats and spends 4 * dim flops on each (the dot and the gradient accumulation)."""
    from . import mf_engine
    dev = torch.device("cuda:0")
    I, hist, n_neg, steps = args.items, 100, 3, 20
    out = []

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    for d in (32, 64, 128):
        g = torch.Generator().manual_seed(d)
        Q = (torch.randn(I, d, generator=g) / d ** 0.5).to(dev)
        c = (torch.randn(I, generator=g) * 0.1).to(dev)
        for n in (256, 4096):
            rs = np.random.RandomState(n + d)
            ptr = torch.arange(0, (n + 1) * hist, hist, dtype=torch.int64, device=dev)
            idx = torch.from_numpy(rs.randint(0, I, n * hist).astype(np.int32)).to(dev)
            neg = torch.from_numpy(rs.randint(0, I, n * hist * n_neg).astype(np.int32)).to(dev)
            kw = dict(loss="pointwise", steps=steps, lr=0.05, weight_decay=1e-6, checked=True)

            def new():
                return mf_engine.fold_in_users(Q, c, ptr, idx, neg, n_neg, **kw)

            def old():
                return mf_engine.fold_in_users_torch(Q, c, ptr, idx, neg, n_neg, **kw)

            for _ in range(3):                               # warm-up: code objects, allocator
                a, b = new(), old()
            torch.cuda.synchronize()
            diff = float(max((a[0] - b[0]).abs().max(), (a[1] - b[1]).abs().max()))
            del a, b
            t_new, t_old = [], []
            for _ in range(args.reps):                       # alternate the two paths
                t_new += timed(new, 1)
                t_old += timed(old, 1)
            rows = n * hist * (1 + n_neg) * steps
            bound = max(rows * (d + 1) * 4 / 8e12, rows * 4 * d / 157.3e12) * 1e3
            r = {"metric": "fold_in", "dim": d, "users": n, "items": I, "history": hist, "n_neg": n_neg,
                 "steps": steps, "loss": "pointwise", "reps": args.reps, "kernel_ms": stats(t_new),
                 "torch_ms": stats(t_old), "median_ratio_torch_over_kernel": float(np.median(t_old) / np.median(t_new)),
                 "kernel_peak_bytes": peak(new), "torch_peak_bytes": peak(old), "max_abs_diff": diff,
                 "bound_ms": bound, "kernel_over_bound": float(np.median(t_new) / bound)}
            print(json.dumps(r), flush=True)
            out.append(r)
        del Q, c
        torch.cuda.empty_cache()
    return out


def main_als(args):
    """``--metric als``: one ALS sweep and its parts (gram, the two half-steps, the long rows of the
    item half-step alone) on a synthetic ML-20M-shaped matrix, the half-steps against
    als.solve_rows_torch on the same inputs; see the module docstring.  ``bytes_bound_ms``: (cg_steps
    + 1) nnz d 4 gathered bytes at 8 TB/s; ``flops_bound_ms``: per pass 4 d flops per entry (the dot
    and the accumulation) and 2 d^2 per row (G p), at 157.3 TFLOP/s."""
    from . import als
    dev = torch.device("cuda:0")
    U, I, nnz, cg, lam, alpha = args.users, args.items, args.nnz, 3, 0.01, 40.0
    rs = np.random.RandomState(0)
    pop = 1.0 / np.sqrt(np.arange(1, I + 1))
    items = rs.choice(I, size=nnz, p=pop / pop.sum()).astype(np.int32)
    users = rs.randint(0, U, nnz).astype(np.int32)
    csr_u = als.interactions_csr(users, items, None, U)
    csr_i = als.interactions_csr(items, users, None, I)
    T = als.long_row_len()
    block_elems, torch_reps = 1 << 26, min(args.reps, 3)
    out = []
    for d in (32, 64, 128):
        g = torch.Generator().manual_seed(d)
        X0 = (torch.randn(U, d, generator=g) / d).to(dev)
        Y0 = (torch.randn(I, d, generator=g) / d).to(dev)
        sides = {}
        for name, (p_, i_, _), own, other in (("user", csr_u, X0, Y0), ("item", csr_i, Y0, X0)):
            pd, idd = torch.from_numpy(p_).to(dev), torch.from_numpy(i_).to(dev)
            order = als.rows_by_length(p_).to(dev)
            lens = np.diff(p_)
            long_rows = torch.from_numpy(np.flatnonzero(lens >= T).astype(np.int64)).to(dev)
            sides[name] = dict(ptr=pd, idx=idd, order=order, own=own, other=other, lens=lens, long_rows=long_rows)

        def half(name, x, torch_path=False, rows=None):
            s_ = sides[name]
            G = als.gram(s_["other"], lam)
            fn = als.solve_rows_torch if torch_path else als.solve_rows
            kw = dict(block_elems=block_elems) if torch_path else {}
            return fn(s_["other"], G, s_["ptr"], s_["idx"], None, alpha, cg, x, rows=s_["order"] if rows is None else rows,
                      **kw)

        def sweep():
            X, Y = X0.clone(), Y0.clone()
            als.solve_rows(Y, als.gram(Y, lam), sides["user"]["ptr"], sides["user"]["idx"], None, alpha, cg, X,
                           rows=sides["user"]["order"])
            als.solve_rows(X, als.gram(X, lam), sides["item"]["ptr"], sides["item"]["idx"], None, alpha, cg, Y,
                           rows=sides["item"]["order"])

        r = {"metric": "als", "dim": d, "users": U, "items": I, "nnz": nnz, "cg_steps": cg, "lam": lam, "alpha": alpha,
             "reps": args.reps, "torch_reps": torch_reps, "torch_block_elems": block_elems, "long_row_len": T}
        for _ in range(2):
            sweep()
        r["sweep_ms"] = stats(timed(sweep, args.reps))
        r["gram_users_ms"] = stats(timed(lambda: als.gram(X0, lam), args.reps))
        r["gram_items_ms"] = stats(timed(lambda: als.gram(Y0, lam), args.reps))
        for name in ("user", "item"):
            s_ = sides[name]
            xk, xt = s_["own"].clone(), s_["own"].clone()
            half(name, xk)
            half(name, xt, torch_path=True)
            torch.cuda.synchronize()
            r[f"{name}_max_abs_diff"] = float((xk - xt).abs().max())
            r[f"{name}_max_abs"] = float(xt.abs().max())
            t_new, t_old = [], []
            for k in range(args.reps):                        # alternate the two paths
                xk.copy_(s_["own"])
                t_new += timed(lambda: half(name, xk), 1)
                if k < torch_reps:
                    xt.copy_(s_["own"])
                    t_old += timed(lambda: half(name, xt, torch_path=True), 1)
            n_rows, n_e = len(s_["lens"]), int(s_["lens"].sum())
            bytes_b = (cg + 1) * n_e * d * 4 / 8e12 * 1e3
            flops_b = (cg + 1) * (4.0 * d * n_e + 2.0 * d * d * n_rows) / 157.3e12 * 1e3
            med = float(np.median(t_new))
            r[f"{name}_half_ms"] = stats(t_new)
            r[f"{name}_half_torch_ms"] = stats(t_old)
            r[f"{name}_torch_over_kernel"] = float(np.median(t_old) / med)
            r[f"{name}_bytes_bound_ms"], r[f"{name}_flops_bound_ms"] = bytes_b, flops_b
            r[f"{name}_kernel_over_bound"] = med / max(bytes_b, flops_b)
            r[f"{name}_longest_row"] = int(s_["lens"].max())
            r[f"{name}_long_rows"] = int(s_["long_rows"].numel())
            r[f"{name}_long_entries_share"] = float(s_["lens"][s_["lens"] >= T].sum() / max(n_e, 1))
            if s_["long_rows"].numel():
                t_long = []
                for _ in range(args.reps):
                    xk.copy_(s_["own"])
                    t_long += timed(lambda: half(name, xk, rows=s_["long_rows"]), 1)
                r[f"{name}_long_rows_alone_ms"] = stats(t_long)
                r[f"{name}_long_share_of_half"] = float(np.median(t_long) / med)
            del xk, xt
        print(json.dumps(r), flush=True)
        out.append(r)
        del X0, Y0, sides
        torch.cuda.empty_cache()
    return out


def _peak_mb(fn, dev):
    """Peak device memory of one call of fn above what was allocated before it, in MB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak / 1e6


def main_candidates(args):
    """``--metric candidates``: score and rank 100 candidates per user out of ``--items`` items, k = 10,
    for 256 and 4096 users: MF at d in {32, 64, 128} -- ``candidates.score_lists`` + ``seg_topk``
    (rg_mf_score_lists, rg_seg_topk) against (a) the torch chain (``score_lists_torch``, ``torch.topk``
    on the (users, 100) view) and (b) what existed before: the full score block
    (``mf_engine.score_users_block``), ``gather`` of the candidates' columns, rg_topk_rows on the
    gathered block -- and NCF at E = 64: ``NCFEngine.scores`` (users repeated per entry) + ``seg_topk``
    against ``NCFEngine.scores_torch`` + ``torch.topk``.  Ids and lists are on the device going in
    (checked once, here), positions on the device coming out; the paths alternate in one process,
    median of ``--reps`` device-event measurements, and the peak device memory of one call of each.
    One JSON line per model and shape (profiles/candidates/eval_time_candidates.jsonl holds a run)."""
    from . import _lib, candidates as cand, mf_engine
    dev = torch.device("cuda:0")
    U, I, C, k = 138493, args.items, 100, 10
    lib = _lib.load()
    out = []

    def lists(n):
        rs = np.random.RandomState(n)
        users = torch.from_numpy(rs.randint(0, U, n)).to(dev)
        idx = torch.from_numpy(rs.randint(0, I, (n, C)).astype(np.int32)).to(dev)
        ptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * C
        return users, ptr, idx

    def measure(paths):
        for _ in range(3):                                   # warm-up: code objects, allocator
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in paths}
        for _ in range(args.reps):                           # alternate the paths
            for name, fn in paths.items():
                ts[name] += timed(fn, 1)
        return ({name + "_ms": stats(t) for name, t in ts.items()},
                {name + "_peak_mb": _peak_mb(fn, dev) for name, fn in paths.items()})

    def emit(r):
        print(json.dumps(r), flush=True)
        out.append(r)

    for d in (32, 64, 128):
        g = torch.Generator().manual_seed(d)
        tabs = [(torch.randn(U, d, generator=g) / d ** 0.5).to(dev), (torch.randn(I, d, generator=g) / d ** 0.5).to(dev),
                (0.1 * torch.randn(U, generator=g)).to(dev), (0.1 * torch.randn(I, generator=g)).to(dev)]
        for n in (256, 4096):
            users, ptr, idx = lists(n)
            idx64 = idx.to(torch.int64)

            def kernel():
                return cand.seg_topk(cand.score_lists(*tabs, users, ptr, idx.reshape(-1), checked=True), ptr,
                                     idx.reshape(-1), k, checked=True)

            def torch_chain():
                s = cand.score_lists_torch(*tabs, users, ptr, idx.reshape(-1))
                return torch.topk(s.view(n, C), k, dim=1).indices

            def block():
                blk = mf_engine.score_users_block(*tabs, users, checked=True)
                sub = torch.gather(blk, 1, idx64)
                pos = torch.empty(n, k, dtype=torch.int32, device=dev)
                _lib.check(lib.rg_topk_rows(_lib.stream_handle(), _lib.ptr(sub), n, C, C, k, _lib.ptr(pos)),
                           "rg_topk_rows")
                return pos
            ms, mb = measure({"kernel": kernel, "torch": torch_chain, "block": block})
            a = cand.score_lists(*tabs, users, ptr, idx.reshape(-1))
            b = cand.score_lists_torch(*tabs, users, ptr, idx.reshape(-1))
            r = {"metric": "candidates", "model": "mf", "dim": d, "users": n, "items": I, "candidates": C, "k": k,
                 "reps": args.reps, **ms, **mb, "max_abs_diff": float((a - b).abs().max()),
                 "speedup_vs_torch_median": ms["torch_ms"]["median"] / ms["kernel_ms"]["median"],
                 "speedup_vs_block_median": ms["block_ms"]["median"] / ms["kernel_ms"]["median"]}
            emit(r)
        del tabs
        torch.cuda.empty_cache()
    E = 64
    eng = make_engine(E, 0, U, I, dev)
    for n in (256, 4096):
        users, ptr, idx = lists(n)
        rep, idx64 = torch.repeat_interleave(users, C), idx.reshape(-1).to(torch.int64)

        def kernel():
            return cand.seg_topk(eng.scores(torch.repeat_interleave(users, ptr[1:] - ptr[:-1]), idx64), ptr,
                                 idx.reshape(-1), k, checked=True)

        def torch_chain():
            return torch.topk(eng.scores_torch(torch.repeat_interleave(users, C), idx64).view(n, C), k, dim=1).indices
        ms, mb = measure({"kernel": kernel, "torch": torch_chain})
        r = {"metric": "candidates", "model": "ncf", "dim": E, "users": n, "items": I, "candidates": C, "k": k,
             "reps": args.reps, **ms, **mb,
             "max_abs_diff": float((eng.scores(rep, idx64) - eng.scores_torch(rep, idx64)).abs().max()),
             "speedup_vs_torch_median": ms["torch_ms"]["median"] / ms["kernel_ms"]["median"]}
        emit(r)
    return out


def main_mmr(args):
    """``--metric mmr``: diversified re-ranking of 100 candidates per user out of ``--items`` items,
    k = 10, lam = 0.7, cosine, for 256 and 4096 users at d in {32, 64, 128}: ``candidates.seg_mmr``
    (rg_seg_mmr, one launch) against ``candidates.seg_mmr_torch`` (the padded gather and k rounds of
    torch ops), and beside them ``seg_topk`` on the same lists (what lam = 1 costs).  Scores, lists,
    table and reciprocal norms are on the device going in, positions on the device coming out; the
    paths alternate in one process, median of ``--reps`` device-event measurements, the peak device
    memory of one call of each, and the intra-list similarity (``seg_mean_sim``) of the picks at
    lam = 1.0 and 0.7.  One JSON line per shape (profiles/mmr/eval_time_mmr.jsonl holds a run)."""
    from . import candidates as cand, mf_engine
    dev = torch.device("cuda:0")
    I, C, k, lam = args.items, 100, 10, 0.7
    out = []
    for d in (32, 64, 128):
        g = torch.Generator().manual_seed(d)
        table = (torch.randn(I, d, generator=g) / d ** 0.5).to(dev)
        rnorm = mf_engine.row_rnorms(table)
        for n in (256, 4096):
            rs = np.random.RandomState(n)
            idx = torch.from_numpy(np.stack([rs.permutation(I)[:C] for _ in range(n)]).astype(np.int32)).to(dev)
            idx = idx.reshape(-1)
            ptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * C
            scores = torch.sigmoid(torch.randn(n * C, generator=g)).to(dev)
            paths = {"kernel": lambda: cand.seg_mmr(scores, ptr, idx, table, k, lam, rnorm=rnorm, checked=True),
                     "torch": lambda: cand.seg_mmr_torch(scores, ptr, idx, table, k, lam, rnorm=rnorm),
                     "seg_topk": lambda: cand.seg_topk(scores, ptr, idx, k, checked=True)}
            for _ in range(3):                                   # warm-up: code objects, allocator
                for fn in paths.values():
                    fn()
            torch.cuda.synchronize()
            ts = {name: [] for name in paths}
            for _ in range(args.reps):                           # alternate the paths
                for name, fn in paths.items():
                    ts[name] += timed(fn, 1)
            a, b = paths["kernel"](), paths["torch"]()

            def ils(pos):
                picks = torch.gather(idx.view(n, C), 1, pos.to(torch.int64)).reshape(-1).contiguous()
                p = torch.arange(n + 1, dtype=torch.int64, device=dev) * k
                return float(cand.seg_mean_sim(p, picks, table, rnorm=rnorm, checked=True).double().mean())
            r = {"metric": "mmr", "dim": d, "users": n, "items": I, "candidates": C, "k": k, "lam": lam,
                 "similarity": "cosine", "reps": args.reps, **{name + "_ms": stats(t) for name, t in ts.items()},
                 **{name + "_peak_mb": _peak_mb(fn, dev) for name, fn in paths.items()},
                 "gathered_block_mb": 4 * n * C * d / 1e6,
                 "rows_equal_torch_fp32": float((a == b).all(dim=1).double().mean()),
                 "intra_list_similarity": {"lam_1.0": ils(cand.seg_mmr(scores, ptr, idx, table, k, 1.0, rnorm=rnorm,
                                                                      checked=True)), "lam_0.7": ils(a)},
                 "speedup_vs_torch_median": float(np.median(ts["torch"]) / np.median(ts["kernel"])),
                 "kernel_over_seg_topk_median": float(np.median(ts["kernel"]) / np.median(ts["seg_topk"]))}
            print(json.dumps(r), flush=True)
            out.append(r)
        del table, rnorm
        torch.cuda.empty_cache()
    return out


def main_topk_wide(args):
    """``--metric topk_wide``: rg_topk_rows_wide on one score block already on the device, against
    the host path it replaces in the @k metrics above k = 32 (the block to the host, argsort per row)
    and, for information, torch.topk; and at k = 32 against rg_topk_rows."""
    import time

    from . import _lib
    dev = torch.device("cuda:0")
    I = args.items
    lib = _lib.load()
    out = []

    def wide(blk, ids, k):
        _lib.check(lib.rg_topk_rows_wide(_lib.stream_handle(), _lib.ptr(blk), blk.shape[0], I, I, k, _lib.ptr(ids),
                                         None), "rg_topk_rows_wide")

    def narrow(blk, ids, k):
        _lib.check(lib.rg_topk_rows(_lib.stream_handle(), _lib.ptr(blk), blk.shape[0], I, I, k, _lib.ptr(ids)),
                   "rg_topk_rows")

    def host(blk, k):
        """What evaluation._scored / _ranked do with a block: download, negate, argsort per row."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = -blk.cpu().numpy()
        top = np.empty((len(scores), k), dtype=np.int64)
        for r in range(len(scores)):
            top[r] = scores[r].argsort(axis=0)[:k]
        return (time.perf_counter() - t0) * 1e3, top

    for n in (256, 4096):
        # sigmoid of a normal logit, as a trained model's block: one magnitude, many shared leading bits
        blk = torch.sigmoid(torch.randn(n, I, generator=torch.Generator().manual_seed(n))).to(dev).contiguous()
        head = blk[:64].cpu().numpy()
        host_reps = 2 if n <= 256 else 1
        for k in (50, 100, 1024):
            ids = torch.empty(n, k, dtype=torch.int32, device=dev)
            new = lambda: wide(blk, ids, k)
            tk = lambda: torch.topk(blk, k, dim=1)
            for _ in range(3):                               # warm-up: code objects, allocator
                new()
                t = tk()
            torch.cuda.synchronize()
            got = ids.cpu().numpy().astype(np.int64)
            stable = bool((got[:64] == np.argsort(-head, axis=1, kind="stable")[:, :k]).all())
            ti = t.indices.cpu().numpy()
            same = float(np.mean([set(x) == set(y) for x, y in zip(got.tolist(), ti.tolist())]))
            del t
            t_new, t_tk, t_host, host_equal = [], [], [], True
            for rep in range(args.reps):                     # alternate the paths on the same block
                t_new += timed(new, 1)
                t_tk += timed(tk, 1)
                if rep < host_reps:
                    ms, top = host(blk, k)
                    t_host.append(ms)
                    host_equal = host_equal and bool((top == got).all())
            r = {"metric": "topk_wide", "users": n, "items": I, "k": k, "reps": args.reps,
                 "wide_ms": stats(t_new), "torch_topk_ms": stats(t_tk),
                 "host_ms": {"reps": host_reps, "times": t_host, "median": float(np.median(t_host))},
                 "median_ratio_host_over_wide": float(np.median(t_host) / np.median(t_new)),
                 "median_ratio_torch_over_wide": float(np.median(t_tk) / np.median(t_new)),
                 "ids_equal_stable_argsort_first_64_rows": stable, "ids_equal_host_argsort": host_equal,
                 "rows_with_torch_topk_id_sets_equal": same, "block_bytes": 4 * n * I}
            print(json.dumps(r), flush=True)
            out.append(r)
        # reported only: rg_topk_rows keeps k <= 32 whatever this says
        ids, ids_n = (torch.empty(n, 32, dtype=torch.int32, device=dev) for _ in range(2))
        new, old = (lambda: wide(blk, ids, 32)), (lambda: narrow(blk, ids_n, 32))
        for _ in range(3):
            new()
            old()
        t_new, t_old = [], []
        for _ in range(args.reps):
            t_new += timed(new, 1)
            t_old += timed(old, 1)
        r = {"metric": "topk_wide", "users": n, "items": I, "k": 32, "reps": args.reps, "wide_ms": stats(t_new),
             "topk_rows_ms": stats(t_old),
             "median_ratio_wide_over_topk_rows": float(np.median(t_new) / np.median(t_old)),
             "ids_equal": bool(torch.equal(ids, ids_n))}
        print(json.dumps(r), flush=True)
        out.append(r)
        del blk, ids, ids_n
        torch.cuda.empty_cache()
    return out


def main_gan_recommend(args):
    """``--metric gan_recommend``: rg_gan_generate, and rg_gan_recommend's stored and fused paths, on
    one batch at the slate evaluation's shape."""
    import ctypes

    from .gan_engine import GANBatch, GANEngine
    from .spotlight.dnn_models.cGAN_models import discriminator, generator
    from .synthetic import ML20M
    dev = torch.device("cuda:0")
    B, N, S, H, E, Z, L = args.users, ML20M["num_items"], 5, 256, 5, 100, args.hist_len
    torch.manual_seed(0)
    G = generator(num_items=N, noise_dim=Z, embedding_dim=E, hidden_layer=[H // 2, H], output_dim=S)
    D = discriminator(num_items=N, embedding_dim=E, hidden_layers=[2 * H, H, H // 2], input_dim=S)
    eng = GANEngine(G.state_dict(), D.state_dict(), N, S, H, E, Z, batch_max=B, device=dev)
    del G, D
    hist = slates_data(B, N, L)[0].numpy().astype(np.int64)
    batch = GANBatch(hist, None, N, S, dev)
    z = torch.rand(B, Z, device=dev)
    paths = {"generate": lambda: eng.generate(batch, z=z),
             "stored": lambda: eng.recommend_slates(batch.hist, z=z, path=1),
             "fused": lambda: eng.recommend_slates(batch.hist, z=z, path=2)}
    for _ in range(3):                                           # warm-up: code objects, the scratch, allocator
        got = {k: fn() for k, fn in paths.items()}
    torch.cuda.synchronize()
    equal = bool(torch.equal(got["stored"], got["fused"]))
    sl = got["fused"].cpu().numpy()
    argmax = got["generate"].cpu().numpy().astype(np.int64)
    ts = {k: [] for k in paths}
    for _ in range(args.reps):                                   # alternate the three
        for k, fn in paths.items():
            ts[k] += timed(fn, 1)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    r = {"metric": "gan_recommend", "rows": B, "items": N, "slate_size": S, "hidden": H, "emb": E, "z": Z,
         "hist_len": L, "reps": args.reps,
         "generate_ms": stats(ts["generate"]), "stored_ms": stats(ts["stored"]), "fused_ms": stats(ts["fused"]),
         "fused_over_stored_median": float(np.median(ts["fused"]) / np.median(ts["stored"])),
         "fused_over_generate_median": float(np.median(ts["fused"]) / np.median(ts["generate"])),
         "peak_bytes": {k: peak(fn) for k, fn in paths.items()},
         "tanh_block_bytes": 4 * B * S * N, "scratch_bytes": int(eng._rec_scratch.numel()),
         "stored_scratch_bytes": int(eng.lib.rg_gan_recommend_scratch_bytes(ctypes.byref(eng.dims), 1)),
         "workspace_bytes": int(eng.ws.numel()), "fused_equals_stored": equal,
         "argmax_rows_with_a_repeat": int(sum(len(set(row)) < S for row in argmax.tolist())),
         "argmax_rows_with_a_seen_item": int(sum(bool(set(a) & set(h)) for a, h in zip(argmax.tolist(), hist.tolist()))),
         "recommend_rows_with_a_repeat_or_seen_item": int(sum(len(set(row)) < S or bool(set(row) & set(h))
                                                              for row, h in zip(sl.tolist(), hist.tolist())))}
    print(json.dumps(r), flush=True)
    return [r]


def main_gan_score(args):
    """``--metric gan_score``: GANEngine.score_slates (rg_gan_score_slates) against the torch path it
    replaces, at 256 and 4096 rows of the slate evaluation's shape."""
    from .CGANs import CGAN
    from .gan_engine import GANEngine
    from .spotlight.dnn_models.cGAN_models import discriminator, generator
    from .synthetic import ML20M
    dev = torch.device("cuda:0")
    N, S, H, E, Z, L, B = ML20M["num_items"], 5, 256, 5, 100, args.hist_len, 256
    torch.manual_seed(0)
    G = generator(num_items=N, noise_dim=Z, embedding_dim=E, hidden_layer=[H // 2, H], output_dim=S)
    D = discriminator(num_items=N, embedding_dim=E, hidden_layers=[2 * H, H, H // 2], input_dim=S)
    eng = GANEngine(G.state_dict(), D.state_dict(), N, S, H, E, Z, batch_max=B, device=dev)
    del G
    D.load_state_dict(eng.d_state_dict())
    D = D.to(dev).eval()
    with temp_cwd():
        model = CGAN(z_dim=Z, batch_size=B, slate_size=S, embedding_dim=E, hidden_layer=H, experiment_name="gan_score")
    model.engine, model.num_items = eng, N

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    out = []
    for rows in (256, 4096):
        hist = slates_data(rows, N, L)[0].to(torch.int32).to(dev).contiguous()
        sl = torch.from_numpy(np.random.RandomState(5).randint(0, N, (rows, S)).astype(np.int32)).to(dev)

        def torch_path():
            with torch.no_grad():
                return D(model.one_hot_encoding(sl, N), hist)[:, 0]

        paths = {"kernel": lambda: eng.score_slates(hist, sl), "torch": torch_path}
        for _ in range(3):                                       # warm-up: code objects, GEMM algorithms, allocator
            got = {k: fn() for k, fn in paths.items()}
        torch.cuda.synchronize()
        diff = float((got["kernel"] - got["torch"]).abs().max())
        ts = {k: [] for k in paths}
        for _ in range(args.reps):                               # alternate the two
            for k, fn in paths.items():
                ts[k] += timed(fn, 1)
        r = {"metric": "gan_score", "rows": rows, "items": N, "slate_size": S, "hidden": H, "emb": E,
             "hist_len": L, "reps": args.reps, "kernel_ms": stats(ts["kernel"]), "torch_ms": stats(ts["torch"]),
             "torch_over_kernel_median": float(np.median(ts["torch"]) / np.median(ts["kernel"])),
             "peak_bytes": {k: peak(fn) for k, fn in paths.items()}, "one_hot_bytes": 4 * rows * S * N,
             "max_abs_diff": diff, "max_abs_score": float(got["torch"].abs().max())}
        if rows == B:                                            # for information: best of 8 per batch
            rec = {"samples_1": lambda: eng.recommend_slates(hist),
                   "samples_8": lambda: model._best_of(hist, 8, True, True)}
            for _ in range(2):
                for fn in rec.values():
                    fn()
            tr = {k: [] for k in rec}
            for _ in range(args.reps):
                for k, fn in rec.items():
                    tr[k] += timed(fn, 1)
            r["recommend_ms"] = {k: stats(v) for k, v in tr.items()}
        print(json.dumps(r), flush=True)
        out.append(r)
        del got
        torch.cuda.empty_cache()
    return out


def main_seq_pool(args):
    """``--metric seq_pool``: one training step (rg_seq_pool_grads + rg_seq_adam_dense) and one
    recommend_next block against the torch ops they replace.  ``bound_ms`` of a step: the forward
    walk gathers 2 rows per position, the reverse walk 2 more, 4 B L (d + 1) floats; the dense Adam
    pass streams 7 floats per parameter (gradient read and zeroed, p, m, v read and written); flops:
    about 8 d per position."""
    from . import seq_engine
    from .spotlight.sequence import ImplicitSequenceModel
    dev = torch.device("cuda:0")
    I, lr = args.items, 1e-2
    out = []
    for d in (32, 64, 128):
        g = torch.Generator().manual_seed(d)
        E0 = torch.randn(I, d, generator=g) / d
        E0[0] = 0
        for B in (256, 4096):
            for L in (10, 50):
                rs = np.random.RandomState(B + L + d)
                seq = torch.from_numpy(rs.randint(1, I, (B, L))).to(dev)
                seq[: B // 4, : L // 2] = 0
                neg = torch.from_numpy(rs.randint(0, I, (1, B, L))).to(dev)
                count = int((seq != 0).sum())
                E, b = E0.to(dev).clone(), torch.zeros(I, device=dev)
                mom = [torch.zeros_like(E), torch.zeros_like(E), torch.zeros_like(b), torch.zeros_like(b)]
                grad = torch.zeros(I, d + 1, device=dev)
                Et, bt = E.clone().requires_grad_(True), b.clone().requires_grad_(True)
                opt = torch.optim.Adam([Et, bt], lr=lr)

                def new():
                    lv, _ = seq_engine.pool_grads(E, b, seq, neg, "bpr", grad=grad, mask_count=count, checked=True)
                    seq_engine.adam_dense(E, b, *mom, grad, 1, lr)
                    return lv

                def old():
                    opt.zero_grad(set_to_none=True)
                    lv = seq_engine.pool_loss_torch(Et, bt, seq, neg, "bpr")
                    lv.backward()
                    with torch.no_grad():
                        Et.grad[0] = 0
                        bt.grad[0] = 0
                    opt.step()
                    return lv.detach()

                lv_new, g_new = seq_engine.pool_grads(E, b, seq, neg, "bpr", mask_count=count, checked=True)
                lv_old = seq_engine.pool_loss_torch(Et, bt, seq, neg, "bpr")
                gE, gb = torch.autograd.grad(lv_old, [Et, bt])
                gE[0] = 0
                gb[0] = 0
                diff = float(max((g_new[:, :d] - gE).abs().max(), (g_new[:, d] - gb).abs().max()))
                loss_diff = abs(float(lv_new) - float(lv_old))
                for _ in range(3):
                    new(), old()
                t_new, t_old = [], []
                for _ in range(args.reps):
                    t_new += timed(new, 1)
                    t_old += timed(old, 1)
                bound = max((4.0 * count * (d + 1) * 4 + 7.0 * I * (d + 1) * 4) / PEAK_HBM,
                            8.0 * d * count / PEAK_FP32_MFMA) * 1e3
                r = {"metric": "seq_pool", "workload": "train_step", "dim": d, "B": B, "L": L, "items": I, "loss": "bpr",
                     "reps": args.reps, "kernel_ms": stats(t_new), "torch_ms": stats(t_old),
                     "median_ratio_torch_over_kernel": float(np.median(t_old) / np.median(t_new)),
                     "max_abs_grad_diff": diff, "abs_loss_diff": loss_diff, "bound_ms": bound,
                     "kernel_over_bound": float(np.median(t_new) / bound)}
                print(json.dumps(r), flush=True)
                out.append(r)
                del opt, Et, bt, E, b, mom, grad
        # serving: one recommend_next block of 4096 sequences of 50 items, k = 10
        model = ImplicitSequenceModel(embedding_dim=d)
        model.set_tables(E0, torch.zeros(I), device=dev)
        rs = np.random.RandomState(d)
        seqs = rs.randint(1, I, (4096, 50))
        seq_dev = torch.from_numpy(seqs).to(dev)

        def new_rec():
            return model.recommend_next(seqs, 10)

        def old_rec():
            _, rL = seq_engine.pool_reprs_torch(model.item_embeddings, seq_dev)
            blk = rL @ model.item_embeddings.T + model.item_biases[None, :]
            blk[:, 0] = float("-inf")
            blk.scatter_(1, seq_dev, float("-inf"))
            return torch.topk(blk, 10, dim=1).indices.cpu().numpy()

        for _ in range(2):
            a, c = new_rec(), old_rec()
        t_new, t_old = [], []
        for _ in range(args.reps):
            t_new += timed(new_rec, 1)
            t_old += timed(old_rec, 1)
        r = {"metric": "seq_pool", "workload": "recommend_next", "dim": d, "sequences": 4096, "L": 50, "items": I,
             "k": 10, "reps": args.reps, "kernel_ms": stats(t_new), "torch_ms": stats(t_old),
             "median_ratio_torch_over_kernel": float(np.median(t_old) / np.median(t_new)),
             "rows_with_other_ids": int((a != c).any(axis=1).sum())}
        print(json.dumps(r), flush=True)
        out.append(r)
        del model
        torch.cuda.empty_cache()
    return out


def main_seq_cnn(args):
    """``--metric seq_cnn``: one training step of the causal-convolution sequence model
    (rg_seq_cnn_grads + rg_seq_adam_dense + rg_seq_adam_flat) and one recommend_next block against
    the torch ops they replace, for the default net (w 3, 1 layer, tanh, residual) and a 3-layer
    net (w 3, dilations 1 / 2 / 4).  ``gemm_bound_ms``: the three GEMM stages of every layer (the
    convolution, the input gradient, the weight gradient: 2 R w d^2 flops each over R = B (L + 1)
    rows) at the fp32 MFMA peak, against their compulsory traffic at 8 TB/s (per layer 9 R d floats:
    the input read, x and y written, dx and y read twice, the input gradient written, the input read
    again); ``grads_ms`` is rg_seq_cnn_grads alone, of which the GEMM stages are all but the score
    and loss launches.  ``bound_ms`` of the step adds the dense Adam pass's 7 floats per parameter."""
    from . import seq_engine
    from .spotlight.sequence import ImplicitSequenceModel
    from .spotlight.sequence.representations import CNNNet
    dev = torch.device("cuda:0")
    I, lr = args.items, 1e-2
    nets = (("w3", dict(kernel_width=3, dilation=1, num_layers=1)),
            ("w3x3_d124", dict(kernel_width=3, dilation=(1, 2, 4), num_layers=3)))
    out = []
    for d in (32, 64, 128):
        for name, kw in nets:
            torch.manual_seed(d)
            net = CNNNet(I, embedding_dim=d, **kw)
            cfg = seq_engine.cnn_config_of(net)
            E0 = net.item_embeddings.weight.data.clone()
            p0 = seq_engine.cnn_pack(cfg, [(c.weight.data, c.bias.data) for c in net.cnn_layers])
            wd2 = sum(cfg.width[l] for l in range(cfg.num_layers)) * d * d
            for B in (256, 4096):
                for L in (10, 50):
                    rs = np.random.RandomState(B + L + d)
                    seq = torch.from_numpy(rs.randint(1, I, (B, L))).to(dev)
                    seq[: B // 4, : L // 2] = 0
                    neg = torch.from_numpy(rs.randint(0, I, (1, B, L))).to(dev)
                    count = int((seq != 0).sum())
                    E, b, p = E0.to(dev).clone(), torch.zeros(I, device=dev), p0.to(dev).clone()
                    mom = [torch.zeros_like(E), torch.zeros_like(E), torch.zeros_like(b), torch.zeros_like(b)]
                    pmom = [torch.zeros_like(p), torch.zeros_like(p)]
                    grad, pg = torch.zeros(I, d + 1, device=dev), torch.zeros_like(p)
                    ws = seq_engine.cnn_workspace(cfg, B, L, 1, dev)
                    Et, bt, pt = (x.clone().requires_grad_(True) for x in (E, b, p))
                    opt = torch.optim.Adam([Et, bt, pt], lr=lr)

                    def grads():
                        return seq_engine.cnn_grads(cfg, E, b, p, seq, neg, "bpr", grad=grad, mask_count=count,
                                                    checked=True, param_grad=pg, workspace=ws)[0]

                    def new():
                        lv = grads()
                        seq_engine.adam_dense(E, b, *mom, grad, 1, lr)
                        seq_engine.adam_flat(p, *pmom, pg, 1, lr)
                        return lv

                    def old():
                        opt.zero_grad(set_to_none=True)
                        lv = seq_engine.cnn_loss_torch(cfg, Et, bt, pt, seq, neg, "bpr")
                        lv.backward()
                        with torch.no_grad():
                            Et.grad[0] = 0
                            bt.grad[0] = 0
                        opt.step()
                        return lv.detach()

                    lv_new, g_new, pg_new = seq_engine.cnn_grads(cfg, E, b, p, seq, neg, "bpr", mask_count=count,
                                                                 checked=True)
                    lv_old = seq_engine.cnn_loss_torch(cfg, Et, bt, pt, seq, neg, "bpr")
                    gE, gb, gp = torch.autograd.grad(lv_old, [Et, bt, pt])
                    gE[0] = 0
                    gb[0] = 0
                    diff = float(max((g_new[:, :d] - gE).abs().max(), (g_new[:, d] - gb).abs().max(),
                                     (pg_new - gp).abs().max()))
                    loss_diff = abs(float(lv_new) - float(lv_old.detach()))
                    for _ in range(3):
                        new(), old()
                    t_new, t_old, t_grads = [], [], []
                    for _ in range(args.reps):
                        t_new += timed(new, 1)
                        t_old += timed(old, 1)
                    for _ in range(args.reps):      # the gradient call alone; the Adam passes zero grad
                        t_grads += timed(grads, 1)
                        seq_engine.adam_dense(E, b, *mom, grad, 1, lr)
                    R = B * (L + 1)
                    gemm = max(6.0 * R * wd2 / PEAK_FP32_MFMA, 9.0 * R * d * cfg.num_layers * 4 / PEAK_HBM) * 1e3
                    bound = gemm + 7.0 * (I * (d + 1) + p.numel()) * 4 / PEAK_HBM * 1e3
                    r = {"metric": "seq_cnn", "workload": "train_step", "net": name, "dim": d, "B": B, "L": L,
                         "items": I, "loss": "bpr", "reps": args.reps, "kernel_ms": stats(t_new),
                         "torch_ms": stats(t_old), "grads_ms": stats(t_grads),
                         "median_ratio_torch_over_kernel": float(np.median(t_old) / np.median(t_new)),
                         "max_abs_grad_diff": diff, "abs_loss_diff": loss_diff, "gemm_gflop": 6.0 * R * wd2 / 1e9,
                         "gemm_bound_ms": gemm, "gemm_bound_share_of_grads": float(gemm / np.median(t_grads)),
                         "bound_ms": bound, "kernel_over_bound": float(np.median(t_new) / bound)}
                    print(json.dumps(r), flush=True)
                    out.append(r)
                    del opt, Et, bt, pt, E, b, p, mom, pmom, grad, pg, ws
            # serving: one recommend_next block of 4096 sequences of 50 items, k = 10
            model = ImplicitSequenceModel(representation=net)
            model.set_tables(E0, torch.zeros(I), device=dev)
            rs = np.random.RandomState(d)
            seqs = rs.randint(1, I, (4096, 50))
            seq_dev = torch.from_numpy(seqs).to(dev)

            def new_rec():
                return model.recommend_next(seqs, 10)

            def old_rec():
                rL = seq_engine.cnn_repr_torch(cfg, model.item_embeddings, model._conv, seq_dev)
                blk = rL @ model.item_embeddings.T + model.item_biases[None, :]
                blk[:, 0] = float("-inf")
                blk.scatter_(1, seq_dev, float("-inf"))
                return torch.topk(blk, 10, dim=1).indices.cpu().numpy()

            for _ in range(2):
                a, c = new_rec(), old_rec()
            t_new, t_old = [], []
            for _ in range(args.reps):
                t_new += timed(new_rec, 1)
                t_old += timed(old_rec, 1)
            r = {"metric": "seq_cnn", "workload": "recommend_next", "net": name, "dim": d, "sequences": 4096, "L": 50,
                 "items": I, "k": 10, "reps": args.reps, "kernel_ms": stats(t_new), "torch_ms": stats(t_old),
                 "median_ratio_torch_over_kernel": float(np.median(t_old) / np.median(t_new)),
                 "rows_with_other_ids": int((a != c).any(axis=1).sum())}
            print(json.dumps(r), flush=True)
            out.append(r)
            del model
            torch.cuda.empty_cache()
    return out


def main_scores(args):
    """The default mode: one block of ``--users`` users against every item, NCFEngine.score_users
    (rg_ncf_score_users) against the pairwise NCFEngine.scores_torch."""
    dev = torch.device("cuda:0")
    U, I, n = 138493, args.items, args.users
    out = []
    for name, E, M in (("ncf_e64", 64, 0), ("neumf_e16_m50", 16, 50)):
        e = make_engine(E, M, U, I, dev)
        users = torch.from_numpy(np.random.RandomState(1).randint(0, U, n)).to(dev)
        pu, pi = users.repeat_interleave(I), torch.arange(I, device=dev).repeat(n)
        new = lambda: e.score_users(users)
        old = lambda: e.scores_torch(pu, pi)
        for _ in range(3):                                   # warm-up: code objects, GEMM algorithms, allocator
            a, b = new(), old().reshape(n, I)
        torch.cuda.synchronize()
        diff = (a - b).abs()
        rel = float((diff / b.abs()).max())
        t_new, t_old = [], []
        for _ in range(args.reps):                           # alternate the two paths
            t_new += timed(new, 1)
            t_old += timed(old, 1)
        flops, bytes_ = algorithmic(E, M, n, I)
        tn = min(t_new) * 1e-3
        r = {"model": name, "users": n, "items": I, "reps": args.reps,
             "kernel_ms": stats(t_new), "pairwise_ms": stats(t_old),
             "speedup_min": min(t_old) / min(t_new), "speedup_median": float(np.median(t_old) / np.median(t_new)),
             "max_abs_diff": float(diff.max()), "max_rel_diff": rel,
             "gflop": flops / 1e9, "mbytes": bytes_ / 1e6,
             "frac_fp32_mfma_peak": flops / tn / PEAK_FP32_MFMA, "frac_hbm_peak": bytes_ / tn / PEAK_HBM}
        if args.big:
            ub = torch.from_numpy(np.random.RandomState(2).randint(0, U, args.big)).to(dev)
            big = lambda: e.score_users(ub)
            big()
            tb = timed(big, max(3, args.reps // 4))
            fb, _ = algorithmic(E, M, args.big, I)
            r["big"] = {"users": args.big, "kernel_ms": stats(tb),
                        "frac_fp32_mfma_peak": fb / (min(tb) * 1e-3) / PEAK_FP32_MFMA,
                        "pairwise": "not run: its concatenated input alone is users x items x 2E floats"}
        print(json.dumps(r), flush=True)
        out.append(r)
        del e
        torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--metric", choices=("scores", "mrr", "slates", "pairs", "mf_scores", "mf_topk", "item_sim",
                                        "gan_recommend", "topk_wide", "gan_score", "fold_in", "candidates", "mmr",
                                        "als", "seq_pool", "seq_cnn"),
                    default="scores")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--users", type=int, default=None)
    ap.add_argument("--hist-len", type=int, default=128)
    ap.add_argument("--items", type=int, default=26744)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--test-users", type=int, default=4096)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    args = ap.parse_args(argv)
    slates = args.metric == "slates"             # its own defaults: every ML-20M user, 5 repetitions
    if args.users is None:
        args.users = ML20M_USERS if slates else 138493 if args.metric == "als" else 256
    if args.reps is None:
        args.reps = 5 if slates or args.metric == "pairs" else 20
    return {"scores": main_scores, "mrr": main_mrr, "slates": main_slates, "pairs": main_pairs,
            "mf_scores": main_mf_scores, "mf_topk": main_mf_topk, "item_sim": main_item_sim,
            "gan_recommend": main_gan_recommend, "topk_wide": main_topk_wide,
            "gan_score": main_gan_score, "fold_in": main_fold_in, "candidates": main_candidates,
            "mmr": main_mmr, "als": main_als, "seq_pool": main_seq_pool,
            "seq_cnn": main_seq_cnn}[args.metric](args)


if __name__ == "__main__":
    main()
