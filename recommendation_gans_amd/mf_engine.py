"""Device-resident MF training engine: the fused replacement of
``ImplicitFactorizationModel.run_train_iteration`` (implicit.py:347-364).

Everything of the step lives in HBM and is only touched by librg_hip.so:

    tables   user_w (U,d) item_w (I,d) user_b (U,) item_b (I,)   x2 (ping-pong)
    optim    m, v of the same shapes (Adam), v only (RMSprop), none (SGD)
    pool     negative pool as int32 (user, item) pairs, 8 B per entry
    sampler  CPython MT19937 state (624 words + position) and two word buffers
    scratch  per-row contribution counters/lists, overflow accumulators, loss partials

Per step: rg_mf_pairs (forward, loss, dL/dz, contribution lists) then
rg_mf_apply_prepare (pull gradients + optimizer over every row, and the next
step's draws -> pool pairs in the same launch).  The native stepper
(rg_stepper.cpp) generates the MT19937 words in 8-step slots ahead of use on a
stream of its own, so the sequential sampler is off the critical path.
"""
import ctypes
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import LOSS_KINDS, OPT_KINDS, RG_MF_LIST_CAP, RG_MF_MAX_NEG, RG_MT_PAD, check, ptr


def _as_u32_tensor(words, device):
    a = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    return torch.from_numpy(a.view(np.int32)).to(device)


class DeviceSampler:
    """CPython ``random`` stream on the GPU, bit-exact with ``random.choices``.

    ``acquire(nwords)`` returns an int32 tensor holding the next ``nwords``
    raw MT state words (bit pattern of uint32; tempered by the consumer) whose producer the current stream
    has waited for; ``release()`` must follow the launch of the consumer and
    starts generating the following ``nwords`` words on the side stream.
    """

    def __init__(self, mt_state, device, prefetch=True):
        self.device = torch.device(device)
        self.state = _as_u32_tensor(mt_state, self.device)
        self.state_before = torch.empty(625, dtype=torch.int32, device=self.device)
        self.prefetch = prefetch
        self.side = torch.cuda.Stream(device=self.device)
        self.bufs = [None, None]
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]
        self.consumed = [None, None]
        self.pending = None      # (buffer index, nwords)
        self.cur = None

    def _gen(self, b, nwords):
        if self.bufs[b] is None or self.bufs[b].numel() < nwords:
            with torch.cuda.stream(self.side):
                self.bufs[b] = torch.empty(nwords + RG_MT_PAD, dtype=torch.int32, device=self.device)
        with torch.cuda.stream(self.side):
            if self.consumed[b] is not None:
                self.side.wait_event(self.consumed[b])
            check(_lib.load().rg_mt_generate(_lib.stream_handle(self.side), ptr(self.state), ptr(self.bufs[b]),
                                             nwords, ptr(self.state_before)), "rg_mt_generate")
            self.ready[b].record(self.side)

    def _discard_pending(self):
        if self.pending is None:
            return
        with torch.cuda.stream(self.side):
            self.state.copy_(self.state_before)   # ordered after the prefetch on the side stream
        self.pending = None

    def acquire(self, nwords):
        cur = torch.cuda.current_stream(self.device)
        if self.pending is not None and self.pending[1] == nwords:
            b = self.pending[0]
            self.pending = None
        else:
            self._discard_pending()
            b = 0 if self.cur is None else 1 - self.cur
            self._gen(b, nwords)
        cur.wait_event(self.ready[b])
        self.cur = b
        self._nwords = nwords
        return self.bufs[b]

    def release(self):
        b = self.cur
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.consumed[b] = ev
        if self.prefetch:
            nb = 1 - b
            self._gen(nb, self._nwords)
            self.pending = (nb, self._nwords)

    def export_state(self):
        """625-word state after the last CONSUMED word (prefetched words are not drawn)."""
        self.side.synchronize()
        torch.cuda.current_stream(self.device).synchronize()
        src = self.state_before if self.pending is not None else self.state
        return src.cpu().numpy().view(np.uint32).copy()

    def import_state(self, mt_state):
        self.side.synchronize()
        self.pending = None
        self.state.copy_(_as_u32_tensor(mt_state, self.device))


def score_users_torch(U, I, ub, ib, users):
    """The (len(users), num_items) score block as a chain of torch ops (gather, one GEMM, two
    broadcast adds, sigmoid): what the evaluation ran before rg_mf_score_users, what it still
    runs for tables the kernel does not take, and the timing baseline of ``score_users_block``."""
    return torch.sigmoid(U[users] @ I.T + ub[users][:, None] + ib[None, :])


def score_block_on_device(U, I, ub, ib):
    """True if ``score_users_block`` takes these tables: all four on one CUDA device, float32,
    contiguous, a dim the kernel has."""
    tabs = (U, I, ub, ib)
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == U.device
               for t in tabs) and U.dim() == 2 and I.dim() == 2 and 1 <= U.shape[1] <= 256 and \
        I.shape[1] == U.shape[1] and I.shape[0] >= 1 and ub.numel() == U.shape[0] and ib.numel() == I.shape[0]


def score_users_block(U, I, ub, ib, users, checked=False):
    """Scores of ``users`` against every item, (len(users), num_items) float32 on the tables'
    device: sigmoid((<U[u], I[i]> + ub[u]) + ib[i]) in one fused launch (rg_mf_score_users: the
    product on the fp32 MFMA, bias and sigmoid in registers, one store per score).  A (user, item)
    score is the same bits wherever the user stands in the block.  The tables (float32, contiguous,
    on one CUDA device) are only read; an id outside [0, U.shape[0]) raises ValueError (one
    download of the ids' bounds; ``checked=True``: the caller has checked these ids already)."""
    if not score_block_on_device(U, I, ub, ib):
        raise ValueError("score_users_block needs contiguous float32 tables of matching shapes on one CUDA device")
    dev = U.device
    users = torch.as_tensor(users).to(dev, torch.int64).reshape(-1).contiguous()
    n, num_items = int(users.numel()), int(I.shape[0])
    out = torch.empty(n, num_items, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if not checked:
        lo, hi = torch.stack(users.aminmax()).tolist()
        if lo < 0 or hi >= U.shape[0]:
            raise ValueError("user ids outside the user table")
    with torch.cuda.device(dev):
        check(_lib.load().rg_mf_score_users(_lib.stream_handle(), ptr(U), ptr(I), ptr(ub), ptr(ib), int(U.shape[1]),
                                            num_items, ptr(users), n, ptr(out), num_items), "rg_mf_score_users")
    return out


def _topk_setup(ids, dev, k, splits, ws_len_fn, num_rows, limit, outside):
    """What the fused top-k calls do ahead of their launch: ``ids`` on ``dev`` as contiguous int64,
    the (n, k) int32 id and float32 value outputs, and the workspace of the library's
    ``ws_len_fn(num_rows, n, k, splits)`` bytes (ValueError with the library's reason for a shape
    it refuses).  ``limit`` not None: ValueError(``outside``) for an id outside [0, limit).
    Returns (ids, out_ids, out_values, workspace); n == 0: nothing was checked beyond the shape
    and there is no workspace (None)."""
    ids = torch.as_tensor(ids).to(dev, torch.int64).reshape(-1).contiguous()
    n = int(ids.numel())
    out_ids = torch.empty(n, k, dtype=torch.int32, device=dev)
    out_values = torch.empty(n, k, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws_len = int(getattr(lib, ws_len_fn)(num_rows, n, k, splits))
    if ws_len < 0:
        raise ValueError(ws_len_fn + ": " + lib.rg_last_error().decode(errors="replace"))
    if n == 0:
        return ids, out_ids, out_values, None
    if limit is not None:
        lo, hi = torch.stack(ids.aminmax()).tolist()
        if lo < 0 or hi >= limit:
            raise ValueError(outside)
    return ids, out_ids, out_values, torch.empty(max(ws_len, 8) // 4, dtype=torch.int32, device=dev)


def topk_users_fused(U, I, ub, ib, users, k, exc_ptr=None, exc_idx=None, splits=0, checked=False):
    """The k best items of ``users`` and their scores, ``(ids int32 [n, k], scores float32 [n, k])``
    on the tables' device, in one fused launch (rg_mf_topk_users; a second small one merges the
    item splits): the scores of ``score_users_block`` bit for bit, -inf over the excluded entries,
    ranked by (score descending, item id ascending) as rg_topk_rows ranks them -- without the
    (len(users), num_items) block.  ``exc_ptr`` (int64 [n + 1]) and ``exc_idx`` (int32) are a CSR
    over the rows of ``users``, on the host or the device, each row's ids ASCENDING; an id outside
    [0, num_items) is ignored; both None: nothing excluded.  ``splits``: item splits per user group
    (0: the library picks).  The tables (those ``score_block_on_device`` accepts) are only read; a
    user id outside [0, U.shape[0]) raises ValueError (one download of the ids' bounds;
    ``checked=True``: the caller has checked these ids already)."""
    if not score_block_on_device(U, I, ub, ib):
        raise ValueError("topk_users_fused needs contiguous float32 tables of matching shapes on one CUDA device")
    if (exc_ptr is None) != (exc_idx is None):
        raise ValueError("exc_ptr and exc_idx go together")
    dev, num_items, k, splits = U.device, int(I.shape[0]), int(k), int(splits)
    users, ids, scores, ws = _topk_setup(users, dev, k, splits, "rg_mf_topk_workspace_len", num_items,
                                         None if checked else U.shape[0], "user ids outside the user table")
    n = int(users.numel())
    if n == 0:
        return ids, scores
    if exc_ptr is not None:
        exc_ptr = torch.as_tensor(exc_ptr).to(dev, torch.int64).reshape(-1).contiguous()
        exc_idx = torch.as_tensor(exc_idx).to(dev, torch.int32).reshape(-1).contiguous()
        if exc_ptr.numel() != n + 1:
            raise ValueError("exc_ptr must have len(users) + 1 entries")
        if not checked:                                 # the kernel trusts exc_ptr to describe exc_idx
            bad = (exc_ptr[0] < 0) | (exc_ptr[-1] > exc_idx.numel()) | (exc_ptr[1:] < exc_ptr[:-1]).any()
            if bool(bad):
                raise ValueError("exc_ptr must ascend from >= 0 to <= len(exc_idx)")
        if exc_idx.numel() == 0:                        # nothing to exclude (and no pointer to pass)
            exc_ptr = exc_idx = None
    with torch.cuda.device(dev):
        check(_lib.load().rg_mf_topk_users(_lib.stream_handle(), ptr(U), ptr(I), ptr(ub), ptr(ib), int(U.shape[1]), num_items,
                                   ptr(users), n, ptr(exc_ptr), ptr(exc_idx), k, splits, ptr(ws), ptr(ids),
                                   ptr(scores)), "rg_mf_topk_users")
    return ids, scores


SIM_METRICS = ("cosine", "dot")


def _sim_table(table, what):
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.float32 and table.dim() == 2 and
            table.is_contiguous() and 1 <= table.shape[1] <= 256 and table.shape[0] >= 1):
        raise ValueError(f"{what} needs a contiguous float32 (rows, dim <= 256) table on a CUDA device")


def row_rnorms(table):
    """1 / sqrt(sum of squares) of every row of ``table`` (contiguous float32 (rows, dim) on a CUDA
    device), float32 (rows,) on its device, exactly 0 for a zero row (rg_row_rnorms).  A row's value
    is the same bits whatever the row count."""
    _sim_table(table, "row_rnorms")
    out = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        check(_lib.load().rg_row_rnorms(_lib.stream_handle(), ptr(table), int(table.shape[0]), int(table.shape[1]),
                                        ptr(out)), "rg_row_rnorms")
    return out


def similar_rows(table, queries, k, metric="cosine", exclude_self=True, rnorm=None, splits=0, checked=False):
    """The k rows of ``table`` most similar to each row id of ``queries``: ``(ids int32 [n, k], sims
    float32 [n, k])`` on the table's device, in one fused launch (rg_item_sim_topk; a second small
    one merges the row splits), without the (queries, rows) block.  ``metric``: "cosine" --
    ``(dot * rnorm[q]) * rnorm[c]`` with the reciprocal norms of ``row_rnorms`` (computed here unless
    ``rnorm`` brings them) -- or "dot", the inner product itself.  Ranked by (similarity descending,
    row id ascending), NaN last; ``exclude_self`` leaves the query's own row out (k <= rows - 1
    then).  ``splits``: row splits per query group (0: the library picks).  The table (contiguous
    float32 (rows, dim <= 256) on a CUDA device: anything else raises, there is no fall-back) is only
    read; a query id outside [0, rows) raises ValueError (one download of the ids' bounds;
    ``checked=True``: the caller has checked these ids already)."""
    _sim_table(table, "similar_rows")
    if metric not in SIM_METRICS:
        raise ValueError(f"unknown metric {metric!r}: one of {SIM_METRICS}")
    dev, rows, k, splits = table.device, int(table.shape[0]), int(k), int(splits)
    if k < 1 or k > min(32, rows - (1 if exclude_self else 0)):
        raise ValueError("k must be in [1, min(32, rows)] (rows - 1 with exclude_self)")
    queries, ids, sims, ws = _topk_setup(queries, dev, k, splits, "rg_item_sim_workspace_len", rows,
                                         None if checked else rows, "query ids outside the table")
    n = int(queries.numel())
    if n == 0:
        return ids, sims
    if metric == "cosine":
        if rnorm is None:
            rnorm = row_rnorms(table)
        elif not (torch.is_tensor(rnorm) and rnorm.device == dev and rnorm.dtype == torch.float32 and
                  rnorm.is_contiguous() and rnorm.numel() == rows):
            raise ValueError("rnorm must be a contiguous float32 tensor of one value per row on the table's device")
    else:
        rnorm = None
    with torch.cuda.device(dev):
        check(_lib.load().rg_item_sim_topk(_lib.stream_handle(), ptr(table), ptr(rnorm), int(table.shape[1]), rows,
                                   ptr(queries), n, _lib.RG_SIM_EXCLUDE_SELF if exclude_self else 0, k, splits,
                                   ptr(ws), ptr(ids), ptr(sims)), "rg_item_sim_topk")
    return ids, sims


FOLD_LOSSES = ("pointwise", "bpr", "hinge", "adaptive_hinge")
FOLD_MAX_NEG, FOLD_MAX_STEPS = 32, 1024     # rg_mf_fold_in_users' ranges


def adam_step_coef(steps, lr, betas):
    """(steps, 2) float64: torch.optim.Adam's per-step scalars of steps 1..steps, evaluated in double
    as its Python code does -- step_size = lr / (1 - beta1^t), bias_correction2_sqrt =
    sqrt(1 - beta2^t) (what rg_opt_t carries for one step)."""
    out = np.empty((int(steps), 2), dtype=np.float64)
    for t in range(1, int(steps) + 1):
        out[t - 1, 0] = float(lr) / (1.0 - float(betas[0]) ** t)
        out[t - 1, 1] = (1.0 - float(betas[1]) ** t) ** 0.5
    return out


def _fold_args(item_w, item_b, hist_ptr, hist_idx, neg_idx, n_neg, loss, steps, init, checked, what):
    """The argument checks both fold-in paths share (ValueError, before anything touches a device
    kernel): returns (hist_ptr, hist_idx, neg_idx [nnz, n_neg], n, dim) with the id
    arrays flat integer tensors, in the dtypes and on the devices they came in."""
    if not (torch.is_tensor(item_w) and torch.is_tensor(item_b) and item_w.dtype == item_b.dtype and
            item_w.dtype in (torch.float32, torch.float64)):
        raise ValueError(f"{what}: the item tables must be floating-point tensors of one dtype")
    if item_w.dim() != 2 or item_w.shape[0] < 1 or item_b.numel() != item_w.shape[0]:
        raise ValueError(f"{what}: item_w must be (num_items >= 1, dim) and item_b hold one value per item")
    num_items, dim = int(item_w.shape[0]), int(item_w.shape[1])
    if dim < 1 or dim > 256:
        raise ValueError(f"{what}: dim must be in [1, 256]")
    if loss not in FOLD_LOSSES:
        raise ValueError(f"{what}: unknown loss {loss!r}: one of {FOLD_LOSSES}")
    n_neg, steps = int(n_neg), int(steps)
    if n_neg < 0 or n_neg > FOLD_MAX_NEG:
        raise ValueError(f"{what}: n_neg must be in [0, {FOLD_MAX_NEG}]")
    if n_neg == 0 and loss != "pointwise":
        raise ValueError(f"{what}: the pairwise losses need n_neg >= 1")
    if steps < 0 or steps > FOLD_MAX_STEPS:
        raise ValueError(f"{what}: steps must be in [0, {FOLD_MAX_STEPS}]")
    ints = (torch.int32, torch.int64)
    hist_ptr, hist_idx = torch.as_tensor(hist_ptr), torch.as_tensor(hist_idx)
    neg_idx = torch.as_tensor(neg_idx) if neg_idx is not None else torch.zeros(0, dtype=torch.int32)
    if hist_ptr.dtype not in ints or hist_idx.dtype not in ints or neg_idx.dtype not in ints:
        raise ValueError(f"{what}: hist_ptr, hist_idx and neg_idx must be int32 or int64")
    hist_ptr, hist_idx, neg_idx = hist_ptr.reshape(-1), hist_idx.reshape(-1), neg_idx.reshape(-1)
    if hist_ptr.numel() < 1:
        raise ValueError(f"{what}: hist_ptr must have n_users + 1 entries")
    n, nnz = int(hist_ptr.numel()) - 1, int(hist_idx.numel())
    if neg_idx.numel() != nnz * n_neg:
        raise ValueError(f"{what}: neg_idx must hold n_neg ids per history entry")
    if not checked:
        bad = (hist_ptr[0] != 0) | (hist_ptr[-1] != nnz) | (hist_ptr[1:] < hist_ptr[:-1]).any()
        if bool(bad):
            raise ValueError(f"{what}: hist_ptr must ascend from 0 to len(hist_idx)")
        for name, ids in (("hist_idx", hist_idx), ("neg_idx", neg_idx)):
            if ids.numel():
                lo, hi = torch.stack(ids.aminmax()).tolist()
                if lo < 0 or hi >= num_items:
                    raise ValueError(f"{what}: {name} holds an item id outside [0, num_items)")
    if init is not None:
        if not (isinstance(init, (tuple, list)) and len(init) == 2 and torch.is_tensor(init[0]) and
                torch.is_tensor(init[1]) and tuple(init[0].shape) == (n, dim) and init[1].numel() == n):
            raise ValueError(f"{what}: init must be (W [n_users, dim], b [n_users]) tensors")
    return hist_ptr, hist_idx, neg_idx.reshape(nnz, n_neg), n, dim


def fold_in_users(item_w, item_b, hist_ptr, hist_idx, neg_idx, n_neg, *, loss, steps, lr, weight_decay=0.0,
                  betas=(0.9, 0.999), eps=1e-8, init=None, return_loss=False, checked=False):
    """Fit the rows of NEW users against the frozen item tables (fold-in): ``(W [n, dim], b [n])``
    float32 on the tables' device, with ``return_loss`` also ``loss [n]``, the loss at the last
    step's parameters before its update.  One launch (rg_mf_fold_in_users): a user's row, bias and
    Adam moments stay in registers for all ``steps``; the item tables are only read.

    User r's history is the CSR row ``hist_idx[hist_ptr[r]:hist_ptr[r + 1]]`` (duplicates count as
    given, an empty row is left at its start), negative j of history entry e is ``neg_idx[e * n_neg
    + j]`` -- the same draws at every step.  ``loss``: one of ``FOLD_LOSSES``, spotlight/losses.py
    on that one user's pairs with prediction sigmoid(<w, Q_i> + b + c_i); the adaptive hinge takes
    the maximum over each positive's own ``n_neg`` negatives (the training step's maximum over the
    whole batch is a quirk of the reference's flat shapes and means nothing for one user).
    ``steps`` full-batch steps of torch's Adam (``lr``, ``betas``, ``eps``, coupled
    ``weight_decay``) from ``init = (W0, b0)``, zeros by default.

    ValueError for tables that are not contiguous float32 on one CUDA device (there is no torch
    fall-back), dim outside [1, 256], n_neg outside [0, 32] (0 only with the pointwise loss), steps
    outside [0, 1024], index arrays that are not integers, a ``hist_ptr`` that does not ascend from
    0 to len(hist_idx), and an item id outside [0, num_items) (one download of the ids' bounds;
    ``checked=True``: the caller has checked pointers and ids already)."""
    what = "fold_in_users"
    if not (torch.is_tensor(item_w) and torch.is_tensor(item_b) and item_w.dtype == torch.float32 and
            item_b.dtype == torch.float32):
        raise ValueError(f"{what}: the item tables must be float32 tensors")
    hp, hi, ni, n, dim = _fold_args(item_w, item_b, hist_ptr, hist_idx, neg_idx, n_neg, loss, steps, init, checked,
                                    what)
    n_neg, steps = int(n_neg), int(steps)
    if not (item_w.is_cuda and item_w.dtype == torch.float32 and item_w.is_contiguous() and item_b.is_contiguous()
            and item_b.device == item_w.device):
        raise ValueError(f"{what} needs contiguous float32 item tables on one CUDA device")
    dev, num_items = item_w.device, int(item_w.shape[0])
    if init is None:
        W = torch.zeros(n, dim, dtype=torch.float32, device=dev)
        b = torch.zeros(n, dtype=torch.float32, device=dev)
    else:
        W = init[0].detach().to(dev, torch.float32, copy=True).contiguous()
        b = init[1].detach().to(dev, torch.float32, copy=True).reshape(-1).contiguous()
    out_loss = torch.zeros(n, dtype=torch.float32, device=dev) if return_loss else None
    if n and steps and hi.numel():
        hp = hp.to(dev, torch.int64).contiguous()
        hi32 = hi.to(dev, torch.int32).contiguous()
        ni32 = ni.to(dev, torch.int32).contiguous() if n_neg else None
        coef = torch.from_numpy(adam_step_coef(steps, lr, betas).astype(np.float32)).to(dev)
        o = _lib.Opt()
        o.kind = OPT_KINDS["adam"]
        o.lr, o.beta1, o.beta2, o.eps, o.weight_decay = lr, betas[0], betas[1], eps, weight_decay
        o.one_minus_beta1, o.one_minus_beta2 = 1 - betas[0], 1 - betas[1]
        with torch.cuda.device(dev):
            check(_lib.load().rg_mf_fold_in_users(_lib.stream_handle(), ptr(item_w), ptr(item_b), dim, num_items,
                                                  ptr(hp), ptr(hi32), ptr(ni32), n_neg, n, LOSS_KINDS[loss],
                                                  ctypes.byref(o), ptr(coef), steps, ptr(W), ptr(b), ptr(out_loss)),
                  "rg_mf_fold_in_users")
    return (W, b, out_loss) if return_loss else (W, b)


def fold_row_losses(loss, sp, sn, mask, P, n_neg):
    """Per-row fold-in losses from padded predictions: ``sp`` (n, L) the positives', ``sn`` (n, L,
    n_neg) their negatives', ``mask`` (n, L) True at real entries, ``P`` (n,) the row lengths as
    floats (an empty row's loss is 0)."""
    Pc = P.clamp(min=1.0)
    zero = sp.new_zeros(())
    if loss == "pointwise":
        out = -torch.where(mask, torch.clamp(torch.log(sp), min=-100.0), zero).sum(1) / Pc
        if n_neg:
            neg = torch.where(mask[:, :, None], torch.clamp(torch.log(1.0 - sn), min=-100.0), zero)
            out = out - neg.sum((1, 2)) / (Pc * n_neg)
        return out
    if loss == "bpr":
        term = 1.0 - torch.sigmoid(sp[:, :, None] - sn)
    elif loss == "hinge":
        term = torch.clamp(sn - sp[:, :, None] + 1.0, min=0.0)
    else:
        return torch.where(mask, torch.clamp(sn.max(dim=2).values - sp + 1.0, min=0.0), zero).sum(1) / Pc
    return torch.where(mask[:, :, None], term, zero).sum((1, 2)) / (Pc * n_neg)


def fold_in_users_torch(item_w, item_b, hist_ptr, hist_idx, neg_idx, n_neg, *, loss, steps, lr, weight_decay=0.0,
                        betas=(0.9, 0.999), eps=1e-8, init=None, return_loss=False, checked=False):
    """``fold_in_users`` as the chain of torch ops it replaces, on the tables' device and in their
    dtype: the histories padded to the longest row, one (n, L (1 + n_neg), dim) gather per step,
    autograd on the summed per-row losses and ``torch.optim.Adam`` on an (n, dim) and an (n,)
    parameter.  Per-row losses and an elementwise optimizer keep the rows independent; an empty row
    is put back to its start.  The timing baseline of the kernel, and in float64 on the CPU the
    reference of its tests."""
    hp, hi, ni, n, dim = _fold_args(item_w, item_b, hist_ptr, hist_idx, neg_idx, n_neg, loss, steps, init, checked,
                                    "fold_in_users_torch")
    n_neg, steps = int(n_neg), int(steps)
    dev, dt = item_w.device, item_w.dtype
    Q, c = item_w.detach(), item_b.detach().reshape(-1)
    if init is None:
        W0, b0 = torch.zeros(n, dim, dtype=dt, device=dev), torch.zeros(n, dtype=dt, device=dev)
    else:
        W0 = init[0].detach().to(dev, dt, copy=True)
        b0 = init[1].detach().to(dev, dt, copy=True).reshape(-1)
    hp, hi, ni = hp.to(dev, torch.int64), hi.to(dev, torch.int64), ni.to(dev, torch.int64)
    lens = hp[1:] - hp[:-1]
    L = int(lens.max()) if n else 0
    last = torch.zeros(n, dtype=dt, device=dev)
    if n == 0 or steps == 0 or L == 0:
        return (W0, b0, last) if return_loss else (W0, b0)
    col = torch.arange(L, device=dev)
    mask = col[None, :] < lens[:, None]
    src = (hp[:-1, None] + col[None, :]).clamp(max=int(hi.numel()) - 1)
    pos = torch.where(mask, hi[src], torch.zeros((), dtype=torch.int64, device=dev))
    neg = torch.where(mask[:, :, None], ni[src], torch.zeros((), dtype=torch.int64, device=dev))
    W, b = W0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    opt = torch.optim.Adam([W, b], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
    P = lens.to(dt)
    for t in range(steps):
        opt.zero_grad(set_to_none=True)
        sp = torch.sigmoid(torch.einsum("nd,nld->nl", W, Q[pos]) + b[:, None] + c[pos])
        sn = torch.sigmoid(torch.einsum("nd,nlkd->nlk", W, Q[neg]) + b[:, None, None] + c[neg])
        rows = fold_row_losses(loss, sp, sn, mask, P, n_neg)
        if t == steps - 1:
            last = rows.detach().clone()
        rows.sum().backward()
        opt.step()
    W, b = W.detach(), b.detach()
    empty = lens == 0
    W[empty] = W0[empty]
    b[empty] = b0[empty]
    return (W, b, last) if return_loss else (W, b)


MFPlan = namedtuple("MFPlan", "perm pos_slot item_slot_off n_planned", defaults=(None,))


def build_plans(items, batch_size, units_per_block, num_items, *, offset=0, stride=None, n_batches=None,
                users=None, world=1, rank=0, cols=None):
    """Per-batch plans (include/rg_hip.h rg_mf_work_t): positives processed in
    item-sorted column order, one partial slot per (item, pair-kernel block), built on
    the device for every batch in ONE launch (rg_mf_plans_build, rg_plan.hip).

    Batch k covers positives [offset + k*stride, offset + k*stride + batch_size) of
    ``items`` (device int64).  ``world`` > 1: only the positives whose user (``users``)
    this ``rank`` owns (u % world == rank) are planned -- the owner-sharded data-parallel
    step.  The reference shuffles the training set once per fit (implicit.py:262), so
    every epoch revisits the same batches: plans are built once per fit.  Returns a list
    of MFPlan (views into three shared tensors; ``n_planned`` = planned positives)."""
    lib = _lib.load()
    dev = items.device
    stride = stride or batch_size
    n = items.numel()
    if n_batches is None:
        n_batches = max(0, -(-(n - offset) // stride))
    cols = cols or batch_size
    if n_batches == 0:
        return []
    perm = torch.empty(n_batches * cols, dtype=torch.int32, device=dev)
    pos_slot = torch.empty(n_batches * cols, dtype=torch.int32, device=dev)
    off = torch.empty(n_batches * (num_items + 1), dtype=torch.int32, device=dev)
    counts = torch.empty(2 * n_batches, dtype=torch.int32, device=dev)
    for t in (items, users):
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous() or t.device != dev):
            raise ValueError("plan inputs must be contiguous int64 tensors on one device")

    def run(with_scratch):
        sl = int(lib.rg_mf_plans_scratch_len(cols, n_batches)) if with_scratch else 0
        scratch = torch.empty(max(sl, 1), dtype=torch.int64, device=dev) if sl > 0 else None
        check(lib.rg_mf_plans_build(_lib.stream_handle(), ptr(users) if world > 1 else None, ptr(items), n, offset,
                                    stride, batch_size, n_batches, cols, units_per_block, num_items, world, rank,
                                    ptr(perm), ptr(pos_slot), ptr(off), ptr(counts), ptr(scratch)),
              "rg_mf_plans_build")
        return counts.cpu().numpy()[0::2]
    # the owner filter plans ~cols / world positives of a batch: the LDS path, no scratch
    # (~12 B per training positive otherwise); a batch over the LDS capacity reports -1
    planned = run(with_scratch=world <= 1)
    if (planned < 0).any():
        planned = run(with_scratch=True)
    return [MFPlan(perm[k * cols:(k + 1) * cols], pos_slot[k * cols:(k + 1) * cols],
                   off[k * (num_items + 1):(k + 1) * (num_items + 1)], int(planned[k])) for k in range(n_batches)]


def build_plan(pos_i, cols, units_per_block, num_items):
    """The plan of one batch (see build_plans); ``pos_i``: its positives' items."""
    return build_plans(pos_i.contiguous(), max(1, pos_i.numel()), units_per_block, num_items, n_batches=1,
                       cols=cols)[0]


def build_epoch_plans(items, batch_size, units_per_block, num_items, offset=0, stride=None):
    """Plans of every batch of an epoch: batch k covers positives
    [offset + k*stride, offset + k*stride + batch_size) of ``items`` (device int64)."""
    return build_plans(items, batch_size, units_per_block, num_items, offset=offset, stride=stride)


class MFEngine:
    """Owns the device state of one BilinearNet training run on one GPU (one rank) and
    the native step runtime (rg_mf_stepper_*) that enqueues each step."""

    def __init__(self, user_w, item_w, user_b, item_b, pool_u, pool_i, mt_state, *, loss="pointwise",
                 optimizer="adam", lr=1e-3, weight_decay=0.0, betas=(0.5, 0.999), eps=1e-8, alpha=0.99,
                 n_neg=5, batch_size=256, device="cuda", rank=0, world_size=1, prefetch=True,
                 dp=None, comm=None):
        """``dp``: data-parallel layout when world_size > 1 --
        "global_stream" (default, reference-exact): every rank holds every row
            and consumes columns [r*B, (r+1)*B) of ONE global draw of n*B*R indices from
            the full pool, with loss means over the global batch; the rank-major data
            gradient is reduce-scattered, each rank updates its row shard, the tables are
            all-gathered (``comm``: an RcclComm, native in rg_mf_stepper_train; without
            one, ``train_step_exchange`` takes the two collectives as callables).  R ranks
            at batch B compute the reference's step at batch R*B;
        "user_shard" (opt-in, faster, NOT the reference's sampling at R > 1): the tables
            passed are this rank's user shard plus every item (sharding.py); own MT stream,
            own sub-pool and positives, the item gradient is the only exchange (``comm``,
            else ``train_step_sharded``);
        "owner" (default when world_size > 1, reference-exact like "global_stream"): the
            FULL tables are passed and this rank keeps the users u % R == rank (local rows
            u // R) and every item; every rank walks the one global draw over the full pool
            and keeps the pairs whose user it owns; the step exchanges the pairs' scores and
            the item gradient only (rg_mf_owner_*, ``comm`` or ``train_step_owner_exchange``).
            ``batch_size`` is per rank; a step's input is the GLOBAL batch of R*B positives
            with this rank's plan (``make_plans(items, users=...)``)."""
        _lib.require_gpu()
        if loss not in LOSS_KINDS:
            raise ValueError(f"unknown loss {loss!r}")
        if optimizer not in OPT_KINDS:
            raise ValueError(f"unknown optimizer {optimizer!r}")
        if not 1 <= n_neg <= RG_MF_MAX_NEG:
            raise ValueError(f"num_negative_samples must be in [1, {RG_MF_MAX_NEG}] for the fused kernel")
        dp = dp or ("owner" if world_size > 1 or comm is not None else None)
        if dp not in (None, "user_shard", "global_stream", "owner"):
            raise ValueError(f"unknown data-parallel layout {dp!r}")
        if loss == "adaptive_hinge" and dp in ("global_stream", "user_shard"):
            raise NotImplementedError("adaptive_hinge over several ranks runs on the owner-sharded layout (dp='owner')")
        self.U_global = int(user_w.shape[0])
        if dp == "owner":
            user_w = user_w[rank::world_size]
            user_b = torch.as_tensor(user_b).reshape(-1)[rank::world_size]
        self.lib = _lib.load()
        self.device = torch.device(device)
        dev = self.device
        self.U, self.I = int(user_w.shape[0]), int(item_w.shape[0])
        self.dim = int(user_w.shape[1])
        if not 1 <= self.dim <= 256:
            raise ValueError("embedding_dim must be in [1, 256]")
        if self.U + self.I >= 2 ** 31:
            raise ValueError("num_users + num_items must be < 2^31")
        f32 = dict(dtype=torch.float32, device=dev)

        def put(t, shape):
            return torch.as_tensor(t, dtype=torch.float32).reshape(shape).to(dev).contiguous()

        self.rank, self.world = int(rank), int(world_size)
        if dp == "global_stream":
            # row shards of the rank-major exchange; tables allocated with world * shard rows
            self.shard_users = -(-self.U // self.world)
            self.shard_items = -(-self.I // self.world)
            rows = (self.shard_users * self.world, self.shard_items * self.world)
        elif dp == "owner" and comm is not None and self.world > 1 and _lib.ab_build() and \
                os.environ.get("RG_OWNER_ITEM_SHARD", "0") == "1":
            # the owner step's sharded item update (reduce-scatter -> this rank's 1/R of the items'
            # optimizer update -> all-gather): item tables allocated with world * shard rows.  A/B
            # build only: with local-copy exchanges rank 0 of 8 measured 81.0 us against 74.6 for
            # the all-reduce and the full item update
            self.shard_users, self.shard_items = 0, -(-self.I // self.world)
            rows = (self.U, self.shard_items * self.world)
        else:
            self.shard_users = self.shard_items = 0
            rows = (self.U, self.I)

        def padded():
            bufs = [torch.zeros(rows[0], self.dim, **f32), torch.zeros(rows[1], self.dim, **f32),
                    torch.zeros(rows[0], **f32), torch.zeros(rows[1], **f32)]
            return bufs, [bufs[0][:self.U], bufs[1][:self.I], bufs[2][:self.U], bufs[3][:self.I]]

        self._pad, self.tabs = [], []
        for _ in range(2):
            b, v = padded()
            self._pad.append(b)
            self.tabs.append(v)
        for dst, src, shape in zip(self.tabs[0], (user_w, item_w, user_b, item_b),
                                   ((self.U, self.dim), (self.I, self.dim), (self.U,), (self.I,))):
            dst.copy_(put(src, shape))
        self.opt_kind = optimizer
        self.m = padded()[1] if optimizer == "adam" else [None] * 4
        self.v = padded()[1] if optimizer != "sgd" else [None] * 4
        self.lr, self.wd, self.betas, self.eps, self.alpha = lr, weight_decay, betas, eps, alpha
        pu = np.asarray(pool_u, dtype=np.int64)
        pi = np.asarray(pool_i, dtype=np.int64)
        if len(pu) == 0 or len(pu) != len(pi):
            raise ValueError("negative pool must be non-empty with matching user/item arrays")
        if pu.min() < 0 or pu.max() >= (self.U_global if dp == "owner" else self.U) or pi.min() < 0 or \
                pi.max() >= self.I:
            raise ValueError("negative pool contains ids outside the model's tables")
        self.pool = torch.from_numpy(np.stack([pu, pi], 1).astype(np.int32)).to(dev).contiguous()
        self.pool_len = len(pu)
        self.loss = loss
        self.n_neg = int(n_neg)
        self.batch_size = int(batch_size)
        self.dp = dp
        self.comm = comm
        if dp == "global_stream":
            self.col_offset, self.global_cols = self.rank * self.batch_size, self.batch_size * self.world
        elif dp == "owner":
            self.col_offset, self.global_cols = 0, self.batch_size * self.world
        else:
            self.col_offset, self.global_cols = 0, self.batch_size
        self.cols = self.global_cols if dp == "owner" else self.batch_size
        self.neg_cols = self.batch_size * self.world
        self.words_per_step = 2 * self.n_neg * self.global_cols
        self.prefetch = prefetch
        rows = self.U + self.I
        self.row_count = torch.zeros(rows, dtype=torch.int32, device=dev)
        self.row_list = torch.empty(rows * RG_MF_LIST_CAP * 2, dtype=torch.int32, device=dev)
        # overflow accumulators: int64 fixed point (order-independent sums, rg_common.h fix_add)
        self.hot_grad = torch.zeros(rows * self.dim, dtype=torch.int64, device=dev)
        self.hot_bias = torch.zeros(rows, dtype=torch.int64, device=dev)
        if dp == "owner":
            self.n_partials = self.lib.rg_mf_owner_partials_len(self.global_cols, self.n_neg, self.dim,
                                                                self.world) // 2
        else:
            self.n_partials = self.lib.rg_mf_partials_len(self.batch_size, self.dim) // 2
        self.partials = torch.zeros(2 * self.n_partials, **f32)
        self.scores_buf = torch.empty(self.batch_size, **f32) if loss == "adaptive_hinge" else None
        self.max_key = torch.zeros(1, dtype=torch.int64, device=dev) if loss == "adaptive_hinge" else None
        self.active_count = torch.zeros(1, dtype=torch.int32, device=dev) if loss == "adaptive_hinge" else None
        self.loss_out = torch.zeros(1, **f32)
        self.part_row = torch.zeros(self.cols * self.dim, **f32)
        self.part_bias = torch.zeros(self.cols, **f32)
        self.units_per_block = int(self.lib.rg_mf_plan_units_per_block(self.dim))
        self.grad_buf = None
        self.item_grad = None
        if dp in ("user_shard", "owner"):
            n = self.I * (self.dim + 1) + 1
            if self.shard_items and dp == "owner":
                n = self.world * int(self.lib.rg_mf_item_grad_chunk(self.shard_items, self.dim))
            self.item_grad = torch.zeros(n, **f32)
        if dp == "owner":
            rl = int(self.lib.rg_mf_owner_rec_len(self.global_cols, self.n_neg))
            ns = int(self.lib.rg_mf_owner_segments(self.global_cols, self.n_neg))
            self.owner_rec = [torch.zeros(4 * rl, dtype=torch.int32, device=dev) for _ in range(2)]
            self.owner_seg = [torch.zeros(ns, dtype=torch.int32, device=dev) for _ in range(2)]
            # adaptive hinge: 4 extra slots after the exchanged scores (rg_mf_owner_adapt)
            extra = 4 if loss == "adaptive_hinge" else 0
            self.owner_scores = [torch.zeros((1 + self.n_neg) * self.global_cols + extra, **f32) for _ in range(2)]
        self.chunk = 0
        if dp == "global_stream":
            self.chunk = int(self.lib.rg_mf_grad_chunk(self.shard_users, self.shard_items, self.dim))
            self.dp_grad = torch.zeros(self.world * self.chunk, **f32)
        self.mt_buf = _as_u32_tensor(mt_state, dev)
        self.pairs = [torch.zeros(int(self.lib.rg_mf_pairs_len(self.batch_size, self.n_neg)), dtype=torch.int32,
                                  device=dev) for _ in range(2)]
        self._work = _lib.MFWork(ptr(self.row_count), ptr(self.row_list), ptr(self.hot_grad), ptr(self.hot_bias),
                                 ptr(self.partials), ptr(self.scores_buf), ptr(self.max_key),
                                 ptr(self.active_count), None, None, None, ptr(self.part_row),
                                 ptr(self.part_bias))
        self._tables = [self._make_tables(0), self._make_tables(1)]
        cfg = _lib.MFStepperConfig()
        cfg.tables[0], cfg.tables[1] = self._tables[0], self._tables[1]
        cfg.work = self._work
        cfg.mt_state = ptr(self.mt_buf)
        cfg.pairs[0], cfg.pairs[1] = ptr(self.pairs[0]), ptr(self.pairs[1])
        cfg.pool, cfg.pool_len = ptr(self.pool), self.pool_len
        cfg.n_neg, cfg.loss = self.n_neg, LOSS_KINDS[loss]
        cfg.cols, cfg.col_offset, cfg.global_cols = self.cols, self.col_offset, self.global_cols
        cfg.neg_cols = self.neg_cols
        cfg.item_grad = ptr(self.item_grad)
        cfg.comm = comm.handle if comm is not None else None
        cfg.opt = self._opt_base()
        cfg.lr_d, cfg.beta1_d, cfg.beta2_d = float(lr), float(betas[0]), float(betas[1])
        cfg.step, cfg.n_partials, cfg.current_set = 0, self.n_partials, 0
        if dp == "global_stream":
            cfg.dp_mode, cfg.rank, cfg.world = 1, self.rank, self.world
            cfg.shard_users, cfg.shard_items = self.shard_users, self.shard_items
            cfg.grad_buf = ptr(self.dp_grad)
        elif dp == "owner":
            cfg.dp_mode, cfg.rank, cfg.world = 2, self.rank, self.world
            cfg.shard_items = self.shard_items
            for k in range(2):
                cfg.owner_rec[k] = ptr(self.owner_rec[k])
                cfg.owner_seg[k] = ptr(self.owner_seg[k])
                cfg.owner_scores[k] = ptr(self.owner_scores[k])
        self._stepper = self.lib.rg_mf_stepper_create(ctypes.byref(cfg))
        if not self._stepper:
            raise RuntimeError("rg_mf_stepper_create: " + self.lib.rg_last_error().decode())
        self._cfg = cfg   # keep alive

    def __del__(self):
        st = getattr(self, "_stepper", None)
        if st:
            try:
                self.lib.rg_mf_stepper_destroy(st)
            except Exception:
                pass
            self._stepper = None

    # ------------------------------------------------------------------ plumbing
    def _make_tables(self, cur):
        a, b = self.tabs[cur], self.tabs[1 - cur]
        m, v = self.m, self.v
        return _lib.MFTables(ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]),
                             ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]),
                             ptr(m[0]), ptr(v[0]), ptr(m[1]), ptr(v[1]),
                             ptr(m[2]), ptr(v[2]), ptr(m[3]), ptr(v[3]),
                             self.U, self.I, self.dim, 0)

    def _opt_base(self):
        o = _lib.Opt()
        o.kind = OPT_KINDS[self.opt_kind]
        o.lr, o.beta1, o.beta2 = self.lr, self.betas[0], self.betas[1]
        o.eps, o.weight_decay, o.alpha = self.eps, self.wd, self.alpha
        o.one_minus_beta1 = 1 - self.betas[0]
        o.one_minus_beta2 = 1 - self.betas[1]
        o.one_minus_alpha = 1 - self.alpha
        return o

    def _state(self):
        cs = ctypes.c_int32()
        st = ctypes.c_int64()
        check(self.lib.rg_mf_stepper_state(self._stepper, ctypes.byref(cs), ctypes.byref(st)), "stepper_state")
        return cs.value, st.value

    @property
    def cur(self):
        return self._state()[0]

    @property
    def t(self):
        return self._state()[1]

    def flush(self):
        """Lazy split step: bring every deferred user row up to the current step
        (rg_mf_stepper_flush, on the current stream; a no-op when no row lags)."""
        check(self.lib.rg_mf_stepper_flush(self._stepper, _lib.stream_handle()), "rg_mf_stepper_flush")

    def lazy_rows(self, enable=False):
        """Diagnostics of the lazy pass: user rows processed since the last call (synchronises);
        ``enable`` switches the (contended) device counter on for the following steps.
        Returns None when the stepper runs the eager pass."""
        n = ctypes.c_uint64()
        lazy = self.lib.rg_mf_stepper_lazy_count(self._stepper, int(bool(enable)), ctypes.byref(n))
        return int(n.value) if lazy == 1 else None

    def params(self):
        """Current (user_w, item_w, user_b, item_b) device tensors (deferred rows flushed)."""
        self.flush()
        return self.tabs[self.cur]

    def loss_scales(self, global_pos):
        n, gc = self.n_neg, self.neg_cols
        if self.loss == "pointwise":
            return 1.0 / global_pos, 1.0 / (n * gc)
        if self.loss in ("bpr", "hinge"):
            return 1.0 / (n * global_pos), 0.0
        return 1.0 / global_pos, 0.0

    def make_plan(self, pos_i):
        return build_plan(pos_i, self.batch_size, self.units_per_block, self.I)

    def make_plans(self, items, offset=0, stride=None, users=None):
        """Plans of every batch [offset + k*stride, +batch_size) of ``items`` in one launch;
        owner layout: of every GLOBAL batch [k*R*B, (k+1)*R*B), this rank's positives
        (``users`` required)."""
        if self.dp == "owner":
            if users is None:
                raise ValueError("the owner-sharded layout plans this rank's positives: pass users=")
            return build_plans(items, self.global_cols, self.units_per_block, self.I, offset=offset,
                               stride=stride or self.global_cols, users=users, world=self.world, rank=self.rank,
                               cols=self.global_cols)
        return build_plans(items, self.batch_size, self.units_per_block, self.I, offset=offset, stride=stride)

    def _loss(self, global_pos, out):
        ia, ib = self.loss_scales(global_pos)
        return _lib.MFLoss(self.n_partials, ia, ib, ptr(out))

    def _check_ids(self, pos_u, pos_i):
        for t in (pos_u, pos_i):
            if t.dtype != torch.int64 or t.device != self.device or not t.is_contiguous():
                raise ValueError("positive ids must be contiguous int64 tensors on the engine's device")
        if pos_u.numel() != pos_i.numel() or pos_u.numel() > self.cols:
            raise ValueError("positive id batch larger than batch_size (owner layout: world * batch_size) "
                             "or mismatched")

    def step_input(self, pos_u, pos_i, global_pos=None, plan=None):
        self._check_ids(pos_u, pos_i)
        n_pos = int(pos_u.numel())
        if self.dp == "owner":
            if plan is None or plan.n_planned is None:
                raise ValueError("the owner-sharded step needs this rank's plan of the global batch (make_plans)")
            global_pos = n_pos
        global_pos = n_pos * self.world if global_pos is None else int(global_pos)
        x = _lib.MFStepIn(ptr(pos_u) if n_pos else None, ptr(pos_i) if n_pos else None, n_pos, global_pos,
                          None, None, None, 0)
        if plan is not None:
            x.plan_perm, x.plan_pos_slot, x.plan_item_slot_off = ptr(plan.perm), ptr(plan.pos_slot), \
                ptr(plan.item_slot_off)
            x.n_planned = plan.n_planned or 0
        x._keep = (pos_u, pos_i, plan)
        return x

    # ------------------------------------------------------------------ step
    def train_step(self, pos_u, pos_i, global_pos=None, plan=None, apply_events=None, next_input=None):
        """One training step on this rank's positives; returns the device loss tensor (1,).
        ``plan``: optional MFPlan for this batch (see build_plan).  ``next_input``: the
        following step's ``step_input(...)`` -- its words and pairs are then produced
        ahead on the side stream.  ``apply_events``: optional (start, end) torch.cuda.Event
        pair recorded around the rg_mf_apply launch (kernel timing for the roofline)."""
        cur = self.step_input(pos_u, pos_i, global_pos, plan)
        return self.train_step_in(cur, next_input if self.prefetch else None, apply_events)

    def train_step_in(self, cur, next_input=None, apply_events=None, loss_out=None, next2=None):
        """One native step for a prebuilt ``step_input``; the loss goes to ``loss_out``
        (a float32 device tensor of >= 1 element) or to the engine's own slot.  ``next_input`` /
        ``next2``: the following steps' inputs (the pipelined single-GPU step runs the next
        step's pair pass and the one after's prepare inside this step's launch)."""
        if self.dp == "user_shard" and self.world > 1 and self.comm is None:
            raise RuntimeError("user-sharded step over several ranks needs an RcclComm (or train_step_sharded)")
        if self.dp == "global_stream" and self.comm is None:
            if self.world > 1:
                raise RuntimeError("dp='global_stream' over several ranks needs an RcclComm (or train_step_exchange)")
            return self.train_step_exchange(cur, next_input, lambda buf, chunk: None, lambda bufs, counts: None,
                                            loss_out=loss_out)
        if self.dp == "owner" and self.comm is None:
            if self.world > 1:
                raise RuntimeError("dp='owner' over several ranks needs an RcclComm (or train_step_owner_exchange)")
            return self.train_step_owner_exchange(cur, next_input, lambda buf: None, loss_out=loss_out,
                                                  apply_events=apply_events)
        ev0 = ev1 = None
        if apply_events is not None:
            ev0, ev1 = (ctypes.c_void_p(e.cuda_event) for e in apply_events)
        out = self.loss_out if loss_out is None else loss_out
        if out.dtype != torch.float32 or out.device != self.device:
            raise ValueError("loss_out must be a float32 tensor on the engine's device")
        if next2 is not None and next_input is not None:
            check(self.lib.rg_mf_stepper_train_ahead(self._stepper, _lib.stream_handle(), ctypes.byref(cur),
                                                     ctypes.byref(next_input), ctypes.byref(next2), ptr(out), ev0,
                                                     ev1), "rg_mf_stepper_train_ahead")
            return out
        check(self.lib.rg_mf_stepper_train(self._stepper, _lib.stream_handle(), ctypes.byref(cur),
                                           ctypes.byref(next_input) if next_input is not None else None,
                                           ptr(out), ev0, ev1), "rg_mf_stepper_train")
        return out

    @property
    def pipelined(self):
        """True if the native step is the single-launch pipelined one (rg_mf_pipe_step, A/B build)."""
        return self.lib.rg_mf_stepper_pipelined(self._stepper) == 1

    @property
    def mt_mode(self):
        """0: one MT walk of every word; 1: jump-ahead segments of the global draw; 2: this rank's
        slice of each step's draw, all-gathered (the owner step over a communicator)."""
        return int(self.lib.rg_mf_stepper_mt_mode(self._stepper))

    @property
    def pipeline_kind(self):
        """0: the split step; 1: the single-launch pipelined step (A/B build); 2: the two-launch
        pipelined step (rg_mf_pipe2_hot / rg_mf_pipe2_cold, opt-in: RG_PIPE2=1)."""
        return int(self.lib.rg_mf_stepper_pipelined(self._stepper))

    def pipe_error(self):
        """True if a pipelined launch's pair workgroups ran out of their bounded wait (then its
        results are wrong; synchronises)."""
        e = ctypes.c_int32(0)
        check(self.lib.rg_mf_stepper_pipe_error(self._stepper, ctypes.byref(e)), "rg_mf_stepper_pipe_error")
        return bool(e.value)

    def _acquire(self, cur):
        batch, work = _lib.MFBatch(), _lib.MFWork()
        check(self.lib.rg_mf_stepper_acquire(self._stepper, _lib.stream_handle(), ctypes.byref(cur),
                                             ctypes.byref(batch), ctypes.byref(work)), "rg_mf_stepper_acquire")
        return batch, work

    def _release(self):
        check(self.lib.rg_mf_stepper_release(self._stepper, _lib.stream_handle()), "rg_mf_stepper_release")

    def _flat_grad(self, nrows):
        n = nrows * (self.dim + 1) + 1
        if self.grad_buf is None or self.grad_buf.numel() < n:
            self.grad_buf = torch.zeros(n, dtype=torch.float32, device=self.device)
        return self.grad_buf[:n]

    def pairs_and_lists(self, pos_u, pos_i, global_pos=None, plan=None):
        """rg_mf_pairs with backward on this step's draw; the lists are then consumed by
        ``grads`` / ``apply_rows``."""
        cur = self.step_input(pos_u, pos_i, global_pos, plan)
        batch, work = self._acquire(cur)
        check(self.lib.rg_mf_pairs(_lib.stream_handle(), self._tables[self.cur], ctypes.byref(batch),
                                   ctypes.byref(work), 1), "rg_mf_pairs")
        self._release()
        self._work_step = work
        self._global_pos = cur.global_pos
        return cur

    def grads(self, pos_u, pos_i, global_pos=None, plan=None, row_begin=0, row_end=-1):
        """pairs + gradient pull of rows [row_begin, row_end) into the flat buffer
        [n*d | n | loss]; no update.  Returns the (device) flat buffer."""
        self.pairs_and_lists(pos_u, pos_i, global_pos, plan)
        return self.pull_grads(row_begin, row_end)

    def pull_grads(self, row_begin=0, row_end=-1):
        re = self.U + self.I if row_end < 0 else row_end
        g = self._flat_grad(re - row_begin)
        check(self.lib.rg_mf_grads(_lib.stream_handle(), self._tables[self.cur], ctypes.byref(self._work_step),
                                   ptr(g), row_begin, re, self._loss(self._global_pos, self.loss_out)),
              "rg_mf_grads")
        return g

    def _opt_step(self, t):
        o = _lib.Opt()
        check(self.lib.rg_mf_stepper_opt(self._stepper, t, ctypes.byref(o)), "rg_mf_stepper_opt")
        return o

    def apply_rows(self, row_begin, row_end, loss=True):
        """Pull + optimizer update of rows [row_begin, row_end) from the current lists
        (does not flip the table sets; see ``finish_step``)."""
        o = self._opt_step(self.t + 1)
        check(self.lib.rg_mf_apply(_lib.stream_handle(), self._tables[self.cur], ctypes.byref(self._work_step),
                                   ctypes.byref(o), row_begin, row_end,
                                   self._loss(self._global_pos, self.loss_out) if loss else None), "rg_mf_apply")

    def apply_dense_rows(self, grad, row_begin, row_end):
        o = self._opt_step(self.t + 1)
        check(self.lib.rg_mf_apply_dense(_lib.stream_handle(), self._tables[self.cur], ptr(grad), ctypes.byref(o),
                                         row_begin, row_end, ptr(self.loss_out)), "rg_mf_apply_dense")

    def finish_step(self):
        """After a split step updated every row: flip the ping-pong sets, count the step."""
        check(self.lib.rg_mf_stepper_advance(self._stepper, 1, 1), "rg_mf_stepper_advance")

    def apply_dense(self, grad):
        """Optimizer update of every row from a (summed) flat gradient buffer."""
        self.apply_dense_rows(grad, 0, self.U + self.I)
        self.finish_step()
        return self.loss_out

    # ------------------------------------------------------------------ replicated DP (global_stream)
    def dp_begin(self, cur, next_input=None, loss_out=None):
        """First half of the replicated step (rg_mf_stepper_dp_begin): this rank's column
        slice of the global draw -> pairs -> the rank-major gradient in ``dp_grad``."""
        out = self.loss_out if loss_out is None else loss_out
        check(self.lib.rg_mf_stepper_dp_begin(self._stepper, _lib.stream_handle(), ctypes.byref(cur),
                                              ctypes.byref(next_input) if next_input is not None else None,
                                              ptr(out)), "rg_mf_stepper_dp_begin")
        return out

    def dp_end(self, loss_out=None):
        """Second half: this rank's rows from its (reduce-scattered) chunk, then the sets
        flip; the caller all-gathers ``dp_gather_buffers()``."""
        out = self.loss_out if loss_out is None else loss_out
        check(self.lib.rg_mf_stepper_dp_end(self._stepper, _lib.stream_handle(), ptr(out)), "rg_mf_stepper_dp_end")
        return out

    def dp_gather_buffers(self):
        """The current set's four padded tables and this layout's all-gather counts (each
        rank's shard = rows [rank * count, (rank + 1) * count) of the flat buffer)."""
        d = self.dim
        return self._pad[self.cur], [self.shard_users * d, self.shard_items * d, self.shard_users, self.shard_items]

    def train_step_exchange(self, cur, next_input, reduce_scatter, all_gather, loss_out=None):
        """The replicated step with caller-run collectives: ``reduce_scatter(buf, chunk)``
        must leave in buf[rank*chunk:(rank+1)*chunk] the sum over ranks of that chunk;
        ``all_gather(bufs, counts)`` must fill every rank's shard of each buffer."""
        out = self.dp_begin(cur, next_input, loss_out)
        reduce_scatter(self.dp_grad, self.chunk)
        self.dp_end(out)
        all_gather(*self.dp_gather_buffers())
        return out

    # ------------------------------------------------------------------ owner-sharded DP
    def train_step_owner_exchange(self, cur, next_input, allreduce, loss_out=None, apply_events=None):
        """The owner-sharded step with caller-run exchanges: ``allreduce(buf)`` must sum
        ``buf`` over the ranks in place (the score vector, then the item gradient) -- what
        rg_mf_stepper_train does natively over RCCL."""
        out = self.loss_out if loss_out is None else loss_out
        st = _lib.stream_handle()
        check(self.lib.rg_mf_stepper_owner_begin(self._stepper, st, ctypes.byref(cur)), "rg_mf_stepper_owner_begin")
        if self.loss != "pointwise":
            allreduce(self.current_scores())
        check(self.lib.rg_mf_stepper_owner_mid(self._stepper, st, ptr(out)), "rg_mf_stepper_owner_mid")
        allreduce(self.item_grad)
        ev0 = ev1 = None
        if apply_events is not None:
            ev0, ev1 = (ctypes.c_void_p(e.cuda_event) for e in apply_events)
        check(self.lib.rg_mf_stepper_owner_end(self._stepper, st, ctypes.byref(next_input)
                                               if next_input is not None else None, ptr(out), ev0, ev1),
              "rg_mf_stepper_owner_end")
        return out

    def current_scores(self):
        """The score vector of the owner step in flight ((1 + n) * R * B floats)."""
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        check(self.lib.rg_mf_stepper_owner_scores(self._stepper, ctypes.byref(p), ctypes.byref(n)),
              "rg_mf_stepper_owner_scores")
        for t in self.owner_scores:
            if t.data_ptr() == p.value:
                return t[:n.value]
        raise RuntimeError("owner score buffer not found")

    def train_step_sharded(self, pos_u, pos_i, global_pos, allreduce, plan=None):
        """The user-sharded step with the item-gradient exchange done by ``allreduce``
        (in-place sum, e.g. torch.distributed over gloo in tests): what
        rg_mf_stepper_train does natively with an RCCL communicator."""
        if self.dp != "user_shard":
            raise RuntimeError("train_step_sharded needs dp='user_shard'")
        self.pairs_and_lists(pos_u, pos_i, global_pos, plan)
        g = self.pull_grads(self.U, self.U + self.I)
        allreduce(g)
        self.apply_rows(0, self.U, loss=False)
        self.apply_dense_rows(g, self.U, self.U + self.I)
        self.finish_step()
        return self.loss_out

    def val_loss(self, pos_u, pos_i, global_pos=None, plan=None, allreduce=None):
        """run_val_iteration (implicit.py:366): forward + loss on the same draw stream, no update.
        Owner layout: (pos_u, pos_i) is the GLOBAL validation batch and ``plan`` this rank's
        plan of it; the scores are exchanged by the communicator or ``allreduce``."""
        if self.dp == "owner":
            cur = self.step_input(pos_u, pos_i, None, plan)
            out = torch.empty(1, dtype=torch.float32, device=self.device)
            st = _lib.stream_handle()
            if self.comm is not None:
                check(self.lib.rg_mf_stepper_owner_val(self._stepper, st, ctypes.byref(cur), ptr(out)),
                      "rg_mf_stepper_owner_val")
            else:
                if allreduce is None and self.world > 1:
                    raise RuntimeError("owner-layout validation over several ranks needs a communicator or allreduce")
                check(self.lib.rg_mf_stepper_owner_begin(self._stepper, st, ctypes.byref(cur)),
                      "rg_mf_stepper_owner_begin")
                if allreduce is not None:
                    allreduce(self.current_scores())
                check(self.lib.rg_mf_stepper_owner_val_end(self._stepper, st, ptr(out)), "rg_mf_stepper_owner_val_end")
            return out
        cur = self.step_input(pos_u, pos_i, global_pos, None)
        batch, work = self._acquire(cur)
        stream = _lib.stream_handle()
        check(self.lib.rg_mf_pairs(stream, self._tables[self.cur], ctypes.byref(batch), ctypes.byref(work), 0),
              "rg_mf_pairs")
        self._release()
        ia, ib = self.loss_scales(cur.global_pos)
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        check(self.lib.rg_loss_finalize(stream, ptr(self.partials), self.n_partials, ia, ib, ptr(out)),
              "rg_loss_finalize")
        return out

    def scores(self, users, items):
        """BilinearNet.forward (representations.py:62-91) for eval/predict."""
        users = users.to(self.device, torch.int64).contiguous()
        items = items.to(self.device, torch.int64).contiguous()
        out = torch.empty(users.numel(), dtype=torch.float32, device=self.device)
        U, I, ub, ib = self.params()      # flushes deferred rows
        check(self.lib.rg_mf_scores(_lib.stream_handle(), ptr(U), ptr(I), ptr(ub), ptr(ib), self.dim,
                                    ptr(users), ptr(items), users.numel(), ptr(out)), "rg_mf_scores")
        return out

    def set_params(self, user_w, item_w, user_b, item_b):
        """Overwrite the current tables (teacher forcing in tests, checkpoint load)."""
        for dst, src in zip(self.params(), (user_w, item_w, user_b, item_b)):
            dst.copy_(torch.as_tensor(src, dtype=torch.float32).reshape(dst.shape))

    def mt_state(self):
        """CPython random state (624 words + position) after the last consumed draw."""
        host = np.zeros(625, dtype=np.uint32)
        check(self.lib.rg_mf_stepper_sync_mt(self._stepper, host.ctypes.data_as(ctypes.c_void_p), 0),
              "rg_mf_stepper_sync_mt")
        return host

    def set_mt_state(self, st):
        host = np.ascontiguousarray(np.asarray(st, dtype=np.uint32))
        check(self.lib.rg_mf_stepper_sync_mt(self._stepper, host.ctypes.data_as(ctypes.c_void_p), 1),
              "rg_mf_stepper_sync_mt")

    def optimizer_state(self):
        if self.dp == "owner" and self.shard_items:
            # each rank updates (and holds current moments for) only its shard of the item rows;
            # the other rows' m / v are stale, so a checkpoint from them would be wrong
            raise NotImplementedError("optimizer_state: the sharded item update (RG_OWNER_ITEM_SHARD, A/B build) "
                                      "keeps each rank's item moments only for its own shard")
        self.flush()
        return {"step": self.t, "m": self.m, "v": self.v}
