"""Candidate lists on the device: score a ragged list of items per user, then rank inside each list.

The lists are a CSR over the call's rows -- list r is ``idx[ptr[r]:ptr[r + 1]]`` (``ptr`` int64
``[n + 1]`` ascending from 0 to ``len(idx)``, ``idx`` int32 item ids, repeats allowed, any length) --
and everything here takes and returns tensors on one CUDA device:

* ``score_lists``   MF scores of every entry (rg_mf_score_lists: the user's row stays in registers
  while its list is walked), ``score_lists_torch`` the chain of torch ops a user would write;
* ``seg_topk``      the positions within each list of its k best entries (rg_seg_topk);
* ``seg_rank``      how many entries of each list rank ahead of its first one (rg_seg_rank);
* ``seg_mmr``       k entries of each list picked greedily by relevance less similarity to the picks
  so far (maximal marginal relevance, rg_seg_mmr), ``seg_mmr_torch`` the chain of torch ops;
* ``seg_mean_sim``  the mean pairwise similarity of each list's entries (rg_seg_mean_sim).

The order is the library's everywhere: key descending (the key of a NaN is -inf, -0.0 and +0.0 are
one key), then the lower item id, then the lower position.  ``ImplicitFactorizationModel.
score_candidates`` / ``rank_candidates`` and ``spotlight.evaluation.sampled_hit_ndcg`` are built on
these.  Arguments of another dtype, shape or device, or non-contiguous ones, raise ValueError before
any launch: there is no conversion and no fall-back here.
"""
import torch

from . import _lib
from ._lib import check, ptr as _ptr

SEG_TOPK_MAX = 32       # rg_seg_topk's largest k (the register lists of rg_topk_lists.h)
SEG_MMR_MAX = 32        # rg_seg_mmr's largest k (RG_SEG_MMR_MAX_K: lane t keeps step t's result)
SEG_MMR_MAX_LEN = 1024  # the longest list of rg_seg_mmr / rg_seg_mean_sim (RG_SEG_MMR_MAX_LEN: 16 entries per lane)


def _flat(t, dtype, what, dev=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 1 and t.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous 1-D {str(dtype).replace('torch.', '')} tensor on a CUDA device")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what} is on {t.device}, the other arguments on {dev}")
    return t


def _lists(ptr, idx, dev, what):
    """The CSR's own checks: returns (n, nnz)."""
    _flat(ptr, torch.int64, f"{what}: ptr", dev)
    _flat(idx, torch.int32, f"{what}: idx", dev)
    if ptr.numel() < 1:
        raise ValueError(f"{what}: ptr must have n + 1 entries")
    return int(ptr.numel()) - 1, int(idx.numel())


def _ptr_bad(ptr, nnz):
    """A device bool: ptr does not ascend from 0 to nnz, or a list is longer than 2^31 - 1."""
    d = ptr[1:] - ptr[:-1]
    return (ptr[0] != 0) | (ptr[-1] != nnz) | (d < 0).any() | (d > 2 ** 31 - 1).any()


def _check_ptr(ptr, nnz, what):
    if bool(_ptr_bad(ptr, nnz)):
        raise ValueError(f"{what}: ptr must ascend from 0 to len(idx)")


def score_lists_torch(U, I, ub, ib, users, ptr, idx):
    """``score_lists`` as the chain of torch ops a user would write -- gather the rows of every entry,
    ``einsum``, two adds, ``sigmoid`` -- on tensors of any device and float dtype: the timing baseline
    of ``score_lists`` and, on float64 CPU copies, the tests' reference."""
    rows = torch.repeat_interleave(torch.arange(users.numel(), device=ptr.device), ptr[1:] - ptr[:-1])
    u, i = users.reshape(-1)[rows].long(), idx.long()
    dot = torch.einsum("ek,ek->e", U[u], I[i])
    return torch.sigmoid((dot + ub.reshape(-1)[u]) + ib.reshape(-1)[i])


def score_lists(U, I, ub, ib, users, ptr, idx, checked=False):
    """MF scores of a ragged list of items per user, float32 ``[len(idx)]`` in list order on the tables'
    device: entry e of list r is ``sigmoid((<U[users[r]], I[idx[e]]> + ub[users[r]]) + ib[idx[e]])``, one
    launch (rg_mf_score_lists).  A (user, item) pair gives the same bits at any position of any list.
    The tables (contiguous float32 on one CUDA device, dim <= 256) are only read; ``users`` is int64
    ``[n]``.  ValueError, before any launch, for arguments of another dtype, shape or device or
    non-contiguous ones, a ``ptr`` that does not ascend from 0 to ``len(idx)``, and an id outside its
    table (one download of the bounds; ``checked=True``: the caller has checked ptr and ids already)."""
    what = "score_lists"
    tabs = (U, I, ub, ib)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and
               t.device == U.device for t in tabs):
        raise ValueError(f"{what} needs contiguous float32 tables on one CUDA device")
    if not (U.dim() == 2 and I.dim() == 2 and 1 <= U.shape[1] <= 256 and I.shape[1] == U.shape[1] and
            ub.numel() == U.shape[0] and ib.numel() == I.shape[0]):
        raise ValueError(f"{what}: tables must be (users, dim) and (items, dim) with 1 <= dim <= 256 and one bias "
                         "per row")
    dev = U.device
    _flat(users, torch.int64, f"{what}: users", dev)
    n, nnz = _lists(ptr, idx, dev, what)
    if users.numel() != n:
        raise ValueError(f"{what}: {users.numel()} users for {n} lists")
    out = torch.empty(nnz, dtype=torch.float32, device=dev)
    if not checked:
        bad = [_ptr_bad(ptr, nnz)]
        if n:
            bad += [users.min() < 0, users.max() >= U.shape[0]]
        if nnz:
            bad += [idx.min() < 0, idx.max() >= I.shape[0]]
        bad = torch.stack(bad).tolist()
        if bad[0]:
            raise ValueError(f"{what}: ptr must ascend from 0 to len(idx)")
        if n and (bad[1] or bad[2]):
            raise ValueError(f"{what}: user ids outside the user table")
        if nnz and (bad[-2] or bad[-1]):
            raise ValueError(f"{what}: item ids outside the item table")
    if n == 0 or nnz == 0:
        return out
    with torch.cuda.device(dev):
        check(_lib.load().rg_mf_score_lists(_lib.stream_handle(), _ptr(U), _ptr(I), _ptr(ub), _ptr(ib),
                                            int(U.shape[1]), _ptr(users), _ptr(ptr), _ptr(idx), n, _ptr(out)),
              "rg_mf_score_lists")
    return out


def _seg_args(scores, ptr, idx, what, checked=False):
    _flat(scores, torch.float32, f"{what}: scores")
    dev = scores.device
    n, nnz = _lists(ptr, idx, dev, what)
    if scores.numel() != nnz:
        raise ValueError(f"{what}: {scores.numel()} scores for {nnz} entries")
    if not checked:
        _check_ptr(ptr, nnz, what)
    return dev, n, nnz


def seg_topk(scores, ptr, idx, k, return_values=False, checked=False):
    """The positions WITHIN each list of its k best entries, int32 ``[n, k]`` on the device
    (rg_seg_topk): ``scores`` (float32 ``[len(idx)]``) in list order, ranked by key descending, then
    item id ascending, then position ascending (a repeated id appears as often as it is listed); a
    list shorter than k fills the rest of its row with -1.  ``return_values``: also the float32 values
    at those positions (-inf in the fill).  ValueError for k outside [1, 32], arguments of another
    dtype, shape or device, or a ``ptr`` that does not ascend from 0 to ``len(idx)`` (one download;
    ``checked=True``: the caller has checked ptr already)."""
    what = "seg_topk"
    if int(k) != k or k < 1 or k > SEG_TOPK_MAX:
        raise ValueError(f"{what}: k must be in [1, {SEG_TOPK_MAX}]")
    k = int(k)
    dev, n, nnz = _seg_args(scores, ptr, idx, what, checked)
    if nnz == 0:                                    # every list is empty: nothing to pass, nothing to launch
        pos = torch.full((n, k), -1, dtype=torch.int32, device=dev)
        return (pos, torch.full((n, k), float("-inf"), dtype=torch.float32, device=dev)) if return_values else pos
    pos = torch.empty(n, k, dtype=torch.int32, device=dev)
    val = torch.empty(n, k, dtype=torch.float32, device=dev) if return_values else None
    with torch.cuda.device(dev):
        check(_lib.load().rg_seg_topk(_lib.stream_handle(), _ptr(scores), _ptr(ptr), _ptr(idx), n, k, _ptr(pos),
                                      _ptr(val)), "rg_seg_topk")
    return (pos, val) if return_values else pos


def seg_rank(scores, ptr, idx, checked=False):
    """Where entry 0 of each list (the target) stands in its list, int32 ``[n, 2]`` on the device
    (rg_seg_rank): column 0 the other entries with a strictly higher key, column 1 those with an
    equal key and a lower item id -- their sum is the number of entries ``seg_topk`` places before
    the target.  An empty list gives (-1, -1).  ValueError as ``seg_topk``."""
    what = "seg_rank"
    dev, n, nnz = _seg_args(scores, ptr, idx, what, checked)
    if nnz == 0:
        return torch.full((n, 2), -1, dtype=torch.int32, device=dev)
    out = torch.empty(n, 2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().rg_seg_rank(_lib.stream_handle(), _ptr(scores), _ptr(ptr), _ptr(idx), n, _ptr(out)),
              "rg_seg_rank")
    return out


# ---------------------------------------------------------------- diversified re-ranking (rg_diverse.hip)
def _sim_args(table, rnorm, dev, what):
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.float32 and table.dim() == 2 and
            table.is_contiguous() and 1 <= table.shape[1] <= 256):
        raise ValueError(f"{what}: table must be a contiguous float32 (rows, dim) tensor on a CUDA device, "
                         "1 <= dim <= 256")
    if table.device != dev:
        raise ValueError(f"{what}: table is on {table.device}, the other arguments on {dev}")
    if rnorm is not None:
        _flat(rnorm, torch.float32, f"{what}: rnorm", dev)
        if rnorm.numel() != table.shape[0]:
            raise ValueError(f"{what}: {rnorm.numel()} reciprocal norms for {table.shape[0]} rows")


def _check_sim_lists(ptr, idx, nnz, rows, what, negative_ok):
    """ptr, the cap on a list's length and the ids against the table, in one download."""
    bad = [_ptr_bad(ptr, nnz), (ptr[1:] - ptr[:-1] > SEG_MMR_MAX_LEN).any()]
    if nnz:
        bad += [idx.max() >= rows, idx.min() < 0]
    bad = torch.stack(bad).tolist()
    if bad[0]:
        raise ValueError(f"{what}: ptr must ascend from 0 to len(idx)")
    if bad[1]:
        raise ValueError(f"{what}: a list is longer than {SEG_MMR_MAX_LEN} entries")
    if nnz and (bad[2] or (bad[3] and not negative_ok)):
        raise ValueError(f"{what}: ids outside the table")


def _mmr_k_lam(k, lam, what):
    if int(k) != k or k < 1 or k > SEG_MMR_MAX:
        raise ValueError(f"{what}: k must be in [1, {SEG_MMR_MAX}]")
    lam = float(lam)
    if not 0.0 < lam <= 1.0:                         # a NaN fails both comparisons
        raise ValueError(f"{what}: lam must be in (0, 1]")
    return int(k), lam


def seg_mmr_torch(scores, ptr, idx, table, k, lam, rnorm=None, return_values=False, return_penalties=False):
    """``seg_mmr`` as the chain of torch ops a user would write, on tensors of any device and float
    dtype: the lists padded to the longest, their rows gathered into one (n, L, dim) block, then k
    rounds of objective, selection, one batched product against the selected rows and ``maximum``
    into the penalties.  The selection is lexicographic and explicit -- the best objective, among
    those the lowest id, among those the lowest position -- not ``argmax``, whose tie rule is not the
    library's.  The timing baseline of ``seg_mmr`` and, on float64 CPU copies, the tests' reference
    (``lam`` is used as given: pass the float32 value the kernel sees)."""
    k, lam = _mmr_k_lam(k, lam, "seg_mmr_torch")
    dev, ft = scores.device, scores.dtype
    n, nnz = int(ptr.numel()) - 1, int(idx.numel())
    pos = torch.full((n, k), -1, dtype=torch.int32, device=dev)
    val = torch.full((n, k), float("-inf"), dtype=ft, device=dev)
    pens = torch.zeros(n, k, dtype=ft, device=dev)

    def result():
        return (pos,) + ((val,) if return_values else ()) + ((pens,) if return_penalties else ()) \
            if return_values or return_penalties else pos
    lens = ptr[1:] - ptr[:-1]
    L = int(lens.max()) if n and nnz else 0
    if L == 0:
        return result()
    ar = torch.arange(L, device=dev)
    valid = ar[None, :] < lens[:, None]
    at = (ptr[:-1, None] + ar[None, :]).clamp(max=nnz - 1)
    ids = torch.where(valid, idx[at].long(), 0)
    raw = scores[at]
    ninf = torch.full_like(raw, float("-inf"))
    key = torch.where(valid & ~torch.isnan(raw), raw, ninf) + 0.0      # NaN -> -inf; -0.0 + 0.0 = +0.0
    rows = table[ids]                                                   # (n, L, dim)
    rn = rnorm[ids] if rnorm is not None else None
    pen = ninf.clone()
    left = valid.clone()
    every = torch.arange(n, device=dev)
    for t in range(k):
        obj = key if t == 0 else torch.where(torch.isinf(key), key, lam * key - (1.0 - lam) * pen)
        best = torch.where(left, obj, ninf).max(dim=1).values
        m = left & (obj == best[:, None])
        low = torch.where(m, ids, torch.iinfo(torch.int64).max).min(dim=1).values
        m &= ids == low[:, None]
        p = torch.where(m, ar[None, :], L).min(dim=1).values
        has = p < L
        pc = p.clamp(max=L - 1)
        pos[:, t] = torch.where(has, p, -1).to(torch.int32)
        val[:, t] = torch.where(has, raw[every, pc], ninf[:, 0])
        if t:
            pens[:, t] = torch.where(has, pen[every, pc], torch.zeros_like(best))
        left &= ar[None, :] != p[:, None]
        if t + 1 < k:
            sim = torch.einsum("nld,nd->nl", rows, rows[every, pc])
            if rn is not None:
                sim = (sim * rn) * rn[every, pc][:, None]
            pen = torch.maximum(pen, sim)
    return result()


def seg_mmr(scores, ptr, idx, table, k, lam, rnorm=None, return_values=False, return_penalties=False, checked=False):
    """Maximal marginal relevance inside each list, one launch (rg_seg_mmr): the positions WITHIN each
    list of k entries picked greedily, int32 ``[n, k]`` on the device, -1 past a short list's end.
    Step 0 takes the list's best entry as ``seg_topk`` does; every later step takes the best
    unselected entry by ``lam * key - (1 - lam) * pen`` (an entry whose key is +-inf keeps its key),
    then the lower id, then the lower position, where ``pen`` is the largest similarity to an entry
    already picked: ``(<table[a], table[b]> * rnorm[a]) * rnorm[b]`` with the reciprocal norms of
    ``mf_engine.row_rnorms`` (cosine), or the inner product itself when ``rnorm`` is None.  ``lam=1``
    is ``seg_topk``.  ``return_values``: also the float32 scores at those positions (-inf in the
    fill); ``return_penalties``: also ``pen`` at the time of each pick (0 at step 0 and in the fill).
    ValueError, before any launch, for k outside [1, 32], lam outside (0, 1], arguments of another
    dtype, shape or device or non-contiguous ones, a ``ptr`` that does not ascend from 0 to
    ``len(idx)``, a list longer than 1024 entries, and an id outside the table (one download;
    ``checked=True``: the caller has checked these already)."""
    what = "seg_mmr"
    k, lam = _mmr_k_lam(k, lam, what)
    dev, n, nnz = _seg_args(scores, ptr, idx, what, checked=True)
    _sim_args(table, rnorm, dev, what)
    if not checked:
        _check_sim_lists(ptr, idx, nnz, table.shape[0], what, negative_ok=False)
    if nnz == 0:
        pos = torch.full((n, k), -1, dtype=torch.int32, device=dev)
        val = torch.full((n, k), float("-inf"), dtype=torch.float32, device=dev) if return_values else None
        pen = torch.zeros(n, k, dtype=torch.float32, device=dev) if return_penalties else None
    else:
        pos = torch.empty(n, k, dtype=torch.int32, device=dev)
        val = torch.empty(n, k, dtype=torch.float32, device=dev) if return_values else None
        pen = torch.empty(n, k, dtype=torch.float32, device=dev) if return_penalties else None
        with torch.cuda.device(dev):
            check(_lib.load().rg_seg_mmr(_lib.stream_handle(), _ptr(scores), _ptr(ptr), _ptr(idx), n, _ptr(table),
                                         _ptr(rnorm), int(table.shape[1]), lam, k, _ptr(pos), _ptr(val), _ptr(pen)),
                  "rg_seg_mmr")
    out = (pos,) + ((val,) if return_values else ()) + ((pen,) if return_penalties else ())
    return out if len(out) > 1 else pos


def seg_mean_sim(ptr, idx, table, rnorm=None, checked=False):
    """The mean similarity over the unordered pairs of each list's entries -- the intra-list
    similarity -- float32 ``[n]`` on the device, one launch (rg_seg_mean_sim), with ``seg_mmr``'s
    similarity.  Entries with a negative id are skipped (``rank_candidates``' -1 fill); a list with
    fewer than two entries left gives 0; an id listed twice is two entries.  ValueError as
    ``seg_mmr`` (an id at or beyond the table's rows is refused, a negative one is not)."""
    what = "seg_mean_sim"
    if not torch.is_tensor(ptr) or not ptr.is_cuda:
        raise ValueError(f"{what}: ptr must be a contiguous 1-D int64 tensor on a CUDA device")
    dev = ptr.device
    n, nnz = _lists(ptr, idx, dev, what)
    _sim_args(table, rnorm, dev, what)
    if not checked:
        _check_sim_lists(ptr, idx, nnz, table.shape[0], what, negative_ok=True)
    if nnz == 0:
        return torch.zeros(n, dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().rg_seg_mean_sim(_lib.stream_handle(), _ptr(ptr), _ptr(idx), n, _ptr(table), _ptr(rnorm),
                                          int(table.shape[1]), _ptr(out)), "rg_seg_mean_sim")
    return out
