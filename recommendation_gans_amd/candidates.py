"""Candidate lists on the device: score a ragged list of items per user, then rank inside each list.

The lists are a CSR over the call's rows -- list r is ``idx[ptr[r]:ptr[r + 1]]`` (``ptr`` int64
``[n + 1]`` ascending from 0 to ``len(idx)``, ``idx`` int32 item ids, repeats allowed, any length) --
and everything here takes and returns tensors on one CUDA device:

* ``score_lists``   MF scores of every entry (rg_mf_score_lists: the user's row stays in registers
  while its list is walked), ``score_lists_torch`` the chain of torch ops a user would write;
* ``seg_topk``      the positions within each list of its k best entries (rg_seg_topk);
* ``seg_rank``      how many entries of each list rank ahead of its first one (rg_seg_rank).

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
