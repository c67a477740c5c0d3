"""Ranking metrics of spotlight/evaluation.py (reference :13-353).

Same definitions as the reference: per test user with at least one test item,
rank all items by -score (``argsort``), precision/recall@k over the top k,
average precision@k, hit ratio; popularity and random baselines.  The scores of a
block of users against every item come from one GEMM on the device
(``model.score_users``) instead of one ``predict`` call per user; the metrics that read
only the first k ranks (precision/recall@k, hit ratio, MAP@k) take them from the
device top-k (``model.topk_users`` -> rg_topk_rows, above k = 32 rg_topk_rows_wide) when the model
has one and k is within its limit -- the model's ``topk_users_max`` (1024 for
ImplicitFactorizationModel, so the usual cut-offs 50 and 100 stay on the device), 32 for a
model that names none -- so only users x k ids reach the host; mrr_score takes the ranks of the test items
from the device (``model.rank_users`` -> rg_rank_rows) when the model has it;
precision_recall_score_slates counts a device slates tensor's hits on the device (rg_slate_hits)."""
import numpy as np
import scipy.stats as st

FLOAT_MAX = np.finfo(np.float32).max


def _get_precision_recall(predictions, targets, k):
    predictions = predictions[:k]
    num_hit = len(set(predictions).intersection(set(targets)))
    return float(num_hit) / k, float(num_hit) / len(targets)


def _row(csr, u):
    """csr[u].indices without building a row matrix (per-user slicing dominated the loop)."""
    return csr.indices[csr.indptr[u]:csr.indptr[u + 1]]


def _user_blocks(test_csr, block=4096):
    """Yields (offset, user block) over the test users with items, in user order, ``block`` at a time."""
    users = np.flatnonzero(np.diff(test_csr.indptr) > 0)
    for s in range(0, len(users), block):
        yield s, users[s:s + block]


def _scored(model, test_csr, train_csr=None, block=4096):
    """Yields (user, row indices, -scores with train items at FLOAT_MAX) for every test
    user with items, in user order."""
    for _, ub in _user_blocks(test_csr, block):
        scores = -model.score_users(ub)                      # (len(ub), I) float32, host
        for r, u in enumerate(ub):
            pred = scores[r]
            if train_csr is not None:
                pred[_row(train_csr, u)] = FLOAT_MAX
            yield u, _row(test_csr, u), pred


TOPK_MAX = 32      # the device top-k limit of a model without a ``topk_users_max`` of its own


def _device_topk(model, k):
    return k <= getattr(model, "topk_users_max", TOPK_MAX) and hasattr(model, "topk_users")


def _ranked(model, test_csr, train_csr=None, block=4096, k=None):
    """Yields (user, row indices, item ranking) for every test user with items; with k,
    the ranking may hold only its first k entries (the device top-k)."""
    if k is not None and _device_topk(model, k):
        for _, ub in _user_blocks(test_csr, block):
            top = model.topk_users(ub, int(k), train_csr)      # (len(ub), k) int64, host
            for r, u in enumerate(ub):
                yield u, _row(test_csr, u), top[r]
        return
    for u, idx, pred in _scored(model, test_csr, train_csr, block):
        yield u, idx, pred.argsort(axis=0)


def _topk_hits(model, test_csr, train_csr, k, block=4096):
    """The device top-k path of the metrics (model.topk_users, k within _device_topk), vectorised over
    the users instead of a Python loop per user (the loop took 0.7 s per 125 k users): the users
    with test items, their top-k rankings, hits[u, j] = ranking j of user u is one of its test
    items (the rankings are distinct ids, so the count of hits in the first x ranks is the
    reference's |set(ranking[:x]) & set(targets)|), and each user's number of test items."""
    users = np.flatnonzero(np.diff(test_csr.indptr) > 0)
    if not len(users):
        return users, np.zeros((0, k), bool), np.zeros(0, np.int64)
    I = np.int64(test_csr.shape[1])
    rows = np.repeat(np.arange(test_csr.shape[0], dtype=np.int64), np.diff(test_csr.indptr))
    keys = np.sort(rows * I + test_csr.indices.astype(np.int64))
    hits = np.empty((len(users), k), bool)
    for s, ub in _user_blocks(test_csr, block):
        top = np.asarray(model.topk_users(ub, int(k), train_csr), dtype=np.int64)[:, :k]
        q = ub[:, None].astype(np.int64) * I + top
        pos = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
        hits[s:s + len(ub)] = keys[pos] == q
    return users, hits, np.diff(test_csr.indptr)[users].astype(np.int64)


def mrr_score(model, test, train=None):
    """Mean reciprocal rank of each test user's items (evaluation.py:13-60): ranks of
    -score with ties averaged (scipy rankdata), train items pushed to the end."""
    test_csr = test.tocsr()
    train_csr = train.tocsr() if train is not None else None
    if hasattr(model, "rank_users"):
        return _mrr_from_ranks(model, test_csr, train_csr)
    return np.array([(1.0 / st.rankdata(pred)[idx]).mean() for _, idx, pred in _scored(model, test_csr, train_csr)])


def _mrr_from_ranks(model, test_csr, train_csr, block=4096):
    """mrr_score's device path (model.rank_users -> rg_rank_rows): the same users in the same
    order as _scored, the ranks of each block's test items counted on the device (above +
    (equal + 1) / 2 is rankdata's average-tie rank), so only two counts per test item reach the
    host instead of the users x items score block."""
    n_t = np.diff(test_csr.indptr)
    users = np.flatnonzero(n_t > 0)
    out = np.empty(len(users), dtype=np.float64)
    for s, ub in _user_blocks(test_csr, block):
        n = n_t[ub]
        ranks = np.asarray(model.rank_users(ub, test_csr, train_csr), dtype=np.float64)
        out[s:s + len(ub)] = np.add.reduceat(1.0 / ranks, np.cumsum(n) - n) / n
    return out


def sequence_mrr_score(model, test, exclude_preceding=False):
    """Reciprocal rank of each sequence's last item given the rest (evaluation.py:62-106)."""
    sequences, targets = test.sequences[:, :-1], test.sequences[:, -1:]
    if hasattr(model, "rank_next"):     # ranks counted on the device, 4096 sequences per call
        mrrs = [1.0 / model.rank_next(sequences[i:i + 4096], targets[i:i + 4096, 0], exclude_preceding)
                for i in range(0, len(sequences), 4096)]
        return np.concatenate(mrrs) if mrrs else np.zeros(0)
    mrrs = []
    for i in range(len(sequences)):
        pred = -model.predict(sequences[i])
        if exclude_preceding:
            pred[sequences[i]] = FLOAT_MAX
        mrrs.append((1.0 / st.rankdata(pred)[targets[i]]).mean())
    return np.array(mrrs)


def precision_recall_score(model, test, train=None, k=10):
    test_csr = test.tocsr()
    train_csr = train.tocsr() if train is not None else None
    ks = np.array([k]) if np.isscalar(k) else np.asarray(k)
    if _device_topk(model, int(ks.max())):
        users, hits, n_t = _topk_hits(model, test_csr, train_csr, int(ks.max()))
        if train_csr is not None:
            print("Cold start users: ", int((np.diff(train_csr.indptr)[users] == 0).sum()))
        else:
            print("Cold start users: ", 0)
        c = np.cumsum(hits, axis=1)
        num = np.stack([c[:, int(x) - 1] for x in ks], axis=1).astype(np.float64)
        return (np.mean((num / ks.astype(np.float64)[None, :]).squeeze()),
                np.mean((num / n_t[:, None].astype(np.float64)).squeeze()))
    precision, recall = [], []
    cold = 0
    for u, targets, ranking in _ranked(model, test_csr, train_csr, k=int(ks.max())):
        if train_csr is not None and not len(_row(train_csr, u)):
            cold += 1
        p, r = zip(*[_get_precision_recall(ranking, targets, x) for x in ks])
        precision.append(p)
        recall.append(r)
    print("Cold start users: ", cold)
    return np.mean(np.array(precision).squeeze()), np.mean(np.array(recall).squeeze())


def rmse_score(net, user_ids, item_ids):
    predictions = net(user_ids, item_ids)
    array = 1 - predictions.cpu().detach().numpy()
    return np.sum(array ** 2)


def hit_ratio(model, test, k=10):
    hits = users = 0
    for _, target, ranking in _ranked(model, test.tocsr(), k=k):
        users += 1
        if target in ranking[:k]:
            hits += 1
    return hits / users


def apk(actual, predicted, k=10):
    if len(predicted) > k:
        predicted = predicted[:k]
    score, num_hits = 0.0, 0.0
    for i, p in enumerate(predicted):
        if p in actual and p not in predicted[:i]:
            num_hits += 1.0
            score += num_hits / (i + 1.0)
    if not actual.any():
        return 0.0
    return score / min(len(actual), k)


def mapk(actual, predicted, k=10):
    return np.mean([apk(a, p, k) for a, p in zip(actual, predicted)])


def map_at_k(model, test, k=5):
    if _device_topk(model, k):
        # apk over every user at once, its sums in apk's order (one position at a time)
        test_csr = test.tocsr()
        users, hits, n_t = _topk_hits(model, test_csr, None, k)
        cum = np.cumsum(hits, axis=1).astype(np.float64)
        score = np.zeros(len(users))
        for i in range(k):
            score = np.where(hits[:, i], score + cum[:, i] / (i + 1.0), score)
        first = test_csr.indices[test_csr.indptr[users]]
        only_zero = (n_t == 1) & (first == 0)          # apk: `not actual.any()` -> 0
        vals = np.where(only_zero, 0.0, score / np.minimum(n_t, k).astype(np.float64))
        return np.mean(vals.squeeze())
    vals = [apk(targets, ranking, k=k) for _, targets, ranking in _ranked(model, test.tocsr(), k=k)]
    return np.mean(np.array(vals).squeeze())


class _PredictRows:
    """``score_users`` over a model that has only the reference's ``predict(user)``."""

    def __init__(self, model):
        self._model = model

    def score_users(self, users):
        return np.stack([np.asarray(self._model.predict(int(u)), dtype=np.float32) for u in users])


def ndcg_at_k(model, test, train=None, k=10):
    """Mean binary-relevance NDCG@k over the FULL ranking (no reference counterpart): per test user
    with items, DCG = sum over the ranks j < k that hold one of its test items of 1 / log2(j + 2),
    IDCG the same sum over the first min(n_test, k) ranks; train items rank last.  float64 on the
    host, from the device top-k's hits (``_topk_hits``) where ``_device_topk(model, k)`` holds, from
    ``_ranked`` otherwise."""
    test_csr = test.tocsr()
    train_csr = train.tocsr() if train is not None else None
    k = int(k)
    disc = 1.0 / np.log2(np.arange(k, dtype=np.float64) + 2.0)
    ideal = np.cumsum(disc)
    if _device_topk(model, k):
        _, hits, n_t = _topk_hits(model, test_csr, train_csr, k)
    else:
        if not hasattr(model, "score_users"):       # a model with ``predict`` alone: one call per user
            model = _PredictRows(model)
        rows = [(np.isin(np.asarray(ranking[:k]), targets), len(targets))
                for _, targets, ranking in _ranked(model, test_csr, train_csr, k=k)]
        hits = np.array([np.pad(h, (0, k - len(h))) for h, _ in rows], dtype=bool).reshape(len(rows), k)
        n_t = np.array([n for _, n in rows], dtype=np.int64)
    dcg = np.zeros(len(n_t), dtype=np.float64)
    for j in range(k):                      # one rank at a time: the same sum on either path
        dcg = np.where(hits[:, j], dcg + disc[j], dcg)
    return np.mean(dcg / ideal[np.minimum(n_t, k) - 1])


def _interaction_keys(csr):
    rows = np.repeat(np.arange(csr.shape[0], dtype=np.int64), np.diff(csr.indptr))
    return rows * np.int64(csr.shape[1]) + csr.indices.astype(np.int64)


def sampled_candidate_lists(test, train=None, n_negatives=99, random_state=None):
    """The candidate lists of the sampled evaluation protocol (He et al., Neural Collaborative
    Filtering, 2017): one list per test interaction (the distinct (user, item) entries of
    ``test.tocsr()``, in its order), ``[target, negatives...]`` with ``n_negatives`` distinct items
    drawn uniformly from those in neither the user's test row nor its train row.  Returns ``(users
    int64 [m], ptr int64 [m + 1], idx int32 [m (1 + n_negatives)])``, the CSR ``score_candidates``
    and ``candidates.seg_rank`` take.  The draw is vectorised on the host -- draw every list at once,
    look the draws up in the sorted ``user * num_items + item`` keys of test and train, redraw only
    the collisions (and repeats within a list) -- from ``random_state`` (default
    ``np.random.RandomState(0)``): an equal seed reproduces it.  ValueError if some test user has
    fewer than ``n_negatives`` eligible items."""
    test_csr = test.tocsr()
    n_neg = int(n_negatives)
    if n_neg < 0:
        raise ValueError("n_negatives must be >= 0")
    rs = random_state if random_state is not None else np.random.RandomState(0)
    I = np.int64(test_csr.shape[1])
    keys = _interaction_keys(test_csr)
    if train is not None:
        train_csr = train.tocsr()
        if train_csr.shape != test_csr.shape:
            raise ValueError(f"train has shape {train_csr.shape}, test {test_csr.shape}")
        keys = np.concatenate([keys, _interaction_keys(train_csr)])
    keys = np.unique(keys)
    users = np.repeat(np.arange(test_csr.shape[0], dtype=np.int64), np.diff(test_csr.indptr))
    targets = test_csr.indices.astype(np.int64)
    m = len(users)
    taken = np.bincount(keys // I, minlength=test_csr.shape[0])
    if m and n_neg and (I - taken[users]).min() < n_neg:
        raise ValueError(f"a test user has fewer than {n_neg} items outside its test and train rows")
    neg = rs.randint(0, I, size=(m, n_neg)).astype(np.int64)

    def clashes(block, block_users):
        q = block_users[:, None] * I + block
        at = np.minimum(np.searchsorted(keys, q), max(len(keys) - 1, 0))
        bad = keys[at] == q if len(keys) else np.zeros(q.shape, bool)
        order = np.argsort(block, axis=1, kind="stable")         # a repeat: the later position is redrawn
        srt = np.take_along_axis(block, order, axis=1)
        rep = np.zeros(block.shape, bool)
        rep[:, 1:] = srt[:, 1:] == srt[:, :-1]
        dup = np.zeros(block.shape, bool)
        np.put_along_axis(dup, order, rep, axis=1)
        return bad | dup

    if m and n_neg:
        live = np.arange(m)
        for _ in range(64):
            bad = clashes(neg[live], users[live])
            hit = bad.any(axis=1)
            live, bad = live[hit], bad[hit]
            if not len(live):
                break
            sub = neg[live]
            sub[bad] = rs.randint(0, I, size=int(bad.sum()))
            neg[live] = sub
        else:
            # lists still clashing (a user with hardly more eligible items than n_negatives): drawn exactly
            for r in live:
                u = users[r]
                lo, hi = np.searchsorted(keys, [u * I, (u + 1) * I])
                free = np.setdiff1d(np.arange(I, dtype=np.int64), keys[lo:hi] - u * I, assume_unique=True)
                neg[r] = rs.choice(free, n_neg, replace=False)
    idx = np.concatenate([targets[:, None], neg], axis=1).astype(np.int32).reshape(-1)
    return users, np.arange(m + 1, dtype=np.int64) * (1 + n_neg), idx


def _ahead_host(scores, idx, width):
    """seg_rank's counts on the host for lists of one width: (m, 2) int64, the entries with a higher
    key than entry 0 and those with an equal key and a lower item id (the key of a NaN is -inf)."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1, width)
    s = np.where(np.isnan(s), np.float32(-np.inf), s)
    i = np.asarray(idx).reshape(-1, width)
    above = (s[:, 1:] > s[:, :1]).sum(axis=1)
    tied = ((s[:, 1:] == s[:, :1]) & (i[:, 1:] < i[:, :1])).sum(axis=1)
    return np.stack([above, tied], axis=1).astype(np.int64)


def sampled_hit_ndcg(model, test, train=None, n_negatives=99, k=10, random_state=None):
    """(HR@k, NDCG@k) of the sampled protocol the NCF paper reports (its 99 negatives and k = 10 are
    the defaults): every test interaction is ranked among the ``n_negatives`` items of its list
    (``sampled_candidate_lists``), ahead = the candidates with a higher score plus those with an equal
    score and a lower item id, HR = mean(ahead < k), NDCG = mean(1 / log2(ahead + 2) where ahead < k,
    else 0).  A model with ``score_candidates`` scores and counts on the device
    (``candidate_target_ranks`` -> rg_seg_rank: two counts per interaction come down); any other
    model takes the host path over ``model.predict(users, items)`` with the same ordering rule."""
    users, ptr, idx = sampled_candidate_lists(test, train, n_negatives, random_state)
    if not len(users):
        raise ValueError("sampled_hit_ndcg: the test set has no interactions")
    width = 1 + int(n_negatives)
    if hasattr(model, "score_candidates") and hasattr(model, "candidate_target_ranks"):
        counts = np.asarray(model.candidate_target_ranks(users, idx.reshape(-1, width)), dtype=np.int64)
    elif hasattr(model, "score_candidates"):
        counts = _ahead_host(model.score_candidates(users, idx.reshape(-1, width)), idx, width)
    else:
        counts = _ahead_host(model.predict(np.repeat(users, width), idx.astype(np.int64)), idx, width)
    ahead = counts.sum(axis=1)
    hit = ahead < int(k)
    gain = np.where(hit, 1.0 / np.log2(ahead.astype(np.float64) + 2.0), 0.0)
    return float(np.mean(hit)), float(np.mean(gain))


def intra_list_similarity(model, item_lists, metric="cosine", space=None):
    """The intra-list similarity of recommendation lists or slates: per list the mean similarity over
    the unordered pairs of its items, then the mean over the lists -- lower is more diverse.
    ``item_lists``: an ``(n, k)`` integer array or a list of id sequences; a negative id (the -1 fill
    of ``rank_candidates`` / ``diversify_candidates``) is skipped, a list with fewer than two items
    counts 0.  The items are compared in ``model``'s item space -- any fitted
    ImplicitFactorizationModel, whatever produced the lists (``recommend*`` outputs and cGAN slates
    alike) -- with ``similar_items``' ``metric`` ("cosine" / "dot") and ``space``.  Computed on the
    device (rg_seg_mean_sim, ``candidates.seg_mean_sim``): the lists go up, one value per list comes
    down.  ValueError for no lists, a list of more than 1024 items, ids that are not integers, an id
    at or beyond ``num_items``, an unknown ``metric`` or an unknown ``space``."""
    import torch
    from .. import candidates as cand
    from .. import mf_engine
    if isinstance(item_lists, np.ndarray) and item_lists.ndim == 2:
        lists = list(item_lists)
    else:
        lists = [np.asarray(r).reshape(-1) for r in item_lists]
    if not len(lists):
        raise ValueError("intra_list_similarity: no lists")
    if any(len(r) and np.asarray(r).dtype.kind not in "iu" for r in lists):
        raise ValueError("intra_list_similarity: the lists must hold integer item ids")
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in lists], out=ptr[1:])
    if np.diff(ptr).max() > cand.SEG_MMR_MAX_LEN:
        raise ValueError(f"intra_list_similarity: a list is longer than {cand.SEG_MMR_MAX_LEN} items")
    idx = np.concatenate(lists).astype(np.int64) if ptr[-1] else np.zeros(0, dtype=np.int64)
    if len(idx) and idx.max() >= model._num_items:
        raise ValueError("intra_list_similarity: item id outside [0, num_items)")
    model._check_metric(metric)
    space = model._check_space(space)
    if not ptr[-1]:
        return 0.0
    table = model._item_table(space).contiguous()
    rnorm = mf_engine.row_rnorms(table) if metric == "cosine" else None
    dev = table.device
    sims = cand.seg_mean_sim(torch.as_tensor(ptr, device=dev), torch.as_tensor(np.maximum(idx, -1).astype(np.int32),
                                                                               device=dev),
                             table, rnorm=rnorm, checked=True)
    return float(sims.double().mean().item())


def evaluate_popItems(item_popularity, test, k=10):
    test = test.tocsr()
    pop = np.asarray(getattr(item_popularity, "values", item_popularity))
    pop_top = pop.argsort()[::-1][:k]
    ks = np.array([k]) if np.isscalar(k) else np.asarray(k)
    precision, recall = [], []
    for row in test:
        if not len(row.indices):
            continue
        p, r = zip(*[_get_precision_recall(pop_top, row.indices, x) for x in ks])
        precision.append(p)
        recall.append(r)
    return np.mean(precision), np.mean(recall),


def evaluate_random(item_popularity, test, k=10):
    all_items = test.num_items
    test = test.tocsr()
    ks = np.array([k]) if np.isscalar(k) else np.asarray(k)
    precision, recall = [], []
    for row in test:
        if not len(row.indices):
            continue
        predictions = np.random.choice(all_items, len(row.indices))
        p, r = zip(*[_get_precision_recall(predictions, row.indices, x) for x in ks])
        precision.append(p)
        recall.append(r)
    return np.mean(np.array(precision).squeeze()), np.mean(np.array(recall).squeeze())


SLATE_HITS_MAX_K = 32


def slate_precision_recall(masks, n_targets, k):
    """The precision / recall lists of precision_recall_score_slates from the device's hit
    masks (rg_slate_hits: bit j of a user's word = slate position j is a first occurrence and
    one of the user's targets) and each user's number of targets: for the users with targets,
    in order, hits / k and hits / len(targets) in float64, hits = the set bits below k, which is
    _get_precision_recall's len(set(pred[:k]) & set(targets))."""
    m = np.ascontiguousarray(masks).reshape(-1)
    m = m.view(np.uint32) if m.dtype == np.int32 else m.astype(np.uint32)
    n = np.asarray(n_targets, dtype=np.int64).reshape(-1)
    if k < 32:
        m = m & np.uint32((1 << int(k)) - 1)
    hits = np.unpackbits(m.view(np.uint8)).reshape(-1, 32).sum(axis=1)
    keep = n > 0
    hits = hits[keep].astype(np.float64)
    return (hits / float(k)).tolist(), (hits / n[keep].astype(np.float64)).tolist()


def _score_slates_device(slates, test, k):
    """precision_recall_score_slates for a slates tensor on a GPU: the hits of every row counted
    by one rg_slate_hits launch, one download of one word per row."""
    import torch
    from ..gan_engine import csr_to_device, slate_hits
    rows = test.shape[0]
    if slates.shape[0] < rows:
        raise IndexError(f"{rows} test rows but only {slates.shape[0]} slates")
    s = slates[:rows]
    if not s.dtype.is_floating_point and s.dtype != torch.int32:
        # an id outside int32 cannot be a CSR index; -1 is none either
        s = torch.where((s >= -2 ** 31) & (s < 2 ** 31), s, -1)
    s = s.to(torch.int32).contiguous()
    tp, ti = csr_to_device(test, rows, s.device)
    masks = slate_hits(s, tp, ti, min(k, s.shape[1])).cpu().numpy()
    return slate_precision_recall(masks, np.diff(test.indptr), k)


def precision_recall_score_slates(slates, test, k=3):
    """spotlight/evaluation.py:355-382: precision / recall@k of each test user's
    generated slate (row u of ``slates`` belongs to row u of the CSR ``test``).  A slates
    tensor on a GPU is counted there (rg_slate_hits) when k <= 32; CPU tensors and arrays
    take the host loop."""
    ks = np.array([k]) if np.isscalar(k) else np.asarray(k)
    test = test.tocsr()
    if getattr(slates, "is_cuda", False):
        k0 = int(ks.reshape(-1)[0])                     # only the first k's figures are returned
        if slates.dim() == 2 and 1 <= min(k0, slates.shape[1]) <= SLATE_HITS_MAX_K:
            return _score_slates_device(slates, test, k0)
        slates = slates.cpu()
    precision, recall = [], []
    for user_id in range(test.shape[0]):
        targets = test.indices[test.indptr[user_id]:test.indptr[user_id + 1]]
        if not len(targets):
            continue
        pred = slates[user_id].numpy() if hasattr(slates[user_id], "numpy") else np.asarray(slates[user_id])
        p, r = zip(*[_get_precision_recall(pred, targets, x) for x in ks])
        precision.append(p[0])
        recall.append(r[0])
    return precision, recall


def precision_recall_slates_atk(fake_slates, real_slates, k=3):
    """spotlight/evaluation.py:394-412, the generator's training precision / recall.
    The reference intersects sets of 0-d torch tensors (rows of the two slate
    tensors), which hash by identity, so every user scores 0; the same operations on
    the same tensor types are kept here so summary.csv matches the reference."""
    ks = np.array([k]) if np.isscalar(k) else np.asarray(k)
    precision, recall = [], []
    for user_id in range(fake_slates.shape[0]):
        p, r = zip(*[_get_precision_recall(fake_slates[user_id, :], real_slates[user_id, :], x) for x in ks])
        precision.append(p[0])
        recall.append(r[0])
    return precision, recall
