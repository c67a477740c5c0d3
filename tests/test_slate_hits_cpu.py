"""The host half of the device slate evaluation (no GPU): evaluation.slate_precision_recall
turns the hit masks of rg_slate_hits and each user's number of held-out items into the two
lists precision_recall_score_slates returns.  Checked against _get_precision_recall per user
on slates and targets built to produce given masks."""
import numpy as np
import pytest

from recommendation_gans_amd.spotlight.evaluation import _get_precision_recall, slate_precision_recall


def users_for(masks, lens, S, rs):
    """Slates of S distinct items and target lists of the given lengths whose hits at the slate
    positions are exactly the masks' bits (the other targets are items outside every slate)."""
    slates, targets = [], []
    for m, n in zip(masks, lens):
        pred = rs.permutation(1000)[:S]
        hit = [int(pred[j]) for j in range(S) if (int(m) >> j) & 1]
        assert len(hit) <= n or n == 0
        rest = (1000 + rs.permutation(1000)[:max(n - len(hit), 0)]).tolist()
        t = np.array(hit + rest, dtype=np.int32) if n else np.zeros(0, np.int32)
        slates.append(pred)
        targets.append(rs.permutation(t))
    return slates, targets


@pytest.mark.parametrize("S,k,dtype", [(5, 5, np.int32), (5, 3, np.uint32), (7, 1, np.int32), (32, 32, np.int32),
                                       (32, 17, np.uint32)])
def test_lists_match_get_precision_recall(S, k, dtype):
    rs = np.random.RandomState(S * 100 + k)
    users = 300
    masks = rs.randint(0, 2 ** 32, users, dtype=np.uint64).astype(np.uint32)
    if S < 32:
        masks &= np.uint32((1 << S) - 1)
    masks[::11] = 0
    masks[5] = (1 << S) - 1 if S < 32 else 0xffffffff      # every position hits (bit 31: a negative int32)
    lens = np.array([bin(int(m)).count("1") + rs.randint(0, 40) for m in masks])
    lens[::7] = 0                                          # users without targets: not in the lists
    slates, targets = users_for(masks, lens, S, rs)
    precision, recall = slate_precision_recall(masks.view(dtype), lens, k)
    want = [_get_precision_recall(p, t, k) for p, t in zip(slates, targets) if len(t)]
    assert len(want) == int((lens > 0).sum()) and len(precision) == len(recall) == len(want)
    assert precision == [w[0] for w in want] and recall == [w[1] for w in want]
    assert all(type(x) is float for x in precision + recall)
    assert float(np.mean(precision)) == float(np.mean([w[0] for w in want]))


def test_no_users_with_targets():
    assert slate_precision_recall(np.array([3, 1], np.int32), [0, 0], 3) == ([], [])
    assert slate_precision_recall(np.zeros(0, np.int32), np.zeros(0, np.int64), 3) == ([], [])
