"""The pooling sequence model without a GPU: the tests' oracle against the fixture recorded from
the reference's PoolNet, ``to_sequence`` on a log worked out by hand, every refusal, the gradient
cases' preconditions, and ``sequence_mrr_score``'s untouched host loop."""
import numpy as np
import pytest
import torch

from recommendation_gans_amd import seq_engine
from recommendation_gans_amd.spotlight import evaluation
from recommendation_gans_amd.spotlight.interactions import Interactions, SequenceInteractions
from recommendation_gans_amd.spotlight.sequence import ImplicitSequenceModel
from recommendation_gans_amd.synthetic import generate_sequential
from tests import fold_in_common as fc
from tests import seq_common as sc


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_oracle_reproduces_the_reference_poolnet_fixture(dtype):
    fx = sc.load_fixture()
    E, b = torch.from_numpy(fx["E"]).to(dtype), torch.from_numpy(fx["b"]).to(dtype)
    seq, tgt = torch.from_numpy(fx["sequences"]), torch.from_numpy(fx["targets"])
    assert not fx["E"][0].any() and fx["b"][0] == 0 and (fx["sequences"] == 0).any()
    every, final = sc.representations(E, seq)
    assert _rel(every.numpy().transpose(0, 2, 1), fx["representations"]) <= 1e-6      # the reference's is [n, d, L]
    assert _rel(final.numpy(), fx["final"]) <= 1e-6
    scores = b[tgt] + (every * E[tgt]).sum(-1)
    assert _rel(scores.numpy(), fx["scores"]) <= 1e-6
    # the step's own scores are the same formula with the sequence as its targets (fixture row 5)
    zp, _ = sc.position_scores(E, b, seq, seq[None])
    assert _rel(zp.numpy()[5], fx["scores"][5]) <= 1e-6
    # the product's torch chain states the same model
    ev2, fin2 = seq_engine.pool_reprs_torch(E, seq)
    assert _rel(ev2.numpy(), every.numpy()) <= 1e-6 and _rel(fin2.numpy(), final.numpy()) <= 1e-6


def _log():
    """Three users, timestamps shuffled: user 0 saw 1..7, user 1 saw 8, 9, user 2 saw 10..12."""
    users = np.array([0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2], dtype=np.int32)
    items = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], dtype=np.int32)
    ts = np.arange(12, dtype=np.int32)
    order = np.random.RandomState(3).permutation(12)
    return Interactions(users[order], items[order], timestamps=ts[order], num_users=3, num_items=13)


def test_to_sequence_windows_and_padding_by_hand():
    log = _log()
    s = log.to_sequence(max_sequence_length=3)                          # step_size None: windows do not overlap
    assert isinstance(s, SequenceInteractions) and s.num_items == 13 and s.max_sequence_length == 3
    assert s.sequences.tolist() == [[5, 6, 7], [2, 3, 4], [0, 0, 1], [0, 8, 9], [10, 11, 12]]
    assert s.user_ids.tolist() == [0, 0, 0, 1, 2]
    s = log.to_sequence(max_sequence_length=3, step_size=1)
    assert s.sequences.tolist() == [[5, 6, 7], [4, 5, 6], [3, 4, 5], [2, 3, 4], [1, 2, 3], [0, 1, 2], [0, 0, 1],
                                    [0, 8, 9], [0, 0, 8], [10, 11, 12], [0, 10, 11], [0, 0, 10]]
    assert s.user_ids.tolist() == [0] * 7 + [1] * 2 + [2] * 3
    # user 1 has two items: with min_sequence_length 3 none of its windows stays
    s = log.to_sequence(max_sequence_length=3, min_sequence_length=3, step_size=1)
    assert s.sequences.tolist() == [[5, 6, 7], [4, 5, 6], [3, 4, 5], [2, 3, 4], [1, 2, 3], [10, 11, 12]]
    assert s.user_ids.tolist() == [0] * 5 + [2]
    s = log.to_sequence(max_sequence_length=4, min_sequence_length=2)
    assert s.sequences.tolist() == [[4, 5, 6, 7], [0, 1, 2, 3], [0, 0, 8, 9], [0, 10, 11, 12]]
    assert len(s) == 4


def test_refusals():
    with pytest.raises(ValueError, match="probabilities.*mask"):
        ImplicitSequenceModel(loss="pointwise")
    for rep in ("cnn", "lstm", "mixture", object()):
        with pytest.raises(NotImplementedError):
            ImplicitSequenceModel(representation=rep)
    with pytest.raises(NotImplementedError):
        ImplicitSequenceModel(optimizer_func=lambda p: torch.optim.SGD(p, lr=0.1))
    for d in (6, 0, 2, 260):
        with pytest.raises(ValueError, match="multiple of 4"):
            ImplicitSequenceModel(embedding_dim=d)
    # item id 0 in the input
    with pytest.raises(ValueError, match="padding"):
        Interactions(np.array([0, 0]), np.array([0, 3]), timestamps=np.array([0, 1]), num_users=1,
                     num_items=4).to_sequence(3)
    with pytest.raises(ValueError, match="timestamps"):
        Interactions(np.array([0, 0]), np.array([1, 3]), num_users=1, num_items=4).to_sequence(3)
    # ids >= num_items
    with pytest.raises(ValueError, match="number of items"):
        SequenceInteractions(np.array([[1, 5]]), num_items=5)
    model = ImplicitSequenceModel(embedding_dim=8)
    model._num_items = 5
    with pytest.raises(ValueError, match="number of items"):
        model._check_input(np.array([[0, 1, 5]]))
    E, b = torch.zeros(5, 8), torch.zeros(5)
    seq, neg = torch.tensor([[0, 1, 2]]), torch.tensor([[[1, 1, 1]]])
    with pytest.raises(ValueError, match="number of items"):
        seq_engine.pool_grads(E, b, torch.tensor([[0, 1, 5]]), neg, "bpr")
    with pytest.raises(ValueError, match="number of items"):
        seq_engine.pool_grads(E, b, seq, torch.tensor([[[1, 7, 1]]]), "bpr")
    with pytest.raises(ValueError, match="negative"):
        seq_engine.pool_grads(E, b, torch.tensor([[0, -1, 2]]), neg, "bpr")
    with pytest.raises(ValueError, match="probabilities.*mask"):
        seq_engine.pool_grads(E, b, seq, neg, "pointwise")
    # d not a multiple of 4, at the engine
    with pytest.raises(ValueError, match="multiple of 4"):
        seq_engine.pool_grads(torch.zeros(5, 6), b, seq, neg, "bpr")
    # a batch of padding alone
    with pytest.raises(ValueError, match="padding only"):
        seq_engine.pool_grads(E, b, torch.zeros(2, 3, dtype=torch.int64), torch.ones(1, 2, 3, dtype=torch.int64), "bpr")
    with pytest.raises(ValueError, match="K, B, L"):
        seq_engine.pool_grads(E, b, seq, torch.ones(1, 2, 3, dtype=torch.int64), "bpr")
    with pytest.raises(ValueError):
        seq_engine.pool_grads(E, b, seq, torch.ones(17, 1, 3, dtype=torch.int64), "bpr")      # K > 16


def test_no_gradient_case_sits_on_a_kink_and_every_feature_is_present():
    """What the GPU comparison assumes of its inputs, checked without a GPU."""
    for i, (d, L, B, K, num_items, loss) in enumerate(sc.CASES):
        case = sc.make_case(d, L, B, K, num_items)
        assert sc.kink_margin(case, loss) > fc.TIE, sc.CASE_IDS[i]
        seq, neg = case["seq"], case["neg"]
        assert seq.min() >= 0 and seq.max() < num_items and neg.min() >= 0 and neg.max() < num_items
        assert (seq[:, -1] != 0).all() and (seq[0] != 0).all()
        if B >= 3 and L >= 2:
            assert (seq[1] == 0).any() and (seq[2] != 0).sum() == 1
        if L >= 2:
            r = min(3, B - 1)
            assert seq[r, -1] == seq[r, -2] or B > 1
    big = sc.make_case(8, 33, 257, 5, 1000)
    assert (big["neg"] == 0).any() and (big["neg"][-1] == big["seq"]).any()
    assert (big["seq"][3, -1] == big["seq"][3, -2]) or (big["seq"][3] != 0).sum() < 2
    data = sc.case_data(3)
    assert data["e32"] > 0 and not data["r64"]["gE"][0].any() and data["r64"]["gb"][0] == 0
    assert not data["r64"]["aE"][0].any() and (data["r64"]["aE"] >= np.abs(data["r64"]["gE"]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("name, d, loss", sc.EDGE_CASES)
def test_no_edge_case_sits_on_a_kink_and_each_holds_its_edge(name, d, loss):
    case = sc.edge_case(name, d)
    assert sc.kink_margin(case, loss) > fc.TIE
    seq, neg, N = case["seq"], case["neg"], case["num_items"]
    assert seq.min() >= 0 and seq.max() < N and neg.min() >= 0 and neg.max() < N
    items = (seq != 0).sum(1)
    if name in ("scatter", "inside"):
        # zeros among the items, not only on the left; a row ending in one; no row of padding alone
        first = (seq != 0).argmax(1)
        assert sum((seq[r, first[r]:] == 0).any() for r in range(len(seq))) > len(seq) // 2
        assert seq[0, -1] == 0 and (items >= 1).all()
    if name == "inside":
        out = sc.edge_case("outside", d)
        bad = sc.outside_ids(N)
        assert np.isin(out["seq"][seq == 0], bad).all() and (out["seq"][seq != 0] == seq[seq != 0]).all()
        moved = out["neg"] != neg
        assert moved.mean() > 0.05 and np.isin(out["neg"][moved], bad).all() and (neg[moved] == 0).all()
        for b in bad:
            assert (out["seq"] == b).any() and (out["neg"] == b).any()
    if name == "empty":
        assert items[4] == 0 and items[8] == 0 and len(seq) == 9 and (np.delete(items, [4, 8]) >= 1).all()
    if name == "maxlen":
        assert seq.shape == (3, seq_engine.SEQ_MAX_LEN) and neg.shape[0] == seq_engine.SEQ_MAX_NEG
        assert items.tolist() == [1024, 512, 1]
    data = sc.edge_data(name, d, loss)
    assert data["e32"] > 0 and not data["r64"]["gE"][0].any() and data["r64"]["gb"][0] == 0


def test_generate_sequential_is_seeded_and_keeps_id_zero_free():
    a = generate_sequential(20, 30, 400, 0.01, 1, np.random.RandomState(5))
    b = generate_sequential(20, 30, 400, 0.01, 1, np.random.RandomState(5))
    assert (a.item_ids == b.item_ids).all() and (a.user_ids == b.user_ids).all()
    assert a.item_ids.min() >= 1 and a.item_ids.max() < 30 and len(a) == 400 and a.num_items == 30
    assert (np.diff(a.user_ids) >= 0).all() and (np.diff(a.timestamps) > 0).all()
    # order 1 with a small concentration is predictable: the most frequent successor of an item
    # follows it far more often than 1 / 29
    nxt = {}
    for x, y in zip(a.item_ids[:-1], a.item_ids[1:]):
        nxt.setdefault(int(x), []).append(int(y))
    hit = sum(max(np.bincount(v)) for v in nxt.values()) / (len(a) - 1)
    assert hit > 0.5
    assert a.to_sequence(5).sequences.shape[1] == 5


class _Stub:
    """A model without rank_next: scores fixed per item, the first item of the sequence favoured."""

    def __init__(self, num_items):
        self.base = np.linspace(0.0, 1.0, num_items)
        self.calls = 0

    def predict(self, sequence):
        self.calls += 1
        out = self.base.copy()
        out[sequence[0]] += 2.0
        return out


def test_sequence_mrr_score_walks_the_old_loop_for_a_model_without_rank_next():
    seqs = np.array([[3, 1, 2, 5], [0, 4, 1, 9], [7, 7, 2, 7]])
    test = SequenceInteractions(seqs, num_items=10)
    stub = _Stub(10)
    got = evaluation.sequence_mrr_score(stub, test)
    assert stub.calls == 3
    # by hand: scores ascend with the id, +2 on the sequence's first id; rank of the last id
    # row 0: favoured 3; target 5 is beaten by 3, 6, 7, 8, 9 -> rank 6
    # row 1: favoured 0; target 9 is beaten by 0 -> rank 2
    # row 2: favoured 7 is the target -> rank 1
    assert np.allclose(got, [1 / 6, 1 / 2, 1.0], rtol=0, atol=1e-15)
    got = evaluation.sequence_mrr_score(stub, test, exclude_preceding=True)
    # row 0: 3 leaves the ranking: 6, 7, 8, 9 -> rank 5; row 1: 0 leaves -> rank 1; row 2: the
    # target itself is excluded (FLOAT_MAX, shared with 2): ranks 9 and 10 tie at 9.5 ... with 7
    # listed once among the distinct ids {7, 2}: average of the last two ranks
    assert np.allclose(got, [1 / 5, 1.0, 1 / 9.5], rtol=0, atol=1e-15)
