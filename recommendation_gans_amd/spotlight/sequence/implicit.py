"""ImplicitSequenceModel (spotlight/sequence/implicit.py of the reference) for two
representations.  ``representation='pooling'``: a session is the mean of the items seen so far
(PoolNet; Covington et al. 2016).  ``representation=<a representations.CNNNet>``: stacked causal
dilated convolutions over the items seen so far (the reference's own way to configure widths and
dilations); the net gives the configuration, ``embedding_dim``, ``num_items`` and the initial
parameters.  Either way the next item is scored b[i] + <r, E[i]>.

The constructor, ``fit`` and ``predict`` keep the reference's signatures.  What differs, on purpose:
  * the reference's class cannot run (its ``sample_items`` call no longer matches sampling.py), so
    the step is defined in include/rg_hip.h (rg_seq_pool_grads) and runs there: forward, loss and
    backward in one launch, torch's dense Adam in a second (rg_seq_adam_dense);
  * ``loss='pointwise'`` is refused: the reference's pointwise loss takes probabilities and drops
    the mask;
  * only ``'pooling'``, a ``CNNNet`` instance and the default Adam exist (NotImplementedError
    otherwise: the strings 'cnn', 'lstm' and 'mixture' among them);
  * negatives come from ``sampling.sample_items(..., device=)``: NumPy's ids, bit for bit, drawn on
    the GPU, the model's RandomState advanced as NumPy advances it.
Serving on top: ``predict_batch`` (a device score block), ``recommend_next`` (top-k, preceding
items and the padding id left out) and ``rank_next`` (what ``evaluation.sequence_mrr_score``
reads)."""
import numpy as np
import torch

from ... import _lib, seq_engine
from ..layers import ScaledEmbedding, ZeroEmbedding
from .representations import CNNNet
from ..sampling import sample_items
from ..torch_utils import shuffle

PADDING_IDX = 0
SERVE_BLOCK = 1024      # sequences per score block of recommend_next / rank_next


class ImplicitSequenceModel:
    def __init__(self, loss="bpr", representation="pooling", embedding_dim=32, n_iter=10, batch_size=256, l2=0.0,
                 learning_rate=1e-2, optimizer_func=None, use_cuda=True, sparse=False, random_state=None,
                 num_negative_samples=5):
        seq_engine.check_loss(loss)
        self._net = self._cnn = None
        if isinstance(representation, CNNNet):
            self._net, self._cnn = representation, seq_engine.cnn_config_of(representation)
            embedding_dim = representation.embedding_dim
        elif isinstance(representation, str) and representation == "cnn":
            raise NotImplementedError("representation 'cnn': pass a representations.CNNNet instance, which carries "
                                      "the widths, dilations and initial parameters")
        elif not (isinstance(representation, str) and representation == "pooling"):
            raise NotImplementedError(f"representation {representation!r}: only 'pooling' and a CNNNet instance "
                                      f"are implemented")
        if optimizer_func is not None:
            raise NotImplementedError("optimizer_func: the fused step runs torch.optim.Adam's update only")
        seq_engine.check_dim(int(embedding_dim))
        if not use_cuda:
            raise ValueError("ImplicitSequenceModel runs on the GPU only (use_cuda=False has no path here)")
        if loss == "adaptive_hinge" and not 1 <= num_negative_samples <= seq_engine.SEQ_MAX_NEG:
            raise ValueError(f"num_negative_samples must be in [1, {seq_engine.SEQ_MAX_NEG}]")
        self._loss = loss
        self._representation = representation
        self._embedding_dim = int(embedding_dim)
        self._n_iter = n_iter
        self._batch_size = int(batch_size)
        self._l2 = float(l2)
        self._learning_rate = float(learning_rate)
        self._use_cuda = use_cuda
        self._random_state = random_state or np.random.RandomState()
        self._num_negative_samples = int(num_negative_samples) if loss == "adaptive_hinge" else 1
        self._num_items = None
        self._step = 0
        self._E = self._b = None

    def __repr__(self):
        return "<{}: {}, d = {}>".format(self.__class__.__name__, "cnn" if self._cnn else "pooling",
                                         self._embedding_dim)

    @property
    def _initialized(self):
        return self._E is not None

    def _initialize(self, interactions, device=None):
        _lib.require_gpu()
        dev = torch.device(device if device is not None else "cuda")
        self._num_items = int(interactions.num_items)
        if self._num_items < 2:
            raise ValueError("the model needs at least one item beside the padding id 0")
        if self._net is not None:
            if self._net.num_items != self._num_items:
                raise ValueError("the net was built for {} items, the interactions hold {}".format(
                    self._net.num_items, self._num_items))
            self.set_tables(self._net.item_embeddings.weight.data, self._net.item_biases.weight.data.reshape(-1),
                            device=dev)
            return
        E = ScaledEmbedding(self._num_items, self._embedding_dim, padding_idx=PADDING_IDX).weight.data
        b = ZeroEmbedding(self._num_items, 1, padding_idx=PADDING_IDX).weight.data.reshape(-1)
        self.set_tables(E, b, device=dev)

    def set_tables(self, E, b, conv=None, device=None):
        """Start from the given tables (row 0 must be zero); the Adam state starts over.  With a
        CNNNet, ``conv`` is the flat vector of the convolutions' parameters
        (``seq_engine.cnn_pack``); None: the net's own current ones."""
        _lib.require_gpu()
        dev = torch.device(device if device is not None else "cuda")
        E = torch.as_tensor(E, dtype=torch.float32)
        b = torch.as_tensor(b, dtype=torch.float32).reshape(-1)
        if E.dim() != 2 or E.shape[1] != self._embedding_dim or b.numel() != E.shape[0]:
            raise ValueError("tables must be E [num_items, embedding_dim] and b [num_items]")
        if bool(E[0].any()) or bool(b[0] != 0):
            raise ValueError("row 0 is the padding row and must be zero")
        self._num_items = int(E.shape[0])
        self._E, self._b = E.to(dev).contiguous().clone(), b.to(dev).contiguous().clone()
        self._moments = [torch.zeros_like(self._E), torch.zeros_like(self._E),
                         torch.zeros_like(self._b), torch.zeros_like(self._b)]
        self._grad = torch.zeros(self._num_items, self._embedding_dim + 1, dtype=torch.float32, device=dev)
        self._step = 0
        if self._cnn is None:
            if conv is not None:
                raise ValueError("conv: the pooling representation has no convolution parameters")
            return
        if conv is None:
            conv = seq_engine.cnn_pack(self._cnn, [(c.weight.data, c.bias.data) for c in self._net.cnn_layers])
        conv = torch.as_tensor(conv, dtype=torch.float32).reshape(-1)
        if conv.numel() != seq_engine.cnn_param_len(self._cnn):
            raise ValueError("conv must hold {} floats".format(seq_engine.cnn_param_len(self._cnn)))
        self._conv = conv.to(dev).contiguous().clone()
        self._conv_moments = [torch.zeros_like(self._conv), torch.zeros_like(self._conv)]
        self._conv_grad = torch.zeros_like(self._conv)
        self._conv_ws = self._conv_ws_shape = None

    def conv_state_dict(self):
        """The convolutions' parameters in the reference's layout: {'cnn_i.weight': [d, d, w, 1],
        'cnn_i.bias': [d]} on the host."""
        if self._cnn is None or not self._initialized:
            raise RuntimeError("no convolution parameters: the model is not an initialised CNN model")
        out = {}
        for i, (W, c) in enumerate(seq_engine.cnn_unpack(self._cnn, self._conv.cpu())):
            out["cnn_{}.weight".format(i)], out["cnn_{}.bias".format(i)] = W.contiguous().clone(), c.clone()
        return out

    @property
    def item_embeddings(self):
        return self._E

    @property
    def item_biases(self):
        return self._b

    def _check_input(self, item_ids):
        item_ids = np.asarray(item_ids)
        if item_ids.size and item_ids.max() >= self._num_items:
            raise ValueError("Maximum item id greater than number of items in model.")
        if item_ids.size and item_ids.min() < 0:
            raise ValueError("Negative item id.")

    def train_batch(self, batch, mask_count=None):
        """One step on a device block of sequences [B, L] whose ids were checked: the negatives'
        draw, rg_seq_pool_grads (a CNNNet: rg_seq_cnn_grads), rg_seq_adam_dense (and
        rg_seq_adam_flat on the convolutions).  Returns the loss as a 0-d device tensor."""
        B, L = (int(x) for x in batch.shape)
        K = self._num_negative_samples
        if mask_count is None:
            mask_count = int((batch != PADDING_IDX).sum())
        if mask_count <= 0:
            raise ValueError("the batch holds padding only (mask.sum() == 0)")
        neg = sample_items(None, None, self._num_items, (K * B, L), random_state=self._random_state,
                           device=self._E.device).view(K, B, L)
        if self._cnn is None:
            loss, _ = seq_engine.pool_grads(self._E, self._b, batch, neg, self._loss, grad=self._grad,
                                            mask_count=mask_count, checked=True)
        else:
            if self._conv_ws is None or self._conv_ws_shape != (B, L, K):      # kept between steps of one shape
                self._conv_ws = seq_engine.cnn_workspace(self._cnn, B, L, K, self._E.device)
                self._conv_ws_shape = (B, L, K)
            loss, _, _ = seq_engine.cnn_grads(self._cnn, self._E, self._b, self._conv, batch, neg, self._loss,
                                              grad=self._grad, mask_count=mask_count, checked=True,
                                              param_grad=self._conv_grad, workspace=self._conv_ws)
        self._step += 1
        mE, vE, mb, vb = self._moments
        seq_engine.adam_dense(self._E, self._b, mE, vE, mb, vb, self._grad, self._step, self._learning_rate,
                              weight_decay=self._l2)
        if self._cnn is not None:
            seq_engine.adam_flat(self._conv, *self._conv_moments, self._conv_grad, self._step, self._learning_rate,
                                 weight_decay=self._l2)
        return loss

    def fit(self, interactions, verbose=False):
        """Fit the model; called again, it resumes (tables, Adam state and step count are kept)."""
        sequences = np.asarray(interactions.sequences).astype(np.int64)
        if sequences.ndim != 2 or sequences.shape[1] < 1 or sequences.shape[1] > seq_engine.SEQ_MAX_LEN:
            raise ValueError(f"sequences must be [n, L] with 1 <= L <= {seq_engine.SEQ_MAX_LEN}")
        if not self._initialized:
            self._initialize(interactions)
        self._check_input(sequences)
        dev = self._E.device
        for epoch_num in range(self._n_iter):
            sequences = shuffle(sequences, random_state=self._random_state)
            counts = (sequences != PADDING_IDX).sum(axis=1)
            seq_dev = torch.from_numpy(sequences).to(dev)
            losses = []
            for i in range(0, len(sequences), self._batch_size):
                losses.append(self.train_batch(seq_dev[i:i + self._batch_size],
                                               mask_count=int(counts[i:i + self._batch_size].sum())))
            epoch_loss = float(torch.stack(losses).double().sum()) / len(losses) if losses else 0.0
            if verbose:
                print("Epoch {}: loss {}".format(epoch_num, epoch_loss))
            if np.isnan(epoch_loss) or epoch_loss == 0.0:
                raise ValueError("Degenerate epoch loss: {}".format(epoch_loss))

    # ------------------------------------------------------------------ serving
    def _sequences_dev(self, sequences):
        if not self._initialized:
            raise RuntimeError("the model is not fitted")
        sequences = np.atleast_2d(np.asarray(sequences)).astype(np.int64)
        if sequences.ndim != 2 or sequences.shape[1] > seq_engine.SEQ_MAX_LEN:
            raise ValueError(f"sequences must be [n, L] with L <= {seq_engine.SEQ_MAX_LEN}")
        self._check_input(sequences)
        return sequences, torch.from_numpy(sequences).to(self._E.device)

    def predict_batch(self, sequences):
        """Raw next-item scores of every item for a block of sequences [n, L]: a float32
        [n, num_items] block on the device (rg_seq_pool_repr or rg_seq_cnn_repr, then
        rg_mf_score_users_raw)."""
        _, seq_dev = self._sequences_dev(sequences)
        return self._scores(seq_dev)

    def _scores(self, seq_dev):
        if self._cnn is not None:
            R = seq_engine.cnn_repr(self._cnn, self._E, self._conv, seq_dev, checked=True)
        else:
            R = seq_engine.pool_repr(self._E, seq_dev, checked=True)
        return seq_engine.score_block_raw(R, self._E, self._b)

    def predict(self, sequences, item_ids=None):
        """The reference's predict: raw scores of ``item_ids`` (default: every item) as the next
        item of ONE sequence, a float32 numpy array."""
        sequences = np.asarray(sequences).reshape(1, -1)
        out = self.predict_batch(sequences)[0]
        if item_ids is None:
            return out.cpu().numpy()
        item_ids = np.asarray(item_ids).reshape(-1).astype(np.int64)
        self._check_input(item_ids)
        return out[torch.from_numpy(item_ids).to(out.device)].cpu().numpy()

    def recommend_next(self, sequences, k=10, exclude_preceding=True):
        """The k best next items of each sequence, int64 [n, k] on the host, best first (equal
        scores: lower id first).  The padding id 0 is never returned, nor, with
        ``exclude_preceding``, an item of the sequence itself."""
        from ...implicit import _topk_block
        sequences, seq_dev = self._sequences_dev(sequences)
        n, L = sequences.shape
        room = self._num_items - 1 - (L if exclude_preceding else 0)
        if not 1 <= k <= min(_lib.RG_TOPK_WIDE_MAX, max(room, 0)):
            raise ValueError(f"k must be in [1, {min(_lib.RG_TOPK_WIDE_MAX, max(room, 0))}] for these sequences")
        out = np.empty((n, k), dtype=np.int64)
        for i in range(0, n, SERVE_BLOCK):
            blk = self._scores(seq_dev[i:i + SERVE_BLOCK])
            blk[:, PADDING_IDX] = float("-inf")
            if exclude_preceding and L:
                blk.scatter_(1, seq_dev[i:i + SERVE_BLOCK], float("-inf"))
            out[i:i + SERVE_BLOCK] = _topk_block(blk, k)[1]
        return out

    def rank_next(self, sequences, targets, exclude_preceding=False):
        """The rank (1 = best, ties averaged: scipy rankdata of -score) of ``targets[r]`` among all
        items as the next item of sequence r, float64 [n] on the host; with ``exclude_preceding``
        the sequence's own ids (the padding id among them when it is padded) rank last, as the
        reference's FLOAT_MAX does.  Counted on the device (rg_rank_rows)."""
        sequences, seq_dev = self._sequences_dev(sequences)
        n, L = sequences.shape
        targets = np.asarray(targets).reshape(-1).astype(np.int64)
        if len(targets) != n:
            raise ValueError("one target per sequence")
        self._check_input(targets)
        dev = self._E.device
        lib = _lib.load()
        ranks = np.empty(n, dtype=np.float64)
        tgt = torch.from_numpy(targets.astype(np.int32)).to(dev)
        exc = seq_dev.to(torch.int32) if exclude_preceding and L else None
        for i in range(0, n, SERVE_BLOCK):
            blk = self._scores(seq_dev[i:i + SERVE_BLOCK])
            m = int(blk.shape[0])
            tp = torch.arange(m + 1, dtype=torch.int64, device=dev)
            ti = tgt[i:i + m].contiguous()
            ep = ei = None
            if exc is not None:
                ep, ei = tp * L, exc[i:i + m].contiguous().reshape(-1)
            counts = torch.empty(2, m, dtype=torch.int32, device=dev)
            _lib.check(lib.rg_rank_rows(_lib.stream_handle(), _lib.ptr(blk), m, self._num_items, self._num_items,
                                        _lib.ptr(tp), _lib.ptr(ti), _lib.ptr(ep), _lib.ptr(ei), _lib.ptr(counts[0]),
                                        _lib.ptr(counts[1])), "rg_rank_rows")
            above, equal = counts.cpu().numpy().astype(np.float64)
            ranks[i:i + m] = above + (equal + 1.0) / 2.0
        return ranks
