"""ImplicitFactorizationModel -- drop-in for the reference's implicit.py:31-471.

Same constructor arguments, attributes, ``fit(train_set, valid_set, verbose)``,
``run_train_iteration`` / ``run_val_iteration``, ``predict``, ``test`` and output
files (``experiments_results/<name>/result_outputs/{configuration.json,
summary.csv, test_summary.json}``, ``saved_models/best_model`` =
``torch.save({'network': state_dict})``).  Training of a BilinearNet runs
through the fused MI355X step (``mf_engine.MFEngine`` over librg_hip.so); there
is no CPU training path.

Semantics kept from the reference:
* ``loss``: 'pointwise' -> pointwise, 'hinge' -> hinge, anything else of the
  allowed names ('bpr', 'adaptive_hinge') -> adaptive hinge (implicit.py:194-199);
  the build's pairwise BPR is the additive name 'pairwise_bpr';
* negatives: ``random.choices(neg_examples, k=num_negative_samples * batch_size)``
  from the module-level ``random`` stream (implicit.py:352), shared by training and
  validation; the device stream starts at ``random.getstate()`` and is written
  back with ``random.setstate`` after ``fit``;
* one shuffle with the model's RandomState before the epochs (implicit.py:262),
  ``set_seed(random_state.randint(-1e8, 1e8))`` at construction (:146);
* the optimizer is what ``optimizer_func(params, weight_decay=l2, lr=lr)`` builds
  (Adam when None), applied densely to every row every step;
* best-by-validation-loss model, degenerate-loss ValueError, id-range ValueErrors.
"""
import copy
import json
import logging
import os
import random

import numpy as np
import torch

from . import _mtstate
from . import als
from . import mf_engine
from .mf_engine import MFEngine
from .ncf_engine import NCFEngine
from .spotlight.factorization.representations import BilinearNet
from .spotlight.optimizers import describe
from .spotlight.sampling import NegativePool
from .spotlight.torch_utils import set_seed, shuffle
from .spotlight import evaluation
from .spotlight import losses
from .utils.storage_utils import save_statistics

logging.basicConfig(format="%(message)s", level=logging.INFO)

_LOSS_MAP = {"pointwise": "pointwise", "hinge": "hinge", "bpr": "adaptive_hinge",
             "adaptive_hinge": "adaptive_hinge", "pairwise_bpr": "bpr"}


def _csr_rows(csr, rows):
    """The CSR slice of ``rows`` (in that order, each row's indices as stored): (indptr int64
    [len(rows) + 1], indices int32)."""
    lo = csr.indptr[rows].astype(np.int64)
    n = csr.indptr[rows + 1].astype(np.int64) - lo
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(n, out=ptr[1:])
    pos = np.arange(ptr[-1], dtype=np.int64) + np.repeat(lo - ptr[:-1], n)
    return ptr, csr.indices[pos].astype(np.int32)


def _csr_rows_sorted(csr, rows):
    """``_csr_rows`` with each row's ids ascending, as rg_mf_topk_users wants them.  A matrix that
    says its indices are sorted (``has_sorted_indices``: scipy checks on first use, a flag set by
    hand is trusted) is not sorted again; a row that is not ascending after all can only lose
    exclusions -- a wrong ranking, never an access outside the tables."""
    ptr, idx = _csr_rows(csr, rows)
    if not csr.has_sorted_indices:
        idx = idx[np.lexsort((idx, np.repeat(np.arange(len(rows)), np.diff(ptr))))]
    return ptr, idx


def _score_block(model, users):
    """(ids as a host int64 array, their contiguous fp32 score block on the device): what the
    device rankings (topk_users, rank_users) read.  A function, not a method: it reads only
    ``_engine.device`` and ``_device_scores``, so the rankings also work bound to a stand-in
    that holds just the tables (bench.eval_model)."""
    ub = np.asarray(users, dtype=np.int64)
    u = torch.as_tensor(ub, device=model._engine.device)
    return ub, model._device_scores(u).to(torch.float32).contiguous()


def _exclude_csr_rows(blk, csr, rows):
    """-inf into the score block ``blk`` (len(rows), num_items) at the entries of ``csr``'s ``rows``
    (in that order); ``csr`` None: nothing."""
    if csr is None:
        return
    sub = csr[rows]
    if sub.nnz:
        r = np.repeat(np.arange(len(rows)), np.diff(sub.indptr))
        blk[torch.as_tensor(r, device=blk.device),
            torch.as_tensor(sub.indices.astype(np.int64), device=blk.device)] = float("-inf")


def _topk_block(blk, k, host=True):
    """The k best column ids of a contiguous fp32 score block's rows as (int32 [rows, k] on the
    device, the same on the host), range-checked before anything is indexed with them:
    rg_topk_rows for k <= 32, rg_topk_rows_wide (radix select, the same order) for
    32 < k <= 1024.  ``host=False``: the range is checked on the device, one flag comes down
    and the second element is None."""
    from . import _lib
    n, cols = blk.shape
    out = torch.empty(n, k, dtype=torch.int32, device=blk.device)
    if k <= 32:
        name = "rg_topk_rows"
        rc = _lib.load().rg_topk_rows(_lib.stream_handle(), _lib.ptr(blk), n, cols, cols, int(k), _lib.ptr(out))
    else:
        name = "rg_topk_rows_wide"
        rc = _lib.load().rg_topk_rows_wide(_lib.stream_handle(), _lib.ptr(blk), n, cols, cols, int(k), _lib.ptr(out),
                                           None)
    _lib.check(rc, name)
    if not host:
        if out.numel() and bool((out.min() < 0) | (out.max() >= cols)):
            raise RuntimeError(f"{name} returned an item id outside the table")
        return out, None
    got = out.cpu().numpy()
    if got.size and (got.min() < 0 or got.max() >= cols):
        raise RuntimeError(f"{name} returned an item id outside the table")
    return out, got


def _histories_csr(histories, num_items):
    """New users' histories as a CSR over item ids, (indptr int64 [n + 1], indices int32): a scipy
    sparse matrix or an Interactions with ``num_items`` columns (its rows, indices as stored), or a
    list of id sequences (each in the order given, duplicates kept).  ValueError for another width or
    an id outside [0, num_items)."""
    if hasattr(histories, "tocsr"):
        csr = histories.tocsr()
        if csr.shape[1] != num_items:
            raise ValueError(f"histories have {csr.shape[1]} columns, the model {num_items} items")
        ptr, idx = csr.indptr.astype(np.int64), csr.indices.astype(np.int64)
    else:
        rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in histories]
        ptr = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rows], out=ptr[1:])
        idx = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    if len(idx) and (idx.min() < 0 or idx.max() >= num_items):
        raise ValueError("history item id outside [0, num_items)")
    return ptr, idx.astype(np.int32)


def _candidate_lists(candidates, n, num_items):
    """Candidate lists as a CSR over item ids, (indptr int64 [n + 1], indices int32): a scipy sparse
    matrix with ``num_items`` columns (its rows, indices as stored), an ``(n, C)`` integer array, or a
    list of id sequences (each in the order given, repeats kept).  ValueError for another number of
    lists than ``n`` users, another width, ids that are not integers or an id outside [0, num_items)."""
    if hasattr(candidates, "tocsr"):
        csr = candidates.tocsr()
        if csr.shape[1] != num_items:
            raise ValueError(f"candidates have {csr.shape[1]} columns, the model {num_items} items")
        rows, ptr, idx = csr.shape[0], csr.indptr.astype(np.int64), csr.indices.astype(np.int64)
    elif isinstance(candidates, np.ndarray) and candidates.ndim == 2:
        if candidates.dtype.kind not in "iu":
            raise ValueError("candidates must hold integer item ids")
        rows = candidates.shape[0]
        ptr = np.arange(rows + 1, dtype=np.int64) * candidates.shape[1]
        idx = candidates.astype(np.int64).reshape(-1)
    else:
        lists = [np.asarray(r).reshape(-1) for r in candidates]
        if any(len(r) and r.dtype.kind not in "iu" for r in lists):
            raise ValueError("candidates must hold integer item ids")
        rows = len(lists)
        ptr = np.zeros(rows + 1, dtype=np.int64)
        np.cumsum([len(r) for r in lists], out=ptr[1:])
        idx = np.concatenate(lists).astype(np.int64) if ptr[-1] else np.zeros(0, dtype=np.int64)
    if rows != n:
        raise ValueError(f"{rows} candidate lists for {n} users")
    if len(idx) and (idx.min() < 0 or idx.max() >= num_items):
        raise ValueError("candidate item id outside [0, num_items)")
    return ptr, idx.astype(np.int32)


def _fold_negatives(nnz, n_neg, num_items, random_state, device=None):
    """The fold-in's negatives, drawn once: ``random_state.randint(0, num_items, nnz * n_neg)`` --
    uniform over the items, so one may coincide with a positive, as in the reference -- through the
    device sampler (``sample_items(..., device=)``: NumPy's values, the RandomState advanced as NumPy
    advances it); entry e's negative j is element e * n_neg + j."""
    from .spotlight.sampling import sample_items
    return sample_items(None, None, num_items, (int(nnz) * int(n_neg),), random_state=random_state, device=device)


def _score_block_fits(n, num_items, device):
    """Whether recommend may build the (n, num_items) fp32 score block: twice its size within the
    device's free memory (the driver's free bytes plus what torch's allocator holds unused).  The
    factor 2 is a guess at what the block path allocates beside the block (the scatter's int64 index
    lists, the int64 copy of the ids, the gathered scores); its true peak at large catalogues has
    not been measured."""
    free, _ = torch.cuda.mem_get_info(device)
    free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    return 2 * 4 * n * num_items <= free


class ImplicitFactorizationModel:
    def __init__(self, loss="pointwise", embedding_dim=32, n_iter=10, batch_size=256, l2=0.0,
                 experiment_name="Implicit_Feedback", learning_rate=1e-2, optimizer_func=None, use_cuda=False,
                 representation=None, sparse=False, model_name="mf", random_state=None, neg_examples=None,
                 num_negative_samples=3, world_size=1):
        self.exeriment_name = experiment_name
        self.experiment_folder = os.path.abspath("experiments_results/" + experiment_name)
        self.experiment_logs = os.path.join(self.experiment_folder, "result_outputs")
        self.experiment_saved_models = os.path.join(self.experiment_folder, "saved_models")
        self.starting_epoch = 0
        for d in (self.experiment_logs, self.experiment_saved_models):
            os.makedirs(d, exist_ok=True)
        assert loss in _LOSS_MAP, loss
        self._loss = loss
        self._embedding_dim = embedding_dim
        self._n_iter = n_iter
        self._learning_rate = learning_rate
        self._batch_size = batch_size
        self._l2 = l2
        self._use_cuda = use_cuda
        self._representation = representation
        self._sparse = sparse
        self._optimizer_func = optimizer_func
        self._random_state = random_state or np.random.RandomState()
        self._num_negative_samples = num_negative_samples
        self.neg_examples = neg_examples
        self._num_users = None
        self._num_items = None
        self._net = None
        self._engine = None
        self.best_model = None
        self.best_validation = None
        self.model_name = model_name
        self.best_epoch = -1
        self.als_losses = None         # fit_als: the objective after every sweep
        self._als = None               # fit_als: (regularization, alpha, cg_steps), fold_in_users_als' defaults
        # additive: data-parallel training over world_size processes (one per GPU, under
        # torchrun, torch.distributed initialised by the caller before any GPU work); the
        # reference's single process at batch world_size * batch_size, reproduced by the
        # owner-sharded layout (mf_engine.MFEngine dp="owner")
        self._world = int(world_size)
        self._rank = 0
        self._full_tables = None
        if self._world > 1:
            import torch.distributed as dist
            if not dist.is_initialized() or dist.get_world_size() != self._world:
                raise RuntimeError("world_size > 1 needs torch.distributed initialised with that many ranks "
                                   "(torchrun; mf_spotlight.py --world_size)")
            self._rank = dist.get_rank()
        set_seed(self._random_state.randint(-10 ** 8, 10 ** 8), cuda=self._use_cuda)

    def __repr__(self):
        return "<ImplicitFactorizationModel: {}>".format(
            "uninitialised" if self._net is None else f"{self._num_users} users x {self._num_items} items, "
                                                      f"d={self._embedding_dim}, loss={self._loss}")

    @property
    def _initialized(self):
        return self._net is not None

    # ------------------------------------------------------------------ setup
    def _device(self):
        if not self._use_cuda:
            raise RuntimeError("this implementation trains on the GPU only (librg_hip.so): pass use_cuda=True")
        return torch.device("cuda", torch.cuda.current_device())

    def _initialize(self, interactions):
        self._num_users, self._num_items = interactions.num_users, interactions.num_items
        dev = self._device()
        net = self._representation
        if net is None:
            net = BilinearNet(self._num_users, self._num_items, self._embedding_dim, sparse=self._sparse)
        self._net = net.to(dev)
        self._opt = describe(self._optimizer_func, self._learning_rate, self._l2)
        # the reference's loss selection (implicit.py:194-199); the fused step computes the same
        # loss in its kernel, this is the function for callers that score pairs themselves
        self._loss_func = losses.bpr_loss if self._loss == "pairwise_bpr" else losses.loss_for(self._loss)
        # implicit.py:351-360: without a negative pool the loss sees the positives only --
        # self._loss_func(positive_prediction) -- and no draw is taken from `random`
        self._no_negatives = not self.neg_examples
        if self._no_negatives:
            if self._loss != "pointwise":   # the reference's pairwise losses need the negatives argument
                raise TypeError(f"{self._loss_func.__name__}() missing 1 required positional argument: "
                                f"'negative_predictions'")
            if self._world > 1:
                raise NotImplementedError("data-parallel training needs a negative pool")
        self._pool = NegativePool.from_pairs([(0, 0)] if self._no_negatives else self.neg_examples)
        engine_loss = "pointwise_pos" if self._no_negatives else _LOSS_MAP[self._loss]
        o = self._opt
        common = dict(loss=engine_loss, optimizer=o["kind"], lr=o["lr"], weight_decay=o["weight_decay"],
                      betas=o.get("betas", (0.9, 0.999)), eps=o.get("eps", 1e-8), alpha=o.get("alpha", 0.99),
                      n_neg=self._num_negative_samples, batch_size=self._batch_size, device=dev)
        ncf_dp = {}
        if self._world > 1:
            import torch.distributed as dist
            comm = None
            if dist.get_backend() == "nccl":           # RCCL: the exchanges run inside the native step
                from .comm import RcclComm
                comm = RcclComm(dev)
            ncf_dp = dict(rank=self._rank, world_size=self._world, comm=comm)
        is_mf = hasattr(net, "user_embeddings") and hasattr(net, "item_biases")
        if self._no_negatives and not is_mf:   # before any engine (and its device state) is built
            raise NotImplementedError("training without a negative pool is implemented for BilinearNet")
        if hasattr(net, "embedding_user_mlp") and hasattr(net, "affine_output"):   # NeuMF (neuMF.py:7-55)
            self._kind = "ncf"
            self._params = [net.embedding_user_mlp.weight, net.embedding_item_mlp.weight,
                            net.embedding_user_mf.weight, net.embedding_item_mf.weight]
            for lin in [m_ for m_ in net.layers if isinstance(m_, torch.nn.Linear)] + [net.affine_output]:
                self._params += [lin.weight, lin.bias]
            self._embedding_dim = net.embedding_user_mlp.weight.shape[1]
            w = [p.detach() for p in self._params]
            self._engine = NCFEngine(w[0], w[1], w[4:], self._pool.user_ids, self._pool.item_ids, _mtstate.current(),
                                     seed=int(torch.randint(0, 2 ** 31 - 1, (1,)).item()), mf_user_w=w[2],
                                     mf_item_w=w[3], **common, **ncf_dp)
        elif hasattr(net, "embedding_user") and hasattr(net, "layers"):          # NCF MLP (mlp.py:5-46)
            self._kind = "ncf"
            self._params = [net.embedding_user.weight, net.embedding_item.weight]
            for lin in [m_ for m_ in net.layers if isinstance(m_, torch.nn.Linear)]:
                self._params += [lin.weight, lin.bias]
            self._embedding_dim = net.embedding_user.weight.shape[1]
            self._engine = NCFEngine(self._params[0].detach(), self._params[1].detach(),
                                     [p.detach() for p in self._params[2:]], self._pool.user_ids,
                                     self._pool.item_ids, _mtstate.current(),
                                     seed=int(torch.randint(0, 2 ** 31 - 1, (1,)).item()), **common, **ncf_dp)
        elif hasattr(net, "user_embeddings") and hasattr(net, "item_biases"):   # BilinearNet
            self._kind = "mf"
            self._params = [net.user_embeddings.weight, net.item_embeddings.weight, net.user_biases.weight,
                            net.item_biases.weight]
            self._embedding_dim = net.user_embeddings.weight.shape[1]
            w = [p.detach() for p in self._params]
            dp = {}
            if self._world > 1:
                dp = dict(rank=self._rank, world_size=self._world, dp="owner", comm=ncf_dp["comm"])
            self._engine = MFEngine(w[0], w[1], w[2].reshape(-1), w[3].reshape(-1), self._pool.user_ids,
                                    self._pool.item_ids, _mtstate.current(), **common, **dp)
        else:
            raise NotImplementedError("the fused steps train BilinearNet, the NCF MLP and NeuMF representations")
        self.configuration = {"num_users": self._num_users, "num_items": self._num_items,
                              "weight_decay": self._l2, "lr": self._learning_rate,
                              "embedding_dim": self._embedding_dim, "batch_size": self._batch_size,
                              "epochs": self._n_iter}
        if self._rank == 0:            # one writer per experiment folder in a data-parallel fit
            with open(os.path.join(self.experiment_logs, "configuration.json"), "w") as fp:
                json.dump(self.configuration, fp)

    def _check_input(self, user_ids, item_ids, allow_items_none=False):
        user_id_max = user_ids if isinstance(user_ids, int) else user_ids.max()
        if user_id_max >= self._num_users:
            raise ValueError("Maximum user id greater than number of users in model.")
        if allow_items_none and item_ids is None:
            return
        item_id_max = item_ids if isinstance(item_ids, int) else item_ids.max()
        if item_id_max >= self._num_items:
            raise ValueError("Maximum item id greater than number of items in model.")

    # ------------------------------------------------------------------ training
    def fit(self, train_set, valid_set, verbose=False):
        self.train_set = train_set
        users, items = shuffle(train_set.user_ids, train_set.item_ids, random_state=self._random_state)
        if not self._initialized:
            self._initialize(train_set)
        self._check_input(train_set.user_ids, train_set.item_ids)
        e, dev = self._engine, self._engine.device
        b = self._batch_size
        B = b * self._world                        # the global batch (one process at world * batch_size)
        R, r = self._world, self._rank
        owner = R > 1 and self._kind == "mf"       # MF: owner-sharded; NCF / NeuMF: replicated columns
        allreduce = None
        if R > 1 and e.comm is None:               # gloo process group: exchanges through torch.distributed
            import torch.distributed as dist
            allreduce = dist.all_reduce
        e.set_mt_state(_mtstate.current())
        tu = torch.from_numpy(np.ascontiguousarray(users, dtype=np.int64)).to(dev)
        ti = torch.from_numpy(np.ascontiguousarray(items, dtype=np.int64)).to(dev)
        vu = torch.from_numpy(np.ascontiguousarray(valid_set.user_ids, dtype=np.int64)).to(dev)
        vi = torch.from_numpy(np.ascontiguousarray(valid_set.item_ids, dtype=np.int64)).to(dev)
        nb = (len(tu) + B - 1) // B
        losses = torch.zeros(nb, dtype=torch.float32, device=dev)
        total = {"train_loss": [], "validation_loss": [], "curr_epoch": []}
        # the batches repeat every epoch (one shuffle): plans (and MF step inputs) are built once
        # (one launch builds every batch's plan, rg_mf_plans_build)
        if owner:
            plans = e.make_plans(ti, users=tu)
        elif R > 1:                                # this rank's columns [r*b, (r+1)*b) of each global batch
            plans = e.make_plans(ti, offset=r * b, stride=B, n_batches=nb)
        else:
            plans = e.make_plans(ti)
        vplans = e.make_plans(vi, users=vu) if owner else None

        def cols(x, s):                            # this rank's columns of global batch s (NCF / NeuMF)
            lo = min(s * B + r * b, len(x))
            return x[lo:min(lo + b, (s + 1) * B, len(x))]
        if self._kind == "mf":
            inputs = [e.step_input(tu[s * B:(s + 1) * B], ti[s * B:(s + 1) * B], None, plans[s]) for s in range(nb)]
        for epoch in range(self._n_iter):
            for s in range(nb):
                nxt = inputs[s + 1] if self._kind == "mf" and s + 1 < nb else None
                if self._kind == "mf" and allreduce is not None:
                    e.train_step_owner_exchange(inputs[s], nxt, allreduce, loss_out=losses[s:s + 1])
                elif self._kind == "mf":
                    e.train_step_in(inputs[s], nxt, loss_out=losses[s:s + 1])
                else:
                    nxt = (cols(tu, s + 1), cols(ti, s + 1), plans[s + 1]) if s + 1 < nb else None
                    e.train_step(cols(tu, s), cols(ti, s), global_pos=min(B, len(tu) - s * B), plan=plans[s],
                                 loss_out=losses[s:s + 1], next_step=nxt, allreduce=allreduce)
            tl = [float(x) for x in losses.cpu().numpy()]          # loss.item() per batch
            train_epoch_loss = sum(tl) / nb
            if np.isnan(train_epoch_loss) or train_epoch_loss == 0.0:
                raise ValueError("Degenerate epoch loss: {}".format(train_epoch_loss))
            if owner:
                vl = [float(e.val_loss(vu[s:s + B], vi[s:s + B], plan=vplans[s // B], allreduce=allreduce)[0])
                      for s in range(0, len(vu), B)]
            elif R > 1:
                vl = [float(e.val_loss(cols(vu, s), cols(vi, s), global_pos=min(B, len(vu) - s * B),
                                       allreduce=allreduce)[0]) for s in range(-(-len(vu) // B))]
            else:
                vl = [float(e.val_loss(vu[s:s + B], vi[s:s + B])[0]) for s in range(0, len(vu), B)]
            valid_epoch_loss = sum(vl) / len(vl)
            if self.best_validation is None or valid_epoch_loss < self.best_validation:
                self.best_model = [t.detach().clone() for t in e.params()]
                self.best_validation = valid_epoch_loss
                self.best_epoch = epoch
            if verbose:
                logging.info("Epoch {}: training_loss {:10.5f}".format(epoch, train_epoch_loss))
                logging.info("Epoch {}: validation_loss {:10.5f}".format(epoch, valid_epoch_loss))
            total["train_loss"].append(np.mean(tl))
            total["validation_loss"].append(np.mean(vl))
            total["curr_epoch"].append(epoch)
            if self._rank == 0:
                save_statistics(experiment_log_dir=self.experiment_logs, filename="summary.csv", stats_dict=total,
                                current_epoch=epoch, continue_from_mode=(self.starting_epoch != 0 or epoch > 0))
        if not self._no_negatives:                     # the Python stream continues after fit
            _mtstate.restore(e.mt_state())
        if self._kind == "mf":
            e.set_params(*self.best_model)
        else:
            e.set_params(self.best_model)
        if owner:                                      # every rank gets the full best tables
            self.best_model = self._gather_tables(self.best_model)
            self._full_tables = [t.to(dev) for t in self.best_model]
        self._load_into_net(self.best_model)
        if self._rank == 0:
            self.save_readable_model(self.experiment_saved_models, self._net.state_dict())
        logging.info("Model chosen from epoch %d", self.best_epoch)

    def _gather_tables(self, local):
        """Full (user_w, item_w, user_b, item_b) from every rank's user rows (u % R == rank,
        local row u // R) and the replicated items."""
        import torch.distributed as dist
        from . import sharding
        mine = [t.detach().cpu().numpy() for t in local]
        shards = [None] * self._world
        dist.all_gather_object(shards, mine[0::2])     # user rows and user biases
        uw = sharding.unshard_rows([x[0] for x in shards], self._num_users)
        ub = sharding.unshard_rows([x[1] for x in shards], self._num_users)
        return [torch.from_numpy(uw), torch.from_numpy(mine[1]).clone(), torch.from_numpy(ub),
                torch.from_numpy(mine[3]).clone()]

    def _tables(self):
        """The MF tables the evaluation reads: the engine's, or after a data-parallel fit
        (the engine then holds this rank's users only) the gathered full tables."""
        return self._full_tables if self._full_tables is not None else self._engine.params()

    def _load_into_net(self, tables):
        with torch.no_grad():
            for p, t in zip(self._params, tables):
                p.copy_(t.reshape(p.shape))

    def run_train_iteration(self, batch_user, batch_item):
        """One fused step on this batch (implicit.py:347-364); returns the loss (device, shape (1,))."""
        e = self._engine
        return e.train_step(batch_user.to(e.device, torch.int64).contiguous(),
                            batch_item.to(e.device, torch.int64).contiguous())

    def run_val_iteration(self, batch_user, batch_item):
        e = self._engine
        return e.val_loss(batch_user.to(e.device, torch.int64).contiguous(),
                          batch_item.to(e.device, torch.int64).contiguous())

    # ------------------------------------------------------------------ inference
    def predict(self, user_ids, item_ids=None):
        self._check_input(user_ids, item_ids, allow_items_none=True)
        if item_ids is None and self._kind != "mf" and np.ndim(user_ids) == 0:
            # one user against every item: the all-item kernel with a block of one user
            if int(user_ids) < 0:
                raise ValueError("user id must be non-negative")
            return self._engine.score_users(np.array([int(user_ids)], dtype=np.int64)).cpu().numpy().flatten()
        if item_ids is None:
            item_ids = np.arange(self._num_items, dtype=np.int64)
        if np.isscalar(user_ids):
            user_ids = np.array(user_ids, dtype=np.int64)
        u = torch.from_numpy(np.asarray(user_ids, dtype=np.int64).reshape(-1))
        i = torch.from_numpy(np.asarray(item_ids, dtype=np.int64).reshape(-1))
        if u.numel() != i.numel():
            u = u.expand(i.numel())
        if self._kind == "mf" and self._full_tables is not None:
            from . import _lib
            dev = self._engine.device
            U, I, ub, ib = self._full_tables
            u, i = u.to(dev).contiguous(), i.to(dev).contiguous()
            out = torch.empty(u.numel(), dtype=torch.float32, device=dev)
            lib = _lib.load()
            _lib.check(lib.rg_mf_scores(_lib.stream_handle(), _lib.ptr(U), _lib.ptr(I), _lib.ptr(ub), _lib.ptr(ib),
                                        U.shape[1], _lib.ptr(u), _lib.ptr(i), u.numel(), _lib.ptr(out)),
                       "rg_mf_scores")
            return out.cpu().numpy().flatten()
        return self._engine.scores(u, i).detach().cpu().numpy().flatten()

    def _device_scores(self, u):
        """(len(u), num_items) fp32 scores on the device: the fused MF block (rg_mf_score_users;
        tables that are not contiguous float32 on a CUDA device keep the chain of torch ops), or
        the eval-mode MLP / NeuMF block of the fused all-item kernel (rg_ncf_score_users)."""
        if self._kind == "mf":
            U, I, ub, ib = self._tables()
            if mf_engine.score_block_on_device(U, I, ub, ib):
                return mf_engine.score_users_block(U, I, ub, ib, u)
            return torch.sigmoid(U[u] @ I.T + ub[u][:, None] + ib[None, :])
        return self._engine.score_users(u)

    def score_users(self, users):
        """Scores of every item for a block of users, (len(users), num_items) float32 on
        the host (evaluation helper)."""
        u = torch.as_tensor(np.asarray(users, dtype=np.int64), device=self._engine.device)
        return self._device_scores(u).cpu().numpy()

    # the largest k of topk_users (rg_topk_rows_wide); spotlight/evaluation.py routes its @k metrics by it
    topk_users_max = 1024

    def topk_users(self, users, k, exclude_csr=None):
        """The first k entries of argsort(-scores) for a block of users (evaluation.py:
        precision/recall@k, hit ratio, MAP@k), ranked on the device by rg_topk_rows, for
        32 < k <= min(1024, num_items) by rg_topk_rows_wide (``_topk_block``); items of
        ``exclude_csr``'s rows rank last (the reference's FLOAT_MAX).  Returns
        (len(users), k) int64 on the host."""
        ub, s = _score_block(self, users)
        _exclude_csr_rows(s, exclude_csr, ub)
        return _topk_block(s, k)[1].astype(np.int64)

    def recommend(self, user_ids, k=10, exclude=None, return_scores=False):
        """The k best items for each of ``user_ids``: ``(len(user_ids), k)`` int64 item ids on the
        host in rank order (higher score first, then the lower item id), with ``return_scores`` also
        their float32 scores.  ``exclude``: an Interactions or a scipy sparse matrix of the model's
        shape (typically the train set) whose items are left out per user; they have the score -inf
        and are only returned, by id, to a user with fewer than k items left.

        Works for every model the class trains (MF, NCF, NeuMF) and any number of users, 4096 at a
        time: the score block on the device (``_device_scores``), -inf over the excluded entries,
        rg_topk_rows, and the scores gathered from the block at the returned ids.  An MF block whose
        score block does not fit the device's free memory (``_score_block_fits``) goes through the
        fused kernel instead (rg_mf_topk_users, ``mf_engine.topk_users_fused``): it scores, excludes
        and ranks in LDS, no (users, items) block exists, and only the block's exclusion rows (ids
        sorted per row) go up.  Measured at 4096 users x 26,744 items the block path is the faster
        one (README), so it is kept wherever it fits.  Both give the same ids and score bits; only
        ids and scores come down.  After a data-parallel fit the gathered full tables are used, as
        in ``predict``.  ValueError for an id outside the model, k < 1, k > min(32, num_items) or an
        ``exclude`` of another shape.  The cap stays 32 here (the fused kernel's lists hold no more);
        ``topk_users`` ranks up to 1024 ids."""
        users = np.asarray(user_ids, dtype=np.int64).reshape(-1)
        k, n, num_items = int(k), len(users), self._num_items
        if k < 1 or k > min(32, num_items):
            raise ValueError("k must be in [1, min(32, num_items)]")
        if n and (users.min() < 0 or users.max() >= self._num_users):
            raise ValueError("user id outside [0, num_users)")
        csr = None
        if exclude is not None:
            csr = exclude.tocsr()
            if csr.shape != (self._num_users, num_items):
                raise ValueError(f"exclude has shape {csr.shape}, the model {(self._num_users, num_items)}")
        ids = np.empty((n, k), dtype=np.int64)
        scores = np.empty((n, k), dtype=np.float32)
        if n == 0:
            return (ids, scores) if return_scores else ids
        dev = self._engine.device
        tables = self._tables() if self._kind == "mf" else None
        # asked once per call, for the largest block: the kernel where that block does not fit
        fused = tables is not None and mf_engine.score_block_on_device(*tables) and \
            not _score_block_fits(min(n, 4096), num_items, dev)
        for s in range(0, n, 4096):
            ub = users[s:s + 4096]
            if fused:
                e_ptr, e_idx = _csr_rows_sorted(csr, ub) if csr is not None else (None, None)
                out, sc = mf_engine.topk_users_fused(*tables, ub, k, e_ptr, e_idx, checked=True)
                got = out.cpu().numpy()
                if got.min() < 0 or got.max() >= num_items:     # before the ids are used for anything
                    raise RuntimeError("rg_mf_topk_users returned an item id outside the table")
                ids[s:s + len(ub)] = got
                if return_scores:
                    scores[s:s + len(ub)] = sc.cpu().numpy()
                continue
            ub, blk = _score_block(self, users[s:s + 4096])
            _exclude_csr_rows(blk, csr, ub)
            out, got = _topk_block(blk, k)                      # checked: never index the block with a bad id
            ids[s:s + len(ub)] = got
            if return_scores:
                scores[s:s + len(ub)] = torch.gather(blk, 1, out.to(torch.int64)).cpu().numpy()
        return (ids, scores) if return_scores else ids

    def _candidate_blocks(self, user_ids, candidates, what):
        """The checks ``score_candidates`` and ``rank_candidates`` share, then per block of 4096 users
        (first user, last, ptr and idx on the device with ptr starting at 0, the entries' scores on the
        device).  MF scores through ``candidates.score_lists`` on ``_tables()`` (the gathered full
        tables after a data-parallel fit), NCF / NeuMF through ``NCFEngine.scores`` -- the pair kernel
        behind ``predict`` -- with the users repeated per entry on the device."""
        from . import candidates as cand
        if not self._initialized:
            raise RuntimeError(f"{what} needs a fitted model")
        users = np.asarray(user_ids, dtype=np.int64).reshape(-1)
        n = len(users)
        if n and (users.min() < 0 or users.max() >= self._num_users):
            raise ValueError("user id outside [0, num_users)")
        ptr, idx = _candidate_lists(candidates, n, self._num_items)
        dev = self._engine.device

        def blocks():
            for s in range(0, n, 4096):
                e = min(s + 4096, n)
                p = torch.as_tensor(ptr[s:e + 1] - ptr[s], device=dev)
                i = torch.as_tensor(idx[ptr[s]:ptr[e]], device=dev)
                u = torch.as_tensor(users[s:e], device=dev)
                if self._kind == "mf":
                    U, I, ub, ib = self._tables()
                    sc = cand.score_lists(U.contiguous(), I.contiguous(), ub.reshape(-1).contiguous(),
                                          ib.reshape(-1).contiguous(), u, p, i, checked=True)
                else:
                    sc = self._engine.scores(torch.repeat_interleave(u, p[1:] - p[:-1]), i.to(torch.int64))
                yield s, e, p, i, sc
        return n, ptr, blocks()

    def score_candidates(self, user_ids, candidates):
        """The scores of a list of candidate items per user: a flat float32 host array in list order
        (user 0's candidates first).  ``candidates``: a list of item-id sequences (one per user, any
        lengths, repeats allowed), an ``(n, C)`` integer array, or a scipy sparse matrix with
        ``num_items`` columns (its rows' indices as stored).  Only the lists go up and the scores come
        down, 4096 users at a time: MF through rg_mf_score_lists (``candidates.score_lists``: no
        (users, items) block), NCF / NeuMF through the pair kernel behind ``predict``, whose bits
        these are.  ValueError for an id outside the model or a number of lists other than
        ``len(user_ids)``."""
        n, ptr, blocks = self._candidate_blocks(user_ids, candidates, "score_candidates")
        out = np.empty(int(ptr[-1]), dtype=np.float32)
        for s, e, _, _, sc in blocks:
            out[ptr[s]:ptr[e]] = sc.cpu().numpy()
        return out

    def rank_candidates(self, user_ids, candidates, k=10, return_scores=False):
        """The k best of each user's candidate items (re-ranking): ``(len(user_ids), k)`` int64 item ids
        on the host in rank order -- higher score first, then the lower item id; an id listed twice
        may be returned twice -- with -1 where a list has fewer than k entries, and with
        ``return_scores`` also their float32 scores (-inf there).  ``candidates`` as in
        ``score_candidates``, whose scores these rank: scored on the device, then rg_seg_topk
        (``candidates.seg_topk``) inside each list; only ids and scores come down.  ValueError for an
        id outside the model, k outside [1, 32] or a number of lists other than ``len(user_ids)``."""
        from . import candidates as cand
        if int(k) != k or k < 1 or k > cand.SEG_TOPK_MAX:
            raise ValueError(f"k must be in [1, {cand.SEG_TOPK_MAX}]")
        k = int(k)
        n, ptr, blocks = self._candidate_blocks(user_ids, candidates, "rank_candidates")
        ids = np.full((n, k), -1, dtype=np.int64)
        scores = np.full((n, k), -np.inf, dtype=np.float32)
        for s, e, p, i, sc in blocks:
            if not i.numel():
                continue
            pos, val = cand.seg_topk(sc, p, i, k, return_values=True, checked=True)
            at = (p[:-1, None] + pos.clamp(min=0)).clamp(max=i.numel() - 1)
            ids[s:e] = torch.where(pos >= 0, i[at].to(torch.int64), -1).cpu().numpy()
            if return_scores:
                scores[s:e] = val.cpu().numpy()
        return (ids, scores) if return_scores else ids

    def candidate_target_ranks(self, user_ids, candidates):
        """Where the FIRST entry of each user's candidate list (the target) stands among the rest, as
        ``evaluation.sampled_hit_ndcg`` reads it: ``(len(user_ids), 2)`` int64 on the host, the other
        entries with a higher score and those with an equal score and a lower item id, (-1, -1) for
        an empty list.  Scored like ``score_candidates``, counted on the device (rg_seg_rank,
        ``candidates.seg_rank``); two counts per list come down."""
        from . import candidates as cand
        n, ptr, blocks = self._candidate_blocks(user_ids, candidates, "candidate_target_ranks")
        out = np.full((n, 2), -1, dtype=np.int64)
        for s, e, p, i, sc in blocks:
            out[s:e] = cand.seg_rank(sc, p, i, checked=True).cpu().numpy()
        return out

    def _similarity(self, metric, space):
        """(item table, reciprocal norms or None) behind the diversified rankings: ``similar_items``'
        table and metric, the norms computed once per call."""
        table = self._item_table(space).contiguous()
        return table, (mf_engine.row_rnorms(table) if metric == "cosine" else None)

    def diversify_candidates(self, user_ids, candidates, k=10, lam=0.7, metric="cosine", space=None,
                             return_scores=False):
        """``rank_candidates`` with diversity: k of each user's candidate items picked greedily by
        maximal marginal relevance -- the best score first, then at every step the candidate with the
        largest ``lam * score - (1 - lam) * (its largest similarity to an item already picked)``,
        ties to the lower item id, then the lower position.  ``(len(user_ids), k)`` int64 item ids on
        the host in pick order, -1 where a list has fewer than k entries, with ``return_scores`` also
        their float32 scores (the model's, not the objective; -inf there).  ``lam=1`` is
        ``rank_candidates``; a smaller ``lam`` trades relevance for variety.

        ``candidates`` as in ``score_candidates``, whose scores are the relevance (MF, NCF, NeuMF);
        the similarity is ``similar_items``': ``metric`` "cosine" or "dot" over the item table
        ``space`` names (NeuMF: "mf", the default, or "mlp"; MF and NCF: None), the reciprocal norms
        computed once per call.  Scored on the device, then one launch per block of 4096 users
        (rg_seg_mmr, ``candidates.seg_mmr``); only ids and scores come down.  ValueError for an id
        outside the model, k outside [1, 32], lam outside (0, 1], a list of more than 1024
        candidates, a number of lists other than ``len(user_ids)``, an unknown ``metric`` or an
        unknown ``space``."""
        from . import candidates as cand
        what = "diversify_candidates"
        k, lam = cand._mmr_k_lam(k, lam, what)
        self._check_metric(metric)
        n, ptr, blocks = self._candidate_blocks(user_ids, candidates, what)
        if n and np.diff(ptr).max() > cand.SEG_MMR_MAX_LEN:
            raise ValueError(f"{what}: a list is longer than {cand.SEG_MMR_MAX_LEN} entries")
        space = self._check_space(space)
        ids = np.full((n, k), -1, dtype=np.int64)
        scores = np.full((n, k), -np.inf, dtype=np.float32)
        if ptr[-1] == 0:
            return (ids, scores) if return_scores else ids
        table, rnorm = self._similarity(metric, space)
        for s, e, p, i, sc in blocks:
            if not i.numel():
                continue
            pos, val = cand.seg_mmr(sc, p, i, table, k, lam, rnorm=rnorm, return_values=True, checked=True)
            at = (p[:-1, None] + pos.clamp(min=0)).clamp(max=i.numel() - 1)
            ids[s:e] = torch.where(pos >= 0, i[at].to(torch.int64), -1).cpu().numpy()
            if return_scores:
                scores[s:e] = val.cpu().numpy()
        return (ids, scores) if return_scores else ids

    def recommend_diverse(self, user_ids, k=10, pool=100, lam=0.7, exclude=None, metric="cosine", space=None,
                          return_scores=False):
        """``recommend`` with diversity: for each user the ``pool`` best items are retrieved and k of
        them are picked by maximal marginal relevance (``diversify_candidates``' rule over that
        pool).  ``(len(user_ids), k)`` int64 item ids on the host in pick order, with
        ``return_scores`` also their float32 scores.  ``lam=1`` returns ``recommend``'s ids and score
        bits; ``exclude`` as in ``recommend``; ``metric`` and ``space`` as in ``similar_items``.

        4096 users at a time, all on the device: the score block (``_device_scores``), -inf over the
        excluded entries, the pool's ids by ``_topk_block`` (rg_topk_rows, rg_topk_rows_wide beyond
        32), their scores gathered from the block, then rg_seg_mmr over the regular (users, pool)
        lists (``candidates.seg_mmr``); only ids and scores come down.  The block is always built:
        there is no fused path here.  ValueError for an id outside the model, k outside
        [1, min(32, num_items)], pool outside [k, min(1024, num_items)], lam outside (0, 1], an
        ``exclude`` of another shape, an unknown ``metric`` or an unknown ``space``."""
        from . import candidates as cand
        what = "recommend_diverse"
        if not self._initialized:
            raise RuntimeError(f"{what} needs a fitted model")
        users = np.asarray(user_ids, dtype=np.int64).reshape(-1)
        n, num_items = len(users), self._num_items
        if int(k) != k or k < 1 or k > min(cand.SEG_MMR_MAX, num_items):
            raise ValueError(f"k must be in [1, min({cand.SEG_MMR_MAX}, num_items)]")
        k, lam = cand._mmr_k_lam(k, lam, what)
        if int(pool) != pool or pool < k or pool > min(cand.SEG_MMR_MAX_LEN, num_items):
            raise ValueError(f"pool must be in [k, min({cand.SEG_MMR_MAX_LEN}, num_items)]")
        pool = int(pool)
        self._check_metric(metric)
        if n and (users.min() < 0 or users.max() >= self._num_users):
            raise ValueError("user id outside [0, num_users)")
        csr = None
        if exclude is not None:
            csr = exclude.tocsr()
            if csr.shape != (self._num_users, num_items):
                raise ValueError(f"exclude has shape {csr.shape}, the model {(self._num_users, num_items)}")
        space = self._check_space(space)
        ids = np.empty((n, k), dtype=np.int64)
        scores = np.empty((n, k), dtype=np.float32)
        if n == 0:
            return (ids, scores) if return_scores else ids
        table, rnorm = self._similarity(metric, space)
        for s in range(0, n, 4096):
            ub, blk = _score_block(self, users[s:s + 4096])
            _exclude_csr_rows(blk, csr, ub)
            cands = _topk_block(blk, pool, host=False)[0]        # checked: never index the block with a bad id
            sc = torch.gather(blk, 1, cands.to(torch.int64)).reshape(-1)
            p = torch.arange(len(ub) + 1, dtype=torch.int64, device=blk.device) * pool
            pos, val = cand.seg_mmr(sc, p, cands.reshape(-1), table, k, lam, rnorm=rnorm, return_values=True,
                                    checked=True)
            ids[s:s + len(ub)] = torch.gather(cands, 1, pos.to(torch.int64)).cpu().numpy()   # pool >= k: no fill
            if return_scores:
                scores[s:s + len(ub)] = val.cpu().numpy()
        return (ids, scores) if return_scores else ids

    def _fold_in_device(self, histories, steps, lr, n_neg, l2, random_state, return_loss):
        """``fold_in_users`` up to the device results: (indptr, indices, (W, b[, loss]) on the device)."""
        if not self._initialized:
            raise RuntimeError("fold_in_users needs a fitted model")
        if self._kind != "mf":
            raise NotImplementedError("fold-in is implemented for the matrix-factorization model (BilinearNet)")
        ptr, idx = _histories_csr(histories, self._num_items)
        loss = "pointwise" if self._no_negatives else _LOSS_MAP[self._loss]
        if n_neg is None:
            n_neg = 0 if self._no_negatives else self._num_negative_samples
        o = self._opt
        dev = self._engine.device
        rs = random_state if random_state is not None else self._random_state
        neg = _fold_negatives(len(idx), n_neg, self._num_items, rs, dev) if n_neg and len(idx) else None
        _, item_w, _, item_b = self._tables()
        out = mf_engine.fold_in_users(item_w, item_b, ptr, idx, neg, n_neg, loss=loss, steps=steps,
                                      lr=o["lr"] if lr is None else lr,
                                      weight_decay=o["weight_decay"] if l2 is None else l2,
                                      betas=o.get("betas", (0.9, 0.999)), eps=o.get("eps", 1e-8),
                                      return_loss=return_loss, checked=True)
        return ptr, idx, out

    def fold_in_users(self, histories, steps=20, lr=None, n_neg=None, l2=None, random_state=None,
                      return_loss=False):
        """Factors and biases for users that were NOT in the training set, from their histories alone
        (fold-in): the item tables stay frozen and each new user's row and bias are fitted with the
        model's own loss by ``steps`` full-batch Adam steps from zero, all users in one launch
        (``mf_engine.fold_in_users``, rg_mf_fold_in_users).  Returns host arrays ``(factors [n, dim],
        biases [n])`` float32, with ``return_loss`` also the per-user loss at the last step.

        ``histories``: a scipy sparse matrix or an Interactions with ``num_items`` columns (one row
        per new user), or a list of item-id sequences; a user with an empty history keeps the zero
        row.  ``lr``, ``n_neg`` and ``l2`` default to the model's learning rate, negatives per
        positive and weight decay (Adam's betas and eps are the model's when it trained with Adam).
        The negatives are drawn once, uniformly over the items (they may coincide with a positive, as
        in the reference), from ``random_state`` or else the model's own RandomState, which the draw
        advances: an equally seeded RandomState reproduces the call.  The adaptive hinge ('bpr' and
        'adaptive_hinge') takes the maximum over each positive's own negatives.  After a
        data-parallel fit the gathered full tables are used, as in ``predict``.  MF only: the NCF and
        NeuMF models raise NotImplementedError."""
        out = self._fold_in_device(histories, steps, lr, n_neg, l2, random_state, return_loss)[2]
        return tuple(t.cpu().numpy() for t in out)

    def fit_als(self, train_set, iterations=15, regularization=0.01, alpha=40.0, cg_steps=3, verbose=False):
        """Fit the MF tables by implicit alternating least squares (Hu, Koren, Volinsky 2008) instead
        of the sampled SGD step of ``fit``: ``iterations`` sweeps of a user and an item half-step, each
        row taking ``cg_steps`` conjugate-gradient iterations on its confidence-weighted normal
        equations (``als.als_sweeps``: rg_als_gram, rg_als_solve_rows).  No negatives and no random
        draws: it works on a default-constructed model, and the result is reproducible bit for bit.

        Confidence is ``1 + alpha * weight`` with ``train_set.weights`` (1 without weights, duplicates
        of a pair counted as given); ``ratings`` are ignored.  The start is the model's current tables
        (``BilinearNet``'s own init on a fresh model).  The result is installed with zero biases, so
        ``sigmoid(x.y)`` ranks like ``x.y`` and ``recommend``, ``similar_items``, the candidate and
        re-ranking calls and the ranking metrics work on it unchanged; a later ``fit`` continues from
        these tables.  ``als_losses`` holds the ALS objective after every sweep (logged with
        ``verbose``); ``regularization``, ``alpha`` and ``cg_steps`` become ``fold_in_users_als``'
        defaults.  MF only (NotImplementedError for NCF, NeuMF and world_size > 1); ValueError for
        regularization <= 0, alpha < 0, iterations < 1, cg_steps outside [1, 64] or embedding_dim >
        128."""
        iterations, cg_steps = int(iterations), int(cg_steps)
        if not (0.0 < float(regularization) < float("inf")):
            raise ValueError("fit_als: regularization must be finite and > 0")
        if not (0.0 <= float(alpha) < float("inf")):
            raise ValueError("fit_als: alpha must be finite and >= 0")
        if iterations < 1:
            raise ValueError("fit_als: iterations must be >= 1")
        if cg_steps < 1 or cg_steps > als.MAX_CG_STEPS:
            raise ValueError(f"fit_als: cg_steps must be in [1, {als.MAX_CG_STEPS}]")
        if self._world > 1:
            raise NotImplementedError("fit_als is single-process")
        if not self._initialized:
            if self._representation is None and self._embedding_dim > als.MAX_DIM:
                raise ValueError(f"fit_als: embedding_dim must be at most {als.MAX_DIM}")
            self._initialize(train_set)
        if self._kind != "mf":
            raise NotImplementedError("fit_als is implemented for the matrix-factorization model (BilinearNet)")
        if self._embedding_dim > als.MAX_DIM:
            raise ValueError(f"fit_als: embedding_dim must be at most {als.MAX_DIM}")
        self._check_input(train_set.user_ids, train_set.item_ids)
        self.train_set = train_set
        w = getattr(train_set, "weights", None)
        csr_u = als.interactions_csr(train_set.user_ids, train_set.item_ids, w, self._num_users)
        csr_i = als.interactions_csr(train_set.item_ids, train_set.user_ids, w, self._num_items)
        user_w, item_w, user_b, item_b = self._engine.params()
        X, Y = user_w.detach().clone().contiguous(), item_w.detach().clone().contiguous()
        self.als_losses = []
        als.als_sweeps(X, Y, csr_u, csr_i, iterations=iterations, lam=float(regularization), alpha=float(alpha),
                       cg_steps=cg_steps, losses=self.als_losses)
        if verbose:
            for s, v in enumerate(self.als_losses):
                logging.info("ALS sweep {}: objective {:14.6f}".format(s, v))
        tables = [X, Y, torch.zeros_like(user_b), torch.zeros_like(item_b)]
        self._engine.set_params(*tables)
        self._full_tables = None
        self._load_into_net(tables)
        self._als = (float(regularization), float(alpha), cg_steps)
        return self

    def _fold_in_als_device(self, histories, regularization, alpha, cg_steps):
        """``fold_in_users_als`` up to the device results: (indptr, indices, (W, b) on the device)."""
        if not self._initialized:
            raise RuntimeError("fold_in_users_als needs a fitted model")
        if self._kind != "mf":
            raise NotImplementedError("fold-in is implemented for the matrix-factorization model (BilinearNet)")
        reg0, alpha0, _ = self._als if self._als is not None else (0.01, 40.0, None)
        reg = reg0 if regularization is None else float(regularization)
        alpha = alpha0 if alpha is None else float(alpha)
        dim = self._embedding_dim
        cg_steps = min(dim, 16) if cg_steps is None else int(cg_steps)
        if not (0.0 < reg < float("inf")):
            raise ValueError("fold_in_users_als: regularization must be finite and > 0")
        if not (0.0 <= alpha < float("inf")):
            raise ValueError("fold_in_users_als: alpha must be finite and >= 0")
        if cg_steps < 1 or cg_steps > als.MAX_CG_STEPS:
            raise ValueError(f"fold_in_users_als: cg_steps must be in [1, {als.MAX_CG_STEPS}]")
        if dim > als.MAX_DIM:
            raise ValueError(f"fold_in_users_als: embedding_dim must be at most {als.MAX_DIM}")
        ptr, idx = _histories_csr(histories, self._num_items)
        _, item_w, _, _ = self._tables()
        dev = self._engine.device
        W = torch.zeros(len(ptr) - 1, dim, dtype=torch.float32, device=dev)
        if len(ptr) > 1:
            Y = item_w.detach().contiguous()
            als.solve_rows(Y, als.gram(Y, reg), ptr, idx, None, alpha, cg_steps, W)
        return ptr, idx, (W, torch.zeros(len(ptr) - 1, dtype=torch.float32, device=dev))

    def fold_in_users_als(self, histories, regularization=None, alpha=None, cg_steps=None):
        """Factors for users that were NOT in the training set by one ALS user half-step from zero
        against the frozen item table (the closed-form counterpart of ``fold_in_users``; meant for a
        model fitted with ``fit_als``, whose item biases are zero): ``cg_steps`` conjugate-gradient
        iterations per user, ``min(dim, 16)`` by default, in one launch.  ``regularization`` and
        ``alpha`` default to those of ``fit_als`` (0.01 and 40 on a model fitted otherwise).
        ``histories`` as in ``fold_in_users``; a user with an empty history gets the zero row.
        Returns host arrays ``(factors [n, dim], biases [n])`` float32, the biases zero."""
        out = self._fold_in_als_device(histories, regularization, alpha, cg_steps)[2]
        return tuple(t.cpu().numpy() for t in out)

    def recommend_for_histories(self, histories, k=10, exclude_history=True, return_scores=False, method="adam",
                                **fold_kwargs):
        """``recommend`` for users the model has never seen: their rows are folded in from
        ``histories`` (``fold_in_users``; ``fold_kwargs`` are its ``steps``, ``lr``, ``n_neg``, ``l2``
        and ``random_state``) and ranked like known users -- ``(len(histories), k)`` int64 item ids on
        the host in rank order (higher score first, then the lower item id), with ``return_scores``
        also their float32 scores.  ``exclude_history`` leaves each row's own history out: those
        items have the score -inf and are only returned, by id, to a row with fewer than k other
        items.  One fold-in for all rows, then 4096 rows at a time: ``mf_engine.score_users_block``
        with the folded rows as the user table, -inf over the block's histories, rg_topk_rows, and the
        scores gathered from the block at the returned ids.  ``method="als"`` folds in with
        ``fold_in_users_als`` instead (``fold_kwargs`` are then its ``regularization``, ``alpha`` and
        ``cg_steps``); another name is a ValueError.  ValueError for k < 1 or k > min(32, num_items),
        as ``recommend``."""
        k, num_items = int(k), self._num_items
        if self._initialized and (k < 1 or k > min(32, num_items)):
            raise ValueError("k must be in [1, min(32, num_items)]")
        if method not in ("adam", "als"):
            raise ValueError(f"recommend_for_histories: unknown method {method!r}: 'adam' or 'als'")
        names = {"steps", "lr", "n_neg", "l2", "random_state"} if method == "adam" else \
            {"regularization", "alpha", "cg_steps"}
        extra = set(fold_kwargs) - names
        if extra:
            raise TypeError(f"recommend_for_histories: unexpected arguments {sorted(extra)}")
        if method == "als":
            args = dict(regularization=None, alpha=None, cg_steps=None)
            args.update(fold_kwargs)
            ptr, idx, (W, b) = self._fold_in_als_device(histories, **args)
        else:
            args = dict(steps=20, lr=None, n_neg=None, l2=None, random_state=None)
            args.update(fold_kwargs)
            ptr, idx, (W, b) = self._fold_in_device(histories, return_loss=False, **args)
        n = len(ptr) - 1
        ids = np.empty((n, k), dtype=np.int64)
        scores = np.empty((n, k), dtype=np.float32)
        dev = self._engine.device
        _, item_w, _, item_b = self._tables()
        for s in range(0, n, 4096):
            e = min(s + 4096, n)
            blk = mf_engine.score_users_block(W[s:e], item_w, b[s:e], item_b, torch.arange(e - s, device=dev),
                                              checked=True)
            if exclude_history and ptr[e] > ptr[s]:
                r = np.repeat(np.arange(e - s), np.diff(ptr[s:e + 1]))
                blk[torch.as_tensor(r, device=dev),
                    torch.as_tensor(idx[ptr[s]:ptr[e]].astype(np.int64), device=dev)] = float("-inf")
            out, got = _topk_block(blk, k)
            ids[s:e] = got
            if return_scores:
                scores[s:e] = torch.gather(blk, 1, out.to(torch.int64)).cpu().numpy()
        return (ids, scores) if return_scores else ids

    def _item_table(self, space):
        """The item embedding table ``similar_items`` compares, on the device: MF's item factors
        (the gathered full table after a data-parallel fit), the NCF tower's item embeddings, or for
        NeuMF the GMF item table (``space="mf"``) or the tower's (``space="mlp"``)."""
        if self._kind == "mf":
            return self._tables()[1]
        return self._engine.mf_w[1] if space == "mf" else self._engine.item_w

    @staticmethod
    def _check_metric(metric):
        if metric not in mf_engine.SIM_METRICS:
            raise ValueError(f"unknown metric {metric!r}: one of {mf_engine.SIM_METRICS}")

    def _check_space(self, space):
        """``space`` as ``_item_table`` takes it: NeuMF's default is "mf"; ValueError for a name the
        model does not have."""
        neumf = self._kind != "mf" and self._engine.neumf
        if neumf and space is None:
            space = "mf"
        if space not in (("mf", "mlp") if neumf else (None,)):
            raise ValueError(f"unknown space {space!r}: NeuMF has 'mf' (the GMF item table, the default) and 'mlp' "
                             "(the tower's); MF and NCF have one item table and take None")
        return space

    def similar_items(self, item_ids, k=10, metric="cosine", include_self=False, space=None, return_scores=False):
        """The k items most similar to each of ``item_ids`` ("more like this"): ``(len(item_ids), k)``
        int64 item ids on the host in rank order (higher similarity first, then the lower item id),
        with ``return_scores`` also their float32 similarities.  ``metric``: "cosine" or "dot" (the
        inner product) of the item embeddings -- MF's item factors, the NCF tower's item embeddings,
        and for NeuMF the table ``space`` names ("mf": the GMF item table, the default; "mlp": the
        tower's; for MF and NCF it must be None).  The item itself is left out unless
        ``include_self``.  Any number of ids, 4096 at a time through the fused kernel
        (``mf_engine.similar_rows``: product, similarity and ranking in LDS, no (ids, items) block);
        the reciprocal norms are computed once per call.  Only ids and similarities come down.
        ValueError for an id outside [0, num_items), k < 1, k > min(32, num_items - 1) (num_items with
        ``include_self``), an unknown ``metric`` or an unknown ``space``.  The cap stays 32: the fused
        kernel ranks in register lists, and the wide selection (rg_topk_rows_wide) reads a score block
        that this path never builds."""
        items = np.asarray(item_ids, dtype=np.int64).reshape(-1)
        k, n, num_items = int(k), len(items), self._num_items
        self._check_metric(metric)
        if k < 1 or k > min(32, num_items - (0 if include_self else 1)):
            raise ValueError("k must be in [1, min(32, num_items - 1)] (num_items with include_self)")
        if n and (items.min() < 0 or items.max() >= num_items):
            raise ValueError("item id outside [0, num_items)")
        space = self._check_space(space)
        ids = np.empty((n, k), dtype=np.int64)
        sims = np.empty((n, k), dtype=np.float32)
        if n == 0:
            return (ids, sims) if return_scores else ids
        table = self._item_table(space)
        rnorm = mf_engine.row_rnorms(table) if metric == "cosine" else None
        for s in range(0, n, 4096):
            out, sc = mf_engine.similar_rows(table, items[s:s + 4096], k, metric=metric, exclude_self=not include_self,
                                             rnorm=rnorm, checked=True)
            got = out.cpu().numpy()
            if got.min() < 0 or got.max() >= num_items:     # before the ids are used for anything
                raise RuntimeError("rg_item_sim_topk returned an item id outside the table")
            ids[s:s + len(got)] = got
            if return_scores:
                sims[s:s + len(got)] = sc.cpu().numpy()
        return (ids, sims) if return_scores else ids

    def rank_users(self, users, targets_csr, exclude_csr=None):
        """The rank of every item of ``targets_csr``'s rows in the full ranking of a block of
        users (evaluation.py:13-60, mrr_score: scipy rankdata of -score, ties averaged), counted
        on the device by rg_rank_rows; items of ``exclude_csr``'s rows rank last (the reference's
        FLOAT_MAX).  Returns a float64 array on the host, one rank per target: the users in the
        order given, each user's targets in the order of its row's ``indices``.  Only the two
        CSR slices go up and two int32 counts per target come down; the score block is only
        read."""
        from . import _lib
        dev = self._engine.device
        t_ptr, t_idx = _csr_rows(targets_csr, np.asarray(users, dtype=np.int64))
        if not len(t_idx):
            return np.zeros(0, dtype=np.float64)
        ub, s = _score_block(self, users)
        tp, ti = torch.as_tensor(t_ptr, device=dev), torch.as_tensor(t_idx, device=dev)
        ep = ei = None
        if exclude_csr is not None:
            e_ptr, e_idx = _csr_rows(exclude_csr, ub)
            if len(e_idx):
                ep, ei = torch.as_tensor(e_ptr, device=dev), torch.as_tensor(e_idx, device=dev)
        counts = torch.empty(2, len(t_idx), dtype=torch.int32, device=dev)
        lib = _lib.load()
        _lib.check(lib.rg_rank_rows(_lib.stream_handle(), _lib.ptr(s), len(ub), self._num_items, self._num_items,
                                    _lib.ptr(tp), _lib.ptr(ti), _lib.ptr(ep), _lib.ptr(ei), _lib.ptr(counts[0]),
                                    _lib.ptr(counts[1])), "rg_rank_rows")
        above, equal = counts.cpu().numpy().astype(np.float64)
        if (above < 0).any():
            raise ValueError("rank_users: target item id outside [0, num_items)")
        return above + (equal + 1.0) / 2.0

    def test(self, test_set, item_popularity, k=5, rmse_flag=False, precision_recall=False, map_recall=True):
        test_results = {"k": k}
        if rmse_flag:
            dev = self._engine.device
            tu = torch.from_numpy(np.asarray(test_set.user_ids, dtype=np.int64))
            ti = torch.from_numpy(np.asarray(test_set.item_ids, dtype=np.int64))
            total = 0.0
            for s in range(0, len(tu), self._batch_size):
                total += evaluation.rmse_score(self._net, tu[s:s + self._batch_size].to(dev),
                                               ti[s:s + self._batch_size].to(dev))
            total /= len(test_set)
            logging.info("BCE: {}".format(np.sqrt(total)))
            test_results["bce"] = float(np.sqrt(total))
        if precision_recall:
            pop_p, pop_r = evaluation.evaluate_popItems(item_popularity, test_set, k=k)
            rand_p, rand_r = evaluation.evaluate_random(item_popularity, test_set, k=k)
            p, r = evaluation.precision_recall_score(self, test=test_set, k=k)
            logging.info(self.model_name + " precision@{} {} recall@{} {}".format(k, p, k, r))
            logging.info("Random: precision@{} {} recall@{} {}".format(k, rand_p, k, rand_r))
            logging.info("PopItem Algorithm: precision@{} {} recall@{} {}".format(k, pop_p, k, pop_r))
            test_results.update(precision=float(p), recall=float(r), rand_prec=float(rand_p),
                                rand_rec=float(rand_r), pop_prec=float(pop_p), pop_rec=float(pop_r), at_k=k)
        if map_recall:
            map_k = evaluation.map_at_k(self, test=test_set, k=k)
            _, r = evaluation.precision_recall_score(self, test=test_set, k=k)
            logging.info(self.model_name + " map@{} {} recall@{} {}".format(k, map_k, k, r))
            test_results["map"] = float(map_k)
        with open(os.path.join(self.experiment_logs, "test_summary.json"), "w") as fp:
            json.dump(test_results, fp)
        return test_results

    def save_readable_model(self, model_save_dir, state_dict):
        fname = os.path.join(model_save_dir, "best_model")
        logging.info("Saving state in {}".format(fname))
        torch.save({"network": {k: v.detach().cpu() for k, v in state_dict.items()}}, f=fname)
