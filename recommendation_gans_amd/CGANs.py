"""Conditional GAN for slate generation (CGANs.py of the reference), on the fused
HIP iterations of rg_gan.hip (recommendation_gans_amd.gan_engine).

``CGAN(G, D, z_dim, n_iter, batch_size, loss_fun, learning_rate, slate_size,
G_optimizer_func, embedding_dim, hidden_layer, D_optimizer_func,
experiment_name, use_cuda, random_state)`` with the reference's methods:
``fit`` (CGANs.py:230-336), ``train_discriminator_iteration`` (:410-457),
``train_generator_iteration`` (:370-408), ``test`` (:507-561),
``one_hot_encoding``, ``preprocess_train``, ``save_readable_model``.  The G / D
modules (spotlight.dnn_models.cGAN_models) supply the architecture and the
initial parameters; training runs on the device and the modules receive the
trained parameters back (``G`` is the best-validation generator after ``fit``).

Behaviour kept from the reference: z ~ U[0, 1) (``torch.rand``), the +-0.01 clamp of
every D parameter at each D iteration, one G iteration every ``n_critic`` = 5 D
iterations on the same batch, weight_decay 0, the per-epoch validation precision
and best-generator snapshot, summary.csv columns, and the training precision /
recall of ``precision_recall_slates_atk`` (0 for every row: the reference's set
intersection of identity-hashed 0-d tensors).  Differences: the reference's
``fit`` raises NameError after its first epoch (``real_score`` is undefined at
CGANs.py:326); here that log line reports the last D iteration's mean D(real)
and training continues.  ``run_val_iteration`` references undefined targets in
the reference (:497-503) and is not provided.
"""
import copy
import json
import logging
import math
import os

import numpy as np
import torch
import torch.nn as nn

from .gan_engine import GANBatch, GANEngine, csr_to_device
from .spotlight import optimizers as sp_optimizers
from .spotlight.evaluation import (SLATE_HITS_MAX_K, precision_recall_score_slates, precision_recall_slates_atk,
                                   slate_precision_recall)
from .spotlight.torch_utils import minibatch
from .utils.storage_utils import save_statistics

logging.basicConfig(format="%(message)s", level=logging.INFO)

# CGAN.test uploads the padded history matrix (users x the longest history, int32) in chunks of
# whole batches of at most this many bytes (every row is as wide as the longest history, so at
# ML-20M's user count a few thousand columns already make it gigabytes)
HIST_UPLOAD_BYTES = 256 << 20


def _row_counts(csr, rows):
    """Targets per user for the first ``rows`` rows of a CSR (rows past its last: 0)."""
    n = np.zeros(rows, dtype=np.int64)
    m = min(rows, csr.shape[0])
    n[:m] = np.diff(csr.indptr[:m + 1])
    return n


class CGAN:
    def __init__(self, G=None, D=None, z_dim=100, n_iter=15, batch_size=128, loss_fun="bce", learning_rate=1e-4,
                 slate_size=3, G_optimizer_func=None, embedding_dim=5, hidden_layer=16, D_optimizer_func=None,
                 experiment_name="CGANs", use_cuda=False, random_state=None):
        self.exeriment_name = experiment_name
        self.experiment_folder = os.path.abspath("experiments_results/" + experiment_name)
        self.experiment_logs = os.path.abspath(os.path.join(self.experiment_folder, "result_outputs"))
        self.experiment_saved_models = os.path.abspath(os.path.join(self.experiment_folder, "saved_models"))
        for d in ("experiments_results", self.experiment_folder, self.experiment_logs, self.experiment_saved_models):
            os.makedirs(d, exist_ok=True)
        self.starting_epoch = 0
        self.training = True
        self._n_iter = n_iter
        self.G, self.D = G, D
        self.slate_size = slate_size
        self._learning_rate = learning_rate
        self._use_cuda = self.use_cuda = use_cuda
        self.G_optimizer_func, self.D_optimizer_func = G_optimizer_func, D_optimizer_func
        self._random_state = random_state or np.random.RandomState()
        self.hidden_layer, self.embedding_dim, self.z_dim = hidden_layer, embedding_dim, z_dim
        self.loss_fun = loss_fun
        self.weight_cliping_limit = 0.01
        self.n_critic = 5
        self._batch_size = batch_size
        self.logistic = nn.Sigmoid()
        self.chosen_epoch = -1
        self.best_model = None
        self.best_precision = -1
        self.gamma = 10
        # the fused path runs on the GPU whatever use_cuda says (there is no CPU path)
        self.device = torch.device("cuda")
        self.dtype = torch.cuda.FloatTensor
        self.engine = None
        self._batches = {}
        assert loss_fun in ("mse", "bce")

    # ------------------------------------------------------------------ setup
    def _opt_kind(self, func):
        d = sp_optimizers.describe(func if func is not None else sp_optimizers.adam_optimizer, self._learning_rate,
                                   0.0)
        return d

    def _initialize(self):
        """CGANs.py:140-179: optimizers (weight_decay 0, lr), configuration.json."""
        gd, dd = self._opt_kind(self.G_optimizer_func), self._opt_kind(self.D_optimizer_func)
        if (gd["kind"], gd.get("alpha"), gd.get("betas")) != (dd["kind"], dd.get("alpha"), dd.get("betas")):
            raise NotImplementedError("G and D optimizers of different kinds are not supported")
        self.criterion = nn.BCEWithLogitsLoss() if self.loss_fun == "mse" else nn.MSELoss()
        S, N, E = self.slate_size, self.num_items, self.embedding_dim
        H = self.G.mult_heads["head_0"].in_features
        self.engine = GANEngine(self.G.state_dict(), self.D.state_dict(), N, S, H, self.G.y, self.G.z,
                                batch_max=self._batch_size, optimizer=gd["kind"], lr=gd["lr"],
                                alpha=gd.get("alpha", 0.99), betas=gd.get("betas", (0.5, 0.999)),
                                eps=gd.get("eps", 1e-8), seed=int(self._random_state.randint(0, 2 ** 31 - 1)))
        configuration = {"batch_size": self._batch_size, "z_dim": self.z_dim, "slate_size": self.slate_size,
                         "n_iter": self._n_iter, "learning_rate": self._learning_rate, "users": self.num_users,
                         "movies": self.num_items, "hidden_layer": self.hidden_layer,
                         "embedding_dim": self.embedding_dim}
        with open(os.path.join(self.experiment_logs, "configuration.json"), "w") as fp:
            json.dump(configuration, fp)

    def _sync_modules(self):
        self.G.load_state_dict(self.engine.g_state_dict())
        self.D.load_state_dict(self.engine.d_state_dict())

    def _batch(self, hist, slates=None, key=None):
        if key is not None and key in self._batches:
            return self._batches[key]
        h = hist.detach().cpu().numpy() if torch.is_tensor(hist) else np.asarray(hist)
        s = None
        if slates is not None:
            s = slates.detach().cpu().numpy() if torch.is_tensor(slates) else np.asarray(slates)
        b = GANBatch(h.astype(np.int64), None if s is None else s.astype(np.int64), self.num_items,
                     self.slate_size, self.device)
        if key is not None:
            self._batches[key] = b
        return b

    # ------------------------------------------------------------------ reference API
    def one_hot_encoding(self, slates, num_items):
        """CGANs.py:181-198: (B, S * num_items) one-hot rows (the fused D step never
        builds them; kept for callers)."""
        oh = nn.functional.one_hot(torch.as_tensor(slates).to(torch.int64), num_classes=num_items)
        return oh.reshape(oh.shape[0], -1).float()

    def preprocess_train(self, interactions):
        """CGANs.py:200-224."""
        from .utils.slate_data_provider import preprocess_train
        rows, vec, _ = preprocess_train(interactions, interactions.shape[0], self.num_items)
        return rows, vec

    def sigmoid(self, x):
        return 1 / (1 + math.exp(-x))

    def train_discriminator_iteration(self, batch_user, batch_slate, _key=None):
        """CGANs.py:410-457.  Returns d_loss (float)."""
        out = self.engine.d_step(self._batch(batch_user, batch_slate, _key))
        self._last_d = out
        return float(out[0])

    def train_generator_iteration(self, batch_user, batch_slate, _key=None):
        """CGANs.py:370-408.  Returns (g_loss, precision list, recall list)."""
        g, slates = self.engine.g_step(self._batch(batch_user, batch_slate, _key), slates=True)
        precision, recall = precision_recall_slates_atk(slates.type(torch.int64), batch_slate, k=self.slate_size)
        return float(g[0]), precision, recall

    def fit(self, train_vec, train_slates, users, movies, valid_vec, valid_cold_users, valid_set):
        self.num_users, self.num_items = users, movies
        self._initialize()
        steps_performed = 0
        user_slate_tensor = torch.from_numpy(np.asarray(train_slates)).float()
        logging.info("training start!!")
        total_losses = {"G_loss": [], "D_loss": [], "G_pre": [], "G_rec": [], "curr_epoch": [], "Val_prec": []}
        real_score = float("nan")
        for epoch_num in range(self._n_iter):
            g_losses, d_losses = [], []
            cur = {"G_loss": [], "D_loss": [], "G_pre": [], "G_rec": [], "Val_prec": []}
            for bi, (batch_user, batch_slate) in enumerate(minibatch(train_vec, user_slate_tensor,
                                                                     batch_size=self._batch_size)):
                steps_performed += 1
                b = self._batch(batch_user, batch_slate, key=("train", bi))
                d_out = self.engine.d_step(b)
                d_losses.append(d_out)
                if steps_performed % self.n_critic == 0:
                    g, slates = self.engine.g_step(b, slates=True)
                    pre, rec = precision_recall_slates_atk(slates.type(torch.int64), batch_slate,
                                                           k=self.slate_size)
                    g_losses.append(g)
                    cur["G_loss"].append(g)
                    cur["D_loss"].append(d_out)
                    cur["G_pre"] += pre
                    cur["G_rec"] += rec
            # one host sync per epoch for the loss logs
            cur["G_loss"] = [float(t[0]) for t in cur["G_loss"]]
            cur["D_loss"] = [float(t[0]) for t in cur["D_loss"]]
            if d_losses:
                real_score = float(d_losses[-1][1])
            results = self.test(valid_vec, valid_set, valid_cold_users)
            logging.info(str(results["precision"]))
            if results["precision"] > self.best_precision:
                self.best_model = self.engine.g_state_dict()
                self.best_precision = results["precision"]
                self.chosen_epoch = epoch_num
            cur["Val_prec"].append(results["precision"])
            total_losses["curr_epoch"].append(epoch_num)
            for key, value in cur.items():
                total_losses[key].append(np.mean(value))
            save_statistics(experiment_log_dir=self.experiment_logs, filename="summary.csv", stats_dict=total_losses,
                            current_epoch=epoch_num,
                            continue_from_mode=True if (self.starting_epoch != 0 or epoch_num > 0) else False)
            logging.info("--------------- Epoch %d ---------------" % epoch_num)
            logging.info("G_Loss: {}".format(np.mean([float(t[0]) for t in g_losses]) if g_losses else float("nan")))
            logging.info("D_Loss: {} D(x): {}".format(np.mean([float(t[0]) for t in d_losses]), self.sigmoid(real_score)))
        self._sync_modules()
        if self.best_model is not None:
            self.engine.load_g_state(self.best_model)
            self.G.load_state_dict(self.best_model)
        logging.info("Model chosen from: {}".format(self.chosen_epoch))
        self.save_readable_model(self.experiment_saved_models, self.G.state_dict())
        self.training = False

    def _history_chunks(self, train_vec):
        """Yields (first row, device int32 histories) over ``train_vec`` in chunks of whole
        batches of at most HIST_UPLOAD_BYTES, each range-checked on the host before it goes up
        (GANBatch's rule: ids in [0, num_items], num_items = padding)."""
        h = train_vec.detach().cpu().numpy() if torch.is_tensor(train_vec) else np.asarray(train_vec)
        if not len(h):
            return
        B = self._batch_size
        per = max(1, HIST_UPLOAD_BYTES // (4 * h.shape[1] * B)) * B
        for r0 in range(0, len(h), per):
            c = h[r0:r0 + per].astype(np.int64)
            if c.min() < 0 or c.max() > self.num_items:
                raise ValueError("history ids must lie in [0, num_items] (num_items = padding)")
            yield r0, torch.from_numpy(c.astype(np.int32)).to(self.device)

    def _slate_marks(self, chunks, users, csr):
        """One group of users (histories in ``chunks``, held-out items in the CSR ``csr``): the
        device int32 hit masks of their generated slates (GANEngine.slate_hits), or, for a slate
        wider than a mask word, the slates themselves."""
        S, dev = self.slate_size, self.device
        if S > SLATE_HITS_MAX_K:
            out = torch.empty(users, S, dtype=torch.int32, device=dev)
            for r0, hist in chunks:
                out[r0:r0 + hist.shape[0]] = self.engine.generate_slates(hist)
            return out
        tp, ti = csr_to_device(csr, users, dev)
        out = torch.empty(users, dtype=torch.int32, device=dev)
        for r0, hist in chunks:
            r1 = r0 + hist.shape[0]
            self.engine.slate_hits(hist, tp[r0:r1 + 1], ti, S, out=out[r0:r1])
        return out

    def test(self, train_vec, test, cold_start_users=None):
        """CGANs.py:507-561: precision / recall@slate_size of the eval-mode generator's
        slates against each user's held-out items; cold-start users condition on the
        padding item only.  Writes test_results.json.

        The slates never leave the device: the histories go up once as int32, the held-out
        items once as a CSR, rg_slate_hits marks each slate's hits, and one word per user
        comes down in a single copy for both groups of users.  The noise is drawn as before
        (one torch.rand per batch, in batch order), so a seed gives the same figures."""
        if self.engine is None:
            raise RuntimeError("call fit() first")
        S = self.slate_size
        test = test.tocsr()
        groups = [(self._slate_marks(self._history_chunks(train_vec), len(train_vec), test), test)]
        if cold_start_users is not None and cold_start_users.shape[0] > 0:
            cold = torch.full((cold_start_users.shape[0], self.embedding_dim), self.num_items, dtype=torch.int32,
                              device=self.device)
            cold_csr = cold_start_users.tocsr()
            groups.append((self._slate_marks([(0, cold)], cold.shape[0], cold_csr), cold_csr))
        if S > SLATE_HITS_MAX_K:
            precision, recall = [], []
            for slates, csr in groups:
                p, r = precision_recall_score_slates(slates.cpu().type(torch.int64), csr[:slates.shape[0], :], k=S)
                precision += p
                recall += r
        else:
            masks = torch.cat([m for m, _ in groups]).cpu().numpy()
            n = np.concatenate([_row_counts(csr, len(m)) for m, csr in groups])
            precision, recall = slate_precision_recall(masks, n, S)
        res = {"precision": float(np.mean(precision)) if precision else float("nan"),
               "recall": float(np.mean(recall)) if recall else float("nan"),
               "at": self.slate_size}
        with open(os.path.join(self.experiment_logs, "test_results.json"), "w") as fp:
            json.dump(res, fp)
        return res

    def recommend(self, train_vec, exclude_history=True, distinct=True, samples=1, return_scores=False):
        """A slate to serve for every row of ``train_vec`` (padded histories, as ``test`` takes
        them): int64 (users, slate_size) on the host.  No counterpart in the reference, whose only
        inference is each head's argmax: here the heads are taken in order, each the best item
        that is not in the user's history (``exclude_history``) and not already in the slate
        (``distinct``); equal head outputs go to the lower id, and ``num_items`` marks a slot for
        which no item was left.  The histories go up once (``_history_chunks``, range-checked),
        the selection runs on the device (GANEngine.recommend_slates) and the slates come down in
        one copy.  ``test`` keeps the reference's argmax slates.

        ``samples`` = M > 1 is discriminator-guided sampling: per history chunk and per batch of
        ``batch_size`` rows, M noise blocks are drawn in order (``torch.rand(rows, z_dim)``), each
        gives a candidate slate per row, the critic scores the M x rows candidates in one
        ``score_slates`` call (the histories repeated by a copy on the device, not uploaded again), and each
        row keeps its best-scored candidate -- equal scores: the lower sample index; a NaN score
        loses to any number.  The selection stays on the device.  ``return_scores`` also returns
        the kept slates' critic scores, float32 (users,) on the host (with ``samples`` = 1: the
        score of the one slate drawn)."""
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
            raise ValueError("samples must be an integer >= 1")
        if self.engine is None:
            raise RuntimeError("call fit() first")
        out = torch.empty(len(train_vec), self.slate_size, dtype=torch.int32, device=self.device)
        scores = torch.empty(len(train_vec), dtype=torch.float32, device=self.device) if return_scores else None
        for r0, hist in self._history_chunks(train_vec):
            r1 = r0 + hist.shape[0]
            if samples == 1:
                out[r0:r1] = self.engine.recommend_slates(hist, exclude_history=exclude_history, distinct=distinct)
                if return_scores:
                    self.engine.score_slates(hist, out[r0:r1], out=scores[r0:r1])
            else:
                out[r0:r1], best = self._best_of(hist, int(samples), exclude_history, distinct)
                if return_scores:
                    scores[r0:r1] = best
        if return_scores:
            return out.cpu().to(torch.int64), scores.cpu()
        return out.cpu().to(torch.int64)

    def _best_of(self, hist, M, exclude_history, distinct):
        """``recommend``'s best of M candidates for one chunk of histories (device int32): the kept
        slates (rows, S) int32 and their critic scores (rows,) float32, both on the device."""
        rows, B, S, dev = hist.shape[0], self._batch_size, self.slate_size, self.device
        cand = torch.empty(M, rows, S, dtype=torch.int32, device=dev)
        for b0 in range(0, rows, B):
            hb = hist[b0:b0 + B]
            for m in range(M):
                z = torch.rand(hb.shape[0], self.engine.Z, device=dev)
                cand[m, b0:b0 + B] = self.engine.recommend_slates(hb, exclude_history=exclude_history,
                                                                  distinct=distinct, z=z)
        # the histories M times over: a copy made on the device (the entry wants contiguous rows)
        sc = self.engine.score_slates(hist.repeat(M, 1), cand.view(M * rows, S)).view(M, rows)
        pick = self._pick_best(sc)
        rr = torch.arange(rows, device=dev)
        return cand[pick, rr], sc[pick, rr]

    @staticmethod
    def _pick_best(sc):
        """Per column of ``sc`` (samples, rows) the sample with the highest score: equal scores go
        to the lower sample index and a NaN loses to any number, -inf included (a column of NaN
        only: sample 0)."""
        nan = torch.isnan(sc)
        best = torch.where(nan, torch.full_like(sc, float("-inf")), sc).max(0).values
        # the first sample that is a number and holds the maximum (argmax returns the first True)
        return ((sc == best) & ~nan).to(torch.uint8).argmax(0)

    def score_slates(self, train_vec, slates):
        """The critic's eval-mode score D(one_hot(slate), history) of one slate per row of
        ``train_vec`` (padded histories, as ``test`` takes them): float32 (users,) on the host.
        ``slates``: an array or tensor (host or device) shaped (users, slate_size) of integral
        values in [0, num_items]; ``num_items``, the id ``recommend`` leaves in an empty slot,
        selects nothing.  The histories go up through ``_history_chunks`` (range-checked), the
        slates are checked on the host, GANEngine.score_slates (rg_gan_score_slates) scores each
        chunk and the scores come down in one copy.  The discriminator is read as stored: no
        clamp, no dropout."""
        if self.engine is None:
            raise RuntimeError("call fit() first")
        s = slates.detach().cpu().numpy() if torch.is_tensor(slates) else np.asarray(slates)
        if s.ndim != 2 or s.shape != (len(train_vec), self.slate_size):
            raise ValueError(f"slates must be ({len(train_vec)}, {self.slate_size}): one slate per history row")
        if s.dtype.kind not in "iuf" or (s.dtype.kind == "f" and not np.all(s == np.floor(s))):
            raise ValueError("slates must hold integral values")
        if s.size and (s.min() < 0 or s.max() > self.num_items):
            raise ValueError("slate ids must lie in [0, num_items] (num_items = an empty slot)")
        sl = torch.from_numpy(np.ascontiguousarray(s.astype(np.int32))).to(self.device)
        out = torch.empty(len(s), dtype=torch.float32, device=self.device)
        for r0, hist in self._history_chunks(train_vec):
            r1 = r0 + hist.shape[0]
            self.engine.score_slates(hist, sl[r0:r1], out=out[r0:r1])
        return out.cpu()

    def save_readable_model(self, model_save_dir, state_dict):
        fname = os.path.join(model_save_dir, "generator")
        logging.info("Saving state in {}".format(fname))
        torch.save({"network": state_dict}, f=fname)
