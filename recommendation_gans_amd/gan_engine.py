"""cGAN training engine on the HIP path (rg_gan.hip through the C-ABI).

Holds the generator / discriminator of spotlight/dnn_models/cGAN_models.py in the
flat device layouts of ``rg_gan_layout`` with their optimizer states, turns user
histories + target slates into device batches, and runs the reference's two
iterations (CGANs.py:410-457 discriminator, :370-408 generator) as one C-ABI call
each.  State dicts come in and go out under the reference's parameter names and
shapes (cGAN_models.py), so checkpoints stay ``torch.save({'network': ...})``
compatible with CGANs.py:565-569.

There is no CPU fallback: constructing an engine loads librg_hip.so and needs a
GPU device.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check

OPT_KINDS = {"adam": 0, "sgd": 1, "rms": 2}
G_BN_BUFFERS = ("running_mean", "running_var")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def csr_to_device(csr, rows, device):
    """The first ``rows`` rows of a scipy CSR as rg_slate_hits' targets: (tgt_ptr int64
    (rows + 1), tgt_idx int32) on ``device``; rows past the matrix's last are empty, and an
    empty index list still gets a valid pointer."""
    n = min(rows, csr.shape[0])
    tp = np.full(rows + 1, csr.indptr[n], dtype=np.int64)
    tp[:n + 1] = csr.indptr[:n + 1]
    ti = np.ascontiguousarray(csr.indices[:tp[-1]], dtype=np.int32)
    if not len(ti):
        ti = np.zeros(1, np.int32)
    return torch.from_numpy(tp).to(device), torch.from_numpy(ti).to(device)


def slate_hits(slates, tgt_ptr, tgt_idx, k, out=None):
    """rg_slate_hits on device tensors: ``slates`` int32 (rows, S) with unit column stride,
    ``tgt_ptr`` int64 (rows + 1) / ``tgt_idx`` int32 the rows' CSR targets, 1 <= k <= min(32, S).
    Returns the int32 (rows,) masks (written into ``out`` when given).  No host
    synchronisation: the arguments' dtypes and shapes are checked, the ids are not."""
    rows, S = slates.shape
    if slates.dtype != torch.int32 or not slates.is_cuda or (S > 1 and slates.stride(1) != 1) or \
            (rows > 1 and slates.stride(0) < S):
        raise ValueError("slates must be a device int32 (rows, S) tensor with contiguous rows")
    if tgt_ptr.dtype != torch.int64 or tgt_idx.dtype != torch.int32 or tgt_ptr.numel() != rows + 1 or \
            not (tgt_ptr.is_contiguous() and tgt_idx.is_contiguous()) or \
            tgt_ptr.device != slates.device or tgt_idx.device != slates.device:
        raise ValueError("tgt_ptr must be int64 (rows + 1) and tgt_idx int32, contiguous, on the slates' device")
    if out is None:
        out = torch.empty(rows, dtype=torch.int32, device=slates.device)
    elif out.dtype not in (torch.int32, torch.uint32) or out.shape != (rows,) or not out.is_contiguous() or \
            out.device != slates.device:
        raise ValueError("out must be a contiguous int32 / uint32 (rows,) tensor on the slates' device")
    if rows == 0:
        return out
    ld = slates.stride(0) if rows > 1 else S
    stream = ctypes.c_void_p(torch.cuda.current_stream(slates.device).cuda_stream)
    check(_lib.load().rg_slate_hits(stream, ptr(slates), rows, S, ld, int(k), ptr(tgt_ptr), ptr(tgt_idx), ptr(out)),
          "rg_slate_hits")
    return out


class GANBatch:
    """Device form of one minibatch: histories (B, L) padded with N, target slates (B, S),
    the history items grouped per item (embedding backward) and the real slates as
    sorted W1 column hits (the one-hot rows of CGANs.py:181-198, never materialised)."""

    def __init__(self, hist, slates, N, S, device):
        hist = np.asarray(hist)
        B, L = hist.shape
        h = hist.astype(np.int64)
        if h.min() < 0 or h.max() > N:
            raise ValueError("history ids must lie in [0, num_items] (num_items = padding)")
        self.rows, self.L = B, L
        self.hist = torch.from_numpy(h.astype(np.int32)).to(device).contiguous()
        b_idx = np.repeat(np.arange(B, dtype=np.int64), L)
        flat = h.reshape(-1)
        keep = flat != N
        items, rows = flat[keep], b_idx[keep]
        order = np.lexsort((rows, items))
        items, rows = items[order], rows[order]
        uniq, start = np.unique(items, return_index=True)
        off = np.append(start, len(items)).astype(np.int32)
        self.n_items = len(uniq)
        self.hist_items = torch.from_numpy(np.ascontiguousarray(uniq.astype(np.int32))).to(device)
        self.hist_off = torch.from_numpy(off).to(device)
        self.hist_rows = torch.from_numpy(np.ascontiguousarray(rows.astype(np.int32))).to(device)
        if len(uniq) == 0:      # keep valid pointers
            self.hist_items = torch.zeros(1, dtype=torch.int32, device=device)
            self.hist_rows = torch.zeros(1, dtype=torch.int32, device=device)
        self.slates = None
        self.n_hits = 0
        if slates is not None:
            sl = np.asarray(slates).astype(np.int64)
            if sl.shape != (B, S) or sl.min() < 0 or sl.max() >= N:
                raise ValueError(f"slates must be ({B}, {S}) item ids in [0, {N})")
            self.slates = torch.from_numpy(sl.astype(np.int32)).to(device).contiguous()
            col = (np.arange(S, dtype=np.int64)[None, :] * N + sl).reshape(-1)
            row = np.repeat(np.arange(B, dtype=np.int64), S)
            o = np.lexsort((row, col))
            self.hit_col = torch.from_numpy(col[o].astype(np.int32)).to(device)
            self.hit_row = torch.from_numpy(row[o].astype(np.int32)).to(device)
            edges = np.arange(0, (S * N + 127) // 128 + 1, dtype=np.int64) * 128      # GEMM column tiles
            self.hit_tile_off = torch.from_numpy(np.searchsorted(col[o], edges).astype(np.int32)).to(device)
            self.n_hits = B * S

    def c_struct(self):
        b = _lib.GANBatch()
        b.rows, b.hist_len, b.hist = self.rows, self.L, ptr(self.hist)
        b.slates = ptr(self.slates)
        b.hist_items, b.hist_off, b.hist_rows = ptr(self.hist_items), ptr(self.hist_off), ptr(self.hist_rows)
        b.n_hist_items = self.n_items
        b.n_hits = self.n_hits
        if self.n_hits:
            b.hit_col, b.hit_row, b.hit_tile_off = ptr(self.hit_col), ptr(self.hit_row), ptr(self.hit_tile_off)
        return b


class GANEngine:
    """Generator + discriminator parameters, optimizer states and workspace on one GPU."""

    def __init__(self, g_state, d_state, num_items, slate_size, hidden, emb_dim, z_dim=100, batch_max=256,
                 optimizer="rms", lr=1e-3, device="cuda:0", alpha=0.99, betas=(0.5, 0.999), eps=1e-8, seed=0):
        if optimizer not in OPT_KINDS:
            raise ValueError(f"optimizer must be one of {sorted(OPT_KINDS)}")
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GANEngine runs on the GPU only (no CPU fallback)")
        self.N, self.S, self.H, self.E, self.Z = num_items, slate_size, hidden, emb_dim, z_dim
        self.dims = _lib.GANDims(num_items, slate_size, hidden, emb_dim, z_dim, batch_max)
        go = (ctypes.c_int64 * (len(_lib.GAN_G_BLOCKS) + 1))()
        do = (ctypes.c_int64 * (len(_lib.GAN_D_BLOCKS) + 1))()
        st = (ctypes.c_int64 * 2)()
        check(self.lib.rg_gan_layout(ctypes.byref(self.dims), go, do, st), "rg_gan_layout")
        self.go = {k: go[i] for i, k in enumerate(_lib.GAN_G_BLOCKS + ["END"])}
        self.do = {k: do[i] for i, k in enumerate(_lib.GAN_D_BLOCKS + ["END"])}
        self.kz, self.ks = st[0], st[1]
        dev = self.device
        self.g = torch.zeros(self.go["END"], dtype=torch.float32, device=dev)
        self.d = torch.zeros(self.do["END"], dtype=torch.float32, device=dev)
        self.opt_kind, self.lr, self.alpha, self.betas, self.eps = optimizer, lr, alpha, betas, eps
        need_m, need_v = optimizer == "adam", optimizer in ("adam", "rms")
        ng, nd = self.go["RM1"], self.do["END"]
        self.g_m = torch.zeros(ng, device=dev) if need_m else None
        self.g_v = torch.zeros(ng, device=dev) if need_v else None
        self.d_m = torch.zeros(nd, device=dev) if need_m else None
        self.d_v = torch.zeros(nd, device=dev) if need_v else None
        self.ws = torch.zeros(int(self.lib.rg_gan_workspace_bytes(ctypes.byref(self.dims))), dtype=torch.uint8,
                              device=dev)
        self.batch_max = batch_max
        self._rec_scratch = None    # rg_gan_recommend's scratch, allocated at the first recommend_slates
        self.g_steps = 0            # optimizer steps taken (Adam bias corrections)
        self.d_steps = 0
        self.bn_tracked = [0, 0]    # num_batches_tracked of the two BatchNorms
        self.seed = int(seed) * 0x100000001 + 1
        self.out = torch.zeros(4, dtype=torch.float32, device=dev)
        self.load_g_state(g_state)
        self.load_d_state(d_state)

    # ------------------------------------------------------------------ layouts
    def _gv(self, blk, shape):
        o = self.go[blk]
        return self.g[o:o + int(np.prod(shape))].view(shape)

    def _dv(self, blk, shape):
        o = self.do[blk]
        return self.d[o:o + int(np.prod(shape))].view(shape)

    def load_g_state(self, sd):
        N, S, H, E, Z = self.N, self.S, self.H, self.E, self.Z
        H1 = H // 2
        with torch.no_grad():
            self._gv("EMB", (N + 1, E)).copy_(sd["embedding_layer.weight"])
            self._gv("W1", (H1, self.kz))[:, :Z + E].copy_(sd["layers.0.weight"])
            self._gv("B1", (H1,)).copy_(sd["layers.0.bias"])
            self._gv("GAMMA1", (H1,)).copy_(sd["layers.1.weight"])
            self._gv("BETA1", (H1,)).copy_(sd["layers.1.bias"])
            self._gv("W2", (H, H1)).copy_(sd["layers.4.weight"])
            self._gv("B2", (H,)).copy_(sd["layers.4.bias"])
            self._gv("GAMMA2", (H,)).copy_(sd["layers.5.weight"])
            self._gv("BETA2", (H,)).copy_(sd["layers.5.bias"])
            wh, bh = self._gv("WH", (self.ks, H)), self._gv("BH", (self.ks,))
            for s in range(S):
                wh[s * N:(s + 1) * N].copy_(sd[f"mult_heads.head_{s}.weight"])
                bh[s * N:(s + 1) * N].copy_(sd[f"mult_heads.head_{s}.bias"])
            for k, (bn, w) in enumerate((("layers.1", H1), ("layers.5", H))):
                self._gv(f"RM{k + 1}", (w,)).copy_(sd[bn + ".running_mean"])
                self._gv(f"RV{k + 1}", (w,)).copy_(sd[bn + ".running_var"])
                self.bn_tracked[k] = int(sd.get(bn + ".num_batches_tracked", torch.tensor(0)))

    def load_d_state(self, sd):
        N, S, H, E = self.N, self.S, self.H, self.E
        SN = S * N
        with torch.no_grad():
            self._dv("EMB", (N + 1, E)).copy_(sd["embedding_layer.weight"])
            w1 = sd["layers.0.weight"]
            self._dv("W1E", (2 * H, E)).copy_(w1[:, :E])
            self._dv("W1S", (2 * H, self.ks))[:, :SN].copy_(w1[:, E:])
            self._dv("B1", (2 * H,)).copy_(sd["layers.0.bias"])
            self._dv("W2", (H, 2 * H)).copy_(sd["layers.3.weight"])
            self._dv("B2", (H,)).copy_(sd["layers.3.bias"])
            self._dv("W3", (H // 2, H)).copy_(sd["layers.6.weight"])
            self._dv("B3", (H // 2,)).copy_(sd["layers.6.bias"])
            self._dv("W4", (1, H // 2)).copy_(sd["layers.9.weight"])
            self._dv("B4", (1,)).copy_(sd["layers.9.bias"])

    def g_state_dict(self):
        """The generator's state_dict (reference names and shapes, CPU copies)."""
        N, S, H, E, Z = self.N, self.S, self.H, self.E, self.Z
        H1 = H // 2
        c = lambda t: t.detach().clone().cpu()  # noqa: E731
        sd = {"embedding_layer.weight": c(self._gv("EMB", (N + 1, E))),
              "layers.0.weight": c(self._gv("W1", (H1, self.kz))[:, :Z + E]),
              "layers.0.bias": c(self._gv("B1", (H1,))),
              "layers.1.weight": c(self._gv("GAMMA1", (H1,))), "layers.1.bias": c(self._gv("BETA1", (H1,))),
              "layers.1.running_mean": c(self._gv("RM1", (H1,))), "layers.1.running_var": c(self._gv("RV1", (H1,))),
              "layers.1.num_batches_tracked": torch.tensor(self.bn_tracked[0]),
              "layers.4.weight": c(self._gv("W2", (H, H1))), "layers.4.bias": c(self._gv("B2", (H,))),
              "layers.5.weight": c(self._gv("GAMMA2", (H,))), "layers.5.bias": c(self._gv("BETA2", (H,))),
              "layers.5.running_mean": c(self._gv("RM2", (H,))), "layers.5.running_var": c(self._gv("RV2", (H,))),
              "layers.5.num_batches_tracked": torch.tensor(self.bn_tracked[1])}
        wh, bh = self._gv("WH", (self.ks, H)), self._gv("BH", (self.ks,))
        for s in range(S):
            sd[f"mult_heads.head_{s}.weight"] = c(wh[s * N:(s + 1) * N])
            sd[f"mult_heads.head_{s}.bias"] = c(bh[s * N:(s + 1) * N])
        return sd

    def d_state_dict(self):
        N, S, H, E = self.N, self.S, self.H, self.E
        c = lambda t: t.detach().clone().cpu()  # noqa: E731
        w1 = torch.cat([self._dv("W1E", (2 * H, E)), self._dv("W1S", (2 * H, self.ks))[:, :S * N]], 1)
        return {"embedding_layer.weight": c(self._dv("EMB", (N + 1, E))), "layers.0.weight": c(w1),
                "layers.0.bias": c(self._dv("B1", (2 * H,))),
                "layers.3.weight": c(self._dv("W2", (H, 2 * H))), "layers.3.bias": c(self._dv("B2", (H,))),
                "layers.6.weight": c(self._dv("W3", (H // 2, H))), "layers.6.bias": c(self._dv("B3", (H // 2,))),
                "layers.9.weight": c(self._dv("W4", (1, H // 2))), "layers.9.bias": c(self._dv("B4", (1,)))}

    # ------------------------------------------------------------------ steps
    def _opt(self, t):
        o = _lib.Opt()
        o.kind = OPT_KINDS[self.opt_kind]
        o.lr, o.beta1, o.beta2 = self.lr, self.betas[0], self.betas[1]
        o.eps, o.weight_decay, o.alpha = self.eps, 0.0, self.alpha    # CGANs.py:153-162: weight_decay=0
        o.one_minus_beta1, o.one_minus_beta2, o.one_minus_alpha = 1 - self.betas[0], 1 - self.betas[1], 1 - self.alpha
        if self.opt_kind == "adam":
            o.step_size = self.lr / (1 - self.betas[0] ** t)
            o.bias_correction2_sqrt = math.sqrt(1 - self.betas[1] ** t)
        return o

    def _model(self):
        m = _lib.GANModel()
        m.dims = self.dims
        m.g, m.g_m, m.g_v = ptr(self.g), ptr(self.g_m), ptr(self.g_v)
        m.d, m.d_m, m.d_v = ptr(self.d), ptr(self.d_m), ptr(self.d_v)
        return m

    def _noise(self, rows, z, masks):
        if z is None:
            z = torch.rand(rows, self.Z, device=self.device)
        z = z.to(self.device, torch.float32).contiguous()
        n = _lib.GANNoise()
        n.z = ptr(z)
        keep = [z]
        if masks is not None:
            for i, m in enumerate(masks):
                mt = torch.as_tensor(m).to(self.device, torch.uint8).contiguous()
                keep.append(mt)
                n.masks[i] = mt.data_ptr()
        self.seed += 1
        n.seed = self.seed
        return n, keep

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def check_batch(self, batch):
        if batch.rows > self.batch_max:
            raise ValueError(f"batch of {batch.rows} rows exceeds batch_max {self.batch_max}")

    def d_step(self, batch, z=None, masks=None):
        """CGAN.train_discriminator_iteration.  Returns the device tensor
        [d_loss, mean D(real), mean D(fake)] (no host sync)."""
        self.check_batch(batch)
        if batch.slates is None:
            raise ValueError("the discriminator step needs the batch's real slates")
        noise, keep = self._noise(batch.rows, z, masks)
        self.d_steps += 1
        out = torch.empty(3, dtype=torch.float32, device=self.device)
        b = batch.c_struct()
        check(self.lib.rg_gan_d_step(self._stream(), ctypes.byref(self._model()), ptr(self.ws), ctypes.byref(b),
                                     ctypes.byref(noise), ctypes.byref(self._opt(self.d_steps)), ptr(out)),
              "rg_gan_d_step")
        self.bn_tracked = [t + 1 for t in self.bn_tracked]
        self._keep = keep
        return out

    def g_step(self, batch, z=None, masks=None, slates=True):
        """CGAN.train_generator_iteration.  Returns (device [g_loss], slates (rows, S) float
        of the eval-mode generator on the same z after the step, or None)."""
        self.check_batch(batch)
        noise, keep = self._noise(batch.rows, z, masks)
        self.g_steps += 1
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        sl = torch.empty(batch.rows, self.S, dtype=torch.float32, device=self.device) if slates else None
        b = batch.c_struct()
        check(self.lib.rg_gan_g_step(self._stream(), ctypes.byref(self._model()), ptr(self.ws), ctypes.byref(b),
                                     ctypes.byref(noise), ctypes.byref(self._opt(self.g_steps)), ptr(out), ptr(sl)),
              "rg_gan_g_step")
        self.bn_tracked = [t + 1 for t in self.bn_tracked]
        self._keep = keep
        return out, sl

    def generate(self, batch, z=None):
        """generator.forward(z, hist, inference=True): (rows, S) float item ids."""
        self.check_batch(batch)
        if z is None:
            z = torch.rand(batch.rows, self.Z, device=self.device)
        z = z.to(self.device, torch.float32).contiguous()
        sl = torch.empty(batch.rows, self.S, dtype=torch.float32, device=self.device)
        b = batch.c_struct()
        check(self.lib.rg_gan_generate(self._stream(), ctypes.byref(self._model()), ptr(self.ws), ctypes.byref(b),
                                       ptr(z), ptr(sl)), "rg_gan_generate")
        self._keep = [z]
        return sl

    def generate_slates(self, hist):
        """The eval-mode generator's slates of every row of ``hist`` (device int32 (users, L),
        ids in [0, N], N = padding; the caller has checked the range), as a device int32
        (users, S) tensor: one ``torch.rand(rows, Z)`` and one rg_gan_generate per consecutive
        block of at most ``batch_max`` rows, in order (the draws ``CGAN.test`` always made, so a
        seed gives the same slates).  The batch descriptor carries only the rows, the history
        width and a pointer into ``hist``: inference reads nothing else of a batch.  No host
        synchronisation."""
        if hist.dtype != torch.int32 or hist.dim() != 2 or hist.device != self.device or not hist.is_contiguous():
            raise ValueError("hist must be a contiguous int32 (users, L) tensor on the engine's device")
        users, L = hist.shape
        sl = torch.empty(users, self.S, dtype=torch.float32, device=self.device)
        model, stream = self._model(), self._stream()
        b = _lib.GANBatch()
        b.hist_len = L
        for r0 in range(0, users, self.batch_max):
            rows = min(self.batch_max, users - r0)
            z = torch.rand(rows, self.Z, device=self.device)
            b.rows = rows
            b.hist = ctypes.c_void_p(hist.data_ptr() + r0 * L * 4)
            check(self.lib.rg_gan_generate(stream, ctypes.byref(model), ptr(self.ws), ctypes.byref(b), ptr(z),
                                           ctypes.c_void_p(sl.data_ptr() + r0 * self.S * 4)), "rg_gan_generate")
        return sl.to(torch.int32)

    def recommend_slates(self, hist, exclude_history=True, distinct=True, z=None, path=0):
        """Slates to serve (rg_gan_recommend) for every row of ``hist`` (device int32 (users, L),
        ids in [0, N], N = padding, as for ``generate_slates``): the heads are taken in order,
        each the best item of its tanh outputs (equal values: the lower id) that is not in the
        row's history (``exclude_history``) and not already in the row's slate (``distinct``); a
        slot with no item left holds N.  With both off these are ``generate_slates``' ids.  One
        ``torch.rand(rows, Z)`` and one call per consecutive block of at most ``batch_max`` rows,
        in order, or the rows of ``z`` (device float32 (users, Z)) when given.  ``path``: 0 the
        library's pick, 1 the stored path, 2 the fused one (a test and measurement selector).
        The scratch is allocated once per engine.  Returns a device int32 (users, S) tensor; no
        host synchronisation."""
        if hist.dtype != torch.int32 or hist.dim() != 2 or hist.device != self.device or not hist.is_contiguous():
            raise ValueError("hist must be a contiguous int32 (users, L) tensor on the engine's device")
        users, L = hist.shape
        if z is not None:
            if z.dtype != torch.float32 or z.shape != (users, self.Z) or z.device != self.device or \
                    not z.is_contiguous():
                raise ValueError("z must be a contiguous float32 (users, Z) tensor on the engine's device")
        flags = (_lib.GAN_REC_EXCLUDE_HISTORY if exclude_history else 0) | (_lib.GAN_REC_DISTINCT if distinct else 0)
        if self._rec_scratch is None:
            n = int(self.lib.rg_gan_recommend_scratch_bytes(ctypes.byref(self.dims), 0))
            if n < 0:
                check(1, "rg_gan_recommend_scratch_bytes")
            self._rec_scratch = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device)
        sl = torch.empty(users, self.S, dtype=torch.int32, device=self.device)
        model, stream = self._model(), self._stream()
        b = _lib.GANBatch()
        b.hist_len = L
        for r0 in range(0, users, self.batch_max):
            rows = min(self.batch_max, users - r0)
            zb = torch.rand(rows, self.Z, device=self.device) if z is None else z[r0:r0 + rows]
            b.rows = rows
            b.hist = ctypes.c_void_p(hist.data_ptr() + r0 * L * 4)
            check(self.lib.rg_gan_recommend(stream, ctypes.byref(model), ptr(self.ws), ctypes.byref(b), ptr(zb),
                                            flags, int(path), ptr(self._rec_scratch),
                                            ctypes.c_void_p(sl.data_ptr() + r0 * self.S * 4)), "rg_gan_recommend")
        return sl

    def score_slates(self, hist, slates, out=None):
        """The critic's eval-mode score of each row's slate (rg_gan_score_slates): ``hist`` device
        int32 (rows, L) and ``slates`` device int32 (rows, >= S), both contiguous; columns of
        ``slates`` from S on are not read.  History and slate ids outside [0, N) -- the padding
        id N included -- select nothing and are never used as an index.  The discriminator's
        parameters are read as stored (not clamped) and left untouched.  Any number of rows, one
        launch, no workspace.  Returns a float32 (rows,) device tensor (``out`` when given) on
        the current stream; no host synchronisation."""
        for name, t in (("hist", hist), ("slates", slates)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.device != self.device or \
                    not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous int32 2-d tensor on the engine's device")
        rows, L = hist.shape
        if slates.shape[0] != rows:
            raise ValueError(f"hist has {rows} rows, slates {slates.shape[0]}")
        if slates.shape[1] < self.S:
            raise ValueError(f"slates must have at least slate_size = {self.S} columns")
        if L < 1:
            raise ValueError("hist must have at least one column")
        if out is None:
            out = torch.empty(rows, dtype=torch.float32, device=self.device)
        elif not torch.is_tensor(out) or out.dtype != torch.float32 or out.shape != (rows,) or \
                out.device != self.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 (rows,) tensor on the engine's device")
        if rows == 0:       # an empty tensor has no pointer to hand over
            return out
        check(self.lib.rg_gan_score_slates(self._stream(), ctypes.byref(self._model()), ptr(hist), L, ptr(slates),
                                           slates.shape[1], rows, ptr(out)), "rg_gan_score_slates")
        return out

    def slate_hits(self, hist, tgt_ptr, tgt_idx, k, out=None):
        """Generates a slate for every row of ``hist`` (``generate_slates``) and marks, with one
        rg_slate_hits launch over all rows, which of each slate's first k items are among the
        row's held-out items: ``tgt_ptr`` (device int64, users + 1) and ``tgt_idx`` (device
        int32) are the users' CSR.  Returns the device int32 tensor of masks (``out`` when
        given): bit j of a row's word is set iff slate position j is a target and holds the
        item's first occurrence in the slate, so the word's popcount is
        len(set(slate[:k]) & set(targets)).  No host synchronisation."""
        return slate_hits(self.generate_slates(hist), tgt_ptr, tgt_idx, k, out=out)

    def workspace_view(self, which, shape):
        off = int(self.lib.rg_gan_workspace_offset(ctypes.byref(self.dims), which))
        n = int(np.prod(shape))
        return self.ws[off:off + 4 * n].view(torch.float32).view(shape)

    def last_fake(self, rows):
        """G(z) of the last step, (rows, S*N)."""
        return self.workspace_view(_lib.GAN_WS_FAKE, (rows, self.ks))[:, :self.S * self.N]

    def last_a2(self, rows):
        """The heads' input of the last generator forward, (rows, H)."""
        return self.workspace_view(_lib.GAN_WS_A2, (rows, self.H))

    def last_d_out(self, rows):
        return self.workspace_view(_lib.GAN_WS_DOUT, (rows,))
