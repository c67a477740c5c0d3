"""Device calls of the pooling sequence model (csrc/rg_seq.hip; include/rg_hip.h states the model):
the fused step's gradients, the dense Adam pass, the final representations and the raw score
block, plus the chain of torch ops they replace (``pool_loss_torch`` / ``pool_repr_torch``: the
timing baseline of ``eval_time --metric seq_pool``), and the same for the causal-convolution model
(csrc/rg_seq_cnn.hip: ``cnn_grads``, ``cnn_repr``, ``adam_flat``, the configuration and parameter
packing, ``cnn_loss_torch`` / ``cnn_repr_torch``).

Ids are int64 tensors on the tables' device.  Every id is range-checked here before a launch (one
download of the bounds; ``checked=True``: the caller has done it), and the kernels read an id
outside the table as padding, so no call indexes outside a table either way."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import LOSS_KINDS, OPT_KINDS, check, ptr

SEQ_LOSSES = ("bpr", "hinge", "adaptive_hinge")
SEQ_MAX_LEN, SEQ_MAX_NEG = 1024, 16        # include/rg_hip.h RG_SEQ_MAX_LEN / RG_SEQ_MAX_NEG
POINTWISE_REFUSAL = ("the sequence model has no pointwise loss: the reference's pointwise_loss takes "
                     "probabilities (it feeds BCELoss) while the sequence nets return raw scores, and it drops "
                     "the padding mask; use 'bpr', 'hinge' or 'adaptive_hinge'")


def check_loss(loss):
    if loss == "pointwise":
        raise ValueError(POINTWISE_REFUSAL)
    if loss not in SEQ_LOSSES:
        raise ValueError(f"loss must be one of {SEQ_LOSSES}, not {loss!r}")


def check_dim(dim):
    if dim < 4 or dim > 256 or dim % 4:
        raise ValueError(f"embedding_dim must be a multiple of 4 in [4, 256], not {dim}")


def check_ids(ids, num_items, what):
    """ValueError unless every id of the tensor / array lies in [0, num_items)."""
    if isinstance(ids, torch.Tensor):
        if not ids.numel():
            return
        lo, hi = torch.stack(ids.aminmax()).tolist()
    else:
        ids = np.asarray(ids)
        if not ids.size:
            return
        lo, hi = int(ids.min()), int(ids.max())
    if lo < 0:
        raise ValueError(f"{what}: negative item id")
    if hi >= num_items:
        raise ValueError(f"{what}: maximum item id greater than number of items in model")


def _tables_ok(E, b):
    return E.is_cuda and b.is_cuda and E.device == b.device and E.dtype == b.dtype == torch.float32 and \
        E.is_contiguous() and b.is_contiguous() and E.dim() == 2 and b.numel() == E.shape[0]


def _ids(x, dev):
    return torch.as_tensor(x).to(dev, torch.int64).contiguous()


def pool_grads(E, b, seq, neg, loss, grad=None, mask_count=None, checked=False):
    """One step's loss (0-d tensor on the device) and gradient buffer [num_items, d + 1] (columns
    [0, d): d loss / d E, column d: d loss / d b; float atomic adds, so its last bits differ from
    run to run) of sequences ``seq`` [B, L] with negatives ``neg`` [K, B, L]: rg_seq_pool_grads.
    ``grad`` must be zero on entry (a new one is made when None).  ``mask_count`` = (seq != 0).sum()
    when the caller has it; a batch of padding alone is refused before any launch."""
    check_loss(loss)
    if E.dim() != 2 or b.numel() != E.shape[0]:
        raise ValueError("pool_grads: E must be [num_items, d] and b [num_items]")
    num_items, dim = int(E.shape[0]), int(E.shape[1])
    check_dim(dim)
    seq, neg = torch.as_tensor(seq), torch.as_tensor(neg)
    if seq.dim() != 2 or neg.dim() != 3 or tuple(neg.shape[1:]) != tuple(seq.shape):
        raise ValueError("pool_grads: seq must be [B, L] and neg [K, B, L]")
    B, L = (int(x) for x in seq.shape)
    K = int(neg.shape[0])
    if not (1 <= L <= SEQ_MAX_LEN and 1 <= K <= SEQ_MAX_NEG and B >= 1):
        raise ValueError(f"pool_grads: needs B >= 1, 1 <= L <= {SEQ_MAX_LEN}, 1 <= K <= {SEQ_MAX_NEG}")
    if not checked:
        check_ids(seq, num_items, "sequences")
        check_ids(neg, num_items, "negatives")
    if mask_count is None:
        mask_count = int((seq != 0).sum())
    if mask_count <= 0:
        raise ValueError("pool_grads: the batch holds padding only (mask.sum() == 0)")
    if not _tables_ok(E, b):
        raise ValueError("pool_grads needs contiguous float32 tables E [num_items, d], b [num_items] on one CUDA device")
    dev = E.device
    seq, neg = _ids(seq, dev), _ids(neg, dev)
    if grad is None:
        grad = torch.zeros(num_items, dim + 1, dtype=torch.float32, device=dev)
    elif grad.shape != (num_items, dim + 1) or grad.dtype != torch.float32 or not grad.is_contiguous() or \
            grad.device != dev:
        raise ValueError("pool_grads: grad must be a contiguous float32 [num_items, d + 1] on the tables' device")
    lib = _lib.load()
    ws = torch.empty(int(lib.rg_seq_pool_workspace_len(B, L, K)), dtype=torch.float32, device=dev)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.rg_seq_pool_grads(_lib.stream_handle(), ptr(seq), ptr(neg), ptr(E), ptr(b), dim, num_items, B, L, K,
                                    LOSS_KINDS[loss], 1.0 / float(mask_count), ptr(grad), ptr(ws), ptr(out)),
              "rg_seq_pool_grads")
    return out[0], grad


def adam_opt(step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """rg_opt_t of torch.optim.Adam's step ``step`` (1-based): the scalars evaluated in double as
    its Python code does."""
    o = _lib.Opt()
    o.kind = OPT_KINDS["adam"]
    o.lr, o.beta1, o.beta2, o.eps, o.weight_decay = lr, betas[0], betas[1], eps, weight_decay
    o.one_minus_beta1, o.one_minus_beta2 = 1 - betas[0], 1 - betas[1]
    o.step_size = float(lr) / (1.0 - float(betas[0]) ** step)
    o.bias_correction2_sqrt = (1.0 - float(betas[1]) ** step) ** 0.5
    return o


def adam_dense(E, b, mE, vE, mb, vb, grad, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam's step ``step`` on every row but row 0, in place, from ``grad``
    [num_items, d + 1], which is zeroed for the next step: rg_seq_adam_dense."""
    tabs = (E, mE, vE)
    vecs = (b, mb, vb)
    num_items, dim = int(E.shape[0]), int(E.shape[1])
    if not (_tables_ok(E, b) and all(t.shape == E.shape and _tables_ok(t, v) for t, v in zip(tabs, vecs)) and
            grad.shape == (num_items, dim + 1) and grad.is_cuda and grad.dtype == torch.float32 and
            grad.is_contiguous() and grad.device == E.device):
        raise ValueError("adam_dense needs contiguous float32 tables, moments and grad [num_items, d + 1] on one "
                         "CUDA device")
    o = adam_opt(step, lr, betas, eps, weight_decay)
    with torch.cuda.device(E.device):
        check(_lib.load().rg_seq_adam_dense(_lib.stream_handle(), ptr(E), ptr(b), ptr(mE), ptr(vE), ptr(mb), ptr(vb),
                                            ptr(grad), dim, num_items, ctypes.byref(o)), "rg_seq_adam_dense")


def pool_repr(E, ids, seq_ptr=None, checked=False):
    """The final representations r_L [n, d] (device) of a padded [n, L] block of ids, or, with
    ``seq_ptr`` [n + 1], of the ragged sequences ids[seq_ptr[r] : seq_ptr[r + 1]]:
    rg_seq_pool_repr."""
    if not (E.is_cuda and E.dtype == torch.float32 and E.is_contiguous() and E.dim() == 2):
        raise ValueError("pool_repr needs a contiguous float32 table on a CUDA device")
    num_items, dim = int(E.shape[0]), int(E.shape[1])
    check_dim(dim)
    dev = E.device
    ids = _ids(ids, dev)
    if seq_ptr is None:
        if ids.dim() != 2:
            raise ValueError("pool_repr: a padded block must be [n, L]")
        n, L = (int(x) for x in ids.shape)
        if L > SEQ_MAX_LEN:
            raise ValueError(f"pool_repr: L must be at most {SEQ_MAX_LEN}")
        p = None
    else:
        p = np.asarray(seq_ptr.cpu() if isinstance(seq_ptr, torch.Tensor) else seq_ptr, dtype=np.int64)
        if p.ndim != 1 or len(p) < 1 or p[0] != 0 or (np.diff(p) < 0).any() or p[-1] != ids.numel() or ids.dim() != 1:
            raise ValueError("pool_repr: seq_ptr must ascend from 0 to len(ids)")
        n, L = len(p) - 1, 0
        p = torch.from_numpy(p).to(dev)
    if not checked:
        check_ids(ids, num_items, "sequences")
    out = torch.empty(n, dim, dtype=torch.float32, device=dev)
    if not ids.numel():                 # empty sequences only: nothing is read through ids
        ids = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().rg_seq_pool_repr(_lib.stream_handle(), ptr(E), dim, num_items, ptr(ids),
                                           ptr(p), L, n, ptr(out)), "rg_seq_pool_repr")
    return out


def score_block_raw(R, E, b):
    """Raw scores (R @ E.T + b) [n, num_items] of representations R [n, d]: rg_mf_score_users_raw
    with R as the user table, arange ids and a zero user bias (the fp32-MFMA score block without
    its sigmoid)."""
    if not (_tables_ok(E, b) and R.is_cuda and R.device == E.device and R.dtype == torch.float32 and
            R.is_contiguous() and R.dim() == 2 and R.shape[1] == E.shape[1]):
        raise ValueError("score_block_raw needs contiguous float32 R [n, d], E [num_items, d], b [num_items] on one "
                         "CUDA device")
    n, num_items, dev = int(R.shape[0]), int(E.shape[0]), E.device
    out = torch.empty(n, num_items, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    users = torch.arange(n, dtype=torch.int64, device=dev)
    zero = torch.zeros(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().rg_mf_score_users_raw(_lib.stream_handle(), ptr(R), ptr(E), ptr(zero), ptr(b), int(E.shape[1]),
                                                num_items, ptr(users), n, ptr(out), num_items),
              "rg_mf_score_users_raw")
    return out


# ------------------------------------------------------------------ the chain of torch ops
def pool_reprs_torch(E, seq):
    """(r_0 .. r_{L-1} as [B, L, d], r_L as [B, d]) of a padded block, padding counted per id."""
    emb = E[seq]                                                        # [B, L, d]
    zero = torch.zeros_like(emb[:, :1])
    S = torch.cat([zero, torch.cumsum(emb, 1)], 1)                      # S_t, t = 0 .. L
    c = torch.cat([torch.zeros_like(seq[:, :1]), torch.cumsum((seq != 0).to(seq.dtype), 1)], 1)
    r = S / (c + 1).to(E.dtype)[:, :, None]
    return r[:, :-1], r[:, -1]


def pool_loss_torch(E, b, seq, neg, loss):
    """The step's loss as torch ops on the given tables (any dtype / device): what autograd
    differentiates in the tests' oracle and what ``eval_time --metric seq_pool`` times."""
    from .spotlight.losses import LOSS_FUNCTIONS
    check_loss(loss)
    r, _ = pool_reprs_torch(E, seq)
    zp = b[seq] + (r * E[seq]).sum(-1)
    zn = b[neg] + (r[None] * E[neg]).sum(-1)
    if loss == "adaptive_hinge":    # adaptive_hinge_loss without its squeeze(), which folds a [B, 1] batch
        loss, zn = "hinge", zn.max(0).values
    return LOSS_FUNCTIONS[loss](zp, zn, mask=(seq != 0))


# ------------------------------------------------------------------ the causal-convolution model
NONLINEARITY_KINDS = {"tanh": 0, "relu": 1}


def cnn_config(dim, widths, dilations, nonlinearity="tanh", residual=True):
    """rg_seq_cnn_t of a stack of ``len(widths)`` layers; ValueError for what the kernels refuse."""
    widths, dilations = tuple(int(w) for w in widths), tuple(int(x) for x in dilations)
    if dim < 16 or dim > 128 or dim % 16:
        raise ValueError(f"the convolution kernels take an embedding_dim that is a multiple of 16 in [16, 128], "
                         f"not {dim}")
    if not 1 <= len(widths) <= _lib.SEQ_CNN_MAX_LAYERS or len(dilations) != len(widths):
        raise ValueError(f"num_layers must be in [1, {_lib.SEQ_CNN_MAX_LAYERS}], one width and dilation per layer")
    if min(widths) < 1 or max(widths) > _lib.SEQ_CNN_MAX_WIDTH:
        raise ValueError(f"every kernel width must be in [1, {_lib.SEQ_CNN_MAX_WIDTH}]")
    if min(dilations) < 1 or max(dilations) > 64:
        raise ValueError("every dilation must be in [1, 64]")
    if nonlinearity not in NONLINEARITY_KINDS:
        raise ValueError("Nonlinearity must be one of (tanh, relu)")
    cfg = _lib.SeqCnn()
    cfg.dim, cfg.num_layers = int(dim), len(widths)
    cfg.nonlinearity, cfg.residual = NONLINEARITY_KINDS[nonlinearity], int(bool(residual))
    for l, (w, x) in enumerate(zip(widths, dilations)):
        cfg.width[l], cfg.dilation[l] = w, x
    return cfg


def cnn_config_of(net):
    """rg_seq_cnn_t of a ``representations.CNNNet``."""
    return cnn_config(net.embedding_dim, net.kernel_width, net.dilation, net.nonlinearity_name,
                      net.residual_connections)


def cnn_param_len(cfg):
    return sum((cfg.width[l] * cfg.dim + 1) * cfg.dim for l in range(cfg.num_layers))


def cnn_pack(cfg, layers):
    """The flat parameter vector of ``layers`` = [(weight [d, d, w, 1], bias [d]), ...] in the
    reference's Conv2d layout: per layer W as [w][d in][d out], then the bias.  A pure permutation:
    ``cnn_unpack`` returns the same bits."""
    parts = []
    for l, (W, c) in enumerate(layers):
        W, c = torch.as_tensor(W), torch.as_tensor(c)
        if tuple(W.shape) != (cfg.dim, cfg.dim, cfg.width[l], 1) or tuple(c.shape) != (cfg.dim,):
            raise ValueError(f"layer {l}: weight must be [d, d, {cfg.width[l]}, 1] and bias [d]")
        parts += [W[:, :, :, 0].permute(2, 1, 0).reshape(-1), c.reshape(-1)]
    if len(layers) != cfg.num_layers:
        raise ValueError("one (weight, bias) per layer")
    return torch.cat(parts).to(torch.float32).contiguous()


def cnn_unpack(cfg, params):
    """[(weight [d, d, w, 1], bias [d]), ...] of a flat parameter vector (any dtype / device)."""
    out, o, d = [], 0, cfg.dim
    for l in range(cfg.num_layers):
        w = cfg.width[l]
        W = params[o:o + w * d * d].reshape(w, d, d).permute(2, 1, 0).unsqueeze(3)
        o += w * d * d
        out.append((W, params[o:o + d]))
        o += d
    return out


def _flat_ok(p, dev, n=None):
    return p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.is_contiguous() and p.dim() == 1 and \
        (n is None or p.numel() == n)


def cnn_workspace(cfg, B, L, K, device):
    """The float32 workspace of ``cnn_grads`` for these shapes (rg_seq_cnn_workspace_len floats)."""
    n = int(_lib.load().rg_seq_cnn_workspace_len(ctypes.byref(cfg), B, L, K))
    if n < 0:
        raise ValueError("cnn_workspace: unsupported configuration or shapes")
    return torch.empty(n, dtype=torch.float32, device=device)


def cnn_grads(cfg, E, b, params, seq, neg, loss, grad=None, mask_count=None, checked=False, param_grad=None,
              workspace=None):
    """One step's loss (0-d device tensor), the item gradient buffer [num_items, d + 1] (as
    ``pool_grads``) and the convolution parameters' gradient [param_len] (written in a fixed order:
    the same bits on every run) under the causal-convolution representation: rg_seq_cnn_grads.
    ``param_grad`` (overwritten) and ``workspace`` (``cnn_workspace`` of at least these shapes) are
    reused when given, so a training loop allocates neither per step."""
    check_loss(loss)
    if E.dim() != 2 or b.numel() != E.shape[0] or E.shape[1] != cfg.dim:
        raise ValueError("cnn_grads: E must be [num_items, d] and b [num_items], d the configuration's")
    num_items, dim = int(E.shape[0]), int(E.shape[1])
    seq, neg = torch.as_tensor(seq), torch.as_tensor(neg)
    if seq.dim() != 2 or neg.dim() != 3 or tuple(neg.shape[1:]) != tuple(seq.shape):
        raise ValueError("cnn_grads: seq must be [B, L] and neg [K, B, L]")
    B, L = (int(x) for x in seq.shape)
    K = int(neg.shape[0])
    if not (1 <= L <= SEQ_MAX_LEN and 1 <= K <= SEQ_MAX_NEG and B >= 1):
        raise ValueError(f"cnn_grads: needs B >= 1, 1 <= L <= {SEQ_MAX_LEN}, 1 <= K <= {SEQ_MAX_NEG}")
    if not checked:
        check_ids(seq, num_items, "sequences")
        check_ids(neg, num_items, "negatives")
    if mask_count is None:
        mask_count = int((seq != 0).sum())
    if mask_count <= 0:
        raise ValueError("cnn_grads: the batch holds padding only (mask.sum() == 0)")
    if not _tables_ok(E, b) or not _flat_ok(params, E.device, cnn_param_len(cfg)):
        raise ValueError("cnn_grads needs contiguous float32 tables E [num_items, d], b [num_items] and a flat "
                         "parameter vector of cnn_param_len floats on one CUDA device")
    dev = E.device
    seq, neg = _ids(seq, dev), _ids(neg, dev)
    if grad is None:
        grad = torch.zeros(num_items, dim + 1, dtype=torch.float32, device=dev)
    elif grad.shape != (num_items, dim + 1) or grad.dtype != torch.float32 or not grad.is_contiguous() or \
            grad.device != dev:
        raise ValueError("cnn_grads: grad must be a contiguous float32 [num_items, d + 1] on the tables' device")
    lib = _lib.load()
    need = int(lib.rg_seq_cnn_workspace_len(ctypes.byref(cfg), B, L, K))
    if need < 0:
        raise ValueError("cnn_grads: too many positions for one call")
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.float32, device=dev)
    pgrad = param_grad if param_grad is not None else torch.empty_like(params)
    if not _flat_ok(ws, dev) or ws.numel() < need or not _flat_ok(pgrad, dev, params.numel()):
        raise ValueError("cnn_grads: workspace and param_grad must be contiguous float32 vectors on the tables' "
                         "device, of cnn_workspace's and the parameters' length")
    out = torch.empty(1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.rg_seq_cnn_grads(_lib.stream_handle(), ctypes.byref(cfg), ptr(seq), ptr(neg), ptr(E), ptr(b),
                                   ptr(params), num_items, B, L, K, LOSS_KINDS[loss], 1.0 / float(mask_count),
                                   ptr(grad), ptr(pgrad), ptr(ws), ptr(out)), "rg_seq_cnn_grads")
    return out[0], grad, pgrad


def cnn_repr(cfg, E, params, ids, checked=False):
    """The final representations x_L [n, d] (device) of a padded [n, L] block of ids:
    rg_seq_cnn_repr."""
    if not (E.is_cuda and E.dtype == torch.float32 and E.is_contiguous() and E.dim() == 2 and
            E.shape[1] == cfg.dim and _flat_ok(params, E.device, cnn_param_len(cfg))):
        raise ValueError("cnn_repr needs a contiguous float32 table [num_items, d] and the flat parameter vector on "
                         "one CUDA device")
    num_items, dim, dev = int(E.shape[0]), int(E.shape[1]), E.device
    ids = _ids(ids, dev)
    if ids.dim() != 2:
        raise ValueError("cnn_repr: a padded block must be [n, L]")
    n, L = (int(x) for x in ids.shape)
    if L > SEQ_MAX_LEN:
        raise ValueError(f"cnn_repr: L must be at most {SEQ_MAX_LEN}")
    if not checked:
        check_ids(ids, num_items, "sequences")
    lib = _lib.load()
    out = torch.empty(n, dim, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    ws_len = int(lib.rg_seq_cnn_repr_workspace_len(ctypes.byref(cfg), n, L))
    ws = torch.empty(ws_len, dtype=torch.float32, device=dev) if ws_len > 0 else None
    if not ids.numel():
        ids = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.rg_seq_cnn_repr(_lib.stream_handle(), ctypes.byref(cfg), ptr(E), ptr(params), num_items, ptr(ids),
                                  L, n, ptr(ws), ptr(out)), "rg_seq_cnn_repr")
    return out


def adam_flat(p, m, v, g, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam's step ``step`` on the flat vector ``p`` in place, from its gradient ``g``
    (not changed): rg_seq_adam_flat."""
    if not (p.dim() == 1 and p.is_cuda and all(_flat_ok(t, p.device, p.numel()) for t in (p, m, v, g))):
        raise ValueError("adam_flat needs contiguous float32 vectors of one length on one CUDA device")
    o = adam_opt(step, lr, betas, eps, weight_decay)
    with torch.cuda.device(p.device):
        check(_lib.load().rg_seq_adam_flat(_lib.stream_handle(), ptr(p), ptr(m), ptr(v), ptr(g), p.numel(),
                                           ctypes.byref(o)), "rg_seq_adam_flat")


def cnn_reprs_torch(cfg, E, params, seq):
    """x_0 .. x_L of the top layer, [B, L + 1, d], as torch ops on the given tables (any dtype /
    device): the chain ``eval_time --metric seq_cnn`` times and autograd differentiates."""
    import torch.nn.functional as F
    f = torch.tanh if cfg.nonlinearity == 0 else F.relu
    emb = F.embedding(seq, E, padding_idx=0)                                       # [B, L, d]
    x = F.pad(emb, (0, 0, 1, 0)).transpose(1, 2).unsqueeze(3)                      # u_0 .. u_L: [B, d, L + 1, 1]
    for l, (W, c) in enumerate(cnn_unpack(cfg, params)):
        y = f(F.conv2d(F.pad(x, (0, 0, (cfg.width[l] - 1) * cfg.dilation[l], 0)), W, c,
                       dilation=(cfg.dilation[l], 1)))
        x = y + x if cfg.residual else y
    return x.squeeze(3).transpose(1, 2)


def cnn_repr_torch(cfg, E, params, seq):
    return cnn_reprs_torch(cfg, E, params, seq)[:, -1]


def cnn_loss_torch(cfg, E, b, params, seq, neg, loss):
    """The step's loss as torch ops (see ``pool_loss_torch``)."""
    from .spotlight.losses import LOSS_FUNCTIONS
    check_loss(loss)
    r = cnn_reprs_torch(cfg, E, params, seq)[:, :-1]
    zp = b[seq] + (r * E[seq]).sum(-1)
    zn = b[neg] + (r[None] * E[neg]).sum(-1)
    if loss == "adaptive_hinge":
        loss, zn = "hinge", zn.max(0).values
    return LOSS_FUNCTIONS[loss](zp, zn, mask=(seq != 0))
