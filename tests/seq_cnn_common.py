"""What the causal-convolution sequence model's tests share (no tests here): the model of
include/rg_hip.h (rg_seq_cnn_grads) stated in torch on the CPU with explicit shifted rows (not
conv2d: a statement independent of ``seq_engine.cnn_reprs_torch`` and of the reference), autograd
gradients in float64 (the reference of every comparison) and float32 (E32); the covering case
list; the fixture recorded from the reference's CNNNet.  Sequences, negatives and the edge
builders are seq_common's, the constants fold_in_common's.

The gradient rule is the project's: |kernel - float64| <= 2 E32 + CANCEL * sum |terms| per element
of dE, db and the convolutions' parameter gradient.  The sum of |terms| comes from one manual
backward pass in float64 run on magnitudes: the backward pass is linear in dz, every path from a
dz to a gradient element is a product of dz, entries of E and W, activations and f', so the same
pass with |dz|, |E|, |x|, |W| and |f'| sums the magnitudes of all path products (seq_common's
non-negative-coefficient argument does not carry through tanh, whose f' multiplies signed sums).

Kink margins are ``seq_common``'s (a hinge argument near 0, an adaptive hinge's two highest
negatives near each other) under this model's scores, plus the smallest |pre-activation| of any
relu unit; test_seq_cnn_cpu.py checks that no case has one within ``fold_in_common.TIE``.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from recommendation_gans_amd import seq_engine
from tests import fold_in_common as fc
from tests import seq_common as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_cnn_d16.npz")

# name: (widths, dilations, nonlinearity, residual)
NETS = {
    "A": ((3,), (1,), "tanh", True),
    "B": ((3, 2), (1, 2), "relu", True),
    "C": ((2, 3, 3), (1, 2, 4), "tanh", False),
    "D": ((1,), (1,), "tanh", True),
    "E": ((8,), (4,), "relu", False),           # at L = 5 the taps lie mostly left of the sequence
    "F": ((3, 3, 2, 3), (1, 2, 4, 1), "tanh", True),
}
FIXTURE_NETS = ("A", "B", "C")

# (net, d, L, B, K, num_items, loss): d {16, 32, 48, 64, 128} (and one 96) x L {1, 2, 5, 33} x B {1, 3, 67} x
# K {1, 5} x items {7, 1000} x the losses; every d, L, net and loss at least twice.  B = 3, L = 5 is
# 18 rows (a partial MFMA row tile, tiles spanning sequences), B = 67, L = 33 is 2278.
CASES = [
    ("A", 16, 5, 3, 1, 7, "bpr"),
    ("A", 32, 33, 67, 5, 1000, "hinge"),
    ("A", 128, 2, 3, 5, 7, "adaptive_hinge"),
    ("A", 64, 1, 1, 1, 7, "hinge"),
    ("B", 16, 33, 67, 1, 1000, "bpr"),
    ("B", 32, 5, 3, 5, 7, "adaptive_hinge"),
    ("B", 48, 2, 67, 1, 1000, "hinge"),
    ("B", 128, 33, 3, 5, 1000, "bpr"),
    ("C", 16, 5, 67, 5, 7, "hinge"),
    ("C", 48, 33, 3, 1, 7, "adaptive_hinge"),
    ("C", 64, 33, 67, 5, 1000, "bpr"),
    ("C", 128, 1, 67, 1, 1000, "hinge"),
    ("D", 16, 2, 1, 5, 7, "adaptive_hinge"),
    ("D", 64, 5, 67, 1, 1000, "bpr"),
    ("D", 32, 1, 3, 5, 7, "hinge"),
    ("E", 16, 5, 3, 5, 1000, "bpr"),
    ("E", 64, 5, 67, 1, 7, "adaptive_hinge"),
    ("E", 32, 5, 1, 1, 1000, "hinge"),
    ("F", 16, 33, 3, 1, 1000, "adaptive_hinge"),
    ("F", 48, 5, 67, 5, 7, "bpr"),
    ("F", 128, 2, 1, 1, 7, "bpr"),
    ("F", 32, 2, 67, 5, 1000, "adaptive_hinge"),
    ("A", 48, 1, 67, 5, 1000, "bpr"),
    ("B", 64, 2, 3, 1, 7, "hinge"),
    # beyond the list: a dim between the power-of-two ones (six column tiles in the MFMA kernels,
    # the 64-lane scalar row layout in the score kernel)
    ("B", 96, 5, 3, 5, 1000, "hinge"),
]
CASE_IDS = ["%s-d%d-L%d-B%d-K%d-I%d-%s" % c for c in CASES]
# seeds chosen on the CPU (test_seq_cnn_cpu.py) so that no case has a kink margin within TIE
SEEDS = {}


def net_config(name, d):
    widths, dils, nonlin, residual = NETS[name]
    return seq_engine.cnn_config(d, widths, dils, nonlin, residual)


def make_params(cfg, rs, scale=0.8):
    """A flat parameter vector: weights of order scale / sqrt(w d), biases of order 0.1."""
    parts = []
    for l in range(cfg.num_layers):
        w, d = cfg.width[l], cfg.dim
        parts += [rs.randn(w * d * d) * scale / np.sqrt(w * d), rs.randn(d) * 0.1]
    return np.concatenate(parts).astype(np.float32)


def make_case(net, d, L, B, K, num_items, seed=0):
    case = sc.make_case(d, L, B, K, num_items, seed=seed)
    cfg = net_config(net, d)
    rs = np.random.RandomState(7919 * seed + 31 * d + L + sum(map(ord, net)))
    return dict(case, net=net, cfg=cfg, params=make_params(cfg, rs))


# ------------------------------------------------------------------ the model in torch
def taps(cfg, params):
    """[(W [w, d in, d out], c [d]), ...] views of the flat vector."""
    out, o, d = [], 0, cfg.dim
    for l in range(cfg.num_layers):
        w = cfg.width[l]
        out.append((params[o:o + w * d * d].reshape(w, d, d), params[o + w * d * d:o + (w * d + 1) * d]))
        o += (w * d + 1) * d
    return out


def layers_forward(cfg, E, params, seq):
    """(xs, ys): xs[0] the virtual input rows u_0 .. u_L [B, L + 1, d] (u_t = E[s_{t-1}], u_0 = 0),
    xs[l + 1] layer l's output, ys[l] its f(pre); E[0] never receives a gradient."""
    f = torch.tanh if cfg.nonlinearity == 0 else F.relu
    x = F.pad(F.embedding(seq, E, padding_idx=0), (0, 0, 1, 0))
    T = x.shape[1]
    xs, ys = [x], []
    for l, (W, c) in enumerate(taps(cfg, params)):
        pre = c.expand(x.shape[0], T, cfg.dim)
        for j in range(cfg.width[l]):
            shift = (cfg.width[l] - 1 - j) * cfg.dilation[l]
            if shift < T:
                pre = pre + F.pad(x[:, :T - shift], (0, 0, shift, 0)) @ W[j]
        y = f(pre)
        x = y + x if cfg.residual else y
        xs.append(x)
        ys.append(y)
    return xs, ys


def position_scores(cfg, E, b, params, seq, neg):
    r = layers_forward(cfg, E, params, seq)[0][-1][:, :-1]
    bias = b.reshape(-1, 1)
    zp = F.embedding(seq, bias, padding_idx=0)[..., 0] + (r * F.embedding(seq, E, padding_idx=0)).sum(-1)
    zn = F.embedding(neg, bias, padding_idx=0)[..., 0] + (r[None] * F.embedding(neg, E, padding_idx=0)).sum(-1)
    return zp, zn


def final_repr(cfg, E, params, seq):
    return layers_forward(cfg, E, params, seq)[0][-1][:, -1]


def final_scores(cfg, E, b, params, seq):
    return final_repr(cfg, E, params, seq) @ E.T + b[None, :]


def _abs_terms(cfg, E, params, seq, neg, xs, ys, dzp, dzn):
    """The sums of |terms| of dE, db and the parameter gradient: the backward pass on magnitudes
    (float64 numpy)."""
    N, d = E.shape
    B, L = seq.shape
    T = L + 1
    aE, ab, ap = np.zeros((N, d)), np.zeros(N), np.zeros(len(params))
    xt = np.abs(xs[-1][:, :-1])
    adzp, adzn = np.abs(dzp), np.abs(dzn)
    np.add.at(aE, seq, adzp[..., None] * xt)
    np.add.at(ab, seq, adzp)
    np.add.at(aE, neg, adzn[..., None] * xt[None])
    np.add.at(ab, neg, adzn)
    adx = np.zeros((B, T, d))
    adx[:, :-1] = adzp[..., None] * np.abs(E[seq]) + (adzn[..., None] * np.abs(E[neg])).sum(0)
    offs, o = [], 0
    for l in range(cfg.num_layers):
        offs.append(o)
        o += (cfg.width[l] * d + 1) * d
    for l in reversed(range(cfg.num_layers)):
        w, dil = cfg.width[l], cfg.dilation[l]
        W = np.abs(params[offs[l]:offs[l] + w * d * d].reshape(w, d, d))
        fp = np.abs(1.0 - ys[l] ** 2) if cfg.nonlinearity == 0 else (ys[l] > 0).astype(np.float64)
        adpre = adx * fp
        ap[offs[l] + w * d * d:offs[l] + (w * d + 1) * d] = adpre.sum((0, 1))
        adx_in = adx.copy() if cfg.residual else np.zeros_like(adx)
        aW = np.zeros((w, d, d))
        for j in range(w):
            shift = (w - 1 - j) * dil
            if shift < T:
                aW[j] = np.einsum("bti,bto->io", np.abs(xs[l][:, :T - shift]), adpre[:, shift:])
                adx_in[:, :T - shift] += adpre[:, shift:] @ W[j].T
        ap[offs[l]:offs[l] + w * d * d] = aW.reshape(-1)
        adx = adx_in
    np.add.at(aE, seq, adx[:, 1:])
    aE[0], ab[0] = 0.0, 0.0
    return aE, ab, ap


def grads(case, loss, dtype=torch.float64, abs_terms=False):
    """loss, dE, db, dparams by autograd; with ``abs_terms`` also their sums of |terms| and the
    smallest |pre-activation| proxy inputs of ``kink_margin``."""
    t = lambda a: torch.from_numpy(a)
    cfg = case["cfg"]
    E = t(case["E"]).to(dtype).requires_grad_(True)
    b = t(case["b"]).to(dtype).requires_grad_(True)
    p = t(case["params"]).to(dtype).requires_grad_(True)
    seq, neg = t(case["seq"]), t(case["neg"])
    zp, zn = position_scores(cfg, E, b, p, seq, neg)
    lv = sc.loss_of_scores(zp, zn, seq, loss)
    dzp, dzn = torch.autograd.grad(lv, [zp, zn], retain_graph=True)
    gE, gb, gp = torch.autograd.grad(lv, [E, b, p])
    out = dict(loss=float(lv.detach()), gE=gE.numpy(), gb=gb.numpy(), gp=gp.numpy())
    if abs_terms:
        with torch.no_grad():
            xs, ys = layers_forward(cfg, E, p, seq)
        aE, ab, ap = _abs_terms(cfg, E.detach().numpy(), p.detach().numpy(), case["seq"], case["neg"],
                                [x.numpy() for x in xs], [y.numpy() for y in ys], dzp.numpy(), dzn.numpy())
        out.update(aE=aE, ab=ab, ap=ap)
    return out


def kink_margin(case, loss):
    """float64 distance from the nearest kink: ``seq_common.kink_margin``'s hinge and adaptive
    hinge margins under this model's scores, and the smallest |pre-activation| of a relu unit."""
    t = lambda a: torch.from_numpy(a)
    cfg = case["cfg"]
    E, b, p = t(case["E"]).double(), t(case["b"]).double(), t(case["params"]).double()
    margin = np.inf
    if cfg.nonlinearity == 1:
        xs, _ = layers_forward(cfg, E, p, t(case["seq"]))
        x = xs[0]           # y = relu(pre) hides a negative pre: form pre again from the layers' inputs
        T = x.shape[1]
        for l, (W, c) in enumerate(taps(cfg, p)):
            pre = c.expand(x.shape[0], T, cfg.dim)
            for j in range(cfg.width[l]):
                shift = (cfg.width[l] - 1 - j) * cfg.dilation[l]
                if shift < T:
                    pre = pre + F.pad(x[:, :T - shift], (0, 0, shift, 0)) @ W[j]
            margin = min(margin, float(pre.abs().min()))
            x = xs[l + 1]
    if loss == "bpr":
        return margin
    zp, zn = position_scores(cfg, E, b, p, t(case["seq"]), t(case["neg"]))
    zp, zn, mask = zp.numpy(), zn.numpy(), case["seq"] != 0
    if loss == "hinge":
        return min(margin, float(np.abs(zn - zp[None] + 1.0)[:, mask].min(initial=np.inf)))
    top = zn.max(0)
    margin = min(margin, float(np.abs(top - zp + 1.0)[mask].min(initial=np.inf)))
    if case["K"] > 1:
        win = np.take_along_axis(case["neg"], zn.argmax(0)[None], 0)
        other = np.where(case["neg"] != win, zn, -np.inf).max(0)
        margin = min(margin, float((top - other)[mask].min(initial=np.inf)))
    return margin


def data_of(case, loss):
    r64 = grads(case, loss, torch.float64, abs_terms=True)
    r32 = grads(case, loss, torch.float32)
    e32 = max(float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in ("gE", "gb", "gp"))
    return dict(case=case, loss=loss, r64=r64, r32=r32, e32=e32)


@functools.lru_cache(maxsize=None)
def case_of(i):
    net, d, L, B, K, num_items, _ = CASES[i]
    return make_case(net, d, L, B, K, num_items, seed=SEEDS.get(i, 0))


@functools.lru_cache(maxsize=None)
def case_data(i):
    """Case i, computed once per process and shared (read-only)."""
    return data_of(case_of(i), CASES[i][6])


def gradient_excess(gE, gb, gp, data):
    """The largest |kernel - float64| / (2 E32 + CANCEL * sum |terms|) over the elements of dE, db
    and the parameter gradient (must be <= 1), and the plain largest |kernel - float64| / E32."""
    r64, e32 = data["r64"], data["e32"]
    worst = plain = 0.0
    for got, ref, a in ((gE, r64["gE"], r64["aE"]), (gb, r64["gb"], r64["ab"]), (gp, r64["gp"], r64["ap"])):
        err = np.abs(np.asarray(got, np.float64) - ref)
        bound = 2.0 * e32 + fc.CANCEL * a
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / bound, 0.0)
        worst = max(worst, float(ratio.max()))
        plain = max(plain, float(err.max()) / e32 if e32 > 0 else (0.0 if err.max() == 0 else np.inf))
    return worst, plain


# ------------------------------------------------------------------ the entries' edges
# (name, net, d, loss): seq_common's edge builders with a net's parameters
EDGE_CASES = [("scatter", "A", 16, "bpr"), ("scatter", "B", 64, "hinge"), ("scatter", "C", 48, "bpr"),
              ("inside", "B", 16, "bpr"), ("inside", "A", 64, "hinge"), ("empty", "C", 16, "adaptive_hinge"),
              ("maxlen", "F", 16, "bpr")]


# parameter seeds chosen on the CPU like SEEDS (several hundred thousand relu units: the default
# seed leaves one within TIE of 0)
EDGE_SEEDS = {("scatter", "B", 64): 6, ("inside", "B", 16): 2}


@functools.lru_cache(maxsize=None)
def edge_case(name, net, d):
    if name == "maxlen":
        base = sc.make_case(d, 1024, 3, 16, 50)        # RG_SEQ_MAX_LEN positions, RG_SEQ_MAX_NEG negatives
    elif name in ("inside", "outside"):
        base = sc.outside_pair(sc.scatter_case(d))[name == "inside"]
    else:
        base = sc.scatter_case(d) if name == "scatter" else sc.empty_rows_case(d)
    cfg = net_config(net, d)
    seed = EDGE_SEEDS.get((name if name != "outside" else "inside", net, d), 0)
    return dict(base, net=net, cfg=cfg, params=make_params(cfg, np.random.RandomState(53 + d + 1000 * seed)))


@functools.lru_cache(maxsize=None)
def edge_data(name, net, d, loss):
    return data_of(edge_case(name, net, d), loss)


# ------------------------------------------------------------------ stepping oracle
class Oracle:
    """The model with torch.optim.Adam on CPU tensors of ``dtype``; step(seq, neg) returns the
    loss before the update."""

    def __init__(self, cfg, E, b, params, loss, lr, l2=0.0, dtype=torch.float64):
        self.cfg, self.loss = cfg, loss
        self.E, self.b, self.p = (torch.as_tensor(a).to(dtype).clone().requires_grad_(True) for a in (E, b, params))
        self.opt = torch.optim.Adam([self.E, self.b, self.p], lr=lr, weight_decay=l2)

    def step(self, seq, neg):
        seq, neg = torch.as_tensor(seq), torch.as_tensor(neg)
        self.opt.zero_grad()
        zp, zn = position_scores(self.cfg, self.E, self.b, self.p, seq, neg)
        lv = sc.loss_of_scores(zp, zn, seq, self.loss)
        lv.backward()
        self.opt.step()
        return float(lv.detach())


def load_fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
