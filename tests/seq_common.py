"""What the pooling sequence model's tests share (no tests here): the model of include/rg_hip.h
(rg_seq_pool_grads) stated in torch on the CPU -- representations, scores, the three losses --
with autograd gradients through ``padding_idx = 0`` and ``torch.optim.Adam``, in float64 (the
reference of every comparison) and float32 (the error a float32 evaluation of the same formulas
has, E32); the case builder; the fixture recorded from the reference's PoolNet.

The gradient rule is fold_in_common's: the kernel may sit at most 2 x E32 from float64 (E32 the
largest float32-vs-float64 deviation over the case's elements), plus that helper's floor -- a
difference below ``fold_in_common.CANCEL`` of an element's sum of |terms| is rounding.  The sum of
|terms| is exact: the gradient is a sum of products dz * (element of E) * 1 / (c + 1) with
non-negative coefficients, so the same graph evaluated at |dz|, |E| sums their magnitudes.

Cases are a covering list chosen before any GPU run.  They select every row layout the kernel is
instantiated for (rg_common.h dispatch_dim; LPU lanes x EPL elements per lane), by d:
    8 / 16 / 32 / 64 / 128 / 256   the 16-byte layouts of 2 / 4 / 8 / 16 / 32 / 64 lanes x 4
    4, 12                          scalar, 16 lanes x 1        24     scalar, 16 lanes x 2
    48                             scalar, 16 lanes x 4        96     scalar, 64 lanes x 2
    160                            scalar, 64 lanes x 3        200    scalar, 64 lanes x 4
with L {1, 2, 5, 33}, B {1, 3, 257}, K {1, 5}, 7 items (every row collides in the atomics) and
1000, the three losses.  A hinge whose argument, or an adaptive hinge whose two highest negatives
(of different items), come within ``fold_in_common.TIE`` of a kink in float64 would make the
gradient a coin toss in float32; ``kink_margin`` measures it and test_seq_cpu.py checks that no
case has one -- the edge cases below (``EDGE_CASES``: padding anywhere, ids outside the table, rows
of padding alone, the longest sequence with the most negatives) included.  ``UNALIGNED`` names the
cases the tests run again on a table that starts 4 bytes off a 16-byte boundary, where every d
takes a scalar layout: the power-of-two dims then fill every lane slot exactly (d == LPU * EPL),
and d 24 keeps its layout.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import fold_in_common as fc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_pool_d8.npz")
LOSSES = ("bpr", "hinge", "adaptive_hinge")

# (d, L, B, K, num_items, loss)
CASES = [
    (4, 1, 1, 1, 7, "bpr"),
    (4, 33, 257, 5, 1000, "adaptive_hinge"),
    (8, 2, 3, 1, 7, "hinge"),
    (8, 5, 257, 1, 7, "bpr"),
    (8, 33, 257, 5, 1000, "hinge"),
    (12, 5, 3, 1, 7, "bpr"),
    (16, 5, 3, 5, 7, "bpr"),
    (64, 33, 3, 5, 7, "adaptive_hinge"),
    (64, 5, 257, 1, 1000, "hinge"),
    (64, 1, 257, 5, 1000, "adaptive_hinge"),
    (128, 2, 257, 5, 7, "bpr"),
    (128, 33, 1, 1, 1000, "hinge"),
    (200, 2, 3, 1, 1000, "hinge"),
    (256, 5, 3, 5, 1000, "adaptive_hinge"),
    (256, 33, 257, 1, 7, "bpr"),
    # the layouts the list above never selected (every one admitted as first written)
    (32, 33, 257, 5, 7, "hinge"),
    (24, 5, 3, 5, 1000, "adaptive_hinge"),
    (48, 33, 257, 1, 1000, "bpr"),
    (96, 2, 3, 5, 7, "hinge"),
    (160, 5, 257, 1, 7, "adaptive_hinge"),
]
CASE_IDS = ["d%d-L%d-B%d-K%d-I%d-%s" % c for c in CASES]
# the cases run again on an unaligned table: of dims 8, 16, 64, 128 and 24 the case with the most
# (position, negative) pairs L * B * K, the first of equals
UNALIGNED = [max((i for i, c in enumerate(CASES) if c[0] == dim), key=lambda i: (np.prod(CASES[i][1:4]), -i))
             for dim in (8, 16, 64, 128, 24)]


def outside_ids(num_items):
    """The out-of-range ids the kernels must read as padding (include/rg_hip.h)."""
    return np.array([num_items, num_items + 5, -1, 2 ** 40], dtype=np.int64)


def make_tables(num_items, d, rs, scale=0.7):
    E = (rs.randn(num_items, d) * scale / np.sqrt(d)).astype(np.float32)
    b = (rs.randn(num_items) * 0.3).astype(np.float32)
    E[0], b[0] = 0.0, 0.0
    return E, b


def make_sequences(B, L, num_items, rs):
    """Left-padded sequences: row 0 full, row 1 with leading padding, row 2 a single item, row 3
    (or the last) repeating an item, the rest of random lengths >= 1."""
    seq = rs.randint(1, num_items, (B, L)).astype(np.int64)
    lens = rs.randint(1, L + 1, B)
    lens[0] = L
    if B > 1:
        lens[1] = max(1, L // 2)
    if B > 2:
        lens[2] = 1
    for r in range(B):
        seq[r, :L - lens[r]] = 0
    r = min(3, B - 1)
    if lens[r] >= 2:
        seq[r, -1] = seq[r, -2]
    elif L >= 2 and B == 1:
        seq[r, -1] = seq[r, -2]
    return seq


def make_case(d, L, B, K, num_items, seed=0):
    rs = np.random.RandomState(100003 * seed + 1009 * d + 101 * L + 7 * B + K + num_items)
    E, b = make_tables(num_items, d, rs)
    seq = make_sequences(B, L, num_items, rs)
    neg = rs.randint(0, num_items, (K, B, L)).astype(np.int64)
    hit = rs.random_sample((B, L))
    neg[0][hit < 0.05] = 0                                   # negatives that hit the padding id
    neg[K - 1][hit > 0.95] = seq[hit > 0.95]                 # negatives that equal the target
    return dict(E=E, b=b, seq=seq, neg=neg, d=d, L=L, B=B, K=K, num_items=num_items)


# ------------------------------------------------------------------ the model in torch
def representations(E, seq):
    """(r_0 .. r_{L-1} [B, L, d], r_L [B, d]); E[0] never receives a gradient (padding_idx)."""
    emb = F.embedding(seq, E, padding_idx=0)
    S = torch.cat([torch.zeros_like(emb[:, :1]), torch.cumsum(emb, 1)], 1)
    c = torch.cat([torch.zeros_like(seq[:, :1]), torch.cumsum((seq != 0).long(), 1)], 1)
    r = S / (c + 1).to(E.dtype)[:, :, None]
    return r[:, :-1], r[:, -1]


def position_scores(E, b, seq, neg):
    r, _ = representations(E, seq)
    bias = b.reshape(-1, 1)
    zp = F.embedding(seq, bias, padding_idx=0)[..., 0] + (r * F.embedding(seq, E, padding_idx=0)).sum(-1)
    zn = F.embedding(neg, bias, padding_idx=0)[..., 0] + (r[None] * F.embedding(neg, E, padding_idx=0)).sum(-1)
    return zp, zn


def loss_of_scores(zp, zn, seq, loss):
    mask = (seq != 0).to(zp.dtype)
    if loss == "bpr":
        term = 1.0 - torch.sigmoid(zp - zn)
    elif loss == "hinge":
        term = torch.clamp(zn - zp + 1.0, min=0.0)
    else:
        term = torch.clamp(zn.max(0).values - zp + 1.0, min=0.0)
    return (term * mask).sum() / mask.sum()


def final_scores(E, b, seq):
    """Raw scores of every item as the next item, [n, num_items]."""
    _, rL = representations(E, seq)
    return rL @ E.T + b[None, :]


def grads(case, loss, dtype=torch.float64, abs_terms=False):
    """loss, dE [num_items, d], db [num_items] by autograd; with ``abs_terms`` also the sums of
    |terms| of both gradients (see the module docstring)."""
    t = lambda a: torch.from_numpy(a)
    E = t(case["E"]).to(dtype).requires_grad_(True)
    b = t(case["b"]).to(dtype).requires_grad_(True)
    seq, neg = t(case["seq"]), t(case["neg"])
    zp, zn = position_scores(E, b, seq, neg)
    lv = loss_of_scores(zp, zn, seq, loss)
    dzp, dzn = torch.autograd.grad(lv, [zp, zn], retain_graph=True)
    gE, gb = torch.autograd.grad(lv, [E, b])
    out = dict(loss=float(lv.detach()), gE=gE.numpy(), gb=gb.numpy())
    if abs_terms:
        Ea = t(case["E"]).to(dtype).abs().requires_grad_(True)
        ba = t(case["b"]).to(dtype).abs().requires_grad_(True)
        zpa, zna = position_scores(Ea, ba, seq, neg)
        aE, ab = torch.autograd.grad((dzp.abs() * zpa).sum() + (dzn.abs() * zna).sum(), [Ea, ba])
        out.update(aE=aE.numpy(), ab=ab.numpy())
    return out


def kink_margin(case, loss):
    """float64 distance of the nearest masked hinge argument from 0, or of an adaptive hinge's two
    highest negatives of different items from each other (inf for bpr)."""
    if loss == "bpr":
        return np.inf
    t = lambda a: torch.from_numpy(a)
    zp, zn = position_scores(t(case["E"]).double(), t(case["b"]).double(), t(case["seq"]), t(case["neg"]))
    zp, zn, mask = zp.numpy(), zn.numpy(), case["seq"] != 0
    if loss == "hinge":
        return float(np.abs(zn - zp[None] + 1.0)[:, mask].min(initial=np.inf))
    top = zn.max(0)
    margin = float(np.abs(top - zp + 1.0)[mask].min(initial=np.inf))
    if case["K"] > 1:
        win = np.take_along_axis(case["neg"], zn.argmax(0)[None], 0)
        other = np.where(case["neg"] != win, zn, -np.inf).max(0)
        margin = min(margin, float((top - other)[mask].min(initial=np.inf)))
    return margin


@functools.lru_cache(maxsize=None)
def case_data(i):
    """Case i, computed once per process and shared (read-only): the float64 reference with the
    sums of |terms|, and E32, the largest deviation of the float32 CPU evaluation from it."""
    d, L, B, K, num_items, loss = CASES[i]
    return data_of(make_case(d, L, B, K, num_items), loss)


def data_of(case, loss):
    """What ``case_data`` holds, of any case."""
    r64 = grads(case, loss, torch.float64, abs_terms=True)
    r32 = grads(case, loss, torch.float32)
    e32 = max(float(np.abs(r32["gE"].astype(np.float64) - r64["gE"]).max()),
              float(np.abs(r32["gb"].astype(np.float64) - r64["gb"]).max()))
    return dict(case=case, loss=loss, r64=r64, r32=r32, e32=e32)


# ------------------------------------------------------------------ the entries' edges
def scatter_case(d, B=67, L=33, K=5, num_items=40):
    """Padding anywhere: about a third of the positions of left-padded sequences zeroed at random,
    row 0 ending in a zero, every row keeping at least one item.  67 rows are more than one wave of
    every layout."""
    case = make_case(d, L, B, K, num_items, seed=1)
    rs = np.random.RandomState(977 + d)
    seq = case["seq"]
    seq[rs.random_sample(seq.shape) < 0.3] = 0
    seq[0, -1] = 0
    for r in np.flatnonzero((seq != 0).sum(1) == 0):
        seq[r, L // 2] = 1 + r % (num_items - 1)
    return case


def outside_pair(case):
    """(outside, inside): ``case`` with its padding zeros in seq, and a tenth of neg, replaced by ids
    outside [0, num_items), and the same case with zeros in those places."""
    rs = np.random.RandomState(31)
    bad = outside_ids(case["num_items"])
    pad = case["seq"] == 0
    hit = rs.random_sample(case["neg"].shape) < 0.1
    out = dict(case, seq=case["seq"].copy(), neg=case["neg"].copy())
    ins = dict(case, seq=case["seq"].copy(), neg=case["neg"].copy())
    out["seq"][pad] = bad[np.arange(pad.sum()) % len(bad)]
    out["neg"][hit] = bad[np.arange(hit.sum()) % len(bad)]
    ins["neg"][hit] = 0
    return out, ins


def empty_rows_case(d, B=9, L=5, K=3, num_items=40):
    """Rows 4 and 8 (the last) are padding alone; the others are ``scatter_case``'s."""
    case = scatter_case(d, B, L, K, num_items)
    case["seq"][[4, 8]] = 0
    return case


def max_len_case():
    """RG_SEQ_MAX_LEN positions with RG_SEQ_MAX_NEG negatives: row 0 full, row 1 half padding,
    row 2 a single item."""
    return make_case(8, 1024, 3, 16, 50)


# (name, d, loss): every edge case whose gradients meet the float64 oracle
EDGE_CASES = [("scatter", 8, "bpr"), ("scatter", 8, "hinge"), ("scatter", 64, "bpr"), ("scatter", 64, "hinge"),
              ("inside", 8, "hinge"), ("inside", 64, "bpr"), ("empty", 8, "adaptive_hinge"), ("maxlen", 8, "bpr")]


@functools.lru_cache(maxsize=None)
def edge_case(name, d):
    if name == "scatter":
        return scatter_case(d)
    if name in ("inside", "outside"):
        return outside_pair(scatter_case(d))[name == "inside"]
    return empty_rows_case(d) if name == "empty" else max_len_case()


@functools.lru_cache(maxsize=None)
def edge_data(name, d, loss):
    """``data_of`` of an edge case, computed once per process (read-only)."""
    return data_of(edge_case(name, d), loss)


def gradient_excess(gE, gb, data):
    """The largest ratio |kernel - float64| / (2 E32 + CANCEL * sum |terms|) over all elements
    (must be <= 1), and the plain largest |kernel - float64| / E32 for the log."""
    r64, e32 = data["r64"], data["e32"]
    worst = plain = 0.0
    for got, ref, a in ((gE, r64["gE"], r64["aE"]), (gb, r64["gb"], r64["ab"])):
        err = np.abs(np.asarray(got, np.float64) - ref)
        bound = 2.0 * e32 + fc.CANCEL * a
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / bound, 0.0)
        worst = max(worst, float(ratio.max()))
        plain = max(plain, float(err.max()) / e32 if e32 > 0 else (0.0 if err.max() == 0 else np.inf))
    return worst, plain


# ------------------------------------------------------------------ stepping oracle
class Oracle:
    """The model with torch.optim.Adam on CPU tensors of ``dtype``; step(seq, neg) returns the
    loss before the update."""

    def __init__(self, E, b, loss, lr, l2=0.0, dtype=torch.float64):
        self.E = torch.as_tensor(E).to(dtype).clone().requires_grad_(True)
        self.b = torch.as_tensor(b).to(dtype).clone().requires_grad_(True)
        self.loss = loss
        self.opt = torch.optim.Adam([self.E, self.b], lr=lr, weight_decay=l2)

    def step(self, seq, neg):
        seq, neg = torch.as_tensor(seq), torch.as_tensor(neg)
        self.opt.zero_grad()
        zp, zn = position_scores(self.E, self.b, seq, neg)
        lv = loss_of_scores(zp, zn, seq, self.loss)
        lv.backward()
        self.opt.step()
        return float(lv.detach())


def adam_formula_step(p, g, m, v, t, lr, wd, cr_sqrt, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's single-tensor update op by op on CPU float32 tensors (each op keeps
    torch's rounding); ``cr_sqrt``: a correctly rounded sqrt instead of ATen's."""
    sqrt = (lambda x: x.double().sqrt().float()) if cr_sqrt else torch.sqrt
    g = g.add(p, alpha=wd)
    m = m.lerp(g, 1 - betas[0])
    v = v.mul(betas[1]).addcmul(g, g, value=1 - betas[1])
    denom = (sqrt(v) / ((1 - betas[1] ** t) ** 0.5)).add(eps)
    return p.addcdiv(m, denom, value=-(lr / (1 - betas[0] ** t))), m, v


def ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def load_fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
