"""Shared pieces of the NCF / NeuMF training-step tests (test_ncf_matrix_gpu.py,
test_ncf_dropout_gpu.py, test_ncf_dropout_cpu.py, test_ncf_controls_cpu.py).  No test lives
here and nothing here needs a GPU until ``run_parity`` builds an engine.  The elementwise
gradient rule and its cases (test_ncf_grads_cpu.py, test_ncf_grads_gpu.py) are in
tests/ncf_grad_common.py, which builds on the pieces below.

* ``make_params``: an NCF tower (M = 0) or a NeuMF model in named_parameters() order, initialised
  as the reference initialises them (N(0, 1) embeddings, Xavier-uniform weights, bias 0.01).
* ``device_masks``: the device dropout RNG restated in NumPy from the kernel's definition
  (rg_ncf.h hash32 / mix32, the row key, the keep bit; documented on rg_ncf_work_t.seed in
  include/rg_hip.h), with uint64 / uint32 wrap-around.
* ``parity_ratio``: how much of oracle.mf.tensor_parity's allowance a tensor uses (reporting
  only; the verdict is always tensor_parity's own).
* ``run_parity``: NCFEngine against NCFOracle / NeuMFOracle in fp32 and fp64 from the same init,
  the pattern of test_ncf_e64_kernel_losses_and_shapes."""
import numpy as np
import torch

from oracle import mf as omf
from oracle import ncf as oncf
from oracle import rng as orng

# ----------------------------------------------------------------------------- device dropout
GOLD64 = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


def hash32(x):
    """rg_ncf.h hash32: murmur3's 64-bit finaliser, low 32 bits.  x: uint64 array."""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def mix32(h):
    """rg_ncf.h mix32: murmur3 fmix32.  h: uint32 array."""
    h = np.asarray(h, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def step_seed(engine_seed, t):
    """The seed of step t (t = 1 on the first train_step): ncf_engine.py NCFEngine._work."""
    return (int(engine_seed) * GOLD64 + int(t)) & MASK64


def row_keys(sseed, neg, gj):
    """key(row) = hash32(step seed ^ (neg ? 1 << 40 : 0) ^ (gj * golden mod 2^64)); gj: the
    positive's global column, or the negative's global draw index (q - 1) * global_cols + column."""
    gj = np.asarray(gj, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = gj * np.uint64(GOLD64)
    x ^= np.uint64(sseed ^ ((1 << 40) if neg else 0))
    return hash32(x)


def keep_bits(keys, units):
    """keep(row, unit) = (mix32(key + unit * 0x85EBCA6B) >> 7) & 1, [rows, units] uint8; ``unit``
    indexes the concatenated hidden layers (the column layout of recorded masks)."""
    with np.errstate(over="ignore"):
        h = keys[:, None] + (np.arange(units, dtype=np.uint32) * np.uint32(0x85EBCA6B))[None, :]
    return ((mix32(h) >> np.uint32(7)) & np.uint32(1)).astype(np.uint8)


def device_masks(engine_seed, t, units, B, n):
    """(mask_pos [B, units], mask_neg [n * B, units]) of step t on one rank (global_cols = B)."""
    s = step_seed(engine_seed, t)
    return (keep_bits(row_keys(s, False, np.arange(B)), units),
            keep_bits(row_keys(s, True, np.arange(n * B)), units))


# ----------------------------------------------------------------------------- models
def make_params(U, I, E, M, seed):
    """(tensors, names) in the reference's named_parameters() order: mlp.py:5-46 for M = 0,
    neuMF.py:7-55 for M > 0."""
    g = torch.Generator().manual_seed(seed)
    sizes = oncf.layer_sizes(E)
    if M:
        t = [torch.randn(U, E, generator=g), torch.randn(I, E, generator=g), torch.randn(U, M, generator=g),
             torch.randn(I, M, generator=g)]
        names = ["embedding_user_mlp.weight", "embedding_item_mlp.weight", "embedding_user_mf.weight",
                 "embedding_item_mf.weight"]
    else:
        t = [torch.randn(U, E, generator=g), torch.randn(I, E, generator=g)]
        names = ["embedding_user.weight", "embedding_item.weight"]
    for k, (a_, b_) in enumerate(zip(sizes[:-1], sizes[1:])):
        t += [(torch.rand(b_, a_, generator=g) - 0.5) * (2 * (6 / (a_ + b_)) ** 0.5), torch.full((b_,), 0.01)]
        names += [f"layers.{3 * k}.weight", f"layers.{3 * k}.bias"]
    a_ = 8 + M
    t += [(torch.rand(1, a_, generator=g) - 0.5) * (2 * (6 / (a_ + 1)) ** 0.5), torch.full((1,), 0.01)]
    names += ["affine_output.weight", "affine_output.bias"]
    return t, names


def oracle_for(M):
    return oncf.NeuMFOracle if M else oncf.NCFOracle


def split_units(mask, E):
    """A [rows, units] mask as the oracle's per-hidden-layer list."""
    out, o = [], 0
    for w in oncf.layer_sizes(E)[1:]:
        out.append(torch.from_numpy(np.ascontiguousarray(mask[:, o:o + w])))
        o += w
    return out


def eval_forward64(P, E, M, u, i):
    """Eval-mode (no dropout) float64 forward of the tower / NeuMF: mlp.py:30-41, neuMF.py:34-55."""
    P = [t.double() for t in P]
    ne = 4 if M else 2
    a = torch.cat([P[0][u], P[1][i]], 1)
    for k in range(ne, len(P) - 2, 2):
        z = a @ P[k].T + P[k + 1]
        a = torch.where(z > 0, z, z * 0.1)
    if M:
        a = torch.cat([a, P[2][u] * P[3][i]], 1)
    return torch.sigmoid(a @ P[-2].T + P[-1]).reshape(-1)


# ----------------------------------------------------------------------------- the acceptance rule
def parity_ratio(got, ref32, ref64, rtol=1e-5, band=3.0, before=None):
    """The share of tensor_parity's allowance (its defaults) that ``got`` uses: the smallest of
    distance / allowed over the rule's alternatives; <= 1 exactly when tensor_parity passes."""
    g = torch.as_tensor(got).double().reshape(-1).cpu()
    r = torch.as_tensor(ref32).double().reshape(-1)
    r64 = torch.as_tensor(ref64).double().reshape(-1)
    e32 = float((g - r).norm())
    scale = max(float(r.norm()), 1e-30)
    if before is not None:
        scale = max(scale, float(torch.as_tensor(before).double().reshape(-1).cpu().norm()))
    a = e32 / (rtol * scale)
    allowed64 = band * float((r - r64).norm()) + 0.1 * rtol * float(r64.norm())
    b = float((g - r64).norm()) / max(allowed64, 1e-300)
    return min(a, b)


def check_params(tag, names, got, o32, o64, before):
    """tensor_parity (existing defaults) on every parameter; returns the worst parity_ratio."""
    worst = 0.0
    for nm, p, r32, r64, b0 in zip(names, got, o32.P.t, o64.P.t, before):
        p = p.reshape(r32.shape)
        ok, msg = omf.tensor_parity(p, r32, r64, before=b0)
        assert ok, f"{tag} {nm}: {msg}"
        worst = max(worst, parity_ratio(p, r32, r64, before=b0))
    return worst


def pad_masks(m, rows, dev):
    out = torch.zeros(rows, m.shape[1], dtype=torch.uint8)
    out[:m.shape[0]] = torch.as_tensor(m, dtype=torch.uint8)
    return out.to(dev).contiguous()


def zipf_batch(rs, U, I, k):
    """Zipf-ish positives: a few hot users and items overflow their per-row lists."""
    return (np.minimum(rs.zipf(1.3, k) - 1, U - 1).astype(np.int64),
            np.minimum(rs.zipf(1.2, k) - 1, I - 1).astype(np.int64))


def run_parity(E, M, loss, optimizer, n, B, U, I, planned, seed, n_pos=None, steps=2, pool=20000, rng_seed=None,
               also_recorded=False, weight_decay=1e-5):
    """``steps`` native steps against the oracle in fp32 and fp64: MT state bit-equal, loss 1e-5
    relative, every parameter by tensor_parity.  ``n_pos`` (< B): a partial last batch with the
    full n * B draw.  ``rng_seed``: the engine draws dropout on the device (masks=None) and the
    oracles get the host restatement's masks; ``also_recorded``: a second engine fed those masks
    as recorded masks, returned for the bit-equality check.  Returns (worst parity ratio,
    [engine losses], engine, second engine or None)."""
    from recommendation_gans_amd.ncf_engine import NCFEngine
    dev = torch.device("cuda:0")
    t, names = make_params(U, I, E, M, seed)
    ne = 4 if M else 2
    rs = np.random.RandomState(seed * 7 + n)
    pool_u, pool_i = rs.randint(0, U, pool), rs.randint(0, I, pool)
    mt = orng.py_seed_state(7)
    kw = dict(loss=loss, lr=1e-2, weight_decay=weight_decay, n_neg=n, batch_size=B)
    extra = dict(mf_user_w=t[2], mf_item_w=t[3]) if M else {}

    device_rng = rng_seed is not None

    def engine():
        return NCFEngine(t[0], t[1], t[ne:], pool_u, pool_i, mt.copy(), optimizer=optimizer, device=dev,
                         seed=rng_seed if device_rng else 0, **extra, **kw)
    e = engine()
    e2 = engine() if also_recorded else None
    Oracle = oracle_for(M)
    o32 = Oracle([x.clone() for x in t], names, pool_u, pool_i, mt.copy(), optimizer=optimizer, **kw)
    o64 = Oracle([x.double() for x in t], names, pool_u, pool_i, mt.copy(), optimizer=optimizer, **kw)
    units = sum(oncf.layer_sizes(E)[1:])
    assert units == e.units
    k = B if n_pos is None else n_pos
    worst, losses = 0.0, []
    tag = f"E={E} M={M} {loss} {optimizer} wd={weight_decay:g} n={n} B={B} n_pos={k} plan={planned}"
    for s in range(steps):
        pu, pi = zipf_batch(rs, U, I, k)
        if not device_rng:
            mp, mn = (rs.rand(k, units) >= 0.5).astype(np.uint8), (rs.rand(n * B, units) >= 0.5).astype(np.uint8)
        else:
            mp, mn = device_masks(rng_seed, s + 1, units, B, n)
            mp = mp[:k]
        recorded = (pad_masks(mp, B, dev), pad_masks(mn, n * B, dev))
        pu_d, pi_d = torch.from_numpy(pu).to(dev), torch.from_numpy(pi).to(dev)
        before = [x.clone() for x in o32.P.t]
        plan = e.make_plan(pi_d) if planned else None
        got = float(e.train_step(pu_d, pi_d, plan=plan, masks=None if device_rng else recorded)[0])
        if e2 is not None:
            got2 = float(e2.train_step(pu_d, pi_d, plan=e2.make_plan(pi_d) if planned else None, masks=recorded)[0])
            losses.append((got, got2))
        else:
            losses.append(got)
        l32 = o32.step(pu, pi, split_units(mp, E), split_units(mn, E))
        o64.step(pu, pi, split_units(mp, E), split_units(mn, E))
        torch.cuda.synchronize()
        assert abs(got - l32) <= 1e-5 * abs(l32), (tag, s, got, l32)
        assert (e.mt_state() == o32.state).all(), f"{tag}: MT state after step {s}"
        worst = max(worst, check_params(f"{tag} step {s}", names, e.params(), o32, o64, before))
    assert int(e.row_count.abs().sum()) == 0 and float(e.hot_grad.abs().sum()) == 0.0
    if M:
        assert float(e.mf_hot_grad.abs().sum()) == 0.0
    print(f"{tag}: worst parity ratio {worst:.3g}")
    return worst, losses, e, e2
