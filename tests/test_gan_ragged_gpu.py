"""cGAN D / G steps and generation on ragged batches, against the float64 restatement
(oracle/gan.py, itself checked against autograd at these kinds of shape in
tests/test_gan_autograd_cpu.py).

One GANEngine and one GANOracle take a shrinking sequence of batches, both free-running, so
every step after the first runs with ``rows < batch_max`` on a workspace whose rows
[rows, batch_max) still hold the previous, larger batch: every weight-gradient GEMM reduces
over K = rows with stale operand rows behind the K mask, and the stacked [real; fake] rows of
the D step sit at offset ``rows``.  Setup as C4's scaled_d case (tests/test_configs_gpu.py): D
rescaled to max |x| = 0.004, recorded z and dropout masks fed to both sides, the float32-rounded
dropout scales, make_golden.gan_case's learning rates.  Rules after every step: D outputs and the
loss within 1e-5 of the outputs' scale; G(z) within 1e-5 relative by norm; every stepped
parameter by tests/test_gan_oracle.param_ok (rtol 1e-5, ``prior`` carried across the steps,
pre-BatchNorm biases exempt); BatchNorm running statistics rtol 1e-5 / atol 1e-7 and
num_batches_tracked; the G step's slates by the near-tie rule (the chosen item's float64 tanh
within 1e-5 of the row's maximum); the pad columns of W1S and pad rows of WH exactly zero.

* Case A (rms, adam, sgd): N = 150, S = 3 (ks = 452, heads straddling the 128-column tiles, the
  fused-argmax path), batches of 160, 131, 37 and 5 rows: two row tiles with a second of 3
  rows and a ragged last split at 131, K below and not a multiple of the K step after.
* Case B: E = 12 (a second, partial embedding column chunk) and L = 260 (hist_sum_kernel's
  stride loop; rows longer than the catalogue, so items repeat), batches of 48 then 9.
* Case C: two rows, the smallest batch training accepts; one row is refused.
* Case D: generate on 37 rows and 1 row after a 160-row call; generate_slates over a full and
  a ragged block.

Histories carry an all-padding row, a full row, a row with a repeated item and an item present
in every other row; real slates put hits on columns 127 / 128, both sides of a head boundary, the
last real column, and one column shared by more rows than a wave has lanes
(tests/gan_common.py)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import gan as og
from tests.gan_common import (DROP_SCALES, GOLDEN_LR, d_step_widths, edge_histories, edge_slates, f64, g_step_widths,
                              noise, random_gan, scale_d)
from tests.test_gan_oracle import param_ok

pytestmark = pytest.mark.gpu

BN_BUFFERS = [f"layers.{k}.running_{s}" for k in (1, 5) for s in ("mean", "var")]


class Pair:
    """The engine and the oracle from one init, with the steps' checks."""

    def __init__(self, N, S, H, E, Z, batch_max, opt, seed):
        from recommendation_gans_amd.gan_engine import GANEngine
        self.N, self.S, self.H, self.E, self.Z = N, S, H, E, Z
        gs, ds = random_gan(N, S, H, E, Z, seed)
        ds = scale_d(ds)
        self.lr = GOLDEN_LR[opt]
        self.eng = GANEngine(gs, ds, N, S, H, E, Z, batch_max=batch_max, optimizer=opt, lr=self.lr)
        self.o = og.GANOracle({k: v.numpy() for k, v in gs.items()}, {k: v.numpy() for k, v in ds.items()}, N, S, H,
                              E, Z, opt=opt, lr=self.lr)
        self.ill = {}
        assert self.eng.ks == (S * N + 3) // 4 * 4

    def batch(self, hist, slates=None):
        from recommendation_gans_amd.gan_engine import GANBatch
        return GANBatch(hist, slates, self.N, self.S, "cuda")

    def prior(self, which, n):
        shape = (self.o.D if which == "D" else self.o.G)[n].shape
        return self.ill.setdefault(which + n, np.zeros(shape, bool))

    def check_buffers(self, gsd, what):
        for n in BN_BUFFERS:
            np.testing.assert_allclose(gsd[n].numpy(), self.o.G[n], rtol=1e-5, atol=1e-7, err_msg=f"{what} {n}")
        for bn in ("layers.1", "layers.5"):
            assert int(gsd[bn + ".num_batches_tracked"]) == int(self.o.G[bn + ".num_batches_tracked"]), what

    def check_pads(self, what):
        e, SN = self.eng, self.S * self.N
        assert not e._dv("W1S", (2 * self.H, e.ks))[:, SN:].any(), f"{what}: W1S pad columns"
        assert not e._gv("WH", (e.ks, self.H))[SN:].any(), f"{what}: WH pad rows"

    def d_step(self, hist, slates, rs, what):
        eng, o, rows = self.eng, self.o, len(hist)
        z, mk = noise(rs, rows, self.Z, d_step_widths(self.H))
        out = eng.d_step(self.batch(hist, slates), z=torch.from_numpy(z), masks=mk).cpu().numpy()
        loss, d_real, d_fake, fake = o.d_step(hist, slates, z.astype(np.float64), f64(mk), DROP_SCALES)
        dval = eng.last_d_out(2 * rows).cpu().numpy()          # [real; fake], the fake rows at offset rows
        scale = np.abs(np.concatenate([d_real.ravel(), d_fake.ravel()])).max()
        errs = (np.abs(dval[:rows] - d_real.ravel()).max(), np.abs(dval[rows:] - d_fake.ravel()).max(),
                abs(out[0] - loss))
        frel = rel(eng.last_fake(rows), fake)
        print(f"{what}: D(real) {errs[0]:.2e} D(fake) {errs[1]:.2e} loss {errs[2]:.2e} of scale {scale:.2e}; "
              f"G(z) rel {frel:.2e}")
        assert max(errs) <= 1e-5 * scale, what
        assert frel <= 1e-5, what
        dsd = eng.d_state_dict()
        for n in o.D:
            ok, msg = param_ok(dsd[n].numpy(), o.D[n], o.last_grads[n], self.lr, prior=self.prior("D", n))
            assert ok, f"{what} D {n}: {msg}"
        # the output bias: the real and the fake pass's sums of dout cancel exactly (the reference's
        # too), so no optimizer moves it, at any batch size
        assert not o.last_grads["layers.9.bias"].any(), what
        assert dsd["layers.9.bias"].numpy().astype(np.float64) == o.D["layers.9.bias"], f"{what}: D output bias moved"
        self.check_buffers(eng.g_state_dict(), what)
        self.check_pads(what)

    def g_step(self, hist, rs, what, upstream_bound_only=False):
        """``upstream_bound_only``: Case C's rule for a two-row batch (see its docstring)."""
        eng, o, rows = self.eng, self.o, len(hist)
        z, mk = noise(rs, rows, self.Z, g_step_widths(self.H))
        z64, mk64 = z.astype(np.float64), f64(mk)
        saved = copy.deepcopy(o.G)                # the train-mode G(z) of this step, stats left alone
        fake = np.concatenate(o.g_forward(z64, hist, mk64[0:2], DROP_SCALES[0], train=True)[0], 1)
        o.G = saved
        gl, slates = eng.g_step(self.batch(hist), z=torch.from_numpy(z), masks=mk)
        gloss, gd_fake, _ = o.g_step(hist, z64, mk64, DROP_SCALES)
        gdout = eng.last_d_out(rows).cpu().numpy()
        scale = np.abs(gd_fake).max()
        errs = (np.abs(gdout - gd_fake.ravel()).max(), abs(float(gl[0]) - gloss))
        frel = rel(eng.last_fake(rows), fake)
        print(f"{what}: D(G(z)) {errs[0]:.2e} loss {errs[1]:.2e} of scale {scale:.2e}; G(z) rel {frel:.2e}")
        assert max(errs) <= 1e-5 * scale, what
        assert frel <= 1e-5, what
        gsd = eng.g_state_dict()
        for n in o.g_params:
            bound_only = n in o.pre_bn_biases() or (upstream_bound_only and not n.startswith("mult_heads"))
            ok, msg = param_ok(gsd[n].numpy(), o.G[n], o.last_grads[n], self.lr, exempt=bound_only,
                               prior=self.prior("G", n))
            assert ok, f"{what} G {n}: {msg}"
        self.check_buffers(gsd, what)
        self.check_pads(what)
        if not upstream_bound_only:
            self.check_slates(slates, z64, hist, what)

    def check_slates(self, slates, z64, hist, what):
        """Near-tie rule: the chosen item's float64 tanh is the row's maximum to 1e-5."""
        got = slates.cpu().numpy()
        assert got.shape == (len(hist), self.S) and (got == np.floor(got)).all() and got.min() >= 0 and \
            got.max() < self.N, what
        heads, _ = self.o.g_forward(z64, hist, train=False)
        for s in range(self.S):
            chosen = heads[s][np.arange(len(hist)), got[:, s].astype(np.int64)]
            assert (chosen >= heads[s].max(1) - 1e-5).all(), f"{what} head {s}"


def rel(got, ref):
    got = got.cpu().numpy().astype(np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)


A_DIMS = dict(N=150, S=3, H=32, E=5, Z=100)
A_L, A_MAX = 6, 160


def a_batch(rs, rows):
    hist = edge_histories(rs, rows, A_DIMS["N"], A_L)
    return hist, edge_slates(rs, rows, A_DIMS["N"], A_DIMS["S"])


@pytest.mark.parametrize("opt", ["rms", "adam", "sgd"])
def test_gan_steps_shrinking_batches(opt):
    """Case A: 160, 131, 37 and 5 rows through one engine, a D step then a G step on each."""
    p = Pair(batch_max=A_MAX, opt=opt, seed=31, **A_DIMS)
    rs = np.random.RandomState(17)
    for rows in (160, 131, 37, 5):
        hist, slates = a_batch(rs, rows)
        if rows == A_MAX:
            col1 = slates[:, 1]
            assert slates[0, 0] == 127 and slates[1, 0] == 128 and slates[0, 2] == 149 and (col1 == 17).sum() > 64
            assert (hist[0] == 150).all() and (hist[1] != 150).all() and (hist[1:] == 3).any(1).all()
        p.d_step(hist, slates, rs, f"{opt} D rows {rows}")
        p.g_step(hist, rs, f"{opt} G rows {rows}")


def test_gan_steps_wide_embedding_long_history():
    """Case B: E = 12 and L = 260, ks = 260 with no padding, batches of 48 then 9 rows."""
    N, S, L = 130, 2, 260
    p = Pair(N, S, 16, 12, 100, batch_max=48, opt="rms", seed=32)
    assert p.eng.ks == S * N
    rs = np.random.RandomState(18)
    for rows in (48, 9):
        hist = edge_histories(rs, rows, N, L, full_rows=(1, 4, 7))
        assert (hist[[1, 4, 7]] != N).all() and (hist[0] == N).all()
        slates = np.stack([rs.choice(N, S, replace=False) for _ in range(rows)])
        slates[0], slates[1] = [127, N - 1], [128, 0]
        p.d_step(hist, slates, rs, f"B D rows {rows}")
        p.g_step(hist, rs, f"B G rows {rows}")


def test_gan_steps_two_rows():
    """Case C: after a 160-row D and G step, a 2-row D step (the full rules) and a 2-row G step.
    BatchNorm over two samples normalises every channel to +-1 / sqrt(1 + eps / var), so the
    backward's dy = rstd (dyhat - mean(dyhat) - yhat mean(dyhat yhat)) cancels almost exactly:
    what is left is rounding in any implementation.  Everything upstream of a BatchNorm
    (layers.0 / 1 / 4 / 5, G's embedding) therefore gets a gradient that is noise at fp32, and
    those tensors are held only to the step bound |delta| <= 30 lr that param_ok uses for exempt
    tensors; the loss, D(G(z)), G(z), the running statistics and the head weights and biases
    keep the full rules.  The eval-mode slates after that step come from those upstream tensors
    and are not compared.  One row is refused by both steps, with nothing launched."""
    from recommendation_gans_amd.gan_engine import ptr
    p = Pair(batch_max=A_MAX, opt="rms", seed=33, **A_DIMS)
    rs = np.random.RandomState(19)
    hist, slates = a_batch(rs, A_MAX)
    p.d_step(hist, slates, rs, "C D rows 160")
    p.g_step(hist, rs, "C G rows 160")
    hist, slates = a_batch(rs, 2)
    assert (hist[0] == 150).all() and (hist[1] != 150).all()
    p.d_step(hist, slates, rs, "C D rows 2")
    p.g_step(hist, rs, "C G rows 2", upstream_bound_only=True)

    eng = p.eng
    g0, d0, ws0 = eng.g.clone(), eng.d.clone(), eng.ws.clone()
    b1 = p.batch(hist[1:], slates[1:])
    z, mk = noise(rs, 1, eng.Z, d_step_widths(eng.H))
    nz, keep = eng._noise(1, torch.from_numpy(z), mk)
    out = torch.zeros(3, device="cuda")
    b = b1.c_struct()
    rc_d = eng.lib.rg_gan_d_step(eng._stream(), ctypes.byref(eng._model()), ptr(eng.ws), ctypes.byref(b),
                                 ctypes.byref(nz), ctypes.byref(eng._opt(3)), ptr(out))
    rc_g = eng.lib.rg_gan_g_step(eng._stream(), ctypes.byref(eng._model()), ptr(eng.ws), ctypes.byref(b),
                                 ctypes.byref(nz), ctypes.byref(eng._opt(3)), ptr(out), None)
    torch.cuda.synchronize()
    assert rc_d != 0 and rc_g != 0
    assert torch.equal(eng.g, g0) and torch.equal(eng.d, d0) and torch.equal(eng.ws, ws0) and not out.any()
    with pytest.raises(RuntimeError, match="2 rows"):
        eng.d_step(b1, z=torch.from_numpy(z), masks=mk)


def test_gan_generate_after_larger_batch():
    """Case D: generate on 37 rows and on 1 row after a 160-row call on the same workspace,
    against the float64 eval-mode forward by the near-tie rule; generate_slates over 197 rows
    (one full block of batch_max = 160, one ragged) gives the slates of the two generate calls
    with the same seeded torch.rand draws."""
    p = Pair(batch_max=A_MAX, opt="rms", seed=34, **A_DIMS)
    eng, N, Z = p.eng, A_DIMS["N"], A_DIMS["Z"]
    g = torch.Generator().manual_seed(6)
    stats = {"layers.1.running_mean": torch.rand(16, generator=g) * 0.2 - 0.1,
             "layers.5.running_var": torch.rand(32, generator=g) * 1.5 + 0.5}
    sd = eng.g_state_dict()
    sd.update(stats)
    eng.load_g_state(sd)
    for k, v in stats.items():
        p.o.G[k] = v.numpy().astype(np.float64)
    rs = np.random.RandomState(20)
    hist = edge_histories(rs, 197, N, A_L)
    hist[160] = N                                 # the ragged block starts on an all-padding row
    torch.manual_seed(12)
    all_slates = eng.generate_slates(torch.from_numpy(hist.astype(np.int32)).cuda())
    torch.manual_seed(12)
    z1, z2 = torch.rand(160, Z, device="cuda"), torch.rand(37, Z, device="cuda")
    s1 = eng.generate(p.batch(hist[:160]), z=z1)
    s2 = eng.generate(p.batch(hist[160:]), z=z2)
    p.check_slates(s1, z1.cpu().numpy().astype(np.float64), hist[:160], "generate 160")
    p.check_slates(s2, z2.cpu().numpy().astype(np.float64), hist[160:], "generate 37 after 160")
    assert all_slates.dtype == torch.int32 and all_slates.shape == (197, 3)
    assert torch.equal(all_slates, torch.cat([s1, s2]).to(torch.int32))
    z3 = torch.rand(1, Z, generator=g)
    s3 = eng.generate(p.batch(hist[5:6]), z=z3)
    p.check_slates(s3, z3.numpy().astype(np.float64), hist[5:6], "generate 1 after 37")
