"""What the device dropout RNG draws (production training: masks=None).  The hash per (step,
example, unit) is restated in NumPy (tests/ncf_common.py device_masks, from rg_ncf.h hash32 /
mix32, the row key and the keep bit; the contract on rg_ncf_work_t.seed in include/rg_hip.h).

Per configuration -- the wave kernel (E = 64), the tile kernel (E = 16, 32), NeuMF (E = 8,
M = 5); pointwise and adaptive hinge (whose scores phase and given-dp phase must see one mask);
with and without a plan (the key must not depend on the plan's permutation); Zipf-ish positives
so lists overflow; three steps, engine seed != 0:

* an engine drawing on the device matches the oracles (fp32, fp64) fed the host-computed masks
  of steps t = 1, 2, 3 -- loss 1e-5 relative, MT state bit-equal, every parameter by
  oracle.mf.tensor_parity.  A keep rate other than the hash's, one mask for positives and
  negatives, a mask that does not move with the step, or a key that follows the tile layout or
  the plan would each put the engine on another trajectory than the oracle's;
* it is bit-equal (every parameter, the loss floats) to a second engine fed the same host masks
  as recorded masks: both paths form the same keep ? 2 m : 0 multiplier and the same sums."""
import pytest
import torch

from tests import ncf_common as nc

pytestmark = pytest.mark.gpu

CONFIGS = [(64, 0), (16, 0), (32, 0), (8, 5)]


@pytest.mark.parametrize("planned", [False, True])
@pytest.mark.parametrize("loss", ["pointwise", "adaptive_hinge"])
@pytest.mark.parametrize("E,M", CONFIGS)
def test_device_dropout_draws_the_documented_masks(E, M, loss, planned):
    worst, losses, e, e2 = nc.run_parity(E, M, loss, "adam", 5, B=600, U=400, I=300, planned=planned, seed=E + M + 1,
                                         steps=3, rng_seed=7 if planned else 9, also_recorded=True)
    bit_equal = all(a == b for a, b in losses) and all(torch.equal(p, q) for p, q in zip(e.params(), e2.params()))
    print(f"E={E} M={M} {loss} plan={planned}: device RNG vs recorded masks bit-equal: {bit_equal}")
    assert all(a == b for a, b in losses), losses
    for k, (p, q) in enumerate(zip(e.params(), e2.params())):
        assert torch.equal(p, q), (k, float((p - q).abs().max()))
