"""Statistics of the device dropout hash on its NumPy restatement (tests/ncf_common.py, held to
the kernel by tests/test_ncf_dropout_gpu.py): the keep rate is 1/2 overall and per unit, the
positives' mask is unrelated to the negatives', and a step's mask to the next step's.  The hash
is deterministic, so nothing here can flake."""
import numpy as np
import pytest

from tests import ncf_common as nc

SEEDS = [0, 3, 7, 9]
STEPS = [1, 2, 3]
SHAPES = [(120, 600, 5), (24, 512, 5), (8, 512, 4), (56, 1024, 4)]       # (units, B, n)


def test_hash_restatement_known_values():
    """murmur3's finalisers on hand-checkable inputs: 0 is a fixed point of both, and the wrap-around
    is the unsigned one (fmix64(1) = 0xB456BCFC34C2CB2C, fmix32(1) = 0x514E28B7: the published
    murmur3 test values)."""
    assert int(nc.hash32(np.array([0], np.uint64))[0]) == 0
    assert int(nc.mix32(np.array([0], np.uint32))[0]) == 0
    assert int(nc.hash32(np.array([1], np.uint64))[0]) == 0x34C2CB2C
    assert int(nc.mix32(np.array([1], np.uint32))[0]) == 0x514E28B7
    assert nc.step_seed(7, 1) == (7 * 0x9E3779B97F4A7C15 + 1) % 2 ** 64
    assert nc.step_seed(0, 3) == 3


@pytest.mark.parametrize("units,B,n", SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_device_dropout_statistics(seed, units, B, n):
    worst_z = worst_col = 0.0
    agree = []
    masks = {t: nc.device_masks(seed, t, units, B, n) for t in STEPS + [STEPS[-1] + 1]}
    for t in STEPS:
        mp, mn = masks[t]
        assert mp.shape == (B, units) and mn.shape == (n * B, units)
        for blk in (mp, mn):
            N = blk.size
            z = abs(blk.mean() - 0.5) / (0.5 / np.sqrt(N))
            worst_z = max(worst_z, z)
            assert z <= 5.0, (seed, t, blk.shape, z)
            zc = np.abs(blk.mean(0) - 0.5) / (0.5 / np.sqrt(blk.shape[0]))
            worst_col = max(worst_col, float(zc.max()))
            assert zc.max() <= 6.0, (seed, t, blk.shape, int(zc.argmax()), float(zc.max()))
        a = float((mp == mn[:B]).mean())
        assert 0.45 <= a <= 0.55, (seed, t, "positives vs first negatives", a)
        agree.append(a)
        for x, y in zip(masks[t], masks[t + 1]):
            a = float((x == y).mean())
            assert 0.45 <= a <= 0.55, (seed, t, "step vs next step", a)
            agree.append(a)
    print(f"seed {seed} units {units} B {B} n {n}: worst overall |z| {worst_z:.2f}, worst column |z| "
          f"{worst_col:.2f}, agreement {min(agree):.3f} .. {max(agree):.3f}")
