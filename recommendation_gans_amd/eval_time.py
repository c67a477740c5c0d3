"""Stand-alone timing of the all-item NCF / NeuMF score block (outside tests and bench.py).

    python -m recommendation_gans_amd.eval_time [--users 256] [--items 26744] [--reps 20] [--big 4096]

Times, for the E = 64 NCF MLP and NeuMF (E = 16, M = 50) at the ML-20M item count, one block of
``--users`` users scored against every item by

  * ``NCFEngine.score_users``  -- rg_ncf_score_users (the split first layer's halves + the fused
    pair kernel), and
  * ``NCFEngine.scores``       -- the pairwise torch path the evaluation used before (gather, cat,
    one GEMM per layer, where, sigmoid through global memory),

with device events around each call after a warm-up, the two paths alternating, and reports
min / median per path, their ratio, the largest difference between the two blocks, and the
kernel path's algorithmic flops and bytes against the fp32 MFMA and HBM peaks.  ``--big N``
also times the kernel path alone on a block of N users: the pairwise path is not run there, its
concatenated input alone is N x items x 2E floats (56 GB at 4096 x 26,744 x 128).  One JSON line
per model on stdout.
"""
import argparse
import json

import numpy as np
import torch

from .ncf_engine import NCFEngine

PEAK_FP32_MFMA = 157.3e12      # flop/s (spec)
PEAK_HBM = 8.0e12              # B/s (spec)


def tower(E):
    sizes = [2 * E]
    while sizes[-1] > 8:
        sizes.append(sizes[-1] // 2)
    return sizes


def make_engine(E, M, U, I, dev):
    """Reference-style init: N(0, 1) embeddings, Xavier-uniform weights, bias 0.01."""
    g = torch.Generator().manual_seed(0)
    sizes = tower(E)
    mlp = []
    for i, o in list(zip(sizes[:-1], sizes[1:])) + [(8 + M, 1)]:
        lim = (6.0 / (i + o)) ** 0.5
        mlp += [(torch.rand(o, i, generator=g) * 2 - 1) * lim, torch.full((o,), 0.01)]
    tabs = dict(mf_user_w=torch.randn(U, M, generator=g), mf_item_w=torch.randn(I, M, generator=g)) if M else {}
    return NCFEngine(torch.randn(U, E, generator=g), torch.randn(I, E, generator=g), mlp, np.zeros(4, np.int64),
                     np.zeros(4, np.int64), np.zeros(625, np.uint32), device=dev, **tabs)


def algorithmic(E, M, n, I):
    """Flops and compulsory bytes of one block on the kernel path (2 flops per MAC)."""
    sizes = tower(E)
    narrow = sum(i * o for i, o in zip(sizes[1:-1], sizes[2:])) + 8      # per pair, after the split layer
    pair = narrow + M + E                                                 # + GMF dot + the halves' add
    halves = (I + n) * E * E + n * M
    flops = 2.0 * (n * I * pair + halves)
    bytes_ = 4.0 * (n * I + I * (E + M) + n * (E + M))                    # block written, tables read once
    return flops, bytes_


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=256)
    ap.add_argument("--items", type=int, default=26744)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big", type=int, default=0)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    U, I, n = 138493, args.items, args.users
    out = []
    for name, E, M in (("ncf_e64", 64, 0), ("neumf_e16_m50", 16, 50)):
        e = make_engine(E, M, U, I, dev)
        users = torch.from_numpy(np.random.RandomState(1).randint(0, U, n)).to(dev)
        pu, pi = users.repeat_interleave(I), torch.arange(I, device=dev).repeat(n)
        new = lambda: e.score_users(users)
        old = lambda: e.scores(pu, pi)
        for _ in range(3):                                   # warm-up: code objects, GEMM algorithms, allocator
            a, b = new(), old().reshape(n, I)
        torch.cuda.synchronize()
        diff = (a - b).abs()
        rel = float((diff / b.abs()).max())
        t_new, t_old = [], []
        for _ in range(args.reps):                           # alternate the two paths
            t_new += timed(new, 1)
            t_old += timed(old, 1)
        flops, bytes_ = algorithmic(E, M, n, I)
        tn = min(t_new) * 1e-3
        r = {"model": name, "users": n, "items": I, "reps": args.reps,
             "kernel_ms": {"min": min(t_new), "median": float(np.median(t_new))},
             "pairwise_ms": {"min": min(t_old), "median": float(np.median(t_old))},
             "speedup_min": min(t_old) / min(t_new), "speedup_median": float(np.median(t_old) / np.median(t_new)),
             "max_abs_diff": float(diff.max()), "max_rel_diff": rel,
             "gflop": flops / 1e9, "mbytes": bytes_ / 1e6,
             "frac_fp32_mfma_peak": flops / tn / PEAK_FP32_MFMA, "frac_hbm_peak": bytes_ / tn / PEAK_HBM}
        if args.big:
            ub = torch.from_numpy(np.random.RandomState(2).randint(0, U, args.big)).to(dev)
            big = lambda: e.score_users(ub)
            big()
            tb = timed(big, max(3, args.reps // 4))
            fb, _ = algorithmic(E, M, args.big, I)
            r["big"] = {"users": args.big, "kernel_ms": {"min": min(tb), "median": float(np.median(tb))},
                        "frac_fp32_mfma_peak": fb / (min(tb) * 1e-3) / PEAK_FP32_MFMA,
                        "pairwise": "not run: its concatenated input alone is users x items x 2E floats"}
        print(json.dumps(r), flush=True)
        out.append(r)
        del e
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
