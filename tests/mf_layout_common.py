"""The embedding dims of the MF-step and list-scoring tests, by the row layout each selects (no tests
here, and nothing from the GPU side is imported).

Every kernel that walks embedding rows takes its lane layout from ``dim`` through ``dispatch_dim``
(csrc/rg_common.h): ``RowLayout<LPU, EPL, VEC>`` spreads a row over LPU lanes with EPL elements
per lane.  The scalar layouts are one ladder, ``dispatch_scalar``, which is ``dispatch_dim``'s tail;
the kernels that are handed tables they do not own (fold-in, list scoring, ALS, the sequence model)
go through ``dispatch_rows``: ``dispatch_dim`` on 16-byte aligned tables, ``dispatch_scalar`` else.

* float4 (``VEC``), one float4 per lane, no mask:
  8 -> ``<2,4,true>``, 16 -> ``<4,4,true>``, 32 -> ``<8,4,true>``, 64 -> ``<16,4,true>``,
  128 -> ``<32,4,true>``, 256 -> ``<64,4,true>``.
* scalar (``!VEC``): lane ``sub`` holds columns ``sub + LPU * e`` and masks them with ``c < D``:
  1..15 (16 is float4)      -> ``<16,1>``   here 1, 7, 15
  17..31 (32 is float4)     -> ``<16,2>``   here 17, 24, 31
  33..63 (64 is float4)     -> ``<16,4>``   here 33, 50, 63
  65..127 (128 is float4)   -> ``<64,2>``   here 65, 100, 127
  129..192                  -> ``<64,3>``   here 129, 160, 191, 192
  193..255 (256 is float4)  -> ``<64,4>``   here 193, 200, 255

Per scalar layout the table holds the first dim of its range (the last element live on lane 0
alone), an interior dim, and the last dim (the last element dead on one lane alone); ``<64,3>``,
the one layout whose elements per lane are no power of two, also its full row 192, which needs no
mask and, not being one of dispatch_dim's six sizes, takes scalar loads although 192 % 4 == 0.
``<16,1>`` starts at 1 (a row on lane 0 alone).

rg_mf_score_lists adds one branch of its own to ``dispatch_rows`` (csrc/rg_cand.hip: ``VecLayout``,
a float4 per lane at the aligned multiples of 4 off the six sizes); tests/candidates_common.py lists
its dims by layout."""

LAYOUT_DIMS = {
    "<16,1>": [1, 7, 15],
    "<16,2>": [17, 24, 31],
    "<16,4>": [33, 50, 63],
    "<64,2>": [65, 100, 127],
    "<64,3>": [129, 160, 191, 192],
    "<64,4>": [193, 200, 255],
    "float4": [8, 16, 32, 64, 128, 256],
}
SCALAR_LAYOUTS = [k for k in LAYOUT_DIMS if k != "float4"]

# what test_mf_step_dims ran before this table existed
OLD_STEP_DIMS = [8, 16, 32, 50, 64, 100, 128, 200, 256, 1, 7]
NEW_STEP_DIMS = [d for dims in LAYOUT_DIMS.values() for d in dims if d not in OLD_STEP_DIMS]

# one interior dim per scalar layout, then the first dim of <16,2> and the first, last and full row
# of <64,3>: the two layouts no test selected before
EDGE_DIMS = [LAYOUT_DIMS[k][1] for k in SCALAR_LAYOUTS] + [17, 129, 191, 192]


def layout_of(dim):
    """The key of LAYOUT_DIMS that ``dispatch_dim(dim)`` selects."""
    if dim in LAYOUT_DIMS["float4"]:
        return "float4"
    for key, top in zip(SCALAR_LAYOUTS, (16, 32, 64, 128, 192, 256)):
        if 1 <= dim <= top:
            return key
    raise ValueError(dim)


# ---------------------------------------------------------------- the new cases of the GPU tests
# Every call of test_mf_gpu.run_parity that the layout work adds, as its keyword arguments: the GPU
# tests run exactly these, and tests/test_parity_cpu.py first steps the oracle alone over the same
# inputs (another fp32 summation order must pass the criterion the GPU result is held to).
PLAN_DIMS_OLD, PLAN_DIMS_NEW = [8, 32, 50, 64, 128, 256], [24, 100, 160, 200]
HOT_DIMS_OLD, HOT_DIMS_NEW = [64], [24, 160]
SCORE_VAL_DIMS_OLD = [64]
SCORE_VAL_DIMS_NEW = EDGE_DIMS + [8, 16, 32, 128, 256]
MF_LOSSES = ["pointwise", "bpr", "hinge", "adaptive_hinge"]


def step_dims_calls(d):
    return [dict(U=200, I=150, d=d, B=64, n=5, loss="bpr", opt="adam"),
            dict(U=200, I=150, d=d, B=64, n=3, loss="pointwise", opt="adam")]


def plan_calls(d, loss):
    return [dict(U=300, I=200, d=d, B=256, n=5, loss=loss, opt=opt, plan=True, hot=(d == 64))
            for opt in ("adam", "sgd")]


def hot_calls(d, loss, plan):
    return [dict(U=50, I=40, d=d, B=256, n=5, loss=loss, opt="adam", hot=True, plan=plan)]


def score_val_calls(d):
    return [dict(U=300, I=200, d=d, B=128, n=5, loss="pointwise", opt="adam")]


def new_parity_calls():
    """The distinct oracle problems among the new calls (``plan`` does not reach the oracle)."""
    calls = [c for d in NEW_STEP_DIMS for c in step_dims_calls(d)]
    calls += [c for d in PLAN_DIMS_NEW for loss in MF_LOSSES for c in plan_calls(d, loss)]
    calls += [c for d in HOT_DIMS_NEW for loss in ("pointwise", "bpr") for c in hot_calls(d, loss, False)]
    calls += [c for d in SCORE_VAL_DIMS_NEW for c in score_val_calls(d)]
    out, seen = [], set()
    for c in calls:
        c = {k: v for k, v in c.items() if k != "plan"}
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


# test_mf_gradients_elementwise: (loss, hot, d)
GRAD_CASES_OLD = [("pointwise", False, 64), ("bpr", False, 64), ("hinge", False, 64), ("adaptive_hinge", False, 64),
                  ("bpr", True, 64), ("bpr", False, 8), ("bpr", False, 50), ("bpr", False, 200),
                  ("pointwise", True, 256), ("bpr", True, 128)]
# d = 1 runs pointwise, not bpr: with one column the N(0, 1) tables saturate the sigmoid, and under
# bpr the fp32 oracle's own gradient is 1.25 times the bound away from the float64 gradient on one
# element (step 2, user row 180), so no fp32 implementation could be held to it there; pointwise at
# d = 1 stays at 0.08 of the bound (tests/test_parity_cpu.py asserts both distances for every case)
GRAD_CASES_NEW = [("pointwise", False, 1)] + [("bpr", False, d) for d in (16, 24, 32, 100, 129, 160, 191, 192)] + \
                 [("pointwise", True, 160), ("bpr", True, 24)]
