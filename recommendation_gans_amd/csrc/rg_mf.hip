// Matrix-factorisation training step for gfx950 (MI355X).
//
// Replaces, per step (implicit.py:347-364 run_train_iteration):
//   BilinearNet.forward on B positives and n*B negatives
//       (spotlight/factorization/representations.py:62-91),
//   the loss (spotlight/losses.py: pointwise :20, bpr :59, hinge :99, adaptive :133),
//   loss.backward() -> embedding_dense_backward into dense (U,d),(I,d),(U,1),(I,1) grads,
//   optimizer.step() (spotlight/optimizers.py) over EVERY row (coupled L2).
//
// Two kernels per step, both HBM-bound:
//   mf_pairs  one "unit" = one batch column b: its positive and its n negatives
//             (flat draws k*B + b).  LPU lanes per unit, one float4 of every
//             gathered row per lane, dot products by DPP row reductions, loss
//             terms, dL/dz.  Instead of scatter-adding row gradients with float
//             atomics (memory-side, ~1.3 TB/s chip-wide) each pair appends a
//             4+4-byte {other row, dz} entry to the list of each of its two rows
//             (one returning int atomic per row); rows touched more than
//             RG_MF_LIST_CAP times spill the excess into dense overflow
//             accumulators with float atomics (Zipf-hot items only).
//   mf_apply  streams every row of both tables once: p, m, v in; the row's
//             gradient is PULLED from its list (gathering the other table's
//             pre-step row, which is why the parameter tables ping-pong) plus
//             weight_decay * p; Adam / SGD / RMSprop; p', m, v out; the list
//             counter and overflow accumulators are reset in the same pass.
//
// This file: the kernels the product path launches (prepare, pair pass, adaptive max, dense
// pass / apply, scores, loss) and every entry point of that path -- rg_mf_prepare* ->
// rg_mf_pairs -> rg_mf_apply_prepare[_gen], the data-parallel and owner shard entries, and
// the NCF / NeuMF entries that reuse the dense pass.  The device bodies the kernels are made
// of are in rg_mf_kernels.h; the whole-step alternatives of the A/B build (overlapped,
// pipelined, two-launch pipelined, lazy) are in rg_mf_alt.hip.  The per-kernel variants inside
// ApplyLaunchF / BackLaunchF only select template arguments of this file's kernels.
#include <algorithm>
#include <type_traits>
#include <cstdlib>

#include <hip/hip_ext.h>

#include "rg_common.h"

#ifdef RG_DIAG_STAMPS
namespace rg {
// the pair-pass stamps of the diagnostic build (rg_mf_kernels.h RG_STAMP / RG_DIAG_FLAG): only
// the kernels of this translation unit record them
__device__ unsigned long long *g_diag_stamps;
__device__ int g_diag_flags;   // timing only (results are wrong): bit 0 skip the list-slot atomics,
                               // bit 1 skip the list-entry stores, bit 2 skip the planned partial rows,
                               // bit 3 return right after the ids
}  // namespace rg
#endif
#include "rg_mf_kernels.h"

namespace rg {

__global__ __launch_bounds__(kBlock) void mf_prepare_kernel(PairsArgs a, int2 *__restrict__ out, int prio) {
    if (prio) __builtin_amdgcn_s_setprio(2);   // small latency-bound kernel running beside the HBM-bound apply
    prepare_one(a, out, (int64_t)blockIdx.x * kBlock + threadIdx.x);
}

template <class L, int PHASE, int NMAX>
__global__ __launch_bounds__(kPairBlock) void mf_pairs_kernel(PairsArgs a) {
    pairs_body<L, PHASE, NMAX>(a, blockIdx.x);
}

// adaptive hinge: the global-max negative receives sum_b 1/Bp over active b
// (spotlight/losses.py:170 torch.max(dim 0) backward -> argmax, first index on ties)
template <class L>
__global__ __launch_bounds__(kWave) void mf_adapt_max_kernel(PairsArgs a) {
    constexpr int LPU = L::LPU, EPL = L::EPL;
    const int lane = threadIdx.x;
    const int sub = lane & (LPU - 1);
    const unsigned long long key = *a.max_key;
    const int64_t j = (int64_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
    const int64_t colg = j % a.global_cols;
    const int64_t col = colg - a.col_offset;
    if (col < 0 || col >= a.cols) return;            // another rank owns the max
    if (lane >= LPU) return;
    const float pm = __uint_as_float((uint32_t)(key >> 32));
    const float dpv = (float)(*a.active_count) * (1.0f / a.n_a);
    const float dz = (dpv * (1.0f - pm)) * pm;
    const uint2 w = a.words[j];
    const int2 pr = a.pool[choice_index(w.x, w.y, a.pool_len)];
    float ur[EPL], ir[EPL];
    L::load(ur, a.user_w, pr.x, a.dim, sub);
    L::load(ir, a.item_w, pr.y, a.dim, sub);
    for (int side = 0; side < 2; ++side) {
        const int64_t row = side ? a.num_users + pr.y : (int64_t)pr.x;
        int sl = 0;
        if (sub == 0) sl = atomicAdd(a.row_count + row, 1);
        sl = __shfl(sl, 0);
        if (sl < kCap) {
            if (sub == 0) store_entry(a.row_list + row * kCap + sl, side ? pr.x : pr.y, dz);
        } else {
            overflow_add<L>(a.hot_grad, row, a.dim, sub, dz, side ? ur : ir);
            if (sub == 0) fix_add(a.hot_bias_grad + row, dz);
        }
    }
}

// Streams every row of [row_begin, row_end) once (item rows first, so the few
// long Zipf-hot item rows start early instead of trailing the grid).
// NT: 1 = streaming stores of the updated p, m, v; 2 = also streaming loads of the
// pre-step p, m, v (each touched once per step)
template <class L, int MODE, int NT = 0, bool SPEC = false>
__global__ __launch_bounds__(kBlock) void mf_apply_kernel(ApplyArgs a) {
    constexpr int LPU = L::LPU, UPW = L::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t k = wave * UPW + (lane / LPU);
    const int64_t rb = a.row_begin, re = a.row_end, nr = re - rb;
    const int D = a.dim;

    const int64_t slot_off = (a.shard_users + a.shard_items) * (int64_t)(D + 1);   // loss slot in a chunk
    if (MODE != kApplyDense && a.loss_out != nullptr && blockIdx.x == 0) {
        const float lv = finalize_loss_wg<kBlock>(a.partials, a.n_partials, a.inv_a, a.inv_b);
        if (threadIdx.x < kWave) {
            if (lane == 0) *a.loss_out = lv;
            if (MODE == kGradOnly && (a.shard_users > 0 || a.item_shard)) {
                for (int s = lane; s < a.world; s += kWave) a.grad[s * a.chunk + slot_off] = lv;   // summed by the RS
            } else if (MODE == kGradOnly && lane == 0) {
                a.grad[nr * (int64_t)(D + 1)] = lv;
            }
        }
    }
    if (MODE == kApplyDense && a.loss_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
        *a.loss_out = (a.shard_users > 0 || a.item_shard) ? a.grad[a.rank * a.chunk + slot_off]
                                                         : a.grad[nr * (int64_t)(D + 1)];

    if (k >= nr) return;
    int64_t r;
    if (MODE == kApplyDense && a.item_shard) {
        r = a.num_users + a.rank * a.shard_items + k;         // this rank's item shard only
    } else if (MODE == kApplyDense && a.shard_users > 0) {
        // this rank's shard: [rb, rb + nu) users, then items from U + rank * Is
        const int64_t u0 = a.rank * a.shard_users, i0 = a.rank * a.shard_items;
        const int64_t u1 = u0 + a.shard_users < a.num_users ? u0 + a.shard_users : a.num_users;
        const int64_t nu = u1 > u0 ? u1 - u0 : 0;
        r = k < nu ? u0 + k : a.num_users + i0 + (k - nu);
    } else {
        const int64_t ia0 = rb > a.num_users ? rb : a.num_users;      // item part [ia0, re)
        const int64_t ni = re > ia0 ? re - ia0 : 0;
        r = k < ni ? ia0 + k : rb + (k - ni);
    }
    apply_row<L, MODE, NT, false, SPEC>(a, r, sub);
}

// the dense update of rows [row_begin, row_end) (blocks [0, apply_blocks), as
// mf_apply_kernel) and the prepare pass of the NEXT step (the remaining blocks) in one
// launch: the split step then needs no side stream and no per-step cross-stream event
// Optional: workgroup 0 walks a LATER step's MT19937 words (rg_mt_gen_t) -- the walk
// (~0.47 ns/word, one workgroup) hides under the HBM-bound pass, so a single-GPU step
// needs no generator stream and no cross-stream event.
template <class L, int NT, bool SPEC = false, bool OWN = false, bool LAZY = false, bool LSPEC = false>
__global__ __launch_bounds__(kBlock) void mf_back_kernel(ApplyArgs a, PairsArgs prep, int2 *prep_out,
                                                         int64_t apply_blocks, MtGenArgs gen, BackGrid bg,
                                                         OwnerArgs own, MlpUpdArgs upd) {
    static_assert(kBlock == kOwnSeg, "an owner prepare segment is one workgroup");
    static_assert(kBlock == kGenThreads, "the MT walk runs on one full workgroup");
    const int64_t B = blockIdx.x;
    int64_t blk = B;
    if (gen.nwords > 0) {
        if (B == 0) {
            __shared__ uint32_t X[kRing + 2];
            mt_generate_block(X, gen.state, gen.out, gen.nwords, gen.state_before);
            return;
        }
        --blk;
    }
    // the next step's prepare (latency-bound random pool reads) in the FIRST blocks, so it
    // overlaps the streaming rows instead of trailing the grid (RG_PREP_FIRST=0: last)
    if (bg.prep_first) {
        if (blk < bg.prep_blocks) {
            if (OWN) owner_prepare_block(own, blk);
            else prepare_one(prep, prep_out, blk * kBlock + threadIdx.x);
            return;
        }
        if (blk < bg.prep_blocks + bg.upd_blocks) {             // the NCF step's MLP update
            __shared__ float red[kMlpSlices][64];
            mlp_update_block<kBlock / kWave>(upd, blk - bg.prep_blocks, red);
            return;
        }
        if (B < bg.apply_start) return;                         // alignment padding
        blk = B - bg.apply_start;
        if (bg.xcd_map) blk = (blk & 7) * (bg.apply_padded >> 3) + (blk >> 3);
        if (blk >= apply_blocks) return;
    } else if (blk >= apply_blocks) {
        if (OWN) owner_prepare_block(own, blk - apply_blocks);
        else prepare_one(prep, prep_out, (blk - apply_blocks) * kBlock + threadIdx.x);
        return;
    }
    constexpr int LPU = L::LPU, UPW = L::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t wave = (blk * kBlock + threadIdx.x) >> 6;
    const int64_t k = wave * UPW + (lane / LPU);
    const int64_t rb = a.row_begin, re = a.row_end, nr = re - rb;
    if (a.loss_out != nullptr && blk == 0 && threadIdx.x < kWave) {
        const float lv = finalize_loss(a.partials, a.n_partials, a.inv_a, a.inv_b, lane);
        if (lane == 0) *a.loss_out = lv;
    }
    const int64_t ia0 = rb > a.num_users ? rb : a.num_users;      // item rows first, as mf_apply_kernel
    const int64_t ni = re > ia0 ? re - ia0 : 0;
    const int64_t r = k < ni ? ia0 + k : rb + (k - ni);
    if (LAZY) {
        // a user row's decision words first (the row's loads depend on them)
        if ((wave * UPW) >= nr) return;                     // wave-uniform: the catch-up loop is per wave
        const bool in = k < nr;
        const int64_t rr = in ? r : rb;
        LazyRow lzr{0, 0, 0, in};
        if (in && rr < a.num_users) {
            lzr.cnt = a.row_count[rr];
            lzr.mk = a.umark[rr];
            lzr.lsr = a.last_rel[rr];
        }
        // a lane group past the end runs as an inactive user row (row 0: no loads, no stores)
        apply_row<L, kApplyPull, NT, false, SPEC, true, LSPEC>(a, in ? r : 0, sub, lzr);
        return;
    }
    if (k >= nr) return;
    apply_row<L, kApplyPull, NT, false, SPEC>(a, r, sub);
}

// The single-GPU dense pass as a software pipeline (the default split step): a grid of a few
// workgroups per CU whose waves each walk a contiguous chunk of row groups (UPW rows per group),
// the NEXT group's independent loads (p, m, v, biases, count, list entries, slot range) issued
// before this group's dependent ones (partner rows, planned partials).  One memory round trip
// per group instead of two: in mf_back_kernel a touched row's wave waited for its list, then for
// its partner rows, with nothing else in flight (rows with a contribution are ~40 % of all,
// ~87 % of the 4-row groups).  Grid as mf_back_kernel's: [MT walk] [next prepare] [pad] [dense].
template <class L>
__global__ __launch_bounds__(kBlock) void mf_dense_kernel(ApplyArgs a, PairsArgs prep, int2 *prep_out,
                                                          int64_t dense_blocks, MtGenArgs gen, BackGrid bg) {
    const int64_t B = blockIdx.x;
    int64_t blk = B;
    if (gen.nwords > 0) {
        if (B == 0) {
            __shared__ uint32_t X[kRing + 2];
            mt_generate_block(X, gen.state, gen.out, gen.nwords, gen.state_before);
            return;
        }
        --blk;
    }
    if (blk < bg.prep_blocks) {
        prepare_one(prep, prep_out, blk * kBlock + threadIdx.x);
        return;
    }
    if (B < bg.apply_start) return;                         // alignment padding
    blk = B - bg.apply_start;
    if (blk >= dense_blocks) return;
    constexpr int LPU = L::LPU, UPW = L::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t rb = a.row_begin, re = a.row_end, nr = re - rb;
    if (a.loss_out != nullptr && blk == 0 && threadIdx.x < kWave) {
        const float lv = finalize_loss(a.partials, a.n_partials, a.inv_a, a.inv_b, lane);
        if (lane == 0) *a.loss_out = lv;
    }
    const int64_t ia0 = rb > a.num_users ? rb : a.num_users;      // item rows first, as mf_apply_kernel
    const int64_t ni = re > ia0 ? re - ia0 : 0;
    // this wave's row groups [g0, g1): contiguous, so a wave's stores fill whole lines
    const int64_t waves = dense_blocks * (kBlock / kWave);
    const int64_t wave = (blk * kBlock + threadIdx.x) >> 6;
    const int64_t groups = (nr + UPW - 1) / UPW;
    const int64_t per = (groups + waves - 1) / waves;
    const int64_t g0 = wave * per, g1 = g0 + per < groups ? g0 + per : groups;
    if (g0 >= g1) return;                                   // wave-uniform
    auto row_of = [&](int64_t g, bool &valid) {
        const int64_t k = g * UPW + lane / LPU;
        valid = k < nr;
        const int64_t kk = valid ? k : 0;
        return kk < ni ? ia0 + kk : rb + (kk - ni);
    };
    LeanRow<L> cur, nxt;
    bool vc, vn;
    int64_t rc = row_of(g0, vc), rn = 0;
    lean_load<L>(a, rc, sub, vc, cur);
    for (int64_t g = g0; g < g1; ++g) {
        const bool more = g + 1 < g1;                       // wave-uniform
        if (more) {
            rn = row_of(g + 1, vn);
            lean_load<L>(a, rn, sub, vn, nxt);
        }
        lean_finish<L>(a, rc, sub, vc, cur);
        if (!more) break;
        cur = nxt;
        rc = rn;
        vc = vn;
    }
}

// ---------------------------------------------------------------------------- scores / loss
template <class L>
__global__ __launch_bounds__(kBlock) void mf_scores_kernel(const float *__restrict__ uw, const float *__restrict__ iw,
                                                           const float *__restrict__ ub, const float *__restrict__ ib,
                                                           int D, const int64_t *__restrict__ users,
                                                           const int64_t *__restrict__ items, int64_t n,
                                                           float *__restrict__ out) {
    constexpr int LPU = L::LPU, EPL = L::EPL, UPW = L::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t k = wave * UPW + (lane / LPU);
    float ur[EPL], ir[EPL];
    L::zero(ur);
    L::zero(ir);
    int64_t u = 0, i = 0;
    if (k < n) {
        u = users[k];
        i = items[k];
        L::load(ur, uw, u, D, sub);
        L::load(ir, iw, i, D, sub);
    }
    // row_dot (rg_common.h) written out: through the helper the compiler allocates the two id
    // registers the other way round, and this kernel is kept instruction for instruction
    float d = 0.0f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) d = fmaf(ur[e], ir[e], d);
    d = group_sum<LPU>(d);      // all lanes converged here (DPP)
    if (k < n && sub == 0) out[k] = sigmoidf_ref((d + ub[u]) + ib[i]);
}

__global__ __launch_bounds__(kWave) void loss_finalize_kernel(const float *__restrict__ partials, int64_t np_,
                                                              double inv_a, double inv_b, float *out) {
    const float lv = finalize_loss(partials, np_, inv_a, inv_b, threadIdx.x);
    if (threadIdx.x == 0) *out = lv;
}

}  // namespace rg

using namespace rg;

namespace {
struct PartialsLenF {
    int64_t cols;
    int64_t *nb;
    template <class L>
    int operator()() { *nb = pairs_blocks<L>(cols); return 0; }
};

struct UnitsPerBlockF {
    int64_t *upb;
    template <class L>
    int operator()() { *upb = kPairBlock / L::LPU; return 0; }
};

struct PairsLaunchF {
    PairsArgs *a;
    hipStream_t s;
    bool adaptive, backward;
    template <class L>
    int operator()() {
        if (a->n_neg <= 5) return run<L, 5>();
        return run<L, kNMax>();
    }
    template <class L, int NMAX>
    int run() {
        const int64_t nb = pairs_blocks<L>(a->cols);
        if (!adaptive) {
            if (backward)
                hipLaunchKernelGGL((mf_pairs_kernel<L, kFused, NMAX>), dim3(nb), dim3(kPairBlock), 0, s, *a);
            else
                hipLaunchKernelGGL((mf_pairs_kernel<L, kLossOnly, NMAX>), dim3(nb), dim3(kPairBlock), 0, s, *a);
            return check_launch("rg_mf_pairs");
        }
        if (hipMemsetAsync(a->max_key, 0, sizeof(unsigned long long), s) != hipSuccess ||
            hipMemsetAsync(a->active_count, 0, sizeof(int32_t), s) != hipSuccess)
            return check_launch("rg_mf_pairs(adaptive memset)");
        hipLaunchKernelGGL((mf_pairs_kernel<L, kAdaptFwd, NMAX>), dim3(nb), dim3(kPairBlock), 0, s, *a);
        if (backward) {
            hipLaunchKernelGGL((mf_pairs_kernel<L, kAdaptBwd, NMAX>), dim3(nb), dim3(kPairBlock), 0, s, *a);
            hipLaunchKernelGGL((mf_adapt_max_kernel<L>), dim3(1), dim3(kWave), 0, s, *a);
        } else {
            hipLaunchKernelGGL((mf_pairs_kernel<L, kAdaptLoss, NMAX>), dim3(nb), dim3(kPairBlock), 0, s, *a);
        }
        return check_launch("rg_mf_pairs(adaptive)");
    }
};

struct ApplyLaunchF {
    ApplyArgs *a;
    hipStream_t s;
    int mode;
    template <class L>
    int operator()() {
        // MF rows (not NCF's contribution rows) on the dense pass's layout: the item gradient and
        // item update of the data-parallel steps, element-wise like the dense pass
        using LB = typename BackLayout<L>::type;
        if constexpr (!std::is_same<LB, L>::value) {
            if (a->contrib == nullptr) return run<LB>();
        }
        return run<L>();
    }
    template <class L>
    int run() {
        const int64_t rows = a->row_end - a->row_begin;
        if (rows <= 0 && a->loss_out == nullptr) return RG_OK;
        const int64_t waves = (rows + L::UPW - 1) / L::UPW;
        int64_t nb = (waves + kBlock / kWave - 1) / (kBlock / kWave);
        if (nb < 1) nb = 1;
#if RG_AB
        // A/B build only (measured no faster): non-temporal stores, the list loaded
        // beside the count
        static const int nt = [] { const char *e = getenv("RG_APPLY_NT"); return e ? atoi(e) : 0; }();
        static const int spec = [] { const char *e = getenv("RG_APPLY_SPEC"); return e ? atoi(e) : 0; }();
        if (mode == kApplyPull && spec && nt == 1)
            hipLaunchKernelGGL((mf_apply_kernel<L, kApplyPull, 1, true>), dim3(nb), dim3(kBlock), 0, s, *a);
        else if (mode == kApplyPull && spec)
            hipLaunchKernelGGL((mf_apply_kernel<L, kApplyPull, 0, true>), dim3(nb), dim3(kBlock), 0, s, *a);
        else if (mode == kApplyPull && nt == 1)
            hipLaunchKernelGGL((mf_apply_kernel<L, kApplyPull, 1>), dim3(nb), dim3(kBlock), 0, s, *a);
        else if (mode == kApplyPull && nt >= 2)
            hipLaunchKernelGGL((mf_apply_kernel<L, kApplyPull, 2>), dim3(nb), dim3(kBlock), 0, s, *a);
        else
#endif
        if (mode == kApplyPull)
            hipLaunchKernelGGL((mf_apply_kernel<L, kApplyPull>), dim3(nb), dim3(kBlock), 0, s, *a);
        else if (mode == kGradOnly)   // list and slot range loaded beside the count
            hipLaunchKernelGGL((mf_apply_kernel<L, kGradOnly, 0, true>), dim3(nb), dim3(kBlock), 0, s, *a);
        else
            hipLaunchKernelGGL((mf_apply_kernel<L, kApplyDense>), dim3(nb), dim3(kBlock), 0, s, *a);
        return check_launch("rg_mf_apply");
    }
};

struct ScoresLaunchF {
    const float *uw, *iw, *ub, *ib;
    int dim;
    const int64_t *users, *items;
    int64_t n;
    float *out;
    hipStream_t s;
    template <class L>
    int operator()() {
        const int64_t waves = (n + L::UPW - 1) / L::UPW;
        const int64_t nb = (waves + kBlock / kWave - 1) / (kBlock / kWave);
        hipLaunchKernelGGL((mf_scores_kernel<L>), dim3(nb), dim3(kBlock), 0, s, uw, iw, ub, ib, dim, users, items,
                           n, out);
        return check_launch("rg_mf_scores");
    }
};
}  // namespace

extern "C" int64_t rg_mf_pairs_len(int64_t cols, int32_t n_neg) {
    if (cols <= 0 || n_neg < 1 || n_neg > kNMax) return -1;
    return 2 * (int64_t)pair_stride(n_neg) * cols;
}

extern "C" int64_t rg_mf_partials_len(int64_t cols, int32_t dim) {
    int64_t nb = -1;
    PartialsLenF f{cols, &nb};
    if (dispatch_dim(dim, f) != 0) return -1;
    return 2 * nb;
}

extern "C" int64_t rg_mf_plan_units_per_block(int32_t dim) {
    int64_t upb = -1;
    UnitsPerBlockF f{&upb};
    if (dispatch_dim(dim, f) != 0) return -1;
    return upb;
}

int rg::check_tables(const rg_mf_tables_t *t) {
    if (t == nullptr) return fail_arg("null tables");
    if (!t->user_w || !t->item_w || !t->user_b || !t->item_b) return fail_arg("null parameter table");
    if (t->num_users <= 0 || t->num_items <= 0) return fail_arg("empty table");
    if (t->num_users + t->num_items >= (int64_t)1 << 31) return fail_arg("num_users + num_items must be < 2^31");
    if (t->dim < 1 || t->dim > 256) return fail_arg("dim must be in [1, 256]");
    return RG_OK;
}

int rg::pairs_args(const rg_mf_tables_t *t, const rg_mf_batch_t *b, const rg_mf_work_t *w, int32_t backward,
                   PairsArgs &a) {
    int rc = check_tables(t);
    if (rc) return rc;
    if (b == nullptr || w == nullptr) return fail_arg("rg_mf_pairs: null batch/work");
    if (b->n_neg < 1 || b->n_neg > kNMax) return fail_arg("rg_mf_pairs: n_neg must be in [1, 8]");
    if (b->cols <= 0 || b->n_pos < 0 || b->n_pos > b->cols) return fail_arg("rg_mf_pairs: bad n_pos/cols");
    if (b->col_offset < 0 || b->col_offset + b->cols > b->global_cols) return fail_arg("rg_mf_pairs: bad column slice");
    if (b->global_pos <= 0 && b->loss != RG_LOSS_POINTWISE && b->loss != RG_LOSS_POINTWISE_POS)
        return fail_arg("rg_mf_pairs: empty global batch");
    if (b->pool_len <= 0 || !b->pool || !b->words) return fail_arg("rg_mf_pairs: empty pool / no words");
    if (b->n_pos > 0 && (!b->pos_user || !b->pos_item)) return fail_arg("rg_mf_pairs: null positives");
    if (b->loss < 0 || b->loss > RG_LOSS_POINTWISE_POS) return fail_arg("rg_mf_pairs: bad loss kind");
    if (!w->loss_partials) return fail_arg("rg_mf_pairs: null loss_partials");
    if (backward && (!w->row_count || !w->row_list || !w->hot_grad || !w->hot_bias_grad))
        return fail_arg("rg_mf_pairs: null backward scratch");
    const bool adaptive = b->loss == RG_LOSS_ADAPTIVE_HINGE;
    if (adaptive && (!w->scores || !w->max_key || !w->active_count))
        return fail_arg("rg_mf_pairs: adaptive hinge needs scores/max_key/active_count");
    if (w->plan_perm && (!w->plan_pos_slot || !w->part_row || !w->part_bias || !w->plan_item_slot_off))
        return fail_arg("rg_mf_pairs: incomplete plan");

    a = PairsArgs{};
    a.user_w = t->user_w; a.item_w = t->item_w; a.user_b = t->user_b; a.item_b = t->item_b;
    a.num_users = t->num_users; a.dim = t->dim;
    a.pos_user = b->pos_user; a.pos_item = b->pos_item;
    a.n_pos = b->n_pos; a.cols = b->cols; a.col_offset = b->col_offset; a.global_cols = b->global_cols;
    a.words = reinterpret_cast<const uint2 *>(b->words);
    a.pool = reinterpret_cast<const int2 *>(b->pool);
    a.pool_len = b->pool_len; a.n_neg = b->n_neg; a.loss = b->loss;
    switch (b->loss) {
        case RG_LOSS_POINTWISE:
            a.n_a = (float)b->global_pos;
            a.n_b = (float)((int64_t)b->n_neg * (b->neg_cols > 0 ? b->neg_cols : b->global_cols));
            break;
        case RG_LOSS_BPR:
        case RG_LOSS_HINGE:
            a.n_a = (float)((int64_t)b->n_neg * b->global_pos);
            a.n_b = 1.0f;
            break;
        default:
            a.n_a = (float)b->global_pos;
            a.n_b = 1.0f;
    }
    a.row_count = w->row_count;
    a.row_list = reinterpret_cast<int2 *>(w->row_list);
    a.hot_grad = reinterpret_cast<long long *>(w->hot_grad);
    a.hot_bias_grad = reinterpret_cast<long long *>(w->hot_bias_grad);
    a.partials = w->loss_partials; a.scores = w->scores;
    a.max_key = reinterpret_cast<unsigned long long *>(w->max_key);
    a.active_count = w->active_count;
    if (!b->pairs) return fail_arg("rg_mf_pairs: batch->pairs not prepared (rg_mf_prepare)");
    a.pairs = reinterpret_cast<const int2 *>(b->pairs);
    a.perm = w->plan_perm;
    a.pos_slot = backward ? w->plan_pos_slot : nullptr;   // partials only in the backward pass
    a.part_row = w->part_row; a.part_bias = w->part_bias;
    if (w->claim_num_users > 0) {
        if (w->claim_num_users != t->num_users || t->num_users >= kClaimIdMask || t->num_items >= kClaimIdMask)
            return fail_arg("rg_mf_pairs: claimed slots need claim_num_users == num_users and ids < 2^27");
        if (adaptive) return fail_arg("rg_mf_pairs: no claimed slots for the adaptive hinge");
        a.claimed = 1;
    }
    return RG_OK;
}

extern "C" int rg_mf_pairs(void *stream, const rg_mf_tables_t *t, const rg_mf_batch_t *b, rg_mf_work_t *w,
                           int32_t backward) {
    PairsArgs a;
    int rc = pairs_args(t, b, w, backward, a);
    if (rc) return rc;
    PairsLaunchF f{&a, (hipStream_t)stream, b->loss == RG_LOSS_ADAPTIVE_HINGE, backward != 0};
    return dispatch_dim(t->dim, f);
}

int rg::prepare_args(const rg_mf_batch_t *b, const rg_mf_work_t *w, const rg_mf_mark_t *mark, PairsArgs &a) {
    if (!b || !b->pairs) return fail_arg("rg_mf_prepare: null batch/pairs");
    if (b->n_neg < 1 || b->n_neg > kNMax) return fail_arg("rg_mf_prepare: n_neg must be in [1, 8]");
    if (b->cols <= 0 || b->n_pos < 0 || b->n_pos > b->cols) return fail_arg("rg_mf_prepare: bad n_pos/cols");
    if (b->col_offset < 0 || b->col_offset + b->cols > b->global_cols) return fail_arg("rg_mf_prepare: bad slice");
    if (b->pool_len <= 0 || !b->pool || !b->words) return fail_arg("rg_mf_prepare: empty pool / no words");
    if (b->n_pos > 0 && (!b->pos_user || !b->pos_item)) return fail_arg("rg_mf_prepare: null positives");
    if (mark && (!mark->stamp || mark->serial == 0 || mark->num_users <= 0))
        return fail_arg("rg_mf_prepare: bad row marks (stamp, serial != 0, num_users)");
    a = PairsArgs{};
    a.pos_user = b->pos_user; a.pos_item = b->pos_item;
    a.n_pos = b->n_pos; a.cols = b->cols; a.col_offset = b->col_offset; a.global_cols = b->global_cols;
    a.words = reinterpret_cast<const uint2 *>(b->words);
    a.pool = reinterpret_cast<const int2 *>(b->pool);
    a.pool_len = b->pool_len; a.n_neg = b->n_neg;
    a.perm = w ? w->plan_perm : nullptr;
    a.pos_slot = w ? w->plan_pos_slot : nullptr;
    a.loss = b->loss;
    if (mark) {
        a.stamp = mark->stamp;
        a.serial = mark->serial;
        a.num_users = mark->num_users;
    }
    if (w && w->claim_num_users > 0) {
        if (mark) return fail_arg("rg_mf_prepare: claimed slots and row marks are exclusive");
        if (!w->row_count) return fail_arg("rg_mf_prepare: claimed slots need row_count");
        if (b->loss == RG_LOSS_ADAPTIVE_HINGE)
            return fail_arg("rg_mf_prepare: no claimed slots for the adaptive hinge (its lists follow the max)");
        a.claimed = 1;
        a.row_count = w->row_count;
        if (w->claim_num_users >= kClaimIdMask) return fail_arg("rg_mf_prepare: claimed slots need ids < 2^27");
        a.num_users = w->claim_num_users;
    }
    return RG_OK;
}

int rg::launch_prepare(void *stream, const PairsArgs &a, int2 *out, int64_t total, int prio, const char *what) {
    hipLaunchKernelGGL(mf_prepare_kernel, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, a,
                       out, prio);
    return check_launch(what);
}

extern "C" int rg_mf_prepare_marked(void *stream, const rg_mf_batch_t *b, const rg_mf_work_t *w,
                                    const rg_mf_mark_t *mark) {
    PairsArgs a;
    int rc = prepare_args(b, w, mark, a);
    if (rc) return rc;
    const int64_t total = prepare_threads(b->cols, b->n_neg);
#if RG_AB
    static const int prio = [] { const char *e = getenv("RG_PREP_PRIO"); return e ? atoi(e) : 1; }();
#else
    constexpr int prio = 1;
#endif
    return launch_prepare(stream, a, reinterpret_cast<int2 *>(b->pairs), total, prio, "rg_mf_prepare");
}

extern "C" int rg_mf_prepare(void *stream, const rg_mf_batch_t *b, const rg_mf_work_t *w) {
    return rg_mf_prepare_marked(stream, b, w, nullptr);
}

int rg::apply_args(const rg_mf_tables_t *t, const rg_mf_work_t *w, const float *grad_in, float *grad_out,
                   const rg_opt_t *opt, int64_t row_begin, int64_t row_end, const rg_mf_loss_t *loss,
                   float *dense_loss_out, int mode, ApplyArgs &a) {
    int rc = check_tables(t);
    if (rc) return rc;
    const int64_t nrows = t->num_users + t->num_items;
    if (row_begin < 0) row_begin = 0;
    if (row_end < 0 || row_end > nrows) row_end = nrows;
    if (row_begin > row_end) return fail_arg("rg_mf_apply: row_begin > row_end");
    if (mode != kGradOnly) {
        if (!opt) return fail_arg("rg_mf_apply: null opt");
        if (!t->user_w_out || !t->item_w_out || !t->user_b_out || !t->item_b_out)
            return fail_arg("rg_mf_apply: null output tables");
        if ((mode == kApplyPull || mode == kApplyCold) && (t->user_w_out == t->user_w || t->item_w_out == t->item_w ||
                                   t->user_b_out == t->user_b || t->item_b_out == t->item_b))
            return fail_arg("rg_mf_apply: output tables must not alias the inputs (ping-pong)");
        if (opt->kind < RG_OPT_ADAM || opt->kind > RG_OPT_RMSPROP) return fail_arg("rg_mf_apply: bad optimizer");
        if (opt->kind == RG_OPT_ADAM && (!t->user_w_m || !t->item_w_m || !t->user_b_m || !t->item_b_m))
            return fail_arg("rg_mf_apply: Adam needs m state");
        if (opt->kind != RG_OPT_SGD && (!t->user_w_v || !t->item_w_v || !t->user_b_v || !t->item_b_v))
            return fail_arg("rg_mf_apply: optimizer needs v state");
    }
    if (mode != kApplyDense && mode != kApplyCold) {
        if (!w || !w->row_count || !w->row_list || !w->hot_grad || !w->hot_bias_grad)
            return fail_arg("rg_mf_apply: null scratch");
        if (loss && loss->out && !w->loss_partials) return fail_arg("rg_mf_apply: loss needs partials");
    }
    if (mode != kApplyPull && mode != kApplyCold && !(grad_in || grad_out))
        return fail_arg("rg_mf_apply: null gradient buffer");
    a = ApplyArgs{};
    a.w_in[0] = t->user_w; a.w_in[1] = t->item_w; a.b_in[0] = t->user_b; a.b_in[1] = t->item_b;
    a.w_out[0] = t->user_w_out; a.w_out[1] = t->item_w_out; a.b_out[0] = t->user_b_out; a.b_out[1] = t->item_b_out;
    a.w_m[0] = t->user_w_m; a.w_m[1] = t->item_w_m; a.w_v[0] = t->user_w_v; a.w_v[1] = t->item_w_v;
    a.b_m[0] = t->user_b_m; a.b_m[1] = t->item_b_m; a.b_v[0] = t->user_b_v; a.b_v[1] = t->item_b_v;
    a.num_users = t->num_users; a.num_items = t->num_items; a.dim = t->dim;
    a.row_begin = row_begin; a.row_end = row_end;
    if (w) {
        a.row_count = w->row_count; a.row_list = reinterpret_cast<const int2 *>(w->row_list);
        a.hot_grad = reinterpret_cast<long long *>(w->hot_grad);
    a.hot_bias_grad = reinterpret_cast<long long *>(w->hot_bias_grad);
        a.partials = w->loss_partials;
        if (w->plan_perm) {
            a.item_slot_off = w->plan_item_slot_off;
            a.part_row = w->part_row; a.part_bias = w->part_bias;
        }
    }
    if (opt) a.opt = *opt;
    if (mode == kApplyDense) {
        a.loss_out = dense_loss_out;
    } else if (loss) {
        a.n_partials = loss->n_partials; a.inv_a = loss->inv_a; a.inv_b = loss->inv_b;
        a.loss_out = loss->out;
    }
    a.grad = grad_out ? grad_out : const_cast<float *>(grad_in);
    a.has_bias = true;
    return RG_OK;
}

static int apply_common(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const float *grad_in,
                        float *grad_out, const rg_opt_t *opt, int64_t row_begin, int64_t row_end,
                        const rg_mf_loss_t *loss, float *dense_loss_out, int mode) {
    ApplyArgs a;
    int rc = apply_args(t, w, grad_in, grad_out, opt, row_begin, row_end, loss, dense_loss_out, mode, a);
    if (rc) return rc;
    ApplyLaunchF f{&a, (hipStream_t)stream, mode};
    return dispatch_dim(t->dim, f);
}

namespace {
struct BackLaunchF {
    ApplyArgs *a;
    PairsArgs *prep;
    int2 *prep_out;
    int64_t prep_blocks;
    MtGenArgs gen;
    hipStream_t s;
    const OwnerArgs *own = nullptr;   // owner-sharded DP: the next step's owner prepare
    bool lazy = false;                // lazy dense pass (rg_mf_apply_lazy)
    const MlpUpdArgs *upd = nullptr;  // NCF step: the MLP update in the same launch (rg_ncf_tail)
    template <class L>
    int operator()() {
        using LB = typename BackLayout<L>::type;
        if constexpr (!std::is_same<LB, L>::value) {
            // the dense pass (MF single-GPU, an owner rank's user rows, the NCF tail's embedding
            // tables pulling their per-example gradient rows) on its own row layout (BackLayout);
            // element-wise arithmetic, so the same bits as the dispatch layout
            if (!lazy) return run<LB, true>();
        }
        return run<L, false>();
    }
    // V: the dense-pass layout of a plain MF launch (no owner / NCF / lazy / A/B variants)
    template <class L, bool V>
    int run() {
        const int64_t rows = a->row_end - a->row_begin;
        const int64_t waves = (rows + L::UPW - 1) / L::UPW;
        int64_t nb = (waves + kBlock / kWave - 1) / (kBlock / kWave);
        if (nb < 1) nb = 1;
#if RG_AB
        // A/B build only (each measured slower or no faster): prepare blocks after the
        // dense blocks, the XCD-aware dense mapping, non-temporal stores, the list read after the
        // count, the persistent pipelined dense kernel
        static const int prep_first = [] { const char *e = getenv("RG_PREP_FIRST"); return e ? atoi(e) : 1; }();
        static const int xcd_map = [] { const char *e = getenv("RG_XCD_MAP"); return e ? atoi(e) : 0; }();
        static const int nt = [] { const char *e = getenv("RG_APPLY_NT"); return e ? atoi(e) : 0; }();
        static const int spec = [] { const char *e = getenv("RG_APPLY_SPEC"); return e ? atoi(e) : 1; }();
        static const int lazy_spec = [] { const char *e = getenv("RG_LAZY_SPEC"); return e ? atoi(e) : 0; }();
        static const int dense_v2 = [] { const char *e = getenv("RG_DENSE_PIPE"); return e ? atoi(e) : 0; }();
#else
        constexpr int prep_first = 1, xcd_map = 0;
#endif
        if (upd && !prep_first) return fail_arg("rg_ncf_tail: the MLP update workgroups need the prepare-first grid");
        const int64_t upd_blocks = upd ? ((int64_t)upd->P + 63) / 64 : 0;
        BackGrid bg{prep_blocks, 0, 0, prep_first, prep_first ? xcd_map : 0, upd_blocks};
        const int64_t head = prep_blocks + upd_blocks + (gen.nwords > 0 ? 1 : 0);
        int64_t total = nb + head;
        if (prep_first) {
            bg.apply_start = (head + 7) / 8 * 8;
            bg.apply_padded = (nb + 7) / 8 * 8;
            total = bg.apply_start + bg.apply_padded;
        }
        const dim3 grid((unsigned)total);
        const OwnerArgs oa = own ? *own : OwnerArgs{};
        const MlpUpdArgs ua = upd ? *upd : MlpUpdArgs{};
        LaunchEvents &le = launch_events();
        const hipEvent_t e0 = le.start, e1 = le.stop;
        le = LaunchEvents{};
        auto go = [&](auto kernel) {
            if (e0 || e1)
                hipExtLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, e0, e1, 0, *a, *prep, prep_out, nb, gen, bg, oa,
                                      ua);
            else
                hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, *a, *prep, prep_out, nb, gen, bg, oa, ua);
        };
        if constexpr (V) {
            if (own) go(mf_back_kernel<L, 0, true, true>);
            else go(mf_back_kernel<L, 0, true>);
            return check_launch("rg_mf_apply_prepare");
        } else {
        if (own) {
            go(mf_back_kernel<L, 0, true, true>);
            return check_launch("rg_mf_apply_prepare");
        }
#if RG_AB
        if constexpr (L::LPU >= kCap) {
            if (!lazy && dense_v2 && a->contrib == nullptr && upd == nullptr) {
                // a few workgroups per CU, each wave walking a chunk of row groups (mf_dense_kernel)
                static const int per_cu = [] { const char *e = getenv("RG_DENSE_PER_CU"); return e ? atoi(e) : 4; }();
                int64_t db = (int64_t)num_cus() * per_cu;
                const int64_t groups = (rows + L::UPW - 1) / L::UPW;
                const int64_t need = (groups + kBlock / kWave - 1) / (kBlock / kWave);
                if (db > need) db = need;
                if (db < 1) db = 1;
                BackGrid dg{prep_blocks, 0, 0, 1, 0};
                dg.apply_start = (head + 7) / 8 * 8;
                const dim3 dgrid((unsigned)(dg.apply_start + db));
                if (e0 || e1)
                    hipExtLaunchKernelGGL(mf_dense_kernel<L>, dgrid, dim3(kBlock), 0, s, e0, e1, 0, *a, *prep, prep_out, db,
                                          gen, dg);
                else
                    hipLaunchKernelGGL(mf_dense_kernel<L>, dgrid, dim3(kBlock), 0, s, *a, *prep, prep_out, db, gen, dg);
                return check_launch("rg_mf_apply_prepare");
            }
        }
        if (lazy && lazy_spec) go(mf_back_kernel<L, 0, true, false, true, true>);
        else if (lazy) go(mf_back_kernel<L, 0, true, false, true>);
        else if (spec && nt == 1) go(mf_back_kernel<L, 1, true>);
        else if (spec && nt == 3) go(mf_back_kernel<L, 3, true>);
        else if (spec) go(mf_back_kernel<L, 0, true>);
        else if (nt == 1) go(mf_back_kernel<L, 1>);
        else if (nt >= 2) go(mf_back_kernel<L, 2>);
        else go(mf_back_kernel<L, 0>);
#else
        if (lazy) return fail_arg("the lazy dense pass is an A/B build (build.py --variant lazy -DRG_AB=1)");
        go(mf_back_kernel<L, 0, true>);   // the list loaded beside the count
#endif
        return check_launch("rg_mf_apply_prepare");
        }
    }
};
}  // namespace

int rg::gen_args(const rg_mt_gen_t *gen, MtGenArgs &g, const char *what) {
    g = MtGenArgs{};
    if (gen && gen->nwords > 0) {
        if (!gen->state || !gen->out) return fail_arg(std::string(what) + ": null MT state / output");
        g.state = gen->state; g.out = gen->out; g.state_before = gen->state_before; g.nwords = gen->nwords;
    }
    return RG_OK;
}

extern "C" int rg_mf_apply_prepare(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const rg_opt_t *opt,
                                   int64_t row_begin, int64_t row_end, const rg_mf_loss_t *loss,
                                   const rg_mf_batch_t *next, const rg_mf_work_t *next_w) {
    return rg_mf_apply_prepare_gen(stream, t, w, opt, row_begin, row_end, loss, next, next_w, nullptr);
}

extern "C" int rg_mf_apply_prepare_gen(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const rg_opt_t *opt,
                                       int64_t row_begin, int64_t row_end, const rg_mf_loss_t *loss,
                                       const rg_mf_batch_t *next, const rg_mf_work_t *next_w,
                                       const rg_mt_gen_t *gen) {
    MtGenArgs g;
    int rc = gen_args(gen, g, "rg_mf_apply_prepare_gen");
    if (rc) return rc;
    ApplyArgs a;
    if ((rc = apply_args(t, w, nullptr, nullptr, opt, row_begin, row_end, loss, nullptr, kApplyPull, a))) return rc;
    PairsArgs prep{};
    int64_t prep_blocks = 0;
    int2 *prep_out = nullptr;
    if (next) {
        if ((rc = prepare_args(next, next_w, nullptr, prep))) return rc;
        prep_out = reinterpret_cast<int2 *>(next->pairs);
        prep_blocks = (prepare_threads(next->cols, next->n_neg) + kBlock - 1) / kBlock;
    }
    BackLaunchF f{&a, &prep, prep_out, prep_blocks, g, (hipStream_t)stream};
    return dispatch_dim(t->dim, f);
}

int rg::launch_back_lazy(void *stream, int32_t dim, ApplyArgs &a, const MtGenArgs &gen) {
    PairsArgs prep{};
    BackLaunchF f{&a, &prep, nullptr, 0, gen, (hipStream_t)stream};
    f.lazy = true;
    return dispatch_dim(dim, f);
}

namespace rg {
int apply_prepare_owner(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const rg_opt_t *opt,
                        int64_t row_begin, int64_t row_end, const rg_mf_loss_t *loss,
                        const rg_mf_owner_batch_t *next) {
    ApplyArgs a;
    int rc = apply_args(t, w, nullptr, nullptr, opt, row_begin, row_end, loss, nullptr, kApplyPull, a);
    if (rc) return rc;
    PairsArgs prep{};
    OwnerArgs oa{};
    int64_t prep_blocks = 0;
    if (next) {
        if ((rc = owner_args(next, oa))) return rc;
        prep_blocks = oa.segs;
    }
    BackLaunchF f{&a, &prep, nullptr, prep_blocks, MtGenArgs{}, (hipStream_t)stream, next ? &oa : nullptr};
    return dispatch_dim(t->dim, f);
}
}  // namespace rg

static int ncf_apply_args(const rg_ncf_model_t *m, rg_mf_work_t *w, const float *contrib, const rg_opt_t *opt,
                          int64_t row_begin, int64_t row_end, ApplyArgs &a) {
    if (!m || !w || !opt || !contrib || !m->user_w || !m->item_w) return fail_arg("rg_ncf_apply: null argument");
    if (!w->row_count || !w->row_list || !w->hot_grad) return fail_arg("rg_ncf_apply: null scratch");
    if (opt->kind == RG_OPT_ADAM && (!m->user_w_m || !m->item_w_m)) return fail_arg("rg_ncf_apply: Adam needs m");
    if (opt->kind != RG_OPT_SGD && (!m->user_w_v || !m->item_w_v)) return fail_arg("rg_ncf_apply: needs v");
    if (w->plan_perm && !w->part_row) return fail_arg("rg_ncf_apply: plan needs part_row");
    const int64_t nrows = m->num_users + m->num_items;
    if (row_begin < 0) row_begin = 0;
    if (row_end < 0 || row_end > nrows) row_end = nrows;
    if (row_begin > row_end) return fail_arg("rg_ncf_apply: row_begin > row_end");
    a = ApplyArgs{};
    a.w_in[0] = m->user_w; a.w_in[1] = m->item_w;
    a.w_out[0] = m->user_w; a.w_out[1] = m->item_w;          // in place: no partner rows are read
    a.w_m[0] = m->user_w_m; a.w_m[1] = m->item_w_m; a.w_v[0] = m->user_w_v; a.w_v[1] = m->item_w_v;
    a.num_users = m->num_users; a.num_items = m->num_items; a.dim = m->dim;
    a.row_begin = row_begin; a.row_end = row_end;
    a.row_count = w->row_count; a.row_list = reinterpret_cast<const int2 *>(w->row_list);
    a.hot_grad = reinterpret_cast<long long *>(w->hot_grad);
    if (w->plan_perm) { a.item_slot_off = w->plan_item_slot_off; a.part_row = w->part_row; }
    a.opt = *opt;
    a.contrib = contrib;
    a.contrib_stride = 2 * (int64_t)m->dim;
    a.has_bias = false;
    return RG_OK;
}

// Data-parallel NCF / NeuMF step (replicated, reference-exact): the embedding rows' data
// gradient pulled from the lists into the flat buffer (before the exchange), and the
// in-place update of every row from the summed buffer (after it).  gmf: the NeuMF GMF tables
// (their rows from ncf_work->mf_contrib; the lists are kept for the MLP tables' pass).
static int ncf_table_args(const rg_ncf_model_t *m, rg_mf_work_t *w, const rg_ncf_work_t *nw, int gmf,
                          int64_t row_begin, int64_t row_end, ApplyArgs &a) {
    if (!m) return fail_arg("rg_ncf_grads: null model");
    if (gmf && (m->mf_dim < 1 || !m->mf_user_w || !m->mf_item_w)) return fail_arg("rg_ncf_grads: no GMF tables");
    const int64_t nrows = m->num_users + m->num_items;
    if (row_begin < 0) row_begin = 0;
    if (row_end < 0 || row_end > nrows) row_end = nrows;
    if (row_begin > row_end) return fail_arg("rg_ncf_grads: row_begin > row_end");
    a = ApplyArgs{};
    a.w_in[0] = gmf ? m->mf_user_w : m->user_w;
    a.w_in[1] = gmf ? m->mf_item_w : m->item_w;
    a.w_out[0] = const_cast<float *>(a.w_in[0]);
    a.w_out[1] = const_cast<float *>(a.w_in[1]);
    a.w_m[0] = gmf ? m->mf_user_m : m->user_w_m; a.w_m[1] = gmf ? m->mf_item_m : m->item_w_m;
    a.w_v[0] = gmf ? m->mf_user_v : m->user_w_v; a.w_v[1] = gmf ? m->mf_item_v : m->item_w_v;
    a.num_users = m->num_users; a.num_items = m->num_items; a.dim = gmf ? m->mf_dim : m->dim;
    a.row_begin = row_begin; a.row_end = row_end;
    if (w) {
        if (!w->row_count || !w->row_list || !nw) return fail_arg("rg_ncf_grads: null scratch");
        a.row_count = w->row_count; a.row_list = reinterpret_cast<const int2 *>(w->row_list);
        a.hot_grad = reinterpret_cast<long long *>(gmf ? nw->mf_hot_grad : w->hot_grad);
        a.contrib = gmf ? nw->mf_contrib : nw->contrib;
        a.contrib_stride = 2 * (int64_t)a.dim;
        a.keep_count = gmf != 0;
        if (w->plan_perm) {
            a.item_slot_off = w->plan_item_slot_off;
            a.part_row = gmf ? nw->mf_part_row : w->part_row;
        }
        if (!a.hot_grad || !a.contrib) return fail_arg("rg_ncf_grads: null contribution rows / overflow rows");
    }
    a.has_bias = false;
    return RG_OK;
}

// NeuMF (spotlight/dnn_models/neuMF.py:7-55): the GMF tables take their gradient rows
// from ncf_work->mf_contrib through the same per-row lists (kept), then the MLP tables
// pull theirs and reset the lists (rg_ncf_apply).
// NeuMF's GMF tables: pull + optimizer through the same per-row lists, keeping the counts for
// the MLP tables' pass that follows (rg_ncf_apply or rg_ncf_tail resets them)
static int neumf_gmf_pass(void *stream, const rg_ncf_model_t *m, rg_mf_work_t *w, const rg_ncf_work_t *nw,
                          const rg_opt_t *opt, int64_t row_begin, int64_t row_end, const MtGenArgs &gen) {
    if (!m || !w || !nw || !opt) return fail_arg("rg_neumf_apply: null argument");
    if (m->mf_dim < 1 || m->mf_dim > RG_NEUMF_MAX_MF_DIM) return fail_arg("rg_neumf_apply: mf_dim out of range");
    if (!m->mf_user_w || !m->mf_item_w || !nw->mf_contrib || !nw->mf_hot_grad)
        return fail_arg("rg_neumf_apply: null GMF table / scratch");
    if (w->plan_perm && !nw->mf_part_row) return fail_arg("rg_neumf_apply: plan needs mf_part_row");
    if (opt->kind == RG_OPT_ADAM && (!m->mf_user_m || !m->mf_item_m)) return fail_arg("rg_neumf_apply: Adam needs m");
    if (opt->kind != RG_OPT_SGD && (!m->mf_user_v || !m->mf_item_v)) return fail_arg("rg_neumf_apply: needs v");
    if (!w->row_count || !w->row_list) return fail_arg("rg_neumf_apply: null scratch");
    const int64_t nrows = m->num_users + m->num_items;
    int64_t rb = row_begin < 0 ? 0 : row_begin, re = row_end < 0 || row_end > nrows ? nrows : row_end;
    if (rb > re) return fail_arg("rg_neumf_apply: row_begin > row_end");
    ApplyArgs a{};
    a.w_in[0] = m->mf_user_w; a.w_in[1] = m->mf_item_w;
    a.w_out[0] = m->mf_user_w; a.w_out[1] = m->mf_item_w;
    a.w_m[0] = m->mf_user_m; a.w_m[1] = m->mf_item_m; a.w_v[0] = m->mf_user_v; a.w_v[1] = m->mf_item_v;
    a.num_users = m->num_users; a.num_items = m->num_items; a.dim = m->mf_dim;
    a.row_begin = rb; a.row_end = re;
    a.row_count = w->row_count; a.row_list = reinterpret_cast<const int2 *>(w->row_list);
    a.hot_grad = reinterpret_cast<long long *>(nw->mf_hot_grad);
    if (w->plan_perm) { a.item_slot_off = w->plan_item_slot_off; a.part_row = nw->mf_part_row; }
    a.opt = *opt;
    a.contrib = nw->mf_contrib;
    a.contrib_stride = 2 * (int64_t)m->mf_dim;
    a.has_bias = false;
    a.keep_count = true;
    if (gen.nwords > 0) {   // with an MT walk: mf_back_kernel's grid (walk block + the same pull)
        PairsArgs prep{};
        BackLaunchF f{&a, &prep, nullptr, 0, gen, (hipStream_t)stream};
        return dispatch_dim(m->mf_dim, f);
    }
    ApplyLaunchF f{&a, (hipStream_t)stream, kApplyPull};
    return dispatch_dim(m->mf_dim, f);
}

extern "C" int rg_ncf_apply(void *stream, const rg_ncf_model_t *m, rg_mf_work_t *w, const float *contrib,
                            const rg_opt_t *opt, int64_t row_begin, int64_t row_end) {
    ApplyArgs a{};
    const int rc = ncf_apply_args(m, w, contrib, opt, row_begin, row_end, a);
    if (rc) return rc;
    ApplyLaunchF f{&a, (hipStream_t)stream, kApplyPull};
    return dispatch_dim(m->dim, f);
}

// The tail of a single-GPU NCF step in one launch (mf_back_kernel's grid): the next step's
// prepare (next = NULL: none), the MLP update from the pair kernel's weight-gradient partials
// (rg_ncf_update's reduction and optimizer, the same sums) with the step's loss, and the
// embedding rows' update (rg_ncf_apply) -- three launches and their tails in one; the three
// parts touch disjoint data.  NeuMF (mf_dim > 0): the GMF tables' pass runs first, in a launch
// of its own (it keeps the per-row counts the MLP tables' pass then consumes), as rg_neumf_apply.
// gen (optional, rg_mf_stepper_tail_gen): workgroup 0 walks a later step's MT words, as in the
// MF split step's dense pass -- no generator-stream kernel beside the pair kernel.
// every check of rg_ncf_tail that does not depend on the stepper's outputs (next batch, MT walk):
// the engine runs it BEFORE the stepper bookkeeping calls (rg_mf_stepper_prefetch_args /
// rg_mf_stepper_tail_gen commit the next unit and the ring slot), so a refused tail never
// leaves the stepper believing a prepare or a walk was launched
static int ncf_tail_checks(const rg_ncf_model_t *m, rg_mf_work_t *w, const rg_ncf_work_t *nw, int64_t nparts,
                           const rg_opt_t *opt, const float *loss_partials, const rg_mf_loss_t *loss, ApplyArgs &a,
                           int64_t &P) {
    if (!m || !w || !nw || !opt || !nw->contrib || !nw->mlp_partials || !m->mlp)
        return fail_arg("rg_ncf_tail: null argument");
    if (opt->kind == RG_OPT_ADAM && !m->mlp_m) return fail_arg("rg_ncf_tail: Adam needs m state");
    if (opt->kind != RG_OPT_SGD && !m->mlp_v) return fail_arg("rg_ncf_tail: optimizer needs v state");
    P = m->mf_dim == 0 ? rg_ncf_mlp_len(m->dim) : rg_neumf_param_len(m->dim, m->mf_dim);
    if (P < 0 || nparts < 1) return fail_arg("rg_ncf_tail: bad dim / mf_dim / partial count");
    if (loss && loss->out && !loss_partials) return fail_arg("rg_ncf_tail: loss needs partials");
    if (m->dim < 1 || m->dim > 256) return fail_arg("rg_ncf_tail: dim must be in [1, 256]");
    return ncf_apply_args(m, w, nw->contrib, opt, 0, -1, a);
}

extern "C" int rg_ncf_tail_validate(const rg_ncf_model_t *m, rg_mf_work_t *w, const rg_ncf_work_t *nw,
                                    int64_t nparts, const rg_opt_t *opt, const float *loss_partials,
                                    const rg_mf_loss_t *loss) {
    ApplyArgs a{};
    int64_t P = 0;
    return ncf_tail_checks(m, w, nw, nparts, opt, loss_partials, loss, a, P);
}

extern "C" int rg_ncf_tail(void *stream, const rg_ncf_model_t *m, rg_mf_work_t *w, const rg_ncf_work_t *nw,
                           int64_t nparts, const rg_opt_t *opt, const float *loss_partials, const rg_mf_loss_t *loss,
                           const rg_mf_batch_t *next, const rg_mf_work_t *next_w, const rg_mt_gen_t *gen) {
    ApplyArgs a{};
    int64_t P = 0;
    int rc = ncf_tail_checks(m, w, nw, nparts, opt, loss_partials, loss, a, P);
    if (rc) return rc;
    MtGenArgs g{};
    if (gen && gen->nwords > 0) {
        if (!gen->state || !gen->out) return fail_arg("rg_ncf_tail: null MT state / output");
        g.state = gen->state; g.out = gen->out; g.state_before = gen->state_before; g.nwords = gen->nwords;
    }
    // NeuMF: the GMF tables' pass first; the walk (if any) rides in that launch -- the longer of
    // the two passes at the reference's sizes (mf 50 vs mlp 16 floats per row)
    if (m->mf_dim != 0) {
        if ((rc = neumf_gmf_pass(stream, m, w, nw, opt, 0, -1, g))) return rc;
        g = MtGenArgs{};
    }
    if (loss && loss->out) {   // finalized by the dense blocks' first workgroup (rg_ncf_update's sums)
        a.partials = loss_partials;
        a.n_partials = loss->n_partials;
        a.inv_a = loss->inv_a;
        a.inv_b = loss->inv_b;
        a.loss_out = loss->out;
    }
    MlpUpdArgs u{};
    u.mlp = m->mlp;
    u.m = opt->kind == RG_OPT_ADAM ? m->mlp_m : nullptr;
    u.v = opt->kind == RG_OPT_SGD ? nullptr : m->mlp_v;
    u.wpart = nw->mlp_partials;
    u.nparts = (int)nparts;
    u.P = (int)P;
    u.opt = *opt;
    u.mode = 0;
    PairsArgs prep{};
    int2 *prep_out = nullptr;
    int64_t prep_blocks = 0;
    if (next) {
        if ((rc = prepare_args(next, next_w, nullptr, prep))) return rc;
        if (next->pairs == nullptr) return fail_arg("rg_ncf_tail: null next pairs");
        prep_out = reinterpret_cast<int2 *>(next->pairs);
        prep_blocks = (prepare_threads(next->cols, next->n_neg) + kBlock - 1) / kBlock;
    }
    BackLaunchF f{&a, &prep, prep_out, prep_blocks, g, (hipStream_t)stream};
    f.upd = &u;
    return dispatch_dim(m->dim, f);
}

extern "C" int rg_ncf_grads(void *stream, const rg_ncf_model_t *m, rg_mf_work_t *w, const rg_ncf_work_t *nw,
                            float *grad, int64_t row_begin, int64_t row_end, int32_t gmf) {
    if (!w || !nw || !grad) return fail_arg("rg_ncf_grads: null argument");
    ApplyArgs a;
    int rc = ncf_table_args(m, w, nw, gmf, row_begin, row_end, a);
    if (rc) return rc;
    a.grad = grad;
    ApplyLaunchF f{&a, (hipStream_t)stream, kGradOnly};
    return dispatch_dim(a.dim, f);
}

extern "C" int rg_ncf_apply_dense(void *stream, const rg_ncf_model_t *m, const float *grad, const rg_opt_t *opt,
                                  int64_t row_begin, int64_t row_end, int32_t gmf) {
    if (!grad || !opt) return fail_arg("rg_ncf_apply_dense: null argument");
    ApplyArgs a;
    int rc = ncf_table_args(m, nullptr, nullptr, gmf, row_begin, row_end, a);
    if (rc) return rc;
    if (opt->kind == RG_OPT_ADAM && (!a.w_m[0] || !a.w_m[1])) return fail_arg("rg_ncf_apply_dense: Adam needs m");
    if (opt->kind != RG_OPT_SGD && (!a.w_v[0] || !a.w_v[1])) return fail_arg("rg_ncf_apply_dense: needs v");
    a.opt = *opt;
    a.grad = const_cast<float *>(grad);
    ApplyLaunchF f{&a, (hipStream_t)stream, kApplyDense};
    return dispatch_dim(a.dim, f);
}

extern "C" int rg_neumf_apply(void *stream, const rg_ncf_model_t *m, rg_mf_work_t *w, const rg_ncf_work_t *nw,
                              const rg_opt_t *opt, int64_t row_begin, int64_t row_end) {
    const int rc = neumf_gmf_pass(stream, m, w, nw, opt, row_begin, row_end, MtGenArgs{});
    if (rc) return rc;
    return rg_ncf_apply(stream, m, w, nw->contrib, opt, row_begin, row_end);
}

extern "C" int rg_mf_apply(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const rg_opt_t *opt,
                           int64_t row_begin, int64_t row_end, const rg_mf_loss_t *loss) {
    return apply_common(stream, t, w, nullptr, nullptr, opt, row_begin, row_end, loss, nullptr, kApplyPull);
}

extern "C" int rg_mf_grads(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, float *grad_dev,
                           int64_t row_begin, int64_t row_end, const rg_mf_loss_t *loss) {
    if (!grad_dev) return fail_arg("rg_mf_grads: null grad");
    return apply_common(stream, t, w, nullptr, grad_dev, nullptr, row_begin, row_end, loss, nullptr, kGradOnly);
}

extern "C" int rg_mf_apply_dense(void *stream, const rg_mf_tables_t *t, const float *grad_dev, const rg_opt_t *opt,
                                 int64_t row_begin, int64_t row_end, float *loss_out_dev) {
    if (!grad_dev) return fail_arg("rg_mf_apply_dense: null grad");
    return apply_common(stream, t, nullptr, grad_dev, nullptr, opt, row_begin, row_end, nullptr, loss_out_dev,
                        kApplyDense);
}

extern "C" int64_t rg_mf_grad_chunk(int64_t shard_users, int64_t shard_items, int32_t dim) {
    if (shard_users < 1 || shard_items < 1 || dim < 1) return -1;
    return ((shard_users + shard_items) * (int64_t)(dim + 1) + 1 + 3) / 4 * 4;
}

static int shard_args(const rg_mf_tables_t *t, int64_t su, int64_t si, int32_t world, int32_t rank, ApplyArgs &a) {
    if (world < 1 || rank < 0 || rank >= world) return fail_arg("rg_mf sharded: bad rank / world");
    if (su < 1 || si < 1 || su * world < t->num_users || si * world < t->num_items)
        return fail_arg("rg_mf sharded: shards do not cover the tables");
    a.shard_users = su;
    a.shard_items = si;
    a.chunk = rg_mf_grad_chunk(su, si, t->dim);
    a.world = world;
    a.rank = rank;
    return RG_OK;
}

extern "C" int rg_mf_grads_sharded(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, float *grad_dev,
                                   int64_t shard_users, int64_t shard_items, int32_t world, const rg_mf_loss_t *loss) {
    if (!grad_dev) return fail_arg("rg_mf_grads_sharded: null grad");
    ApplyArgs a;
    int rc = apply_args(t, w, nullptr, grad_dev, nullptr, 0, -1, loss, nullptr, kGradOnly, a);
    if (rc || (rc = shard_args(t, shard_users, shard_items, world, 0, a))) return rc;
    ApplyLaunchF f{&a, (hipStream_t)stream, kGradOnly};
    return dispatch_dim(t->dim, f);
}

extern "C" int rg_mf_apply_shard(void *stream, const rg_mf_tables_t *t, const float *grad_dev, const rg_opt_t *opt,
                                 int64_t shard_users, int64_t shard_items, int32_t world, int32_t rank,
                                 float *loss_out_dev) {
    if (!grad_dev) return fail_arg("rg_mf_apply_shard: null grad");
    ApplyArgs a;
    int rc = apply_args(t, nullptr, grad_dev, nullptr, opt, 0, -1, nullptr, loss_out_dev, kApplyDense, a);
    if (rc || (rc = shard_args(t, shard_users, shard_items, world, rank, a))) return rc;
    const int64_t u0 = rank * shard_users, i0 = rank * shard_items;
    const int64_t nu = u0 < t->num_users ? std::min(shard_users, t->num_users - u0) : 0;
    const int64_t ni = i0 < t->num_items ? std::min(shard_items, t->num_items - i0) : 0;
    a.row_begin = 0;
    a.row_end = nu + ni;            // rows of the shard, mapped in mf_apply_kernel
    ApplyLaunchF f{&a, (hipStream_t)stream, kApplyDense};
    return dispatch_dim(t->dim, f);
}

extern "C" int64_t rg_mf_item_grad_chunk(int64_t shard_items, int32_t dim) {
    if (shard_items < 1 || dim < 1) return -1;
    return (shard_items * (int64_t)(dim + 1) + 1 + 3) / 4 * 4;
}

static int item_shard_args(const rg_mf_tables_t *t, int64_t si, int32_t world, int32_t rank, ApplyArgs &a) {
    if (world < 1 || rank < 0 || rank >= world) return fail_arg("rg_mf item shard: bad rank / world");
    if (si < 1 || si * world < t->num_items) return fail_arg("rg_mf item shard: shards do not cover the items");
    a.shard_users = 0;
    a.shard_items = si;
    a.item_shard = 1;
    a.chunk = rg_mf_item_grad_chunk(si, t->dim);
    a.world = world;
    a.rank = rank;
    return RG_OK;
}

extern "C" int rg_mf_grads_item_shard(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, float *grad_dev,
                                      int64_t shard_items, int32_t world, const rg_mf_loss_t *loss) {
    if (!grad_dev) return fail_arg("rg_mf_grads_item_shard: null grad");
    ApplyArgs a;
    int rc = apply_args(t, w, nullptr, grad_dev, nullptr, t->num_users, t->num_users + t->num_items, loss, nullptr,
                        kGradOnly, a);
    if (rc || (rc = item_shard_args(t, shard_items, world, 0, a))) return rc;
    ApplyLaunchF f{&a, (hipStream_t)stream, kGradOnly};
    return dispatch_dim(t->dim, f);
}

extern "C" int rg_mf_apply_item_shard(void *stream, const rg_mf_tables_t *t, const float *grad_dev,
                                      const rg_opt_t *opt, int64_t shard_items, int32_t world, int32_t rank,
                                      float *loss_out_dev) {
    if (!grad_dev) return fail_arg("rg_mf_apply_item_shard: null grad");
    ApplyArgs a;
    int rc = apply_args(t, nullptr, grad_dev, nullptr, opt, 0, -1, nullptr, loss_out_dev, kApplyDense, a);
    if (rc || (rc = item_shard_args(t, shard_items, world, rank, a))) return rc;
    const int64_t i0 = rank * shard_items;
    a.row_begin = 0;
    a.row_end = i0 < t->num_items ? std::min(shard_items, t->num_items - i0) : 0;   // mapped in mf_apply_kernel
    ApplyLaunchF f{&a, (hipStream_t)stream, kApplyDense};
    return dispatch_dim(t->dim, f);
}

extern "C" int rg_loss_finalize(void *stream, const float *partials, int64_t n_partials, double inv_a,
                                double inv_b, float *out) {
    if (!partials || !out || n_partials < 0) return fail_arg("rg_loss_finalize: bad args");
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, partials, n_partials,
                       inv_a, inv_b, out);
    return check_launch("rg_loss_finalize");
}

extern "C" int rg_mf_scores(void *stream, const float *uw, const float *iw, const float *ub, const float *ib,
                            int32_t dim, const int64_t *users, const int64_t *items, int64_t n, float *out) {
    if (!uw || !iw || !ub || !ib || !users || !items || !out) return fail_arg("rg_mf_scores: null pointer");
    if (n < 0) return fail_arg("rg_mf_scores: n < 0");
    if (n == 0) return RG_OK;
    ScoresLaunchF f{uw, iw, ub, ib, dim, users, items, n, out, (hipStream_t)stream};
    return dispatch_dim(dim, f);
}

#ifdef RG_DIAG_STAMPS
extern "C" int rg_diag_set_stamps(unsigned long long *dev_buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(rg::g_diag_stamps), &dev_buf, sizeof(dev_buf)) == hipSuccess ? RG_OK
                                                                                                  : RG_E_LAUNCH;
}
extern "C" int rg_diag_set_flags(int flags) {
    return hipMemcpyToSymbol(HIP_SYMBOL(rg::g_diag_flags), &flags, sizeof(flags)) == hipSuccess ? RG_OK : RG_E_LAUNCH;
}
#endif
