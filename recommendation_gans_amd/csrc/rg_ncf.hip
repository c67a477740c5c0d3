// NCF MLP training step on gfx950 (spotlight/dnn_models/mlp.py:5-46 trained by
// implicit.py:347-364; layers [2E, E, ..., 8] -> 1 as ncf_spotlight.py:53-56).
//
// This file: the MLP update kernel, the adaptive-hinge kernels and the C ABI.  rg_ncf_pairs
// launches one of two kernels (ncf_use_wave): ncf_wave_kernel (rg_ncf_wave.hip, the E = 64 MLP: one
// wave per tile of ncfw::kR = 48, described there) or ncf_pairs_kernel (rg_ncf_tile.hip, the rest:
// one workgroup of 4 waves, 8 at E = 64, walks tiles of kRows = 32 examples), described here.
// A tile holds whole
// columns (a positive and its n negatives, pairs prepared by rg_mf_prepare), so
// pairwise losses are resolved inside the tile.  Everything of a tile lives in
// LDS: the MLP parameters (loaded once per workgroup), the activations of every
// layer, the per-unit backward multipliers and the workgroup's running weight
// gradient.  Each layer's three products run on the fp32 MFMA (16x16x4):
//     Z_k = A_k W_k^T,   dW_k += delta_k^T A_k,   dA_k = delta_k W_k.
// LeakyReLU(0.1) then Dropout(0.5) fold into one exact multiplier per unit,
// m in {0, 2, 0.2} (training) or {1, 0.1} (eval): A_{k+1} = Z_k * m and
// delta = dA * m reproduce torch's rounding (power-of-two scalings commute).
// Outputs: per-example input gradients dX (rows of 2E) for the embedding update
// (rg_ncf_apply pulls them through the per-row lists), planned per-tile partial
// rows for the positives' items, the workgroup's weight-gradient partial and
// deterministic loss partials.
//
// NeuMF (spotlight/dnn_models/neuMF.py:7-55) is the same tower plus a GMF branch:
// the output Linear sees cat(A_NH, U_mf[u] * I_mf[i]) (mf_dim M > 0).  The GMF rows
// are gathered beside A_0, the output layer adds M products, and the GMF backward
// (dU_mf = dz w_m I_mf, dI_mf = dz w_m U_mf) runs before the tower's backward and
// writes its own per-example rows (mf_contrib), overflow rows and planned partials.
#include <cstdlib>

#include "rg_ncf.h"
#include "rg_mlp_update.h"

namespace rg {

// reduce the weight-gradient partials + optimizer update of the MLP parameters in
// place: a block owns 64 parameters, its kUpdWaves waves sum fixed slices of the
// partials (coalesced 256-B loads, four independent chains so the loads pipeline)
// and combine in LDS in a fixed order (deterministic); block 0 also finalises the loss
constexpr int kUpdWaves = 16;
// mode 0: reduce + update; 1 (data parallel, before the exchange): reduce into grad[0, P)
// and this rank's loss share into grad[P]; 2 (after it): update from grad, loss = grad[P]
__global__ __launch_bounds__(kUpdWaves * 64) void ncf_update_kernel(float *mlp, float *m, float *v, const float *wpart,
                                                        int nparts, int P, rg_opt_t opt, const float *loss_partials,
                                                        int64_t n_partials, double inv_a, double inv_b,
                                                        float *loss_out, int mode, float *grad) {
    __shared__ float red[kMlpSlices][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (mode == 2) {
        const int e = blockIdx.x * 64 + lane;
        if (loss_out && blockIdx.x == 0 && threadIdx.x == 0) *loss_out = grad[P];
        if (wave != 0 || e >= P) return;
        float mm = m ? m[e] : 0.0f, vv = v ? v[e] : 0.0f;
        mlp[e] = opt_update(opt, mlp[e], grad[e], mm, vv);
        if (m) m[e] = mm;
        if (v) v[e] = vv;
        return;
    }
    if ((loss_out || mode == 1) && loss_partials && blockIdx.x == 0 && wave == 0) {
        double sa = 0.0, sb = 0.0;
        int64_t i = lane;
        // batches of 8 strided pairs: the loads of a batch in flight before the same in-order sums
        for (; i + 7 * 64 < n_partials; i += 8 * 64) {
            float2 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = reinterpret_cast<const float2 *>(loss_partials)[i + q * 64];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                sa += (double)v[q].x;
                sb += (double)v[q].y;
            }
        }
        for (; i < n_partials; i += 64) {
            sa += (double)loss_partials[2 * i];
            sb += (double)loss_partials[2 * i + 1];
        }
        for (int off = 32; off > 0; off >>= 1) {
            sa += __shfl_xor(sa, off);
            sb += __shfl_xor(sb, off);
        }
        if (lane == 0) {
            const float lv = (float)(sa * inv_a + sb * inv_b);
            if (loss_out) *loss_out = lv;
            if (mode == 1) grad[P] = lv;
        }
    }
    static_assert(kUpdWaves == kMlpSlices, "one slice per wave");
    const MlpUpdArgs u{mlp, m, v, wpart, nparts, P, opt, mode, grad};
    mlp_update_block<kUpdWaves>(u, blockIdx.x, red);
}

// adaptive hinge from forward-only scores: dp of every row (positives: hinge
// against the max negative; the argmax negative: minus the sum over active positives)
__global__ __launch_bounds__(256) void ncf_adapt_dp_kernel(const float *scores, float *dp, int64_t rows, int TR, int tc,
                                                          int NP, int64_t n_pos_cols, int64_t cols, float n_a,
                                                          float *loss_partial) {
    __shared__ float smax[256];
    __shared__ int64_t sidx[256];
    __shared__ float scnt[256], sloss[256];
    const int tid = threadIdx.x;
    float best = -1.0f;
    int64_t bi = -1;
    for (int64_t r = tid; r < rows; r += 256) {
        const int64_t tile = r / TR, rr = r % TR;
        const int q = (int)(rr / tc);
        const int64_t s = tile * tc + rr % tc;
        dp[r] = 0.0f;
        if (q >= 1 && q < NP && s < cols && scores[r] > best) { best = scores[r]; bi = r; }
    }
    smax[tid] = best;
    sidx[tid] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {     // max, first occurrence in draw order on ties
        if (tid < w) {
            const bool take = smax[tid + w] > smax[tid];
            if (take) { smax[tid] = smax[tid + w]; sidx[tid] = sidx[tid + w]; }
        }
        __syncthreads();
    }
    const float mx = smax[0];
    float cnt = 0.0f, ls = 0.0f;
    for (int64_t r = tid; r < rows; r += 256) {
        const int64_t tile = r / TR, rr = r % TR;
        const int64_t s = tile * tc + rr % tc;
        if (rr / tc == 0 && rr < (int64_t)tc && s < n_pos_cols) {
            const float x = (mx - scores[r]) + 1.0f;
            ls += fmaxf(x, 0.0f);
            if (x >= 0.0f) { dp[r] = -(1.0f / n_a); cnt += 1.0f; }
        }
    }
    scnt[tid] = cnt;
    sloss[tid] = ls;
    __syncthreads();
    if (tid == 0) {
        float c = 0.0f, l = 0.0f;
        for (int i = 0; i < 256; ++i) { c += scnt[i]; l += sloss[i]; }
        if (sidx[0] >= 0) dp[sidx[0]] = c * (1.0f / n_a);
        loss_partial[0] = l;
        loss_partial[1] = 0.0f;
    }
}

static bool ncf_use_wave(int E, int M) {
#if RG_AB
    // the tile kernel for E = 64 (measured slower), A/B build only
    static const bool off = [] {
        const char *s = getenv("RG_NCF_TILE");
        return s && s[0] == '1';
    }();
#else
    constexpr bool off = false;
#endif
    return E == 64 && M == 0 && !off;
}

// -1 (dispatch_ncf_dim's) for an embedding_dim without a tower
int ncf_mlp_len(int E) { return dispatch_ncf_dim(E, [](auto e) { return NcfTower<decltype(e)::value>::P; }); }
int ncf_mask_units(int E) {
    return dispatch_ncf_dim(E, [](auto e) { return NcfTower<decltype(e)::value>::mask_units(); });
}

}  // namespace rg

using namespace rg;

extern "C" int64_t rg_ncf_mlp_len(int32_t dim) { return ncf_mlp_len(dim); }
extern "C" int64_t rg_neumf_param_len(int32_t dim, int32_t mf_dim) {
    const int p = ncf_mlp_len(dim);
    return p < 0 || mf_dim < 1 || mf_dim > RG_NEUMF_MAX_MF_DIM ? -1 : p + mf_dim;
}
static int64_t ncf_param_len(const rg_ncf_model_t *m) {
    return m->mf_dim == 0 ? ncf_mlp_len(m->dim) : rg_neumf_param_len(m->dim, m->mf_dim);
}
extern "C" int64_t rg_ncf_mask_units(int32_t dim) { return ncf_mask_units(dim); }
// rows per tile: 48 (ncfw::kR) for the wave kernel (E = 64 MLP: 8 columns of 1 + 5 rows, one
// tile per wave at B = 8192), 32 for the tile kernel (the other towers, NeuMF)
extern "C" int64_t rg_ncf_rows_per_tile(int32_t dim, int32_t mf_dim) {
    if (ncf_mlp_len(dim) < 0 || mf_dim < 0 || mf_dim > RG_NEUMF_MAX_MF_DIM) return -1;
    return ncf_use_wave(dim, mf_dim) ? ncfw::kR : kRows;
}
extern "C" int64_t rg_ncf_cols_per_tile(int32_t n_neg, int32_t dim, int32_t mf_dim) {
    const int64_t R = rg_ncf_rows_per_tile(dim, mf_dim);
    return R < 0 || n_neg < 0 || n_neg >= R ? -1 : R / (n_neg + 1);
}
extern "C" int64_t rg_ncf_tiles(int64_t cols, int32_t n_neg, int32_t dim, int32_t mf_dim) {
    const int64_t tc = rg_ncf_cols_per_tile(n_neg, dim, mf_dim);
    return tc <= 0 ? -1 : (cols + tc - 1) / tc;
}
// the scores / dp layout of an adaptive-hinge launch: the work's tile_rows (the model's
// rg_ncf_rows_per_tile, checked by rg_ncf_pairs)
static int ncf_geometry(const rg_ncf_work_t *nw, const rg_mf_batch_t *b, int &TR, int &tc, int64_t &tiles) {
    TR = nw->tile_rows;
    if (TR != kRows && TR != ncfw::kR) return fail_arg("rg_ncf: ncf_work.tile_rows must be rg_ncf_rows_per_tile(dim, mf_dim)");
    if (b->n_neg < 1 || b->n_neg >= TR) return fail_arg("rg_ncf: n_neg out of range");
    tc = TR / (b->n_neg + 1);
    tiles = (b->cols + tc - 1) / tc;
    return RG_OK;
}
// workgroups resident per CU by LDS (at most 4): the E = 64 MLP takes a CU's LDS alone,
// the small towers (and NeuMF's) leave room for several tiles in flight per CU, which is
// what hides their gather / barrier latency
extern "C" int64_t rg_ncf_blocks(int64_t cols, int32_t n_neg, int32_t dim, int32_t mf_dim) {
    const int64_t t = rg_ncf_tiles(cols, n_neg, dim, mf_dim);
    const int lds = ncf_tile_lds_floats(dim, mf_dim);
    if (t <= 0 || lds <= 0 || lds > kLdsMax || mf_dim < 0 || mf_dim > RG_NEUMF_MAX_MF_DIM) return -1;
    if (ncf_use_wave(dim, mf_dim)) {   // one wave per tile, 4 waves per workgroup, one workgroup per CU
        const int64_t w = (t + ncfw::kWaves - 1) / ncfw::kWaves;
        return w < 256 ? w : 256;
    }
    int per_cu = kLdsMax / lds;
    if (per_cu > 4) per_cu = 4;
    const int64_t cap = 256 * (int64_t)per_cu;
    return t < cap ? t : cap;
}

extern "C" int rg_ncf_pairs(void *stream, const rg_ncf_model_t *m, const rg_mf_batch_t *b, rg_mf_work_t *w,
                            rg_ncf_work_t *nw, int32_t phase) {
    if (!m || !b || !w || !nw) return fail_arg("rg_ncf_pairs: null argument");
    if (ncf_mlp_len(m->dim) < 0) return fail_arg("rg_ncf_pairs: embedding_dim must be 8, 16, 32 or 64");
    if (b->n_neg < 1 || b->n_neg > RG_MF_MAX_NEG) return fail_arg("rg_ncf_pairs: n_neg out of range");
    if (b->loss < RG_LOSS_POINTWISE || b->loss > RG_LOSS_ADAPTIVE_HINGE)   // no positives-only NCF step
        return fail_arg("rg_ncf_pairs: loss must be pointwise, bpr, hinge or adaptive hinge");
    if (!b->pairs || !m->user_w || !m->item_w || !m->mlp) return fail_arg("rg_ncf_pairs: null tables / pairs");
    if (b->n_pos > b->cols) return fail_arg("rg_ncf_pairs: n_pos > cols");
    if (phase != kNcfScores && phase != kNcfLossOnly && (!w->row_count || !w->row_list || !w->hot_grad ||
                                                         !w->loss_partials || !nw->contrib || !nw->mlp_partials))
        return fail_arg("rg_ncf_pairs: null scratch");
    if (phase == kNcfLossOnly && !w->loss_partials) return fail_arg("rg_ncf_pairs: loss needs partials");
    if (phase == kNcfScores && !nw->scores) return fail_arg("rg_ncf_pairs: scores buffer needed");
    if (phase == kNcfGivenDp && !nw->dp) return fail_arg("rg_ncf_pairs: dp buffer needed");
    if ((phase == kNcfFused || phase == kNcfLossOnly) && b->loss == RG_LOSS_ADAPTIVE_HINGE)
        return fail_arg("rg_ncf_pairs: adaptive hinge runs as scores -> rg_ncf_adapt_dp -> given-dp");
    if (nw->training && (nw->mask_pos == nullptr) != (nw->mask_neg == nullptr))
        return fail_arg("rg_ncf_pairs: give both dropout mask arrays or neither");
    if (w->plan_pos_slot && !w->part_row) return fail_arg("rg_ncf_pairs: plan needs part_row");
    if (ncf_param_len(m) < 0) return fail_arg("rg_ncf_pairs: mf_dim out of range");
    if (m->mf_dim > 0) {
        if (!m->mf_user_w || !m->mf_item_w) return fail_arg("rg_ncf_pairs: NeuMF needs the GMF tables");
        if (phase != kNcfScores && phase != kNcfLossOnly && (!nw->mf_contrib || !nw->mf_hot_grad))
            return fail_arg("rg_ncf_pairs: NeuMF needs mf_contrib / mf_hot_grad");
        if (phase != kNcfScores && phase != kNcfLossOnly && w->plan_pos_slot && !nw->mf_part_row)
            return fail_arg("rg_ncf_pairs: NeuMF plan needs mf_part_row");
    }
    NcfArgs a{};
    a.user_w = m->user_w; a.item_w = m->item_w; a.mlp = m->mlp;
    a.num_users = m->num_users; a.num_items = m->num_items;
    a.pairs = reinterpret_cast<const int2 *>(b->pairs);
    a.n_pos = b->n_pos; a.cols = b->cols; a.global_cols = b->global_cols; a.col_offset = b->col_offset;
    a.n_neg = b->n_neg; a.loss = b->loss;
    if (nw->tile_rows != rg_ncf_rows_per_tile(m->dim, m->mf_dim))
        return fail_arg("rg_ncf_pairs: ncf_work.tile_rows must be rg_ncf_rows_per_tile(dim, mf_dim)");
    a.tc = (int)rg_ncf_cols_per_tile(b->n_neg, m->dim, m->mf_dim);
    a.tiles = rg_ncf_tiles(b->cols, b->n_neg, m->dim, m->mf_dim);
    if (a.tiles >= ((int64_t)1 << 31)) return fail_arg("rg_ncf_pairs: more than 2^31 tiles");
    const int64_t negc = b->neg_cols > 0 ? b->neg_cols : b->global_cols;
    switch (b->loss) {
        case RG_LOSS_POINTWISE: a.n_a = (float)b->global_pos; a.n_b = (float)((int64_t)b->n_neg * negc); break;
        case RG_LOSS_BPR:
        case RG_LOSS_HINGE: a.n_a = (float)((int64_t)b->n_neg * b->global_pos); a.n_b = 1.0f; break;
        default: a.n_a = (float)b->global_pos; a.n_b = 1.0f;
    }
    a.perm = w->plan_perm; a.pos_slot = w->plan_pos_slot;
    a.row_count = w->row_count; a.row_list = reinterpret_cast<int2 *>(w->row_list);
    a.hot_grad = reinterpret_cast<long long *>(w->hot_grad); a.part_row = w->part_row;
    a.loss_partials = w->loss_partials;
    a.contrib = nw->contrib; a.wpart = nw->mlp_partials; a.scores = nw->scores; a.dp_in = nw->dp;
    a.mask_pos = nw->mask_pos; a.mask_neg = nw->mask_neg; a.seed = nw->seed; a.training = nw->training;
    a.mf_dim = m->mf_dim; a.mf_user_w = m->mf_user_w; a.mf_item_w = m->mf_item_w;
    a.mf_contrib = nw->mf_contrib; a.mf_hot_grad = reinterpret_cast<long long *>(nw->mf_hot_grad);
    a.mf_part_row = nw->mf_part_row;
    const int blocks = (int)rg_ncf_blocks(b->cols, b->n_neg, m->dim, m->mf_dim);
    if (blocks <= 0) return fail_arg("rg_ncf_pairs: no launch shape for this dim / mf_dim");
    if (ncf_use_wave(m->dim, m->mf_dim)) return ncf_wave_launch(a, (hipStream_t)stream, blocks, phase);
    return ncf_tile_launch(a, (hipStream_t)stream, blocks, m->dim, phase);
}

extern "C" int rg_ncf_adapt_dp(void *stream, const rg_mf_batch_t *b, rg_ncf_work_t *nw, float *loss_partials) {
    if (!b || !nw || !nw->scores || !nw->dp || !loss_partials) return fail_arg("rg_ncf_adapt_dp: null argument");
    int TR = 0, tc = 0;
    int64_t tiles = 0;
    if (ncf_geometry(nw, b, TR, tc, tiles)) return RG_E_ARG;
    hipLaunchKernelGGL(ncf_adapt_dp_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nw->scores, nw->dp,
                       tiles * TR, TR, tc, b->n_neg + 1, b->n_pos, b->cols, (float)b->global_pos, loss_partials);
    return check_launch("rg_ncf_adapt_dp");
}

// ---- adaptive hinge over several ranks (each holds its column slice of ONE global draw) ----
// The global maximum negative (torch.max over the flat draw: the largest score, the first
// draw index j = k * global_cols + column on ties) is found in three small launches around
// two float SUM all-reduces of the caller: each rank's (score, j) goes into its own slot of a
// zeroed [world][4] buffer (one writer per slot, x + 0 = x: the sum is an all-gather), every
// rank picks the same winner, and the active-positive count is summed before the winner's
// rank sets its row's dp (spotlight/losses.py:133-172, implicit.py:194-199).
__device__ __forceinline__ bool adapt_better(float s, int64_t j, float bs, int64_t bj) {
    return s > bs || (s == bs && j < bj);
}

__device__ __forceinline__ int adapt_winner(const float *slots, int world) {
    int w = 0;
    float bs = slots[0];
    int64_t bj = ((int64_t)slots[1] << 16) | (int64_t)slots[2];
    for (int r = 1; r < world; ++r) {
        const float sc = slots[4 * r];
        const int64_t j = ((int64_t)slots[4 * r + 1] << 16) | (int64_t)slots[4 * r + 2];
        if (adapt_better(sc, j, bs, bj)) { w = r; bs = sc; bj = j; }
    }
    return w;
}

__global__ __launch_bounds__(256) void ncf_adapt_local_kernel(const float *scores, int64_t rows, int TR, int tc, int NP,
                                                             int64_t cols, const int32_t *perm, int64_t global_cols,
                                                             int64_t col_offset, float *slots, int rank, int world,
                                                             int32_t *local_row) {
    __shared__ float ss[256];
    __shared__ int64_t sj[256], sr[256];
    const int tid = threadIdx.x;
    float best = -1.0f;
    int64_t bj = INT64_MAX, br = -1;
    for (int64_t r = tid; r < rows; r += 256) {
        const int64_t tile = r / TR, rr = r % TR;
        const int q = (int)(rr / tc);
        const int64_t s = tile * tc + rr % tc;
        if (q >= 1 && q < NP && s < cols) {
            const int64_t col = perm ? (int64_t)perm[s] : s;
            const int64_t j = (int64_t)(q - 1) * global_cols + col_offset + col;
            if (adapt_better(scores[r], j, best, bj)) { best = scores[r]; bj = j; br = r; }
        }
    }
    ss[tid] = best; sj[tid] = bj; sr[tid] = br;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && adapt_better(ss[tid + w], sj[tid + w], ss[tid], sj[tid])) {
            ss[tid] = ss[tid + w]; sj[tid] = sj[tid + w]; sr[tid] = sr[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int i = 0; i < 4 * world; ++i) slots[i] = 0.0f;
        const int64_t j = sj[0] == INT64_MAX ? 0 : sj[0];
        slots[4 * rank] = ss[0];
        slots[4 * rank + 1] = (float)(j >> 16);
        slots[4 * rank + 2] = (float)(j & 0xffff);
        local_row[0] = (int32_t)sr[0];
    }
}

__global__ __launch_bounds__(256) void ncf_adapt_global_kernel(const float *scores, float *dp, int64_t rows, int TR, int tc,
                                                              int64_t n_pos_cols, float n_a, const float *slots,
                                                              int world, float *count, float *loss_partial) {
    __shared__ float scnt[256], sloss[256];
    const int tid = threadIdx.x;
    const float mx = slots[4 * adapt_winner(slots, world)];
    float cnt = 0.0f, ls = 0.0f;
    for (int64_t r = tid; r < rows; r += 256) {
        const int64_t tile = r / TR, rr = r % TR;
        const int64_t s = tile * tc + rr % tc;
        dp[r] = 0.0f;
        if (rr < (int64_t)tc && s < n_pos_cols) {
            const float x = (mx - scores[r]) + 1.0f;
            ls += fmaxf(x, 0.0f);
            if (x >= 0.0f) { dp[r] = -(1.0f / n_a); cnt += 1.0f; }
        }
    }
    scnt[tid] = cnt;
    sloss[tid] = ls;
    __syncthreads();
    if (tid == 0) {
        float c = 0.0f, l = 0.0f;
        for (int i = 0; i < 256; ++i) { c += scnt[i]; l += sloss[i]; }
        count[0] = c;
        loss_partial[0] = l;
        loss_partial[1] = 0.0f;
    }
}

__global__ void ncf_adapt_winner_kernel(float *dp, const float *slots, int world, int rank, const int32_t *local_row,
                                        const float *count, float n_a) {
    if (threadIdx.x == 0 && adapt_winner(slots, world) == rank && local_row[0] >= 0)
        dp[local_row[0]] = count[0] * (1.0f / n_a);
}

extern "C" int rg_ncf_adapt_local(void *stream, const rg_mf_batch_t *b, const rg_mf_work_t *w, rg_ncf_work_t *nw,
                                  float *slots, int32_t rank, int32_t world, int32_t *local_row) {
    if (!b || !w || !nw || !nw->scores || !slots || !local_row || world < 1 || rank < 0 || rank >= world)
        return fail_arg("rg_ncf_adapt_local: bad argument");
    int TR = 0, tc = 0;
    int64_t tiles = 0;
    if (ncf_geometry(nw, b, TR, tc, tiles)) return RG_E_ARG;
    hipLaunchKernelGGL(ncf_adapt_local_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nw->scores, tiles * TR, TR,
                       tc, b->n_neg + 1, b->cols, w->plan_perm, b->global_cols, b->col_offset, slots, rank, world,
                       local_row);
    return check_launch("rg_ncf_adapt_local");
}

extern "C" int rg_ncf_adapt_global(void *stream, const rg_mf_batch_t *b, rg_ncf_work_t *nw, const float *slots,
                                   int32_t world, float *count, float *loss_partials) {
    if (!b || !nw || !nw->scores || !nw->dp || !slots || !count || !loss_partials || world < 1)
        return fail_arg("rg_ncf_adapt_global: bad argument");
    int TR = 0, tc = 0;
    int64_t tiles = 0;
    if (ncf_geometry(nw, b, TR, tc, tiles)) return RG_E_ARG;
    hipLaunchKernelGGL(ncf_adapt_global_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nw->scores, nw->dp,
                       tiles * TR, TR, tc, b->n_pos, (float)b->global_pos, slots, world, count, loss_partials);
    return check_launch("rg_ncf_adapt_global");
}

extern "C" int rg_ncf_adapt_winner(void *stream, const rg_mf_batch_t *b, rg_ncf_work_t *nw, const float *slots,
                                   int32_t world, int32_t rank, const int32_t *local_row, const float *count) {
    if (!b || !nw || !nw->dp || !slots || !local_row || !count || world < 1 || rank < 0 || rank >= world)
        return fail_arg("rg_ncf_adapt_winner: bad argument");
    hipLaunchKernelGGL(ncf_adapt_winner_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, nw->dp, slots, world, rank,
                       local_row, count, (float)b->global_pos);
    return check_launch("rg_ncf_adapt_winner");
}

extern "C" int rg_ncf_update(void *stream, const rg_ncf_model_t *m, const rg_ncf_work_t *nw, int64_t nparts,
                             const rg_opt_t *opt, const float *loss_partials, const rg_mf_loss_t *loss) {
    if (!m || !nw || !opt || !nw->mlp_partials || !m->mlp) return fail_arg("rg_ncf_update: null argument");
    if (opt->kind == RG_OPT_ADAM && !m->mlp_m) return fail_arg("rg_ncf_update: Adam needs m state");
    if (opt->kind != RG_OPT_SGD && !m->mlp_v) return fail_arg("rg_ncf_update: optimizer needs v state");
    if (loss && loss->out && !loss_partials) return fail_arg("rg_ncf_update: loss needs partials");
    const int P = (int)ncf_param_len(m);
    if (P < 0) return fail_arg("rg_ncf_update: bad dim / mf_dim");
    const bool with_loss = loss && loss->out;
    hipLaunchKernelGGL(ncf_update_kernel, dim3((P + 63) / 64), dim3(kUpdWaves * 64), 0, (hipStream_t)stream, m->mlp,
                       opt->kind == RG_OPT_ADAM ? m->mlp_m : nullptr, opt->kind == RG_OPT_SGD ? nullptr : m->mlp_v,
                       nw->mlp_partials, (int)nparts, P, *opt, with_loss ? loss_partials : nullptr,
                       with_loss ? loss->n_partials : 0, with_loss ? loss->inv_a : 0.0,
                       with_loss ? loss->inv_b : 0.0, with_loss ? loss->out : nullptr, 0, nullptr);
    return check_launch("rg_ncf_update");
}

extern "C" int rg_ncf_mlp_grad(void *stream, const rg_ncf_model_t *m, const rg_ncf_work_t *nw, int64_t nparts,
                               const float *loss_partials, const rg_mf_loss_t *loss, float *grad) {
    if (!m || !nw || !nw->mlp_partials || !grad || !loss || !loss_partials)
        return fail_arg("rg_ncf_mlp_grad: null argument");
    const int P = (int)ncf_param_len(m);
    if (P < 0) return fail_arg("rg_ncf_mlp_grad: bad dim / mf_dim");
    hipLaunchKernelGGL(ncf_update_kernel, dim3((P + 63) / 64), dim3(kUpdWaves * 64), 0, (hipStream_t)stream, m->mlp,
                       nullptr, nullptr, nw->mlp_partials, (int)nparts, P, rg_opt_t{}, loss_partials,
                       loss->n_partials, loss->inv_a, loss->inv_b, loss->out, 1, grad);
    return check_launch("rg_ncf_mlp_grad");
}

extern "C" int rg_ncf_mlp_apply(void *stream, const rg_ncf_model_t *m, const float *grad, const rg_opt_t *opt,
                                float *loss_out) {
    if (!m || !grad || !opt || !m->mlp) return fail_arg("rg_ncf_mlp_apply: null argument");
    if (opt->kind == RG_OPT_ADAM && !m->mlp_m) return fail_arg("rg_ncf_mlp_apply: Adam needs m state");
    if (opt->kind != RG_OPT_SGD && !m->mlp_v) return fail_arg("rg_ncf_mlp_apply: optimizer needs v state");
    const int P = (int)ncf_param_len(m);
    if (P < 0) return fail_arg("rg_ncf_mlp_apply: bad dim / mf_dim");
    hipLaunchKernelGGL(ncf_update_kernel, dim3((P + 63) / 64), dim3(kUpdWaves * 64), 0, (hipStream_t)stream, m->mlp,
                       opt->kind == RG_OPT_ADAM ? m->mlp_m : nullptr, opt->kind == RG_OPT_SGD ? nullptr : m->mlp_v,
                       nullptr, 0, P, *opt, nullptr, 0, 0.0, 0.0, loss_out, 2, const_cast<float *>(grad));
    return check_launch("rg_ncf_mlp_apply");
}

#ifdef RG_DIAG_STAMPS
extern "C" int rg_diag_set_ncf_stamps(unsigned long long *dev_buf) {
    const int rc = ncf_tile_set_stamps(dev_buf);
    return rc != RG_OK ? rc : ncf_wave_set_stamps(dev_buf);
}
#endif
