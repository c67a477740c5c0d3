// Item-to-item similarity ("more like this"): the k rows of an embedding table most similar to
// each query row, without the (queries, rows) block.  For query row q and candidate row c
//     dot  = <table[q], table[c]>          rg_mf_score_tile.h's product(), user_w = item_w = table
//     sim  = (dot * rnorm[q]) * rnorm[c]   cosine: two fp32 multiplies in that order (rnorm given)
//          = dot                           inner product (rnorm null)
// -inf at c == q with RG_SIM_EXCLUDE_SELF; the key of a NaN is -inf; the k best columns by (key
// descending, column ascending) and their values leave the device.
//
//   rnorms   rg_row_rnorms: 1 / sqrt(sum of squares) per row, 0 for a zero row.  16 lanes per row;
//            lane l owns columns 4 (l + 16 c) .. + 3 of chunk c = 0, 1, ... and adds their squares in
//            ascending order with one fma each, then the 16 partials meet in a DPP butterfly
//            (group_sum: every step adds a value and its partner's, which commute exactly).  The
//            order depends on dim alone -- not on the row's position, the row count or whether the
//            columns came as one 16-byte load (dim % 4 == 0, aligned table) or as scalars.
//   top-k    the grid, tiles, LDS score tile, four-threads-per-row register lists, LDS merge and
//            second launch of rg_mf_topk.hip (rg_topk_lists.h holds what the two share), with the
//            queries in the users' place.  There are no exclusion lists: the one excluded column of
//            a row, its own, is written as -inf by the finishing function.
//   sims     the finishing function, the sibling of mf_tile::scores(): it reads rnorm once per
//            row and once per column of the wave's accumulators.
//   ids      a workgroup first compares the (up to 64) query ids of its group with [0, num_rows):
//            if one is outside, the group's rows get the id -1 and the value NaN and the workgroup
//            ends before product() gathers anything.  So no query id indexes the table or rnorm
//            unchecked, and no id the kernel produced indexes anything.
//
// No atomics.  The table, rnorm and the queries are only read.
#include "rg_topk_lists.h"

namespace rg {
namespace {

using namespace mf_tile;
using namespace topk;

constexpr int kTStride = kTile + 4;                 // row stride of the LDS score tile (floats), as rg_mf_topk.hip
static_assert(kGroup * kTStride <= kItemFloats, "the score tile takes the item image's place");
constexpr int kLdsFloats = kItemFloats + kUserFloats;

// ---------------------------------------------------------------- reciprocal norms
constexpr int kNormLanes = 16, kNormRows = kThreads / kNormLanes;   // lanes per row, rows per workgroup

template <bool VEC>
__global__ __launch_bounds__(kThreads) void row_rnorms_kernel(const float *__restrict__ table, int64_t rows, int dim,
                                                              float *__restrict__ out) {
    const int tid = threadIdx.x, l = tid % kNormLanes;
    const int64_t r = (int64_t)blockIdx.x * kNormRows + tid / kNormLanes;
    float s = 0.0f;
    if (r < rows) {
        const float *p = table + r * dim;
        for (int c = 4 * l; c < dim; c += 4 * kNormLanes) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if constexpr (VEC) {
                v = *reinterpret_cast<const float4 *>(p + c);       // dim % 4 == 0: c + 3 < dim
            } else {
                v.x = p[c];
                if (c + 1 < dim) v.y = p[c + 1];
                if (c + 2 < dim) v.z = p[c + 2];
                if (c + 3 < dim) v.w = p[c + 3];
            }
            s = fmaf(v.x, v.x, s);
            s = fmaf(v.y, v.y, s);
            s = fmaf(v.z, v.z, s);
            s = fmaf(v.w, v.w, s);
        }
    }
    s = group_sum<kNormLanes>(s);                   // every lane of the wave takes part
    if (r < rows && l == 0) out[r] = s == 0.0f ? 0.0f : 1.0f / sqrtf(s);
}

// ---------------------------------------------------------------- similarity top-k
struct SimArgs {
    Tables t;                                       // user_w = item_w = the table, users = the queries; no biases
    const float *rnorm;                             // null: inner product
    int64_t groups, tiles;
    int splits, k;
    bool exclude_self;
    float *dst_v;                                   // [n_queries][splits][k]; null: values not wanted
    int32_t *dst_i;
};

// The similarities of an active wave's accumulators: sink(ul, c, sim) for every query
// u0 + ul < n_users of the wave (ul = 16 wave + 4 g + r in the group) and every column
// c = 16 nb + j of the tile with i0 + c < num_items.  The query ids are in range (the caller's check).
template <class Sink>
__device__ __forceinline__ void sims(const SimArgs &a, int64_t i0, int64_t u0, const v4f (&acc)[NB], Sink &&sink) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
    float rc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int64_t item = i0 + 16 * nb + j;
        rc[nb] = a.rnorm && item < a.t.num_items ? a.rnorm[item] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ul = wave * 16 + 4 * g + r;
        const int64_t u = u0 + ul;
        if (u >= a.t.n_users) continue;
        const int64_t q = a.t.users[u];
        const float rq = a.rnorm ? a.rnorm[q] : 0.0f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int64_t item = i0 + 16 * nb + j;
            if (item >= a.t.num_items) continue;
            float s = acc[nb][r];
            if (a.rnorm) s = (s * rq) * rc[nb];     // multiplies only: nothing to contract
            if (a.exclude_self && item == q) s = -INFINITY;
            sink(ul, 16 * nb + j, s);
        }
    }
}

template <bool VEC, int K>
__global__ __launch_bounds__(kThreads, 2) void item_sim_kernel(SimArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[kLdsFloats];
    float *sI = smem, *sU = smem + kItemFloats, *sT = smem;
    const int tid = threadIdx.x, ul = tid >> 2, q = tid & 3;
    const int64_t split = (int64_t)blockIdx.x / a.groups, grp = (int64_t)blockIdx.x - split * a.groups;
    const int64_t u0 = grp * kGroup, r = u0 + ul;
    const bool has_user = r < a.t.n_users;
    const int64_t t_begin = split * a.tiles / a.splits, t_end = (split + 1) * a.tiles / a.splits;

    // ---- the group's query ids against the table, before anything is gathered by them
    const bool bad = tid < kGroup && u0 + tid < a.t.n_users &&
                     (uint64_t)a.t.users[u0 + tid] >= (uint64_t)a.t.num_items;
    if (__syncthreads_or(bad)) {
        if (has_user) {
            const int64_t dst = (r * a.splits + split) * a.k;
            for (int j = q; j < a.k; j += 4) {
                a.dst_i[dst + j] = -1;
                if (a.dst_v) a.dst_v[dst + j] = NAN;
            }
        }
        return;
    }

    TopList<K> top;
    top.init();
    const float *trow = sT + ul * kTStride;
    for (int64_t t = t_begin; t < t_end; ++t) {
        const int64_t i0 = t * kTile;
        const int ncols = (int)(a.t.num_items - i0 < kTile ? a.t.num_items - i0 : kTile);
        v4f acc[NB];
        const bool active = product<VEC>(a.t, i0, u0, sI, sU, acc);
        __syncthreads();                            // every wave has read sI: the score tile takes its place
        if (active)
            sims(a, i0, u0, acc, [&](int row, int c, float s) { sT[row * kTStride + c] = s; });
        __syncthreads();
        if (has_user)
            for (int c = q; c < ncols; c += 4) top.insert(trow[c], (int)(i0 + c));
        __syncthreads();                            // the tile has been scanned: sI and sU are free
    }

    // ---- the four lists of a query into one, kPerPass threads' lists in LDS at a time (rg_mf_topk.hip)
    constexpr int kPasses = 2 * K * kThreads > kLdsFloats ? 2 : 1, kPerPass = kThreads / kPasses;
    static_assert(2 * K * kPerPass <= kLdsFloats, "merge lists fit the staging LDS");
    float *sv = smem;
    int *si = reinterpret_cast<int *>(smem + K * kPerPass);
    const int lt = tid % kPerPass;
    for (int h = 0; h < kPasses; ++h) {
        const bool mine = tid / kPerPass == h;
        if (mine) top.store(sv + lt * K, si + lt * K);
        __syncthreads();
        for (int s = 1; s < 4; s <<= 1) {
            if (mine && (lt & (2 * s - 1)) == 0) merge_pair<K>(sv, si, lt, lt + s);
            __syncthreads();
        }
        if (mine && has_user) {
            const int64_t dst = (r * a.splits + split) * a.k;
            for (int j = q; j < a.k; j += 4) {
                a.dst_i[dst + j] = si[(lt - q) * K + j];
                if (a.dst_v) a.dst_v[dst + j] = sv[(lt - q) * K + j];
            }
        }
        __syncthreads();
    }
}

template <bool VEC, int K>
int launch(hipStream_t s, const SimArgs &a, const float *ws_v, const int32_t *ws_i, int32_t *out_idx, float *out_sims) {
    hipLaunchKernelGGL((item_sim_kernel<VEC, K>), dim3((unsigned)(a.groups * a.splits)), dim3(kThreads), 0, s, a);
    if (a.splits > 1)
        hipLaunchKernelGGL((mf_topk_merge_kernel<K>), dim3((unsigned)a.t.n_users), dim3(kMergeThreads), 0, s, ws_v, ws_i,
                           (int64_t)a.splits * a.k, a.k, out_idx, out_sims);
    return check_launch("rg_item_sim_topk");
}

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int rg_row_rnorms(void *stream, const float *table, int64_t rows, int32_t dim, float *out) {
    if (!table || !out) return fail_arg("rg_row_rnorms: null pointer");
    if (dim < 1) return fail_arg("rg_row_rnorms: dim < 1");
    if (rows < 0) return fail_arg("rg_row_rnorms: rows < 0");
    const int64_t blocks = (rows + kNormRows - 1) / kNormRows;
    if (blocks > INT_MAX) return fail_arg("rg_row_rnorms: too many rows for one launch (rows > 16 (2^31 - 1))");
    if (rows == 0) return RG_OK;
    const hipStream_t st = (hipStream_t)stream;
    if (dim % 4 == 0 && (uintptr_t)table % 16 == 0)
        hipLaunchKernelGGL(row_rnorms_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, table, rows, dim, out);
    else
        hipLaunchKernelGGL(row_rnorms_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, table, rows, dim, out);
    return check_launch("rg_row_rnorms");
}

extern "C" int64_t rg_item_sim_workspace_len(int64_t num_rows, int64_t n_queries, int32_t k, int32_t splits) {
    if (check_shape("rg_item_sim_workspace_len", num_rows, n_queries, k, splits) != RG_OK) return -1;
    return 8 * n_queries * k * pick_splits(num_rows, n_queries, splits);   // queries x splits < 2^30: no overflow
}

extern "C" int rg_item_sim_topk(void *stream, const float *table, const float *rnorm, int32_t dim, int64_t num_rows,
                                const int64_t *queries_dev, int64_t n_queries, int32_t flags, int32_t k,
                                int32_t splits, void *workspace_dev, int32_t *out_idx, float *out_sims) {
    if (!table || !queries_dev || !workspace_dev || !out_idx) return fail_arg("rg_item_sim_topk: null pointer");
    if (flags & ~RG_SIM_EXCLUDE_SELF) return fail_arg("rg_item_sim_topk: unknown flag bits");
    if (dim < 1 || dim > 256) return fail_arg("rg_item_sim_topk: dim must be in [1, 256]");
    if (const int rc = check_shape("rg_item_sim_topk", num_rows, n_queries, k, splits)) return rc;
    const bool exclude_self = flags & RG_SIM_EXCLUDE_SELF;
    if (exclude_self && k > num_rows - 1)
        return fail_arg("rg_item_sim_topk: k must be in [1, min(32, num_rows - 1)] with RG_SIM_EXCLUDE_SELF");
    if (n_queries == 0) return RG_OK;
    const int64_t tiles = (num_rows + kTile - 1) / kTile, groups = (n_queries + kGroup - 1) / kGroup;
    const int64_t s = pick_splits(num_rows, n_queries, splits);
    float *ws_v = static_cast<float *>(workspace_dev);
    int32_t *ws_i = reinterpret_cast<int32_t *>(ws_v + n_queries * s * k);
    SimArgs a{{table, table, nullptr, nullptr, queries_dev, num_rows, n_queries, dim}, rnorm, groups, tiles,
              (int)s, k, exclude_self, s == 1 ? out_sims : ws_v, s == 1 ? out_idx : ws_i};
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = vec_loads(table, table, dim);
    if (k <= 8)
        return vec ? launch<true, 8>(st, a, ws_v, ws_i, out_idx, out_sims)
                   : launch<false, 8>(st, a, ws_v, ws_i, out_idx, out_sims);
    if (k <= 16)
        return vec ? launch<true, 16>(st, a, ws_v, ws_i, out_idx, out_sims)
                   : launch<false, 16>(st, a, ws_v, ws_i, out_idx, out_sims);
    return vec ? launch<true, 32>(st, a, ws_v, ws_i, out_idx, out_sims)
               : launch<false, 32>(st, a, ws_v, ws_i, out_idx, out_sims);
}
