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
//   top-k    rg_topk_tiles.h's tile_topk_kernel with the queries in the users' place: its grid,
//            tiles, LDS score tile, register lists, LDS merge and second launch.  This file holds the
//            Op.  There are no exclusion lists (no mask, and one barrier per tile less than MF
//            recommend): the one excluded column of a row, its own, is written as -inf by finish.
//   finish   the sibling of mf_tile::scores(): it reads rnorm once per row and once per column of
//            the wave's accumulators.
//   ids      a workgroup first compares the (up to 64) query ids of its group with [0, num_rows):
//            if one is outside, the group's rows get the id -1 and the value NaN and the workgroup
//            ends before product() gathers anything.  So no query id indexes the table or rnorm
//            unchecked, and no id the kernel produced indexes anything.
//
// No atomics.  The table, rnorm and the queries are only read.
#include "rg_topk_tiles.h"

namespace rg {
namespace {

using namespace topk;

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
// Tables: user_w = item_w = the table, users = the queries; no biases
struct SimOp {
    static constexpr bool kMasks = false;
    const float *rnorm;                             // null: inner product
    bool exclude_self;

    // the group's query ids against the table, before anything is gathered by them
    __device__ __forceinline__ bool begin(const Tables &t, int64_t u0, int64_t) const {
        const int tid = threadIdx.x;
        const bool bad = tid < kGroup && u0 + tid < t.n_users && (uint64_t)t.users[u0 + tid] >= (uint64_t)t.num_items;
        return !__syncthreads_or(bad);
    }
    // The similarities of an active wave's accumulators into the LDS tile: row ul, column c for
    // every query u0 + ul < n_users of the wave (ul = 16 wave + 4 g + r in the group) and every
    // column c = 16 nb + j of the tile with i0 + c < num_items.  The query ids are in range (begin).
    __device__ __forceinline__ void finish(const Tables &t, int64_t i0, int64_t u0, const v4f (&acc)[NB],
                                           float *sT) const {
        const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
        float rc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int64_t item = i0 + 16 * nb + j;
            rc[nb] = rnorm && item < t.num_items ? rnorm[item] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ul = wave * 16 + 4 * g + r;
            const int64_t u = u0 + ul;
            if (u >= t.n_users) continue;
            const int64_t q = t.users[u];
            const float rq = rnorm ? rnorm[q] : 0.0f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int64_t item = i0 + 16 * nb + j;
                if (item >= t.num_items) continue;
                float s = acc[nb][r];
                if (rnorm) s = (s * rq) * rc[nb];   // multiplies only: nothing to contract
                if (exclude_self && item == q) s = -INFINITY;
                sT[ul * kTStride + 16 * nb + j] = s;
            }
        }
    }
};

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
    return workspace_len("rg_item_sim_workspace_len", num_rows, n_queries, k, splits);
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
    return run("rg_item_sim_topk", (hipStream_t)stream,
               Tables{table, table, nullptr, nullptr, queries_dev, num_rows, n_queries, dim},
               SimOp{rnorm, exclude_self}, k, splits, workspace_dev, out_idx, out_sims);
}
