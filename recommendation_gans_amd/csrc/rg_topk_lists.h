// What the fused top-k kernels share (rg_mf_topk.hip: MF recommend; rg_item_sim.hip: item-to-item
// similarity): the order, the register top-K lists, their LDS merge, the second launch that merges
// the splits, and the host-side shape rules of the (row group, split) grid over rg_mf_score_tile.h's
// tiles.
//
// (key, column) is a total order -- key descending, column ascending, the key of a NaN is -inf --
// so no two candidates compare equal and the k best and their order do not depend on the splits,
// their boundaries, the thread that saw a column or the order of any merge.
//
// Everything here has internal linkage (an unnamed namespace, as in the sources that include it):
// each translation unit gets its own copy of the merge kernel.
#pragma once
#include <climits>

#include "rg_mf_score_tile.h"

namespace rg {
namespace topk {
namespace {

using namespace mf_tile;

constexpr int kTopkMax = 32;
constexpr int kMergeThreads = 64;                   // second launch: one wave per user

__device__ __forceinline__ float key_of(float x) { return x != x ? -INFINITY : x; }    // NaN ranks last
__device__ __forceinline__ bool better(float ka, int ia, float kb, int ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// a sorted top-K of (value, column) in registers, best first; filler (-inf, INT_MAX)
template <int K>
struct TopList {
    float v[K];
    int ix[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < K; ++j) { v[j] = -INFINITY; ix[j] = INT_MAX; }
    }
    // carry the displaced element down the list: selects with static indices, no branch per slot
    __device__ __forceinline__ void insert(float x, int xi) {
        float xk = key_of(x);
        if (!better(xk, xi, key_of(v[K - 1]), ix[K - 1])) return;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float tv = v[j], tk = key_of(tv);
            const int ti = ix[j];
            const bool in = better(xk, xi, tk, ti);
            v[j] = in ? x : tv;
            ix[j] = in ? xi : ti;
            x = in ? tv : x;
            xi = in ? ti : xi;
            xk = in ? tk : xk;
        }
    }
    __device__ __forceinline__ void store(float *sv, int *si) const {
#pragma unroll
        for (int j = 0; j < K; ++j) { sv[j] = v[j]; si[j] = ix[j]; }
    }
};

// LDS lists of K entries, list l at [l K, l K + K): the K best of lists a and b into a, by one
// thread.  The two heads never pass K - 1 together (p + q == j), so every read is inside a list.
template <int K>
__device__ __forceinline__ void merge_pair(float *sv, int *si, int a, int b) {
    const float *av = sv + a * K, *bv = sv + b * K;
    const int *ai = si + a * K, *bi = si + b * K;
    float mv[K];
    int mi[K];
    int p = 0, q = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float x = av[p], y = bv[q];
        const int xi = ai[p], yi = bi[q];
        const bool take_a = better(key_of(x), xi, key_of(y), yi);
        mv[j] = take_a ? x : y;
        mi[j] = take_a ? xi : yi;
        p += take_a ? 1 : 0;
        q += take_a ? 0 : 1;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) { sv[a * K + j] = mv[j]; si[a * K + j] = mi[j]; }
}

// splits > 1: the k best of a user's cand = splits x k candidates (ws_v / ws_i [n_users][cand])
template <int K>
__global__ __launch_bounds__(kMergeThreads) void mf_topk_merge_kernel(const float *__restrict__ ws_v,
                                                                      const int32_t *__restrict__ ws_i, int64_t cand,
                                                                      int k, int32_t *__restrict__ out_idx,
                                                                      float *__restrict__ out_scores) {
    __shared__ float sv[kMergeThreads * K];
    __shared__ int si[kMergeThreads * K];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    TopList<K> top;
    top.init();
    for (int64_t c = tid; c < cand; c += kMergeThreads) top.insert(ws_v[r * cand + c], ws_i[r * cand + c]);
    top.store(sv + tid * K, si + tid * K);
    __syncthreads();
    for (int s = 1; s < kMergeThreads; s <<= 1) {
        if ((tid & (2 * s - 1)) == 0) merge_pair<K>(sv, si, tid, tid + s);
        __syncthreads();
    }
    if (tid < k) {
        out_idx[r * k + tid] = si[tid];
        if (out_scores) out_scores[r * k + tid] = sv[tid];
    }
}

// shape checks shared by the entry points; 0 or the failure's status
int check_shape(const char *fn, int64_t num_items, int64_t n_users, int32_t k, int32_t splits) {
    const std::string f = std::string(fn) + ": ";
    if (num_items < 1) return fail_arg(f + "num_items < 1");
    if (num_items > INT_MAX) return fail_arg(f + "num_items must fit int32");
    if (n_users < 0) return fail_arg(f + "n_users < 0");
    if (k < 1 || k > kTopkMax || k > num_items) return fail_arg(f + "k must be in [1, min(32, num_items)]");
    const int64_t tiles = (num_items + kTile - 1) / kTile;
    if (splits < 0 || splits > tiles)
        return fail_arg(f + "splits must be in [0, item tiles] (" + std::to_string(tiles) + " tiles of " +
                        std::to_string(kTile) + " items)");
    // a launch holds fewer than 2^32 threads: (user group, split) workgroups, and a wave per user.
    // The library's own pick (splits == 0) is 1 unless user groups x splits stays below 6 CUs, so it
    // is refused exactly when one split is: no need to ask the device before refusing.
    const int64_t groups = (n_users + kGroup - 1) / kGroup;
    if (groups > 0 && ((splits > 0 ? splits : 1) > (int64_t)(UINT_MAX / kThreads) / groups ||
                       n_users > (int64_t)(UINT_MAX / kMergeThreads)))
        return fail_arg(f + "too many users x splits for one launch (user groups x splits > 2^24 - 1 or users > "
                            "2^26 - 1)");
    return RG_OK;
}

// splits == 0: enough splits to give every CU three workgroups (two resident, one waiting), in [1, tiles].
// The only HIP call ahead of the launch (the CU count, cached): after every refusal.
int64_t pick_splits(int64_t num_items, int64_t n_users, int32_t splits) {
    if (splits > 0) return splits;
    const int64_t tiles = (num_items + kTile - 1) / kTile, groups = (n_users + kGroup - 1) / kGroup;
    const int64_t want = groups > 0 ? (3 * (int64_t)num_cus() + groups - 1) / groups : 1;
    return want < 1 ? 1 : want > tiles ? tiles : want;
}

}  // namespace
}  // namespace topk
}  // namespace rg
