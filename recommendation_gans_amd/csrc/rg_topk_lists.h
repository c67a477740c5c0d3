// Sorted top-K lists of (value, column), shared by every kernel that selects on the device
// (rg_eval.hip: rg_topk_rows; rg_topk_tiles.h: the fused tile-walk kernels and the merge of their
// splits): the order, the register list with its insertion, the pairwise LDS merge and the merge
// tree.  Pure list code: it knows nothing of tiles, grids or tables.
//
// (key, column) is a total order -- key descending, column ascending, the key of a NaN is -inf --
// so no two candidates compare equal and the k best and their order do not depend on the thread
// that saw a column or the order of any merge.
//
// Everything here has internal linkage (an unnamed namespace, as in the sources that include it).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

namespace rg {
namespace topk {
namespace {

constexpr int kTopkMax = 32;

__device__ __forceinline__ float key_of(float x) { return x != x ? -INFINITY : x; }    // NaN ranks last
// NANS false: the lists hold no NaN (the caller put keys in), so a value is its own key
template <bool NANS>
__device__ __forceinline__ float key_if(float x) { return NANS ? key_of(x) : x; }
__device__ __forceinline__ bool better(float ka, int ia, float kb, int ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// a sorted top-K of (value, column) in registers, best first; filler (-inf, INT_MAX)
template <int K, bool NANS = true>
struct TopList {
    float v[K];
    int ix[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < K; ++j) { v[j] = -INFINITY; ix[j] = INT_MAX; }
    }
    // Carry the displaced element down the list, behind an early test against the last element.
    // The list holds the raw value (a NaN stays the NaN it was) and compares by key.
    // Selects with static indices, not a branch per slot: as a branch, the compiler's code for
    // slot 0 lost an element that entered on the id alone (equal key, lower id), which is how a
    // -inf entry meets the (-inf, INT_MAX) filler, and the filler's id came out instead.
    __device__ __forceinline__ void insert(float x, int xi) {
        float xk = key_if<NANS>(x);
        if (!better(xk, xi, key_if<NANS>(v[K - 1]), ix[K - 1])) return;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float tv = v[j], tk = key_if<NANS>(tv);
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
template <int K, bool NANS = true>
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
        const bool take_a = better(key_if<NANS>(x), xi, key_if<NANS>(y), yi);
        mv[j] = take_a ? x : y;
        mi[j] = take_a ? xi : yi;
        p += take_a ? 1 : 0;
        q += take_a ? 0 : 1;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) { sv[a * K + j] = mv[j]; si[a * K + j] = mi[j]; }
}

// THREADS consecutive LDS lists into the first: at stride s, thread t (t % 2s == 0) merges lists
// t and t + s into t.  Called by every thread of the workgroup (it holds barriers, and opens with
// none: the caller's barrier orders the lists' stores before it); a thread with `on` false only
// keeps the barriers.
template <int K, int THREADS, bool NANS = true>
__device__ __forceinline__ void merge_tree(float *sv, int *si, int tid, bool on = true) {
    for (int s = 1; s < THREADS; s <<= 1) {
        if (on && (tid & (2 * s - 1)) == 0) merge_pair<K, NANS>(sv, si, tid, tid + s);
        __syncthreads();
    }
}

}  // namespace
}  // namespace topk
}  // namespace rg
