// Candidate lists (rg_mf_score_lists, rg_seg_topk, rg_seg_rank): score a ragged list of items per
// user, then rank inside each list -- re-ranking a retrieval stage's candidates, and the sampled
// evaluation protocol (one held-out item among drawn negatives).  The lists are a CSR over the
// call's rows: list r is list_idx[list_ptr[r] .. list_ptr[r + 1]).  One launch per entry, no
// workspace, no atomics.
//
// rg_mf_score_lists: a list is owned by one group of L::LPU lanes (the pair kernel's row layout,
// rg_common.h, as in rg_mf_fold.hip), 64 / LPU lists per wave, one wave per workgroup.  The user's
// row and bias stay in registers while the list is walked kIF entries at a time (kIF gathered item
// rows in flight per group); a score (row_score, rg_common.h, with the other row-group helpers
// used here) is the lane's fmaf chain over its elements in ascending order,
// the group's butterfly (group_sum), then (dot + b) + c and the sigmoid -- one fixed order that
// depends on dim and the tables' alignment alone, so a (user, item) pair is the same bits at any
// position of any list.  The wave loops to its longest list; the shorter ones are masked with
// selects (their loads read item row 0) and store nothing.
//
// rg_seg_topk / rg_seg_rank: one wave per list, four waves per workgroup (they share nothing).
// The order is rg_topk_lists.h's -- key descending, the key of a NaN is -inf, then the id
// ascending -- completed by the position ascending, so a repeated id is a distinct entry and
// (key, id, position) is a total order: the result does not depend on which lane saw an entry.
// The top-k keeps a sorted list per lane (the shared TopList's insertion, restated here with the
// position as a third field: TopList carries (value, column) only), walks the list 64 entries at
// a time, and then takes the best head of the 64 lists k times (a butterfly over the lanes; the
// lane that held it pops).  The rank counts, over the other entries, the keys above entry 0's and
// the equal keys with a lower id: those the top-k places before it.
#include "rg_common.h"
#include "rg_topk_lists.h"

#include <limits.h>

namespace rg {
namespace {

constexpr int kIF = 4;            // item rows in flight per lane group
constexpr int kSegWaves = 4;      // lists (waves) per workgroup of the segmented kernels
constexpr int kSegUnroll = 2;     // loads in flight per lane while a list is walked

struct ScoreListArgs {
    const float *user_w, *item_w, *user_b, *item_b;
    int32_t dim;
    const int64_t *users, *list_ptr;
    const int32_t *list_idx;
    int64_t n;
    float *out;
};

// dim % 4 == 0 off the pair kernel's sizes, 16-byte aligned tables: lane `sub` of the row's LPU
// owns the float4 at floats [4 sub, 4 sub + 4) when that lies inside the row, zeros otherwise
template <int LPU_>
struct VecLayout {
    static constexpr int LPU = LPU_;
    static constexpr int EPL = 4;
    static constexpr int UPW = kWave / LPU;
    __device__ static __forceinline__ void load(float (&v)[EPL], const float *__restrict__ base, int64_t row, int D,
                                                int sub) {
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (sub * 4 < D) t = *reinterpret_cast<const float4 *>(base + row * (int64_t)D + sub * 4);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    __device__ static __forceinline__ void zero(float (&v)[EPL]) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) v[e] = 0.0f;
    }
};

template <class L>
__global__ void __launch_bounds__(kWave) mf_score_lists_kernel(const ScoreListArgs a) {
    constexpr int LPU = L::LPU, EPL = L::EPL, UPW = L::UPW;
    const int lane = threadIdx.x;
    const int sub = lane & (LPU - 1);
    const int64_t r = (int64_t)blockIdx.x * UPW + lane / LPU;
    const bool in = r < a.n;
    const int64_t off = in ? a.list_ptr[r] : 0;
    const int64_t len = in ? a.list_ptr[r + 1] - off : 0;
    const int64_t maxlen = wave_max64(len);
    if (maxlen <= 0) return;

    const int D = a.dim;
    const float *__restrict__ Q = a.item_w;
    const float *__restrict__ C = a.item_b;
    const int32_t *__restrict__ idx = a.list_idx;
    float p[EPL], pb = 0.0f;
    L::zero(p);
    if (len > 0) {
        const int64_t u = a.users[r];
        L::load(p, a.user_w, u, D, sub);
        pb = a.user_b[u];
    }
    for (int64_t e0 = 0; e0 < maxlen; e0 += kIF) {
        bool ev[kIF];
        int id[kIF];
#pragma unroll
        for (int j = 0; j < kIF; ++j) {
            ev[j] = e0 + j < len;
            id[j] = ev[j] ? idx[off + e0 + j] : 0;
        }
        float q[kIF][EPL], c[kIF];
#pragma unroll
        for (int j = 0; j < kIF; ++j) {
            L::load(q[j], Q, id[j], D, sub);
            c[j] = C[id[j]];
        }
#pragma unroll
        for (int j = 0; j < kIF; ++j) {
            const float s = row_score<L>(p, q[j], pb, c[j]);
            if (ev[j] && sub == 0) a.out[off + e0 + j] = s;
        }
    }
}

// the layout of `dim`: dispatch_rows' (rg_common.h), but with 16-byte aligned tables a float4 per
// lane at the multiples of 4 that are not the pair kernel's own sizes
template <typename F>
int dispatch_lists(int dim, bool aligned, F &&f) {
    const bool pair_dim = dim == 8 || dim == 16 || dim == 32 || dim == 64 || dim == 128 || dim == 256;
    if (aligned && dim % 4 == 0 && !pair_dim) {
        if (dim <= 64) return f.template operator()<VecLayout<16>>();
        if (dim <= 128) return f.template operator()<VecLayout<32>>();
        return f.template operator()<VecLayout<64>>();
    }
    return dispatch_rows(dim, aligned, f);
}

struct ScoreListLaunch {
    const ScoreListArgs &a;
    hipStream_t stream;
    template <class L>
    int operator()() const {
        return launch_row_groups<L>(mf_score_lists_kernel<L>, a.n, a, stream, "rg_mf_score_lists",
                                    "too many lists for one launch");
    }
};

// ---------------------------------------------------------------- segmented order
// (key, id, position): rg_topk_lists.h's better() on (key, id), then the lower position
__device__ __forceinline__ bool seg_better(float ka, int ia, int pa, float kb, int ib, int pb) {
    return topk::better(ka, ia, kb, ib) || (ka == kb && ia == ib && pa < pb);
}

// A lane's sorted top-K of (value, id, position), best first; filler (-inf, INT_MAX, INT_MAX):
// a position is below INT_MAX, so every real entry is ahead of the filler.  TopList's insertion
// (the early test, then selects with static indices), with the position carried along.
template <int K>
struct SegList {
    float v[K];
    int id[K], pos[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < K; ++j) { v[j] = -INFINITY; id[j] = INT_MAX; pos[j] = INT_MAX; }
    }
    __device__ __forceinline__ void insert(float x, int xi, int xp) {
        float xk = topk::key_of(x);
        if (!seg_better(xk, xi, xp, topk::key_of(v[K - 1]), id[K - 1], pos[K - 1])) return;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float tv = v[j], tk = topk::key_of(tv);
            const int ti = id[j], tp = pos[j];
            const bool in = seg_better(xk, xi, xp, tk, ti, tp);
            v[j] = in ? x : tv;
            id[j] = in ? xi : ti;
            pos[j] = in ? xp : tp;
            x = in ? tv : x;
            xi = in ? ti : xi;
            xp = in ? tp : xp;
            xk = in ? tk : xk;
        }
    }
    // drop the head
    __device__ __forceinline__ void pop(bool take) {
#pragma unroll
        for (int j = 0; j + 1 < K; ++j) {
            v[j] = take ? v[j + 1] : v[j];
            id[j] = take ? id[j + 1] : id[j];
            pos[j] = take ? pos[j + 1] : pos[j];
        }
        v[K - 1] = take ? -INFINITY : v[K - 1];
        id[K - 1] = take ? INT_MAX : id[K - 1];
        pos[K - 1] = take ? INT_MAX : pos[K - 1];
    }
};

template <int K>
__global__ void __launch_bounds__(kSegWaves * kWave) seg_topk_kernel(const float *__restrict__ scores,
                                                                     const int64_t *__restrict__ list_ptr,
                                                                     const int32_t *__restrict__ list_idx, int64_t n,
                                                                     int k, int32_t *__restrict__ out_pos,
                                                                     float *__restrict__ out_val) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kSegWaves + threadIdx.x / kWave;
    if (r >= n) return;                                   // the whole wave: the waves share nothing
    const int64_t off = list_ptr[r];
    const int64_t len = list_ptr[r + 1] - off;            // <= INT_MAX (the entry's contract)
    SegList<K> best;
    best.init();
    for (int64_t c0 = 0; c0 < len; c0 += kSegUnroll * kWave) {
        float x[kSegUnroll];
        int xi[kSegUnroll];
#pragma unroll
        for (int j = 0; j < kSegUnroll; ++j) {
            const int64_t c = c0 + j * kWave + lane;
            x[j] = c < len ? scores[off + c] : 0.0f;
            xi[j] = c < len ? list_idx[off + c] : 0;
        }
#pragma unroll
        for (int j = 0; j < kSegUnroll; ++j) {
            const int64_t c = c0 + j * kWave + lane;
            if (c < len) best.insert(x[j], xi[j], (int)c);
        }
    }
    // k times the best head of the 64 lists; lane j keeps rank j (k <= 32 < 64)
    int rp = -1;
    float rv = -INFINITY;
    for (int j = 0; j < k; ++j) {
        float bv = best.v[0];
        int bi = best.id[0], bp = best.pos[0];
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o), op = __shfl_xor(bp, o);
            const bool take = seg_better(topk::key_of(ov), oi, op, topk::key_of(bv), bi, bp);
            bv = take ? ov : bv;
            bi = take ? oi : bi;
            bp = take ? op : bp;
        }
        // every lane holds the same winner (a total order; fillers are all equal); INT_MAX: none left
        const bool some = bp != INT_MAX;
        if (lane == j) {
            rp = some ? bp : -1;
            rv = some ? bv : -INFINITY;
        }
        best.pop(some && best.pos[0] == bp);
    }
    if (lane < k) {
        out_pos[r * k + lane] = rp;
        if (out_val) out_val[r * k + lane] = rv;
    }
}

__global__ void __launch_bounds__(kSegWaves * kWave) seg_rank_kernel(const float *__restrict__ scores,
                                                                     const int64_t *__restrict__ list_ptr,
                                                                     const int32_t *__restrict__ list_idx, int64_t n,
                                                                     int32_t *__restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kSegWaves + threadIdx.x / kWave;
    if (r >= n) return;
    const int64_t off = list_ptr[r];
    const int64_t len = list_ptr[r + 1] - off;
    if (len <= 0) {
        if (lane < 2) out[r * 2 + lane] = -1;
        return;
    }
    const float tk = topk::key_of(scores[off]);
    const int ti = list_idx[off];
    int above = 0, ahead = 0;
    for (int64_t c0 = 1; c0 < len; c0 += kSegUnroll * kWave) {
        float x[kSegUnroll];
        int xi[kSegUnroll];
#pragma unroll
        for (int j = 0; j < kSegUnroll; ++j) {
            const int64_t c = c0 + j * kWave + lane;
            x[j] = c < len ? scores[off + c] : 0.0f;
            xi[j] = c < len ? list_idx[off + c] : 0;
        }
#pragma unroll
        for (int j = 0; j < kSegUnroll; ++j) {
            const bool on = c0 + j * kWave + lane < len;
            const float xk = topk::key_of(x[j]);
            above += (on && xk > tk) ? 1 : 0;
            ahead += (on && xk == tk && xi[j] < ti) ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        above += __shfl_xor(above, o);
        ahead += __shfl_xor(ahead, o);
    }
    if (lane == 0) {
        out[r * 2] = above;
        out[r * 2 + 1] = ahead;
    }
}

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int rg_mf_score_lists(void *stream, const float *user_w, const float *item_w, const float *user_b,
                                 const float *item_b, int32_t dim, const int64_t *users_dev, const int64_t *list_ptr,
                                 const int32_t *list_idx, int64_t n, float *out) {
    if (!user_w || !item_w || !user_b || !item_b || !users_dev || !list_ptr || !list_idx || !out)
        return fail_arg("rg_mf_score_lists: null pointer");
    if (dim < 1 || dim > 256) return fail_arg("rg_mf_score_lists: dim must be in [1, 256]");
    if (n < 0) return fail_arg("rg_mf_score_lists: n < 0");
    if (n == 0) return RG_OK;
    const ScoreListArgs a{user_w, item_w, user_b, item_b, dim, users_dev, list_ptr, list_idx, n, out};
    const bool aligned = (((uintptr_t)item_w | (uintptr_t)user_w) & 15u) == 0;
    return dispatch_lists(dim, aligned, ScoreListLaunch{a, (hipStream_t)stream});
}

extern "C" int rg_seg_topk(void *stream, const float *scores, const int64_t *list_ptr, const int32_t *list_idx,
                           int64_t n, int32_t k, int32_t *out_pos, float *out_val) {
    if (!scores || !list_ptr || !list_idx || !out_pos) return fail_arg("rg_seg_topk: null pointer");
    if (k < 1 || k > topk::kTopkMax)
        return fail_arg("rg_seg_topk: k must be in [1, " + std::to_string(topk::kTopkMax) + "]");
    if (n < 0) return fail_arg("rg_seg_topk: n < 0");
    if (n == 0) return RG_OK;
    const int64_t blocks = (n + kSegWaves - 1) / kSegWaves;
    if (blocks > (int64_t)INT_MAX) return fail_arg("rg_seg_topk: too many lists for one launch");
    const dim3 grid((unsigned)blocks), block(kSegWaves * kWave);
    hipStream_t s = (hipStream_t)stream;
    if (k <= 8)
        hipLaunchKernelGGL(seg_topk_kernel<8>, grid, block, 0, s, scores, list_ptr, list_idx, n, (int)k, out_pos, out_val);
    else if (k <= 16)
        hipLaunchKernelGGL(seg_topk_kernel<16>, grid, block, 0, s, scores, list_ptr, list_idx, n, (int)k, out_pos, out_val);
    else
        hipLaunchKernelGGL(seg_topk_kernel<32>, grid, block, 0, s, scores, list_ptr, list_idx, n, (int)k, out_pos, out_val);
    return check_launch("rg_seg_topk");
}

extern "C" int rg_seg_rank(void *stream, const float *scores, const int64_t *list_ptr, const int32_t *list_idx,
                           int64_t n, int32_t *out) {
    if (!scores || !list_ptr || !list_idx || !out) return fail_arg("rg_seg_rank: null pointer");
    if (n < 0) return fail_arg("rg_seg_rank: n < 0");
    if (n == 0) return RG_OK;
    const int64_t blocks = (n + kSegWaves - 1) / kSegWaves;
    if (blocks > (int64_t)INT_MAX) return fail_arg("rg_seg_rank: too many lists for one launch");
    hipLaunchKernelGGL(seg_rank_kernel, dim3((unsigned)blocks), dim3(kSegWaves * kWave), 0, (hipStream_t)stream, scores,
                       list_ptr, list_idx, n, out);
    return check_launch("rg_seg_rank");
}
