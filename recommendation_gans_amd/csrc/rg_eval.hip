// Top-k item ranking for the evaluation metrics (spotlight/evaluation.py:108-185,
// 192-213, 278-353: precision/recall@k, hit ratio and MAP@k read only the first k
// entries of each user's ranking, argsort(-scores)).
//
// One workgroup per user row: every thread keeps a sorted top-K of its strided slice
// of the row in registers (rg_topk_lists.h's TopList, K <= kTopkMax), the 256 lists are
// merged in LDS by its merge_tree, and the row's k best item ids are written in rank
// order.  Order: higher score first, then the lower item id (numpy's default argsort
// leaves the order of equal scores unspecified; for distinct scores the ranking is
// the reference's).  Only users x k ids leave the device instead of the users x items
// score block.
#include <cfloat>
#include <climits>

#include "rg_common.h"
#include "rg_topk_lists.h"

namespace rg {
namespace {

using topk::kTopkMax;
constexpr int kTopkThreads = 256;

template <int K>
__global__ __launch_bounds__(kTopkThreads) void topk_kernel(const float *__restrict__ scores, int64_t cols, int64_t ld,
                                                            int k, int32_t *__restrict__ out) {
    __shared__ float sv[kTopkThreads * K];
    __shared__ int si[kTopkThreads * K];
    const int tid = threadIdx.x;
    const float *row = scores + (int64_t)blockIdx.x * ld;
    // only ids leave, so the lists carry a NaN's key (-inf) in the NaN's place: nothing in them is a NaN
    topk::TopList<K, false> top;
    top.init();
    for (int64_t c = tid; c < cols; c += kTopkThreads) top.insert(topk::key_of(row[c]), (int)c);
    top.store(sv + tid * K, si + tid * K);
    __syncthreads();
    topk::merge_tree<K, kTopkThreads, false>(sv, si, tid);
    if (tid < k) out[(int64_t)blockIdx.x * k + tid] = si[tid];
}

// ---------------------------------------------------------------- rank of given items
// mrr_score (spotlight/evaluation.py:13-60) ranks every item of a user (scipy rankdata of
// -score, ties averaged, train items at FLOAT_MAX) and reads the ranks of the test items.
// The average-tie rank of a target t is above(t) + (equal(t) + 1) / 2, above = the items
// ranked strictly ahead of t, equal = the items tied with it (t included): two integer
// counts per target, no sort.
//
// One workgroup per row.  The row's excluded ids are set in an LDS bitmap, one bit per
// column (a duplicate id sets the same bit again; an id outside [0, cols) is skipped).
// The targets are taken kRankChunk at a time: their keys are held in registers, every
// thread walks its strided slice of the row once per chunk and counts, per target, the
// keys above and equal; the counts are summed over the wave by shuffles and over the
// waves through LDS.  The row is re-read from L2 for each further chunk (targets x cols
// compares per row, small next to producing the scores).
constexpr int kRankThreads = 256;
constexpr int kRankWaves = kRankThreads / kWave;
constexpr int kRankChunk = RG_RANK_CHUNK;

// key of column c: excluded -> -FLT_MAX (the reference's FLOAT_MAX on -score), NaN -> -inf
template <bool EXC>
__device__ __forceinline__ float rank_key(float x, int c, const uint32_t *bits) {
    if (x != x) x = -INFINITY;
    if (EXC && ((bits[c >> 5] >> (c & 31)) & 1u)) x = -FLT_MAX;
    return x;
}

template <bool EXC>
__global__ __launch_bounds__(kRankThreads) void rank_kernel(const float *__restrict__ scores, int cols, int64_t ld,
                                                            const int64_t *__restrict__ tgt_ptr,
                                                            const int32_t *__restrict__ tgt_idx,
                                                            const int64_t *__restrict__ exc_ptr,
                                                            const int32_t *__restrict__ exc_idx,
                                                            int32_t *__restrict__ out_above,
                                                            int32_t *__restrict__ out_equal) {
    extern __shared__ uint32_t bits[];               // EXC: [(cols + 31) / 32]
    __shared__ float tkey[kRankChunk];
    __shared__ int part[kRankWaves][2 * kRankChunk];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t r = blockIdx.x;
    const int64_t t0 = tgt_ptr[r], t1 = tgt_ptr[r + 1];
    if (t1 <= t0) return;                            // the whole workgroup: no barrier is skipped
    const float *row = scores + r * ld;
    if (EXC) {
        for (int w = tid; w < (cols + 31) / 32; w += kRankThreads) bits[w] = 0u;
        __syncthreads();
        const int64_t e1 = exc_ptr[r + 1];
        for (int64_t e = exc_ptr[r] + tid; e < e1; e += kRankThreads) {
            const int id = exc_idx[e];
            if (id >= 0 && id < cols) atomicOr(&bits[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
    }
    for (int64_t c0 = t0; c0 < t1; c0 += kRankChunk) {
        const int n = (int)(t1 - c0 < kRankChunk ? t1 - c0 : kRankChunk);
        // target id of this thread's slot; an id outside [0, cols) is never used as an index
        const int my = tid < n ? tgt_idx[c0 + tid] : -1;
        const bool my_ok = my >= 0 && my < cols;
        if (tid < kRankChunk) tkey[tid] = my_ok ? rank_key<EXC>(row[my], my, bits) : NAN;   // NaN key: counts 0
        __syncthreads();
        float k[kRankChunk];
        int above[kRankChunk], equal[kRankChunk];
#pragma unroll
        for (int j = 0; j < kRankChunk; ++j) { k[j] = tkey[j]; above[j] = 0; equal[j] = 0; }
#pragma unroll 4
        for (int c = tid; c < cols; c += kRankThreads) {
            const float x = rank_key<EXC>(row[c], c, bits);
#pragma unroll
            for (int j = 0; j < kRankChunk; ++j) {
                above[j] += x > k[j] ? 1 : 0;
                equal[j] += x == k[j] ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < kRankChunk; ++j) {
            int a = above[j], q = equal[j];
            for (int o = kWave / 2; o; o >>= 1) { a += __shfl_xor(a, o); q += __shfl_xor(q, o); }
            if (lane == 0) { part[wave][j] = a; part[wave][kRankChunk + j] = q; }
        }
        __syncthreads();
        if (tid < n) {
            int a = 0, q = 0;
            for (int w = 0; w < kRankWaves; ++w) { a += part[w][tid]; q += part[w][kRankChunk + tid]; }
            out_above[c0 + tid] = my_ok ? a : -1;
            out_equal[c0 + tid] = my_ok ? q : 0;
        }
    }
}

template <bool EXC>
int rank_launch(hipStream_t s, const float *scores, int64_t rows, int cols, int64_t ld, const int64_t *tgt_ptr,
                const int32_t *tgt_idx, const int64_t *exc_ptr, const int32_t *exc_idx, int32_t *out_above,
                int32_t *out_equal) {
    const size_t lds = EXC ? (size_t)((cols + 31) / 32) * sizeof(uint32_t) : 0;
    if (EXC) {
        static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void *>(rank_kernel<EXC>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     RG_RANK_MAX_COLS / 8) == hipSuccess;
        if (!attr) return fail_arg("rg_rank_rows: cannot reserve LDS");
    }
    hipLaunchKernelGGL((rank_kernel<EXC>), dim3((unsigned)rows), dim3(kRankThreads), lds, s, scores, cols, ld, tgt_ptr,
                       tgt_idx, exc_ptr, exc_idx, out_above, out_equal);
    return check_launch("rg_rank_rows");
}

// ---------------------------------------------------------------- slate hits
// precision / recall of a generated slate (spotlight/evaluation.py:355-382) read one number
// per user: |set(slate[:k]) & set(targets)|.  It is the popcount of a k-bit word: bit j is set
// when slate position j holds one of the row's targets and no earlier position holds the same
// item.
//
// One wave per row, kHitsRows rows per workgroup.  Lane j < k loads slate position j; the k
// ids are then read into scalar registers (readlane with constant lane numbers).  The lanes
// stride over the row's targets, each compares its target with the k ids and ORs the matches
// into its own word; the words are OR-ed over the wave by shuffles.  Lane j also finds whether
// an earlier position holds its id, and a ballot gives those positions as a mask.  No LDS,
// atomics or barriers, so a wave whose row is past the end or has no targets leaves early.
constexpr int kHitsThreads = 256;
constexpr int kHitsRows = RG_SLATE_HITS_ROWS_PER_BLOCK;
constexpr int kHitsMaxK = 32;
static_assert(kHitsRows * kWave == kHitsThreads, "one wave per row");

template <int K>
__global__ __launch_bounds__(kHitsThreads) void slate_hits_kernel(const int32_t *__restrict__ slates, int64_t rows,
                                                                  int64_t ld, int k,
                                                                  const int64_t *__restrict__ tgt_ptr,
                                                                  const int32_t *__restrict__ tgt_idx,
                                                                  uint32_t *__restrict__ out_mask) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kHitsRows + __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    if (r >= rows) return;
    const int64_t t0 = tgt_ptr[r], t1 = tgt_ptr[r + 1];
    if (t1 <= t0) {
        if (lane == 0) out_mask[r] = 0u;
        return;
    }
    // positions [k, K) read as 0: whatever they match is cleared by the k-bit mask at the end
    const int sid = lane < k ? slates[r * ld + lane] : 0;
    int s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = __builtin_amdgcn_readlane(sid, j);
    uint32_t m = 0u;
    for (int64_t e = t0 + lane; e < t1; e += kWave) {
        const int t = tgt_idx[e];
#pragma unroll
        for (int j = 0; j < K; ++j) m |= (t == s[j] ? 1u : 0u) << j;
    }
    for (int o = kWave / 2; o; o >>= 1) m |= __shfl_xor(m, o);
    bool dup = false;
#pragma unroll
    for (int j = 0; j < K; ++j) dup |= j < lane && s[j] == sid;
    const uint32_t dups = (uint32_t)__ballot(dup);      // bit j: an earlier position holds position j's item
    if (lane == 0) out_mask[r] = m & ~dups & (k >= 32 ? 0xffffffffu : (1u << k) - 1u);
}

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int rg_topk_rows(void *stream, const float *scores, int64_t rows, int64_t cols, int64_t ld, int32_t k,
                            int32_t *out_idx) {
    if (!scores || !out_idx) return fail_arg("rg_topk_rows: null argument");
    if (rows < 0 || cols < 1 || ld < cols) return fail_arg("rg_topk_rows: bad shape");
    if (k < 1 || k > kTopkMax || k > cols) return fail_arg("rg_topk_rows: k must be in [1, min(32, cols)]");
    if (cols > INT_MAX) return fail_arg("rg_topk_rows: cols must fit int32");
    if (rows == 0) return RG_OK;
    if (rows > INT_MAX) return fail_arg("rg_topk_rows: too many rows for one launch");
    const dim3 grid((unsigned)rows), block(kTopkThreads);
    const hipStream_t s = (hipStream_t)stream;
    if (k <= 8)
        hipLaunchKernelGGL((topk_kernel<8>), grid, block, 0, s, scores, cols, ld, k, out_idx);
    else if (k <= 16)
        hipLaunchKernelGGL((topk_kernel<16>), grid, block, 0, s, scores, cols, ld, k, out_idx);
    else
        hipLaunchKernelGGL((topk_kernel<32>), grid, block, 0, s, scores, cols, ld, k, out_idx);
    return check_launch("rg_topk_rows");
}

extern "C" int rg_rank_rows(void *stream, const float *scores, int64_t rows, int64_t cols, int64_t ld,
                            const int64_t *tgt_ptr, const int32_t *tgt_idx, const int64_t *exc_ptr,
                            const int32_t *exc_idx, int32_t *out_above, int32_t *out_equal) {
    if (!scores || !tgt_ptr || !tgt_idx || !out_above || !out_equal) return fail_arg("rg_rank_rows: null argument");
    if ((exc_ptr == nullptr) != (exc_idx == nullptr))
        return fail_arg("rg_rank_rows: exc_ptr and exc_idx must both be given or both be null");
    if (rows < 0 || cols < 1 || ld < cols) return fail_arg("rg_rank_rows: bad shape");
    if (cols > INT_MAX) return fail_arg("rg_rank_rows: cols must fit int32");
    if (cols > RG_RANK_MAX_COLS)
        return fail_arg("rg_rank_rows: cols above RG_RANK_MAX_COLS (" + std::to_string(RG_RANK_MAX_COLS) + ")");
    if (rows == 0) return RG_OK;
    if (rows > INT_MAX) return fail_arg("rg_rank_rows: too many rows for one launch");
    const hipStream_t s = (hipStream_t)stream;
    if (exc_ptr)
        return rank_launch<true>(s, scores, rows, (int)cols, ld, tgt_ptr, tgt_idx, exc_ptr, exc_idx, out_above,
                                 out_equal);
    return rank_launch<false>(s, scores, rows, (int)cols, ld, tgt_ptr, tgt_idx, nullptr, nullptr, out_above, out_equal);
}

extern "C" int rg_slate_hits(void *stream, const int32_t *slates, int64_t rows, int32_t slate_size, int64_t ld,
                             int32_t k, const int64_t *tgt_ptr, const int32_t *tgt_idx, uint32_t *out_mask) {
    if (!slates || !tgt_ptr || !tgt_idx || !out_mask) return fail_arg("rg_slate_hits: null argument");
    if (rows < 0 || slate_size < 1 || ld < slate_size) return fail_arg("rg_slate_hits: bad shape");
    if (k < 1 || k > kHitsMaxK || k > slate_size)
        return fail_arg("rg_slate_hits: k must be in [1, min(32, slate_size)]");
    if (rows > (int64_t)INT_MAX * kHitsRows) return fail_arg("rg_slate_hits: too many rows for one launch");
    if (rows == 0) return RG_OK;
    const dim3 grid((unsigned)((rows + kHitsRows - 1) / kHitsRows)), block(kHitsThreads);
    const hipStream_t s = (hipStream_t)stream;
    if (k <= 8)
        hipLaunchKernelGGL((slate_hits_kernel<8>), grid, block, 0, s, slates, rows, ld, k, tgt_ptr, tgt_idx, out_mask);
    else if (k <= 16)
        hipLaunchKernelGGL((slate_hits_kernel<16>), grid, block, 0, s, slates, rows, ld, k, tgt_ptr, tgt_idx, out_mask);
    else
        hipLaunchKernelGGL((slate_hits_kernel<32>), grid, block, 0, s, slates, rows, ld, k, tgt_ptr, tgt_idx, out_mask);
    return check_launch("rg_slate_hits");
}
