// Diversified re-ranking of candidate lists (rg_seg_mmr, rg_seg_mean_sim): maximal marginal
// relevance inside each list of rg_cand.hip's CSR, and the mean pairwise similarity of a list (the
// intra-list similarity).  One launch per entry, no workspace, no atomics.
//
// Both kernels: one wave per list, one wave per workgroup.  Entry e of a list belongs to lane
// e % 64 (slot e / 64, at most 16 slots: RG_SEG_MMR_MAX_LEN entries).  The similarity of two
// entries is
//     dot = dot_rows(row of e, row of j)     one fmaf chain over the columns 0 .. dim - 1
//     sim = (dot * rnorm[id_e]) * rnorm[id_j]   or dot itself when rnorm is null
// and dot_rows is the only product code here: a lane walks its entry's row against the selected
// row, whichever memory the rows are in.  The rows of a list are gathered ONCE into LDS (row e at
// e * (dim | 1): the odd stride spreads the lanes' rows over the banks) when len * (dim | 1) floats
// fit the workgroup's stage -- stage_floats(dim), a size that depends on dim alone -- and read from
// the table (L2) at every step when they do not.  The values are the same, the chain is the same,
// so the bits do not depend on the path, the position, the list or the call.
//
// rg_seg_mmr: a chain of k dependent steps per list.  A lane keeps its entries' keys, ids, running
// penalties and reciprocal norms in registers (static slot indices; the slot count is a template
// argument picked per list from its length: 2, 4 or 16).  A step is: every lane's best unselected
// entry by (objective, id, position) -- rg_seg_topk's order on the objective -- a butterfly over
// the lanes for the list's best (a total order: every lane ends with the same winner), then ONE
// new product per unselected entry, against the winner's row, folded into the entry's penalty
// with fmaxf (a maximum does not depend on the order it is taken in).  Lane t keeps step t's
// result; the outputs are stored once, at the end.  Step 0's objective is the key, so it is
// rg_seg_topk's first entry; with lam == 1 the penalty is multiplied by zero at every step and
// the whole row is rg_seg_topk's.
//
// rg_seg_mean_sim: ids and reciprocal norms of the list in LDS (entries with id < 0 are skipped),
// for j ascending the lanes take the entries e > j, each lane adds its similarities in double in
// that fixed order (j ascending, e ascending), then a butterfly of the 64 partial sums and one
// division by the number of pairs.
#include "rg_common.h"
#include "rg_topk_lists.h"

#include <limits.h>

namespace rg {
namespace {

constexpr int kMaxLen = RG_SEG_MMR_MAX_LEN;
constexpr int kMaxStageFloats = 16 * 1024;      // 64 KiB: the most LDS a workgroup stages rows in
constexpr int kMinStageFloats = 4 * 1024;
constexpr int kStageLen = 128;                  // lists up to this length are staged at every dim that fits

// floats of LDS the rows of one list may take: kStageLen rows at this dim, within [16, 64] KiB
int stage_floats(int dim) {
    const int want = kStageLen * (dim | 1);
    return want < kMinStageFloats ? kMinStageFloats : want > kMaxStageFloats ? kMaxStageFloats : want;
}

// (key, id, position): rg_cand.hip's order
__device__ __forceinline__ bool seg_better(float ka, int ia, int pa, float kb, int ib, int pb) {
    return topk::better(ka, ia, kb, ib) || (ka == kb && ia == ib && pa < pb);
}

// the one product: an fmaf chain over the columns in ascending order
__device__ __forceinline__ float dot_rows(const float *__restrict__ a, const float *__restrict__ b, int dim) {
    float d = 0.0f;
    int c = 0;
    for (; c + 4 <= dim; c += 4) {
        const float a0 = a[c], a1 = a[c + 1], a2 = a[c + 2], a3 = a[c + 3];
        const float b0 = b[c], b1 = b[c + 1], b2 = b[c + 2], b3 = b[c + 3];
        d = fmaf(a0, b0, d);
        d = fmaf(a1, b1, d);
        d = fmaf(a2, b2, d);
        d = fmaf(a3, b3, d);
    }
    for (; c < dim; ++c) d = fmaf(a[c], b[c], d);
    return d;
}

__device__ __forceinline__ float sim_of(float dot, bool cosine, float re, float rj) {
    return cosine ? __fmul_rn(__fmul_rn(dot, re), rj) : dot;
}

// the rows of the list's first `len` entries into LDS, row e at e * stride; an entry with id < 0
// (rg_seg_mean_sim's skipped ones) leaves its row unwritten -- nothing reads it
__device__ __forceinline__ void stage_rows(float *__restrict__ smem, const float *__restrict__ table,
                                           const int32_t *__restrict__ ids, int len, int dim, int stride, int lane) {
    constexpr int kU = 4;
    const int total = len * dim;
    for (int f0 = 0; f0 < total; f0 += kU * kWave) {
        float v[kU];
        int at[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int f = f0 + u * kWave + lane;
            at[u] = -1;
            v[u] = 0.0f;
            if (f < total) {
                const int e = f / dim, c = f - e * dim;
                const int id = ids[e];
                if (id >= 0) {
                    at[u] = e * stride + c;
                    v[u] = table[(int64_t)id * dim + c];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (at[u] >= 0) smem[at[u]] = v[u];
    }
}

struct MmrArgs {
    const float *scores;
    const int64_t *list_ptr;
    const int32_t *list_idx;
    int64_t n;
    const float *table, *rnorm;
    int32_t dim;
    float lam, oml;         // lam and 1 - lam
    int32_t k, stage;       // stage: floats of LDS behind the kernel
    int32_t *out_pos;
    float *out_val, *out_pen;
};

template <int NS, bool STAGED>
__device__ __forceinline__ void mmr_list(const MmrArgs &a, int64_t r, int64_t off, int len, int lane, float *smem) {
    const int dim = a.dim;
    const int stride = STAGED ? (dim | 1) : dim;
    const float *__restrict__ rows = STAGED ? smem : a.table;
    const bool cosine = a.rnorm != nullptr;
    float key[NS], pen[NS], rn[NS];
    int id[NS];
    unsigned sel = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int e = s * kWave + lane;
        const bool on = e < len;
        key[s] = topk::key_of(on ? a.scores[off + e] : 0.0f);
        id[s] = on ? a.list_idx[off + e] : 0;
        pen[s] = -INFINITY;
        rn[s] = on && cosine ? a.rnorm[id[s]] : 0.0f;
    }
    if (STAGED) {
        stage_rows(smem, a.table, a.list_idx + off, len, dim, stride, lane);
        __syncthreads();        // one wave: orders the other lanes' LDS stores before this lane's loads
    }
    const int steps = a.k < len ? a.k : len;
    int rp = -1;
    float rpen = 0.0f;
    for (int t = 0; t < steps; ++t) {
        float bo = -INFINITY, bn = 0.0f;
        int bi = INT_MAX, bp = INT_MAX;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int e = s * kWave + lane;
            if (e < len && !((sel >> s) & 1u)) {
                const float kx = key[s];
                const float o = (t == 0 || isinf(kx)) ? kx : __fsub_rn(__fmul_rn(a.lam, kx), __fmul_rn(a.oml, pen[s]));
                if (seg_better(o, id[s], e, bo, bi, bp)) {
                    bo = o;
                    bi = id[s];
                    bp = e;
                    bn = pen[s];
                }
            }
        }
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const float oo = __shfl_xor(bo, o), on = __shfl_xor(bn, o);
            const int oi = __shfl_xor(bi, o), op = __shfl_xor(bp, o);
            const bool take = seg_better(oo, oi, op, bo, bi, bp);
            bo = take ? oo : bo;
            bn = take ? on : bn;
            bi = take ? oi : bi;
            bp = take ? op : bp;
        }
        // t < steps <= len: an unselected entry was left, so (bi, bp) is a real entry on every lane
        if (lane == t) {
            rp = bp;
            rpen = t == 0 ? 0.0f : bn;
        }
        if ((bp & (kWave - 1)) == lane) sel |= 1u << (bp >> 6);
        if (t + 1 == steps) break;
        const float rj = cosine ? a.rnorm[bi] : 0.0f;
        const float *__restrict__ pj = rows + (STAGED ? (int64_t)bp : (int64_t)bi) * stride;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int e = s * kWave + lane;
            if (e < len && !((sel >> s) & 1u)) {
                const float d = dot_rows(rows + (STAGED ? (int64_t)e : (int64_t)id[s]) * stride, pj, dim);
                pen[s] = fmaxf(pen[s], sim_of(d, cosine, rn[s], rj));
            }
        }
    }
    if (lane < a.k) {
        a.out_pos[r * a.k + lane] = rp;
        if (a.out_val) a.out_val[r * a.k + lane] = rp >= 0 ? a.scores[off + rp] : -INFINITY;
        if (a.out_pen) a.out_pen[r * a.k + lane] = rpen;
    }
}

__global__ void __launch_bounds__(kWave) seg_mmr_kernel(const MmrArgs a) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t off = a.list_ptr[r];
    const int64_t full = a.list_ptr[r + 1] - off;
    const int len = full > kMaxLen ? kMaxLen : full < 0 ? 0 : (int)full;      // never beyond the cap
    const bool staged = len * (a.dim | 1) <= a.stage;
    if (len <= 2 * kWave) {
        if (staged) mmr_list<2, true>(a, r, off, len, lane, smem);
        else mmr_list<2, false>(a, r, off, len, lane, smem);
    } else if (len <= 4 * kWave) {
        if (staged) mmr_list<4, true>(a, r, off, len, lane, smem);
        else mmr_list<4, false>(a, r, off, len, lane, smem);
    } else {
        if (staged) mmr_list<kMaxLen / kWave, true>(a, r, off, len, lane, smem);
        else mmr_list<kMaxLen / kWave, false>(a, r, off, len, lane, smem);
    }
}

struct MeanArgs {
    const int64_t *list_ptr;
    const int32_t *list_idx;
    int64_t n;
    const float *table, *rnorm;
    int32_t dim, stage;
    float *out;
};

template <bool STAGED>
__device__ __forceinline__ double mean_list(const MeanArgs &a, int len, int lane, const int *sid, const float *srn,
                                            float *srows) {
    const int dim = a.dim;
    const int stride = STAGED ? (dim | 1) : dim;
    const float *__restrict__ rows = STAGED ? srows : a.table;
    const bool cosine = a.rnorm != nullptr;
    double acc = 0.0;
    for (int j = 0; j + 1 < len; ++j) {
        const int idj = sid[j];
        if (idj < 0) continue;                              // the whole wave
        const float rj = srn[j];
        const float *__restrict__ pj = rows + (STAGED ? (int64_t)j : (int64_t)idj) * stride;
        for (int e = ((j + 1) & ~(kWave - 1)) + lane; e < len; e += kWave) {
            const int ide = sid[e];
            if (e > j && ide >= 0) {
                const float d = dot_rows(rows + (STAGED ? (int64_t)e : (int64_t)ide) * stride, pj, dim);
                acc += (double)sim_of(d, cosine, srn[e], rj);
            }
        }
    }
    return acc;
}

__global__ void __launch_bounds__(kWave) seg_mean_sim_kernel(const MeanArgs a) {
    extern __shared__ float smem[];
    int *sid = reinterpret_cast<int *>(smem);               // [kMaxLen] ids, then [kMaxLen] reciprocal norms
    float *srn = smem + kMaxLen;
    float *srows = smem + 2 * kMaxLen;
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t off = a.list_ptr[r];
    const int64_t full = a.list_ptr[r + 1] - off;
    const int len = full > kMaxLen ? kMaxLen : full < 0 ? 0 : (int)full;
    int mine = 0;
    for (int e = lane; e < len; e += kWave) {
        const int id = a.list_idx[off + e];
        sid[e] = id;
        srn[e] = id >= 0 && a.rnorm ? a.rnorm[id] : 0.0f;
        mine += id >= 0 ? 1 : 0;
    }
    const bool staged = len * (a.dim | 1) <= a.stage;
    if (staged) stage_rows(srows, a.table, a.list_idx + off, len, a.dim, a.dim | 1, lane);
    __syncthreads();
    double acc = staged ? mean_list<true>(a, len, lane, sid, srn, srows) : mean_list<false>(a, len, lane, sid, srn, srows);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        acc += __shfl_xor(acc, o);                          // a value and its partner's: they commute exactly
        mine += __shfl_xor(mine, o);
    }
    if (lane == 0) {
        const double pairs = 0.5 * (double)mine * (double)(mine - 1);
        a.out[r] = mine < 2 ? 0.0f : (float)(acc / pairs);
    }
}

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int rg_seg_mmr(void *stream, const float *scores, const int64_t *list_ptr, const int32_t *list_idx,
                          int64_t n, const float *table, const float *rnorm, int32_t dim, float lam, int32_t k,
                          int32_t *out_pos, float *out_val, float *out_pen) {
    if (!scores || !list_ptr || !list_idx || !table || !out_pos) return fail_arg("rg_seg_mmr: null pointer");
    if (dim < 1 || dim > 256) return fail_arg("rg_seg_mmr: dim must be in [1, 256]");
    if (k < 1 || k > RG_SEG_MMR_MAX_K)
        return fail_arg("rg_seg_mmr: k must be in [1, " + std::to_string(RG_SEG_MMR_MAX_K) + "]");
    if (!(lam > 0.0f && lam <= 1.0f)) return fail_arg("rg_seg_mmr: lam must be in (0, 1]");
    if (n < 0) return fail_arg("rg_seg_mmr: n < 0");
    if (n == 0) return RG_OK;
    if (n > (int64_t)INT_MAX) return fail_arg("rg_seg_mmr: too many lists for one launch");
    const int stage = stage_floats(dim);
    const MmrArgs a{scores, list_ptr, list_idx, n, table, rnorm, dim, lam, 1.0f - lam, k, stage, out_pos, out_val, out_pen};
    hipLaunchKernelGGL(seg_mmr_kernel, dim3((unsigned)n), dim3(kWave), (size_t)stage * sizeof(float),
                       (hipStream_t)stream, a);
    return check_launch("rg_seg_mmr");
}

extern "C" int rg_seg_mean_sim(void *stream, const int64_t *list_ptr, const int32_t *list_idx, int64_t n,
                               const float *table, const float *rnorm, int32_t dim, float *out) {
    if (!list_ptr || !list_idx || !table || !out) return fail_arg("rg_seg_mean_sim: null pointer");
    if (dim < 1 || dim > 256) return fail_arg("rg_seg_mean_sim: dim must be in [1, 256]");
    if (n < 0) return fail_arg("rg_seg_mean_sim: n < 0");
    if (n == 0) return RG_OK;
    if (n > (int64_t)INT_MAX) return fail_arg("rg_seg_mean_sim: too many lists for one launch");
    // the ids and reciprocal norms take 2 * kMaxLen words of the workgroup's 64 KiB
    int stage = stage_floats(dim);
    if (stage > kMaxStageFloats - 2 * kMaxLen) stage = kMaxStageFloats - 2 * kMaxLen;
    const MeanArgs a{list_ptr, list_idx, n, table, rnorm, dim, stage, out};
    hipLaunchKernelGGL(seg_mean_sim_kernel, dim3((unsigned)n), dim3(kWave), (size_t)(stage + 2 * kMaxLen) * sizeof(float),
                       (hipStream_t)stream, a);
    return check_launch("rg_seg_mean_sim");
}
