// Implicit ALS (rg_als_gram, rg_als_solve_rows): one half-step of confidence-weighted alternating
// least squares (Hu, Koren, Volinsky 2008) on a pair of MF tables, by conjugate gradients per row.
//
// For a row with list N (a CSR row, duplicates as given), values v_i (1 when row_val is null),
// c_i = 1 + alpha v_i and G = Y^T Y + lam I (rg_als_gram of the other table Y):
//     A = G + sum_{i in N} (c_i - 1) y_i y_i^T          b = sum_{i in N} c_i y_i
// and cg_steps iterations of CG on A x = b from the row's current x (include/rg_hip.h has the
// iteration).  A is never formed: A p = G p + sum_i (c_i - 1) (y_i . p) y_i, one gather pass over
// the list per product -- cg_steps + 1 passes for the step, one more for loss_out.
//
// Two paths, chosen per row by the length of its list alone (rg_als_long_row_len()):
//  * short (als_short_kernel): a row is owned by one group of L::LPU lanes (the pair kernel's lane
//    x float4 layout, rg_common.h) for all passes, 64 / LPU rows per wave; x, r, p and A p stay in
//    registers.  G is staged once per workgroup in LDS (dim^2 floats, 64 KB at dim 128) and the
//    workgroups stride over the call's rows, so it is staged once per compute-unit slot, not once
//    per row.  G p: the group writes p to its LDS slot and every lane walks j = 0 .. dim - 1 with
//    p_j (a broadcast read) and its own elements of G's row j -- G is symmetric, so row j at the
//    lane's columns is column j at the lane's rows, and a VEC lane reads them as one 16-byte word.
//  * long (als_long_kernel): one workgroup of kLongWaves waves per row.  Its NG = kLongWaves * 64 /
//    LPU lane groups each take one contiguous chunk of ceil(len / NG) entries, their partial sums
//    meet in LDS and EVERY group adds the NG partials in the order 0 .. NG - 1: all groups then hold
//    the same x, r, p, bit for bit, and go on redundantly (no second broadcast).
// Order of a row's sums: inside a chunk (short: the whole list is one chunk) entry e goes to sum
// e % 4 in ascending order and the four sums are added as a tree, then the chunks ascending; the
// lane reduction is the same butterfly in every group; the wave loops to its longest row and masks
// with selects.  So a row's bits depend on its own list, values, start and
// G alone -- not on its place in the call, the number of rows or the other rows.  No atomics.
// The layout dispatch (dispatch_rows, capped at dim 128), the dots (row_dot) and wave_max64 are the
// row-group helpers of rg_common.h; the launch, with its dynamic LDS and strided grids, is its own.
//
// rg_als_gram: blocks of kGramRows rows each write a [dim][dim] partial (an 8 x 8 register tile per
// thread, the rows staged through LDS kGramTile at a time: a tile's rows summed in ascending order,
// the tiles' sums added in ascending order), and a
// second kernel adds the partials in ascending block order and lam on the diagonal: the same bits
// every run, and G[i][j] == G[j][i] bit for bit (fmaf(a, b, s) == fmaf(b, a, s)).
#include "rg_common.h"

#include <limits.h>

namespace rg {
namespace {

constexpr int kMaxDim = 128;
constexpr int kLongRowLen = 256;   // lists this long or longer take a workgroup
constexpr int kKB = 4;             // list entries in flight per lane group
constexpr int kShortWaves = 8;
constexpr int kLongWaves = 8;
constexpr int kLdsMax = 96 * 1024;
constexpr int kLdsCu = 160 * 1024;  // LDS of a compute unit

constexpr int kGramRows = 1024;    // rows per partial
constexpr int kGramTile = 16;      // rows staged at once
constexpr int kGramThreads = 256;  // 16 x 16 threads, an 8 x 8 tile of G each

struct AlsArgs {
    const float *Y, *G;
    int32_t dim;
    const int64_t *ptr;
    const int32_t *idx;
    const float *val;
    float alpha;
    const int64_t *rows;
    int64_t n_rows;
    int32_t steps;
    float *X, *loss_out;
};

// One pass over entries [lo, lo + cnt) of the list, the wave looping to max_cnt (wave-uniform):
//   MODE 0: acc = sum (c_i - 1) (y_i . v) y_i and bs = sum c_i y_i
//   MODE 1: acc alone
//   MODE 2: ls = sum ((c_i - 1) s^2 - 2 c_i s + c_i), s = y_i . v
template <class L, int MODE>
__device__ __forceinline__ void gather_pass(const AlsArgs &a, int sub, int64_t lo, int64_t cnt, int64_t max_cnt,
                                            const float (&v)[L::EPL], float (&acc)[L::EPL], float (&bs)[L::EPL],
                                            float &ls) {
    constexpr int EPL = L::EPL;
    const int D = a.dim;
    // kKB interleaved sums (entry e of the chunk goes to sum e % kKB), added as a tree at the end:
    // chains a quarter as long for the rounding, and kKB independent ones for the pipeline
    float au[kKB][EPL], bu[kKB][EPL], lu[kKB];
#pragma unroll
    for (int u = 0; u < kKB; ++u) {
        L::zero(au[u]);
        L::zero(bu[u]);
        lu[u] = 0.0f;
    }
    for (int64_t e0 = 0; e0 < max_cnt; e0 += kKB) {
        bool ok[kKB];
        int id[kKB];
        float c1[kKB];
#pragma unroll
        for (int u = 0; u < kKB; ++u) {
            ok[u] = e0 + u < cnt;
            id[u] = ok[u] ? a.idx[lo + e0 + u] : 0;
            c1[u] = ok[u] ? a.alpha * (a.val != nullptr ? a.val[lo + e0 + u] : 1.0f) : 0.0f;
        }
        float y[kKB][EPL];
#pragma unroll
        for (int u = 0; u < kKB; ++u) L::load(y[u], a.Y, id[u], D, sub);
#pragma unroll
        for (int u = 0; u < kKB; ++u) {
            const float s = row_dot<L>(y[u], v);
            const float c = 1.0f + c1[u];
            if (MODE != 2) {
                const float t = c1[u] * s;
#pragma unroll
                for (int e = 0; e < EPL; ++e) au[u][e] = ok[u] ? fmaf(t, y[u][e], au[u][e]) : au[u][e];
            }
            if (MODE == 0) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) bu[u][e] = ok[u] ? fmaf(c, y[u][e], bu[u][e]) : bu[u][e];
            }
            if (MODE == 2) {
                const float term = fmaf(c1[u] * s, s, fmaf(-2.0f * c, s, c));
                lu[u] = ok[u] ? lu[u] + term : lu[u];
            }
        }
    }
    static_assert(kKB == 4, "the tree below adds four sums");
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        acc[e] = (au[0][e] + au[1][e]) + (au[2][e] + au[3][e]);
        if (MODE == 0) bs[e] = (bu[0][e] + bu[1][e]) + (bu[2][e] + bu[3][e]);
    }
    ls = (lu[0] + lu[1]) + (lu[2] + lu[3]);
}

// out = G v for the group's row: v goes through the group's LDS slot ps [LPU * EPL]
template <class L>
__device__ __forceinline__ void g_times(const float *Gs, float *ps, int D, int sub, const float (&v)[L::EPL],
                                        float (&out)[L::EPL]) {
    constexpr int EPL = L::EPL;
#pragma unroll
    for (int e = 0; e < EPL; ++e) ps[L::elem(sub, e)] = v[e];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // four interleaved sums over j (j % 4), added as a tree: chains of dim / 4 additions
    float o4[4][EPL];
#pragma unroll
    for (int q = 0; q < 4; ++q) L::zero(o4[q]);
    for (int j0 = 0; j0 < D; j0 += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + q;
            const bool in = j < D;
            const float pj = in ? ps[j] : 0.0f;
            if constexpr (L::VEC) {        // D is a multiple of 4: j is always inside
                const float4 g = *reinterpret_cast<const float4 *>(Gs + j * D + sub * 4);
                o4[q][0] = fmaf(g.x, pj, o4[q][0]);
                o4[q][1] = fmaf(g.y, pj, o4[q][1]);
                o4[q][2] = fmaf(g.z, pj, o4[q][2]);
                o4[q][3] = fmaf(g.w, pj, o4[q][3]);
            } else {
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int c = sub + L::LPU * e;
                    const float g = (in && c < D) ? Gs[j * D + c] : 0.0f;
                    o4[q][e] = fmaf(g, pj, o4[q][e]);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) out[e] = (o4[0][e] + o4[1][e]) + (o4[2][e] + o4[3][e]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();      // the slot is rewritten by the next product
}

// long path: the groups' partial vectors (and scalars) added in group order by every group
template <class L, int NG, bool WITH_B>
__device__ __forceinline__ void reduce_groups(float *red_a, float *red_b, int gid, int sub, float (&acc)[L::EPL],
                                              float (&bs)[L::EPL]) {
    constexpr int EPL = L::EPL, DP = L::LPU * L::EPL;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        red_a[gid * DP + L::elem(sub, e)] = acc[e];
        if (WITH_B) red_b[gid * DP + L::elem(sub, e)] = bs[e];
    }
    __syncthreads();
    L::zero(acc);
    if (WITH_B) L::zero(bs);
#pragma unroll 2
    for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            acc[e] += red_a[g * DP + L::elem(sub, e)];
            if (WITH_B) bs[e] += red_b[g * DP + L::elem(sub, e)];
        }
    }
    __syncthreads();
}

template <int NG>
__device__ __forceinline__ float reduce_scalar(float *red_s, int gid, int sub, float v) {
    if (sub == 0) red_s[gid] = v;
    __syncthreads();
    float s = 0.0f;
#pragma unroll 4
    for (int g = 0; g < NG; ++g) s += red_s[g];
    __syncthreads();
    return s;
}

// The half-step of one row per lane group (short) or of one row by every group of the workgroup
// (LONG: [lo, lo + cnt) is the group's chunk, `red` the reduction scratch, gid the group's number).
// act: the group has a row to solve; every lane of the wave runs every instruction.
template <class L, bool LONG, int NG>
__device__ __forceinline__ void als_row(const AlsArgs &a, const float *Gs, float *ps, float *red, int sub, int gid,
                                        int64_t row, int64_t lo, int64_t cnt, int64_t max_cnt, bool act) {
    constexpr int EPL = L::EPL, DP = L::LPU * L::EPL;
    const int D = a.dim;
    float *red_a = red, *red_b = red + NG * DP, *red_s = red + 2 * NG * DP;
    float x[EPL], r[EPL], p[EPL], ap[EPL], acc[EPL], bs[EPL];
    float ls;
    L::zero(x);
    if (act) L::load(x, a.X, row, D, sub);

    if (a.steps > 0) {
        gather_pass<L, 0>(a, sub, lo, cnt, max_cnt, x, acc, bs, ls);
        if (LONG) reduce_groups<L, NG, true>(red_a, red_b, gid, sub, acc, bs);
        g_times<L>(Gs, ps, D, sub, x, ap);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            r[e] = bs[e] - (ap[e] + acc[e]);
            p[e] = r[e];
        }
        float rs = row_dot<L>(r, r);
        bool go = act;
        for (int it = 0; it < a.steps; ++it) {
            go = go && rs != 0.0f;
            if (__ballot(go) == 0) break;      // LONG: every group holds the same values, so all waves agree
            gather_pass<L, 1>(a, sub, lo, cnt, max_cnt, p, acc, bs, ls);
            if (LONG) reduce_groups<L, NG, false>(red_a, red_b, gid, sub, acc, bs);
            g_times<L>(Gs, ps, D, sub, p, ap);
#pragma unroll
            for (int e = 0; e < EPL; ++e) ap[e] += acc[e];
            const float pap = row_dot<L>(p, ap);
            go = go && pap > 0.0f;
            const float al = rs / pap;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                x[e] = go ? fmaf(al, p[e], x[e]) : x[e];
                r[e] = go ? fmaf(-al, ap[e], r[e]) : r[e];
            }
            const float rn = row_dot<L>(r, r);
            const float beta = rn / rs;
#pragma unroll
            for (int e = 0; e < EPL; ++e) p[e] = go ? fmaf(beta, p[e], r[e]) : p[e];
            rs = go ? rn : rs;
        }
        if (act && (!LONG || gid == 0)) L::store(a.X, row, D, sub, x);
    }

    if (a.loss_out != nullptr) {
        gather_pass<L, 2>(a, sub, lo, cnt, max_cnt, x, acc, bs, ls);
        if (LONG) ls = reduce_scalar<NG>(red_s, gid, sub, ls);
        g_times<L>(Gs, ps, D, sub, x, ap);
        const float q = row_dot<L>(x, ap);
        if (act && sub == 0 && (!LONG || gid == 0)) a.loss_out[row] = q + ls;
    }
}

__device__ __forceinline__ void stage_g(float *Gs, const float *G, int D) {
    for (int q = threadIdx.x; q < D * D; q += blockDim.x) Gs[q] = G[q];
    __syncthreads();
}

__host__ __device__ constexpr int round4(int n) { return (n + 3) & ~3; }

template <class L>
__global__ void __launch_bounds__(kShortWaves *kWave) als_short_kernel(const AlsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LPU = L::LPU, EPL = L::EPL, UPW = L::UPW, DP = LPU * EPL;
    const int D = a.dim;
    float *Gs = lds;
    stage_g(Gs, a.G, D);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int sub = lane & (LPU - 1), grp = lane / LPU;
    float *ps = lds + round4(D * D) + (wave * UPW + grp) * DP;
    const int64_t tiles = (a.n_rows + UPW - 1) / UPW;      // a tile: the rows of one wave
    for (int64_t t = (int64_t)blockIdx.x * kShortWaves + wave; t < tiles; t += (int64_t)gridDim.x * kShortWaves) {
        const int64_t k = t * UPW + grp;
        const bool in = k < a.n_rows;
        const int64_t row = in ? (a.rows != nullptr ? a.rows[k] : k) : 0;
        const int64_t off = in ? a.ptr[row] : 0;
        const int64_t len = in ? a.ptr[row + 1] - off : 0;
        const bool mine = in && len < kLongRowLen;        // the long rows are the other kernel's
        const bool act = mine && len > 0;
        if (mine && len == 0) {                            // the exact solve of an empty row
            float z[EPL];
            L::zero(z);
            L::store(a.X, row, D, sub, z);
            if (sub == 0 && a.loss_out != nullptr) a.loss_out[row] = 0.0f;
        }
        const int64_t cnt = act ? len : 0;
        const int64_t max_cnt = wave_max64(cnt);
        if (max_cnt == 0) continue;
        als_row<L, false, 1>(a, Gs, ps, nullptr, sub, 0, row, off, cnt, max_cnt, act);
    }
}

template <class L>
__global__ void __launch_bounds__(kLongWaves *kWave) als_long_kernel(const AlsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LPU = L::LPU, EPL = L::EPL, UPW = L::UPW, DP = LPU * EPL, NG = kLongWaves * UPW;
    const int D = a.dim;
    float *Gs = lds;
    stage_g(Gs, a.G, D);
    const int gid = threadIdx.x / LPU, sub = threadIdx.x & (LPU - 1);
    float *ps = lds + round4(D * D) + gid * DP;
    float *red = lds + round4(D * D) + NG * DP;
    for (int64_t k = blockIdx.x; k < a.n_rows; k += gridDim.x) {
        const int64_t row = a.rows != nullptr ? a.rows[k] : k;
        const int64_t off = a.ptr[row];
        const int64_t len = a.ptr[row + 1] - off;
        if (len < kLongRowLen) continue;                   // the same for every thread of the workgroup
        const int64_t chunk = (len + NG - 1) / NG;
        const int64_t lo = (int64_t)gid * chunk < len ? (int64_t)gid * chunk : len;
        const int64_t cnt = lo + chunk < len ? chunk : len - lo;
        als_row<L, true, NG>(a, Gs, ps, red, sub, gid, row, off + lo, cnt, chunk, true);
    }
}

// floats of dynamic LDS of the two kernels for layout L at dim D
template <class L>
constexpr size_t short_lds(int D) {
    return (size_t)round4(D * D) + (size_t)kShortWaves * kWave * L::EPL;
}
template <class L>
constexpr size_t long_lds(int D) {
    return (size_t)round4(D * D) + (size_t)3 * kLongWaves * kWave * L::EPL + (size_t)kLongWaves * L::UPW;
}

struct AlsLaunch {
    const AlsArgs &a;
    hipStream_t stream;
    template <class L>
    int operator()() const {
        static const bool attr =
            hipFuncSetAttribute(reinterpret_cast<const void *>(als_short_kernel<L>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void *>(als_long_kernel<L>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax) == hipSuccess;
        if (!attr) return fail_arg("rg_als_solve_rows: cannot reserve LDS");
        // resident workgroups per compute unit by LDS (at most 4 of 8 waves); the workgroups stride
        // over the rows, so more of them would only stage G again
        const size_t lds_s = short_lds<L>(a.dim) * sizeof(float), lds_l = long_lds<L>(a.dim) * sizeof(float);
        const int64_t slots_s = (int64_t)num_cus() * (kLdsCu / lds_s < 4 ? kLdsCu / lds_s : 4);
        const int64_t slots_l = (int64_t)num_cus() * (kLdsCu / lds_l < 4 ? kLdsCu / lds_l : 4);
        const int64_t tiles = (a.n_rows + L::UPW - 1) / L::UPW;
        const int64_t want_s = (tiles + kShortWaves - 1) / kShortWaves;
        hipLaunchKernelGGL((als_short_kernel<L>), dim3((unsigned)(want_s < slots_s ? want_s : slots_s)),
                           dim3(kShortWaves * kWave), lds_s, stream, a);
        const int rc = check_launch("rg_als_solve_rows");
        if (rc != RG_OK) return rc;
        hipLaunchKernelGGL((als_long_kernel<L>), dim3((unsigned)(a.n_rows < slots_l ? a.n_rows : slots_l)),
                           dim3(kLongWaves * kWave), lds_l, stream, a);
        return check_launch("rg_als_solve_rows");
    }
};

// ---------------------------------------------------------------- Gram matrix
__global__ void __launch_bounds__(kGramThreads) als_gram_partial_kernel(const float *__restrict__ table, int64_t n,
                                                                        int D, float *__restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float s[kGramTile][kMaxDim];
    const int i0 = (threadIdx.x / 16) * 8, j0 = (threadIdx.x % 16) * 8;
    float acc[8][8], tile[8][8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[u][v] = 0.0f;
    const int64_t r0 = (int64_t)blockIdx.x * kGramRows;
    const int64_t r1 = r0 + kGramRows < n ? r0 + kGramRows : n;
    const bool mine = i0 < D && j0 < D;
    for (int64_t rt = r0; rt < r1; rt += kGramTile) {
        __syncthreads();
        for (int q = threadIdx.x; q < kGramTile * kMaxDim; q += kGramThreads) {
            const int rr = q / kMaxDim, c = q % kMaxDim;
            const int64_t row = rt + rr;
            s[rr][c] = (row < r1 && c < D) ? table[row * (int64_t)D + c] : 0.0f;
        }
        __syncthreads();
        if (mine) {
            // two levels: the tile's kGramTile rows first, then the tile into the block's sum --
            // chains of 16 and 64 additions, not one of 1024
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int v = 0; v < 8; ++v) tile[u][v] = 0.0f;
            for (int rr = 0; rr < kGramTile; ++rr) {      // a row past r1 is zeros: fmaf(0, 0, s) == s
                float ai[8], bj[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    ai[u] = s[rr][i0 + u];
                    bj[u] = s[rr][j0 + u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int v = 0; v < 8; ++v) tile[u][v] = fmaf(ai[u], bj[v], tile[u][v]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int v = 0; v < 8; ++v) acc[u][v] += tile[u][v];
        }
    }
    if (mine) {
        float *out = ws + (int64_t)blockIdx.x * D * D;
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int v = 0; v < 8; ++v)
                if (i0 + u < D && j0 + v < D) out[(i0 + u) * D + j0 + v] = acc[u][v];
    }
}

__global__ void __launch_bounds__(256) als_gram_reduce_kernel(const float *__restrict__ ws, int64_t blocks, int D,
                                                              float lam, float *__restrict__ G) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= D * D) return;
    float s = 0.0f;
    for (int64_t b = 0; b < blocks; ++b) s += ws[b * D * D + e];
    G[e] = (e / D == e % D) ? s + lam : s;
}

int64_t gram_blocks(int64_t n_rows) { return (n_rows + kGramRows - 1) / kGramRows; }

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int32_t rg_als_long_row_len(void) { return kLongRowLen; }

extern "C" int64_t rg_als_gram_workspace_len(int64_t n_rows, int32_t dim) {
    if (n_rows < 0 || dim < 1 || dim > kMaxDim) {
        fail_arg("rg_als_gram_workspace_len: n_rows < 0 or dim outside [1, 128]");
        return -1;
    }
    const int64_t b = gram_blocks(n_rows);
    return (b > 0 ? b : 1) * (int64_t)dim * dim;
}

extern "C" int rg_als_gram(void *stream, const float *table, int64_t n_rows, int32_t dim, float lam,
                           float *workspace_dev, float *out_G) {
    if (!table || !workspace_dev || !out_G) return fail_arg("rg_als_gram: null pointer");
    if (dim < 1 || dim > kMaxDim) return fail_arg("rg_als_gram: dim must be in [1, 128]");
    if (n_rows < 0) return fail_arg("rg_als_gram: n_rows < 0");
    if (!(lam >= 0.0f) || lam > 3.0e38f) return fail_arg("rg_als_gram: lam must be finite and >= 0");
    const int64_t blocks = gram_blocks(n_rows);
    if (blocks > (int64_t)INT_MAX) return fail_arg("rg_als_gram: too many rows for one launch");
    if (blocks > 0) {
        hipLaunchKernelGGL(als_gram_partial_kernel, dim3((unsigned)blocks), dim3(kGramThreads), 0,
                           (hipStream_t)stream, table, n_rows, (int)dim, workspace_dev);
        const int rc = check_launch("rg_als_gram");
        if (rc != RG_OK) return rc;
    }
    hipLaunchKernelGGL(als_gram_reduce_kernel, dim3((unsigned)((dim * dim + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, workspace_dev, blocks, (int)dim, lam, out_G);
    return check_launch("rg_als_gram");
}

extern "C" int rg_als_solve_rows(void *stream, const float *other_table, const float *G, int32_t dim,
                                 const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, float alpha,
                                 const int64_t *rows, int64_t n_rows, int32_t cg_steps, float *x_inout,
                                 float *loss_out) {
    if (!other_table || !G || !row_ptr || !x_inout) return fail_arg("rg_als_solve_rows: null pointer");
    if (dim < 1 || dim > kMaxDim) return fail_arg("rg_als_solve_rows: dim must be in [1, 128]");
    if (cg_steps < 0 || cg_steps > 64) return fail_arg("rg_als_solve_rows: cg_steps must be in [0, 64]");
    if (!(alpha >= 0.0f) || alpha > 3.0e38f) return fail_arg("rg_als_solve_rows: alpha must be finite and >= 0");
    if (n_rows < 0) return fail_arg("rg_als_solve_rows: n_rows < 0");
    if (n_rows == 0) return RG_OK;
    if (!row_idx) return fail_arg("rg_als_solve_rows: row_idx is null");
    const AlsArgs a{other_table, G, dim, row_ptr, row_idx, row_val, alpha, rows, n_rows, cg_steps, x_inout, loss_out};
    const bool aligned = (((uintptr_t)other_table | (uintptr_t)x_inout) & 15u) == 0;
    // the layouts of dim <= kMaxDim alone: none of the wider ones is built for these kernels
    return dispatch_rows<kMaxDim>(dim, aligned, AlsLaunch{a, (hipStream_t)stream});
}
