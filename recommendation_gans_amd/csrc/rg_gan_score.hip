// cGAN critic at inference: rg_gan_score_slates, the eval-mode discriminator.forward
// (spotlight/dnn_models/cGAN_models.py:102-109, no dropout) of integer slates, in ONE launch.
//
// The reference feeds D a one-hot block [rows][S*N]; its first layer is then a GEMM against
// layers.0.weight of which S columns per row are non-zero.  Here the ids select those columns:
//     c      = sum_l D_EMB[hist[r][l]]                      (ids outside [0, N): nothing)
//     u1[j]  = W1E[j] . c + sum_s W1S[j][s*N + slates[r][s]] + B1[j]      (the same)
//     h1     = LeakyReLU_0.2(u1),  h2 = LeakyReLU(W2 h1 + B2),  h3 = LeakyReLU(W3 h2 + B3)
//     out[r] = W4 . h3 + B4
// on the parameters as stored (the +-0.01 clamp is the D iteration's, CGANs.py:438-439, and is
// not applied; line 105's LeakyReLU of the input is overwritten by line 106 and is not either).
//
// A workgroup of 4 waves owns 16 rows, one MFMA column block.
//   ids      the tile's slate ids become W1S column offsets in LDS (-1: selects nothing)
//   c        thread (row, sub = tid % 16) sums history positions sub, sub + 16, .. in order, ids
//            and embedding rows of 4 positions in flight (as hist_sum_kernel); the 16 partials
//            join in a fixed xor tree
//   layer 1  a thread owns a unit j and 4 rows: the E-long fmaf chain against c, then the S
//            gathered W1S entries added in slot order, 4 rows x 8 slots of loads issued before
//            the first add (each is a 4-byte read of its own line: W1S is [2H][ks] row-major)
//   2, 3     fp32 16x16x4 MFMA: the weights (row-major, from L2) are the A operand, 16 output
//            features per tile, up to 4 tiles per wave at a time; the activations [row][k + 4
//            pad] in LDS are the B operand.  A lane multiplies columns 16 ti + 4 g + r of its
//            weight row (one 16-byte load) by the same k of h, so a tile's K order is fixed by
//            the dims.  Output rows past the layer's width load zero weights and a zero bias and
//            so write exact zeros, which is what the next layer's K padding reads.
//   out      thread (row, sub) takes k = sub, sub + 16, .. of the W4 dot, the same xor tree.
// h1 and h2 (and h3, over h1's space) live in LDS; nothing but out[r] is written to global
// memory.  No atomics, and no sum depends on the row's place in the tile, the wave that holds
// it or the batch: a row's score has the same bits wherever it is scored.
#include <climits>

#include "rg_common.h"
#include "rg_mfma.h"

namespace rg {
namespace {

constexpr int kRows = 16;                  // rows per workgroup: one MFMA column block
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kSub = kThreads / kRows;     // threads per row in the history sum and the output dot
constexpr int kTB = 4;                     // output tiles a wave accumulates at a time
constexpr int kRG = 4;                     // rows per thread in layer 1
constexpr int kSB = 8;                     // slate slots whose gathers are issued together
constexpr int kHB = 4;                     // history positions in flight per thread
constexpr int kEChunk = 8;                 // embedding columns accumulated per pass
constexpr float kSlope = 0.2f;             // LeakyReLU(0.2), cGAN_models.py:95
constexpr int kLdsMax = 160 * 1024;
static_assert(kSub == 16 && kRows % kRG == 0, "the xor trees below span 16 lanes");

__host__ __device__ constexpr int r16(int x) { return (x + 15) & ~15; }

struct ScoreArgs {
    const float *w1s, *emb, *w1e, *b1, *w2, *b2, *w3, *b3, *w4, *b4;
    const int32_t *hist, *slates;
    int64_t ks, ld, rows;
    int N, S, H, E, L;
    float *out;
};

// LDS (floats): c [16][E], the slate columns [16][S] (int), h1 [16][2H + 4], h2 [16][r16(H) + 4];
// h3 [16][r16(H/2) + 4] over h1.  Every block starts on a multiple of 16 bytes.
struct Lds {
    int oCol, oH1, oH2, St1, St2, St3, total;
    __host__ __device__ Lds(int H, int E, int S) {
        St1 = 2 * H + 4;
        St2 = r16(H) + 4;
        St3 = r16(H / 2) + 4;
        oCol = kRows * E;
        oH1 = oCol + kRows * S;
        oH2 = oH1 + kRows * St1;
        total = oH2 + kRows * St2;
    }
};

__device__ __forceinline__ float lrelu(float x) { return x > 0.0f ? x : x * kSlope; }

// sum over the 16 threads of a row (lanes that differ in their low 4 bits), the same in each
__device__ __forceinline__ float row_sum(float v) {
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// sOut[row][f] = LeakyReLU(W[f] . sIn[row] + bias[f]) for f < r16(out) (zeros from f = out on);
// W [out][K] row-major in global memory, K a multiple of 8; sIn holds r16(K) columns
__device__ __forceinline__ void mfma_layer(const float *__restrict__ W, const float *__restrict__ bias, int out, int K,
                                           const float *sIn, int StIn, float *sOut, int StOut, int wave, int g, int j) {
    const int nt = r16(out) / 16, nk = r16(K) / 16;
    for (int tb = wave; tb < nt; tb += kWaves * kTB) {
        v4f acc[kTB];
        const float *wrow[kTB];
        bool rowok[kTB];
#pragma unroll
        for (int q = 0; q < kTB; ++q) {
            const int t = tb + kWaves * q, f = 16 * t + 4 * g;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[q][r] = f + r < out ? bias[f + r] : 0.0f;
            rowok[q] = 16 * t + j < out;
            wrow[q] = W + (int64_t)(rowok[q] ? 16 * t + j : 0) * K;
        }
        for (int ti = 0; ti < nk; ++ti) {
            const int k = 16 * ti + 4 * g;
            const v4f b = *reinterpret_cast<const v4f *>(sIn + j * StIn + k);
            v4f a[kTB];
#pragma unroll
            for (int q = 0; q < kTB; ++q)
                a[q] = rowok[q] && k < K ? *reinterpret_cast<const v4f *>(wrow[q] + k) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < kTB; ++q) acc[q] = mfma(a[q][r], b[r], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < kTB; ++q) {
            const int t = tb + kWaves * q;
            if (t >= nt) continue;
            v4f y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = lrelu(acc[q][r]);
            *reinterpret_cast<v4f *>(sOut + j * StOut + 16 * t + 4 * g) = y;
        }
    }
}

__global__ __launch_bounds__(kThreads) void gan_score_kernel(ScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int N = a.N, S = a.S, H = a.H, E = a.E, L = a.L, H2 = 2 * H, H1 = H / 2;
    const Lds o(H, E, S);
    float *sC = lds, *sH1 = lds + o.oH1, *sH2 = lds + o.oH2, *sH3 = sH1;
    int *sCol = reinterpret_cast<int *>(lds + o.oCol);
    const int64_t r0 = (int64_t)blockIdx.x * kRows;

    // ---- slate ids -> W1S column offsets (rows past the batch and ids outside [0, N): -1)
    for (int idx = tid; idx < kRows * S; idx += kThreads) {
        const int r = idx / S, s = idx % S;
        const int id = r0 + r < a.rows ? a.slates[(r0 + r) * a.ld + s] : -1;
        sCol[idx] = (uint32_t)id < (uint32_t)N ? s * N + id : -1;
    }

    // ---- c = sum of the history's embedding rows
    {
        const int r = tid / kSub, sub = tid % kSub;
        const bool live = r0 + r < a.rows;
        const int32_t *hrow = a.hist + (r0 + (live ? r : 0)) * L;
        for (int e0 = 0; e0 < E; e0 += kEChunk) {
            float acc[kEChunk];
#pragma unroll
            for (int e = 0; e < kEChunk; ++e) acc[e] = 0.0f;
            for (int l0 = sub; l0 < L; l0 += kSub * kHB) {
                int it[kHB];
#pragma unroll
                for (int u = 0; u < kHB; ++u) {
                    const int l = l0 + kSub * u;
                    const int id = live && l < L ? hrow[l] : -1;
                    it[u] = (uint32_t)id < (uint32_t)N ? id : -1;
                }
                float x[kHB][kEChunk];
#pragma unroll
                for (int u = 0; u < kHB; ++u)
#pragma unroll
                    for (int e = 0; e < kEChunk; ++e)
                        x[u][e] = it[u] >= 0 && e0 + e < E ? a.emb[(int64_t)it[u] * E + e0 + e] : 0.0f;
#pragma unroll
                for (int u = 0; u < kHB; ++u)
#pragma unroll
                    for (int e = 0; e < kEChunk; ++e) acc[e] += x[u][e];
            }
#pragma unroll
            for (int e = 0; e < kEChunk; ++e) {
                const float v = row_sum(acc[e]);
                if (sub == 0 && e0 + e < E) sC[r * E + e0 + e] = v;
            }
        }
    }
    __syncthreads();

    // ---- layer 1: unit un of rows 4 rg .. 4 rg + 3
    for (int idx = tid; idx < H2 * (kRows / kRG); idx += kThreads) {
        const int un = idx % H2, rg = idx / H2;
        float v[kRG];
#pragma unroll
        for (int q = 0; q < kRG; ++q) v[q] = 0.0f;
        const float *we = a.w1e + (int64_t)un * E;
        for (int e = 0; e < E; ++e) {
            const float w = we[e];
#pragma unroll
            for (int q = 0; q < kRG; ++q) v[q] = fmaf(w, sC[(kRG * rg + q) * E + e], v[q]);
        }
        const float *ws = a.w1s + (int64_t)un * a.ks;
        for (int s0 = 0; s0 < S; s0 += kSB) {
            float x[kSB][kRG];
#pragma unroll
            for (int u = 0; u < kSB; ++u)
#pragma unroll
                for (int q = 0; q < kRG; ++q) {
                    const int col = s0 + u < S ? sCol[(kRG * rg + q) * S + s0 + u] : -1;
                    x[u][q] = col >= 0 ? ws[col] : 0.0f;
                }
#pragma unroll
            for (int u = 0; u < kSB; ++u)
#pragma unroll
                for (int q = 0; q < kRG; ++q) v[q] += x[u][q];
        }
        const float b = a.b1[un];
#pragma unroll
        for (int q = 0; q < kRG; ++q) sH1[(kRG * rg + q) * o.St1 + un] = lrelu(v[q] + b);
    }
    __syncthreads();

    // ---- layers 2 and 3 on the MFMA (h3 overwrites h1, which every wave has finished reading)
    mfma_layer(a.w2, a.b2, H, H2, sH1, o.St1, sH2, o.St2, wave, g, j);
    __syncthreads();
    mfma_layer(a.w3, a.b3, H1, H, sH2, o.St2, sH3, o.St3, wave, g, j);
    __syncthreads();

    // ---- out = W4 . h3 + B4
    {
        const int r = tid / kSub, sub = tid % kSub;
        float p = 0.0f;
        for (int k = sub; k < H1; k += kSub) p = fmaf(sH3[r * o.St3 + k], a.w4[k], p);
        p = row_sum(p);
        if (sub == 0 && r0 + r < a.rows) a.out[r0 + r] = p + a.b4[0];
    }
}

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int rg_gan_score_slates(void *stream, const rg_gan_model_t *mdl, const int32_t *hist, int32_t hist_len,
                                   const int32_t *slates, int64_t ld, int64_t rows, float *out) {
    if (!mdl || !mdl->d || !hist || !slates || !out)
        return fail_arg("rg_gan_score_slates: null model / model->d / hist / slates / out");
    const rg_gan_dims_t &dm = mdl->dims;
    if (dm.num_items <= 0 || dm.slate_size <= 0 || dm.hidden < 2 || dm.hidden % 8 || dm.emb_dim <= 0 ||
        dm.z_dim <= 0 || dm.batch_max <= 0)
        return fail_arg("rg_gan_score_slates: bad dims (hidden must be a positive multiple of 8)");
    if ((int64_t)dm.num_items * dm.slate_size > INT_MAX - 4)
        return fail_arg("rg_gan_score_slates: bad dims (slate_size * num_items must fit 31 bits)");
    if (hist_len < 1) return fail_arg("rg_gan_score_slates: hist_len < 1 (empty history)");
    // the kernel's position counters step past hist_len by up to kSub * kHB before they stop
    if (hist_len > INT_MAX - 2 * kSub * kHB) return fail_arg("rg_gan_score_slates: hist_len too large");
    if (ld < dm.slate_size) return fail_arg("rg_gan_score_slates: ld < slate_size");
    if (rows < 0) return fail_arg("rg_gan_score_slates: rows < 0");
    if (rows > (int64_t)INT_MAX * kRows) return fail_arg("rg_gan_score_slates: too many rows for one launch");
    // an upper bound of Lds::total in 64 bits, before the 32-bit layout is formed
    if (4 * kRows * ((int64_t)dm.emb_dim + dm.slate_size + 3 * (int64_t)dm.hidden + 16) > kLdsMax)
        return fail_arg("rg_gan_score_slates: bad dims (hidden, emb_dim and slate_size exceed a workgroup's LDS)");
    if ((uintptr_t)mdl->d % 16) return fail_arg("rg_gan_score_slates: model->d must be 16-byte aligned");
    if (rows == 0) return RG_OK;
    const Lds o(dm.hidden, dm.emb_dim, dm.slate_size);

    int64_t go[RG_GAN_G_END + 1], dof[RG_GAN_D_END + 1], strides[2];
    if (rg_gan_layout(&dm, go, dof, strides) != 0) return RG_E_ARG;
    const float *d = mdl->d;
    const ScoreArgs a{d + dof[RG_GAN_D_W1S], d + dof[RG_GAN_D_EMB], d + dof[RG_GAN_D_W1E], d + dof[RG_GAN_D_B1],
                      d + dof[RG_GAN_D_W2],  d + dof[RG_GAN_D_B2],  d + dof[RG_GAN_D_W3],  d + dof[RG_GAN_D_B3],
                      d + dof[RG_GAN_D_W4],  d + dof[RG_GAN_D_B4],  hist, slates, strides[1], ld, rows,
                      dm.num_items, dm.slate_size, dm.hidden, dm.emb_dim, hist_len, out};
    const size_t lds = (size_t)o.total * sizeof(float);
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void *>(gan_score_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax) == hipSuccess;
    if (!attr) return fail_arg("rg_gan_score_slates: cannot reserve LDS");
    hipLaunchKernelGGL(gan_score_kernel, dim3((unsigned)((rows + kRows - 1) / kRows)), dim3(kThreads), lds,
                       (hipStream_t)stream, a);
    return check_launch("rg_gan_score_slates");
}
