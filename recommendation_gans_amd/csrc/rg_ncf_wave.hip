// NCF training step, the wave-per-tile kernel (the step as a whole: rg_ncf.hip): ncf_wave_kernel<PHASE>.
// E = 64 tower (C3, mf_dim = 0): one WAVE per tile of ncfw::kR = 48 rows (8 whole columns of
// 1 + 5 rows: 1,024 tiles at B = 8192, n = 5, one per wave of the 256 x 4-wave grid), the forward
// one example block at a time; 32-row tiles (1,639 tiles, two rounds) measured 73.3 against 64.0 us.
//
// The tile kernel (rg_ncf_tile.hip) keeps every activation in LDS and spreads a tile's MFMA tiles
// over 8 waves: ~12 workgroup barriers and an LDS -> MFMA -> LDS round trip per layer, 14 % of the
// fp32 MFMA peak.  Here a wave owns a whole tile and runs the chain with no barrier:
//
//   * "T layout": a 16x16 MFMA C tile of a layer's output transposed, Y^T[feature][example]
//     -- lane (g, j) holds features 16t + 4g + r (r = 0..3) of example 16 nb + j (3 example
//     blocks nb).  Fed back as the B operand of the next product, k-step r of tile t takes
//     feature 16t + 4g + r from lane group g, so  Y_{k+1}^T = W_{k+1} Y_k^T  and
//     dA_k^T = W_k^T delta_k^T  consume the previous result straight from registers (the A
//     operand, a weight, is read from LDS in the same permuted k order).
//   * the forward and the backward each run one example block at a time (a third of the
//     activations / deltas live), each weight-gradient accumulator still taking the tile's
//     examples in row order (block 0's k-steps, then block 1's, ...).
//   * the weight gradients dW_k = sum_e delta_k[e] X_k[e]^T contract over EXAMPLES, which the
//     T layout keeps on lanes; X_k and delta_k are staged into the wave's own LDS rows
//     ([example][feature], unpadded with a rotated column order: conflict-free both ways) and
//     read back with examples on the k axis.  X_0 (the gathered embeddings) is re-read from L2
//     in that layout.  dW accumulates in MFMA accumulators across the wave's tiles; the hidden
//     biases' gradients are per-lane column sums taken from the same reads (no ones operand).
//   * one workgroup of 4 waves per CU (151 KB of LDS, 512 registers per lane); at the end the
//     4 waves' gradients are summed in wave order in LDS into the workgroup's partial.
// Every sum is a fixed-order f32 chain (MFMA = k-ordered fmaf chain), so results are
// deterministic; the order differs from the tile kernel's, so the two agree to fp32 rounding.
#include "rg_ncf.h"
#include "rg_mfma.h"

namespace rg {

namespace ncfw {
constexpr int kThreads = 64 * kWaves;
// The forward runs one 16-example block at a time (as the backward), so a 48-row tile -- 8 whole
// columns of 1 + 5 rows, 1,024 tiles at B = 8192: one per wave slot, no second round -- fits the
// registers (12 B of scratch).  The alternatives that were measured (32-row tiles, every block's
// forward at once, an early first tile) are in DESIGN §9, "Retired build switches".
constexpr int NB = kR / 16;            // example blocks of 16 per tile
// weights in LDS (floats): W_k row-major [out][in + 4] (b128 rows land on distinct 16-B slots),
// W4 and the output row padded to 16 rows of zeros, biases padded with zeros
constexpr int S1 = 132, S2 = 68, S3 = 36, S4 = 20, SO = 20;
constexpr int oW1 = 0, oW2 = oW1 + 64 * S1, oW3 = oW2 + 32 * S2, oW4 = oW3 + 16 * S3, oWo = oW4 + 16 * S4;
constexpr int oB1 = oWo + 16 * SO, oB2 = oB1 + 64, oB3 = oB2 + 32, oB4 = oB3 + 16, oBo = oB4 + 16;
constexpr int kWFloats = oBo + 4;
// per wave: staged activations / deltas [48][F] (F = 64, 32, 16, 16 features, unpadded: the
// column of row r is rotated by 16 (r & 3) for F = 64 and by 16 ((r >> 1) & 1) for F = 32, so the
// example-on-k reads of lane (g, x) -- row 4 s + g, column 16 t + x -- hit 64 distinct banks),
// then the tile's small per-row arrays
constexpr int R1S = 64, R2S = 32, R3S = 16, R4S = 16;
constexpr int oR1 = 0, oR2 = oR1 + kR * R1S, oR3 = oR2 + kR * R2S, oR4 = oR3 + kR * R3S, oSm = oR4 + kR * R4S;
constexpr int kSmall = 11;
constexpr int kWaveFloats = oSm + kSmall * kR;
constexpr int kLdsFloats = kWFloats + kWaves * kWaveFloats;
constexpr int P = NcfTower<64>::P;
static_assert(kLdsFloats <= kLdsMax, "LDS");
static_assert((kR / 2) * 64 <= kR * R2S, "planned item halves ([tc <= kR / 2][64]) fit the delta2 rows");
static_assert(kWFloats % 4 == 0 && kWaveFloats % 4 == 0, "16-B alignment");
static_assert(kR <= 64 && kR % 16 == 0, "one lane per row, whole example blocks");

// float index of (row, column) in a staged [kR][RS] buffer (column a multiple of 4 for float4
// accesses stays inside its 16-column group)
template <int RS>
__device__ __forceinline__ int at(int row, int col) {
    if constexpr (RS == 64) return row * 64 + ((col + 16 * (row & 3)) & 63);
    else if constexpr (RS == 32) return row * 32 + ((col + 16 * ((row >> 1) & 1)) & 31);
    else return row * RS + col;
}

// orders this wave's LDS traffic for the compiler: DS instructions of one wave execute in
// order, so a wavefront-scope fence (no wait instruction) is all a cross-lane LDS hand-off
// inside the wave needs
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// torch's LeakyReLU(0.1) -> Dropout(0.5) multiplier from the kept bit and the sign of the
// output (A = z m with m > 0 keeps the sign of z; a dropped unit's delta is 0)
__device__ __forceinline__ float mult(float y, bool keep, bool training) {
    const float m1 = y > 0.0f ? 1.0f : 0.1f;
    return training ? (keep ? 2.0f * m1 : 0.0f) : m1;
}

// ---- one example block (16 examples, lane j = example 16 nb + j): the forward and the backward
// run block by block so a third of the tile's activations / deltas is live at a time ----
// dA^T (TI tiles) = W^T delta^T for one block
template <int TI, int TO>
__device__ __forceinline__ void bwd1(const v4f (&d)[TO], v4f (&da)[TI], const float *W, int S, int g, int x) {
#pragma unroll
    for (int t = 0; t < TI; ++t) da[t] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a[TI];
#pragma unroll
            for (int ti = 0; ti < TI; ++ti) a[ti] = W[(16 * to + 4 * g + r) * S + 16 * ti + x];
#pragma unroll
            for (int ti = 0; ti < TI; ++ti) da[ti] = mfma(a[ti], d[to][r], da[ti]);
        }
}
// dW += the block's examples (k-steps s0 .. s0 + 3 of the tile: rows 4 s + g), bias column sums
template <int TOo, int TIi, int SD, int SX>
__device__ __forceinline__ void dw1b(v4f (&acc)[TOo][TIi], float (&bs)[TOo], const float *D, const float *X, int g,
                                     int x, int s0) {
#pragma unroll
    for (int s = s0; s < s0 + 4; ++s) {
        float a[TOo], b[TIi];
#pragma unroll
        for (int to = 0; to < TOo; ++to) a[to] = D[at<SD>(4 * s + g, 16 * to + x)];
#pragma unroll
        for (int ti = 0; ti < TIi; ++ti) b[ti] = X[at<SX>(4 * s + g, 16 * ti + x)];
#pragma unroll
        for (int to = 0; to < TOo; ++to) {
#pragma unroll
            for (int ti = 0; ti < TIi; ++ti) acc[to][ti] = mfma(a[to], b[ti], acc[to][ti]);
            bs[to] += a[to];
        }
    }
}
template <int T, int RS>
__device__ __forceinline__ void unstage1(v4f (&y)[T], const float *R, int row, int g) {
#pragma unroll
    for (int t = 0; t < T; ++t) y[t] = *reinterpret_cast<const v4f *>(R + at<RS>(row, 16 * t + 4 * g));
}
template <int T, int RS>
__device__ __forceinline__ void stage1(const v4f (&y)[T], float *R, int row, int g) {
#pragma unroll
    for (int t = 0; t < T; ++t) *reinterpret_cast<v4f *>(R + at<RS>(row, 16 * t + 4 * g)) = y[t];
}

// Y^T (TO tiles) = W X^T for one example block (the forward one 16-example block at a time)
template <int TI, int TO>
__device__ __forceinline__ void fwd1(const v4f (&x)[TI], v4f (&y)[TO], const float *W, int S, int g, int m) {
#pragma unroll
    for (int t = 0; t < TO; ++t) y[t] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ti = 0; ti < TI; ++ti) {
        v4f a[TO];
#pragma unroll
        for (int t = 0; t < TO; ++t) a[t] = *reinterpret_cast<const v4f *>(W + (16 * t + m) * S + 16 * ti + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < TO; ++t) y[t] = mfma(a[t][r], x[ti][r], y[t]);
    }
}

// bit of unit (t, nb, r) of a layer in its keep word
__device__ __forceinline__ constexpr int kbit(int t, int nb, int r) { return (t * NB + nb) * 4 + r; }
}  // namespace ncfw

// Diagnostic build only: per-wave phase stamps of its first two tiles (16 slots per tile),
// each draining the wave's loads and LDS traffic first (scripts/ncf_stamps.py --wave); this
// unit's copy of the buffer pointer (rg_diag_set_ncf_stamps sets it beside the tile kernel's)
#ifdef RG_DIAG_STAMPS
__device__ unsigned long long *g_ncfw_stamps;
int ncf_wave_set_stamps(unsigned long long *dev_buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_ncfw_stamps), &dev_buf, sizeof(dev_buf)) == hipSuccess ? RG_OK : RG_E_LAUNCH;
}
#define WS(k)                                                                                              \
    do {                                                                                                   \
        if (g_ncfw_stamps && tl_ < 2) {                                                                     \
            unsigned long long t_;                                                                         \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)"      \
                         : "=s"(t_)::"memory");                                                            \
            if (lane == 0) g_ncfw_stamps[(((int64_t)blockIdx.x * ncfw::kWaves + wave) * 3 + tl_) * 16 + (k)] = t_; \
        }                                                                                                  \
    } while (0)
// stamps inside the backward's block loop: block 0's only (the later blocks' phases are the
// "blocks 1.." stamp pair, so no stamp is overwritten by a later block)
#define WSB(k)          \
    do {                \
        if (nb == 0) WS(k); \
    } while (0)
#define WSK(k)                                                                                             \
    do {                                                                                                   \
        if (g_ncfw_stamps) {                                                                                \
            unsigned long long t_;                                                                         \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)"      \
                         : "=s"(t_)::"memory");                                                            \
            if (lane == 0) g_ncfw_stamps[(((int64_t)blockIdx.x * ncfw::kWaves + wave) * 3 + 2) * 16 + (k)] = t_; \
        }                                                                                                  \
    } while (0)
#else
#define WS(k) \
    do {      \
    } while (0)
#define WSK(k) \
    do {      \
    } while (0)
#define WSB(k) \
    do {      \
    } while (0)
#endif

template <int PHASE>
__global__ __launch_bounds__(ncfw::kThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) void ncf_wave_kernel(NcfArgs a) {
    using namespace ncfw;
    using S64 = NcfTower<64>;
    constexpr bool kBackward = PHASE != kNcfScores && PHASE != kNcfLossOnly;
    constexpr int WO = S64::w_off(4);
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
    float *sw = lds;
    float *ws = lds + kWFloats + wave * kWaveFloats;
    float *R1 = ws + oR1, *R2 = ws + oR2, *R3 = ws + oR3, *R4 = ws + oR4;
    int *sU = reinterpret_cast<int *>(ws + oSm), *sI = sU + kR, *sR = sI + kR;
    uint32_t *sK = reinterpret_cast<uint32_t *>(sR + kR);
    float *sP = reinterpret_cast<float *>(sK + kR), *sDz = sP + kR, *sLa = sDz + kR, *sLb = sLa + kR;
    int *sLu = reinterpret_cast<int *>(sLb + kR), *sLi = sLu + kR, *sPs = sLi + kR;
    WSK(0);   // kernel entry (diag: kernel-level record 2)

    // ---- parameters: every load issued first, then the LDS stores (the first tile's record is
    // fetched in between), then one barrier ----
    constexpr int kTail = kWFloats - oW4;   // W4 rows (8..15 zero), the output row, the biases
    constexpr int PT1 = 64 * 128 / 4 / kThreads, PT2 = 32 * 64 / 4 / kThreads, PT3 = (16 * 32 / 4 + kThreads - 1) / kThreads;
    constexpr int PTT = (kTail + kThreads - 1) / kThreads;
    static_assert(64 * 128 / 4 % kThreads == 0 && 32 * 64 / 4 % kThreads == 0, "weight copy shape");
    float4 wv1[PT1], wv2[PT2], wv3[PT3];
    float wvt[PTT];
    {
        const float4 *W1 = reinterpret_cast<const float4 *>(a.mlp + S64::w_off(0));
        const float4 *W2 = reinterpret_cast<const float4 *>(a.mlp + S64::w_off(1));
        const float4 *W3 = reinterpret_cast<const float4 *>(a.mlp + S64::w_off(2));
#pragma unroll
        for (int k = 0; k < PT1; ++k) wv1[k] = W1[tid + k * kThreads];
#pragma unroll
        for (int k = 0; k < PT2; ++k) wv2[k] = W2[tid + k * kThreads];
#pragma unroll
        for (int k = 0; k < PT3; ++k) wv3[k] = W3[min(tid + k * kThreads, 16 * 32 / 4 - 1)];
#pragma unroll
        for (int k = 0; k < PTT; ++k) {   // flat source index of LDS float oW4 + e (or -1: zero)
            const int o = oW4 + min(tid + k * kThreads, kTail - 1);
            int src = -1;
            if (o < oWo) {
                const int row = (o - oW4) / S4, col = (o - oW4) % S4;
                if (row < 8 && col < 16) src = S64::w_off(3) + row * 16 + col;
            } else if (o < oB1) {
                if (o - oWo < 8) src = WO + (o - oWo);
            } else if (o < oB2) {
                src = S64::w_off(0) + 64 * 128 + (o - oB1);
            } else if (o < oB3) {
                src = S64::w_off(1) + 32 * 64 + (o - oB2);
            } else if (o < oB4) {
                src = S64::w_off(2) + 16 * 32 + (o - oB3);
            } else if (o < oBo) {
                if (o - oB4 < 8) src = S64::w_off(3) + 8 * 16 + (o - oB4);
            } else if (o == oBo) {
                src = WO + 8;
            }
            const float v = a.mlp[src < 0 ? 0 : src];
            wvt[k] = src < 0 ? 0.0f : v;
        }
    }
    const float *W1s = sw + oW1, *W2s = sw + oW2, *W3s = sw + oW3, *W4s = sw + oW4, *Wos = sw + oWo;
    const bool training = a.training != 0;
    const int n = a.n_neg, NP = n + 1, tc = a.tc;
    constexpr int units = S64::mask_units();
    const bool pairwise = a.loss == RG_LOSS_BPR || a.loss == RG_LOSS_HINGE;

    // running gradients of this wave: the weight tiles and the output layer's [w_out | b_out]
    // tile in MFMA accumulators, the hidden biases as per-lane column sums (lane (g, x): the
    // examples e = g mod 4 of feature 16 t + x)
    v4f gW1[4][8], gW2[2][4], gW3[1][2], gW4[1][1], gO;
    float bB1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, bB2[2] = {0.0f, 0.0f}, bB3[1] = {0.0f}, bB4[1] = {0.0f};
    const v4f z4 = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) gW1[p][q] = z4;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) gW2[p][q] = z4;
    gW3[0][0] = gW3[0][1] = gW4[0][0] = gO = z4;

    // a column's pair record for row r = q * tc + cl of `tile` (lanes 0..31): the loads are
    // issued unconditionally from clamped indices (fetch) and resolved when the values are
    // needed, a tile later (finish), so no wait sits in between
    struct RowRaw {
        int2 pr;
        int ps, perm;
        int64_t s;
        int q;
        bool valid;
    };
    auto fetch_row = [&](int64_t tile, int r) {
        RowRaw w;
        w.q = r / tc;
        const int cl = r % tc;
        w.s = tile * tc + cl;
        bool valid = tile < a.tiles && w.q < NP && w.s < a.cols;
        if (valid && w.q == 0) valid = w.s < a.n_pos;
        if (valid && w.q > 0 && pairwise) valid = w.s < a.n_pos;
        w.valid = valid;
        w.pr = make_int2(-1, -1);
        w.ps = -1;
        w.perm = 0;
        if (tile < a.tiles) {   // (a tile past the end has no record to read: cols may be 0)
            const int64_t sc = w.s < a.cols ? w.s : a.cols - 1;
            w.pr = a.pairs[sc * pair_stride(a.n_neg) + min(w.q, n)];
            w.ps = a.pos_slot != nullptr ? a.pos_slot[sc] : -1;
            w.perm = a.perm ? a.perm[sc] : 0;
        }
        return w;
    };
    auto finish_row = [&](const RowRaw &w, int &u, int &i, int &ps, int64_t &gj) {
        u = w.valid ? w.pr.x : -1;
        i = w.valid ? w.pr.y : -1;
        ps = (kBackward && w.valid && w.q == 0) ? w.ps : -1;
        const int64_t colid = a.perm && w.s < a.cols ? (int64_t)w.perm : w.s;
        gj = w.q == 0 ? a.col_offset + colid : (int64_t)(w.q - 1) * a.global_cols + a.col_offset + colid;
    };

    const int64_t waves_total = (int64_t)gridDim.x * kWaves;
    const int64_t first = (int64_t)blockIdx.x * kWaves + wave;
    RowRaw nxt{};   // the next tile's record (lanes 0..31), in flight during this tile
    if (lane < kR) nxt = fetch_row(first, lane);
    // a tile's start: its record resolved into the wave's row arrays, the gather of X0 issued
    auto begin_tile = [&](int tcl, int &ru, int &ri, int &rps, int (&ue)[NB], int (&ie)[NB], int (&re)[NB],
                          uint32_t (&ke)[NB], v4f (&x0)[8][NB]) {
        int64_t ngj = 0;
        if (lane < kR) {
            finish_row(nxt, ru, ri, rps, ngj);
            const int r = lane, q = r / tcl;
            sU[r] = ru;
            sI[r] = ri;
            sR[r] = (int)ngj;
            sK[r] = hash32(a.seed ^ ((uint64_t)(q == 0 ? 0 : 1) << 40) ^ ((uint64_t)ngj * 0x9E3779B97F4A7C15ULL));
            sDz[r] = 0.0f;
            sPs[r] = rps;
        }
        wave_sync();
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            ue[nb] = sU[nb * 16 + j];
            ie[nb] = sI[nb * 16 + j];
            re[nb] = sR[nb * 16 + j];
            ke[nb] = sK[nb * 16 + j];
        }
        // ---- gather X0^T (T layout): features 16 t + 4 g .. + 3 of example nb * 16 + j; a row
        // that is not a valid pair reads row 0 (its dz is 0, so none of its values reach a
        // gradient, and its score is never used) ----
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const float *pu = a.user_w + (int64_t)(ue[nb] >= 0 ? ue[nb] : 0) * 64 + 4 * g;
            const float *pi = a.item_w + (int64_t)(ue[nb] >= 0 ? ie[nb] : 0) * 64 + 4 * g;
#pragma unroll
            for (int t = 0; t < 8; ++t) x0[t][nb] = *reinterpret_cast<const v4f *>(t < 4 ? pu + 16 * t : pi + 16 * (t - 4));
        }
    };
    // the weights into LDS (the first record's loads above are in flight meanwhile; inline, not
    // a lambda: a captured register array would live in scratch)
#pragma unroll
    for (int k = 0; k < PT1; ++k) {
        const int e = tid + k * kThreads;
        *reinterpret_cast<float4 *>(sw + oW1 + (e / 32) * S1 + (e % 32) * 4) = wv1[k];
    }
#pragma unroll
    for (int k = 0; k < PT2; ++k) {
        const int e = tid + k * kThreads;
        *reinterpret_cast<float4 *>(sw + oW2 + (e / 16) * S2 + (e % 16) * 4) = wv2[k];
    }
#pragma unroll
    for (int k = 0; k < PT3; ++k) {
        const int e = tid + k * kThreads;
        if (e < 16 * 32 / 4) *reinterpret_cast<float4 *>(sw + oW3 + (e / 8) * S3 + (e % 8) * 4) = wv3[k];
    }
#pragma unroll
    for (int k = 0; k < PTT; ++k)
        if (tid + k * kThreads < kTail) sw[oW4 + tid + k * kThreads] = wvt[k];
    __syncthreads();
    float warm = 0.0f;   // the next tile's embedding lines, touched during this tile's backward
    for (int64_t tile = first; tile < a.tiles; tile += waves_total) {
        int tc = a.tc;   // opaque per tile: keeps the loss / row addresses from being hoisted (and spilled)
        asm volatile("" : "+s"(tc));
        const int tl_ = (int)((tile - first) / waves_total);
        (void)tl_;
        WS(0);
        int ru = -1, ri = -1, rps = -1, ue[NB], ie[NB], re[NB];
        uint32_t ke[NB];
        v4f x0[8][NB];
        begin_tile(tc, ru, ri, rps, ue, ie, re, ke, x0);
        if (warm == 1.0e30f && a.n_pos < 0) a.scores[0] = warm;   // keeps the warm-up loads (never taken)
        WS(1);
        // dropout bits of every unit of the tile, computed while the gather is in flight
        // (bit kbit(t, nb, r) of a layer's word: feature 16 t + 4 g + r, example nb * 16 + j)
        auto keep_bits = [&](auto tc_, int out, int mask_base) -> uint64_t {
            constexpr int T = decltype(tc_)::value;
            uint64_t keep = 0;
            if (!training) return keep;
            if (a.mask_pos) {   // recorded masks (parity tests): every byte load first
                uint8_t mv[T][NB][4];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const uint8_t *mk = (nb * 16 + j < tc ? a.mask_pos : a.mask_neg) +
                                        (int64_t)(ue[nb] >= 0 ? re[nb] : 0) * units + mask_base;
#pragma unroll
                    for (int t = 0; t < T; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) mv[t][nb][r] = mk[min(16 * t + 4 * g + r, out - 1)];
                }
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            keep |= (uint64_t)(mv[t][nb][r] != 0 && ue[nb] >= 0 && 16 * t + 4 * g + r < out)
                                    << kbit(t, nb, r);
            } else {
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int f = 16 * t + 4 * g + r;
                            const uint32_t h = mix32(ke[nb] + (uint32_t)(mask_base + f) * 0x85EBCA6BU);
                            keep |= (uint64_t)(((h >> 7) & 1U) & (uint32_t)(f < out)) << kbit(t, nb, r);
                        }
            }
            return keep;
        };
        // layer 1 (4 x NB x 4 = 48 bits) in kb1; layers 2, 3, 4 (24 + 12 + 12 bits) in kb2
        const uint64_t kb1 = keep_bits(std::integral_constant<int, 4>{}, 64, S64::mask_off(0));
        const uint64_t kb2 = keep_bits(std::integral_constant<int, 2>{}, 32, S64::mask_off(1)) |
                             keep_bits(std::integral_constant<int, 1>{}, 16, S64::mask_off(2)) << 24 |
                             keep_bits(std::integral_constant<int, 1>{}, 8, S64::mask_off(3)) << 36;
        static_assert(kbit(3, NB - 1, 3) < 64 && kbit(1, NB - 1, 3) + 1 + 2 * (kbit(0, NB - 1, 3) + 1) <= 64,
                      "keep words");
        // list slots claimed behind the gather (their round trip overlaps it and the first layer;
        // the entries are written after it)
        int lu = -1, li = -1;
        if (kBackward && lane < kR && ru >= 0) {
            lu = atomicAdd(a.row_count + ru, 1);
            if (rps < 0 && !(lane < tc && a.pos_slot != nullptr)) li = atomicAdd(a.row_count + a.num_users + ri, 1);
        }
        WS(2);
        // ---- forward, one 16-example block at a time (as the backward): one block's activations
        // live at once, so a 48-row tile (three blocks) fits the registers of a 32-row one ----
        // bias, LeakyReLU(0.1), Dropout(0.5) as one multiplier per unit
        auto activate1 = [&](auto &y, const float *b, uint64_t kw, int bit0, int nb) {
            constexpr int T = sizeof(y) / sizeof(y[0]);
            v4f bv[T];
#pragma unroll
            for (int t = 0; t < T; ++t) bv[t] = *reinterpret_cast<const v4f *>(b + 16 * t + 4 * g);
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = y[t][r] + bv[t][r];
                    const float m1 = z > 0.0f ? 1.0f : 0.1f;
                    const float m = training ? (((kw >> (bit0 + kbit(t, nb, r))) & 1U) ? 2.0f * m1 : 0.0f) : m1;
                    y[t][r] = z * m;
                }
        };
        const float bo = sw[oBo];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int row = nb * 16 + j;
            v4f xb[8], a1[4], a2[2], a3[1], a4[1], zb[1];
#pragma unroll
            for (int t = 0; t < 8; ++t) xb[t] = x0[t][nb];
            fwd1<8, 4>(xb, a1, W1s, S1, g, j);
            activate1(a1, sw + oB1, kb1, 0, nb);
            stage1<4, R1S>(a1, R1, row, g);
            fwd1<4, 2>(a1, a2, W2s, S2, g, j);
            activate1(a2, sw + oB2, kb2, 0, nb);
            stage1<2, R2S>(a2, R2, row, g);
            fwd1<2, 1>(a2, a3, W3s, S3, g, j);
            activate1(a3, sw + oB3, kb2, 24, nb);
            stage1<1, R3S>(a3, R3, row, g);
            fwd1<1, 1>(a3, a4, W4s, S4, g, j);
            activate1(a4, sw + oB4, kb2, 36, nb);
            if (kBackward) {   // A_4 rows with a ones feature (8) for the output layer's bias gradient
                v4f a4s[1] = {a4[0]};
                if (g == 2) a4s[0][0] = 1.0f;
                stage1<1, R4S>(a4s, R4, row, g);
            }
            fwd1<1, 1>(a4, zb, Wos, SO, g, j);
            if (g == 0) {
                const float p = sigmoidf_ref(zb[0][0] + bo);
                sP[row] = p;
                if (PHASE == kNcfScores) a.scores[tile * kR + row] = ue[nb] >= 0 ? p : 0.0f;
            }
        }
        WS(3);
        // list entries of the claimed slots (the atomics have returned by now)
        if (kBackward && lane < kR) {
            const int64_t ex = tile * kR + lane;
            if (lu >= 0 && lu < kNcfCap) store_entry(a.row_list + (int64_t)ru * kNcfCap + lu, (int)ex, 1.0f);
            if (li >= 0 && li < kNcfCap)
                store_entry(a.row_list + (a.num_users + ri) * kNcfCap + li, (int)ex, 1.0f);
            sLu[lane] = lu;
            sLi[lane] = li;
        }
        // the next tile's record, in flight during this tile's loss and backward
        if (lane < kR) nxt = fetch_row(tile + waves_total, lane);
        wave_sync();
        WS(4);
        if (PHASE == kNcfScores) continue;
        // ---- loss: one lane per row, then the positives' lanes sum their column in q order
        // (the tile kernel's arithmetic and summation order) ----
        float *sT = reinterpret_cast<float *>(sK);   // row -> the positive's dL/dp term (sK is dead here)
        if (lane < kR) {
            const int r = lane, q = r / tc, cl = r % tc;
            const bool v = q < NP && sU[r] >= 0, vp = sU[cl] >= 0;
            const float p = sP[r], pp = sP[cl];
            float dpr = 0.0f, ta = 0.0f, tb = 0.0f, t0 = 0.0f;
            if (PHASE == kNcfGivenDp) {
                if (v) dpr = a.dp_in[tile * kR + r];
            } else if (a.loss == RG_LOSS_POINTWISE) {
                if (v && q == 0) {
                    ta = -fmaxf(logf(p), -100.0f);
                    dpr = ((p - 1.0f) / fmaxf((1.0f - p) * p, 1e-12f)) / a.n_a;
                } else if (v) {
                    tb = -fmaxf(logf(1.0f - p), -100.0f);
                    dpr = (p / fmaxf((1.0f - p) * p, 1e-12f)) / a.n_b;
                }
            } else if (v && vp && q > 0) {   // bpr / hinge on the neg.view(n, B) pairing
                const float gg = 1.0f / a.n_a;
                if (a.loss == RG_LOSS_BPR) {
                    const float sg = sigmoidf_ref(pp - p);
                    ta = 1.0f - sg;
                    const float dx = (-gg) * (1.0f - sg) * sg;
                    t0 = dx;
                    dpr = -dx;
                } else {
                    const float xx = (p - pp) + 1.0f;
                    ta = fmaxf(xx, 0.0f);
                    const float dx = xx >= 0.0f ? gg : 0.0f;
                    t0 = -dx;
                    dpr = dx;
                }
            }
            sLa[r] = ta;
            sLb[r] = tb;
            sT[r] = t0;
            wave_sync();
            if (q == 0 && PHASE != kNcfGivenDp) {   // the positive: its column's sums in q order
                constexpr int QM = RG_MF_MAX_NEG + 1;
                float la = ta, lb = 0.0f;
                float ca[QM], cb[QM], c0[QM];
                bool cv[QM];
#pragma unroll
                for (int k = 1; k < QM; ++k) {
                    const int rr = min(k * tc + cl, kR - 1);
                    ca[k] = sLa[rr];
                    cb[k] = sLb[rr];
                    c0[k] = sT[rr];
                    cv[k] = k < NP && sU[rr] >= 0;
                }
                if (a.loss == RG_LOSS_POINTWISE) {
#pragma unroll
                    for (int k = 1; k < QM; ++k)
                        if (cv[k]) lb += cb[k];
                } else {
                    la = 0.0f;
                    float d0 = 0.0f;
#pragma unroll
                    for (int k = 1; k < QM; ++k)
                        if (cv[k] && v) { la += ca[k]; d0 += c0[k]; }
                    dpr = d0;
                }
                wave_sync();
                sLa[cl] = la;   // column totals (row cl is this lane's own row)
                sLb[cl] = lb;
            }
            sDz[r] = v ? (dpr * (1.0f - p)) * p : 0.0f;
        }
        wave_sync();
        if (lane == 0) {   // column order, as the one-thread loop summed them
            constexpr int CM = kR / 2;   // columns per tile at most (n >= 1)
            float va[CM], vb[CM];
#pragma unroll
            for (int cl = 0; cl < CM; ++cl) {
                va[cl] = cl < tc ? sLa[cl] : 0.0f;
                vb[cl] = cl < tc ? sLb[cl] : 0.0f;
            }
            float la = 0.0f, lb = 0.0f;
#pragma unroll
            for (int cl = 0; cl < CM; ++cl)
                if (cl < tc) { la += va[cl]; lb += vb[cl]; }
            a.loss_partials[2 * tile] = la;
            a.loss_partials[2 * tile + 1] = lb;
        }
        if (PHASE == kNcfLossOnly) { wave_sync(); continue; }
        // the next tile's rows (its record arrived during the loss): one load per 128-B line of
        // each user / item row, so its gather at the next tile's start hits L2
        if (lane < kR && nxt.valid) {
            const float *pu = a.user_w + (int64_t)nxt.pr.x * 64, *pi = a.item_w + (int64_t)nxt.pr.y * 64;
            warm += (pu[0] + pu[32]) + (pi[0] + pi[32]);
        }
        WS(5);
        // ---- backward, one example block at a time (lane j: example 16 nb + j).  Every weight-
        // gradient accumulator still takes the tile's examples in row order (block 0's k-steps,
        // then block 1's, ...), so the sums are those of one pass over the tile ----
        auto mult4 = [&](v4f &d, const v4f &y, uint64_t kw, int bit) {
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = d[r] * mult(y[r], (kw >> (bit + r)) & 1, training);
        };
        WS(6);
#pragma unroll 1
        for (int nb = 0; nb < NB; ++nb) {
            const int row = nb * 16 + j, s0 = 4 * nb;
            // X0 of the block with examples on the k axis for dW1 (lane (g, x): X0[4 s + g][16 t + x],
            // user columns t < 4, item columns t >= 4), re-read from L2 now for use after three
            // layers; rows that are not valid pairs read row 0 (their delta is 0)
            float xn[4][8];
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                const int e = 4 * (s0 + s2) + g, u = sU[e], i = sI[e];
                const float *pu = a.user_w + (int64_t)(u >= 0 ? u : 0) * 64 + j;
                const float *pi = a.item_w + (int64_t)(u >= 0 ? i : 0) * 64 + j;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    xn[s2][t] = pu[16 * t];
                    xn[s2][4 + t] = pi[16 * t];
                }
            }
            const float dzb = sDz[row];
            // output layer: [dW_out | db_out] += sum_e [A_4 | 1][e] dz[e]; delta_4 = (dz w_out) m_4
            // (A_4's feature 8 is the ones column: its output weight is 0, so its delta is too)
#pragma unroll
            for (int s = s0; s < s0 + 4; ++s) gO = mfma(R4[(4 * s + g) * R4S + j], sDz[4 * s + g], gO);
            v4f y4b[1], d4b[1], y3b[1], d3b[1];
            unstage1<1, R4S>(y4b, R4, row, g);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                d4b[0][r] = (dzb * Wos[4 * g + r]) * mult(y4b[0][r], (kb2 >> (36 + kbit(0, nb, r))) & 1, training);
            unstage1<1, R3S>(y3b, R3, row, g);                  // A_3 back from its staged rows
            bwd1<1, 1>(d4b, d3b, W4s, S4, g, j);
            mult4(d3b[0], y3b[0], kb2, 24 + kbit(0, nb, 0));
            wave_sync();                                        // A_4 reads done before delta_4 lands there
            stage1<1, R4S>(d4b, R4, row, g);
            wave_sync();
            dw1b<1, 1, R4S, R3S>(gW4, bB4, R4, R3, g, j, s0);   // dW4 += delta4^T A_3
            v4f y2b[2], d2b[2];
            unstage1<2, R2S>(y2b, R2, row, g);
            bwd1<2, 1>(d3b, d2b, W3s, S3, g, j);
#pragma unroll
            for (int t = 0; t < 2; ++t) mult4(d2b[t], y2b[t], kb2, kbit(t, nb, 0));
            wave_sync();                                        // A_3 reads done before delta_3 lands there
            stage1<1, R3S>(d3b, R3, row, g);
            wave_sync();
            dw1b<1, 2, R3S, R2S>(gW3, bB3, R3, R2, g, j, s0);
            v4f y1b[4], d1b[4];
            unstage1<4, R1S>(y1b, R1, row, g);
            bwd1<4, 2>(d2b, d1b, W2s, S2, g, j);
#pragma unroll
            for (int t = 0; t < 4; ++t) mult4(d1b[t], y1b[t], kb1, kbit(t, nb, 0));
            wave_sync();
            stage1<2, R2S>(d2b, R2, row, g);
            wave_sync();
            WSB(7);
            dw1b<2, 4, R2S, R1S>(gW2, bB2, R2, R1, g, j, s0);
            WSB(8);
            wave_sync();
            stage1<4, R1S>(d1b, R1, row, g);
            wave_sync();
            WSB(9);
            // dW1 += delta1^T X0 (the block's k-steps), db1 alongside
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                float av[4];
#pragma unroll
                for (int to = 0; to < 4; ++to) av[to] = R1[at<R1S>(4 * (s0 + s2) + g, 16 * to + j)];
#pragma unroll
                for (int to = 0; to < 4; ++to) {
#pragma unroll
                    for (int t = 0; t < 8; ++t) gW1[to][t] = mfma(av[to], xn[s2][t], gW1[to][t]);
                    bB1[to] += av[to];
                }
            }
            WSB(10);
            // dX0^T = W1^T delta1^T: the block's input gradient rows, in four quarters of 32
            // columns (user 0-31, 32-63, item 0-31, 32-63), each stored at once, overflow rows
            // (lists full) in fixed point
            const int lu = sLu[row], li = sLi[row], ur = sU[row], ir = sI[row];
            float *ctile = a.contrib + (int64_t)__builtin_amdgcn_readfirstlane((int)tile) * (kR * 128);
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int hh = qq >> 1, c0 = 32 * (qq & 1);   // table half, first column in the row
                v4f dx[2];
                bwd1<2, 4>(d1b, dx, W1s + 32 * qq, S1, g, j);
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    // write-through (16-B sc1): these 25 MB of rows leave the XCD's L2 as they are
                    // written instead of waiting dirty for the kernel's end-of-kernel write-back
                    // (measured: ncf_wave_kernel 63.7-64.1 -> 62.5-63.0 us, profiles/r6/ncf/); the
                    // resource starts at this wave's tile (a wave-uniform base, small offsets)
                    __builtin_amdgcn_raw_buffer_store_b128(
                        dx[t], __builtin_amdgcn_make_buffer_rsrc(ctile, 0, 0xffffffff, 0x00020000),
                        (row * 128 + 32 * qq + 16 * t + 4 * g) * 4, 0, kSc1);
                if ((hh == 0 ? lu : li) >= kNcfCap) {
                    const int64_t orow = hh == 0 ? (int64_t)ur : a.num_users + ir;
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) fix_add(a.hot_grad + orow * 64 + c0 + 16 * t + 4 * g + r, dx[t][r]);
                }
            }
            WSB(11);
        }
        WS(12);
        if (a.pos_slot != nullptr) {
            // planned positives: lane c runs the segments of equal plan slots in column order (the
            // same sums as a per-segment loop) over the positives' item halves just stored
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // this wave's contrib stores visible
            float acc = 0.0f;
            int prev = -2;
            for (int cl = 0; cl < tc; ++cl) {
                const int slot = sPs[cl];
                if (slot != prev) acc = 0.0f;
                acc += a.contrib[(tile * kR + cl) * (int64_t)128 + 64 + lane];
                prev = slot;
                if (slot >= 0 && (cl + 1 == tc || sPs[cl + 1] != slot)) a.part_row[(int64_t)slot * 64 + lane] = acc;
            }
        }
        wave_sync();
        WS(13);
    }
    if constexpr (!kBackward) return;
    // ---- the workgroup's weight-gradient partial: ((w0 + w2) + (w1 + w3)) -- waves 0 and 1 store
    // into two LDS images, then waves 2 and 3 add into them (each address has one adder, so the
    // sums are deterministic), and the global write adds the two images ----
    float *red = lds;   // every wave is past its tiles (barrier below): weights and scratch are free
    static_assert(2 * P <= kLdsFloats, "two gradient images");
    // the hidden biases: the four lane groups' column sums, (g0 + g1) + (g2 + g3) on every lane
    auto gsum = [](float v) {
        v += __shfl_xor(v, 16);
        return v + __shfl_xor(v, 32);
    };
    float sB1[4], sB2[2];
#pragma unroll
    for (int to = 0; to < 4; ++to) sB1[to] = gsum(bB1[to]);
#pragma unroll
    for (int to = 0; to < 2; ++to) sB2[to] = gsum(bB2[to]);
    const float sB3 = gsum(bB3[0]), sB4 = gsum(bB4[0]);
    auto each_bias = [&](auto &&f) {   // lanes of group 0, one per feature
#pragma unroll
        for (int to = 0; to < 4; ++to) f(S64::w_off(0) + 64 * 128 + 16 * to + j, sB1[to], g == 0);
#pragma unroll
        for (int to = 0; to < 2; ++to) f(S64::w_off(1) + 32 * 64 + 16 * to + j, sB2[to], g == 0);
        f(S64::w_off(2) + 16 * 32 + j, sB3, g == 0);
        f(S64::w_off(3) + 8 * 16 + min(j, 7), sB4, g == 0 && j < 8);
    };
    WSK(1);   // tiles done
    __syncthreads();
    WSK(2);   // the workgroup's last wave is done
    for (int round = 0; round < 2; ++round) {
        if ((wave >> 1) == round) {
            float *img = red + (wave & 1) * P;
            // this lane's values and their flat indices, in a fixed order
            auto each = [&](auto &&f) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int orow = 4 * g + r;   // row of a 16x16 tile held in register r
#pragma unroll
                    for (int to = 0; to < 4; ++to)
#pragma unroll
                        for (int t = 0; t < 8; ++t) f(S64::w_off(0) + (16 * to + orow) * 128 + 16 * t + j, gW1[to][t][r], true);
#pragma unroll
                    for (int to = 0; to < 2; ++to)
#pragma unroll
                        for (int t = 0; t < 4; ++t) f(S64::w_off(1) + (16 * to + orow) * 64 + 16 * t + j, gW2[to][t][r], true);
#pragma unroll
                    for (int t = 0; t < 2; ++t) f(S64::w_off(2) + orow * 32 + 16 * t + j, gW3[0][t][r], true);
                    f(S64::w_off(3) + min(orow, 7) * 16 + j, gW4[0][0][r], orow < 8);
                    f(WO + min(orow, 8), gO[r], j == 0 && orow <= 8);   // w_out (8), then b_out
                }
            };
            if (round == 0) {
                each([&](int idx, float v, bool ok) { if (ok) img[idx] = v; });
                each_bias([&](int idx, float v, bool ok) { if (ok) img[idx] = v; });
            } else {
                each_bias([&](int idx, float v, bool ok) { if (ok) img[idx] = img[idx] + v; });   // one adder per image and address: read a group, add, store (a round trip per group)
                auto group = [&](auto nv, auto &&idx_of, auto &&val_of, auto &&ok_of) {
                    constexpr int N = decltype(nv)::value;
                    float cur[N];
#pragma unroll
                    for (int q = 0; q < N; ++q) cur[q] = ok_of(q) ? img[idx_of(q)] : 0.0f;
#pragma unroll
                    for (int q = 0; q < N; ++q)
                        if (ok_of(q)) img[idx_of(q)] = cur[q] + val_of(q);
                };
                using I32 = std::integral_constant<int, 32>;
                using I16 = std::integral_constant<int, 16>;
                using I8 = std::integral_constant<int, 8>;
                using I4 = std::integral_constant<int, 4>;
                auto yes = [](int) { return true; };
#pragma unroll
                for (int to = 0; to < 4; ++to)   // W1: (to, t, r)
                    group(I32{}, [&](int q) { return S64::w_off(0) + (16 * to + 4 * g + (q & 3)) * 128 + 16 * (q >> 2) + j; },
                          [&](int q) { return gW1[to][q >> 2][q & 3]; }, yes);
#pragma unroll
                for (int to = 0; to < 2; ++to)   // W2
                    group(I16{}, [&](int q) { return S64::w_off(1) + (16 * to + 4 * g + (q & 3)) * 64 + 16 * (q >> 2) + j; },
                          [&](int q) { return gW2[to][q >> 2][q & 3]; }, yes);
                group(I8{}, [&](int q) { return S64::w_off(2) + (4 * g + (q & 3)) * 32 + 16 * (q >> 2) + j; },
                      [&](int q) { return gW3[0][q >> 2][q & 3]; }, yes);
                group(I4{}, [&](int q) { return S64::w_off(3) + min(4 * g + q, 7) * 16 + j; },
                      [&](int q) { return gW4[0][0][q]; }, [&](int q) { return 4 * g + q < 8; });
                if (j == 0)   // the output row
                    group(I4{}, [&](int q) { return WO + min(4 * g + q, 8); },
                          [&](int q) { return gO[q]; }, [&](int q) { return 4 * g + q <= 8; });
            }
        }
        __syncthreads();
        WSK(3 + round);   // round 0 stored, round 1 added
    }
    for (int e = tid; e < P; e += kThreads) a.wpart[(int64_t)blockIdx.x * P + e] = red[e] + red[P + e];
    WSK(5);   // kernel exit
}

template <int PHASE>
static int wave_launch(NcfArgs &a, hipStream_t s, int blocks) {
    const size_t lds = (size_t)ncfw::kLdsFloats * sizeof(float);
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void *>(ncf_wave_kernel<PHASE>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
    if (!attr) return fail_arg("ncf_wave_kernel: cannot reserve LDS");
    hipLaunchKernelGGL((ncf_wave_kernel<PHASE>), dim3(blocks), dim3(ncfw::kThreads), lds, s, a);
    return check_launch("rg_ncf_pairs");
}

int ncf_wave_launch(NcfArgs &a, hipStream_t s, int blocks, int phase) {
    return dispatch_ncf_phase(phase, [&](auto ph) { return wave_launch<decltype(ph)::value>(a, s, blocks); });
}

}  // namespace rg
