// NCF / NeuMF training step, the workgroup-per-tile kernel ncf_pairs_kernel<E, PHASE>: every tower
// but the E = 64 MLP (rg_ncf_wave.hip), and every NeuMF.  rg_ncf.hip describes it with the step.
#include "rg_ncf.h"
#include "rg_mfma.h"

namespace rg {

constexpr int kNcfThreads = 256;

// the kernel's LDS float offsets: padded weights, activations, multipliers, dW, misc
template <int E>
struct NcfShape : NcfTower<E> {
    using T = NcfTower<E>;
    using T::H;
    using T::NH;
    using T::P;
    static constexpr int sw_off(int k) {
        int o = 0;
        for (int j = 0; j < k; ++j) o += H(j + 1) * (H(j) + 1) + H(j + 1);
        return o;
    }
    static constexpr int SW = sw_off(NH) + 9;
    static constexpr int sa_off(int k) {
        int o = 0;
        for (int j = 0; j < k; ++j) o += kRows * (H(j) + 1);
        return o;
    }
    static constexpr int SA = sa_off(NH + 1);
    static constexpr int LDS = SW + SA + SA + P + 13 * kRows + 8;   // W, A, M(=A layout), dW, misc
    // NeuMF extra floats: dW (M more), output GMF weights (M), GMF rows unless they fit
    // the dX region (M <= E: row stride 2E + 1 holds U_mf | I_mf)
    static constexpr int lds_neumf(int M) { return M == 0 ? LDS : LDS + 2 * M + (M <= E ? 0 : kRows * (2 * M + 1)); }
};

// Diagnostic build only (RG_DIAG_STAMPS): s_memrealtime at the tile phase boundaries of
// the first two tiles of every workgroup (thread 0, after the phase's barrier), for
// scripts/ncf_stamps.py.  The product library has no stamp code.
#ifdef RG_DIAG_STAMPS
__device__ unsigned long long *g_ncf_stamps;
int ncf_tile_set_stamps(unsigned long long *dev_buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_ncf_stamps), &dev_buf, sizeof(dev_buf)) == hipSuccess ? RG_OK : RG_E_LAUNCH;
}
#define NS(k)                                                                                       \
    do {                                                                                             \
        if (g_ncf_stamps && threadIdx.x == 0 && tl_ < 2) {                                           \
            unsigned long long t_;                                                                   \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
            g_ncf_stamps[((int64_t)blockIdx.x * 2 + tl_) * 8 + (k)] = t_;                            \
        }                                                                                            \
    } while (0)
#else
#define NS(k) \
    do {      \
    } while (0)
#endif

// C tile (16x16 at i0, j0) of A.B on LDS operands, K a compile-time multiple of 4.
// A(i, k) = A[i * ai + k * ak], B(k, j) = B[k * bk + j * bj]; rows >= imax / cols >= jmax read 0.
// Every operand of the tile is read first (one batch of LDS reads; rows outside the
// tile read row 0 and are zeroed after), then the K/4 MFMAs issue over four
// independent accumulators: no LDS round trip or MFMA dependency between
// consecutive MFMAs.
template <int K, int KB = K>
__device__ __forceinline__ v4f mma16(const float *A, int ai, int ak, const float *B, int bk, int bj, int i0, int j0,
                                     int imax, int jmax, int lane) {
    // KB: K values read per batch (a multiple of 16 dividing K); the accumulator sequence,
    // and so the result, does not depend on it
    constexpr int NK = K / 4, NB = (KB < K ? KB : K) / 4;
    static_assert(NK % NB == 0 && NB % 4 == 0 || NB == NK, "batch shape");
    const int li = lane & 15, lk = lane >> 4;
    const bool iv = i0 + li < imax, jv = j0 + li < jmax;
    const float *pa = A + (iv ? (i0 + li) : 0) * ai + lk * ak;
    const float *pb = B + lk * bk + (jv ? (j0 + li) : 0) * bj;
    v4f acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s0 = 0; s0 < NK; s0 += NB) {
        float av[NB], bv[NB];
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            av[s] = pa[4 * (s0 + s) * ak];
            bv[s] = pb[4 * (s0 + s) * bk];
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the read batch ahead of the MFMAs
#pragma unroll
        for (int s = 0; s < NB; ++s)
            acc[(s0 + s) & 3] =
                __builtin_amdgcn_mfma_f32_16x16x4f32(iv ? av[s] : 0.0f, jv ? bv[s] : 0.0f, acc[(s0 + s) & 3], 0, 0, 0);
    }
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

template <int E>
constexpr int ncf_threads() { return E >= 64 ? 512 : kNcfThreads; }

template <int E, int PHASE>
__global__ __launch_bounds__(ncf_threads<E>()) void ncf_pairs_kernel(NcfArgs a) {
    constexpr int kNT = ncf_threads<E>(), kNW = kNT / 64;
    constexpr int kKB = kNT > kNcfThreads ? 32 : 1024;   // MFMA operand batch (K values): registers for 2 waves / SIMD
    using S = NcfShape<E>;
    constexpr int NH = S::NH, IN0 = 2 * E;
    const int M = a.mf_dim, P = S::P + M;  // flat parameters: tower, output W (8 + M), output b
    constexpr int WO = S::w_off(NH);       // flat offset of the output layer
    extern __shared__ float lds[];
    float *sW = lds;                      // padded weights
    float *sA = sW + S::SW;               // activations A_0 .. A_NH, [kRows][H_k + 1]
    float *sM = sA + S::SA;               // multipliers / deltas, same layout as sA (k >= 1)
    float *sP = sM + S::SA;               // p per row
    float *sDz = sP + kRows;              // dL/dlogit per row
    int *sU = reinterpret_cast<int *>(sDz + kRows);
    int *sI = sU + kRows;
    int *sR = sI + kRows;                 // per row: reference row of its mask (pos: column, neg: draw j)
    uint32_t *sK = reinterpret_cast<uint32_t *>(sR + kRows);   // per row: dropout hash key
    float *sLa = reinterpret_cast<float *>(sK + kRows);        // per column loss terms
    float *sLb = sLa + kRows;
    int *sLu = reinterpret_cast<int *>(sLb + kRows);          // per row: user list slot (-1: none)
    int *sLi = sLu + kRows;                                   // per row: item list slot (-1: none / planned)
    int *sPs = sLi + kRows;                                   // per row: plan slot of a positive (-1: none)
    float *sX = sM + S::sa_off(0);                            // dX rows [kRows][IN0 + 1] (M_0 is unused)
    int *sUn = sPs + kRows;                                   // next tile's ids (E = 64: written, never read)
    int *sIn = sUn + kRows;
    float *sG = reinterpret_cast<float *>(sIn + kRows) + 8;   // weight-gradient accumulator (flat, P)
    float *sWm = sG + P;                                      // NeuMF output weights of the GMF units
    // NeuMF GMF rows: U_mf at [r * gs], I_mf at [r * gs + M] (dX region, free until the tower's last backward)
    const int gs = M <= E ? IN0 + 1 : 2 * M + 1;
    float *sGm = M <= E ? sX : sWm + M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr bool kBackward = PHASE != kNcfScores && PHASE != kNcfLossOnly;
    const int n = a.n_neg, NP = n + 1, tc = a.tc;
    // E = 64 training (8 waves, a CU's LDS alone): ids and list slots run one tile ahead.  The
    // next tile's pair ids are loaded at this tile's start and its list slots claimed during
    // this tile's backward, so the atomics' round trip is off the next tile's path; the A_0
    // rows are gathered at the tile's start.  The small towers keep their registers for
    // occupancy (several tiles per CU).
    constexpr bool kPipe = E >= 64 && kBackward;
    bool pre_ok = false;                  // registers hold this tile's ids and slots
    int nu = -1, ni = -1, nps = -1, nlu = -1, nli = -1, ncol = 0;

    // ---- parameters into LDS (row stride H_k + 1), gradient accumulator zeroed ----
    for (int k = 0; k < NH; ++k) {
        const int in = S::H(k), out = S::H(k + 1);
        const float *W = a.mlp + S::w_off(k);
        float *dst = sW + S::sw_off(k);
        for (int e = tid; e < out * in; e += kNT) dst[(e / in) * (in + 1) + e % in] = W[e];
        for (int e = tid; e < out; e += kNT) dst[out * (in + 1) + e] = W[out * in + e];
    }
    for (int e = tid; e < 9; e += kNT) sW[S::sw_off(NH) + e] = a.mlp[WO + (e < 8 ? e : 8 + M)];
    for (int e = tid; e < M; e += kNT) sWm[e] = a.mlp[WO + 8 + e];
    for (int e = tid; e < P; e += kNT) sG[e] = 0.0f;
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int tl_ = (int)((tile - blockIdx.x) / gridDim.x);
        NS(0);
        const int64_t c0 = tile * tc;
        // ---- row ids: row r = q * tc + cl ----------------------------------------------
        if (tid < kRows) {
            const int r = tid, q = r / tc, cl = r % tc;
            const int64_t s = c0 + cl;
            const bool pairwise = a.loss == RG_LOSS_BPR || a.loss == RG_LOSS_HINGE;
            bool valid = q < NP && s < a.cols;
            if (valid && q == 0) valid = s < a.n_pos;
            if (valid && q > 0 && pairwise) valid = s < a.n_pos;
            int u = -1, i = -1;
            if (kPipe && pre_ok) {
                u = nu;
                i = ni;
            } else if (valid) {
                const int2 pr = a.pairs[s * pair_stride(a.n_neg) + q];
                u = pr.x;
                i = pr.y;
            }
            sU[r] = u;
            sI[r] = i;
            // the example's identity for dropout: recorded-mask row, or the hash key
            const int64_t colid = (kPipe && pre_ok) ? (int64_t)ncol : a.perm && s < a.cols ? (int64_t)a.perm[s] : s;
            // (global: a data-parallel rank's column slice keys its examples as the single
            // process at the global batch does -- draw index, or column for the positive)
            const int64_t gj = q == 0 ? a.col_offset + colid : (int64_t)(q - 1) * a.global_cols + a.col_offset + colid;
            sR[r] = (int)gj;
            sK[r] = hash32(a.seed ^ ((uint64_t)(q == 0 ? 0 : 1) << 40) ^ ((uint64_t)gj * 0x9E3779B97F4A7C15ULL));
            // list slots are claimed now (the entry does not depend on the gradient), so the
            // atomics' round trip overlaps the gather; overflow rows add from LDS at the end
            int lu = -1, li = -1, ps = -1;
            if (kPipe && pre_ok) {
                // slots claimed during the previous tile's backward; their entries are
                // written now that the atomics have long returned
                lu = nlu;
                li = nli;
                ps = nps;
                const int64_t ex = tile * kRows + r;
                if (lu >= 0 && lu < kNcfCap) store_entry(a.row_list + (int64_t)u * kNcfCap + lu, (int)ex, 1.0f);
                if (li >= 0 && li < kNcfCap)
                    store_entry(a.row_list + (a.num_users + i) * kNcfCap + li, (int)ex, 1.0f);
            } else if (kBackward && u >= 0) {
                const int64_t ex = tile * kRows + r;
                lu = atomicAdd(a.row_count + u, 1);
                if (lu < kNcfCap) store_entry(a.row_list + (int64_t)u * kNcfCap + lu, (int)ex, 1.0f);
                if (q == 0 && a.pos_slot != nullptr) {
                    ps = a.pos_slot[s];
                } else {
                    const int64_t row = a.num_users + i;
                    li = atomicAdd(a.row_count + row, 1);
                    if (li < kNcfCap) store_entry(a.row_list + row * kNcfCap + li, (int)ex, 1.0f);
                }
            }
            sLu[r] = lu;
            sLi[r] = li;
            sPs[r] = ps;
            if constexpr (kPipe) {      // the next tile's record entries, consumed at backward start
                nu = ni = -1;
                const int64_t nt = tile + gridDim.x, s2 = nt * tc + cl;
                bool v2 = nt < a.tiles && q < NP && s2 < a.cols;
                if (v2 && q == 0) v2 = s2 < a.n_pos;
                if (v2 && q > 0 && pairwise) v2 = s2 < a.n_pos;
                if (v2) {
                    const int2 pr = a.pairs[s2 * pair_stride(a.n_neg) + q];
                    nu = pr.x;
                    ni = pr.y;
                }
                nps = (v2 && q == 0 && a.pos_slot != nullptr) ? a.pos_slot[s2] : -1;
                ncol = (int)(a.perm && s2 < a.cols ? (int64_t)a.perm[s2] : s2);
            }
        }
        __syncthreads();
        NS(1);
        // ---- gather A_0 = [U[u] | I[i]] ------------------------------------------------
        for (int e = tid; e < kRows * (IN0 / 4); e += kNT) {
            const int r = e / (IN0 / 4), c4 = (e % (IN0 / 4)) * 4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (sU[r] >= 0)
                v = c4 < E ? *reinterpret_cast<const float4 *>(a.user_w + (int64_t)sU[r] * E + c4)
                           : *reinterpret_cast<const float4 *>(a.item_w + (int64_t)sI[r] * E + (c4 - E));
            float *d = sA + r * (IN0 + 1) + c4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        for (int e = tid; e < kRows * 2 * M; e += kNT) {      // NeuMF GMF rows
            const int r = e / (2 * M), c = e % (2 * M);
            float v = 0.0f;
            if (sU[r] >= 0)
                v = c < M ? a.mf_user_w[(int64_t)sU[r] * M + c] : a.mf_item_w[(int64_t)sI[r] * M + (c - M)];
            sGm[r * gs + c] = v;
        }
        __syncthreads();
        NS(2);
        // ---- forward hidden layers ---------------------------------------------------------
        static_for<NH>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            constexpr int in = S::H(k), out = S::H(k + 1), mask_base = S::mask_off(k);
            const float *Ak = sA + S::sa_off(k);
            float *An = sA + S::sa_off(k + 1);
            float *Mn = sM + S::sa_off(k + 1);
            const float *Wk = sW + S::sw_off(k);
            const float *bk = Wk + out * (in + 1);
            constexpr int ct = out < 16 ? 1 : out / 16;
            for (int t = wave; t < 2 * ct; t += kNW) {
                const int i0 = (t / ct) * 16, j0 = (t % ct) * 16;
                const v4f z = mma16<in, kKB>(Ak, in + 1, 1, Wk, 1, in + 1, i0, j0, kRows, out, lane);
                const int col = j0 + (lane & 15);
                if (col < out) {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int row = i0 + (lane >> 4) * 4 + rr;
                        const float zz = z[rr] + bk[col];
                        float m = zz > 0.0f ? 1.0f : 0.1f;
                        if (a.training) {
                            bool keep;
                            if (a.mask_pos) {
                                const int units = S::mask_units();
                                const uint8_t *mk = row < tc ? a.mask_pos : a.mask_neg;
                                keep = sU[row] >= 0 && mk[(int64_t)sR[row] * units + mask_base + col] != 0;
                            } else {
                                keep = (mix32(sK[row] + (uint32_t)(mask_base + col) * 0x85EBCA6BU) >> 7) & 1U;
                            }
                            m = keep ? 2.0f * m : 0.0f;
                        }
                        An[row * (out + 1) + col] = zz * m;
                        Mn[row * (out + 1) + col] = m;
                    }
                }
            }
            __syncthreads();
            if (k == 0) NS(3);
        });
        // ---- output layer, scores, loss ---------------------------------------------------
        {
            const float *wo = sW + S::sw_off(NH);
            const float *AN = sA + S::sa_off(NH);
            if (tid < kRows) {
                float d = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) d = fmaf(AN[tid * 9 + j], wo[j], d);
                const float *gu = sGm + tid * gs;
#pragma unroll 8
                for (int c = 0; c < M; ++c) d = fmaf(gu[c] * gu[M + c], sWm[c], d);   // GMF = U_mf * I_mf
                const float p = sigmoidf_ref(d + wo[8]);
                sP[tid] = p;
                sDz[tid] = 0.0f;   // rows no column writes below keep dz = 0
                if (PHASE == kNcfScores) a.scores[tile * kRows + tid] = sU[tid] >= 0 ? p : 0.0f;
            }
        }
        __syncthreads();
        NS(4);
        if (PHASE == kNcfScores) continue;
        // dL/dlogit per row (columns: one thread each) and the tile's loss partials
        if (tid < tc) {
            float la = 0.0f, lb = 0.0f;
            {
                const int cl = tid;
                // loops over the column's pairs run to the compile-time bound with a guard (the
                // loads come from a clamped row), so dp[] stays in registers and the LDS
                // reads of all pairs issue together
                constexpr int QM = RG_MF_MAX_NEG + 1;
                float dp[QM];
#pragma unroll
                for (int q = 0; q < QM; ++q) dp[q] = 0.0f;
                const int r0 = cl;
                const bool has_pos = sU[r0] >= 0;
                if (PHASE == kNcfGivenDp) {
#pragma unroll
                    for (int q = 0; q < QM; ++q)
                        if (q < NP && sU[q * tc + cl] >= 0) dp[q] = a.dp_in[tile * kRows + q * tc + cl];
                } else if (a.loss == RG_LOSS_POINTWISE) {
                    if (has_pos) {
                        const float p = sP[r0];
                        la += -fmaxf(logf(p), -100.0f);
                        dp[0] = ((p - 1.0f) / fmaxf((1.0f - p) * p, 1e-12f)) / a.n_a;
                    }
#pragma unroll
                    for (int q = 1; q < QM; ++q) {
                        const int r = min(q * tc + cl, kRows - 1);
                        const bool ok = q < NP && sU[r] >= 0;
                        const float p = sP[r];
                        if (ok) {
                            lb += -fmaxf(logf(1.0f - p), -100.0f);
                            dp[q] = (p / fmaxf((1.0f - p) * p, 1e-12f)) / a.n_b;
                        }
                    }
                } else if (has_pos) {   // bpr / hinge on the neg.view(n, B) pairing
                    const float g = 1.0f / a.n_a, pp = sP[r0];
#pragma unroll
                    for (int q = 1; q < QM; ++q) {
                        const int r = min(q * tc + cl, kRows - 1);
                        if (q >= NP || sU[r] < 0) continue;
                        if (a.loss == RG_LOSS_BPR) {
                            const float sg = sigmoidf_ref(pp - sP[r]);
                            la += 1.0f - sg;
                            const float dx = (-g) * (1.0f - sg) * sg;
                            dp[0] += dx;
                            dp[q] = -dx;
                        } else {
                            const float x = (sP[r] - pp) + 1.0f;
                            la += fmaxf(x, 0.0f);
                            const float dx = x >= 0.0f ? g : 0.0f;
                            dp[0] -= dx;
                            dp[q] = dx;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < QM; ++q) {
                    const int r = min(q * tc + cl, kRows - 1);
                    const float p = sP[r];
                    if (q < NP) sDz[r] = sU[r] >= 0 ? (dp[q] * (1.0f - p)) * p : 0.0f;
                }
            }
            sLa[tid] = la;
            sLb[tid] = lb;
        }
        __syncthreads();
        if (tid == 0) {     // column order, as the one-thread loop summed them
            float la = 0.0f, lb = 0.0f;
            for (int cl = 0; cl < tc; ++cl) { la += sLa[cl]; lb += sLb[cl]; }
            a.loss_partials[2 * tile] = la;
            a.loss_partials[2 * tile + 1] = lb;
        }
        // (no barrier: thread 0 only reads sLa / sLb, rewritten at the next tile's loss phase)
        NS(5);
        if (PHASE == kNcfLossOnly) continue;         // validation: loss only (run_val_iteration)
        // ---- backward ------------------------------------------------------------------------
        const bool has_next = tile + gridDim.x < a.tiles;
        if constexpr (kPipe) {
            if (tid < kRows && has_next) {
                const int r = tid, q = r / tc;
                nlu = nli = -1;
                if (nu >= 0) {   // entries are written at the next tile's start (results not waited on here)
                    nlu = atomicAdd(a.row_count + nu, 1);
                    if (!(q == 0 && a.pos_slot != nullptr)) nli = atomicAdd(a.row_count + a.num_users + ni, 1);
                }
                sUn[r] = nu;   // dead stores since the A_0 prefetch that read them went; kept: DESIGN §9
                sIn[r] = ni;
            }
        }
        {
            // output layer: dW_out += sum_r dz_r A_NH[r], db_out += sum_r dz_r; G_NH = dz w_out^T
            const float *wo = sW + S::sw_off(NH);
            const float *AN = sA + S::sa_off(NH);
            float *MN = sM + S::sa_off(NH);
            for (int e = tid; e < 9 + M; e += kNT) {     // e: 8 tower units, bias, M GMF units
                float acc = 0.0f;
                auto term = [&](int r) {
                    return e < 8 ? AN[r * 9 + e] : e == 8 ? 1.0f : sGm[r * gs + e - 9] * sGm[r * gs + M + e - 9];
                };
                // in row order; E = 64 reads the operands in batches of kCh (one LDS round
                // trip per batch), the small towers one by one (their registers buy occupancy)
                if constexpr (E >= 64) {
                    constexpr int kCh = 8;
#pragma unroll 1
                    for (int r0 = 0; r0 < kRows; r0 += kCh) {
                        float dz[kCh], tv[kCh];
#pragma unroll
                        for (int r = 0; r < kCh; ++r) {
                            dz[r] = sDz[r0 + r];
                            tv[r] = term(r0 + r);
                        }
#pragma unroll
                        for (int r = 0; r < kCh; ++r) acc = fmaf(dz[r], tv[r], acc);
                    }
                } else {
                    for (int r = 0; r < kRows; ++r) acc = fmaf(sDz[r], term(r), acc);
                }
                sG[WO + (e < 8 ? e : e == 8 ? 8 + M : e - 1)] += acc;
            }
            for (int e = tid; e < kRows * 8; e += kNT) {
                const int r = e / 8, j = e % 8;
                MN[r * 9 + j] = (sDz[r] * wo[j]) * MN[r * 9 + j];      // delta_{NH-1} = G * m
            }
            if (M > 0) {
                // GMF backward: dU_mf = (dz w_c) I_mf, dI_mf = (dz w_c) U_mf (neuMF.py:43-50 under autograd)
                for (int e = tid; e < kRows * M; e += kNT) {
                    const int r = e / M, c = e % M;
                    const float dg = sDz[r] * sWm[c];
                    const float du = dg * sGm[r * gs + M + c], di = dg * sGm[r * gs + c];
                    float *row = a.mf_contrib + (tile * kRows + r) * (int64_t)(2 * M);
                    row[c] = du;
                    row[M + c] = di;
                    if (sLu[r] >= kNcfCap) fix_add(a.mf_hot_grad + (int64_t)sU[r] * M + c, du);
                    if (sLi[r] >= kNcfCap) fix_add(a.mf_hot_grad + (a.num_users + sI[r]) * M + c, di);
                }
                if (a.pos_slot != nullptr) {
                    for (int e = tid; e < tc * M; e += kNT) {
                        const int cl = e / M, c = e % M;
                        const int slot = sPs[cl];
                        if (slot < 0 || (cl > 0 && sPs[cl - 1] == slot)) continue;
                        float acc = 0.0f;
                        for (int cc = cl; cc < tc && sPs[cc] == slot; ++cc)
                            acc += (sDz[cc] * sWm[c]) * sGm[cc * gs + c];
                        a.mf_part_row[(int64_t)slot * M + c] = acc;
                    }
                }
            }
            __syncthreads();
        }
        if constexpr (kPipe) {
            pre_ok = has_next;
        }
        static_for<NH>([&](auto kc) {
            constexpr int k = NH - 1 - decltype(kc)::value;
            constexpr int in = S::H(k), out = S::H(k + 1);
            const float *Ak = sA + S::sa_off(k);
            const float *Dk = sM + S::sa_off(k + 1);     // delta_k: [kRows][out + 1]
            const float *Wk = sW + S::sw_off(k);
            float *gW = sG + S::w_off(k);
            // dW_k (out x in) += delta^T A_k ; db_k += column sums of delta
            constexpr int ro = out < 16 ? 1 : out / 16, ci = in / 16;
            for (int t = wave; t < ro * ci; t += kNW) {
                const int i0 = (t / ci) * 16, j0 = (t % ci) * 16;
                const v4f c = mma16<kRows>(Dk, 1, out + 1, Ak, in + 1, 1, i0, j0, out, in, lane);
                const int col = j0 + (lane & 15);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int o = i0 + (lane >> 4) * 4 + rr;
                    if (o < out) gW[o * in + col] += c[rr];
                }
            }
            for (int o = tid; o < out; o += kNT) {
                float acc = 0.0f;
                if constexpr (E >= 64) {   // batches of LDS reads, then the same in-order sum
                    constexpr int kCh = 8;
#pragma unroll 1
                    for (int r0 = 0; r0 < kRows; r0 += kCh) {
                        float col[kCh];
#pragma unroll
                        for (int r = 0; r < kCh; ++r) col[r] = Dk[(r0 + r) * (out + 1) + o];
#pragma unroll
                        for (int r = 0; r < kCh; ++r) acc += col[r];
                    }
                } else {
                    for (int r = 0; r < kRows; ++r) acc += Dk[r * (out + 1) + o];
                }
                gW[out * in + o] += acc;
            }
            // dA_k = delta W_k (kRows x in): k > 0 -> delta_{k-1} = dA * m_k ; k == 0 -> dX
            constexpr int cj = in / 16;
            for (int t = wave; t < 2 * cj; t += kNW) {
                const int i0 = (t / cj) * 16, j0 = (t % cj) * 16;
                const v4f c = mma16<(out < 4 ? 4 : out), kKB>(Dk, out + 1, 1, Wk, in + 1, 1, i0, j0, kRows, in, lane);
                const int col = j0 + (lane & 15);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int row = i0 + (lane >> 4) * 4 + rr;
                    if constexpr (k > 0) {
                        float *Mk = sM + S::sa_off(k);
                        Mk[row * (in + 1) + col] = c[rr] * Mk[row * (in + 1) + col];
                    } else {
                        a.contrib[(tile * kRows + row) * (int64_t)IN0 + col] = c[rr];
                        sX[row * (IN0 + 1) + col] = c[rr];
                    }
                }
            }
            __syncthreads();
            if (k == NH - 1) NS(6);
        });
        // ---- embedding gradient: overflow rows (hot users/items), planned item partials -----------
        for (int e = tid; e < 2 * kRows * E; e += kNT) {
            const int r = e / (2 * E), half = (e / E) & 1, c = e % E;
            const int sl = half ? sLi[r] : sLu[r];
            if (sl >= kNcfCap) {
                const int64_t row = half ? a.num_users + sI[r] : (int64_t)sU[r];
                fix_add(a.hot_grad + row * E + c, sX[r * (IN0 + 1) + half * E + c]);
            }
        }
        if (a.pos_slot != nullptr) {
            // positives' item halves, same plan slot -> one partial row (fixed order, plain stores)
            for (int e = tid; e < tc * E; e += kNT) {
                const int cl = e / E, c = e % E;
                const int slot = sPs[cl];
                if (slot < 0 || (cl > 0 && sPs[cl - 1] == slot)) continue;   // not the segment head
                float acc = 0.0f;
                for (int cc = cl; cc < tc && sPs[cc] == slot; ++cc) acc += sX[cc * (IN0 + 1) + E + c];
                a.part_row[(int64_t)slot * E + c] = acc;
            }
        }
        __syncthreads();
        NS(7);
    }
    // ---- the workgroup's weight-gradient partial ------------------------------------------------
    if (kBackward)
        for (int e = tid; e < P; e += kNT) a.wpart[(int64_t)blockIdx.x * P + e] = sG[e];
}

template <int E, int PHASE>
static int tile_launch(NcfArgs &a, hipStream_t s, int blocks) {
    const int need = NcfShape<E>::lds_neumf(a.mf_dim);
    if (need > kLdsMax) return fail_arg("rg_ncf_pairs: NeuMF mf_dim too large for this embedding_dim (LDS)");
    const size_t lds = (size_t)need * sizeof(float);
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void *>(ncf_pairs_kernel<E, PHASE>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 kLdsMax * (int)sizeof(float)) == hipSuccess;
    if (!attr) return fail_arg("ncf_pairs_kernel: cannot reserve LDS");
    hipLaunchKernelGGL((ncf_pairs_kernel<E, PHASE>), dim3(blocks), dim3(ncf_threads<E>()), lds, s, a);
    return check_launch("rg_ncf_pairs");
}

int ncf_tile_launch(NcfArgs &a, hipStream_t s, int blocks, int E, int phase) {
    return dispatch_ncf_phase(phase, [&](auto ph) {
        return dispatch_ncf_dim(E, [&](auto e) { return tile_launch<decltype(e)::value, decltype(ph)::value>(a, s, blocks); });
    });
}

int ncf_tile_lds_floats(int E, int M) {
    return dispatch_ncf_dim(E, [&](auto e) { return NcfShape<decltype(e)::value>::lds_neumf(M); });
}

}  // namespace rg
