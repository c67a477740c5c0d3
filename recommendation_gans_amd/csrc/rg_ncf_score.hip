// NCF / NeuMF inference: eval-mode scores (no dropout) of a block of users against EVERY item
// (spotlight/dnn_models/mlp.py:30-41, neuMF.py:34-55), the score block the evaluation metrics
// and predict(user) rank (spotlight/evaluation.py: _scored, _topk_hits).
//
// Items are contiguous and the first (widest) layer separates:
//     W1 [u; i] + b1 = (W1[:, :E] u + b1) + W1[:, E:] i = Hu[u] + Hi[i],
// one vector per user and one per item, neither depending on the pair.  Two launches:
//
//   halves   Hi [I][E] = item_w W1[:, E:]^T,  Hu [nu][E] = user_w[users] W1[:, :E]^T + b1 and, for
//            NeuMF, Gu [nu][MP] = affine_w[8:] * mf_user_w[users] (MP = M rounded up to 4, zero
//            padded), so the GMF term of the logit is the plain dot Gu[u] . mf_item_w[i].
//   scores   grid (item tile of 64, group of 64 users), 4 waves; wave w owns the group's users
//            [16 w, 16 w + 16).  A lane (g = lane / 16, j = lane % 16) keeps its slice of the
//            tile's Hi rows in registers for every user (item 16 nb + j of block nb, features
//            16 t + 4 g .. + 3: the MFMA's B / C layout, as ncfw::fwd1 of rg_ncf_wave.hip), so per
//            (user, 16 items) the first layer is an add and a LeakyReLU.  The narrow layers
//            E -> E/2 -> .. -> 8 run on __builtin_amdgcn_mfma_f32_16x16x4f32 with the weights in
//            LDS (row-major [out][in + 4], the 8-wide layer padded to 16 rows of zeros), each
//            layer's C tiles being the next layer's B operand with no shuffle.  The output dot
//            (8 wide; the whole tower for E = 8) is VALU: four products per lane and a sum over
//            the four lane groups.  The wave collects the 16 users' logits in the C layout of a
//            (16 users x 16 items) tile -- which is where the GMF product Gu . mf_item^T of the
//            same 16 users lands as M / 4 more MFMAs (mf_item rows of the tile staged in LDS once)
//            -- then adds the bias, takes the sigmoid once per pair (precise expf, sigmoidf_ref)
//            and stores out[u][i]: 16 consecutive items (64 B) per user and lane group.
//
// fp32 throughout, the model is only read, every sum has a fixed order (no atomics): two calls
// give the same bits.  Item tails and the last user group are masked; out's padding columns
// [I, ld) are not written.
//
// Arbitrary (user, item) pairs (predict(users, items)) cannot split the first layer; they have a
// kernel of their own below (rg_ncf_score_pairs), which shares the tower and the LDS weight layout.
#include <climits>

#include "rg_ncf.h"
#include "rg_mfma.h"

namespace rg {
namespace {

constexpr int kTile = RG_NCF_SCORE_ITEM_TILE, NB = kTile / 16;
constexpr int kWaves = 4, kThreads = 64 * kWaves, kGroup = 16 * kWaves;
static_assert(kGroup == RG_NCF_SCORE_USER_GROUP && kTile % 16 == 0, "header constants");
constexpr int kHalfRows = 64;     // rows of Hi / Hu per workgroup of the halves pass

__host__ __device__ constexpr int pad4(int m) { return (m + 3) & ~3; }
// row stride of the staged mf_item rows: MP + 2, so the 16 rows x 2 k-columns a 32-lane half reads
// (ds_read_b32, 32 banks) fall on 32 distinct banks ((MP + 2) / 2 is odd)
__host__ __device__ constexpr int im_stride(int mp) { return mp + 2; }

// layer k maps H(k) = 2E >> k features to H(k + 1); k = 0 is the split layer, k = NH the output
template <int E>
struct Shape : NcfTower<E> {
    using NcfTower<E>::H;
    // a layer in LDS: row-major [rows(k)][S(k)], the rows padded to 16 with zeros
    static constexpr int tiles(int k) { return H(k) < 16 ? 1 : H(k) / 16; }   // 16-feature tiles of layer k's input
    static constexpr int rows(int k) { return 16 * tiles(k + 1); }
    static constexpr int S(int k) { return H(k) + 4; }
};

// LDS (floats) of a kernel whose first MFMA layer is K0: the weights of layers K0 .. NH - 1, their
// biases, the 16-float output row; what the kernel stages of its own starts at `end`
template <int E, int K0>
struct TowerLds {
    using S = Shape<E>;
    static constexpr int lw_off(int k) {
        int o = 0;
        for (int j = K0; j < k; ++j) o += S::rows(j) * S::S(j);
        return o;
    }
    static constexpr int lb_off(int k) {
        int o = lw_off(S::NH);
        for (int j = K0; j < k; ++j) o += S::rows(j);
        return o;
    }
    static constexpr int oWo = lb_off(S::NH), end = oWo + 16;
};

// a lane's four products of the 8-wide (padded 16) output dot
__device__ __forceinline__ float out_dot(v4f wo, v4f x) {
    return fmaf(wo[3], x[3], fmaf(wo[2], x[2], fmaf(wo[1], x[1], wo[0] * x[0])));
}

// sum over the four lane groups (lanes j, 16 + j, 32 + j, 48 + j), left in each of them
__device__ __forceinline__ float group_sum(float p) {
    p += __shfl_xor(p, 16);
    p += __shfl_xor(p, 32);
    return p;
}

__device__ __forceinline__ v4f lrelu(v4f z) {
    v4f y;
#pragma unroll
    for (int r = 0; r < 4; ++r) y[r] = z[r] > 0.0f ? z[r] : z[r] * 0.1f;
    return y;
}

struct HalvesArgs {
    const float *user_w, *item_w, *mlp, *mf_user_w;
    const int64_t *users;
    int64_t num_items, n_users;
    int M, MP;
    float *Hi, *Hu, *Gu;
};

// blocks [0, ceil(I / 64)): rows of Hi; the rest: rows of Hu (and Gu) of 64 users each.  Thread
// (row r = tid / E, feature e = tid % E): one k-ordered fmaf chain per output.
template <int E>
__global__ __launch_bounds__(kThreads) void ncf_score_halves_kernel(HalvesArgs a) {
    using S = Shape<E>;
    __shared__ float sWt[E * E];          // [k][e]: this half of W1, transposed
    __shared__ float sX[kHalfRows * (E + 1)];
    const int tid = threadIdx.x;
    const int64_t item_blocks = (a.num_items + kHalfRows - 1) / kHalfRows;
    const bool item_side = blockIdx.x < item_blocks;
    const int64_t r0 = (item_side ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - item_blocks) * kHalfRows;
    const int64_t nrows = item_side ? a.num_items : a.n_users;
    const float *W1 = a.mlp + S::w_off(0), *b1 = W1 + E * 2 * E;
    for (int idx = tid; idx < E * E; idx += kThreads) {
        const int e = idx / E, k = idx % E;
        sWt[k * E + e] = W1[e * 2 * E + (item_side ? E : 0) + k];
    }
    for (int idx = tid; idx < kHalfRows * E; idx += kThreads) {
        const int r = idx / E, k = idx % E;
        float x = 0.0f;
        if (r0 + r < nrows) x = item_side ? a.item_w[(r0 + r) * E + k] : a.user_w[a.users[r0 + r] * E + k];
        sX[r * (E + 1) + k] = x;
    }
    __syncthreads();
    const int e = tid % E;
    const float bias = item_side ? 0.0f : b1[e];
    float *dst = item_side ? a.Hi : a.Hu;
    for (int r = tid / E; r < kHalfRows && r0 + r < nrows; r += kThreads / E) {
        float acc = bias;
#pragma unroll 8
        for (int k = 0; k < E; ++k) acc = fmaf(sX[r * (E + 1) + k], sWt[k * E + e], acc);
        dst[(r0 + r) * E + e] = acc;
    }
    if (!item_side && a.M > 0) {
        const float *aw = a.mlp + S::w_off(S::NH) + 8;     // affine_output's GMF columns
        for (int idx = tid; idx < kHalfRows * a.MP; idx += kThreads) {
            const int r = idx / a.MP, c = idx % a.MP;
            if (r0 + r < nrows)
                a.Gu[(r0 + r) * a.MP + c] = c < a.M ? aw[c] * a.mf_user_w[a.users[r0 + r] * a.M + c] : 0.0f;
        }
    }
}

struct ScoreArgs {
    const float *mlp, *Hi, *Hu, *Gu, *mf_item_w;
    int64_t num_items, n_users, ld;
    int M, MP;
    float *out;
};

// layers K .. NH - 1 on the MFMA, x = layer K's input in the T layout (tile t, block nb, register
// r: feature 16 t + 4 g + r of item 16 nb + j); last = the 8 (padded 16) inputs of the output dot
// (K0: the kernel's first MFMA layer, which fixes the LDS layout; N: 16-column blocks per wave)
template <int E, int K0, int N, int K = K0>
__device__ __forceinline__ void tower(const v4f (&x)[Shape<E>::tiles(K)][N], v4f (&last)[N], const float *lds, int g,
                                      int m) {
    using S = Shape<E>;
    using L = TowerLds<E, K0>;
    if constexpr (K == S::NH) {
#pragma unroll
        for (int nb = 0; nb < N; ++nb) last[nb] = x[0][nb];
    } else {
        constexpr int TI = S::tiles(K), TO = S::tiles(K + 1), St = S::S(K);
        const float *W = lds + L::lw_off(K), *B = lds + L::lb_off(K);
        v4f y[TO][N];
#pragma unroll
        for (int t = 0; t < TO; ++t) {
            const v4f b = *reinterpret_cast<const v4f *>(B + 16 * t + 4 * g);
#pragma unroll
            for (int nb = 0; nb < N; ++nb) y[t][nb] = b;
        }
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) {
            v4f a[TO];
#pragma unroll
            for (int t = 0; t < TO; ++t) a[t] = *reinterpret_cast<const v4f *>(W + (16 * t + m) * St + 16 * ti + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < TO; ++t)
#pragma unroll
                    for (int nb = 0; nb < N; ++nb) y[t][nb] = mfma(a[t][r], x[ti][nb][r], y[t][nb]);
        }
#pragma unroll
        for (int t = 0; t < TO; ++t)
#pragma unroll
            for (int nb = 0; nb < N; ++nb) y[t][nb] = lrelu(y[t][nb]);
        tower<E, K0, N, K + 1>(y, last, lds, g, m);
    }
}

// the all-item kernel's LDS: the tower from layer 1, the group's Hu rows, the tile's mf_item rows
template <int E>
struct ScoreLds : TowerLds<E, 1> {
    static constexpr int oHu = TowerLds<E, 1>::end, oIm = oHu + kGroup * E;
    static constexpr int lds_floats(int mp) { return oIm + (mp ? kTile * im_stride(mp) : 0); }
};

template <int E>
__global__ __launch_bounds__(kThreads, 2) void ncf_score_kernel(ScoreArgs a) {
    using S = Shape<E>;
    using L = ScoreLds<E>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int64_t i0 = (int64_t)blockIdx.x * kTile, u0 = (int64_t)blockIdx.y * kGroup;
    const int SM = im_stride(a.MP);

    // ---- stage: the MFMA layers' weights and biases (zero padded), the output row, the group's Hu
    // rows, the tile's mf_item rows
    static_for<S::NH - 1>([&](auto kc) {
        constexpr int K = decltype(kc)::value + 1, in = S::H(K), out = S::H(K + 1), R = S::rows(K), St = S::S(K);
        const float *Wg = a.mlp + S::w_off(K);
        for (int idx = tid; idx < R * St; idx += kThreads) {
            const int r = idx / St, c = idx % St;
            lds[L::lw_off(K) + idx] = r < out && c < in ? Wg[r * in + c] : 0.0f;
        }
        for (int idx = tid; idx < R; idx += kThreads) lds[L::lb_off(K) + idx] = idx < out ? Wg[out * in + idx] : 0.0f;
    });
    if (tid < 16) lds[L::oWo + tid] = tid < 8 ? a.mlp[S::w_off(S::NH) + tid] : 0.0f;
    for (int idx = tid; idx < kGroup * E; idx += kThreads) {
        const int64_t u = u0 + idx / E;
        lds[L::oHu + idx] = u < a.n_users ? a.Hu[u * E + idx % E] : 0.0f;
    }
    if (a.M > 0)
        for (int idx = tid; idx < kTile * SM; idx += kThreads) {
            const int r = idx / SM, c = idx % SM;
            lds[L::oIm + idx] = i0 + r < a.num_items && c < a.M ? a.mf_item_w[(i0 + r) * a.M + c] : 0.0f;
        }
    const float bo = a.mlp[S::w_off(S::NH) + 8 + a.M];
    __syncthreads();                       // the only barrier: a wave without users may leave now
    const int64_t uw = u0 + wave * 16;     // this wave's first user
    if (uw >= a.n_users) return;

    // ---- this lane's slice of the tile's Hi rows (rows past I read row I - 1; masked at the store)
    constexpr int T0 = S::tiles(1);
    const int fcol = E >= 16 ? 4 * g : 4 * (g & 1);    // E = 8: lane groups 2, 3 repeat 0, 1 under zero weights
    v4f hi[T0][NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        int64_t item = i0 + 16 * nb + j;
        item = item < a.num_items ? item : a.num_items - 1;
#pragma unroll
        for (int t = 0; t < T0; ++t) hi[t][nb] = *reinterpret_cast<const v4f *>(a.Hi + item * E + 16 * t + fcol);
    }
    const v4f wo = *reinterpret_cast<const v4f *>(lds + L::oWo + 4 * g);

    // ---- the tower, one user at a time; acc[nb][r] = logit of (user uw + 4 g + r, item 16 nb + j)
    v4f acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int uu = 0; uu < 16; ++uu) {
        if (uw + uu >= a.n_users) break;               // wave-uniform
        const float *hu = lds + L::oHu + (wave * 16 + uu) * E;
        v4f x[T0][NB];
#pragma unroll
        for (int t = 0; t < T0; ++t) {
            const v4f h = *reinterpret_cast<const v4f *>(hu + 16 * t + fcol);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) x[t][nb] = lrelu(hi[t][nb] + h);
        }
        v4f last[NB];
        tower<E, 1, NB>(x, last, lds, g, j);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const float p = group_sum(out_dot(wo, last[nb]));
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[nb][r] = 4 * g + r == uu ? p : acc[nb][r];
        }
    }

    // ---- NeuMF: + Gu (16 users x MP) . mf_item^T (MP x 16 items) per block, into the same C tiles
    if (a.M > 0) {
        int64_t um = uw + j;
        um = um < a.n_users ? um : a.n_users - 1;
        const float *gp = a.Gu + um * a.MP + g;
        const float *ip = lds + L::oIm + j * SM + g;
        for (int k = 0; k < a.MP; k += 4) {
            const float av = gp[k];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma(av, ip[16 * nb * SM + k], acc[nb]);
        }
    }

    // ---- bias, sigmoid, store (64 B of consecutive items per user and lane group)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t u = uw + 4 * g + r;
        if (u >= a.n_users) continue;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int64_t item = i0 + 16 * nb + j;
            if (item < a.num_items) a.out[u * a.ld + item] = sigmoidf_ref(acc[nb][r] + bo);
        }
    }
}

// ---------------------------------------------------------------- arbitrary (user, item) pairs
// rg_ncf_score_pairs: nothing separates, so the first layer is a real 2E-wide product and runs on
// the MFMA like the rest.  A workgroup stages EVERY layer's weights in LDS once (the layout of the
// all-item kernel: row-major [out][in + 4], rows padded to 16 with zeros) and then walks tiles of
// RG_NCF_SCORE_PAIR_TILE pairs, tile = blockIdx.x, + gridDim.x, ...; wave w owns pairs
// [32 w, 32 w + 32) of a tile as two MFMA column blocks.  A lane (g, j) loads its slice of pair
// 16 nb + j's input straight from the tables in the B layout: features 16 t + 4 g .. + 3 of
// [user_w[u] | item_w[i]], one 16-byte load each, the four lane groups of a pair covering 64
// consecutive bytes of a row -- no LDS round trip and no shuffle.  After the tower the lane holds
// four products of the 8-wide output dot; NeuMF adds its share of the GMF term (columns c = g
// mod 4 of affine_w[8 + c] * mf_user_w[u][c] * mf_item_w[i][c], c ascending); two shuffles sum
// the four lane groups, then bias, sigmoid and one store per pair (lane group nb stores block nb:
// 64 consecutive bytes).  A pair's sums depend on its column only through which lane holds it,
// never on the tile, the wave or the batch: equal pairs give equal bits anywhere.
constexpr int kPairTile = RG_NCF_SCORE_PAIR_TILE, PNB = kPairTile / (16 * kWaves);
static_assert(PNB * 16 * kWaves == kPairTile && PNB >= 1 && PNB <= 4, "header constant");

// the pair kernel's LDS: the whole tower, the output row's GMF columns
template <int E>
struct PairLds : TowerLds<E, 0> {
    static constexpr int oAw = TowerLds<E, 0>::end;
    static constexpr int lds_floats(int mp) { return oAw + mp; }
};

struct PairArgs {
    const float *user_w, *item_w, *mlp, *mf_user_w, *mf_item_w;
    const int64_t *users, *items;
    int64_t n, tiles;
    int M, MP;
    float *out;
};

template <int E>
__global__ __launch_bounds__(kThreads, 2) void ncf_score_pairs_kernel(PairArgs a) {
    using S = Shape<E>;
    using L = PairLds<E>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;

    // ---- stage: every layer's weights and biases (zero padded), the output row, the GMF columns
    static_for<S::NH>([&](auto kc) {
        constexpr int K = decltype(kc)::value, in = S::H(K), out = S::H(K + 1), R = S::rows(K), St = S::S(K);
        const float *Wg = a.mlp + S::w_off(K);
        for (int idx = tid; idx < R * St; idx += kThreads) {
            const int r = idx / St, c = idx % St;
            lds[L::lw_off(K) + idx] = r < out && c < in ? Wg[r * in + c] : 0.0f;
        }
        for (int idx = tid; idx < R; idx += kThreads) lds[L::lb_off(K) + idx] = idx < out ? Wg[out * in + idx] : 0.0f;
    });
    const float *aff = a.mlp + S::w_off(S::NH);
    if (tid < 16) lds[L::oWo + tid] = tid < 8 ? aff[tid] : 0.0f;
    for (int idx = tid; idx < a.MP; idx += kThreads) lds[L::oAw + idx] = idx < a.M ? aff[8 + idx] : 0.0f;
    const float bo = aff[8 + a.M];
    __syncthreads();                       // the only barrier
    const v4f wo = *reinterpret_cast<const v4f *>(lds + L::oWo + 4 * g);
    const float *aw = lds + L::oAw;

    constexpr int T0 = S::tiles(0);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t p0 = tile * kPairTile + wave * (16 * PNB);      // this wave's first pair
        if (p0 >= a.n) break;                                         // wave-uniform; later tiles lie further out
        // ---- gather (pairs past n read pair n - 1; masked at the store)
        int64_t u[PNB], it[PNB];
#pragma unroll
        for (int nb = 0; nb < PNB; ++nb) {
            int64_t p = p0 + 16 * nb + j;
            p = p < a.n ? p : a.n - 1;
            u[nb] = a.users[p];
            it[nb] = a.items[p];
        }
        v4f x[T0][PNB];
#pragma unroll
        for (int t = 0; t < T0; ++t) {
            const int f = 16 * t + 4 * g;                             // < E: the user's row, else the item's
#pragma unroll
            for (int nb = 0; nb < PNB; ++nb)
                x[t][nb] = *reinterpret_cast<const v4f *>(f < E ? a.user_w + u[nb] * E + f : a.item_w + it[nb] * E + (f - E));
        }
        v4f last[PNB];
        tower<E, 0, PNB>(x, last, lds, g, j);

        // ---- this lane group's quarter of the logit: output dot, then the GMF columns c = g mod 4
        float p[PNB];
#pragma unroll
        for (int nb = 0; nb < PNB; ++nb) p[nb] = out_dot(wo, last[nb]);
        if (a.M > 0) {
            const float *mu[PNB], *mi[PNB];
#pragma unroll
            for (int nb = 0; nb < PNB; ++nb) {
                mu[nb] = a.mf_user_w + u[nb] * a.M;
                mi[nb] = a.mf_item_w + it[nb] * a.M;
            }
#pragma unroll 4
            for (int k = 0; k < a.MP; k += 4) {
                const int c = k + g, cc = c < a.M ? c : a.M - 1;      // padding columns: read in bounds, not added
                const float w = aw[c];
#pragma unroll
                for (int nb = 0; nb < PNB; ++nb) {
                    const float q = fmaf(w * mu[nb][cc], mi[nb][cc], p[nb]);
                    p[nb] = c < a.M ? q : p[nb];
                }
            }
        }
        float z = 0.0f;
#pragma unroll
        for (int nb = 0; nb < PNB; ++nb) {
            const float s = group_sum(p[nb]);
            z = g == nb ? s : z;
        }
        // ---- bias, sigmoid, store: lane group nb stores block nb
        const int64_t po = p0 + 16 * g + j;
        if (g < PNB && po < a.n) a.out[po] = sigmoidf_ref(z + bo);
    }
}

// The model check of the three entry points.  The shape part reads no pointer of the model
// (rg_ncf_score_workspace_len sizes a model whose tables do not exist yet); `count` names n.
int score_check_shape(const rg_ncf_model_t *m, int64_t n, const char *count, const std::string &w) {
    if (!m) return fail_arg(w + ": null model");
    if (rg_ncf_mlp_len(m->dim) < 0) return fail_arg(w + ": dim must be 8, 16, 32 or 64");
    if (m->mf_dim < 0 || m->mf_dim > RG_NEUMF_MAX_MF_DIM) return fail_arg(w + ": mf_dim out of range");
    if (m->num_items < 1 || m->num_users < 1) return fail_arg(w + ": empty tables");
    if (n < 0) return fail_arg(w + ": " + count + " < 0");
    return RG_OK;
}

// The shape part, then the pointers: the model's tables and `args` (whether the call's own pointers
// are all there).
int score_check_model(const rg_ncf_model_t *m, int64_t n, const char *count, bool args, const std::string &w) {
    const int rc = score_check_shape(m, n, count, w);
    if (rc != RG_OK) return rc;
    if (!args || !m->user_w || !m->item_w || !m->mlp) return fail_arg(w + ": null argument");
    if (m->mf_dim > 0 && (!m->mf_user_w || !m->mf_item_w)) return fail_arg(w + ": mf_dim > 0 without the GMF tables");
    return RG_OK;
}

struct ScoreLaunch {
    hipStream_t s;
    const rg_ncf_model_t *m;
    const int64_t *users;
    int64_t n_users;
    float *ws, *out;
    int64_t ld;
    template <class EC>
    int operator()(EC) const {
        constexpr int E = EC::value;
        const int MP = pad4(m->mf_dim);
        float *Hi = ws, *Hu = Hi + m->num_items * E, *Gu = Hu + n_users * E;
        const HalvesArgs h{m->user_w, m->item_w, m->mlp, m->mf_user_w, users, m->num_items, n_users, m->mf_dim, MP, Hi, Hu, Gu};
        const int64_t hblocks = (m->num_items + kHalfRows - 1) / kHalfRows + (n_users + kHalfRows - 1) / kHalfRows;
        hipLaunchKernelGGL((ncf_score_halves_kernel<E>), dim3((unsigned)hblocks), dim3(kThreads), 0, s, h);
        const ScoreArgs a{m->mlp, Hi, Hu, Gu, m->mf_item_w, m->num_items, n_users, ld, m->mf_dim, MP, out};
        const dim3 grid((unsigned)((m->num_items + kTile - 1) / kTile), (unsigned)((n_users + kGroup - 1) / kGroup));
        hipLaunchKernelGGL((ncf_score_kernel<E>), grid, dim3(kThreads), ScoreLds<E>::lds_floats(MP) * sizeof(float), s, a);
        return check_launch("rg_ncf_score_users");
    }
};

// workgroups that are resident at once (LDS and registers of the compiled kernel): the grid's cap, so
// every workgroup stages the weights once and the tiles spread evenly over one resident set
template <int E>
int pairs_resident(int MP) {
    static int per_cu[RG_NEUMF_MAX_MF_DIM / 4 + 1] = {};
    int &k = per_cu[MP / 4];
    if (k == 0) {
        int b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, ncf_score_pairs_kernel<E>, kThreads,
                                                         PairLds<E>::lds_floats(MP) * sizeof(float)) != hipSuccess || b < 1)
            b = 1;
        k = b > 8 ? 8 : b;
    }
    return k * num_cus();
}

struct PairsLaunch {
    hipStream_t s;
    const rg_ncf_model_t *m;
    const int64_t *users, *items;
    int64_t n;
    float *out;
    template <class EC>
    int operator()(EC) const {
        constexpr int E = EC::value;
        const int MP = pad4(m->mf_dim);
        const int64_t tiles = (n + kPairTile - 1) / kPairTile, cap = pairs_resident<E>(MP);
        const PairArgs a{m->user_w, m->item_w, m->mlp, m->mf_user_w, m->mf_item_w, users, items, n, tiles, m->mf_dim, MP, out};
        hipLaunchKernelGGL((ncf_score_pairs_kernel<E>), dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(kThreads),
                           PairLds<E>::lds_floats(MP) * sizeof(float), s, a);
        return check_launch("rg_ncf_score_pairs");
    }
};

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int rg_ncf_score_pairs(void *stream, const rg_ncf_model_t *m, const int64_t *users_dev, const int64_t *items_dev,
                                  int64_t n, float *out_dev) {
    const int rc = score_check_model(m, n, "n", users_dev && items_dev && out_dev, "rg_ncf_score_pairs");
    if (rc != RG_OK) return rc;
    if ((uintptr_t)m->user_w % 16 || (uintptr_t)m->item_w % 16)
        return fail_arg("rg_ncf_score_pairs: the embedding tables must be 16-byte aligned");
    if (n == 0) return RG_OK;
    return dispatch_ncf_dim(m->dim, PairsLaunch{(hipStream_t)stream, m, users_dev, items_dev, n, out_dev});
}

extern "C" int64_t rg_ncf_score_workspace_len(const rg_ncf_model_t *m, int64_t n_users) {
    if (score_check_shape(m, n_users, "n_users", "rg_ncf_score_workspace_len") != RG_OK) return -1;
    return (m->num_items + n_users) * m->dim + n_users * pad4(m->mf_dim);
}

extern "C" int rg_ncf_score_users(void *stream, const rg_ncf_model_t *m, const int64_t *users_dev, int64_t n_users,
                                  float *workspace_dev, float *out_dev, int64_t ld) {
    const int rc = score_check_model(m, n_users, "n_users", users_dev && workspace_dev && out_dev, "rg_ncf_score_users");
    if (rc != RG_OK) return rc;
    if (ld < m->num_items) return fail_arg("rg_ncf_score_users: ld < num_items");
    if ((uintptr_t)workspace_dev % 16) return fail_arg("rg_ncf_score_users: workspace must be 16-byte aligned");
    if (n_users == 0) return RG_OK;
    if ((n_users + kGroup - 1) / kGroup > 65535 || (m->num_items + kHalfRows - 1) / kHalfRows > INT_MAX / 2)
        return fail_arg("rg_ncf_score_users: too many users or items for one launch");
    return dispatch_ncf_dim(m->dim, ScoreLaunch{(hipStream_t)stream, m, users_dev, n_users, workspace_dev, out_dev, ld});
}
