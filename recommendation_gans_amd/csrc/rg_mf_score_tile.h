// What the MF inference kernels share (rg_mf_score.hip: the score block; rg_mf_topk.hip: the
// fused score, exclude and top-k): one (item tile, user group) of
//     sigmoid((<user_w[users[r]], item_w[c]> + user_b[users[r]]) + item_b[c])
// staged, multiplied and finished by a workgroup of 4 waves.  Both kernels call the same two
// functions, so a (user, item) score is the same bits from either.
//
//   stage    K runs in chunks of 64 columns.  Thread (rl = tid / 16, cl = tid % 16) carries rows
//            rl, rl + 16, ... of the tile's items and of the group's gathered users through
//            registers into LDS: one 16-byte load per row and chunk when dim % 4 == 0 and both
//            tables are 16-byte aligned (columns 4 cl .. 4 cl + 3), else four scalar loads (columns
//            cl, cl + 16, cl + 32, cl + 48), zeros past dim -- K is padded to a multiple of 4.
//            Every load of a chunk is issued before the first is used, and the next chunk's loads
//            are issued before this chunk's product.  LDS rows have a stride of 66 floats
//            (ds_read_b32 has 32 banks per 32-lane half; 16 rows x 2 k-columns at stride 66 fall on
//            32 distinct banks).  50,688 B of LDS whatever the dim: three workgroups fit a CU.
//   product  4 waves; wave w owns the group's users [16 w, 16 w + 16) against the whole tile:
//            NB = tile / 16 accumulators of v_mfma_f32_16x16x4_f32, A = the users' rows (lane
//            (g = lane / 16, j = lane % 16): user j, k = 4 s + g of step s), B = the items' rows
//            (item 16 nb + j, same k).  One A read and NB B reads feed NB MFMAs.
//   scores   acc[nb][r] is (user 4 g + r, item 16 nb + j): bias, sigmoidf_ref, then the caller's
//            sink -- 16 consecutive items per user and lane group.
//
// Every score has ONE accumulator chain from 0 with k ascending (the MFMA sums its four k in
// order; chunks and steps follow in order): no split-K, no atomics, nothing depends on where the
// user stands in the block or on the block's size.
#pragma once
#include "rg_common.h"
#include "rg_mfma.h"

namespace rg {
namespace mf_tile {

constexpr int kTile = RG_MF_SCORE_ITEM_TILE, NB = kTile / 16;
constexpr int kWaves = 4, kThreads = 64 * kWaves, kGroup = 16 * kWaves;
static_assert(kGroup == RG_MF_SCORE_USER_GROUP && kTile % 16 == 0, "header constants");
constexpr int kChunk = 64;              // k columns staged at a time
constexpr int kStride = kChunk + 2;     // LDS row stride (floats): kStride / 2 odd, see above
constexpr int RI = kTile / 16, RU = kGroup / 16;   // rows per staging thread: items, users
constexpr int kItemFloats = kTile * kStride, kUserFloats = kGroup * kStride;   // the two LDS images

struct Tables {
    const float *user_w, *item_w, *user_b, *item_b;
    const int64_t *users;
    int64_t num_items, n_users;
    int dim;
};

// 16-byte loads: dim % 4 == 0 and both tables 16-byte aligned
inline bool vec_loads(const float *user_w, const float *item_w, int dim) {
    return dim % 4 == 0 && (uintptr_t)user_w % 16 == 0 && (uintptr_t)item_w % 16 == 0;
}

// a staging thread's share of columns [k0, k0 + kc) of table row `row` (zeros for row < 0 and
// past kc): VEC columns 4 cl .. 4 cl + 3, else cl, cl + 16, cl + 32, cl + 48
template <bool VEC>
__device__ __forceinline__ float4 load_slice(const float *__restrict__ tab, int64_t row, int dim, int k0, int kc,
                                             int cl) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (row < 0) return v;
    const float *p = tab + row * dim + k0;
    if constexpr (VEC) {
        if (4 * cl < kc) v = *reinterpret_cast<const float4 *>(p + 4 * cl);
    } else {
        if (cl < kc) v.x = p[cl];
        if (cl + 16 < kc) v.y = p[cl + 16];
        if (cl + 32 < kc) v.z = p[cl + 32];
        if (cl + 48 < kc) v.w = p[cl + 48];
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store_slice(float *row, int cl, float4 v) {
    if constexpr (VEC) {
        float2 *p = reinterpret_cast<float2 *>(row + 4 * cl);    // LDS rows are 8-byte aligned
        p[0] = make_float2(v.x, v.y);
        p[1] = make_float2(v.z, v.w);
    } else {
        row[cl] = v.x;
        row[cl + 16] = v.y;
        row[cl + 32] = v.z;
        row[cl + 48] = v.w;
    }
}

// Stage and multiply items [i0, i0 + kTile) x users [u0, u0 + kGroup) into acc.  Called by every
// thread of the workgroup (it holds barriers); sI [kItemFloats] and sU [kUserFloats] must be free
// on entry -- the caller orders its earlier use of them before the call -- and may still be read
// by other waves on return.  Returns whether this wave has users (wave-uniform): a wave without
// any only stages, and its acc is not to be used.
template <bool VEC>
__device__ __forceinline__ bool product(const Tables &a, int64_t i0, int64_t u0, float *sI, float *sU,
                                        v4f (&acc)[NB]) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int rl = tid >> 4, cl = tid & 15;

    // ---- the rows this thread stages (-1: none)
    int64_t irow[RI], urow[RU];
#pragma unroll
    for (int t = 0; t < RI; ++t) irow[t] = i0 + rl + 16 * t < a.num_items ? i0 + rl + 16 * t : -1;
#pragma unroll
    for (int t = 0; t < RU; ++t) urow[t] = u0 + rl + 16 * t < a.n_users ? a.users[u0 + rl + 16 * t] : -1;
    float4 vi[RI], vu[RU];
    auto load_chunk = [&](int k0) {
        const int kc = a.dim - k0 < kChunk ? a.dim - k0 : kChunk;
#pragma unroll
        for (int t = 0; t < RU; ++t) vu[t] = load_slice<VEC>(a.user_w, urow[t], a.dim, k0, kc, cl);
#pragma unroll
        for (int t = 0; t < RI; ++t) vi[t] = load_slice<VEC>(a.item_w, irow[t], a.dim, k0, kc, cl);
    };
    load_chunk(0);

#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    const bool active = u0 + wave * 16 < a.n_users;     // wave-uniform: a wave without users only stages
    const float *pa = sU + (wave * 16 + j) * kStride + g;
    const float *pb = sI + j * kStride + g;
    auto step = [&](int k) {                            // k = 4 s: columns 4 s + g of every row
        const float av = pa[k];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma(av, pb[16 * nb * kStride + k], acc[nb]);
    };
    for (int k0 = 0; k0 < a.dim; k0 += kChunk) {
        const int kc = a.dim - k0 < kChunk ? a.dim - k0 : kChunk, kcp = (kc + 3) & ~3;
        if (k0) __syncthreads();                        // the previous chunk has been read
#pragma unroll
        for (int t = 0; t < RU; ++t) store_slice<VEC>(sU + (rl + 16 * t) * kStride, cl, vu[t]);
#pragma unroll
        for (int t = 0; t < RI; ++t) store_slice<VEC>(sI + (rl + 16 * t) * kStride, cl, vi[t]);
        __syncthreads();
        if (k0 + kChunk < a.dim) load_chunk(k0 + kChunk);
        if (active) {
            int k = 0;
            for (; k + 16 <= kcp; k += 16) {
                step(k);
                step(k + 4);
                step(k + 8);
                step(k + 12);
            }
            for (; k < kcp; k += 4) step(k);
        }
    }
    return active;
}

// The scores of an active wave's accumulators: sink(ul, u, nb, item, score) for every user
// u = u0 + ul < n_users of the wave (ul = 16 wave + 4 g + r in the group) and every item
// i0 + 16 nb + j < num_items.
// RAW: the score before the sigmoid (rg_mf_score_users_raw).
template <bool RAW = false, class Sink>
__device__ __forceinline__ void scores(const Tables &a, int64_t i0, int64_t u0, const v4f (&acc)[NB], Sink &&sink) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
    float bi[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int64_t item = i0 + 16 * nb + j;
        bi[nb] = item < a.num_items ? a.item_b[item] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ul = wave * 16 + 4 * g + r;
        const int64_t u = u0 + ul;
        if (u >= a.n_users) continue;
        const float bu = a.user_b[a.users[u]];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int64_t item = i0 + 16 * nb + j;
            if (item < a.num_items) {
                const float z = (acc[nb][r] + bu) + bi[nb];
                sink(ul, u, nb, item, RAW ? z : sigmoidf_ref(z));
            }
        }
    }
}

}  // namespace mf_tile
}  // namespace rg
