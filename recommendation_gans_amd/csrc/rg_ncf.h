// What the NCF / NeuMF units share: the tower's shape (rg_ncf_tile.hip, rg_ncf_wave.hip,
// rg_ncf_score.hip), the training kernels' arguments, phases and dropout hash, the dispatch on
// the embedding width and the phase, and what the host API (rg_ncf.hip) needs of each training
// kernel: its tile size and its launch.
#pragma once
#include <type_traits>

#include "rg_common.h"

namespace rg {

constexpr int kNcfCap = RG_MF_LIST_CAP;
constexpr int kLdsMax = 160 * 1024 / 4;
constexpr int kRows = 32;              // tile kernel: examples per tile (two 16-row MFMA tiles)
namespace ncfw {
constexpr int kWaves = 4;              // wave kernel: waves (one tile each) per workgroup
constexpr int kR = 48;                 // rows per tile: 3 example blocks of 16 (n = 5: 8 whole columns)
}  // namespace ncfw

// layer sizes H_k = 2E >> k, k = 0..NH (H_NH = 8); NH hidden Linear layers + output 8 -> 1
template <int E>
struct NcfTower {
    static constexpr int NH = E == 8 ? 1 : E == 16 ? 2 : E == 32 ? 3 : 4;
    static constexpr int H(int k) { return (2 * E) >> k; }
    static constexpr int w_off(int k) {       // flat parameter offset of layer k (W then b)
        int o = 0;
        for (int j = 0; j < k; ++j) o += H(j + 1) * H(j) + H(j + 1);
        return o;
    }
    static constexpr int P = w_off(NH) + 8 + 1;                  // + output W (1x8), b (1)
    static constexpr int mask_off(int k) {    // first dropout unit of hidden layer k
        int u = 0;
        for (int j = 1; j <= k; ++j) u += H(j);
        return u;
    }
    static constexpr int mask_units() {
        int u = 0;
        for (int k = 1; k <= NH; ++k) u += H(k);
        return u;
    }
};

// f(integral_constant<int, E>) for the embedding widths the towers exist for, else -1 with no
// message: the -1 of the length queries (rg_ncf_mlp_len ...), which is RG_E_ARG for a launch; the
// entry points check the width first (ncf_mlp_len < 0) and word their own message
static_assert(RG_E_ARG == -1, "dispatch_ncf_dim's -1 is both");
template <typename F>
int dispatch_ncf_dim(int E, F &&f) {
    switch (E) {
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        default: return -1;
    }
}

struct NcfArgs {
    const float *user_w, *item_w;
    const float *mlp;                 // flat parameters (named_parameters order)
    int64_t num_users, num_items;
    const int2 *pairs;                // prepared, one record per column (rg_common.h pair_stride)
    int64_t n_pos, cols, global_cols, col_offset;
    int n_neg, loss, tc;              // tc: columns per tile
    int64_t tiles;
    float n_a, n_b;                   // loss denominators (as rg_mf_pairs)
    const int32_t *perm, *pos_slot;   // plan (optional)
    int32_t *row_count;
    int2 *row_list;
    long long *hot_grad;                  // int64 fixed point (rg_common.h fix_add)
    float *part_row;
    float *loss_partials;             // [tiles * 2]
    float *contrib;                   // [tiles * rows per tile * 2E]
    float *wpart;                     // [gridDim.x * P]
    float *scores;                    // [tiles * rows per tile] (forward-only phase)
    const float *dp_in;               // [tiles * rows per tile] (given-dp phase)
    const uint8_t *mask_pos, *mask_neg;
    uint64_t seed;
    int training;
    // NeuMF (mf_dim > 0)
    int mf_dim;
    const float *mf_user_w, *mf_item_w;
    float *mf_contrib;
    long long *mf_hot_grad;
    float *mf_part_row;
};

enum NcfPhase { kNcfFused = 0, kNcfScores = 1, kNcfGivenDp = 2, kNcfLossOnly = 3 };

// f(integral_constant<int, PHASE>) of rg_ncf_pairs' phase argument
template <typename F>
int dispatch_ncf_phase(int phase, F &&f) {
    switch (phase) {
        case kNcfFused: return f(std::integral_constant<int, kNcfFused>{});
        case kNcfScores: return f(std::integral_constant<int, kNcfScores>{});
        case kNcfGivenDp: return f(std::integral_constant<int, kNcfGivenDp>{});
        case kNcfLossOnly: return f(std::integral_constant<int, kNcfLossOnly>{});
        default: return fail_arg("rg_ncf_pairs: bad phase");
    }
}

__device__ __forceinline__ uint32_t hash32(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return (uint32_t)x;
}

// murmur3 fmix32: the per-unit dropout bit from the row's key
__device__ __forceinline__ uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bU;
    h ^= h >> 13;
    h *= 0xc2b2ae35U;
    h ^= h >> 16;
    return h;
}

// rg_ncf_tile.hip (its LDS floats at mf_dim M: -1 for another E) and rg_ncf_wave.hip (E = 64, M = 0)
int ncf_tile_launch(NcfArgs &a, hipStream_t s, int blocks, int E, int phase);
int ncf_tile_lds_floats(int E, int M);
int ncf_wave_launch(NcfArgs &a, hipStream_t s, int blocks, int phase);
#ifdef RG_DIAG_STAMPS   // each kernel unit has its own stamp buffer pointer; rg_diag_set_ncf_stamps sets both
int ncf_tile_set_stamps(unsigned long long *dev_buf);
int ncf_wave_set_stamps(unsigned long long *dev_buf);
#endif

}  // namespace rg
