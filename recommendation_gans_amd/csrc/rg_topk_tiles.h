// The fused top-k over rg_mf_score_tile.h's tiles (rg_mf_topk.hip: MF recommend; rg_item_sim.hip:
// item-to-item similarity): the k best columns of every row of a block, without the block.  The
// kernel body, the merge of the splits and the host-side shape rules are here, once; a feature
// brings an Op with what is its own.
//
//   grid     one workgroup of 4 waves per (group of RG_MF_SCORE_USER_GROUP rows, split s of
//            `splits`), the row group the fast index: the workgroups that run together walk the
//            same tiles, which stay in L2.  Split s owns the tiles
//            [s tiles / splits, (s + 1) tiles / splits) and walks them in ascending order.
//   tile     staged and multiplied by mf_tile::product(), finished by the Op.  The finish writes
//            the 64 x 128 values into an LDS tile (row stride 132 floats: the 16 rows x 16 columns
//            a half-wave writes, and the 8 rows x 4 quarters it scans, fall on 32 distinct banks)
//            that takes the place of the item image once every wave has read it: 50,688 B of LDS
//            as for the score block.  The lists cost registers: two workgroups per CU; at three
//            the compiler spills.
//   select   thread (ul = tid / 4, q = tid % 4) scans a quarter of row ul's tile row (columns q,
//            q + 4, ...) into a TopList<K> in registers, K in {8, 16, 32}.  The list carries the
//            raw value (NaN kept, so the NaN that comes out is the one the finish wrote) and
//            compares by key (NaN -> -inf).
//   merge    after the last tile the four lists of a row are merged in LDS (K = 32: two waves'
//            lists at a time, 32 KB) and k (value, id) pairs per (row, split) are written:
//            splits == 1 straight to the outputs, else to the workspace, where a second launch
//            (one wave per row) selects the k best of the splits x k candidates with the same
//            insertion and merge.  A split with fewer than k columns pads with the filler
//            (-inf, INT_MAX), which loses to every column: num_items >= k, so no filler is output.
//
// An Op is a small struct passed by value to the kernel:
//   kMasks                      whether mask() does anything (false: it and its barrier are left out)
//   begin(t, u0, first)         before the first tile, by every thread (u0: the group's first row;
//                               first: the split's first column); false from it, the same for the
//                               whole workgroup, ends the workgroup: its rows get the id -1 and the
//                               value NaN
//   finish(t, i0, u0, acc, sT)  an active wave's accumulators into the LDS tile sT (row stride kTStride)
//   mask(i0, ncols, trow)       -inf over this thread's share of the row's excluded columns of the tile
//
// The order of a row's candidates does not depend on the splits or their boundaries (rg_topk_lists.h).
// No atomics.  Everything here has internal linkage: each translation unit gets its own copy of the
// merge kernel.
#pragma once
#include "rg_mf_score_tile.h"
#include "rg_topk_lists.h"

namespace rg {
namespace topk {
namespace {

using namespace mf_tile;

constexpr int kMergeThreads = 64;                   // second launch: one wave per row
constexpr int kTStride = kTile + 4;                 // row stride of the LDS score tile (floats)
static_assert(kGroup * kTStride <= kItemFloats, "the score tile takes the item image's place");
constexpr int kLdsFloats = kItemFloats + kUserFloats;

struct TileArgs {
    Tables t;                                       // users = the block's rows
    int64_t groups, tiles;
    int splits, k;
    float *dst_v;                                   // [n_users][splits][k]; null: values not wanted
    int32_t *dst_i;
};

template <class Op, bool VEC, int K>
__global__ __launch_bounds__(kThreads, 2) void tile_topk_kernel(TileArgs a, Op op) {
    __shared__ __attribute__((aligned(16))) float smem[kLdsFloats];
    float *sI = smem, *sU = smem + kItemFloats, *sT = smem;
    const int tid = threadIdx.x, ul = tid >> 2, q = tid & 3;
    const int64_t split = (int64_t)blockIdx.x / a.groups, grp = (int64_t)blockIdx.x - split * a.groups;
    const int64_t u0 = grp * kGroup, r = u0 + ul;
    const bool has_user = r < a.t.n_users;
    const int64_t t_begin = split * a.tiles / a.splits, t_end = (split + 1) * a.tiles / a.splits;
    // entries q, q + 4, ... of the row's k pairs of this split
    auto put = [&](int j, int id, float v) {
        const int64_t dst = (r * a.splits + split) * a.k + j;
        a.dst_i[dst] = id;
        if (a.dst_v) a.dst_v[dst] = v;
    };

    if (!op.begin(a.t, u0, t_begin * kTile)) {
        if (has_user)
            for (int j = q; j < a.k; j += 4) put(j, -1, NAN);
        return;
    }

    TopList<K> top;
    top.init();
    float *trow = sT + ul * kTStride;
    for (int64_t t = t_begin; t < t_end; ++t) {
        const int64_t i0 = t * kTile;
        const int ncols = (int)(a.t.num_items - i0 < kTile ? a.t.num_items - i0 : kTile);
        v4f acc[NB];
        const bool active = product<VEC>(a.t, i0, u0, sI, sU, acc);
        __syncthreads();                            // every wave has read sI: the score tile takes its place
        if (active) op.finish(a.t, i0, u0, acc, sT);
        __syncthreads();
        if constexpr (Op::kMasks) {
            op.mask(i0, ncols, trow);
            __syncthreads();
        }
        if (has_user)
            for (int c = q; c < ncols; c += 4) top.insert(trow[c], (int)(i0 + c));
        __syncthreads();                            // the tile has been scanned: sI and sU are free
    }

    // ---- the four lists of a row into one, kPerPass threads' lists in LDS at a time
    constexpr int kPasses = 2 * K * kThreads > kLdsFloats ? 2 : 1, kPerPass = kThreads / kPasses;
    static_assert(2 * K * kPerPass <= kLdsFloats, "merge lists fit the staging LDS");
    float *sv = smem;
    int *si = reinterpret_cast<int *>(smem + K * kPerPass);
    const int lt = tid % kPerPass;
    for (int h = 0; h < kPasses; ++h) {
        const bool mine = tid / kPerPass == h;
        if (mine) top.store(sv + lt * K, si + lt * K);
        __syncthreads();
        merge_tree<K, 4>(sv, si, lt, mine);
        if (mine && has_user)
            for (int j = q; j < a.k; j += 4) put(j, si[(lt - q) * K + j], sv[(lt - q) * K + j]);
        __syncthreads();
    }
}

// splits > 1: the k best of a row's cand = splits x k candidates (ws_v / ws_i [n_users][cand])
template <int K>
__global__ __launch_bounds__(kMergeThreads) void mf_topk_merge_kernel(const float *__restrict__ ws_v,
                                                                      const int32_t *__restrict__ ws_i, int64_t cand,
                                                                      int k, int32_t *__restrict__ out_idx,
                                                                      float *__restrict__ out_scores) {
    __shared__ float sv[kMergeThreads * K];
    __shared__ int si[kMergeThreads * K];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    TopList<K> top;
    top.init();
    for (int64_t c = tid; c < cand; c += kMergeThreads) top.insert(ws_v[r * cand + c], ws_i[r * cand + c]);
    top.store(sv + tid * K, si + tid * K);
    __syncthreads();
    merge_tree<K, kMergeThreads>(sv, si, tid);
    if (tid < k) {
        out_idx[r * k + tid] = si[tid];
        if (out_scores) out_scores[r * k + tid] = sv[tid];
    }
}

// shape checks shared by the entry points; 0 or the failure's status
int check_shape(const char *fn, int64_t num_items, int64_t n_users, int32_t k, int32_t splits) {
    const std::string f = std::string(fn) + ": ";
    if (num_items < 1) return fail_arg(f + "num_items < 1");
    if (num_items > INT_MAX) return fail_arg(f + "num_items must fit int32");
    if (n_users < 0) return fail_arg(f + "n_users < 0");
    if (k < 1 || k > kTopkMax || k > num_items) return fail_arg(f + "k must be in [1, min(32, num_items)]");
    const int64_t tiles = (num_items + kTile - 1) / kTile;
    if (splits < 0 || splits > tiles)
        return fail_arg(f + "splits must be in [0, item tiles] (" + std::to_string(tiles) + " tiles of " +
                        std::to_string(kTile) + " items)");
    // a launch holds fewer than 2^32 threads: (user group, split) workgroups, and a wave per user.
    // The library's own pick (splits == 0) is 1 unless user groups x splits stays below 6 CUs, so it
    // is refused exactly when one split is: no need to ask the device before refusing.
    const int64_t groups = (n_users + kGroup - 1) / kGroup;
    if (groups > 0 && ((splits > 0 ? splits : 1) > (int64_t)(UINT_MAX / kThreads) / groups ||
                       n_users > (int64_t)(UINT_MAX / kMergeThreads)))
        return fail_arg(f + "too many users x splits for one launch (user groups x splits > 2^24 - 1 or users > "
                            "2^26 - 1)");
    return RG_OK;
}

// splits == 0: enough splits to give every CU three workgroups (two resident, one waiting), in [1, tiles].
// The only HIP call ahead of the launch (the CU count, cached): after every refusal.
int64_t pick_splits(int64_t num_items, int64_t n_users, int32_t splits) {
    if (splits > 0) return splits;
    const int64_t tiles = (num_items + kTile - 1) / kTile, groups = (n_users + kGroup - 1) / kGroup;
    const int64_t want = groups > 0 ? (3 * (int64_t)num_cus() + groups - 1) / groups : 1;
    return want < 1 ? 1 : want > tiles ? tiles : want;
}

// bytes of the workspace run() wants, or -1 (rg_last_error says why)
int64_t workspace_len(const char *fn, int64_t num_items, int64_t n_users, int32_t k, int32_t splits) {
    if (check_shape(fn, num_items, n_users, k, splits) != RG_OK) return -1;
    return 8 * n_users * k * pick_splits(num_items, n_users, splits);   // users x splits < 2^30: no overflow
}

template <class Op, bool VEC, int K>
void launch(hipStream_t s, const TileArgs &a, const Op &op, const float *ws_v, const int32_t *ws_i, int32_t *out_idx,
            float *out_v) {
    hipLaunchKernelGGL((tile_topk_kernel<Op, VEC, K>), dim3((unsigned)(a.groups * a.splits)), dim3(kThreads), 0, s, a,
                       op);
    if (a.splits > 1)
        hipLaunchKernelGGL((mf_topk_merge_kernel<K>), dim3((unsigned)a.t.n_users), dim3(kMergeThreads), 0, s, ws_v, ws_i,
                           (int64_t)a.splits * a.k, a.k, out_idx, out_v);
}

// The top-k of t.users' rows under `op`, for a shape check_shape passed with n_users > 0: the k
// ids and values to out_idx / out_v (null: values not wanted), through `workspace` of
// workspace_len() bytes when there is more than one split.
template <class Op>
int run(const char *fn, hipStream_t st, const Tables &t, const Op &op, int32_t k, int32_t splits, void *workspace,
        int32_t *out_idx, float *out_v) {
    const int64_t tiles = (t.num_items + kTile - 1) / kTile, groups = (t.n_users + kGroup - 1) / kGroup;
    const int64_t s = pick_splits(t.num_items, t.n_users, splits);
    float *ws_v = static_cast<float *>(workspace);
    int32_t *ws_i = reinterpret_cast<int32_t *>(ws_v + t.n_users * s * k);
    const TileArgs a{t, groups, tiles, (int)s, k, s == 1 ? out_v : ws_v, s == 1 ? out_idx : ws_i};
    const bool vec = vec_loads(t.user_w, t.item_w, t.dim);
    const auto go = k <= 8    ? (vec ? launch<Op, true, 8> : launch<Op, false, 8>)
                    : k <= 16 ? (vec ? launch<Op, true, 16> : launch<Op, false, 16>)
                              : (vec ? launch<Op, true, 32> : launch<Op, false, 32>);
    go(st, a, op, ws_v, ws_i, out_idx, out_v);
    return check_launch(fn);
}

}  // namespace
}  // namespace topk
}  // namespace rg
