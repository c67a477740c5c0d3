// MF recommend: the k best items of a block of users, without the score block.  Row r's key
// for column c is -inf if c is in the row's exclusion list, -inf if the score is NaN, else the
// score sigmoid((<user_w[u], item_w[c]> + user_b[u]) + item_b[c]); the k best columns by (key
// descending, column ascending) and their scores leave the device -- what rg_mf_score_users,
// -inf over the exclusions, rg_topk_rows and a gather give, id for id and bit for bit.
//
//   grid     one workgroup of 4 waves per (group of RG_MF_SCORE_USER_GROUP users, split s of
//            `splits`), the user group the fast index: the workgroups that run together walk the
//            same item tiles, which stay in L2.  Split s owns the item tiles
//            [s tiles / splits, (s + 1) tiles / splits) and walks them in ascending order.
//   tile     staged and multiplied by rg_mf_score_tile.h's product(), finished by its scores():
//            the arithmetic of rg_mf_score_users, not restated here.  The sink writes the 64 x 128
//            scores into an LDS tile (row stride 132 floats: the 16 rows x 16 columns a half-wave
//            writes, and the 8 users x 4 quarters it scans, fall on 32 distinct banks) that takes
//            the place of the item image once every wave has read it: 50,688 B of LDS as for the
//            score block.  The lists cost registers (182 / 198 / 232 VGPRs at K = 8 / 16 / 32, no
//            scratch): two workgroups per CU; at three the compiler spills.
//   exclude  thread (ul = tid / 4, q = tid % 4) owns entries q, q + 4, ... of user ul's exclusion
//            row (ascending ids by contract).  Its cursor starts at the split's first item (a
//            binary search) and only moves forward: ids below the tile are passed, ids inside it
//            become -inf in the LDS tile, the first id at or past the tile's end stops the walk
//            until the next tile.  An id is compared with the tile's range [i0, i0 + ncols) before
//            it becomes an LDS index; ids < 0 or >= num_items never do.
//   select   the same four threads each scan a quarter of the user's tile row (columns q, q + 4,
//            ...) into a sorted top-K in registers, K in {8, 16, 32}: rg_eval.hip's select-based
//            insertion behind an early test against the list's last element.  The list carries the
//            raw value (NaN kept, so the NaN that comes out is the one the score kernel writes)
//            and compares by key (NaN -> -inf).
//   merge    after the last tile the four lists of a user are merged in LDS (K = 32: two waves'
//            lists at a time, 32 KB) and k (score, id) pairs per (user, split) are written:
//            splits == 1 straight to the outputs, else to the workspace, where a second launch
//            (one wave per user) selects the k best of the splits x k candidates with the same
//            insertion and merge.  A split with fewer than k columns pads with the filler
//            (-inf, INT_MAX), which loses to every column: num_items >= k, so no filler is output.
//
// (key, column) is a total order: no two candidates compare equal, so the k best and their order
// do not depend on the splits, their boundaries, the thread that saw a column or the order of any
// merge.  No atomics.  The tables, users and exclusions are only read.
#include "rg_topk_lists.h"

namespace rg {
namespace {

using namespace mf_tile;
using namespace topk;

constexpr int kTStride = kTile + 4;                 // row stride of the LDS score tile (floats)
static_assert(kGroup * kTStride <= kItemFloats, "the score tile takes the item image's place");
constexpr int kLdsFloats = kItemFloats + kUserFloats;

struct TopkArgs {
    Tables t;
    const int64_t *exc_ptr;
    const int32_t *exc_idx;
    int64_t groups, tiles;
    int splits, k;
    float *dst_v;                                   // [n_users][splits][k]; null: scores not wanted
    int32_t *dst_i;
};


template <bool VEC, int K>
__global__ __launch_bounds__(kThreads, 2) void mf_topk_kernel(TopkArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[kLdsFloats];
    float *sI = smem, *sU = smem + kItemFloats, *sT = smem;
    const int tid = threadIdx.x, ul = tid >> 2, q = tid & 3;
    const int64_t split = (int64_t)blockIdx.x / a.groups, grp = (int64_t)blockIdx.x - split * a.groups;
    const int64_t u0 = grp * kGroup, r = u0 + ul;
    const bool has_user = r < a.t.n_users;
    const int64_t t_begin = split * a.tiles / a.splits, t_end = (split + 1) * a.tiles / a.splits;

    // ---- this thread's cursor into the user's exclusion row: entries q, q + 4, ... from the first
    // id that is not below the split's first item
    int64_t e = 0, e_end = 0;
    if (a.exc_ptr && has_user) {
        const int64_t e0 = a.exc_ptr[r], first = t_begin * kTile;
        e_end = a.exc_ptr[r + 1];
        int64_t lo = e0, hi = e_end;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.exc_idx[mid] < first) lo = mid + 1; else hi = mid;
        }
        e = lo + ((q - (int)((lo - e0) & 3)) & 3);
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
        if (active)
            scores(a.t, i0, u0, acc, [&](int row, int64_t, int, int64_t item, float s) {
                sT[row * kTStride + (int)(item - i0)] = s;
            });
        __syncthreads();
        while (e < e_end) {
            const int64_t id = a.exc_idx[e];
            if (id >= i0 + ncols) break;            // later tiles (or never: id >= num_items)
            if (id >= i0) trow[(int)(id - i0)] = -INFINITY;
            e += 4;
        }
        __syncthreads();
        if (has_user)
            for (int c = q; c < ncols; c += 4) top.insert(trow[c], (int)(i0 + c));
        __syncthreads();                            // the tile has been scanned: sI and sU are free
    }

    // ---- the four lists of a user into one, kPerPass threads' lists in LDS at a time
    constexpr int kPasses = 2 * K * kThreads > kLdsFloats ? 2 : 1, kPerPass = kThreads / kPasses;
    static_assert(2 * K * kPerPass <= kLdsFloats, "merge lists fit the staging LDS");
    float *sv = smem;
    int *si = reinterpret_cast<int *>(smem + K * kPerPass);
    const int lt = tid % kPerPass;
    for (int h = 0; h < kPasses; ++h) {
        const bool mine = tid / kPerPass == h;
        if (mine) top.store(sv + lt * K, si + lt * K);
        __syncthreads();
        for (int s = 1; s < 4; s <<= 1) {
            if (mine && (lt & (2 * s - 1)) == 0) merge_pair<K>(sv, si, lt, lt + s);
            __syncthreads();
        }
        if (mine && has_user) {
            const int64_t dst = (r * a.splits + split) * a.k;
            for (int j = q; j < a.k; j += 4) {
                a.dst_i[dst + j] = si[(lt - q) * K + j];
                if (a.dst_v) a.dst_v[dst + j] = sv[(lt - q) * K + j];
            }
        }
        __syncthreads();
    }
}


template <bool VEC, int K>
int launch(hipStream_t s, const TopkArgs &a, const float *ws_v, const int32_t *ws_i, int32_t *out_idx,
           float *out_scores) {
    hipLaunchKernelGGL((mf_topk_kernel<VEC, K>), dim3((unsigned)(a.groups * a.splits)), dim3(kThreads), 0, s, a);
    if (a.splits > 1)
        hipLaunchKernelGGL((mf_topk_merge_kernel<K>), dim3((unsigned)a.t.n_users), dim3(kMergeThreads), 0, s, ws_v, ws_i,
                           (int64_t)a.splits * a.k, a.k, out_idx, out_scores);
    return check_launch("rg_mf_topk_users");
}


}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int64_t rg_mf_topk_workspace_len(int64_t num_items, int64_t n_users, int32_t k, int32_t splits) {
    if (check_shape("rg_mf_topk_workspace_len", num_items, n_users, k, splits) != RG_OK) return -1;
    return 8 * n_users * k * pick_splits(num_items, n_users, splits);   // users x splits < 2^30: no overflow
}

extern "C" int rg_mf_topk_users(void *stream, const float *user_w, const float *item_w, const float *user_b,
                                const float *item_b, int32_t dim, int64_t num_items, const int64_t *users_dev,
                                int64_t n_users, const int64_t *exc_ptr, const int32_t *exc_idx, int32_t k,
                                int32_t splits, void *workspace_dev, int32_t *out_idx, float *out_scores) {
    if (!user_w || !item_w || !user_b || !item_b || !users_dev || !workspace_dev || !out_idx)
        return fail_arg("rg_mf_topk_users: null pointer");
    if ((exc_ptr == nullptr) != (exc_idx == nullptr))
        return fail_arg("rg_mf_topk_users: exc_ptr and exc_idx must both be given or both be null");
    if (dim < 1 || dim > 256) return fail_arg("rg_mf_topk_users: dim must be in [1, 256]");
    if (const int rc = check_shape("rg_mf_topk_users", num_items, n_users, k, splits)) return rc;
    if (n_users == 0) return RG_OK;
    const int64_t tiles = (num_items + kTile - 1) / kTile, groups = (n_users + kGroup - 1) / kGroup;
    const int64_t s = pick_splits(num_items, n_users, splits);
    float *ws_v = static_cast<float *>(workspace_dev);
    int32_t *ws_i = reinterpret_cast<int32_t *>(ws_v + n_users * s * k);
    TopkArgs a{{user_w, item_w, user_b, item_b, users_dev, num_items, n_users, dim}, exc_ptr, exc_idx, groups, tiles,
               (int)s, k, s == 1 ? out_scores : ws_v, s == 1 ? out_idx : ws_i};
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = vec_loads(user_w, item_w, dim);
    if (k <= 8)
        return vec ? launch<true, 8>(st, a, ws_v, ws_i, out_idx, out_scores)
                   : launch<false, 8>(st, a, ws_v, ws_i, out_idx, out_scores);
    if (k <= 16)
        return vec ? launch<true, 16>(st, a, ws_v, ws_i, out_idx, out_scores)
                   : launch<false, 16>(st, a, ws_v, ws_i, out_idx, out_scores);
    return vec ? launch<true, 32>(st, a, ws_v, ws_i, out_idx, out_scores)
               : launch<false, 32>(st, a, ws_v, ws_i, out_idx, out_scores);
}
