// MF inference: scores of a block of users against EVERY item,
//     out[r][c] = sigmoid((<user_w[users[r]], item_w[c]> + user_b[users[r]]) + item_b[c]),
// BilinearNet.forward (spotlight/factorization/representations.py:62-91) over the whole item
// table: the score block the evaluation metrics rank (spotlight/evaluation.py: _scored,
// _topk_hits, mrr_score).  One launch replaces gather, GEMM, two broadcast adds and a sigmoid,
// each of the last four a pass over the (users x items) block through global memory.
//
//   grid     one workgroup per (item tile of RG_MF_SCORE_ITEM_TILE, group of RG_MF_SCORE_USER_GROUP
//            users), the user group the fast index: workgroups that run together share an item
//            tile and walk the users, whose gathered rows (1 MB at 4096 x 64) stay in L2.
//   tile     staging, product and the score arithmetic are rg_mf_score_tile.h's, shared with the
//            fused top-k kernel (rg_mf_topk.hip).
//   epilogue one store per score -- 16 consecutive items (64 B) per user and lane group, a wave
//            covering whole rows of the tile.
//
// Every output has ONE accumulator chain from 0 with k ascending (the MFMA sums its four k in
// order; chunks and steps follow in order): no split-K, no atomics, nothing depends on where the
// user stands in the block or on the block's size.  A (user, item) score is the same bits at any
// position, in any block, on any call.  The tables are only read; item tails and the last user
// group are masked; out's padding columns [num_items, ld) and rows past n_users are not written.
#include <climits>

#include "rg_mf_score_tile.h"

namespace rg {
namespace {

using namespace mf_tile;

struct Args {
    Tables t;
    int64_t ld, groups;
    float *out;
};

template <bool VEC, bool RAW>
__global__ __launch_bounds__(kThreads, 2) void mf_score_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) float sI[kItemFloats];
    __shared__ __attribute__((aligned(16))) float sU[kUserFloats];
    const int64_t tile = (int64_t)blockIdx.x / a.groups, grp = (int64_t)blockIdx.x - tile * a.groups;
    const int64_t i0 = tile * kTile, u0 = grp * kGroup;
    v4f acc[NB];
    if (!product<VEC>(a.t, i0, u0, sI, sU, acc)) return;
    scores<RAW>(a.t, i0, u0, acc, [&](int, int64_t u, int, int64_t item, float s) { a.out[u * a.ld + item] = s; });
}

}  // namespace
}  // namespace rg

using namespace rg;

template <bool RAW>
static int score_users(const char *name, void *stream, const float *user_w, const float *item_w, const float *user_b,
                       const float *item_b, int32_t dim, int64_t num_items, const int64_t *users_dev,
                       int64_t n_users, float *out_dev, int64_t ld) {
    const std::string who(name);
    if (!user_w || !item_w || !user_b || !item_b || !users_dev || !out_dev)
        return fail_arg(who + ": null pointer");
    if (dim < 1 || dim > 256) return fail_arg(who + ": dim must be in [1, 256]");
    if (num_items < 1) return fail_arg(who + ": num_items < 1");
    if (ld < num_items) return fail_arg(who + ": ld < num_items");
    if (n_users < 0) return fail_arg(who + ": n_users < 0");
    if (n_users == 0) return RG_OK;
    const int64_t tiles = (num_items + kTile - 1) / kTile, groups = (n_users + kGroup - 1) / kGroup;
    if (tiles > (int64_t)(UINT_MAX / kThreads) / groups)     // a launch holds fewer than 2^32 threads
        return fail_arg(who + ": too many users x items for one launch (item tiles x user groups > 2^24 - 1)");
    const Args a{{user_w, item_w, user_b, item_b, users_dev, num_items, n_users, dim}, ld, groups, out_dev};
    const dim3 grid((unsigned)(tiles * groups));
    if (vec_loads(user_w, item_w, dim))
        hipLaunchKernelGGL((mf_score_kernel<true, RAW>), grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((mf_score_kernel<false, RAW>), grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    return check_launch(name);
}

extern "C" int rg_mf_score_users(void *stream, const float *user_w, const float *item_w, const float *user_b,
                                 const float *item_b, int32_t dim, int64_t num_items, const int64_t *users_dev,
                                 int64_t n_users, float *out_dev, int64_t ld) {
    return score_users<false>("rg_mf_score_users", stream, user_w, item_w, user_b, item_b, dim, num_items, users_dev,
                              n_users, out_dev, ld);
}

// the same block before the sigmoid
extern "C" int rg_mf_score_users_raw(void *stream, const float *user_w, const float *item_w, const float *user_b,
                                     const float *item_b, int32_t dim, int64_t num_items, const int64_t *users_dev,
                                     int64_t n_users, float *out_dev, int64_t ld) {
    return score_users<true>("rg_mf_score_users_raw", stream, user_w, item_w, user_b, item_b, dim, num_items,
                             users_dev, n_users, out_dev, ld);
}
