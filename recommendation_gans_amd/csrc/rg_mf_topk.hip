// MF recommend: the k best items of a block of users, without the score block.  Row r's key
// for column c is -inf if c is in the row's exclusion list, -inf if the score is NaN, else the
// score sigmoid((<user_w[u], item_w[c]> + user_b[u]) + item_b[c]); the k best columns by (key
// descending, column ascending) and their scores leave the device -- what rg_mf_score_users,
// -inf over the exclusions, rg_topk_rows and a gather give, id for id and bit for bit.
//
// The grid, the tile walk, the register lists, their merge and the second launch are
// rg_topk_tiles.h's tile_topk_kernel (182 / 198 / 232 VGPRs at K = 8 / 16 / 32 here, no scratch);
// this file holds the Op that makes it MF recommend:
//   finish   rg_mf_score_tile.h's scores(): the arithmetic of rg_mf_score_users, not restated here.
//   exclude  thread (ul = tid / 4, q = tid % 4) owns entries q, q + 4, ... of user ul's exclusion
//            row (ascending ids by contract).  Its cursor starts at the split's first item (a
//            binary search) and only moves forward: ids below the tile are passed, ids inside it
//            become -inf in the LDS tile, the first id at or past the tile's end stops the walk
//            until the next tile.  An id is compared with the tile's range [i0, i0 + ncols) before
//            it becomes an LDS index; ids < 0 or >= num_items never do.
//
// The tables, users and exclusions are only read.
#include "rg_topk_tiles.h"

namespace rg {
namespace {

using namespace topk;

struct MfOp {
    static constexpr bool kMasks = true;
    const int64_t *exc_ptr;
    const int32_t *exc_idx;
    int64_t e, e_end;                               // this thread's cursor, set by begin()

    // entries q, q + 4, ... of the user's exclusion row from the first id that is not below `first`
    __device__ __forceinline__ bool begin(const Tables &t, int64_t u0, int64_t first) {
        const int q = threadIdx.x & 3;
        const int64_t r = u0 + (threadIdx.x >> 2);
        e = e_end = 0;
        if (exc_ptr && r < t.n_users) {
            const int64_t e0 = exc_ptr[r];
            e_end = exc_ptr[r + 1];
            int64_t lo = e0, hi = e_end;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (exc_idx[mid] < first) lo = mid + 1; else hi = mid;
            }
            e = lo + ((q - (int)((lo - e0) & 3)) & 3);
        }
        return true;
    }
    __device__ __forceinline__ void finish(const Tables &t, int64_t i0, int64_t u0, const v4f (&acc)[NB],
                                           float *sT) const {
        scores(t, i0, u0, acc, [&](int row, int64_t, int, int64_t item, float s) {
            sT[row * kTStride + (int)(item - i0)] = s;
        });
    }
    __device__ __forceinline__ void mask(int64_t i0, int ncols, float *trow) {
        while (e < e_end) {
            const int64_t id = exc_idx[e];
            if (id >= i0 + ncols) break;            // later tiles (or never: id >= num_items)
            if (id >= i0) trow[(int)(id - i0)] = -INFINITY;
            e += 4;
        }
    }
};

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int64_t rg_mf_topk_workspace_len(int64_t num_items, int64_t n_users, int32_t k, int32_t splits) {
    return workspace_len("rg_mf_topk_workspace_len", num_items, n_users, k, splits);
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
    return run("rg_mf_topk_users", (hipStream_t)stream,
               Tables{user_w, item_w, user_b, item_b, users_dev, num_items, n_users, dim},
               MfOp{exc_ptr, exc_idx, 0, 0}, k, splits, workspace_dev, out_idx, out_scores);
}
