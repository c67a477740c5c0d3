// MF fold-in (rg_mf_fold_in_users): fit the rows and biases of users that were not in the
// training set against FROZEN item tables, with the model's own loss and torch's Adam, in one
// launch.  A user is owned by one group of L::LPU lanes (the pair kernel's row layout,
// rg_common.h: a lane holds EPL elements of every row) for all of its steps, 64 / LPU users per
// wave, one wave per workgroup (the waves share nothing, so small workgroups spread over more
// compute units).  The user's row p, bias b, the Adam moments m and v and the step's gradient
// stay in registers; every step walks the row's positives, kPB at a time, each with its
// negatives in chunks of kNC, gathering the item rows (coalesced LPU-lane row loads, served by
// L2 after the first step), reducing the dot over the group's lanes (DPP), forming dz per pair
// and accumulating dz * Q_i; then the update (opt_update, rg_common.h).  Nothing but the result
// is written.  The layout dispatch, the score, the wave's longest row and the launch are the
// row-group helpers of rg_common.h (dispatch_rows, row_score, wave_max64, launch_row_groups).
//
// Order of a user's sums: every positive first sums its own term -- its negatives' dz * Q_j with
// j ascending, then its own dz * Q_i (and likewise its loss terms) -- and the positives' terms are
// added in ascending order: chains of 1 + n_neg and of P additions, not one of P (1 + n_neg), which
// a float32 sum over a long history would feel.  The wave loops to its longest row and
// masks the shorter ones with selects (never with a multiply), and the lane reduction is the
// same butterfly in every group: a user's bits depend on its own row alone.
#include "rg_common.h"

#include <limits.h>

namespace rg {
namespace {

constexpr int kPB = 2;   // positives in flight per group
constexpr int kNC = 4;   // negatives per positive in flight

struct FoldArgs {
    const float *item_w, *item_b;
    int32_t dim;
    const int64_t *hist_ptr;
    const int32_t *hist_idx, *neg_idx;
    int32_t n_neg;
    int64_t n_users;
    int32_t loss;
    rg_opt_t opt;
    const float2 *step_coef;
    int32_t steps;
    float *user_w, *user_b, *loss_out;
};

// per-group state of one positive while its negatives are walked
struct PosState {
    float sp;      // the positive's score
    float dpos;    // dL/ds of the positive, summed over its negatives (pairwise losses)
    float best;    // adaptive hinge: the highest negative score so far (-1: none yet; scores are in [0, 1])
};

template <class L>
__global__ void __launch_bounds__(kWave) mf_fold_kernel(const FoldArgs a) {
    constexpr int LPU = L::LPU, EPL = L::EPL, UPW = L::UPW;
    const int lane = threadIdx.x;
    const int sub = lane & (LPU - 1);
    const int64_t r = (int64_t)blockIdx.x * UPW + lane / LPU;
    const bool in = r < a.n_users;
    const int64_t off = in ? a.hist_ptr[r] : 0;
    const int64_t P = in ? a.hist_ptr[r + 1] - off : 0;
    const bool act = P > 0;
    // an empty row keeps its parameters; its loss is the empty sum
    if (in && !act && sub == 0 && a.loss_out != nullptr) a.loss_out[r] = 0.0f;
    const int64_t maxP = wave_max64(P);
    if (maxP == 0) return;

    const int D = a.dim, n = a.n_neg, loss = a.loss;
    const float *__restrict__ Q = a.item_w;
    const float *__restrict__ C = a.item_b;
    float p[EPL], m[EPL], v[EPL], g[EPL];
    float pb = 0.0f, mb = 0.0f, vb = 0.0f;
    L::zero(p); L::zero(m); L::zero(v);
    if (act) {
        L::load(p, a.user_w, r, D, sub);
        pb = a.user_b[r];
    }
    const float inv_p = 1.0f / (float)(act ? P : 1);
    const float inv_pn = 1.0f / (float)(act && n > 0 ? P * (int64_t)n : 1);
    const bool pointwise = loss == RG_LOSS_POINTWISE, adaptive = loss == RG_LOSS_ADAPTIVE_HINGE;
    rg_opt_t o = a.opt;
    float la = 0.0f, lb = 0.0f;

    for (int t = 0; t < a.steps; ++t) {
        const float2 sc = a.step_coef[t];
        o.step_size = sc.x;
        o.bias_correction2_sqrt = sc.y;
        const bool want_loss = a.loss_out != nullptr && t == a.steps - 1;
        float gb = 0.0f;
        L::zero(g);
        la = lb = 0.0f;

        for (int64_t p0 = 0; p0 < maxP; p0 += kPB) {
            bool pv[kPB];
            int pid[kPB];
            int nid[kPB][kNC];
            // ids of the block's positives and of their first chunk of negatives: one round trip
#pragma unroll
            for (int u = 0; u < kPB; ++u) {
                pv[u] = p0 + u < P;
                pid[u] = pv[u] ? a.hist_idx[off + p0 + u] : 0;
#pragma unroll
                for (int c = 0; c < kNC; ++c)
                    nid[u][c] = (pv[u] && c < n) ? a.neg_idx[(off + p0 + u) * (int64_t)n + c] : 0;
            }
            float qp[kPB][EPL], cp[kPB];
            float qb[kPB][EPL];      // adaptive hinge: the row of the highest negative so far
            float tg[kPB][EPL], tgb[kPB], tl[kPB];   // the positive's own term: gradient, bias gradient, loss
            PosState st[kPB];
#pragma unroll
            for (int u = 0; u < kPB; ++u) {
                L::load(qp[u], Q, pid[u], D, sub);
                cp[u] = C[pid[u]];
                L::zero(qb[u]);
                L::zero(tg[u]);
                tgb[u] = tl[u] = 0.0f;
            }
            for (int j0 = 0; j0 < (n > 0 ? n : 1); j0 += kNC) {
                if (j0 > 0) {
#pragma unroll
                    for (int u = 0; u < kPB; ++u)
#pragma unroll
                        for (int c = 0; c < kNC; ++c)
                            nid[u][c] = (pv[u] && j0 + c < n) ? a.neg_idx[(off + p0 + u) * (int64_t)n + j0 + c] : 0;
                }
                float qn[kPB][kNC][EPL], cn[kPB][kNC];
#pragma unroll
                for (int u = 0; u < kPB; ++u)
#pragma unroll
                    for (int c = 0; c < kNC; ++c) {
                        L::load(qn[u][c], Q, nid[u][c], D, sub);
                        cn[u][c] = C[nid[u][c]];
                    }
                if (j0 == 0) {
#pragma unroll
                    for (int u = 0; u < kPB; ++u) {
                        st[u].sp = row_score<L>(p, qp[u], pb, cp[u]);
                        st[u].dpos = 0.0f;
                        st[u].best = -1.0f;
                    }
                }
#pragma unroll
                for (int u = 0; u < kPB; ++u) {
#pragma unroll
                    for (int c = 0; c < kNC; ++c) {
                        const bool nv = pv[u] && j0 + c < n;
                        const float sn = row_score<L>(p, qn[u][c], pb, cn[u][c]);
                        const float sp = st[u].sp;
                        float dzn = 0.0f;      // dL/dz of this negative
                        if (pointwise) {
                            // -max(log(1 - s), -100) / (P n): d/dz = s / (P n) where the log is not clamped
                            if (want_loss) tl[u] = nv ? tl[u] - fmaxf(logf(1.0f - sn), -100.0f) : tl[u];
                            dzn = (1.0f - sn > 0.0f) ? sn * inv_pn : 0.0f;
                        } else if (loss == RG_LOSS_BPR) {
                            const float sg = sigmoidf_ref(sp - sn);
                            tl[u] = nv ? tl[u] + (1.0f - sg) : tl[u];
                            const float dx = -(((1.0f - sg) * sg) * inv_pn);    // dL/ds(positive)
                            st[u].dpos = nv ? st[u].dpos + dx : st[u].dpos;
                            dzn = ((-dx) * (1.0f - sn)) * sn;
                        } else if (loss == RG_LOSS_HINGE) {
                            const float x = (sn - sp) + 1.0f;
                            tl[u] = nv ? tl[u] + fmaxf(x, 0.0f) : tl[u];
                            const float dx = x >= 0.0f ? inv_pn : 0.0f;        // clamp passes the gradient at 0
                            st[u].dpos = nv ? st[u].dpos - dx : st[u].dpos;
                            dzn = (dx * (1.0f - sn)) * sn;
                        } else {   // adaptive hinge: only the highest negative (the lowest j of equals) counts
                            const bool up = nv && sn > st[u].best;
                            st[u].best = up ? sn : st[u].best;
#pragma unroll
                            for (int e = 0; e < EPL; ++e) qb[u][e] = up ? qn[u][c][e] : qb[u][e];
                        }
                        if (!adaptive) {
#pragma unroll
                            for (int e = 0; e < EPL; ++e) tg[u][e] = nv ? fmaf(dzn, qn[u][c][e], tg[u][e]) : tg[u][e];
                            tgb[u] = nv ? tgb[u] + dzn : tgb[u];
                        }
                    }
                }
            }
            // the block's positives (and the adaptive hinge's winners)
#pragma unroll
            for (int u = 0; u < kPB; ++u) {
                const float sp = st[u].sp;
                float dzp;
                if (pointwise) {
                    if (want_loss) la = pv[u] ? la - fmaxf(logf(sp), -100.0f) : la;
                    lb = pv[u] ? lb + tl[u] : lb;
                    dzp = sp > 0.0f ? (sp - 1.0f) * inv_p : 0.0f;
                } else {
                    float dpos = st[u].dpos;
                    if (adaptive) {
                        const float best = st[u].best;
                        const float x = (best - sp) + 1.0f;
                        tl[u] = fmaxf(x, 0.0f);
                        const float dx = x >= 0.0f ? inv_p : 0.0f;
                        dpos = -dx;
                        const float dzb = (dx * (1.0f - best)) * best;
#pragma unroll
                        for (int e = 0; e < EPL; ++e) tg[u][e] = dzb * qb[u][e];
                        tgb[u] = dzb;
                    }
                    la = pv[u] ? la + tl[u] : la;
                    dzp = (dpos * (1.0f - sp)) * sp;
                }
#pragma unroll
                for (int e = 0; e < EPL; ++e) g[e] = pv[u] ? g[e] + fmaf(dzp, qp[u][e], tg[u][e]) : g[e];
                gb = pv[u] ? gb + (tgb[u] + dzp) : gb;
            }
        }

        // the step's Adam update (every lane of the group carries the same bias values)
#pragma unroll
        for (int e = 0; e < EPL; ++e) p[e] = opt_update(o, p[e], g[e], m[e], v[e]);
        pb = opt_update(o, pb, gb, mb, vb);
    }

    if (!act) return;
    L::store(a.user_w, r, D, sub, p);
    if (sub == 0) {
        a.user_b[r] = pb;
        if (a.loss_out != nullptr) {
            float lv;
            if (pointwise) lv = la * inv_p + (n > 0 ? lb * inv_pn : 0.0f);
            else lv = la * (adaptive ? inv_p : inv_pn);
            a.loss_out[r] = lv;
        }
    }
}

struct FoldLaunch {
    const FoldArgs &a;
    hipStream_t stream;
    template <class L>
    int operator()() const {
        return launch_row_groups<L>(mf_fold_kernel<L>, a.n_users, a, stream, "rg_mf_fold_in_users",
                                    "too many users for one launch");
    }
};

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int rg_mf_fold_in_users(void *stream, const float *item_w, const float *item_b, int32_t dim,
                                   int64_t num_items, const int64_t *hist_ptr, const int32_t *hist_idx,
                                   const int32_t *neg_idx, int32_t n_neg, int64_t n_users, int32_t loss,
                                   const rg_opt_t *opt, const float *step_coef, int32_t steps, float *user_w,
                                   float *user_b, float *loss_out) {
    if (!item_w || !item_b || !hist_ptr || !opt || !user_w || !user_b)
        return fail_arg("rg_mf_fold_in_users: null pointer");
    if (dim < 1 || dim > 256) return fail_arg("rg_mf_fold_in_users: dim must be in [1, 256]");
    if (num_items < 1 || num_items > (int64_t)INT_MAX)
        return fail_arg("rg_mf_fold_in_users: num_items must be in [1, 2^31 - 1]");
    if (n_neg < 0 || n_neg > 32) return fail_arg("rg_mf_fold_in_users: n_neg must be in [0, 32]");
    if (steps < 0 || steps > 1024) return fail_arg("rg_mf_fold_in_users: steps must be in [0, 1024]");
    if (n_users < 0) return fail_arg("rg_mf_fold_in_users: n_users < 0");
    if (loss != RG_LOSS_POINTWISE && loss != RG_LOSS_BPR && loss != RG_LOSS_HINGE && loss != RG_LOSS_ADAPTIVE_HINGE)
        return fail_arg("rg_mf_fold_in_users: loss must be pointwise, bpr, hinge or adaptive hinge");
    if (n_neg == 0 && loss != RG_LOSS_POINTWISE)
        return fail_arg("rg_mf_fold_in_users: the pairwise losses need n_neg >= 1");
    if (n_neg > 0 && !neg_idx) return fail_arg("rg_mf_fold_in_users: neg_idx is null with n_neg > 0");
    if (opt->kind != RG_OPT_ADAM) return fail_arg("rg_mf_fold_in_users: the optimizer must be Adam");
    if (steps == 0 || n_users == 0) return RG_OK;
    if (!hist_idx) return fail_arg("rg_mf_fold_in_users: hist_idx is null");
    if (!step_coef) return fail_arg("rg_mf_fold_in_users: step_coef is null");
    const FoldArgs a{item_w, item_b, dim, hist_ptr, hist_idx, neg_idx, n_neg, n_users, loss, *opt,
                     reinterpret_cast<const float2 *>(step_coef), steps, user_w, user_b, loss_out};
    const bool aligned = (((uintptr_t)item_w | (uintptr_t)user_w) & 15u) == 0;
    return dispatch_rows(dim, aligned, FoldLaunch{a, (hipStream_t)stream});
}
