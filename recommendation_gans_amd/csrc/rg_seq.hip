// The pooling sequence model (Covington et al. 2016: a user is the mean of the items seen so far):
// the fused training step's gradients (rg_seq_pool_grads), its dense Adam pass
// (rg_seq_adam_dense) and the final representations that serving reads (rg_seq_pool_repr).
//
// rg_seq_pool_grads: a sequence is owned by one group of L::LPU lanes (the pair kernel's row
// layout, rg_common.h: a lane holds EPL elements of every row), 64 / LPU sequences per wave, one
// wave per workgroup (the waves share nothing).  The running sum S of the rows seen so far and
// the non-padding count c stay in registers.  The layout dispatch, the dot and the launch are the
// row-group helpers of rg_common.h (dispatch_rows: the vector layouts need 16-byte rows, every
// other dim and an unaligned table take the scalar-load ones; row_dot; launch_row_groups).
//   forward walk, t = 0 .. L-1:  r_t = S / (c + 1); the target's row and the K negatives' rows are
//     gathered, the dots reduced over the group's lanes (DPP), the loss term and dz formed; the
//     target-side and negative-side gradients (dz * r_t, dz) go out as float atomics; the K + 1
//     dz of the position go to the workspace; then S += E[s_t], c += 1 when s_t is an item.
//   reverse walk, t = L-1 .. 0:  G = sum_{t' > t} g_t' is carried in registers (a suffix sum
//     formed as one, never as total minus prefix); G goes out to E[s_t] when s_t is an item; then
//     g_t = (dzp E[s_t] + sum_k dzn_k E[n_k]) / (c_t + 1) is rebuilt from the stored dz and a
//     second gather of the rows (L2) and added to G.
// The dz live in a global workspace, not in LDS as first sketched: at L = 1024, K = 16 one
// sequence's dz are 68 KB and a wave holds up to 32 sequences.  The group's first lane writes a
// position's dz and the same lane reads them back (program order of one thread), then broadcasts
// them over the group.
//
// The gradient rows are float atomic adds into the zeroed [num_items][dim + 1] buffer: the ORDER
// of a row's additions differs from run to run, so gradients agree between runs to float32
// rounding, not to the bit.  The loss does not: a sequence's terms are summed by its own group in
// position order into partial r, and one wave reduces the partials in a fixed order, in double.
// Row 0 (padding) is never written.
#include "rg_seq.h"

#include <limits.h>

namespace rg {
namespace {

struct SeqArgs {
    const int64_t *seq, *neg;
    const float *E, *b;
    int32_t dim, L, K, loss;
    int64_t B, num_items;
    float inv_count;
    float *grad, *dz, *partials;
};

template <class L>
__global__ void __launch_bounds__(kWave) seq_pool_grads_kernel(const SeqArgs a) {
    constexpr int LPU = L::LPU, EPL = L::EPL, UPW = L::UPW;
    const int lane = threadIdx.x;
    const int sub = lane & (LPU - 1);
    const int lead = lane & ~(LPU - 1);
    const int64_t r = (int64_t)blockIdx.x * UPW + lane / LPU;
    // a group past the batch walks sequence 0 with the others (the lane reductions need every
    // lane) and emits nothing
    const bool in = r < a.B;
    const int64_t row = in ? r : 0;
    const int D = a.dim, Ls = a.L, K = a.K, loss = a.loss;
    const float *__restrict__ E = a.E;
    const float *__restrict__ bias = a.b;
    const int64_t *__restrict__ s = a.seq + row * Ls;
    float *dzs = a.dz + row * (int64_t)Ls * (K + 1);
    const float w = a.inv_count;
    const bool adaptive = loss == RG_LOSS_ADAPTIVE_HINGE;

    float S[EPL];
    L::zero(S);
    int c = 0;
    float lsum = 0.0f;
    int64_t pid_next = safe_id(s[0], a.num_items);
    for (int t = 0; t < Ls; ++t) {
        const int64_t pid = pid_next;
        if (t + 1 < Ls) pid_next = safe_id(s[t + 1], a.num_items);
        // a padded position has no loss term, no gradient and adds nothing to S (a group's lanes
        // share pid, and every cross-lane step below stays inside the group)
        if (pid == 0) continue;
        const bool live = in;
        const float den = (float)(c + 1);
        float rt[EPL], qp[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) rt[e] = S[e] / den;
        L::load(qp, E, pid, D, sub);
        const float zp = bias[pid] + row_dot<L>(rt, qp);
        float dzp = 0.0f;
        float best = 0.0f, lterm = 0.0f;
        int bestk = -1;
        int64_t bestid = 0;
        for (int k = 0; k < K; ++k) {
            const int64_t nid = safe_id(a.neg[((int64_t)k * a.B + row) * Ls + t], a.num_items);
            float qn[EPL];
            L::load(qn, E, nid, D, sub);
            const float zn = bias[nid] + row_dot<L>(rt, qn);
            if (adaptive) {   // the highest negative, equal scores going to the lowest k
                if (bestk < 0 || zn > best) {
                    best = zn;
                    bestk = k;
                    bestid = nid;
                }
                continue;
            }
            float dzn;
            if (loss == RG_LOSS_BPR) {
                const float sg = sigmoidf_ref(zp - zn);
                lterm += 1.0f - sg;
                dzn = ((1.0f - sg) * sg) * w;
            } else {   // hinge; the clamp passes the gradient at 0
                const float x = (zn - zp) + 1.0f;
                lterm += fmaxf(x, 0.0f);
                dzn = x >= 0.0f ? w : 0.0f;
            }
            dzn = live ? dzn : 0.0f;
            dzp -= dzn;
            if (in && sub == 0) dzs[(int64_t)t * (K + 1) + 1 + k] = dzn;
            if (live && nid != 0 && dzn != 0.0f) emit_row<L>(a.grad, nid, D, sub, dzn, rt);
        }
        if (adaptive) {
            const float x = (best - zp) + 1.0f;
            lterm = fmaxf(x, 0.0f);
            const float dzn = (live && x >= 0.0f) ? w : 0.0f;
            dzp = -dzn;
            if (in && sub == 0)
                for (int k = 0; k < K; ++k) dzs[(int64_t)t * (K + 1) + 1 + k] = k == bestk ? dzn : 0.0f;
            if (live && bestid != 0 && dzn != 0.0f) emit_row<L>(a.grad, bestid, D, sub, dzn, rt);
        }
        if (in && sub == 0) dzs[(int64_t)t * (K + 1)] = dzp;
        if (live) {
            lsum += lterm;
            if (dzp != 0.0f) emit_row<L>(a.grad, pid, D, sub, dzp, rt);
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) S[e] += qp[e];
        ++c;
    }
    if (in && sub == 0) a.partials[r] = lsum;

    // reverse walk: G = sum_{t' > t} g_t'
    float G[EPL];
    L::zero(G);
    for (int t = Ls - 1; t >= 0; --t) {
        const int64_t pid = safe_id(s[t], a.num_items);
        if (pid == 0) continue; // no dz was stored for a padded position, and G does not reach it
        --c;                    // c_t: the items before position t
        if (in && t < Ls - 1) {
            float *g = a.grad + pid * (int64_t)(D + 1);
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int col = L::elem(sub, e);
                if (col < D) unsafeAtomicAdd(g + col, G[e]);
            }
        }
        if (t == 0) break;      // r_0 = 0 whatever the tables hold: g_0 reaches nothing
        const float den = (float)(c + 1);
        float acc[EPL], q[EPL];
        float dz = sub == 0 ? dzs[(int64_t)t * (K + 1)] : 0.0f;
        dz = __shfl(dz, lead);
        L::load(q, E, pid, D, sub);
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = dz * q[e];
        for (int k = 0; k < K; ++k) {
            float dzn = sub == 0 ? dzs[(int64_t)t * (K + 1) + 1 + k] : 0.0f;
            dzn = __shfl(dzn, lead);
            const int64_t nid = safe_id(a.neg[((int64_t)k * a.B + row) * Ls + t], a.num_items);
            L::load(q, E, nid, D, sub);
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[e] = fmaf(dzn, q[e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) G[e] += acc[e] / den;
    }
}

// loss = sum(partials) * inv_count: lane l sums partials l, l + 64, ... in order, then the
// butterfly -- the same order on every run
__global__ void __launch_bounds__(kWave) seq_loss_kernel(const float *__restrict__ partials, int64_t n,
                                                         double inv_count, float *out) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kWave) s += (double)partials[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) *out = (float)(s * inv_count);
}

struct SeqLaunch {
    const SeqArgs &a;
    hipStream_t stream;
    template <class L>
    int operator()() const {
        return launch_row_groups<L>(seq_pool_grads_kernel<L>, a.B, a, stream, "rg_seq_pool_grads",
                                    "too many sequences for one launch");
    }
};

// ------------------------------------------------------------------ dense Adam
struct SeqAdamArgs {
    float *E, *b, *mE, *vE, *mb, *vb, *grad;
    int64_t num_items;
    int32_t dim;
    rg_opt_t opt;
};

// element i of the [num_items][dim + 1] gradient buffer: the update of its parameter
// (opt_update, the MF dense pass's op order), then the gradient zeroed for the next step.
// Row 0 is padding: its gradient slot is zeroed and nothing else of it is touched.
__global__ void __launch_bounds__(256) seq_adam_kernel(const SeqAdamArgs a) {
    const int64_t n = a.num_items * (int64_t)(a.dim + 1);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t row = i / (a.dim + 1);
        const int col = (int)(i - row * (a.dim + 1));
        const float g = a.grad[i];
        a.grad[i] = 0.0f;
        if (row == 0) continue;
        if (col < a.dim) {
            const int64_t j = row * a.dim + col;
            float m = a.mE[j], v = a.vE[j];
            a.E[j] = opt_update(a.opt, a.E[j], g, m, v);
            a.mE[j] = m;
            a.vE[j] = v;
        } else {
            float m = a.mb[row], v = a.vb[row];
            a.b[row] = opt_update(a.opt, a.b[row], g, m, v);
            a.mb[row] = m;
            a.vb[row] = v;
        }
    }
}

// ------------------------------------------------------------------ final representations
struct SeqReprArgs {
    const float *E;
    const int64_t *ids, *ptr;
    int32_t dim, L;
    int64_t n, num_items;
    float *out;
};

template <class L>
__global__ void __launch_bounds__(kWave) seq_pool_repr_kernel(const SeqReprArgs a) {
    constexpr int LPU = L::LPU, EPL = L::EPL, UPW = L::UPW;
    const int lane = threadIdx.x;
    const int sub = lane & (LPU - 1);
    const int64_t r = (int64_t)blockIdx.x * UPW + lane / LPU;
    if (r >= a.n) return;   // no lane reductions here: a group's work is its own
    const int64_t begin = a.ptr ? a.ptr[r] : r * a.L;
    const int64_t end = a.ptr ? a.ptr[r + 1] : begin + a.L;
    constexpr int kU = 4;   // rows in flight per group
    float S[EPL];
    L::zero(S);
    int c = 0;
    for (int64_t j0 = begin; j0 < end; j0 += kU) {
        int64_t id[kU];
        float q[kU][EPL];
#pragma unroll
        for (int u = 0; u < kU; ++u) id[u] = j0 + u < end ? safe_id(a.ids[j0 + u], a.num_items) : 0;
#pragma unroll
        for (int u = 0; u < kU; ++u) L::load(q[u], a.E, id[u], a.dim, sub);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (id[u] != 0) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) S[e] += q[u][e];
                ++c;
            }
        }
    }
    const float den = (float)(c + 1);
#pragma unroll
    for (int e = 0; e < EPL; ++e) S[e] /= den;
    L::store(a.out, r, a.dim, sub, S);
}

struct SeqReprLaunch {
    const SeqReprArgs &a;
    hipStream_t stream;
    template <class L>
    int operator()() const {
        return launch_row_groups<L>(seq_pool_repr_kernel<L>, a.n, a, stream, "rg_seq_pool_repr",
                                    "too many sequences for one launch");
    }
};

bool seq_dim_ok(int32_t dim) { return dim >= 4 && dim <= 256 && dim % 4 == 0; }

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int64_t rg_seq_pool_workspace_len(int64_t B, int32_t L, int32_t K) {
    if (B < 0 || L < 1 || L > RG_SEQ_MAX_LEN || K < 1 || K > RG_SEQ_MAX_NEG) return -1;
    return B * (int64_t)L * (K + 1) + B;
}

extern "C" int rg_seq_pool_grads(void *stream, const int64_t *seq, const int64_t *neg, const float *E,
                                 const float *b, int32_t dim, int64_t num_items, int64_t B, int32_t L, int32_t K,
                                 int32_t loss, float inv_count, float *grad, float *workspace, float *loss_out) {
    if (!seq || !neg || !E || !b || !grad || !workspace || !loss_out)
        return fail_arg("rg_seq_pool_grads: null pointer");
    if (!seq_dim_ok(dim)) return fail_arg("rg_seq_pool_grads: dim must be a multiple of 4 in [4, 256]");
    if (num_items < 2 || num_items > (int64_t)INT_MAX)
        return fail_arg("rg_seq_pool_grads: num_items must be in [2, 2^31 - 1]");
    if (L < 1 || L > RG_SEQ_MAX_LEN) return fail_arg("rg_seq_pool_grads: L must be in [1, 1024]");
    if (K < 1 || K > RG_SEQ_MAX_NEG) return fail_arg("rg_seq_pool_grads: K must be in [1, 16]");
    if (B < 1) return fail_arg("rg_seq_pool_grads: B < 1");
    if (loss != RG_LOSS_BPR && loss != RG_LOSS_HINGE && loss != RG_LOSS_ADAPTIVE_HINGE)
        return fail_arg("rg_seq_pool_grads: loss must be bpr, hinge or adaptive hinge (the reference's pointwise "
                        "loss takes probabilities and drops the mask)");
    if (!(inv_count > 0.0f) || inv_count > 1.0f)
        return fail_arg("rg_seq_pool_grads: inv_count must be 1 / (number of non-padding positions), in (0, 1]");
    float *partials = workspace + B * (int64_t)L * (K + 1);
    const SeqArgs a{seq, neg, E, b, dim, L, K, loss, B, num_items, inv_count, grad, workspace, partials};
    const bool aligned = ((uintptr_t)E & 15u) == 0;
    const int rc = dispatch_rows(dim, aligned, SeqLaunch{a, (hipStream_t)stream});
    if (rc != RG_OK) return rc;
    hipLaunchKernelGGL(seq_loss_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, partials, B,
                       (double)inv_count, loss_out);
    return check_launch("rg_seq_pool_grads (loss)");
}

extern "C" int rg_seq_adam_dense(void *stream, float *E, float *b, float *mE, float *vE, float *mb, float *vb,
                                 float *grad, int32_t dim, int64_t num_items, const rg_opt_t *opt) {
    if (!E || !b || !mE || !vE || !mb || !vb || !grad || !opt) return fail_arg("rg_seq_adam_dense: null pointer");
    if (dim < 1 || dim > 256) return fail_arg("rg_seq_adam_dense: dim must be in [1, 256]");
    if (num_items < 1 || num_items > (int64_t)INT_MAX)
        return fail_arg("rg_seq_adam_dense: num_items must be in [1, 2^31 - 1]");
    if (opt->kind != RG_OPT_ADAM) return fail_arg("rg_seq_adam_dense: the optimizer must be Adam");
    const SeqAdamArgs a{E, b, mE, vE, mb, vb, grad, num_items, dim, *opt};
    const int64_t n = num_items * (int64_t)(dim + 1);
    const int64_t want = (n + 255) / 256, cap = (int64_t)num_cus() * 8;
    hipLaunchKernelGGL(seq_adam_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return check_launch("rg_seq_adam_dense");
}

extern "C" int rg_seq_pool_repr(void *stream, const float *E, int32_t dim, int64_t num_items, const int64_t *ids,
                                const int64_t *ptr, int32_t L, int64_t n, float *out) {
    if (!E || !out) return fail_arg("rg_seq_pool_repr: null pointer");
    if (!seq_dim_ok(dim)) return fail_arg("rg_seq_pool_repr: dim must be a multiple of 4 in [4, 256]");
    if (num_items < 2 || num_items > (int64_t)INT_MAX)
        return fail_arg("rg_seq_pool_repr: num_items must be in [2, 2^31 - 1]");
    if (n < 0) return fail_arg("rg_seq_pool_repr: n < 0");
    if (!ptr && (L < 0 || L > RG_SEQ_MAX_LEN)) return fail_arg("rg_seq_pool_repr: L must be in [0, 1024]");
    if (n == 0) return RG_OK;
    if (!ids && (ptr || L > 0)) return fail_arg("rg_seq_pool_repr: ids is null");
    const SeqReprArgs a{E, ids, ptr, dim, L, n, num_items, out};
    const bool aligned = (((uintptr_t)E | (uintptr_t)out) & 15u) == 0;
    return dispatch_rows(dim, aligned, SeqReprLaunch{a, (hipStream_t)stream});
}
