// The causal-convolution sequence model (CNNNet of the reference's sequence/representations.py;
// include/rg_hip.h states the model): the training step's gradients (rg_seq_cnn_grads), the final
// representations that serving reads (rg_seq_cnn_repr) and Adam on the flat vector of the
// convolutions' parameters (rg_seq_adam_flat).
//
// Rows.  Position t = 0 .. L of sequence b is row b (L + 1) + t of every activation buffer
// [B (L + 1)][d].  Layer 0 reads the virtual rows u_t = E[s_{t-1}] (u_0 = 0, a padded or
// out-of-table id = 0), gathered from E by id; with them layer 0 is the formula of every other
// layer, x_t = f(c + sum_j W[j] in_{t - (w-1-j) dil}) (+ in_t), rows before the sequence reading 0.
//
// A step is 3 num_layers + 3 launches, each a plain grid of independent waves:
//   conv (per layer)     one wave per 16 rows: 16 x d output tile on the fp32 16x16x4 MFMA, the A
//                        operand gathered per tap with its shift straight into the operand layout
//                        (lane l: row l & 15, k = l >> 4), W[j] the B operand from global memory
//                        (w d^2 floats, L2-resident); bias, f and the residual in the epilogue.
//                        y = f(pre) is kept beside x = y + in when there is a residual: f' is
//                        taken from y exactly (tanh: 1 - y^2, relu: y > 0).
//   score                the row-group layout of rg_common.h, one group per row: the target's
//                        and the K negatives' scores under x_t of the top layer, the loss term,
//                        dz, the item-side gradients as float atomics (pooling's emit_row) and
//                        dx_t = dzp E[s_t] + sum_k dzn_k E[n_k] to the workspace.  No walk along
//                        t: every position is its own row.
//   loss                 one workgroup sums the rows' terms in a fixed order, in double.
//   wgrad (per layer)    dW[j] = in_shifted^T dpre over the rows, dpre = dx * f'(y) formed while
//                        the B operand is loaded.  A wave owns (slice of rows, tap, 16 input
//                        channels) and all d output channels, and writes its sums to the slice's
//                        own copy of the parameter vector: no atomics.  dc: column sums of dpre in
//                        the tap-0 waves.
//   input grad (per layer) dx_in = sum_j dpre_{t + (w-1-j) dil} W[j]^T (+ dx when residual), rows
//                        past the sequence's end reading 0; the same 16-row tiles as conv.  Layer
//                        0 adds its result to grad[s_{t-1}] with float atomics.
//   reduce               param_grad[i] = sum over slices in slice order: the same bits every run.
// Separate launches, not one persistent kernel: each stage needs every row of the one before (a
// tap reaches back up to 448 rows, the weight gradient sums over all of them), so fusing them
// needs a grid-wide barrier per stage; the activations are a few MB and stay in L2 / MALL between
// launches.
#include "rg_mfma.h"
#include "rg_seq.h"

#include <limits.h>

namespace rg {
namespace {

constexpr int kMaxSlices = 64;     // row slices of the weight gradient (copies of the parameter vector)
constexpr int kSliceRows = 256;    // fewer slices for small batches: at least this many rows each

// where a layer's input rows come from
struct InSrc {
    const float *in;         // the previous layer's x [n][Tin][d]; null: layer 0, rows of E by id
    const float *E;
    const int64_t *ids;      // [n][L]
    int64_t num_items;
    int32_t L, Tin, d;
};

// the input row of sequence b at position p (<= L), null when it reads as zero
__device__ __forceinline__ const float *in_row(const InSrc &s, int64_t b, int p) {
    if (p < 0) return nullptr;
    if (!s.in) {
        if (p == 0) return nullptr;
        const int64_t id = safe_id(s.ids[b * s.L + (p - 1)], s.num_items);
        return id ? s.E + id * s.d : nullptr;
    }
    // the window [L + 1 - Tin, L] holds every position a later window reaches (cnn_windows)
    return s.in + (b * s.Tin + (p - (s.L + 1 - s.Tin))) * (int64_t)s.d;
}

__device__ __forceinline__ float act(float pre, int relu) { return relu ? fmaxf(pre, 0.0f) : tanhf(pre); }
__device__ __forceinline__ float act_grad(float y, int relu) { return relu ? (y > 0.0f ? 1.0f : 0.0f) : 1.0f - y * y; }

// ------------------------------------------------------------------ forward: one layer
struct ConvArgs {
    InSrc s;
    const float *W, *c;      // [w][d][d], [d]
    float *y, *x;            // [n][Tout][d]; y null: not kept
    int64_t n;
    int32_t Tout, w, dil, relu, residual;
};

template <int DT>
__global__ void __launch_bounds__(kWave) cnn_conv_kernel(const ConvArgs a) {
    constexpr int d = 16 * DT;
    const int lane = threadIdx.x, g = lane >> 4, m = lane & 15;
    const int64_t R = a.n * a.Tout, r0 = (int64_t)blockIdx.x * 16;
    const int t0 = a.s.L + 1 - a.Tout;
    const int64_t ra = r0 + m;
    const bool va = ra < R;
    const int64_t ba = va ? ra / a.Tout : 0;
    const int ta = va ? (int)(ra - ba * a.Tout) + t0 : 0;
    // four accumulator sets, k-step s of every 16 channels into set s: independent MFMA chains (the
    // instruction's dependent latency exceeds its issue interval) and sums a quarter as long, added
    // pairwise at the end, which keeps x_t within the float32 error of a blocked host evaluation
    v4f part[4][DT];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int nt = 0; nt < DT; ++nt) part[s][nt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < a.w; ++j) {
        const float *src = va ? in_row(a.s, ba, ta - (a.w - 1 - j) * a.dil) : nullptr;
        const float *Wj = a.W + (int64_t)j * d * d + g * d + m;
        for (int k0 = 0; k0 < d; k0 += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float av = src ? src[k0 + 4 * s + g] : 0.0f;
#pragma unroll
                for (int nt = 0; nt < DT; ++nt)
                    part[s][nt] = mfma(av, Wj[(k0 + 4 * s) * d + nt * 16], part[s][nt]);
            }
        }
    }
    v4f acc[DT];
#pragma unroll
    for (int nt = 0; nt < DT; ++nt) acc[nt] = (part[0][nt] + part[1][nt]) + (part[2][nt] + part[3][nt]);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t r = r0 + 4 * g + v;
        if (r >= R) continue;
        const int64_t b = r / a.Tout;
        const float *res = a.residual ? in_row(a.s, b, (int)(r - b * a.Tout) + t0) : nullptr;
#pragma unroll
        for (int nt = 0; nt < DT; ++nt) {
            const int col = nt * 16 + m;
            const float y = act(acc[nt][v] + a.c[col], a.relu);
            if (a.y) a.y[r * d + col] = y;
            a.x[r * d + col] = res ? y + res[col] : y;
        }
    }
}

// ------------------------------------------------------------------ scores, loss terms, dz, dx
struct ScoreArgs {
    const int64_t *seq, *neg;
    const float *E, *b, *x;      // x: the top layer's [B (L + 1)][d]
    int32_t dim, L, K, loss;
    int64_t B, num_items;
    float inv_count;
    float *grad, *dx, *partials;
};

template <class L>
__global__ void __launch_bounds__(kWave) cnn_score_kernel(const ScoreArgs a) {
    constexpr int LPU = L::LPU, EPL = L::EPL, UPW = L::UPW;
    const int lane = threadIdx.x;
    const int sub = lane & (LPU - 1);
    const int D = a.dim, Ls = a.L, K = a.K, loss = a.loss;
    const int64_t R = a.B * (Ls + 1);
    const int64_t r = (int64_t)blockIdx.x * UPW + lane / LPU;
    // a group past the rows, at position L or on a padded target runs row 0's arithmetic with the
    // others (the lane reductions need every lane) and emits nothing
    const bool in = r < R;
    const int64_t bq = in ? r / (Ls + 1) : 0;
    const int t = in ? (int)(r - bq * (Ls + 1)) : Ls;
    const int64_t pid = t < Ls ? safe_id(a.seq[bq * Ls + t], a.num_items) : 0;
    const bool live = pid != 0;
    const float w = a.inv_count;
    const bool adaptive = loss == RG_LOSS_ADAPTIVE_HINGE;

    float x[EPL], qp[EPL], dx[EPL], qbest[EPL];
    L::load(x, a.x, in ? r : 0, D, sub);
    L::load(qp, a.E, pid, D, sub);
    L::zero(dx);
    L::zero(qbest);
    const float zp = a.b[pid] + row_dot<L>(x, qp);
    float dzp = 0.0f, best = 0.0f, lterm = 0.0f;
    int bestk = -1;
    int64_t bestid = 0;
    for (int k = 0; k < K; ++k) {
        const int64_t nid = t < Ls ? safe_id(a.neg[((int64_t)k * a.B + bq) * Ls + t], a.num_items) : 0;
        float qn[EPL];
        L::load(qn, a.E, nid, D, sub);
        const float zn = a.b[nid] + row_dot<L>(x, qn);
        if (adaptive) {   // the highest negative, equal scores going to the lowest k
            if (bestk < 0 || zn > best) {
                best = zn;
                bestk = k;
                bestid = nid;
#pragma unroll
                for (int e = 0; e < EPL; ++e) qbest[e] = qn[e];
            }
            continue;
        }
        float dzn;
        if (loss == RG_LOSS_BPR) {
            const float sg = sigmoidf_ref(zp - zn);
            lterm += 1.0f - sg;
            dzn = ((1.0f - sg) * sg) * w;
        } else {   // hinge; the clamp passes the gradient at 0
            const float h = (zn - zp) + 1.0f;
            lterm += fmaxf(h, 0.0f);
            dzn = h >= 0.0f ? w : 0.0f;
        }
        dzn = live ? dzn : 0.0f;
        dzp -= dzn;
#pragma unroll
        for (int e = 0; e < EPL; ++e) dx[e] = fmaf(dzn, qn[e], dx[e]);
        if (nid != 0 && dzn != 0.0f) emit_row<L>(a.grad, nid, D, sub, dzn, x);
    }
    if (adaptive) {
        const float h = (best - zp) + 1.0f;
        lterm = fmaxf(h, 0.0f);
        const float dzn = (live && h >= 0.0f) ? w : 0.0f;
        dzp = -dzn;
#pragma unroll
        for (int e = 0; e < EPL; ++e) dx[e] = dzn * qbest[e];
        if (bestid != 0 && dzn != 0.0f) emit_row<L>(a.grad, bestid, D, sub, dzn, x);
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) dx[e] = fmaf(dzp, qp[e], dx[e]);
    if (live && dzp != 0.0f) emit_row<L>(a.grad, pid, D, sub, dzp, x);
    if (in) {
        L::store(a.dx, r, D, sub, dx);   // zero at position L and under padding (every dz is)
        if (sub == 0) a.partials[r] = live ? lterm : 0.0f;
    }
}

// loss = sum(partials) * inv_count: thread i sums partials i, i + 1024, ... in order, then a
// tree over the threads -- the same order on every run
__global__ void __launch_bounds__(1024) cnn_loss_kernel(const float *__restrict__ partials, int64_t n,
                                                        double inv_count, float *out) {
    __shared__ double sh[1024];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += (double)partials[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (float)(sh[0] * inv_count);
}

// ------------------------------------------------------------------ backward: one layer
struct BackArgs {
    InSrc s;                 // the layer's input rows (Tin = L + 1)
    const float *dx, *y;     // d loss / d x of the layer's output and its f(pre), [B (L + 1)][d]
    const float *W;
    float *dxin;             // d loss / d input rows; null: layer 0, to grad by id
    float *grad;
    float *part;             // [slices][param_len]: the weight gradient's per-slice sums
    int64_t B, param_len, off_w, off_c;
    int32_t w, dil, relu, residual, slices;
};

template <int DT>
__global__ void __launch_bounds__(kWave) cnn_input_grad_kernel(const BackArgs a) {
    constexpr int d = 16 * DT;
    const int lane = threadIdx.x, g = lane >> 4, m = lane & 15;
    const int T = a.s.L + 1;
    const int64_t R = a.B * T, r0 = (int64_t)blockIdx.x * 16;
    const int64_t ra = r0 + m;
    const bool va = ra < R;
    const int64_t ba = va ? ra / T : 0;
    const int ta = va ? (int)(ra - ba * T) : 0;
    v4f acc[DT];
#pragma unroll
    for (int nt = 0; nt < DT; ++nt) acc[nt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < a.w; ++j) {
        // output row t + shift read this row through tap j; past the sequence's end there is none
        const int tq = ta + (a.w - 1 - j) * a.dil;
        const bool ok = va && tq < T;
        const int64_t q = ok ? (ba * T + tq) * d + g : 0;
        const float *Wj = a.W + (int64_t)j * d * d + m * d + g;   // B[k][n] = W[j][in n][out k]
        for (int k0 = 0; k0 < d; k0 += 4) {
            const float av = ok ? a.dx[q + k0] * act_grad(a.y[q + k0], a.relu) : 0.0f;
#pragma unroll
            for (int nt = 0; nt < DT; ++nt) acc[nt] = mfma(av, Wj[nt * 16 * d + k0], acc[nt]);
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t r = r0 + 4 * g + v;
        if (r >= R) continue;
        int64_t id = 0;
        if (!a.dxin) {   // layer 0: row (b, t) is E[s_{t-1}]
            const int64_t b = r / T;
            const int t = (int)(r - b * T);
            if (t > 0) id = safe_id(a.s.ids[b * a.s.L + (t - 1)], a.s.num_items);
            if (id == 0) continue;
        }
#pragma unroll
        for (int nt = 0; nt < DT; ++nt) {
            const int col = nt * 16 + m;
            const float val = a.residual ? acc[nt][v] + a.dx[r * d + col] : acc[nt][v];
            if (a.dxin)
                a.dxin[r * d + col] = val;
            else
                unsafeAtomicAdd(a.grad + id * (int64_t)(d + 1) + col, val);
        }
    }
}

// grid (slices, w * DT): block (s, j * DT + mt) sums rows of slice s into dW[j][16 mt .. + 16][:]
template <int DT>
__global__ void __launch_bounds__(kWave) cnn_wgrad_kernel(const BackArgs a) {
    constexpr int d = 16 * DT;
    const int lane = threadIdx.x, g = lane >> 4, m = lane & 15;
    const int T = a.s.L + 1;
    const int64_t R = a.B * T;
    const int j = blockIdx.y / DT, mt = blockIdx.y % DT;
    const int64_t per = (((R + a.slices - 1) / a.slices) + 3) & ~(int64_t)3;
    const int64_t rs = (int64_t)blockIdx.x * per;
    const int64_t re = rs + per < R ? rs + per : R;
    const int shift = (a.w - 1 - j) * a.dil;
    v4f acc[DT];
    float bsum[DT];
#pragma unroll
    for (int nt = 0; nt < DT; ++nt) {
        acc[nt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        bsum[nt] = 0.0f;
    }
    for (int64_t rr = rs; rr < re; rr += 4) {
        const int64_t r = rr + g;
        const bool ok = r < re;
        const int64_t b = ok ? r / T : 0;
        const float *src = ok ? in_row(a.s, b, (int)(r - b * T) - shift) : nullptr;
        const float av = src ? src[mt * 16 + m] : 0.0f;
        const int64_t q = ok ? r * d + m : 0;
#pragma unroll
        for (int nt = 0; nt < DT; ++nt) {
            const float bv = ok ? a.dx[q + nt * 16] * act_grad(a.y[q + nt * 16], a.relu) : 0.0f;
            acc[nt] = mfma(av, bv, acc[nt]);
            bsum[nt] += bv;
        }
    }
    float *part = a.part + (int64_t)blockIdx.x * a.param_len;
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int nt = 0; nt < DT; ++nt)
            part[a.off_w + ((int64_t)j * d + mt * 16 + 4 * g + v) * d + nt * 16 + m] = acc[nt][v];
    if (blockIdx.y == 0) {
#pragma unroll
        for (int nt = 0; nt < DT; ++nt) {
            float s = bsum[nt];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (g == 0) part[a.off_c + nt * 16 + m] = s;
        }
    }
}

__global__ void __launch_bounds__(256) cnn_reduce_kernel(const float *__restrict__ part, int slices, int64_t n,
                                                         float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int k = 1; k < slices; ++k) s += part[(int64_t)k * n + i];
    out[i] = s;
}

// ------------------------------------------------------------------ Adam on a flat vector
struct FlatAdamArgs {
    float *p, *m, *v;
    const float *g;
    int64_t n;
    rg_opt_t opt;
};

__global__ void __launch_bounds__(256) seq_adam_flat_kernel(const FlatAdamArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        float m = a.m[i], v = a.v[i];
        a.p[i] = opt_update(a.opt, a.p[i], a.g[i], m, v);
        a.m[i] = m;
        a.v[i] = v;
    }
}

// ------------------------------------------------------------------ host
const char *cfg_error(const rg_seq_cnn_t *c) {
    if (!c) return "null configuration";
    if (c->dim < 16 || c->dim > 128 || c->dim % 16) return "dim must be a multiple of 16 in [16, 128]";
    if (c->num_layers < 1 || c->num_layers > RG_SEQ_CNN_MAX_LAYERS) return "num_layers must be in [1, 4]";
    if (c->nonlinearity != 0 && c->nonlinearity != 1) return "nonlinearity must be 0 (tanh) or 1 (relu)";
    if (c->residual != 0 && c->residual != 1) return "residual must be 0 or 1";
    for (int l = 0; l < c->num_layers; ++l) {
        if (c->width[l] < 1 || c->width[l] > RG_SEQ_CNN_MAX_WIDTH) return "every width must be in [1, 8]";
        if (c->dilation[l] < 1 || c->dilation[l] > 64) return "every dilation must be in [1, 64]";
    }
    return nullptr;
}

int64_t layer_len(const rg_seq_cnn_t &c, int l) { return ((int64_t)c.width[l] * c.dim + 1) * c.dim; }

int slices_for(int64_t R) {
    const int64_t s = R / kSliceRows;
    return s < 1 ? 1 : s > kMaxSlices ? kMaxSlices : (int)s;
}

// rows (tiles of 16) of one launch
bool rows_ok(int64_t n, int64_t T) { return n <= ((int64_t)INT_MAX - 15) / T; }

template <class F>
int dispatch_dt(int dim, F &&f) {
    switch (dim / 16) {
        case 1: return f.template operator()<1>();
        case 2: return f.template operator()<2>();
        case 3: return f.template operator()<3>();
        case 4: return f.template operator()<4>();
        case 5: return f.template operator()<5>();
        case 6: return f.template operator()<6>();
        case 7: return f.template operator()<7>();
        default: return f.template operator()<8>();
    }
}

struct ConvLaunch {
    const ConvArgs &a;
    hipStream_t stream;
    template <int DT>
    int operator()() const {
        const int64_t tiles = (a.n * a.Tout + 15) / 16;
        hipLaunchKernelGGL(cnn_conv_kernel<DT>, dim3((unsigned)tiles), dim3(kWave), 0, stream, a);
        return check_launch("rg_seq_cnn (conv)");
    }
};

struct BackLaunch {
    const BackArgs &a;
    hipStream_t stream;
    template <int DT>
    int operator()() const {
        hipLaunchKernelGGL(cnn_wgrad_kernel<DT>, dim3((unsigned)a.slices, (unsigned)(a.w * DT)), dim3(kWave), 0,
                           stream, a);
        int rc = check_launch("rg_seq_cnn_grads (weight gradient)");
        if (rc != RG_OK) return rc;
        const int64_t tiles = (a.B * (a.s.L + 1) + 15) / 16;
        hipLaunchKernelGGL(cnn_input_grad_kernel<DT>, dim3((unsigned)tiles), dim3(kWave), 0, stream, a);
        return check_launch("rg_seq_cnn_grads (input gradient)");
    }
};

struct ScoreLaunch {
    const ScoreArgs &a;
    hipStream_t stream;
    template <class L>
    int operator()() const {
        return launch_row_groups<L>(cnn_score_kernel<L>, a.B * (a.L + 1), a, stream, "rg_seq_cnn_grads (scores)",
                                    "too many positions for one launch");
    }
};

// the positions a layer has to produce for the top layer's x_L alone: T[top] = 1 and each layer
// below the window its successor's taps reach, cut at the sequence's start
void cnn_windows(const rg_seq_cnn_t &c, int L, int (&T)[RG_SEQ_CNN_MAX_LAYERS]) {
    T[c.num_layers - 1] = 1;
    for (int l = c.num_layers - 1; l > 0; --l) {
        const int t = T[l] + (c.width[l] - 1) * c.dilation[l];
        T[l - 1] = t < L + 1 ? t : L + 1;
    }
}

}  // namespace
}  // namespace rg

using namespace rg;

extern "C" int64_t rg_seq_cnn_param_len(const rg_seq_cnn_t *cfg) {
    if (cfg_error(cfg)) return -1;
    int64_t n = 0;
    for (int l = 0; l < cfg->num_layers; ++l) n += layer_len(*cfg, l);
    return n;
}

extern "C" int64_t rg_seq_cnn_workspace_len(const rg_seq_cnn_t *cfg, int64_t B, int32_t L, int32_t K) {
    if (cfg_error(cfg) || B < 0 || L < 1 || L > RG_SEQ_MAX_LEN || K < 1 || K > RG_SEQ_MAX_NEG || !rows_ok(B, L + 1))
        return -1;
    const int64_t R = B * (L + 1), act = R * cfg->dim;
    return act * cfg->num_layers * (cfg->residual ? 2 : 1) + 2 * act + R + slices_for(R) * rg_seq_cnn_param_len(cfg);
}

extern "C" int rg_seq_cnn_grads(void *stream, const rg_seq_cnn_t *cfg, const int64_t *seq, const int64_t *neg,
                                const float *E, const float *b, const float *params, int64_t num_items, int64_t B,
                                int32_t L, int32_t K, int32_t loss, float inv_count, float *grad, float *param_grad,
                                float *workspace, float *loss_out) {
    if (!seq || !neg || !E || !b || !params || !grad || !param_grad || !workspace || !loss_out)
        return fail_arg("rg_seq_cnn_grads: null pointer");
    if (const char *why = cfg_error(cfg)) return fail_arg(std::string("rg_seq_cnn_grads: ") + why);
    if (num_items < 2 || num_items > (int64_t)INT_MAX)
        return fail_arg("rg_seq_cnn_grads: num_items must be in [2, 2^31 - 1]");
    if (L < 1 || L > RG_SEQ_MAX_LEN) return fail_arg("rg_seq_cnn_grads: L must be in [1, 1024]");
    if (K < 1 || K > RG_SEQ_MAX_NEG) return fail_arg("rg_seq_cnn_grads: K must be in [1, 16]");
    if (B < 1) return fail_arg("rg_seq_cnn_grads: B < 1");
    if (!rows_ok(B, L + 1)) return fail_arg("rg_seq_cnn_grads: too many positions for one launch");
    if (loss != RG_LOSS_BPR && loss != RG_LOSS_HINGE && loss != RG_LOSS_ADAPTIVE_HINGE)
        return fail_arg("rg_seq_cnn_grads: loss must be bpr, hinge or adaptive hinge (the reference's pointwise "
                        "loss takes probabilities and drops the mask)");
    if (!(inv_count > 0.0f) || inv_count > 1.0f)
        return fail_arg("rg_seq_cnn_grads: inv_count must be 1 / (number of non-padding positions), in (0, 1]");
    const hipStream_t st = (hipStream_t)stream;
    const rg_seq_cnn_t &c = *cfg;
    const int d = c.dim, nl = c.num_layers;
    const int64_t R = B * (L + 1), act = R * d, plen = rg_seq_cnn_param_len(cfg);
    const int slices = slices_for(R);
    float *x[RG_SEQ_CNN_MAX_LAYERS], *y[RG_SEQ_CNN_MAX_LAYERS];
    float *w = workspace;
    for (int l = 0; l < nl; ++l) {
        x[l] = w, w += act;
        y[l] = x[l];
        if (c.residual) y[l] = w, w += act;
    }
    float *dx[2] = {w, w + act};
    float *partials = w + 2 * act, *part = partials + R;

    int64_t off[RG_SEQ_CNN_MAX_LAYERS];
    for (int l = 0, o = 0; l < nl; o += layer_len(c, l), ++l) off[l] = o;
    auto src = [&](int l) { return InSrc{l ? x[l - 1] : nullptr, E, seq, num_items, L, L + 1, d}; };
    for (int l = 0; l < nl; ++l) {
        const float *W = params + off[l];
        const ConvArgs a{src(l), W, W + (int64_t)c.width[l] * d * d, c.residual ? y[l] : nullptr, x[l], B,
                         L + 1, c.width[l], c.dilation[l], c.nonlinearity, c.residual};
        const int rc = dispatch_dt(d, ConvLaunch{a, st});
        if (rc != RG_OK) return rc;
    }
    {
        const ScoreArgs a{seq, neg, E, b, x[nl - 1], d, L, K, loss, B, num_items, inv_count, grad, dx[0], partials};
        const bool aligned = (((uintptr_t)E | (uintptr_t)workspace) & 15u) == 0;
        int rc = dispatch_rows<128>(d, aligned, ScoreLaunch{a, st});
        if (rc != RG_OK) return rc;
        hipLaunchKernelGGL(cnn_loss_kernel, dim3(1), dim3(1024), 0, st, partials, R, (double)inv_count, loss_out);
        rc = check_launch("rg_seq_cnn_grads (loss)");
        if (rc != RG_OK) return rc;
    }
    for (int l = nl - 1, cur = 0; l >= 0; --l, cur ^= 1) {
        const BackArgs a{src(l), dx[cur], y[l], params + off[l], l ? dx[cur ^ 1] : nullptr, grad, part, B, plen,
                         off[l], off[l] + (int64_t)c.width[l] * d * d, c.width[l], c.dilation[l], c.nonlinearity,
                         c.residual, slices};
        const int rc = dispatch_dt(d, BackLaunch{a, st});
        if (rc != RG_OK) return rc;
    }
    hipLaunchKernelGGL(cnn_reduce_kernel, dim3((unsigned)((plen + 255) / 256)), dim3(256), 0, st, part, slices, plen,
                       param_grad);
    return check_launch("rg_seq_cnn_grads (reduce)");
}

extern "C" int64_t rg_seq_cnn_repr_workspace_len(const rg_seq_cnn_t *cfg, int64_t n, int32_t L) {
    if (cfg_error(cfg) || n < 0 || L < 0 || L > RG_SEQ_MAX_LEN || !rows_ok(n, L + 1)) return -1;
    int T[RG_SEQ_CNN_MAX_LAYERS];
    cnn_windows(*cfg, L, T);
    int64_t rows = 0;
    for (int l = 0; l + 1 < cfg->num_layers; ++l) rows += T[l];
    return n * rows * cfg->dim;
}

extern "C" int rg_seq_cnn_repr(void *stream, const rg_seq_cnn_t *cfg, const float *E, const float *params,
                               int64_t num_items, const int64_t *ids, int32_t L, int64_t n, float *workspace,
                               float *out) {
    if (!E || !params || !out) return fail_arg("rg_seq_cnn_repr: null pointer");
    if (const char *why = cfg_error(cfg)) return fail_arg(std::string("rg_seq_cnn_repr: ") + why);
    if (num_items < 2 || num_items > (int64_t)INT_MAX)
        return fail_arg("rg_seq_cnn_repr: num_items must be in [2, 2^31 - 1]");
    if (n < 0) return fail_arg("rg_seq_cnn_repr: n < 0");
    if (L < 0 || L > RG_SEQ_MAX_LEN) return fail_arg("rg_seq_cnn_repr: L must be in [0, 1024]");
    if (!rows_ok(n, L + 1)) return fail_arg("rg_seq_cnn_repr: too many positions for one launch");
    if (n == 0) return RG_OK;
    if (!ids && L > 0) return fail_arg("rg_seq_cnn_repr: ids is null");
    if (!workspace && rg_seq_cnn_repr_workspace_len(cfg, n, L) > 0)
        return fail_arg("rg_seq_cnn_repr: workspace is null");
    const rg_seq_cnn_t &c = *cfg;
    const int d = c.dim, nl = c.num_layers;
    int T[RG_SEQ_CNN_MAX_LAYERS];
    cnn_windows(c, L, T);
    const float *W = params, *prev = nullptr;
    float *w = workspace;
    for (int l = 0; l < nl; ++l) {
        float *dst = l + 1 < nl ? w : out;
        const ConvArgs a{InSrc{prev, E, ids, num_items, L, l ? T[l - 1] : L + 1, d}, W, W + (int64_t)c.width[l] * d * d,
                         nullptr, dst, n, T[l], c.width[l], c.dilation[l], c.nonlinearity, c.residual};
        const int rc = dispatch_dt(d, ConvLaunch{a, (hipStream_t)stream});
        if (rc != RG_OK) return rc;
        prev = dst;
        if (l + 1 < nl) w += n * (int64_t)T[l] * d;
        W += layer_len(c, l);
    }
    return RG_OK;
}

extern "C" int rg_seq_adam_flat(void *stream, float *p, float *m, float *v, const float *g, int64_t n,
                                const rg_opt_t *opt) {
    if (!p || !m || !v || !g || !opt) return fail_arg("rg_seq_adam_flat: null pointer");
    if (n < 0) return fail_arg("rg_seq_adam_flat: n < 0");
    if (opt->kind != RG_OPT_ADAM) return fail_arg("rg_seq_adam_flat: the optimizer must be Adam");
    if (n == 0) return RG_OK;
    const FlatAdamArgs a{p, m, v, g, n, *opt};
    const int64_t want = (n + 255) / 256, cap = (int64_t)num_cus() * 8;
    hipLaunchKernelGGL(seq_adam_flat_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return check_launch("rg_seq_adam_flat");
}
