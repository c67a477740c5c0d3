// Device side of the matrix-factorisation step shared by rg_mf.hip (the kernels and entry
// points of the product path) and rg_mf_alt.hip (the measured-slower whole-step alternatives
// of the A/B build): constants, kernel argument structs, and the __device__
// bodies both files' kernels are made of -- the prepare body, the pair pass (pairs_body),
// the per-row gradient pull + optimizer update (apply_row, the lean_load / lean_finish
// split) and the loss finalisers.  Row layouts and dispatch_dim are in rg_common.h.
//
// Device functions and types only: no __global__ kernel, no launch functor, no extern "C".
// The library is built without relocatable device code, so every kernel is defined and
// launched in exactly one of the two translation units; the host helpers declared at the
// end are defined once, in rg_mf.hip.  Both files must be compiled with the same -D
// defines (build.py treats them as one unit).
#pragma once
#include "rg_common.h"
#include "rg_mt.h"
#include "rg_owner.h"
#include "rg_mlp_update.h"

namespace rg {

constexpr int kCap = RG_MF_LIST_CAP;
constexpr int kNMax = RG_MF_MAX_NEG;
constexpr int kBlock = 256;
constexpr int kPairBlock = 256;   // threads of a pair-pass workgroup (the plan's block)
constexpr int kPullGroup = 4;     // list entries whose partner rows apply_row loads per round
constexpr int kLeanPullGroup = 2; // the same for lean_finish (one entry per lane)

// kFused: forward + loss + lists.  kLossOnly: forward + loss (validation).
// Adaptive hinge needs the global max first: kAdaptFwd (scores + max),
// then kAdaptBwd (positives vs max + lists) or kAdaptLoss (loss only).
enum Phase : int { kFused = 0, kLossOnly = 1, kAdaptFwd = 2, kAdaptBwd = 3, kAdaptLoss = 4 };

struct PairsArgs {
    const float *user_w, *item_w, *user_b, *item_b;
    int64_t num_users;
    int32_t dim;
    const int64_t *pos_user, *pos_item;
    int64_t n_pos, cols, col_offset, global_cols;
    const uint2 *words;
    const int2 *pool;
    int64_t pool_len;
    int32_t n_neg, loss;
    float n_a, n_b;            // mean denominators (as ATen divides: grad / numel)
    int32_t *row_count;
    int2 *row_list;
    long long *hot_grad, *hot_bias_grad;     // int64 fixed point (rg_common.h fix_add)
    float *partials;
    float *scores;             // adaptive: [cols] positive scores
    unsigned long long *max_key;
    int32_t *active_count;
    const int32_t *perm;       // plan: processing position -> column (null: identity)
    const int32_t *pos_slot;   // plan: position -> partial slot of its positive's item side
    float *part_row, *part_bias;
    const int2 *pairs;         // prepared (user, item) per pair: [(1 + n) * cols], processing order
    int32_t *stamp;            // prepare: per-row serial of the last stamping prepare (null: no stamps)
    int32_t serial;
    int32_t *umark;            // prepare (lazy dense pass): umark[user] = umark_step for every pair's user
    int32_t umark_step;
    // claimed list slots (rg_mf_work_t claim_num_users): the prepare claims them in row_count and
    // stores them in the ids' bits 27-30; the pair pass reads them instead of claiming
    int32_t claimed;
    // pipelined step (mf_pipe_kernel): the prepare appends every user it claims a first slot of
    // (the users this step's pair pass reads) to hot_out, its length in *nhot_out
    int32_t *hot_out, *nhot_out;
};

// Prepared ids carry ownership flags in bit 31 when the prepare pass stamped rows:
// the first pair (any order) to stamp a row with this step's serial owns it, and
// the hot-row apply (mf_hot_kernel) updates each touched row through its owner only.
constexpr int32_t kOwnerBit = (int32_t)0x80000000;
constexpr int32_t kIdMask = 0x7fffffff;
// claimed records: slot min(slot, kCap) of the row side in bits 27-30 of its id
constexpr int kSlotShift = 27;
constexpr int32_t kClaimIdMask = (1 << kSlotShift) - 1;

// Diagnostic build only (RG_DIAG_STAMPS, librg_hip_diag.so; scripts/mf_pairs_stamps.py):
// per-wave s_memrealtime stamps at the pair pass's phase boundaries, each after a full
// vmcnt drain so it marks when that phase's data had landed.  The product library has
// no stamp code.  g_diag_stamps / g_diag_flags are __device__ globals of rg_mf.hip (defined
// there before this header is included); rg_mf_alt.hip includes this header with
// RG_DIAG_STAMPS undefined, so its kernels carry no stamps.
#ifdef RG_DIAG_STAMPS
#define RG_DIAG_FLAG(b) ((g_diag_flags >> (b)) & 1)
#else
#define RG_DIAG_FLAG(b) 0
#endif
#ifdef RG_DIAG_STAMPS
#define RG_STAMP(k)                                                                                   \
    do {                                                                                              \
        if (g_diag_stamps) {                                                                          \
            unsigned long long t_;                                                                    \
            asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
            if ((threadIdx.x & 63) == 0) g_diag_stamps[(blk * (kPairBlock / 64) + (threadIdx.x >> 6)) * 8 + (k)] = t_; \
        }                                                                                             \
    } while (0)
#else
#define RG_STAMP(k) \
    do {            \
    } while (0)
#endif

// rg_mf_prepare: record s of the prepared pairs (rg_common.h pair_stride): [q] for
// q = 0 (positive) and q = 1 + k (negative k), [n + 1] the positive's plan slot; one
// thread per entry, column-major so the record is written contiguously.
// With stamps, every row a pair touches (valid or not: extra rows are harmless, a
// missed one would not be) is stamped with the serial, and the first stamper owns it.
// Returns the user this entry claimed a FIRST list slot of (the users the prepared step's pair pass
// reads, for a hot list), else -1.
__device__ __forceinline__ int prepare_body(const PairsArgs &a, int2 *__restrict__ out, int64_t idx) {
    const int NP = 1 + a.n_neg, E = NP + 1;              // entries written per column
    const int64_t total = (int64_t)E * a.cols;
    if (idx >= total) return -1;
    const int64_t s = idx / E;
    const int q = (int)(idx - s * E);
    int2 *rec = out + s * pair_stride(a.n_neg);
    if (q == NP) {                                       // the plan slot of the positive
        rec[q] = make_int2(a.pos_slot != nullptr && s < a.n_pos ? a.pos_slot[s] : -1, 0);
        return -1;
    }
    const int64_t col = a.perm ? (int64_t)a.perm[s] : s;
    int2 r;
    if (q == 0) {
        r = (s < a.n_pos) ? make_int2((int)a.pos_user[col], (int)a.pos_item[col]) : make_int2(0, 0);
    } else {
        const int64_t j = (q - 1) * a.global_cols + a.col_offset + col;
        const uint2 w = a.words[j];
        r = a.pool[choice_index(w.x, w.y, a.pool_len)];
    }
    if (a.umark != nullptr) a.umark[r.x] = a.umark_step;   // plain store: every writer stores the same value
    int hot = -1;
    if (a.claimed) {
        // the list slots the pair pass would claim (pairs_body's validity): the positive if the
        // position has one, a negative if its column pairs with a positive or the loss is
        // pointwise; the planned positives' item side is reduced in LDS instead
        const bool pairwise = a.loss == RG_LOSS_BPR || a.loss == RG_LOSS_HINGE;
        const bool v = q == 0 ? s < a.n_pos : (a.loss != RG_LOSS_POINTWISE_POS && (s < a.n_pos || !pairwise));
        if (v) {
            const int su = atomicAdd(a.row_count + r.x, 1);
            if (su == 0) hot = r.x;
            const bool item_side = !(q == 0 && a.pos_slot != nullptr);
            const int si = item_side ? atomicAdd(a.row_count + a.num_users + r.y, 1) : 0;
            r.x |= (su < kCap ? su : kCap) << kSlotShift;
            r.y |= (si < kCap ? si : kCap) << kSlotShift;
        }
    }
    if (a.stamp != nullptr) {
        const int32_t ou = atomicExch(a.stamp + r.x, a.serial);
        const int32_t oi = atomicExch(a.stamp + a.num_users + r.y, a.serial);
        if (ou != a.serial) r.x |= kOwnerBit;
        if (oi != a.serial) r.y |= kOwnerBit;
    }
    rec[q] = r;
    return hot;
}

// append each lane's `user` (>= 0) to a.hot_out: one atomic per wave (a ballot and a prefix count),
// not one per user -- tens of thousands of returning atomics on ONE counter serialise; every lane of
// the wave calls it
__device__ __forceinline__ void hot_append(const PairsArgs &a, int user) {
    const unsigned long long m = __ballot(user >= 0);
    if (m == 0) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int leader = __ffsll((unsigned long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(a.nhot_out, __popcll(m));
    base = __shfl(base, leader);
    if (user >= 0) a.hot_out[base + __popcll(m & ((1ull << lane) - 1ull))] = user;
}

// one prepared entry (every thread of the workgroup calls it: the hot-list append is per wave)
__device__ __forceinline__ void prepare_one(const PairsArgs &a, int2 *__restrict__ out, int64_t idx) {
    const int hot = prepare_body(a, out, idx);
    if (a.hot_out != nullptr) hot_append(a, hot);
}


__host__ __device__ inline int64_t prepare_threads(int64_t cols, int n_neg) { return (int64_t)(n_neg + 3) * cols; }

// atomically add a row-vector contribution (overflow path, rare; fixed point, rg_common.h)
template <class L>
__device__ __forceinline__ void overflow_add(long long *__restrict__ hot, int64_t row, int D, int sub, float dz,
                                             const float (&o)[L::EPL]) {
#pragma unroll
    for (int e = 0; e < L::EPL; ++e) {
        const int c = L::elem(sub, e);
        if (L::VEC || c < D) fix_add(hot + row * (int64_t)D + c, dz * o[e]);
    }
}

// select x[q] for a runtime q without dynamic register indexing (no scratch)
template <int N, class T>
__device__ __forceinline__ T pick(const T (&x)[N], int q) {
    T r = x[0];
#pragma unroll
    for (int k = 1; k < N; ++k) r = (q == k) ? x[k] : r;
    return r;
}

constexpr int kLdsFloats = 5 * kPairBlock;   // >= units per block * (dim + 1) for every layout (1280 at 256 threads)

// One unit = one batch column: pair q = 0 is the positive, q = 1..n the
// negatives k*global_cols + col.  Every gather uses an always-valid index and is
// issued unconditionally (results of invalid pairs are masked afterwards), so a
// wave has all of its rows in flight at once.  The gathered rows die after their
// dot product except the positive's user row, which feeds the planned item-side
// partial sums; the rare list-overflow path re-gathers.
//
// One lane per pair: the dot products are reduced across the unit, so all LPU lanes hold
// all of them; what follows a dot product is per pair, not per element, and lane
// q % LPU alone does it for pair q (in rounds of LPU pairs where 1 + n > LPU) -- its two
// bias gathers, sigmoid((dot + b) + c), the transcendental part of its loss term (the BPR
// sigmoid, the hinge margin, the pointwise log and division) and its dz.  The positive's
// score and each negative's term are broadcast back by shuffles with constant lanes, and
// every lane forms the unit's sums (la, lb, the positive's dL/dp) from them, k = 1..n
// left to right: each value comes from the instruction sequence it always came from, on
// the same operands (same bits); a wave runs ceil((1 + n) / LPU) sigmoid chains per phase
// instead of 1 + n.  Nothing indexes a register array by a lane-dependent pair: own ids
// come from the record, own dots by a select over constant indices, dz goes through LDS.
//
// List tasks: t = 2q + side (side 0: user row of pair q, 1: its item row), spread
// over the unit's lanes as t = sub + j*LPU.  With a plan, the positives are
// processed in item-sorted order and the positive's item side (t = 1, the Zipf-hot
// rows) is instead reduced per block in LDS into one partial row per
// (item, block): plain stores, no atomics, fixed order.
template <class L, int PHASE, int NMAX, bool SC1 = false>
__device__ __forceinline__ void pairs_body(const PairsArgs &a, const int64_t blk) {
    constexpr int LPU = L::LPU, EPL = L::EPL, NP = NMAX + 1;
    constexpr int UPB = kPairBlock / LPU;                  // units per block
    constexpr int TPL = (2 * NP + LPU - 1) / LPU;      // list tasks per lane
    constexpr int R = (NP + LPU - 1) / LPU;            // rounds of own pairs per lane
    constexpr bool kBackward = (PHASE == kFused) || (PHASE == kAdaptBwd);
    constexpr bool kScoresFromBuf = (PHASE == kAdaptBwd) || (PHASE == kAdaptLoss);
    __shared__ float red[2][kPairBlock / kWave];
    __shared__ float lrow[UPB * (LPU * EPL + 1)];   // a planned partial row (D <= LPU * EPL) per unit
    __shared__ int lslot[UPB];
    __shared__ float ldz[kBackward ? UPB * NP : 1];
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int ubase = lane & ~(LPU - 1);
    const int ublk = threadIdx.x / LPU;               // unit within the block
    const int64_t s = blk * UPB + ublk;                 // processing position
    const bool active = s < a.cols;
    const bool plan = a.pos_slot != nullptr;
    const bool has_pos = active && s < a.n_pos;        // a plan puts the positives first
    const int D = a.dim;
    const int n = a.n_neg;
    const bool pairwise = (a.loss == RG_LOSS_BPR) || (a.loss == RG_LOSS_HINGE);
    const bool negs = a.loss != RG_LOSS_POINTWISE_POS;   // no negative pool: positives only
    RG_STAMP(0);

    // ---- ids of every pair, prepared in processing order (one coalesced round trip) ----
    int uid[NP], iid[NP];
    bool valid[NP];
    valid[0] = has_pos;
#pragma unroll
    for (int k = 0; k < NMAX; ++k)   // flat negatives that pair with no positive only matter to pointwise / adaptive
        valid[k + 1] = !kScoresFromBuf && negs && active && k < n && (has_pos || !pairwise);
    // the column's record: every pair's ids and the positive's plan slot in one line
    // (the slot entry is loaded with the ids, unconditionally: issued after them it became a
    // second round trip that queued behind the gathers of the waves already past this point)
    const int2 *rec = a.pairs + (active ? s : 0) * (int64_t)pair_stride(n);
    const int2 slot_entry = rec[n + 1];
    const bool claimed = kBackward && a.claimed;
    const int32_t idm = a.claimed ? kClaimIdMask : kIdMask;   // drop the ownership flags / slots
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int2 pr = rec[(valid[q] || q == 0) ? q : 0];
        uid[q] = pr.x & idm;
        iid[q] = pr.y & idm;
    }
    const int myslot = (kBackward && plan && has_pos) ? slot_entry.x : -1;
    // each list task's own pair, loaded from the record beside the ids: indexing uid[] /
    // iid[] / valid[] by the lane-dependent pair index made the compiler keep them as a
    // per-thread LDS array (18 KB per workgroup), which slowed this whole phase ~10x
    int tu[TPL], ti[TPL];
    bool tv[TPL];
    int slot[TPL];
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
        const int t = sub + j * LPU, q = t >> 1;
        const bool inb = t < 2 * NP && q <= n;
        tv[j] = inb && (q == 0 ? has_pos : (!kScoresFromBuf && negs && active && (has_pos || !pairwise)));
        const int2 e = rec[inb ? q : 0];
        tu[j] = e.x & idm;
        ti[j] = e.y & idm;
        slot[j] = claimed ? (int)(((uint32_t)((t & 1) ? e.y : e.x) >> kSlotShift) & 15u) : 0;
    }
    // each lane's own pairs (q = sub + r*LPU), from the record for the same reason: their
    // biases are one gather per table and round, issued with the row gathers
    int mu[R], mi[R];
    bool vm[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int q = sub + r * LPU;
        vm[r] = q < NP && q <= n && (q == 0 ? has_pos : (!kScoresFromBuf && negs && active && (has_pos || !pairwise)));
        const int2 e = rec[vm[r] ? q : 0];
        mu[r] = e.x & idm;
        mi[r] = e.y & idm;
    }
    RG_STAMP(1);
    if (RG_DIAG_FLAG(3)) return;

    // ---- claim list slots early (their latency hides under the gathers) -------
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
        const int t = sub + j * LPU;
        if (kBackward && !claimed && t < 2 * NP && !(plan && t == 1)) {
            if (tv[j] && !RG_DIAG_FLAG(0)) {
                const int64_t row = (t & 1) ? a.num_users + ti[j] : (int64_t)tu[j];
                slot[j] = atomicAdd(a.row_count + row, 1);
            }
        }
    }

    // ---- gather rows, scores ---------------------------------------------------
    // pm[r]: the score of this lane's own pair q = sub + r*LPU; p0: the positive's, on every lane
    float pm[R], p0;
    float upos[EPL];      // the positive's user row (planned item-side partial sums)
    L::zero(upos);
    if (kScoresFromBuf) {
        p0 = has_pos ? a.scores[s] : 0.5f;
#pragma unroll
        for (int r = 0; r < R; ++r) pm[r] = p0;   // only pair 0 (lane sub 0) is used
        if (plan && kBackward) L::load(upos, a.user_w, uid[0], D, sub);
    } else {
        float ur[NP][EPL], ir[NP][EPL], ub[R], ib[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (SC1) {   // rows written by this launch's hot workgroups (mf_pipe_kernel)
                ub[r] = L::load1_sc1(a.user_b + mu[r]);
                ib[r] = L::load1_sc1(a.item_b + mi[r]);
            } else {
                ub[r] = a.user_b[mu[r]];
                ib[r] = a.item_b[mi[r]];
            }
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if constexpr (SC1) {
                L::load_sc1(ur[q], a.user_w, uid[q], D, sub);
                L::load_sc1(ir[q], a.item_w, iid[q], D, sub);
            } else {
                L::load(ur[q], a.user_w, uid[q], D, sub);
                L::load(ir[q], a.item_w, iid[q], D, sub);
            }
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) upos[e] = ur[0][e];
        float dot[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) dot[q] = row_dot<L>(ur[q], ir[q]);
        // the unit's lanes all hold every dot product: lane q % LPU alone adds pair q's biases
        // and takes its sigmoid (row_score's order: sigmoid((dot + b) + c))
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float d = dot[r * LPU];
#pragma unroll
            for (int c = 1; c < LPU && r * LPU + c < NP; ++c) d = (sub == c) ? dot[r * LPU + c] : d;
            pm[r] = sigmoidf_ref((d + ub[r]) + ib[r]);
        }
        p0 = __shfl(pm[0], ubase);
    }

    RG_STAMP(2);
    // ---- loss terms and dL/dp ---------------------------------------------------
    // Each lane does the transcendental part of its own pairs' terms; the unit's sums (la, lb,
    // dL/dp of the positive) are then taken on every lane from the broadcast terms, k = 1..n in
    // order.  Shuffles sit outside the lane-dependent conditions: every lane takes part.
    float la = 0.0f, lb = 0.0f;
    float dp0 = 0.0f;      // dL/dp of the positive (every lane)
    float dpm[R];          // dL/dp of the lane's own pairs
#pragma unroll
    for (int r = 0; r < R; ++r) dpm[r] = 0.0f;
    if (PHASE == kAdaptFwd) {
        if (sub == 0 && has_pos) a.scores[s] = p0;
        const int64_t col = a.perm ? (int64_t)a.perm[active ? s : 0] : s;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int q = sub + r * LPU;
            if (vm[r] && q >= 1) {
                const int64_t j = (int64_t)(q - 1) * a.global_cols + a.col_offset + col;
                const unsigned long long key = ((unsigned long long)__float_as_uint(pm[r]) << 32) |
                                               (unsigned long long)(0xFFFFFFFFu - (uint32_t)j);
                atomicMax(a.max_key, key);
            }
        }
    } else if (kScoresFromBuf) {  // adaptive hinge, positives only (max negative: mf_adapt_max_kernel)
        if (has_pos) {
            const unsigned long long key = *a.max_key;
            const float m = __uint_as_float((uint32_t)(key >> 32));
            const float x = (m - p0) + 1.0f;
            la = fmaxf(x, 0.0f);
            if (x >= 0.0f) {
                dp0 = -(1.0f / a.n_a);
                if (PHASE == kAdaptBwd && sub == 0) atomicAdd(a.active_count, 1);
            }
        }
        if (sub == 0) dpm[0] = dp0;
    } else if (a.loss == RG_LOSS_POINTWISE || a.loss == RG_LOSS_POINTWISE_POS) {
        // the positive: -max(log p, -100) and ((p - 1) / max((1 - p) p, 1e-12)) / n_a;
        // a negative:   -max(log(1 - p), -100) and (p / max((1 - p) p, 1e-12)) / n_b
        float tm[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool pos = sub + r * LPU == 0;
            const float pq = pm[r];
            tm[r] = -fmaxf(logf(pos ? pq : 1.0f - pq), -100.0f);
            const float d = ((pos ? pq - 1.0f : pq) / fmaxf((1.0f - pq) * pq, 1e-12f)) / (pos ? a.n_a : a.n_b);
            if (vm[r]) dpm[r] = d;
        }
        if (has_pos) la = tm[0];   // lane sub 0's is the positive's; the loss sum reads that lane only
#pragma unroll
        for (int k = 1; k < NP; ++k) {
            const float t = __shfl(tm[k / LPU], ubase + k % LPU);
            if (valid[k]) lb += t;
        }
    } else {  // bpr / hinge on the neg.view(n, B) pairing
        const float g = 1.0f / a.n_a;
        const bool bpr = a.loss == RG_LOSS_BPR;
        float om[R];   // own negative: sigmoid(p0 - p) (bpr), (p - p0) + 1 (hinge)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (bpr) om[r] = sigmoidf_ref(p0 - pm[r]);
            else om[r] = (pm[r] - p0) + 1.0f;
        }
#pragma unroll
        for (int k = 1; k < NP; ++k) {
            const float o = __shfl(om[k / LPU], ubase + k % LPU);
            if (has_pos && valid[k]) {
                float dk;
                if (bpr) {
                    const float sg = o;
                    la += 1.0f - sg;
                    const float dx = (-g) * (1.0f - sg) * sg;
                    dp0 += dx;
                    dk = -dx;
                } else {
                    const float x = o;
                    la += fmaxf(x, 0.0f);
                    const float dx = x >= 0.0f ? g : 0.0f;
                    dp0 -= dx;
                    dk = dx;
                }
                if (sub == k % LPU) dpm[k / LPU] = dk;
            }
        }
        if (sub == 0) dpm[0] = dp0;
    }

    // ---- dz, list entries, planned partials ----------------------------------------
    if (kBackward) {
        // each lane's own pairs; the list tasks (and the planned partial, pair 0) index dz by
        // another pair: stage it through LDS.  A unit's lanes share one wave and a wave's LDS
        // operations complete in order, so only the compiler must keep the reads after the
        // writes (no workgroup barrier)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int q = sub + r * LPU;
            if (q < NP) ldz[ublk * NP + q] = (dpm[r] * (1.0f - pm[r])) * pm[r];
        }
        static_assert(kWave % LPU == 0, "a unit's lanes must share a wave");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RG_STAMP(3);
        bool ovf = false;
#pragma unroll
        for (int j = 0; j < TPL; ++j) {
            const int t = sub + j * LPU;
            if (t < 2 * NP && !(plan && t == 1)) {
                const int q = t >> 1;
                if (tv[j]) {
                    const int u = tu[j], i = ti[j];
                    const int64_t row = (t & 1) ? a.num_users + i : (int64_t)u;
                    if (slot[j] < kCap) {
                        if (!RG_DIAG_FLAG(1)) store_entry(a.row_list + row * kCap + slot[j], (t & 1) ? u : i, ldz[ublk * NP + q]);
                    }
                    else
                        ovf = true;
                }
            }
        }
        if (__any(ovf)) {   // wave-uniform: rows touched more than kCap times this step (re-gather)
#pragma unroll
            for (int t = 0; t < 2 * NP; ++t) {
                const int sl = __shfl(slot[t / LPU], ubase + (t % LPU));
                const int q = t >> 1;
                if (valid[q] && sl >= kCap && !(plan && t == 1)) {
                    const float dzq = ldz[ublk * NP + q];
                    float o[EPL];
                    if (t & 1) {
                        const int64_t row = a.num_users + iid[q];
                        if constexpr (SC1) L::load_sc1(o, a.user_w, uid[q], D, sub);
                        else L::load(o, a.user_w, uid[q], D, sub);
                        overflow_add<L>(a.hot_grad, row, D, sub, dzq, o);
                        if (sub == 0) fix_add(a.hot_bias_grad + row, dzq);
                    } else {
                        if constexpr (SC1) L::load_sc1(o, a.item_w, iid[q], D, sub);
                        else L::load(o, a.item_w, iid[q], D, sub);
                        overflow_add<L>(a.hot_grad, uid[q], D, sub, dzq, o);
                        if (sub == 0) fix_add(a.hot_bias_grad + uid[q], dzq);
                    }
                }
            }
        }
        RG_STAMP(4);
        if (plan) {
            // block-level segmented sum of the positives' item-side rows, sorted by item
            const int stride = D + 1;
            const float dz0 = ldz[ublk * NP];
            if (has_pos) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int c = L::elem(sub, e);
                    if (L::VEC || c < D) lrow[ublk * stride + c] = dz0 * upos[e];
                }
                if (sub == 0) lrow[ublk * stride + D] = dz0;
            }
            if (sub == 0) lslot[ublk] = myslot;
            lds_barrier();
            if (has_pos && (ublk == 0 || lslot[ublk - 1] != myslot)) {   // segment head
                float acc[EPL];
                float accb = 0.0f;
                L::zero(acc);
                for (int v = ublk; v < UPB && lslot[v] == myslot; ++v) {
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        const int c = L::elem(sub, e);
                        if (L::VEC || c < D) acc[e] += lrow[v * stride + c];
                    }
                    accb += lrow[v * stride + D];
                }
                if (!RG_DIAG_FLAG(2)) {
                    L::store(a.part_row, myslot, D, sub, acc);
                    if (sub == 0) a.part_bias[myslot] = accb;
                }
            }
        }
    }

    // ---- deterministic loss partials: wave DPP sum -> block -> partials[block] ----
    if (PHASE != kAdaptFwd) {
        float va = (sub == 0) ? la : 0.0f;
        float vb = (sub == 0) ? lb : 0.0f;
        va = group_sum<kWave>(va);
        vb = group_sum<kWave>(vb);
        const int w = threadIdx.x >> 6;
        if (lane == 0) { red[0][w] = va; red[1][w] = vb; }
        lds_barrier();
        if (threadIdx.x == 0) {
            float sa = 0.0f, sb = 0.0f;
#pragma unroll
            for (int i = 0; i < kPairBlock / kWave; ++i) { sa += red[0][i]; sb += red[1][i]; }
            a.partials[2 * blk] = sa;
            a.partials[2 * blk + 1] = sb;
        }
    }
    RG_STAMP(5);
}

// ---------------------------------------------------------------------------- apply
struct ApplyArgs {
    const float *w_in[2], *b_in[2];
    float *w_out[2], *b_out[2];
    float *w_m[2], *w_v[2], *b_m[2], *b_v[2];
    int64_t num_users, num_items;
    int32_t dim;
    int64_t row_begin, row_end;   // unified rows: users [0, U), items [U, U + I)
    int32_t *row_count;
    const int2 *row_list;
    long long *hot_grad, *hot_bias_grad;     // int64 fixed point
    const int32_t *item_slot_off; // plan: item i's partial slots [off[i], off[i+1])
    const float *part_row, *part_bias;
    rg_opt_t opt;
    const float *partials;
    int64_t n_partials;
    double inv_a, inv_b;
    float *loss_out;
    float *grad;                  // flat [(re-rb)*D | (re-rb) | loss] (kGradOnly / kApplyDense)
    // NCF: list entries {example slot, 1.0f} point at per-example gradient rows
    // contrib[slot * contrib_stride + table * D ..] instead of partner rows (then no biases)
    const float *contrib;
    int64_t contrib_stride;
    bool has_bias;
    bool keep_count;              // NeuMF: the MF tables read the lists first, the MLP tables reset them
    // rank-major flat gradient of the replicated data-parallel step (rg_mf_grads_sharded /
    // rg_mf_apply_shard; shard_users == 0: the plain [(re-rb)*D | (re-rb) | loss] layout):
    // chunk s (chunk floats) = [user rows s*Us .. (s+1)*Us | item rows s*Is .. | their
    // biases (Us + Is) | loss], D floats per row
    int64_t shard_users, shard_items, chunk;
    int32_t world, rank;
    // owner-sharded step's item exchange (rg_mf_grads_item_shard / rg_mf_apply_item_shard): the
    // rank-major chunks hold item rows only (shard_users = 0): chunk s = [item rows s*Is .. | their
    // biases | loss]
    int32_t item_shard;
    // lazy dense pass: a USER row with a zero data gradient that the next step
    // does not read is skipped; its cold updates (weight decay + optimizer state only) are
    // applied, in order and with each step's constants, when the row is next processed
    int32_t *last_rel;            // [num_users] last step applied to the row, minus lazy_base
    const int32_t *umark;         // [num_users] step whose pair pass reads the row (prepare marks)
    const float2 *step_consts;    // [s] Adam (step_size, bias_correction2_sqrt) of absolute step s
    int64_t lazy_base;            // absolute step of last_rel == 0
    int32_t lazy_t;               // this step (absolute)
    int32_t lazy_full;            // process every user row (no next step known)
    unsigned long long *lazy_rows;   // optional: count of user rows processed (diagnostic steps)
    int32_t lazy_dbg;             // timing experiments only (RG_LAZY_DBG; wrong results): bit 0 no catch-up,
                                  // 1 every user row processed, 2 no constants window, 3 no odd-lag reload
    int32_t lazy_cap;             // > 0: a row that has missed this many steps is processed anyway
    // apply_row<..., GUARD>: a row with guard[r] > 0 is left alone (another launch updates it); the
    // guard is loaded beside the row's other loads, so it costs no round trip of its own
    const int32_t *guard;
};

// sort the first ne of kCap list entries ascending by (other, dz bits) -- an 8-input
// sorting network (19 compare-exchanges, register only); entries past ne key as +inf
__device__ __forceinline__ uint64_t ent_key(int2 e, bool valid) {
    return valid ? ((uint64_t)(uint32_t)e.x << 32) | (uint64_t)(uint32_t)e.y : ~0ull;
}
__device__ __forceinline__ void sort_entries(int2 (&ent)[8], int ne) {
    uint64_t k[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) k[e] = ent_key(ent[e], e < ne);
#define RG_CX(i, j)                                     \
    {                                                   \
        const uint64_t lo = k[i] < k[j] ? k[i] : k[j];  \
        const uint64_t hi = k[i] < k[j] ? k[j] : k[i];  \
        k[i] = lo;                                      \
        k[j] = hi;                                      \
    }
    RG_CX(0, 2) RG_CX(1, 3) RG_CX(4, 6) RG_CX(5, 7)
    RG_CX(0, 4) RG_CX(1, 5) RG_CX(2, 6) RG_CX(3, 7)
    RG_CX(0, 1) RG_CX(2, 3) RG_CX(4, 5) RG_CX(6, 7)
    RG_CX(2, 4) RG_CX(3, 5)
    RG_CX(1, 4) RG_CX(3, 6)
    RG_CX(1, 2) RG_CX(3, 4) RG_CX(5, 6)
#undef RG_CX
#pragma unroll
    for (int e = 0; e < 8; ++e) ent[e] = make_int2((int)(uint32_t)(k[e] >> 32), (int)(uint32_t)k[e]);
}

// location of unified row r's gradient in the flat buffer: *row_base + k*D, bias at *bias
__device__ __forceinline__ void grad_loc(const ApplyArgs &a, int t, int64_t lr_, int64_t gk, int64_t nr,
                                         const float *&row_base, int64_t &k, int64_t &bias) {
    if (a.shard_users > 0 || a.item_shard) {
        const int64_t s = t ? lr_ / a.shard_items : lr_ / a.shard_users;
        k = t ? a.shard_users + lr_ % a.shard_items : lr_ % a.shard_users;
        row_base = a.grad + s * a.chunk;
        bias = s * a.chunk + (a.shard_users + a.shard_items) * (int64_t)a.dim + k;
    } else {
        row_base = a.grad;
        k = gk;
        bias = nr * (int64_t)a.dim + gk;
    }
}

// mf_apply modes: pull the gradient from the lists and update (single GPU);
// pull into the flat dense gradient (before an all-reduce);
// update from the (all-reduced) flat gradient.
enum ApplyMode : int { kApplyPull = 0, kGradOnly = 1, kApplyDense = 2, kApplyCold = 3 /* arg checks only */ };

// loss of the step from the pair kernel's per-block partials (one wave, fixed order)
__device__ __forceinline__ float finalize_loss(const float *__restrict__ partials, int64_t np_, double inv_a,
                                               double inv_b, int lane) {
    // eight partials per lane in flight per round (the owner step's backward leaves ~3k): one
    // round trip per 512 partials instead of per 64; fixed order, so the sum is deterministic
    constexpr int kU = 8;
    double sa = 0.0, sb = 0.0;
    for (int64_t i0 = lane; i0 < np_; i0 += kU * kWave) {
        float2 v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = i0 + (int64_t)u * kWave;
            v[u] = i < np_ ? reinterpret_cast<const float2 *>(partials)[i] : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            sa += (double)v[u].x;
            sb += (double)v[u].y;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sa += __shfl_xor(sa, off);
        sb += __shfl_xor(sb, off);
    }
    return (float)(sa * inv_a + sb * inv_b);
}

// The same loss over a whole workgroup (every thread of it calls this; every thread gets
// the value): a data-parallel step's backward leaves thousands of partials, which one wave
// reads in ~6 dependent rounds -- a floor under the short launch that finalizes them.
// Fixed partition and combine order: deterministic.
template <int NT>
__device__ __forceinline__ float finalize_loss_wg(const float *__restrict__ partials, int64_t np_, double inv_a,
                                                  double inv_b) {
    constexpr int kU = 8, NW = NT / kWave;
    __shared__ double red[2][NW];
    __shared__ float out;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    double sa = 0.0, sb = 0.0;
    for (int64_t i0 = tid; i0 < np_; i0 += (int64_t)kU * NT) {
        float2 v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = i0 + (int64_t)u * NT;
            v[u] = i < np_ ? reinterpret_cast<const float2 *>(partials)[i] : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            sa += (double)v[u].x;
            sb += (double)v[u].y;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sa += __shfl_xor(sa, off);
        sb += __shfl_xor(sb, off);
    }
    if (lane == 0) { red[0][w] = sa; red[1][w] = sb; }
    __syncthreads();
    if (tid == 0) {
        double ta = 0.0, tb = 0.0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { ta += red[0][k]; tb += red[1][k]; }
        out = (float)(ta * inv_a + tb * inv_b);
    }
    __syncthreads();
    return out;
}

// Gradient + optimizer update of unified row r (users [0, U), items [U, U + I)).
// COLD: a row no pair of the step touches -- its data gradient is exactly zero
// (only the coupled weight decay acts), so nothing of the step's scratch is read.
struct LazyRow {
    int cnt;          // list count (data gradient this step)
    int32_t mk, lsr;  // prepare mark, last step applied (relative)
    bool active;      // false: a lane group past the end of the rows
};

// wave-uniform maximum (every lane ends with the same value)
__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o));
    return __builtin_amdgcn_readfirstlane(x);
}

// this lane's Adam constants of window step `lane` (absolute step s0 + lane, lane < n)
__device__ __forceinline__ float2 window_const(const ApplyArgs &a, int64_t s0, int n) {
    const int lane = threadIdx.x & (kWave - 1);
    return (a.opt.kind == RG_OPT_ADAM && lane < n) ? a.step_consts[s0 + lane] : make_float2(0.0f, 0.0f);
}

// The cold updates a row missed (zero data gradient: the coupled weight decay and the
// optimizer state only), in step order, each with its own Adam constants -- the exact
// operation sequence the eager dense pass applies to a row no pair touches (opt_update with
// gdata = 0), so the row ends bit-identical.  The loop runs over the wave's window of the
// `wmax` steps before `upto`, so the step is wave-uniform: its constants come from lane k of
// `cl` (loaded beside the row, 64 steps per load) by readlane, and each row updates only at
// the last `mylag` steps of the window.
template <class L>
__device__ __forceinline__ void catch_up(const ApplyArgs &a, float2 cl, int wmax, int mylag, int64_t upto, int sub,
                                         float (&p)[L::EPL], float (&m)[L::EPL], float (&v)[L::EPL], float &pb,
                                         float &mb, float &vb) {
    if (wmax <= 0) return;
    rg_opt_t o = a.opt;
    const bool adam = o.kind == RG_OPT_ADAM;
    const int first = wmax - mylag;
    for (int c0 = 0; c0 < wmax; c0 += kWave) {
        if (c0 > 0) cl = window_const(a, upto - wmax + c0, wmax - c0);
        const int n = wmax - c0 < kWave ? wmax - c0 : kWave;
        for (int k = 0; k < n; ++k) {
            if (adam) {
                o.step_size = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cl.x), k));
                o.bias_correction2_sqrt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cl.y), k));
            }
            if (c0 + k < first) continue;
#pragma unroll
            for (int q = 0; q < L::EPL; ++q) p[q] = opt_update(o, p[q], 0.0f, m[q], v[q]);
            if (sub == 0 && a.has_bias) pb = opt_update(o, pb, 0.0f, mb, vb);
        }
    }
}

// Ascending sort of the 8 list entries held one per lane (lanes sub 0..7 of each LPU-lane row
// group; sub >= 8 hold +inf keys and sort among themselves): a bitonic network over lane
// XOR partners, 6 compare-exchange stages of 64-bit keys.  The result (entry e on lane e) is
// the order sort_entries gives, so the row sums its contributions in the same order.
template <int LPU>
__device__ __forceinline__ uint64_t lane_sort8(uint64_t key, int sub) {
#pragma unroll
    for (int k = 2; k <= 8; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const uint64_t o = __shfl_xor(key, j, LPU);
            const bool up = (sub & k) == 0;
            const bool lower = (sub & j) == 0;
            const uint64_t lo = key < o ? key : o, hi = key < o ? o : key;
            key = (lower == up) ? lo : hi;
        }
    }
    return key;
}

// Pull-and-update of unified row r (the single-GPU dense pass, MODE kApplyPull) with a small
// register footprint: each row's 8 list entries are held one per lane and sorted across the
// lanes (apply_row holds all 8 in every lane and sorts them in registers).  Split in two so a
// wave can hold the NEXT row group's loads in flight while it finishes this one
// (mf_dense_kernel): lean_load issues every load a row needs that does not depend on another
// load (p, m, v, biases, count, its list entries, the item's partial-slot range); lean_finish
// pulls the partner rows (and planned partials) those name, updates and stores.  The
// summation order is apply_row's (sorted entries, fma chain; overflowed rows in fixed point;
// planned partials after), so the result is bit-identical to it.
template <class L>
struct LeanRow {
    float p[L::EPL], m[L::EPL], v[L::EPL];
    float pb, mb, vb;
    int c;
    int2 ent;
    int s0, s1;
};

template <class L>
__device__ __forceinline__ void lean_load(const ApplyArgs &a, const int64_t r, const int sub, const bool valid,
                                          LeanRow<L> &x) {
    const int t = r < a.num_users ? 0 : 1;
    const int64_t lr_ = t ? r - a.num_users : r;
    const bool adam = a.opt.kind == RG_OPT_ADAM;
    const bool has_v = a.opt.kind != RG_OPT_SGD;
    const int D = a.dim;
    L::zero(x.p); L::zero(x.m); L::zero(x.v);
    x.pb = x.mb = x.vb = 0.0f;
    x.c = 0;
    x.ent = make_int2(0, 0);
    x.s0 = x.s1 = 0;
    if (!valid) return;
    L::load(x.p, a.w_in[t], lr_, D, sub);
    if (adam) L::load(x.m, a.w_m[t], lr_, D, sub);
    if (has_v) L::load(x.v, a.w_v[t], lr_, D, sub);
    if (sub == 0 && a.has_bias) {
        x.pb = a.b_in[t][lr_];
        if (adam) x.mb = a.b_m[t][lr_];
        if (has_v) x.vb = a.b_v[t][lr_];
    }
    x.c = a.row_count[r];
    if (sub < kCap) x.ent = a.row_list[r * kCap + sub];
    if (t == 1 && a.item_slot_off != nullptr) { x.s0 = a.item_slot_off[lr_]; x.s1 = a.item_slot_off[lr_ + 1]; }
}

template <class L, bool WT = false>
__device__ __forceinline__ void lean_finish(const ApplyArgs &a, const int64_t r, const int sub, const bool valid,
                                            LeanRow<L> &x) {
    constexpr int EPL = L::EPL, LPU = L::LPU, PG = kLeanPullGroup;
    static_assert(LPU >= kCap, "one list entry per lane");
    const int D = a.dim;
    const int t = r < a.num_users ? 0 : 1;
    const int64_t lr_ = t ? r - a.num_users : r;
    const bool adam = a.opt.kind == RG_OPT_ADAM;
    const bool has_v = a.opt.kind != RG_OPT_SGD;
    const int c = x.c;
    float g[EPL];
    float gb = 0.0f;
    L::zero(g);
    const int lane = threadIdx.x & (kWave - 1);
    const int rowbase = lane & ~(LPU - 1);
    if (__any(c > 0)) {
        const int ne = c < kCap ? c : kCap;
        const uint64_t key = lane_sort8<LPU>(ent_key(x.ent, sub < ne), sub);
        const float *other = a.contrib ? a.contrib + t * D : a.w_in[t ^ 1];
        const int64_t ostride = a.contrib ? a.contrib_stride : (int64_t)D;
        const bool fixp = c > kCap;   // an overflowed row sums list and surplus in fixed point
        long long gf[EPL];
        long long gbf = 0;
#pragma unroll
        for (int q = 0; q < EPL; ++q) gf[q] = 0;
#pragma unroll
        for (int h = 0; h < kCap; h += PG) {
            if (h > 0 && !__any(ne > h)) break;
            uint64_t k[PG];
            float o[PG][EPL];
#pragma unroll
            for (int e = 0; e < PG; ++e) {
                k[e] = __shfl(key, rowbase + h + e);
                if (h + e < ne) L::load_strided(o[e], other, (int)(uint32_t)(k[e] >> 32), ostride, D, sub);
                else L::zero(o[e]);
            }
#pragma unroll
            for (int e = 0; e < PG; ++e) {
                if (h + e < ne) {
                    const float dz = __uint_as_float((uint32_t)k[e]);
                    if (fixp) {
#pragma unroll
                        for (int q = 0; q < EPL; ++q) gf[q] += to_fix(dz * o[e][q]);
                        gbf += to_fix(dz);
                    } else {
#pragma unroll
                        for (int q = 0; q < EPL; ++q) g[q] = fmaf(dz, o[e][q], g[q]);
                        gb += dz;
                    }
                }
            }
        }
        if (fixp) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int cc = L::elem(sub, e);
                if (L::VEC || cc < D) {
                    long long *hp = a.hot_grad + r * (int64_t)D + cc;
                    gf[e] += *hp;
                    *hp = 0;
                }
            }
#pragma unroll
            for (int q = 0; q < EPL; ++q) g[q] = from_fix(gf[q]);
            if (sub == 0 && a.has_bias) {
                gbf += a.hot_bias_grad[r];
                a.hot_bias_grad[r] = 0;
            }
            gb = from_fix(gbf);
        }
        if (valid && sub == 0 && c > 0 && !a.keep_count) a.row_count[r] = 0;
    }
    const int s0 = x.s0, s1 = x.s1;
    if (__any(s1 > s0)) {   // planned positive partials of this item, in slot order
        for (int sl = s0; __any(sl < s1); sl += PG) {
            float h[PG][EPL];
            float hb[PG];
#pragma unroll
            for (int u = 0; u < PG; ++u) {
                const bool in = sl + u < s1;
                if (in) {
                    L::load(h[u], a.part_row, sl + u, D, sub);
                    hb[u] = a.has_bias ? a.part_bias[sl + u] : 0.0f;
                } else {
                    L::zero(h[u]);
                    hb[u] = 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < PG; ++u) {
                if (sl + u < s1) {
#pragma unroll
                    for (int q = 0; q < EPL; ++q) g[q] += h[u][q];
                    gb += hb[u];
                }
            }
        }
    }
    if (!valid) return;
#pragma unroll
    for (int q = 0; q < EPL; ++q) x.p[q] = opt_update(a.opt, x.p[q], g[q], x.m[q], x.v[q]);
    // WT: the row and bias write-through (another workgroup of the launch reads them:
    // mf_pipe_kernel's pair pass); the optimizer state is not read there
    if (WT) L::store_wt(a.w_out[t], lr_, D, sub, x.p);
    else L::store(a.w_out[t], lr_, D, sub, x.p);
    if (adam) L::store(a.w_m[t], lr_, D, sub, x.m);
    if (has_v) L::store(a.w_v[t], lr_, D, sub, x.v);
    if (sub == 0 && a.has_bias) {
        x.pb = opt_update(a.opt, x.pb, gb, x.mb, x.vb);
        if (WT) L::store1_wt(a.b_out[t] + lr_, x.pb);
        else a.b_out[t][lr_] = x.pb;
        if (adam) a.b_m[t][lr_] = x.mb;
        if (has_v) a.b_v[t][lr_] = x.vb;
    }
}

template <class L, int MODE, int NT, bool COLD, bool SPEC = false, bool LAZY = false, bool LSPEC = false,
          bool GUARD = false>
__device__ __forceinline__ void apply_row(const ApplyArgs &a, const int64_t r, const int sub,
                                          const LazyRow lzr = LazyRow{}) {
    constexpr int EPL = L::EPL;
    const int64_t rb = a.row_begin, nr = a.row_end - rb;
    const int D = a.dim;
    const int t = r < a.num_users ? 0 : 1;          // 0: user table, 1: item table
    const int64_t lr_ = t ? r - a.num_users : r;
    const int64_t gk = r - rb;                      // index in the flat gradient
    const bool adam = a.opt.kind == RG_OPT_ADAM;
    const bool has_v = a.opt.kind != RG_OPT_SGD;

    // lazy user row: processed iff it has a data gradient this step (list count), the next
    // step's pair pass reads it (prepare mark), or the pass is a full one; its current value
    // is in the set written at its last step -- w_in if an even number of steps was missed
    // since, else w_out (then the update is in place)
    const bool lz = LAZY && t == 0;
    int lag = 0;
    const int32_t lsr = lzr.lsr;
    // proc: this row is updated this step (false: a lazily skipped user row, which still runs
    // through to the wave's catch-up loop -- a wave-collective -- doing nothing)
    const int missed = lz ? (int)((int64_t)a.lazy_t - 1 - a.lazy_base - lsr) : 0;
    const bool proc = !lz || (lzr.active && (a.lazy_full || (a.lazy_dbg & 2) || lzr.cnt > 0 ||
                                             lzr.mk == a.lazy_t + 1 || (a.lazy_cap > 0 && missed >= a.lazy_cap)));
    const int cnt = proc ? lzr.cnt : 0;
    const float *src_w = a.w_in[t], *src_b = a.b_in[t];
    float p[EPL], m[EPL], v[EPL], g[EPL];
    float pb = 0.0f, mb = 0.0f, vb = 0.0f;
    L::zero(p); L::zero(m); L::zero(v);
    int2 lspec[LSPEC ? kCap : 1];
    if (lz) {
        // LSPEC: p (from the set a row processed last step holds it in), m, v and the list are
        // loaded with the decision words, in one round trip as the eager pass; a processed row
        // that missed an odd number of steps reloads p from the other set
        if (LSPEC && lzr.active) {
            L::load(p, a.w_in[0], lr_, D, sub);
            if (adam) L::load(m, a.w_m[0], lr_, D, sub);
            if (has_v) L::load(v, a.w_v[0], lr_, D, sub);
            if (sub == 0 && a.has_bias) {
                pb = a.b_in[0][lr_];
                if (adam) mb = a.b_m[0][lr_];
                if (has_v) vb = a.b_v[0][lr_];
            }
            const int4 *lst = reinterpret_cast<const int4 *>(a.row_list + r * kCap);
#pragma unroll
            for (int e = 0; e < kCap / 2; ++e) {
                const int4 q = lst[e];
                lspec[2 * e] = make_int2(q.x, q.y);
                lspec[2 * e + 1] = make_int2(q.z, q.w);
            }
        }
        lag = proc ? missed : 0;
        if (lag & 1) {
            src_w = a.w_out[t];
            src_b = a.b_out[t];
        }
    }
    // the wave's catch-up window and its constants (issued with the row's loads)
    const int wmax = LAZY ? wave_max(lag) : 0;
    const float2 wconst = (LAZY && wmax > 0 && !(a.lazy_dbg & 4)) ? window_const(a, (int64_t)a.lazy_t - wmax, wmax)
                                                                    : make_float2(0.0f, 0.0f);
    if (LSPEC && lz && proc && (lag & 1) && !(a.lazy_dbg & 8)) {
        L::load(p, src_w, lr_, D, sub);
        if (sub == 0 && a.has_bias) pb = src_b[lr_];
    }

    if (MODE != kGradOnly && proc && !(LSPEC && lz)) {
        if (NT == 2) {
            L::load_nt(p, src_w, lr_, D, sub);
            if (adam) L::load_nt(m, a.w_m[t], lr_, D, sub); else L::zero(m);
            if (has_v) L::load_nt(v, a.w_v[t], lr_, D, sub); else L::zero(v);
        } else {
            L::load(p, src_w, lr_, D, sub);
            if (!(LSPEC && lz)) {
                if (adam) L::load(m, a.w_m[t], lr_, D, sub); else L::zero(m);
                if (has_v) L::load(v, a.w_v[t], lr_, D, sub); else L::zero(v);
            }
        }
        if (sub == 0 && a.has_bias) {
            pb = src_b[lr_];
            if (!(LSPEC && lz)) {
                if (adam) mb = a.b_m[t][lr_];
                if (has_v) vb = a.b_v[t][lr_];
            }
        }
    }
    L::zero(g);
    float gb = 0.0f;
    bool guarded = false;
    if constexpr (GUARD) guarded = a.guard[r] > 0;

    if (MODE == kApplyDense) {
        const float *gbase;
        int64_t gkk, gbi;
        grad_loc(a, t, lr_, gk, nr, gbase, gkk, gbi);
        L::load(g, gbase, gkk, D, sub);
        if (sub == 0) gb = a.grad[gbi];
    } else if (!COLD) {
        const int c = lz ? cnt : (COLD ? 0 : a.row_count[r]);
        // SPEC: the list and the item's partial-slot range are loaded beside the count
        // (entries past the count are stale and never used), so a touched row's partner
        // rows are its only dependent round trip
        int2 spec[SPEC ? kCap : 1];
        int s0 = 0, s1 = 0;
        if (SPEC && !lz) {
            const int4 *lst = reinterpret_cast<const int4 *>(a.row_list + r * kCap);
#pragma unroll
            for (int e = 0; e < kCap / 2; ++e) {
                const int4 v = lst[e];
                spec[2 * e] = make_int2(v.x, v.y);
                spec[2 * e + 1] = make_int2(v.z, v.w);
            }
            if (t == 1 && a.item_slot_off != nullptr) { s0 = a.item_slot_off[lr_]; s1 = a.item_slot_off[lr_ + 1]; }
        }
        // kGradOnly (the data-parallel item gradient: a short, latency-bound launch over rows
        // that are nearly all touched): every load of the row -- all partner rows, the
        // overflow accumulators, the first planned partials -- issues in ONE round trip after
        // the list instead of a dependent chain; the sums keep their order (same bits)
        constexpr bool kOneTrip = MODE == kGradOnly && SPEC;
        float h0[kOneTrip ? 4 : 1][EPL];
        float hb0[kOneTrip ? 4 : 1];
        const bool parts = t == 1 && a.item_slot_off != nullptr;
        if (kOneTrip && parts && s1 > s0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ss = s0 + u < s1 ? s0 + u : s0;
                L::load(h0[kOneTrip ? u : 0], a.part_row, ss, D, sub);
                hb0[kOneTrip ? u : 0] = a.has_bias ? a.part_bias[ss] : 0.0f;
            }
        }
        if (c > 0 && !guarded) {
            const int ne = c < kCap ? c : kCap;
            int2 ent[kCap];
#pragma unroll
            for (int e = 0; e < kCap; ++e)
                ent[e] = e < ne ? ((LSPEC && lz) ? lspec[LSPEC ? e : 0]
                                   : (SPEC && !lz) ? spec[SPEC ? e : 0] : a.row_list[r * kCap + e]) : make_int2(0, 0);
            // the entries' slots were claimed by atomics in arrival order: sorted by (partner,
            // dz bits) the row sums them in an order independent of that timing, so a step
            // whose rows do not overflow is bit-reproducible run to run
            sort_entries(ent, ne);
            // MF: the partner row of the other table; NCF: the stored gradient half
            const float *other = a.contrib ? a.contrib + t * D : a.w_in[t ^ 1];
            const int64_t ostride = a.contrib ? a.contrib_stride : (int64_t)D;
            // partner rows in groups of PG list entries (kPullGroup; most touched rows have
            // 1-2 entries): a later group's gathers issue only when some row of the wave needs them,
            // and the smaller register footprint raises occupancy
            constexpr int PG = kOneTrip ? kCap : kPullGroup;
            // an overflowed row (c > kCap) sums list and surplus in fixed point (see fix_add)
            const bool fixp = c > kCap;
            long long gf[EPL];
            long long gbf = 0;
#pragma unroll
            for (int q = 0; q < EPL; ++q) gf[q] = 0;
            long long hv[kOneTrip ? EPL : 1];
            long long hbv = 0;
            if (kOneTrip && fixp) {     // the surplus' accumulators, loaded with the partner rows
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int cc = L::elem(sub, e);
                    hv[kOneTrip ? e : 0] = (L::VEC || cc < D) ? a.hot_grad[r * (int64_t)D + cc] : 0;
                }
                if (sub == 0 && a.has_bias) hbv = a.hot_bias_grad[r];
            }
#pragma unroll
            for (int h = 0; h < kCap / PG; ++h) {
                if (h > 0 && !__any(ne > h * PG)) break;
                float o[PG][EPL];
#pragma unroll
                for (int e = 0; e < PG; ++e) {
                    if (h * PG + e < ne) L::load_strided(o[e], other, ent[h * PG + e].x, ostride, D, sub);
                    else L::zero(o[e]);
                }
#pragma unroll
                for (int e = 0; e < PG; ++e) {
                    if (h * PG + e < ne) {
                        const float dz = __int_as_float(ent[h * PG + e].y);
                        if (fixp) {
#pragma unroll
                            for (int q = 0; q < EPL; ++q) gf[q] += to_fix(dz * o[e][q]);
                            gbf += to_fix(dz);
                        } else {
#pragma unroll
                            for (int q = 0; q < EPL; ++q) g[q] = fmaf(dz, o[e][q], g[q]);
                            gb += dz;
                        }
                    }
                }
            }
            if (fixp) {
                // the surplus' accumulators (fixed point), read and reset
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int cc = L::elem(sub, e);
                    if (L::VEC || cc < D) {
                        long long *hp = a.hot_grad + r * (int64_t)D + cc;
                        gf[e] += kOneTrip ? hv[kOneTrip ? e : 0] : *hp;
                        *hp = 0;
                    }
                }
#pragma unroll
                for (int q = 0; q < EPL; ++q) g[q] = from_fix(gf[q]);
                if (sub == 0 && a.has_bias) {
                    gbf += kOneTrip ? hbv : a.hot_bias_grad[r];
                    a.hot_bias_grad[r] = 0;
                }
                gb = from_fix(gbf);
            }
            if (sub == 0 && !a.keep_count) a.row_count[r] = 0;
        }
        if (parts && !guarded) {   // planned positive partials of this item
            if (!SPEC || lz) { s0 = a.item_slot_off[lr_]; s1 = a.item_slot_off[lr_ + 1]; }
            for (int sl = s0; sl < s1; sl += 4) {
                float h[4][EPL];
                float hb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (kOneTrip && sl == s0) {        // the first four, loaded beside the partner rows
#pragma unroll
                        for (int q = 0; q < EPL; ++q) h[u][q] = h0[kOneTrip ? u : 0][q];
                        hb[u] = hb0[kOneTrip ? u : 0];
                        continue;
                    }
                    const int ss = sl + u < s1 ? sl + u : s0;
                    L::load(h[u], a.part_row, ss, D, sub);
                    hb[u] = a.has_bias ? a.part_bias[ss] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (sl + u < s1) {
#pragma unroll
                        for (int q = 0; q < EPL; ++q) g[q] += h[u][q];
                        gb += hb[u];
                    }
                }
            }
        }
        if (MODE == kGradOnly) {
            const float *gbase;
            int64_t gkk, gbi;
            grad_loc(a, t, lr_, gk, nr, gbase, gkk, gbi);
            L::store(const_cast<float *>(gbase), gkk, D, sub, g);
            if (sub == 0) a.grad[gbi] = gb;
            return;
        }
    }

    if (LAZY && !(a.lazy_dbg & 1))   // every lane of the wave (item / skipped rows: nothing to catch up)
        catch_up<L>(a, wconst, wmax, lag, a.lazy_t, sub, p, m, v, pb, mb, vb);
    if (!proc || guarded) return;
#pragma unroll
    for (int q = 0; q < EPL; ++q) p[q] = opt_update(a.opt, p[q], g[q], m[q], v[q]);
    if (NT == 3) {          // optimizer state streamed past the caches, the new row kept (next gathers)
        L::store(a.w_out[t], lr_, D, sub, p);
        if (adam) L::store_nt(a.w_m[t], lr_, D, sub, m);
        if (has_v) L::store_nt(a.w_v[t], lr_, D, sub, v);
    } else if (NT >= 1) {
        L::store_nt(a.w_out[t], lr_, D, sub, p);
        if (adam) L::store_nt(a.w_m[t], lr_, D, sub, m);
        if (has_v) L::store_nt(a.w_v[t], lr_, D, sub, v);
    } else {
        L::store(a.w_out[t], lr_, D, sub, p);
        if (adam) L::store(a.w_m[t], lr_, D, sub, m);
        if (has_v) L::store(a.w_v[t], lr_, D, sub, v);
    }
    if (sub == 0 && a.has_bias) {
        pb = opt_update(a.opt, pb, gb, mb, vb);
        a.b_out[t][lr_] = pb;
        if (adam) a.b_m[t][lr_] = mb;
        if (has_v) a.b_v[t][lr_] = vb;
    }
    if (lz && sub == 0) {
        a.last_rel[r] = (int32_t)((int64_t)a.lazy_t - a.lazy_base);
        if (a.lazy_rows) atomicAdd(a.lazy_rows, 1ull);
    }
}

// the MT19937 walk one workgroup of a dense-pass launch can carry (rg_mt_gen_t)
struct MtGenArgs {
    uint32_t *state, *out, *state_before;
    int64_t nwords;
};

// Grid of mf_back_kernel: [MT walk block (optional)] [prepare blocks] [padding] [apply
// blocks, apply_padded = a multiple of 8 starting at an absolute index that is one].
// Workgroups go to the 8 XCDs round-robin by absolute index, so with xcd_map the apply
// block of absolute index B processes row group (B % 8) * apply_padded / 8 + B / 8: each
// XCD streams one contiguous eighth of the rows, and the per-row small arrays (biases,
// counts: 4 B per row, 16 B per wave) fill whole lines in ONE XCD's L2 instead of each
// line being fetched and partially written back by all eight.
struct BackGrid {
    int64_t prep_blocks, apply_start, apply_padded;
    int32_t prep_first, xcd_map;
    int64_t upd_blocks;   // NCF step: MLP update workgroups after the prepare's (rg_ncf_tail)
};

template <class L>
int64_t pairs_blocks(int64_t cols) {
    constexpr int64_t UPB = kPairBlock / L::LPU;
    return (cols + UPB - 1) / UPB;
}

// ---------------------------------------------------------------------------- host helpers
// Argument checks and conversions of the C structs, and the two launches of product kernels
// that rg_mf_alt.hip needs (one launcher per kernel); all defined in rg_mf.hip.
#pragma GCC visibility push(hidden)
int check_tables(const rg_mf_tables_t *t);
int pairs_args(const rg_mf_tables_t *t, const rg_mf_batch_t *b, const rg_mf_work_t *w, int32_t backward,
               PairsArgs &a);
int prepare_args(const rg_mf_batch_t *b, const rg_mf_work_t *w, const rg_mf_mark_t *mark, PairsArgs &a);
int apply_args(const rg_mf_tables_t *t, const rg_mf_work_t *w, const float *grad_in, float *grad_out,
               const rg_opt_t *opt, int64_t row_begin, int64_t row_end, const rg_mf_loss_t *loss,
               float *dense_loss_out, int mode, ApplyArgs &a);
int gen_args(const rg_mt_gen_t *gen, MtGenArgs &g, const char *what);
// mf_prepare_kernel over `total` threads (prepare_threads)
int launch_prepare(void *stream, const PairsArgs &a, int2 *out, int64_t total, int prio, const char *what);
// the whole-table dense pass with a.last_rel / a.umark set (mf_back_kernel's LAZY instantiations)
int launch_back_lazy(void *stream, int32_t dim, ApplyArgs &a, const MtGenArgs &gen);
#pragma GCC visibility pop

}  // namespace rg
