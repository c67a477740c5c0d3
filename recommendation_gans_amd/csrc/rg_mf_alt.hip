// Whole-step alternatives of the matrix-factorisation step (gfx950 / MI355X): four ways to
// run a training step that measured slower than the split step of rg_mf.hip (DESIGN §4.1,
// §9).  rg_stepper_alt.cpp selects them by switches that are constant off in the product
// library; their tests run on the A/B build (build.py --variant NAME -DRG_AB=1).
//
//   overlapped step           (RG_FUSED)  rg_mf_step_front / _cold / _hot
//   single-launch pipelined   (RG_PIPE)   rg_mf_pipe_step
//   two-launch pipelined      (RG_PIPE2)  rg_mf_pipe2_hot / _cold, rg_mf_prepare_hot
//   lazy dense pass           (RG_LAZY)   rg_mf_pairs_prepare, rg_mf_apply_lazy, rg_mf_lazy_flush
//
// Each section holds one alternative complete: kernels, argument structs, launch functors and
// C entry points.  The kernels are built from the device bodies of rg_mf_kernels.h; a product
// kernel is never instantiated here (one launcher per kernel: the library has no relocatable
// device code) -- where an alternative needs one it calls rg_mf.hip's host function.
#include <algorithm>
#include <type_traits>
#include <cstdlib>

#include <hip/hip_ext.h>

// the diagnostic build's stamp globals live in rg_mf.hip: no stamps in this file's kernels
#undef RG_DIAG_STAMPS
#include "rg_mf_kernels.h"

namespace rg {

// ---------------------------------------------------------------------------- overlapped step
// One training step as two launches instead of prepare / pairs / apply:
//
//   mf_front_kernel  blocks [0, P)        the pair pass of this step (pairs_body)
//                    blocks [P, P + Q)    the prepare pass of the NEXT step (stamps
//                                         the rows it will touch with its serial)
//                    blocks [P + Q, ...)  the optimizer update of every COLD row of
//                                         this step (stamp != this step's serial):
//                                         zero data gradient, so it needs nothing
//                                         from the pair pass and streams beside it
//   mf_hot_kernel    the update of the touched rows, one per owner flag of the
//                    prepared pairs, pulling the pair pass's lists / partials
//
// The latency-bound pair pass (gathers, atomics, LDS) thus hides under two thirds
// of the HBM-bound dense optimizer pass instead of preceding all of it.
struct FrontArgs {
    int64_t pair_blocks, prep_blocks;
    int2 *prep_out;                 // next step's pairs buffer (prep_blocks > 0)
    const int32_t *cold_stamp;      // this step's stamps
    int32_t cold_serial;
};

template <class L, int NMAX>
__global__ __launch_bounds__(kBlock) void mf_front_kernel(PairsArgs pa, PairsArgs prep, ApplyArgs aa, FrontArgs f) {
    const int64_t blk = blockIdx.x;
    if (blk < f.pair_blocks) {
        if constexpr (kPairBlock == kBlock) pairs_body<L, kFused, NMAX>(pa, blk);   // (host refuses otherwise)
        return;
    }
    if (blk < f.pair_blocks + f.prep_blocks) {
        prepare_one(prep, f.prep_out, (blk - f.pair_blocks) * kBlock + threadIdx.x);
        return;
    }
    constexpr int LPU = L::LPU, UPW = L::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t wave = ((blk - f.pair_blocks - f.prep_blocks) * kBlock + threadIdx.x) >> 6;
    const int64_t r = aa.row_begin + wave * UPW + (lane / LPU);
    if (r >= aa.row_end) return;
    if (f.cold_stamp[r] == f.cold_serial) return;           // touched: mf_hot_kernel
    apply_row<L, kApplyPull, 0, true>(aa, r, sub);
}

// the cold-row update of the front grid as a launch of its own (two-stream schedule:
// beside rg_mf_pairs on another stream, at its own register budget)
template <class L>
__global__ __launch_bounds__(kBlock) void mf_cold_kernel(ApplyArgs a, const int32_t *__restrict__ stamp,
                                                        int32_t serial) {
    constexpr int LPU = L::LPU, UPW = L::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t r = a.row_begin + wave * UPW + (lane / LPU);
    if (r >= a.row_end) return;
    if (stamp[r] == serial) return;
    apply_row<L, kApplyPull, 0, true>(a, r, sub);
}

// row-ordered variant: scan the rows, update those stamped with this step's serial
// (sequential addresses with holes instead of the pairs' random order)
template <class L>
__global__ __launch_bounds__(kBlock) void mf_hot_scan_kernel(ApplyArgs a, const int32_t *__restrict__ stamp,
                                                            int32_t serial) {
    constexpr int LPU = L::LPU, UPW = L::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    if (a.loss_out != nullptr && blockIdx.x == 0 && threadIdx.x < kWave) {
        const float lv = finalize_loss(a.partials, a.n_partials, a.inv_a, a.inv_b, lane);
        if (lane == 0) *a.loss_out = lv;
    }
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t r = a.row_begin + wave * UPW + (lane / LPU);
    if (r >= a.row_end) return;
    if (stamp[r] != serial) return;
    apply_row<L, kApplyPull, 0, false>(a, r, sub);
}

// slot k = (pair k >> 1, side k & 1): the row the slot's pair touches on that side,
// updated here iff the slot owns it (exactly one owner per touched row)
template <class L>
__global__ __launch_bounds__(kBlock) void mf_hot_kernel(ApplyArgs a, const int2 *__restrict__ pairs, int64_t n_slots,
                                                       int stride, int np_) {
    constexpr int LPU = L::LPU, UPW = L::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    if (a.loss_out != nullptr && blockIdx.x == 0 && threadIdx.x < kWave) {
        const float lv = finalize_loss(a.partials, a.n_partials, a.inv_a, a.inv_b, lane);
        if (lane == 0) *a.loss_out = lv;
    }
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t k = wave * UPW + (lane / LPU);
    if (k >= n_slots) return;
    if ((int)((k >> 1) % stride) >= np_) return;   // a record's plan-slot / padding entries
    const int2 pr = pairs[k >> 1];
    const int32_t x = (k & 1) ? pr.y : pr.x;
    if (x >= 0) return;                                     // owner flag (bit 31) not set
    const int64_t r = (k & 1) ? a.num_users + (x & kIdMask) : (int64_t)(x & kIdMask);
    if (r < a.row_begin || r >= a.row_end) return;
    apply_row<L, kApplyPull, 0, false>(a, r, sub);
}

}  // namespace rg

using namespace rg;

namespace {
struct FrontLaunchF {
    PairsArgs *pa, *prep;
    ApplyArgs *aa;
    FrontArgs f;
    hipStream_t s;
    template <class L>
    int operator()() {
        f.pair_blocks = pairs_blocks<L>(pa->cols);
        const int64_t cold_rows = aa->row_end - aa->row_begin;
        const int64_t cold_waves = (cold_rows + L::UPW - 1) / L::UPW;
        const int64_t cold_blocks = (cold_waves + kBlock / kWave - 1) / (kBlock / kWave);
        const dim3 grid((unsigned)(f.pair_blocks + f.prep_blocks + cold_blocks));
        if (pa->n_neg <= 5)
            hipLaunchKernelGGL((mf_front_kernel<L, 5>), grid, dim3(kBlock), 0, s, *pa, *prep, *aa, f);
        else
            hipLaunchKernelGGL((mf_front_kernel<L, kNMax>), grid, dim3(kBlock), 0, s, *pa, *prep, *aa, f);
        return check_launch("rg_mf_step_front");
    }
};

struct HotLaunchF {
    ApplyArgs *a;
    const int2 *pairs;
    int64_t n_slots;
    int stride, np_;
    const rg_mf_mark_t *mark;
    hipStream_t s;
    template <class L>
    int operator()() {
        if (mark) {
            const int64_t rows = a->row_end - a->row_begin;
            const int64_t waves = (rows + L::UPW - 1) / L::UPW;
            const int64_t nb = (waves + kBlock / kWave - 1) / (kBlock / kWave);
            hipLaunchKernelGGL((mf_hot_scan_kernel<L>), dim3(nb < 1 ? 1 : nb), dim3(kBlock), 0, s, *a, mark->stamp,
                               mark->serial);
            return check_launch("rg_mf_step_hot");
        }
        const int64_t waves = (n_slots + L::UPW - 1) / L::UPW;
        const int64_t nb = (waves + kBlock / kWave - 1) / (kBlock / kWave);
        hipLaunchKernelGGL((mf_hot_kernel<L>), dim3(nb < 1 ? 1 : nb), dim3(kBlock), 0, s, *a, pairs, n_slots, stride,
                           np_);
        return check_launch("rg_mf_step_hot");
    }
};
}  // namespace

extern "C" int rg_mf_step_front(void *stream, const rg_mf_tables_t *t, const rg_mf_batch_t *cur, rg_mf_work_t *w,
                                const rg_mf_mark_t *cur_mark, const rg_opt_t *opt, int64_t cold_begin,
                                int64_t cold_end, const rg_mf_batch_t *next, const rg_mf_work_t *next_w,
                                const rg_mf_mark_t *next_mark) {
    if (kPairBlock != kBlock) return fail_arg("rg_mf_step_front: built with a pair-pass workgroup != 256 threads");
    if (!cur_mark || !cur_mark->stamp || cur_mark->serial == 0)
        return fail_arg("rg_mf_step_front: the current step's pairs must be prepared with row marks");
    if (cur && cur->loss == RG_LOSS_ADAPTIVE_HINGE)
        return fail_arg("rg_mf_step_front: adaptive hinge needs the global max first (use rg_mf_pairs)");
    PairsArgs pa, prep{};
    int rc = pairs_args(t, cur, w, 1, pa);
    if (rc) return rc;
    ApplyArgs aa;
    if ((rc = apply_args(t, w, nullptr, nullptr, opt, cold_begin, cold_end, nullptr, nullptr, kApplyPull, aa)))
        return rc;
    FrontArgs f{};
    f.cold_stamp = cur_mark->stamp;
    f.cold_serial = cur_mark->serial;
    if (next) {
        if (!next_mark || next_mark->stamp == cur_mark->stamp || next_mark->serial == cur_mark->serial)
            return fail_arg("rg_mf_step_front: the next step needs its own stamp array and serial");
        if ((rc = prepare_args(next, next_w, next_mark, prep))) return rc;
        if (next->pairs == cur->pairs) return fail_arg("rg_mf_step_front: next pairs buffer aliases the current");
        f.prep_out = reinterpret_cast<int2 *>(next->pairs);
        f.prep_blocks = (prepare_threads(next->cols, next->n_neg) + kBlock - 1) / kBlock;
    }
    FrontLaunchF fl{&pa, &prep, &aa, f, (hipStream_t)stream};
    return dispatch_dim(t->dim, fl);
}

namespace {
struct ColdLaunchF {
    ApplyArgs *a;
    const rg_mf_mark_t *mark;
    hipStream_t s;
    template <class L>
    int operator()() {
        const int64_t rows = a->row_end - a->row_begin;
        if (rows <= 0) return RG_OK;
        const int64_t waves = (rows + L::UPW - 1) / L::UPW;
        const int64_t nb = (waves + kBlock / kWave - 1) / (kBlock / kWave);
        hipLaunchKernelGGL((mf_cold_kernel<L>), dim3(nb), dim3(kBlock), 0, s, *a, mark->stamp, mark->serial);
        return check_launch("rg_mf_step_cold");
    }
};
}  // namespace

extern "C" int rg_mf_step_cold(void *stream, const rg_mf_tables_t *t, const rg_mf_mark_t *mark, const rg_opt_t *opt,
                               int64_t row_begin, int64_t row_end) {
    if (!mark || !mark->stamp || mark->serial == 0) return fail_arg("rg_mf_step_cold: bad mark");
    ApplyArgs a;
    int rc = apply_args(t, nullptr, nullptr, nullptr, opt, row_begin, row_end, nullptr, nullptr, kApplyCold, a);
    if (rc) return rc;
    ColdLaunchF f{&a, mark, (hipStream_t)stream};
    return dispatch_dim(t->dim, f);
}

extern "C" int rg_mf_step_hot(void *stream, const rg_mf_tables_t *t, const rg_mf_batch_t *cur, rg_mf_work_t *w,
                              const rg_mf_mark_t *mark, const rg_opt_t *opt, int64_t row_begin, int64_t row_end,
                              const rg_mf_loss_t *loss) {
    if (!cur || !cur->pairs) return fail_arg("rg_mf_step_hot: null batch/pairs");
    if (mark && (!mark->stamp || mark->serial == 0)) return fail_arg("rg_mf_step_hot: bad mark");
    ApplyArgs a;
    int rc = apply_args(t, w, nullptr, nullptr, opt, row_begin, row_end, loss, nullptr, kApplyPull, a);
    if (rc) return rc;
    HotLaunchF f{&a, reinterpret_cast<const int2 *>(cur->pairs), 2 * (int64_t)pair_stride(cur->n_neg) * cur->cols,
                 pair_stride(cur->n_neg), 1 + cur->n_neg, mark,
                 (hipStream_t)stream};
    return dispatch_dim(t->dim, f);
}

namespace rg {

// ---------------------------------------------------------------------------- pipelined step
// One launch per training step t that also runs the pair pass of step t + 1 and the prepare of
// step t + 2 (rg_mf_pipe_step, the stepper's default single-GPU step):
//
//   [prepare t+2]  the next-but-one step's draws -> pool pairs, list-slot claims, and the list
//                  of users it claims a first slot of (the users pair pass t+2 will read)
//   [hot items]    the dense update of every item row              } the rows pair pass t+1
//   [hot users]    the dense update of the users of step t+1's list } reads; write-through
//                  stores, then each workgroup adds 1 to the gate
//   [cold users 1] the dense update of the other users
//   [pair t+1]     waits until the gate counts every hot workgroup, then runs step t+1's pair
//                  pass on the updated rows (loads past L1) beside the cold stream
//   [cold users 2]
//
// The latency-bound pair pass (~11 us on its own) thus overlaps the HBM-bound update of the rows
// it does not read.  Deadlock-free by construction: only pair workgroups wait, on workgroups that
// never wait, and they are too few (cols / units-per-workgroup) to hold every slot of the chip.
// Results are bit-identical to the split step (same per-row and per-column arithmetic).
struct PipeArgs {
    const int32_t *hot_users, *nhot;   // step t+1's hot user list
    const int32_t *counts_next;        // step t+1's claims (a user with one is hot)
    int32_t *gate, *gate_next, *nhot_free, *err;
    int64_t prep_blocks, item_blocks, huser_blocks, cold1_blocks, pair_blocks, cold2_blocks;
    int64_t users_begin;               // unified row of user 0 in the dense rows (0)
    uint32_t spin_limit;
};

template <class L, bool WT>
__device__ __forceinline__ void pipe_rows(const ApplyArgs &a, const int64_t r, const bool valid, const int sub) {
    LeanRow<L> x;
    lean_load<L>(a, r, sub, valid, x);
    lean_finish<L, WT>(a, r, sub, valid, x);
}

template <class L, int NMAX>
__global__ __launch_bounds__(kBlock) void mf_pipe_kernel(ApplyArgs a, PairsArgs pa, PairsArgs prep, int2 *prep_out,
                                                         PipeArgs pp, MtGenArgs gen) {
    static_assert(kPairBlock == kBlock, "the pair workgroups share the launch's block size");
    constexpr int LPU = L::LPU, UPW = L::UPW;
    int64_t blk = blockIdx.x;
    if (gen.nwords > 0) {
        if (blk == 0) {
            __shared__ uint32_t X[kRing + 2];
            mt_generate_block(X, gen.state, gen.out, gen.nwords, gen.state_before);
            return;
        }
        --blk;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t rows_per_block = (kBlock / kWave) * UPW;
    const int64_t U = a.num_users;
    if (blk < pp.prep_blocks) {                              // prepare of step t + 2
        if (blk == 0 && threadIdx.x == 0) {                  // counters of later launches
            *pp.gate_next = 0;
            *pp.nhot_free = 0;
        }
        if (blk == 0 && a.loss_out != nullptr && threadIdx.x >= kWave && threadIdx.x < 2 * kWave) {
            const float lv = finalize_loss(a.partials, a.n_partials, a.inv_a, a.inv_b, lane);   // step t's loss
            if (lane == 0) *a.loss_out = lv;
        }
        prepare_one(prep, prep_out, blk * kBlock + threadIdx.x);
        return;
    }
    blk -= pp.prep_blocks;
    const int64_t in_block = (threadIdx.x >> 6) * UPW + lane / LPU;   // row slot of this lane group
    const bool hot = blk < pp.item_blocks + pp.huser_blocks;
    int64_t row = 0;
    bool valid = false;
    if (hot) {                                               // the rows pair pass t + 1 reads
        if (blk < pp.item_blocks) {
            const int64_t k = blk * rows_per_block + in_block;
            valid = k < a.num_items;
            row = U + (valid ? k : 0);
        } else {
            const int64_t k = (blk - pp.item_blocks) * rows_per_block + in_block;
            valid = k < *pp.nhot;
            row = valid ? (int64_t)pp.hot_users[k] : 0;
        }
    } else {
        blk -= pp.item_blocks + pp.huser_blocks;
        int64_t cold;
        if (blk < pp.cold1_blocks) {
            cold = blk;
        } else if (blk < pp.cold1_blocks + pp.pair_blocks) {     // pair pass of step t + 1
        const int64_t pb = blk - pp.cold1_blocks;
        if (threadIdx.x == 0) {
            const int target = (int)(pp.item_blocks + pp.huser_blocks);
            uint32_t spins = 0;
            while (__hip_atomic_load(pp.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > pp.spin_limit) {               // bounded: flag and go on (wrong results)
                    atomicOr(pp.err, 1);
                    break;
                }
            }
        }
        __syncthreads();
        pairs_body<L, kFused, NMAX, true>(pa, pb);
        return;
        } else {
            cold = blk - pp.pair_blocks;
        }
        // cold users: chunk `cold` of the user rows, minus the hot ones
        const int64_t u = cold * rows_per_block + in_block;
        valid = u < U && pp.counts_next[u] <= 0;
        row = valid ? u : 0;
    }
    if (__any(valid)) {
        if (hot) pipe_rows<L, true>(a, row, valid, sub);   // read by the pair pass: write-through
        else pipe_rows<L, false>(a, row, valid, sub);
    }
    if (hot) {   // publish: every wave's write-through stores done, then one add for the workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(pp.gate, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace rg

namespace {
struct PipeLaunchF {
    ApplyArgs *a;
    PairsArgs *pa, *prep;
    int2 *prep_out;
    PipeArgs pp;
    MtGenArgs gen;
    int64_t pair_cols, pair_users;
    hipStream_t s;
    template <class L>
    int operator()() {
        if constexpr (L::LPU < kCap) {
            return fail_arg("rg_mf_pipe_step: dim must be a multiple of 4 and >= 32");
        } else {
            const int64_t rpb = (kBlock / kWave) * L::UPW;
            pp.item_blocks = (a->num_items + rpb - 1) / rpb;
            const int64_t hu = pair_users < a->num_users ? pair_users : a->num_users;
            pp.huser_blocks = (hu + rpb - 1) / rpb;
            const int64_t cold = (a->num_users + rpb - 1) / rpb;
            // cold rows ahead of the pair workgroups: about one chip's worth, so the hot rows are
            // mostly done when the pair workgroups start waiting
            static const int64_t c1 = [] { const char *e = getenv("RG_PIPE_COLD1"); return e ? atoll(e) : 2048LL; }();
            pp.cold1_blocks = cold < c1 ? cold : c1;
            pp.cold2_blocks = cold - pp.cold1_blocks;
            pp.pair_blocks = pairs_blocks<L>(pair_cols);
            const int64_t total = (gen.nwords > 0 ? 1 : 0) + pp.prep_blocks + pp.item_blocks + pp.huser_blocks +
                                  pp.cold1_blocks + pp.pair_blocks + pp.cold2_blocks;
            LaunchEvents &le = launch_events();
            const hipEvent_t e0 = le.start, e1 = le.stop;
            le = LaunchEvents{};
            auto go = [&](auto kernel) {
                if (e0 || e1)
                    hipExtLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(kBlock), 0, s, e0, e1, 0, *a, *pa, *prep,
                                          prep_out, pp, gen);
                else
                    hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(kBlock), 0, s, *a, *pa, *prep, prep_out, pp,
                                       gen);
            };
            if (pa->n_neg <= 5) go(mf_pipe_kernel<L, 5>);
            else go(mf_pipe_kernel<L, kNMax>);
            return check_launch("rg_mf_pipe_step");
        }
    }
};
}  // namespace

extern "C" int rg_mf_pipe_step(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const rg_opt_t *opt,
                               const rg_mf_loss_t *loss, const rg_mf_batch_t *pair_b, rg_mf_work_t *pair_w,
                               const rg_mf_batch_t *next, const rg_mf_work_t *next_w, const rg_mf_pipe_t *pipe,
                               const rg_mt_gen_t *gen) {
#if !RG_AB
    (void)stream; (void)t; (void)w; (void)opt; (void)loss; (void)pair_b; (void)pair_w; (void)next; (void)next_w;
    (void)pipe; (void)gen;
    // measured 4x slower than the split step: carried by the A/B build only
    return fail_arg("rg_mf_pipe_step: the pipelined step is an A/B build (build.py --variant NAME -DRG_AB=1)");
#else
    if (kPairBlock != kBlock) return fail_arg("rg_mf_pipe_step: built with a pair-pass workgroup != 256 threads");
    if (!pipe || !pipe->hot_users || !pipe->nhot || !pipe->counts_next || !pipe->gate || !pipe->gate_next ||
        !pipe->nhot_free || !pipe->err)
        return fail_arg("rg_mf_pipe_step: incomplete rg_mf_pipe_t");
    if (!pair_b || !pair_w) return fail_arg("rg_mf_pipe_step: null pair batch / work");
    if (pair_b->loss != RG_LOSS_POINTWISE && pair_b->loss != RG_LOSS_BPR && pair_b->loss != RG_LOSS_HINGE)
        return fail_arg("rg_mf_pipe_step: pointwise, bpr or hinge only (the adaptive hinge needs the max first)");
    if (pair_w->claim_num_users <= 0) return fail_arg("rg_mf_pipe_step: the paired step must carry claimed slots");
    if ((t->num_users > t->num_items ? t->num_users : t->num_items) * (int64_t)t->dim * 4 >= ((int64_t)1 << 31))
        return fail_arg("rg_mf_pipe_step: tables of 2 GiB or more (32-bit write-through offsets)");
    if (pair_w->row_list == w->row_list || pair_w->hot_grad == w->hot_grad || pair_w->loss_partials == w->loss_partials ||
        (w->part_row && pair_w->part_row == w->part_row))
        return fail_arg("rg_mf_pipe_step: the paired step's scratch must not alias this step's");
    ApplyArgs a;
    int rc = apply_args(t, w, nullptr, nullptr, opt, 0, -1, loss, nullptr, kApplyPull, a);
    if (rc) return rc;
    // the pair pass reads the tables this launch writes
    rg_mf_tables_t pt = *t;
    pt.user_w = t->user_w_out; pt.item_w = t->item_w_out; pt.user_b = t->user_b_out; pt.item_b = t->item_b_out;
    PairsArgs pa;
    if ((rc = pairs_args(&pt, pair_b, pair_w, 1, pa))) return rc;
    PairsArgs prep{};
    int2 *prep_out = nullptr;
    PipeArgs pp{};
    if (next) {
        if ((rc = prepare_args(next, next_w, nullptr, prep))) return rc;
        if (!prep.claimed || !pipe->hot_out || !pipe->nhot_out)
            return fail_arg("rg_mf_pipe_step: the prepared step needs claimed slots and a hot list");
        if (next->pairs == pair_b->pairs) return fail_arg("rg_mf_pipe_step: prepared pairs alias the paired step's");
        prep.hot_out = pipe->hot_out;
        prep.nhot_out = pipe->nhot_out;
        prep_out = reinterpret_cast<int2 *>(next->pairs);
        pp.prep_blocks = (prepare_threads(next->cols, next->n_neg) + kBlock - 1) / kBlock;
    } else {
        pp.prep_blocks = 1;   // block 0 still resets the counters and finalizes the loss
        prep.cols = 0;
    }
    MtGenArgs g{};
    if (gen && gen->nwords > 0) {
        if (!gen->state || !gen->out) return fail_arg("rg_mf_pipe_step: null MT state / output");
        g.state = gen->state; g.out = gen->out; g.state_before = gen->state_before; g.nwords = gen->nwords;
    }
    pp.hot_users = pipe->hot_users; pp.nhot = pipe->nhot; pp.counts_next = pipe->counts_next;
    pp.gate = pipe->gate; pp.gate_next = pipe->gate_next; pp.nhot_free = pipe->nhot_free; pp.err = pipe->err;
    static const uint32_t spin = [] { const char *e = getenv("RG_PIPE_SPIN"); return e ? (uint32_t)atoll(e) : 4000000u; }();
    pp.spin_limit = spin;
    PipeLaunchF f{&a, &pa, &prep, prep_out, pp, g, pair_b->cols, (int64_t)(1 + pair_b->n_neg) * pair_b->cols,
                  (hipStream_t)stream};
    return dispatch_dim(t->dim, f);
#endif
}

namespace rg {

// ---------------------------------------------------------------------------- two-launch pipelined step
// The single-GPU step as two launches per step t, overlapping step t+1's latency-bound pair pass
// with the HBM-bound update of the rows that pass does not read:
//
//   hot launch  (mf_pipe2_hot_kernel):  the dense update of step t for every item row and for the
//               users step t+1's pair pass reads (its prepare's hot list); step t's loss
//   cold launch (mf_pipe2_cold_kernel): [step t+1's pair pass] [the MT walk of a later unit]
//               [step t+2's prepare, appending its hot list] [the dense update of step t for every
//               other user (its claim count of step t+1 is zero)]
//
// The pair pass reads only rows the hot launch wrote (stream order: no gate, no spin), and the
// cold rows it leaves to the same launch are rows it does not read.  Per-row and per-column
// arithmetic is the split step's, so results are bit-identical to it.  A unit's scratch alternates
// by parity (claims in three count arrays, lists / overflow accumulators / partials in two sets:
// rg_stepper.cpp train_pipe2).
struct Pipe2Args {
    const int32_t *hot;           // hot launch: the users step t+1's pair pass reads
    const int32_t *nhot;          // hot launch: their number (device)
    int64_t hot_blocks, item_blocks;
    int32_t *nhot_clear;          // hot launch: zeroed (the list the cold launch's prepare appends to)
    const int32_t *counts_next;   // cold launch: step t+1's claims (a user with one is hot)
    int64_t pair_blocks, prep_blocks, cold_blocks;
};

template <class LD>
__global__ __launch_bounds__(kBlock) void mf_pipe2_hot_kernel(ApplyArgs a, Pipe2Args p, MtGenArgs gen) {
    int64_t blk = blockIdx.x;
    if (gen.nwords > 0) {
        if (blk == 0) {
            __shared__ uint32_t X[kRing + 2];
            mt_generate_block(X, gen.state, gen.out, gen.nwords, gen.state_before);
            return;
        }
        --blk;
    }
    constexpr int LPU = LD::LPU, UPW = LD::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    if (blk == 0) {
        if (threadIdx.x == 0 && p.nhot_clear != nullptr) *p.nhot_clear = 0;
        if (a.loss_out != nullptr && threadIdx.x >= kWave && threadIdx.x < 2 * kWave) {
            const float lv = finalize_loss(a.partials, a.n_partials, a.inv_a, a.inv_b, lane);   // step t's loss
            if (lane == 0) *a.loss_out = lv;
        }
    }
    constexpr int64_t rpb = (kBlock / kWave) * UPW;
    const int64_t in_block = (threadIdx.x >> 6) * UPW + lane / LPU;
    int64_t r;
    if (blk < p.item_blocks) {
        const int64_t k = blk * rpb + in_block;
        if (k >= a.num_items) return;
        r = a.num_users + k;
    } else {
        const int64_t j = (blk - p.item_blocks) * rpb + in_block;
        if (j >= (int64_t)*p.nhot) return;
        r = p.hot[j];
    }
    apply_row<LD, kApplyPull, 0, false, true>(a, r, sub);
}

template <class LP, class LD, int NMAX>
__global__ __launch_bounds__(kBlock) void mf_pipe2_cold_kernel(ApplyArgs a, PairsArgs pa, PairsArgs prep,
                                                               int2 *prep_out, Pipe2Args p, MtGenArgs gen) {
    static_assert(kPairBlock == kBlock, "the pair workgroups share the launch's block size");
    int64_t blk = blockIdx.x;
    if (blk < p.pair_blocks) {                  // first in the grid: the step's latency chain
        pairs_body<LP, kFused, NMAX>(pa, blk);
        return;
    }
    blk -= p.pair_blocks;
    if (gen.nwords > 0) {
        if (blk == 0) {
            __shared__ uint32_t X[kRing + 2];
            mt_generate_block(X, gen.state, gen.out, gen.nwords, gen.state_before);
            return;
        }
        --blk;
    }
    if (blk < p.prep_blocks) {
        prepare_one(prep, prep_out, blk * kBlock + threadIdx.x);
        return;
    }
    blk -= p.prep_blocks;
    constexpr int LPU = LD::LPU, UPW = LD::UPW;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t u = blk * ((kBlock / kWave) * UPW) + (threadIdx.x >> 6) * UPW + lane / LPU;
    if (u >= a.num_users) return;
    // a user with a claim of step t+1 was updated by the hot launch: its guard is loaded beside its
    // other loads (wasted bytes for it, but no round trip in front of every row)
    apply_row<LD, kApplyPull, 0, false, true, false, false, true>(a, u, sub);
}

}  // namespace rg

namespace {
struct Pipe2HotF {
    ApplyArgs *a;
    Pipe2Args p;
    MtGenArgs gen;
    int64_t hot_cap;
    hipStream_t s;
    template <class L>
    int operator()() {
        using LD = typename BackLayout<L>::type;
        constexpr int64_t rpb = (kBlock / kWave) * LD::UPW;
        p.item_blocks = (a->num_items + rpb - 1) / rpb;
        p.hot_blocks = (hot_cap + rpb - 1) / rpb;
        int64_t total = p.item_blocks + p.hot_blocks + (gen.nwords > 0 ? 1 : 0);
        if (total < 1) total = 1;
        LaunchEvents &le = launch_events();
        const hipEvent_t e0 = le.start, e1 = le.stop;
        le = LaunchEvents{};
        if (e0 || e1)
            hipExtLaunchKernelGGL(mf_pipe2_hot_kernel<LD>, dim3((unsigned)total), dim3(kBlock), 0, s, e0, e1, 0, *a, p,
                                  gen);
        else
            hipLaunchKernelGGL(mf_pipe2_hot_kernel<LD>, dim3((unsigned)total), dim3(kBlock), 0, s, *a, p, gen);
        return check_launch("rg_mf_pipe2_hot");
    }
};

struct Pipe2ColdF {
    ApplyArgs *a;
    PairsArgs *pa, *prep;
    int2 *prep_out;
    Pipe2Args p;
    MtGenArgs gen;
    hipStream_t s;
    template <class L>
    int operator()() {
        if (pa->n_neg <= 5) return run<L, 5>();
        return run<L, kNMax>();
    }
    template <class L, int NMAX>
    int run() {
        using LD = typename BackLayout<L>::type;
        constexpr int64_t rpb = (kBlock / kWave) * LD::UPW;
        p.pair_blocks = pairs_blocks<L>(pa->cols);
        p.cold_blocks = (a->num_users + rpb - 1) / rpb;
        const int64_t total = p.pair_blocks + (gen.nwords > 0 ? 1 : 0) + p.prep_blocks + p.cold_blocks;
        LaunchEvents &le = launch_events();
        const hipEvent_t e0 = le.start, e1 = le.stop;
        le = LaunchEvents{};
        if (e0 || e1)
            hipExtLaunchKernelGGL((mf_pipe2_cold_kernel<L, LD, NMAX>), dim3((unsigned)total), dim3(kBlock), 0, s, e0,
                                  e1, 0, *a, *pa, *prep, prep_out, p, gen);
        else
            hipLaunchKernelGGL((mf_pipe2_cold_kernel<L, LD, NMAX>), dim3((unsigned)total), dim3(kBlock), 0, s, *a, *pa,
                               *prep, prep_out, p, gen);
        return check_launch("rg_mf_pipe2_cold");
    }
};
}  // namespace

extern "C" int rg_mf_prepare_hot(void *stream, const rg_mf_batch_t *b, const rg_mf_work_t *w, int32_t *hot_out,
                                 int32_t *nhot_out) {
    PairsArgs a;
    int rc = prepare_args(b, w, nullptr, a);
    if (rc) return rc;
    if (!a.claimed || !hot_out || !nhot_out) return fail_arg("rg_mf_prepare_hot: needs claimed slots and a hot list");
    a.hot_out = hot_out;
    a.nhot_out = nhot_out;
    const int64_t total = prepare_threads(b->cols, b->n_neg);
    return launch_prepare(stream, a, reinterpret_cast<int2 *>(b->pairs), total, 0, "rg_mf_prepare_hot");
}

extern "C" int rg_mf_pipe2_hot(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const rg_opt_t *opt,
                               const rg_mf_loss_t *loss, const int32_t *hot_users, const int32_t *nhot,
                               int64_t hot_cap, int32_t *nhot_clear, const rg_mt_gen_t *gen) {
    if (!hot_users || !nhot || hot_cap < 0) return fail_arg("rg_mf_pipe2_hot: null hot list");
    ApplyArgs a;
    int rc = apply_args(t, w, nullptr, nullptr, opt, 0, -1, loss, nullptr, kApplyPull, a);
    if (rc) return rc;
    MtGenArgs g;
    if ((rc = gen_args(gen, g, "rg_mf_pipe2_hot"))) return rc;
    Pipe2Args p{};
    p.hot = hot_users;
    p.nhot = nhot;
    p.nhot_clear = nhot_clear;
    Pipe2HotF f{&a, p, g, hot_cap < t->num_users ? hot_cap : t->num_users, (hipStream_t)stream};
    return dispatch_dim(t->dim, f);
}

extern "C" int rg_mf_pipe2_cold(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const rg_opt_t *opt,
                                const rg_mf_batch_t *pair_b, rg_mf_work_t *pair_w, const int32_t *counts_next,
                                const rg_mf_batch_t *next, const rg_mf_work_t *next_w, int32_t *hot_out,
                                int32_t *nhot_out, const rg_mt_gen_t *gen) {
    if (kPairBlock != kBlock) return fail_arg("rg_mf_pipe2_cold: built with a pair-pass workgroup != 256 threads");
    if (!pair_b || !pair_w || !counts_next) return fail_arg("rg_mf_pipe2_cold: null pair batch / work / counts");
    if (pair_b->loss != RG_LOSS_POINTWISE && pair_b->loss != RG_LOSS_BPR && pair_b->loss != RG_LOSS_HINGE)
        return fail_arg("rg_mf_pipe2_cold: pointwise, bpr or hinge only (the adaptive hinge needs the max first)");
    if (pair_w->claim_num_users <= 0 || pair_w->row_count != counts_next)
        return fail_arg("rg_mf_pipe2_cold: the paired step must carry claimed slots in counts_next");
    if (pair_w->row_list == w->row_list || pair_w->hot_grad == w->hot_grad || pair_w->loss_partials == w->loss_partials ||
        (w->part_row && pair_w->part_row == w->part_row) || pair_w->row_count == w->row_count)
        return fail_arg("rg_mf_pipe2_cold: the paired step's scratch must not alias this step's");
    ApplyArgs a;
    int rc = apply_args(t, w, nullptr, nullptr, opt, 0, t->num_users, nullptr, nullptr, kApplyPull, a);
    if (rc) return rc;
    // the pair pass of step t+1 reads the tables this step writes (their rows the hot launch wrote)
    rg_mf_tables_t pt = *t;
    pt.user_w = t->user_w_out; pt.item_w = t->item_w_out; pt.user_b = t->user_b_out; pt.item_b = t->item_b_out;
    PairsArgs pa;
    if ((rc = pairs_args(&pt, pair_b, pair_w, 1, pa))) return rc;
    PairsArgs prep{};
    int2 *prep_out = nullptr;
    a.guard = counts_next;
    Pipe2Args p{};
    p.counts_next = counts_next;
    if (next) {
        if ((rc = prepare_args(next, next_w, nullptr, prep))) return rc;
        if (!prep.claimed || !hot_out || !nhot_out)
            return fail_arg("rg_mf_pipe2_cold: the prepared step needs claimed slots and a hot list");
        if (next->pairs == pair_b->pairs) return fail_arg("rg_mf_pipe2_cold: prepared pairs alias the paired step's");
        if (next_w->row_count == counts_next || next_w->row_count == w->row_count)
            return fail_arg("rg_mf_pipe2_cold: the prepared step's claims alias a live count array");
        prep.hot_out = hot_out;
        prep.nhot_out = nhot_out;
        prep_out = reinterpret_cast<int2 *>(next->pairs);
        p.prep_blocks = (prepare_threads(next->cols, next->n_neg) + kBlock - 1) / kBlock;
    }
    MtGenArgs g;
    if ((rc = gen_args(gen, g, "rg_mf_pipe2_cold"))) return rc;
    Pipe2ColdF f{&a, &pa, &prep, prep_out, p, g, (hipStream_t)stream};
    return dispatch_dim(t->dim, f);
}

// ---------------------------------------------------------------------------- lazy dense pass
namespace rg {

// the pair pass of this step (blocks [0, pair_blocks)) and the prepare pass of the NEXT
// step (the remaining blocks) in one launch: the lazy split step needs the
// next step's user marks before its dense pass starts, so the prepare moves out of the
// dense pass into this latency-bound launch, where its random pool reads run beside the
// pair pass's gathers
template <class L, int NMAX>
__global__ __launch_bounds__(kPairBlock) void mf_pairs_prep_kernel(PairsArgs a, PairsArgs prep, int2 *prep_out,
                                                                   int64_t pair_blocks) {
    const int64_t blk = blockIdx.x;
    if (blk < pair_blocks) {
        pairs_body<L, kFused, NMAX>(a, blk);
        return;
    }
    if constexpr (kPairBlock == kBlock) prepare_one(prep, prep_out, (blk - pair_blocks) * kBlock + threadIdx.x);
}

// Catch every lazily skipped user row up to step lazy_t (all of its cold updates), into the
// current set: the in-side tables of `a` (the set the last step wrote).  A row last updated
// at step ls holds its value in the set written then: the current one if lazy_t - ls is even
// (updated in place), else the other (a.w_out).
template <class L>
__global__ __launch_bounds__(kBlock) void mf_lazy_flush_kernel(ApplyArgs a) {
    constexpr int LPU = L::LPU, UPW = L::UPW, EPL = L::EPL;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPU - 1);
    const int64_t r = (((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6) * UPW + (lane / LPU);
    if (((((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6) * UPW) >= a.num_users) return;   // wave-uniform
    const bool in = r < a.num_users;
    const int32_t lsr = in ? a.last_rel[r] : 0;
    const int lag = in ? (int)((int64_t)a.lazy_t - a.lazy_base - lsr) : 0;
    const int D = a.dim;
    const bool adam = a.opt.kind == RG_OPT_ADAM;
    const bool has_v = a.opt.kind != RG_OPT_SGD;
    const float *src_w = (lag & 1) ? a.w_out[0] : a.w_in[0];
    const float *src_b = (lag & 1) ? a.b_out[0] : a.b_in[0];
    const int64_t rr = in ? r : 0;
    float p[EPL], m[EPL], v[EPL];
    float pb = 0.0f, mb = 0.0f, vb = 0.0f;
    L::zero(p); L::zero(m); L::zero(v);
    if (lag > 0) {              // current rows are read and written by nobody
        L::load(p, src_w, rr, D, sub);
        if (adam) L::load(m, a.w_m[0], rr, D, sub);
        if (has_v) L::load(v, a.w_v[0], rr, D, sub);
        if (sub == 0) {
            pb = src_b[rr];
            if (adam) mb = a.b_m[0][rr];
            if (has_v) vb = a.b_v[0][rr];
        }
    }
    // steps [lazy_t + 1 - lag, lazy_t] (the flush's window ends at lazy_t itself)
    const int wmax = wave_max(lag > 0 ? lag : 0);
    const float2 wc = wmax > 0 ? window_const(a, (int64_t)a.lazy_t + 1 - wmax, wmax) : make_float2(0.0f, 0.0f);
    catch_up<L>(a, wc, wmax, lag > 0 ? lag : 0, (int64_t)a.lazy_t + 1, sub, p, m, v, pb, mb, vb);
    if (lag <= 0) return;
    L::store(const_cast<float *>(a.w_in[0]), r, D, sub, p);
    if (adam) L::store(a.w_m[0], r, D, sub, m);
    if (has_v) L::store(a.w_v[0], r, D, sub, v);
    if (sub == 0) {
        const_cast<float *>(a.b_in[0])[r] = pb;
        if (adam) a.b_m[0][r] = mb;
        if (has_v) a.b_v[0][r] = vb;
        a.last_rel[r] = (int32_t)((int64_t)a.lazy_t - a.lazy_base);
    }
}

}  // namespace rg

namespace {
struct PairsPrepLaunchF {
    PairsArgs *a, *prep;
    int2 *prep_out;
    int64_t prep_blocks;
    hipStream_t s;
    template <class L>
    int operator()() {
        const int64_t nb = pairs_blocks<L>(a->cols);
        const dim3 grid((unsigned)(nb + prep_blocks));
        if (a->n_neg <= 5)
            hipLaunchKernelGGL((mf_pairs_prep_kernel<L, 5>), grid, dim3(kPairBlock), 0, s, *a, *prep, prep_out, nb);
        else
            hipLaunchKernelGGL((mf_pairs_prep_kernel<L, kNMax>), grid, dim3(kPairBlock), 0, s, *a, *prep, prep_out, nb);
        return check_launch("rg_mf_pairs_prepare");
    }
};

struct FlushLaunchF {
    ApplyArgs *a;
    hipStream_t s;
    template <class L>
    int operator()() {
        const int64_t waves = (a->num_users + L::UPW - 1) / L::UPW;
        const int64_t nb = (waves + kBlock / kWave - 1) / (kBlock / kWave);
        hipLaunchKernelGGL((mf_lazy_flush_kernel<L>), dim3(nb < 1 ? 1 : nb), dim3(kBlock), 0, s, *a);
        return check_launch("rg_mf_lazy_flush");
    }
};

int lazy_args(const rg_mf_lazy_t *lz, const rg_opt_t *opt, ApplyArgs &a) {
    if (!lz || !lz->last_rel) return fail_arg("lazy dense pass: null rg_mf_lazy_t / last_rel");
    if (lz->step < 1 || lz->base < 0 || lz->base > lz->step || lz->step >= ((int64_t)1 << 31))
        return fail_arg("lazy dense pass: bad step / base");
    if (opt && opt->kind == RG_OPT_ADAM && (!lz->step_consts || lz->n_consts <= lz->step))
        return fail_arg("lazy dense pass: Adam needs the per-step constants up to this step");
    a.last_rel = lz->last_rel;
    a.umark = lz->umark;
    a.step_consts = reinterpret_cast<const float2 *>(lz->step_consts);
    a.lazy_base = lz->base;
    a.lazy_t = (int32_t)lz->step;
    a.lazy_full = lz->full;
    a.lazy_rows = reinterpret_cast<unsigned long long *>(lz->rows_done);
#if RG_AB
    static const int dbg = [] { const char *e = getenv("RG_LAZY_DBG"); return e ? atoi(e) : 0; }();
    static const int cap = [] { const char *e = getenv("RG_LAZY_CAP"); return e ? atoi(e) : 0; }();
    a.lazy_dbg = dbg;
    a.lazy_cap = cap;
#else
    a.lazy_dbg = 0;
    a.lazy_cap = 0;
#endif
    return RG_OK;
}
}  // namespace

extern "C" int rg_mf_pairs_prepare(void *stream, const rg_mf_tables_t *t, const rg_mf_batch_t *b, rg_mf_work_t *w,
                                   const rg_mf_batch_t *next, const rg_mf_work_t *next_w, int32_t *umark,
                                   int32_t umark_step) {
    if (!next) return rg_mf_pairs(stream, t, b, w, 1);
    PairsArgs prep{};
    int rc = prepare_args(next, next_w, nullptr, prep);
    if (rc) return rc;
    prep.umark = umark;
    prep.umark_step = umark_step;
    prep.num_users = t ? t->num_users : 0;
    const int64_t total = prepare_threads(next->cols, next->n_neg);
    if (b && b->loss == RG_LOSS_ADAPTIVE_HINGE) {   // several launches: the global max first
        if ((rc = rg_mf_pairs(stream, t, b, w, 1))) return rc;
        return launch_prepare(stream, prep, reinterpret_cast<int2 *>(next->pairs), total, 0,
                              "rg_mf_pairs_prepare(prepare)");
    }
    if (kPairBlock != kBlock) return fail_arg("rg_mf_pairs_prepare: built with a pair-pass workgroup != 256 threads");
    PairsArgs a;
    if ((rc = pairs_args(t, b, w, 1, a))) return rc;
    PairsPrepLaunchF f{&a, &prep, reinterpret_cast<int2 *>(next->pairs), (total + kBlock - 1) / kBlock,
                       (hipStream_t)stream};
    return dispatch_dim(t->dim, f);
}

extern "C" int rg_mf_apply_lazy(void *stream, const rg_mf_tables_t *t, rg_mf_work_t *w, const rg_opt_t *opt,
                                const rg_mf_loss_t *loss, const rg_mf_lazy_t *lazy, const rg_mt_gen_t *gen) {
    MtGenArgs g{};
    if (gen && gen->nwords > 0) {
        if (!gen->state || !gen->out) return fail_arg("rg_mf_apply_lazy: null MT state / output");
        g.state = gen->state; g.out = gen->out; g.state_before = gen->state_before; g.nwords = gen->nwords;
    }
    ApplyArgs a;
    int rc = apply_args(t, w, nullptr, nullptr, opt, 0, -1, loss, nullptr, kApplyPull, a);
    if (rc) return rc;
    if ((rc = lazy_args(lazy, opt, a))) return rc;
    if (!lazy->full && !lazy->umark) return fail_arg("rg_mf_apply_lazy: a partial pass needs the user marks");
    return launch_back_lazy(stream, t->dim, a, g);
}

extern "C" int rg_mf_lazy_flush(void *stream, const rg_mf_tables_t *t, const rg_opt_t *opt, const rg_mf_lazy_t *lazy) {
    int rc = check_tables(t);
    if (rc) return rc;
    if (!opt || opt->kind < RG_OPT_ADAM || opt->kind > RG_OPT_RMSPROP) return fail_arg("rg_mf_lazy_flush: bad opt");
    if (!t->user_w_out || !t->user_b_out) return fail_arg("rg_mf_lazy_flush: null other-set user tables");
    ApplyArgs a{};
    a.w_in[0] = t->user_w; a.b_in[0] = t->user_b; a.w_out[0] = t->user_w_out; a.b_out[0] = t->user_b_out;
    a.w_m[0] = t->user_w_m; a.w_v[0] = t->user_w_v; a.b_m[0] = t->user_b_m; a.b_v[0] = t->user_b_v;
    if (opt->kind == RG_OPT_ADAM && (!a.w_m[0] || !a.b_m[0])) return fail_arg("rg_mf_lazy_flush: Adam needs m");
    if (opt->kind != RG_OPT_SGD && (!a.w_v[0] || !a.b_v[0])) return fail_arg("rg_mf_lazy_flush: needs v");
    a.num_users = t->num_users; a.num_items = t->num_items; a.dim = t->dim;
    a.opt = *opt;
    a.has_bias = true;
    if ((rc = lazy_args(lazy, opt, a))) return rc;
    FlushLaunchF f{&a, (hipStream_t)stream};
    return dispatch_dim(t->dim, f);
}
