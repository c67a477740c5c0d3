// The MF stepper's whole-step alternatives (host code, no kernels): the steps that measured
// slower than rg_stepper.cpp's split step and are selected only by switches of the A/B build
// (ab_flag: constant off in the product library), with their buffers and the
// C entries that only serve them.
//
//   lazy split step (RG_LAZY)        train_lazy, lazy_flush; rg_mf_stepper_flush / _lazy_count
//   pipelined step (RG_PIPE)         train_pipe, pipe_abandon; rg_mf_stepper_pipelined / _pipe_error
//   two-launch pipelined (RG_PIPE2)  train_pipe2 (the same per-unit scratch as RG_PIPE)
//   overlapped step (RG_FUSED)       train_fused (pointwise / bpr / hinge):
//       rg_mf_step_front(pairs of t | marked prepare of t+1 | cold-row update of t)
//       -> rg_mf_step_hot(touched rows of t, loss): two launches per step on one stream, the row
//       stamps (two arrays, owned here) telling touched rows from cold ones
//
// rg_stepper.cpp dispatches to train_* in rg_mf_stepper_train[_ahead], calls alt_create /
// alt_destroy from create / destroy, and lazy_flush / pipe_abandon before an external consumer
// takes a unit; the kernels behind these steps are in rg_mf_alt.hip.
#include <algorithm>
#include <cstdlib>

#include "rg_stepper.h"

#pragma GCC visibility push(hidden)
namespace rg {
namespace stepper {

// ---------------------------------------------------------------- lazy split step
// Adam constants of every absolute step < upto on the device (grown by doubling; the
// copy is synchronous and happens O(log steps) times in a run)
int ensure_consts(Stepper &st, int64_t upto) {
    if (upto < st.n_consts) return RG_OK;
    int64_t cap = st.n_consts > 0 ? st.n_consts : 4096;
    while (cap <= upto) cap *= 2;
    float *host = static_cast<float *>(std::malloc((size_t)cap * 2 * sizeof(float)));
    if (!host) { rg::set_error("stepper: out of host memory"); return RG_E_LAUNCH; }
    for (int64_t s = 0; s < cap; ++s) {
        const rg_opt_t o = opt_at(st, s > 0 ? s : 1);
        host[2 * s] = o.step_size;
        host[2 * s + 1] = o.bias_correction2_sqrt;
    }
    float *dev = nullptr;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMalloc(&dev, (size_t)cap * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dev, host, (size_t)cap * 2 * sizeof(float), hipMemcpyHostToDevice);
    std::free(host);
    if (e != hipSuccess) return hip_fail("stepper: step constants", e);
    if (st.consts) (void)hipFree(st.consts);
    st.consts = dev;
    st.n_consts = cap;
    return RG_OK;
}

rg_mf_lazy_t lazy_of(const Stepper &st, int64_t step, bool full) {
    rg_mf_lazy_t l{};
    l.last_rel = st.last_rel;
    l.umark = st.umark;
    l.step_consts = st.consts;
    l.n_consts = st.n_consts;
    l.base = st.lazy_base;
    l.step = step;
    l.full = full ? 1 : 0;
    l.rows_done = st.count_rows ? st.rows_done : nullptr;
    return l;
}

// every user row up to the current step, into the current set (no-op when none lags)
int lazy_flush(Stepper &st, hipStream_t s) {
    if (!st.lazy || !st.lazy_pending) return RG_OK;
    int rc = ensure_consts(st, st.cfg.step + 1);
    if (rc) return rc;
    const rg_opt_t o = opt_at(st, st.cfg.step > 0 ? st.cfg.step : 1);
    const rg_mf_lazy_t l = lazy_of(st, st.cfg.step, true);
    if ((rc = rg_mf_lazy_flush(s, &st.cfg.tables[st.set], &o, &l))) return rc;
    st.lazy_pending = false;
    return RG_OK;
}

// Lazy split step (single rank):
//   main  rg_mf_pairs_prepare (this step's pairs + the NEXT step's prepare, which marks the
//         users that step reads) -> rg_mf_apply_lazy (items, and the users with a gradient
//         or a mark; a full pass when no next step is known; + the inline MT walk)
// Every row a kernel reads is current; rows nobody reads lag until rg_mf_stepper_flush /
// the next full pass / an external consumer (acquire) catches them up.
int train_lazy(Stepper &st, hipStream_t s, const rg_mf_step_in_t &cur, const rg_mf_step_in_t *next,
               float *loss_out, void *ev0, void *ev1) {
    const int64_t unit = st.taken;
    int rc = st.inline_gen ? generate_upto(st, unit + 1, 0) : keep_ahead(st, unit);
    if (rc) return rc;
    rg_mf_work_t w = work_for(st, cur);
    const rg_mf_batch_t batch = make_batch(st, cur, unit);
    if ((rc = wait_side(st, s, (int)(unit % 2)))) return rc;
    if (!(st.prepared && st.prep_unit == unit && same_input(st.prep_in, cur))) {
        // the pairs were not prepared (with marks) by the previous lazy step: bring every row
        // up to date first, so whatever this step reads is current
        if ((rc = lazy_flush(st, s))) return rc;
        if ((rc = wait_words(st, s, unit))) return rc;
        if ((rc = rg_mf_prepare(s, &batch, &w))) return rc;
        st.prepared = true;
        st.prep_unit = unit;
        st.prep_in = cur;
        st.prep_serial = 0;
    }
    if (!st.lazy_pending) {                    // every row current at cfg.step: restart the clock
        hipError_t e = hipMemsetAsync(st.last_rel, 0, (size_t)st.cfg.tables[0].num_users * sizeof(int32_t), s);
        if (e != hipSuccess) return hip_fail("stepper: reset last_rel", e);
        st.lazy_base = st.cfg.step;
    }
    if (st.cfg.loss == RG_LOSS_ADAPTIVE_HINGE && (rc = wait_words(st, s, unit))) return rc;
    const int64_t t = st.cfg.step + 1;
    if ((rc = ensure_consts(st, t + 1))) return rc;
    rg_mf_batch_t nbatch{};
    rg_mf_work_t nw{};
    if (next) {
        // only the slot holding unit + 1: this unit is not released yet, and keeping two
        // slots ahead of unit + 1 could overwrite its words under the adaptive-max kernel
        // (release() below keeps the ring ahead once the pair pass is enqueued)
        if (!st.inline_gen && (rc = generate_upto(st, unit + 1, 0))) return rc;
        if ((rc = wait_side(st, s, (int)((unit + 1) % 2)))) return rc;
        if ((rc = wait_words(st, s, unit + 1))) return rc;
        nbatch = make_batch(st, *next, unit + 1);
        nw = work_for(st, *next);
    }
    const rg_mf_tables_t *tb = &st.cfg.tables[st.set];
    if ((rc = rg_mf_pairs_prepare(s, tb, &batch, &w, next ? &nbatch : nullptr, next ? &nw : nullptr, st.umark,
                                  (int32_t)(t + 1))))
        return rc;
    if ((rc = release(st, s))) return rc;
    rg_mt_gen_t gen{};
    int gen_slot = -1;
    if (st.inline_gen && st.gen_slots == rel_slot(st, unit + 2)) {
        gen_slot = (int)(st.gen_slots % kSlots);
        if ((rc = begin_production(st, s, gen_slot))) return rc;
        gen.state = st.cfg.mt_state;
        gen.out = st.words[gen_slot];
        gen.state_before = st.start_state[gen_slot];
        gen.nwords = st.G * st.W;
    }
    st.cfg.step = t;
    const rg_opt_t o = opt_at(st, t);
    const rg_mf_loss_t l = loss_of(st, cur.global_pos, loss_out);
    const rg_mf_lazy_t lz = lazy_of(st, t, next == nullptr);
    rg::launch_events() = rg::LaunchEvents{(hipEvent_t)ev0, (hipEvent_t)ev1};
    rc = rg_mf_apply_lazy(s, tb, &w, &o, &l, &lz, gen_slot >= 0 ? &gen : nullptr);
    rg::launch_events() = rg::LaunchEvents{};
    if (rc) return rc;
    if (gen_slot >= 0) end_production(st, s, gen_slot);
    if (next) {
        st.prepared = true;
        st.prep_unit = unit + 1;
        st.prep_in = *next;
        st.prep_serial = 0;
    }
    st.lazy_pending = next != nullptr;
    st.set = 1 - st.set;
    return RG_OK;
}

// ---------------------------------------------------------------- pipelined step
rg_mf_work_t pipe_work(const Stepper &st, const rg_mf_step_in_t &in, int64_t unit) {
    rg_mf_work_t w = work_for(st, in);
    w.row_count = st.pcounts[unit % 3];
    w.claim_num_users = st.cfg.tables[0].num_users;
    if (unit % 2) {
        w.row_list = st.p_list1;
        w.hot_grad = st.p_hg1;
        w.hot_bias_grad = st.p_hbg1;
        w.loss_partials = st.p_part1;
        w.part_row = st.p_prow1;
        w.part_bias = st.p_pbias1;
    }
    return w;
}

int pipe_memset(void *p, size_t bytes, hipStream_t s, const char *what) {
    hipError_t e = hipMemsetAsync(p, 0, bytes, s);
    return e == hipSuccess ? RG_OK : hip_fail(what, e);
}

int pipe_clean_counts(Stepper &st, hipStream_t s, int k) {
    if (!st.pdirty[k]) return RG_OK;
    const rg_mf_tables_t &t = st.cfg.tables[0];
    int rc = pipe_memset(st.pcounts[k], (size_t)(t.num_users + t.num_items) * sizeof(int32_t), s,
                         "stepper: reset claims");
    if (rc == RG_OK) st.pdirty[k] = false;
    return rc;
}

// the overflow accumulators of set k after a pair pass whose dense pass never ran
int pipe_clean_accum(Stepper &st, hipStream_t s, int k) {
    if (!st.pair_dirty[k]) return RG_OK;
    const rg_mf_tables_t &t = st.cfg.tables[0];
    const int64_t rows = t.num_users + t.num_items;
    int64_t *hg = k ? st.p_hg1 : reinterpret_cast<int64_t *>(st.cfg.work.hot_grad);
    int64_t *hb = k ? st.p_hbg1 : reinterpret_cast<int64_t *>(st.cfg.work.hot_bias_grad);
    int rc = pipe_memset(hg, (size_t)rows * t.dim * sizeof(int64_t), s, "stepper: reset overflow");
    if (rc == RG_OK) rc = pipe_memset(hb, (size_t)rows * sizeof(int64_t), s, "stepper: reset overflow");
    if (rc == RG_OK) st.pair_dirty[k] = false;
    return rc;
}

// drop every pipelined unit not trained yet (a pair pass and / or a prepare ahead): their
// claims and overflow adds are cleared; their words stay (input independent)
int pipe_abandon(Stepper &st, hipStream_t s) {
    if (!st.pipe && !st.pipe2) return RG_OK;
    int rc = RG_OK;
    for (int k = 0; k < 3 && rc == RG_OK; ++k) rc = pipe_clean_counts(st, s, k);
    for (int k = 0; k < 2 && rc == RG_OK; ++k) rc = pipe_clean_accum(st, s, k);
    st.paired = -1;
    st.hot_prepped = -1;
    st.last_pipe = -1;
    st.prepared = false;
    st.count_dirty[0] = st.count_dirty[1] = false;
    return rc;
}

// Pipelined step of unit t = taken (see rg_mf_pipe_step).  Cold start (no pair pass of t
// pending): prepare t (claims), pair pass t, prepare t+1 with its hot list, each its own launch;
// then, while `next` is known, one launch per step.  Without `next` the step is the plain dense
// pass and the pipeline drains.
int train_pipe(Stepper &st, hipStream_t s, const rg_mf_step_in_t &cur, const rg_mf_step_in_t *next,
               const rg_mf_step_in_t *next2, float *loss_out, void *ev0, void *ev1) {
    const int64_t unit = st.taken;
    int rc = generate_upto(st, unit + (next2 ? 2 : next ? 1 : 0), 0);
    if (rc) return rc;
    const rg_mf_tables_t *tb = &st.cfg.tables[st.set];
    const rg_mf_tables_t &t0 = st.cfg.tables[0];
    rg_mf_work_t w = pipe_work(st, cur, unit);
    const rg_mf_batch_t batch = make_batch(st, cur, unit);
    if (!(st.paired == unit && same_input(st.paired_in, cur))) {
        // cold start: whatever ran ahead belongs to another input
        if ((rc = pipe_abandon(st, s))) return rc;
        if ((rc = wait_side(st, s, (int)(unit % 2))) || (rc = wait_words(st, s, unit))) return rc;
        if ((rc = rg_mf_prepare(s, &batch, &w))) return rc;
        st.pdirty[unit % 3] = true;
        if ((rc = rg_mf_pairs(s, tb, &batch, &w, 1))) return rc;
        st.pair_dirty[unit % 2] = true;
        st.paired = unit;
        st.paired_in = cur;
    }
    st.cfg.step += 1;
    const rg_opt_t o = opt_at(st, st.cfg.step);
    const rg_mf_loss_t l = loss_of(st, cur.global_pos, loss_out);
    if (!next) {                       // the last step of a sequence: dense pass only
        if ((rc = release(st, s))) return rc;
        rg::launch_events() = rg::LaunchEvents{(hipEvent_t)ev0, (hipEvent_t)ev1};
        rc = rg_mf_apply_prepare_gen(s, tb, &w, &o, 0, t0.num_users + t0.num_items, &l, nullptr, nullptr, nullptr);
        rg::launch_events() = rg::LaunchEvents{};
        if (rc) return rc;
        st.pdirty[unit % 3] = false;
        st.pair_dirty[unit % 2] = false;
        st.paired = -1;
        st.last_pipe = -1;
        st.set = 1 - st.set;
        return RG_OK;
    }
    // step t+1: prepared with claims and its hot list (done by the previous launch, or now)
    const int64_t u1 = unit + 1, u2 = unit + 2;
    rg_mf_work_t w1 = pipe_work(st, *next, u1);
    const rg_mf_batch_t b1 = make_batch(st, *next, u1);
    int32_t *nhot = st.pint, *gate = st.pint + 3, *err = st.pint + 5;
    if (!(st.hot_prepped == u1 && same_input(st.hot_in, *next))) {
        if ((rc = pipe_clean_counts(st, s, (int)(u1 % 3)))) return rc;
        if ((rc = pipe_clean_accum(st, s, (int)(u1 % 2)))) return rc;
        if ((rc = wait_side(st, s, (int)(u1 % 2))) || (rc = wait_words(st, s, u1))) return rc;
        if ((rc = pipe_memset(nhot + u1 % 3, sizeof(int32_t), s, "stepper: hot list"))) return rc;
        if ((rc = rg_mf_prepare_hot(s, &b1, &w1, st.hot[u1 % 3], nhot + u1 % 3))) return rc;
        st.pdirty[u1 % 3] = true;
        st.hot_prepped = u1;
        st.hot_in = *next;
    }
    if (st.last_pipe != unit - 1) {    // counters a previous launch of the sequence would have reset
        if ((rc = pipe_memset(gate + unit % 2, sizeof(int32_t), s, "stepper: gate")) ||
            (rc = pipe_memset(nhot + u2 % 3, sizeof(int32_t), s, "stepper: hot list")))
            return rc;
    }
    rg_mf_batch_t b2{};
    rg_mf_work_t w2{};
    if (next2) {
        if ((rc = pipe_clean_counts(st, s, (int)(u2 % 3)))) return rc;
        if ((rc = wait_side(st, s, (int)(u2 % 2))) || (rc = wait_words(st, s, u2))) return rc;
        b2 = make_batch(st, *next2, u2);
        w2 = pipe_work(st, *next2, u2);
    }
    if ((rc = pipe_clean_accum(st, s, (int)(u1 % 2)))) return rc;   // set u1 % 2 is the pair pass's
    if ((rc = release(st, s))) return rc;
    rg_mt_gen_t gen{};
    int gen_slot = -1;
    if (st.inline_gen && st.gen_slots == rel_slot(st, unit + 3)) {
        gen_slot = (int)(st.gen_slots % kSlots);
        if ((rc = begin_production(st, s, gen_slot))) return rc;
        gen.state = st.cfg.mt_state;
        gen.out = st.words[gen_slot];
        gen.state_before = st.start_state[gen_slot];
        gen.nwords = st.G * st.W;
    }
    rg_mf_pipe_t pp{};
    pp.hot_users = st.hot[u1 % 3];
    pp.nhot = nhot + u1 % 3;
    pp.counts_next = st.pcounts[u1 % 3];
    pp.gate = gate + unit % 2;
    pp.gate_next = gate + u1 % 2;
    pp.nhot_free = nhot + unit % 3;
    pp.hot_out = next2 ? st.hot[u2 % 3] : nullptr;
    pp.nhot_out = next2 ? nhot + u2 % 3 : nullptr;
    pp.err = err;
    rg::launch_events() = rg::LaunchEvents{(hipEvent_t)ev0, (hipEvent_t)ev1};
    rc = rg_mf_pipe_step(s, tb, &w, &o, &l, &b1, &w1, next2 ? &b2 : nullptr, next2 ? &w2 : nullptr, &pp,
                         gen_slot >= 0 ? &gen : nullptr);
    rg::launch_events() = rg::LaunchEvents{};
    if (rc) return rc;
    if (gen_slot >= 0) end_production(st, s, gen_slot);
    st.pdirty[unit % 3] = false;                 // the dense pass consumed and reset its claims
    st.pair_dirty[unit % 2] = false;             // and its overflow accumulators
    st.pair_dirty[u1 % 2] = true;
    st.paired = u1;
    st.paired_in = *next;
    if (next2) {
        st.pdirty[u2 % 3] = true;
        st.hot_prepped = u2;
        st.hot_in = *next2;
    } else {
        st.hot_prepped = -1;
    }
    st.last_pipe = unit;
    st.set = 1 - st.set;
    return RG_OK;
}

// Two-launch pipelined step of unit t = taken (rg_mf_pipe2_hot / rg_mf_pipe2_cold):
//   hot  (t): step t's dense update of every item row and of the users step t+1's pair pass reads
//   cold (t): step t+1's pair pass | the MT walk | step t+2's prepare | step t's dense update of
//             every other user
// Preconditions carried from the previous call: step t's pair pass ran (its lists), step t+1 was
// prepared with claims and its hot list.  A cold start (nothing pending, or pending for another
// input) runs prepare t, pair pass t and prepare t+1 as launches of their own; without `next` the
// step is the plain dense pass and the pipeline drains; without `next2` the cold launch prepares
// nothing ahead (the next call prepares its t+1 on its own).
int train_pipe2(Stepper &st, hipStream_t s, const rg_mf_step_in_t &cur, const rg_mf_step_in_t *next,
                const rg_mf_step_in_t *next2, float *loss_out, void *ev0, void *ev1) {
    const int64_t unit = st.taken;
    int rc = st.inline_gen ? generate_upto(st, unit + (next2 ? 2 : next ? 1 : 0), 0) : keep_ahead(st, unit);
    if (rc) return rc;
    const rg_mf_tables_t *tb = &st.cfg.tables[st.set];
    const rg_mf_tables_t &t0 = st.cfg.tables[0];
    rg_mf_work_t w = pipe_work(st, cur, unit);
    const rg_mf_batch_t batch = make_batch(st, cur, unit);
    if (!(st.paired == unit && same_input(st.paired_in, cur))) {
        // cold start: whatever ran ahead belongs to another input
        if ((rc = pipe_abandon(st, s))) return rc;
        if ((rc = wait_side(st, s, (int)(unit % 2))) || (rc = wait_words(st, s, unit))) return rc;
        if ((rc = rg_mf_prepare(s, &batch, &w))) return rc;
        st.pdirty[unit % 3] = true;
        if ((rc = rg_mf_pairs(s, tb, &batch, &w, 1))) return rc;
        st.pair_dirty[unit % 2] = true;
        st.paired = unit;
        st.paired_in = cur;
    }
    st.cfg.step += 1;
    const rg_opt_t o = opt_at(st, st.cfg.step);
    const rg_mf_loss_t l = loss_of(st, cur.global_pos, loss_out);
    const int64_t U = t0.num_users, R = U + t0.num_items;
    if (!next) {                       // the last step of a sequence: dense pass only
        if ((rc = release(st, s))) return rc;
        rg::launch_events() = rg::LaunchEvents{(hipEvent_t)ev0, (hipEvent_t)ev1};
        rc = rg_mf_apply_prepare_gen(s, tb, &w, &o, 0, R, &l, nullptr, nullptr, nullptr);
        rg::launch_events() = rg::LaunchEvents{};
        if (rc) return rc;
        st.pdirty[unit % 3] = false;
        st.pair_dirty[unit % 2] = false;
        st.paired = -1;
        st.hot_prepped = -1;
        st.set = 1 - st.set;
        return RG_OK;
    }
    const int64_t u1 = unit + 1, u2 = unit + 2;
    rg_mf_work_t w1 = pipe_work(st, *next, u1);
    const rg_mf_batch_t b1 = make_batch(st, *next, u1);
    int32_t *nhot = st.pint;
    if (!(st.hot_prepped == u1 && same_input(st.hot_in, *next))) {
        if ((rc = pipe_clean_counts(st, s, (int)(u1 % 3)))) return rc;
        if ((rc = pipe_clean_accum(st, s, (int)(u1 % 2)))) return rc;
        if ((rc = wait_side(st, s, (int)(u1 % 2))) || (rc = wait_words(st, s, u1))) return rc;
        if ((rc = pipe_memset(nhot + u1 % 3, sizeof(int32_t), s, "stepper: hot list"))) return rc;
        if ((rc = rg_mf_prepare_hot(s, &b1, &w1, st.hot[u1 % 3], nhot + u1 % 3))) return rc;
        st.pdirty[u1 % 3] = true;
        st.hot_prepped = u1;
        st.hot_in = *next;
    }
    rg_mf_batch_t b2{};
    rg_mf_work_t w2{};
    if (next2) {
        if ((rc = pipe_clean_counts(st, s, (int)(u2 % 3)))) return rc;
        if ((rc = wait_side(st, s, (int)(u2 % 2))) || (rc = wait_words(st, s, u2))) return rc;
        b2 = make_batch(st, *next2, u2);
        w2 = pipe_work(st, *next2, u2);
    }
    if ((rc = pipe_clean_accum(st, s, (int)(u1 % 2)))) return rc;   // set u1 % 2 is the pair pass's
    if ((rc = release(st, s))) return rc;
    rg_mt_gen_t gen{};
    int gen_slot = -1;
    if (st.inline_gen && st.gen_slots == rel_slot(st, unit + 3)) {
        gen_slot = (int)(st.gen_slots % kSlots);
        if ((rc = begin_production(st, s, gen_slot))) return rc;
        gen.state = st.cfg.mt_state;
        gen.out = st.words[gen_slot];
        gen.state_before = st.start_state[gen_slot];
        gen.nwords = st.G * st.W;
    }
    const int64_t hot_cap = std::min<int64_t>(U, (int64_t)(1 + st.cfg.n_neg) * st.cfg.cols);
    if ((rc = rg_mf_pipe2_hot(s, tb, &w, &o, &l, st.hot[u1 % 3], nhot + u1 % 3, hot_cap,
                              next2 ? nhot + u2 % 3 : nullptr, nullptr))) {
        st.cfg.step -= 1;                          // nothing of this step ran
        return rc;
    }
    rg::launch_events() = rg::LaunchEvents{(hipEvent_t)ev0, (hipEvent_t)ev1};   // the cold launch
    rc = rg_mf_pipe2_cold(s, tb, &w, &o, &b1, &w1, st.pcounts[u1 % 3], next2 ? &b2 : nullptr,
                          next2 ? &w2 : nullptr, next2 ? st.hot[u2 % 3] : nullptr, next2 ? nhot + u2 % 3 : nullptr,
                          gen_slot >= 0 ? &gen : nullptr);
    rg::launch_events() = rg::LaunchEvents{};
    if (rc) {
        // the hot launch updated part of the rows: the step is half applied and cannot be resumed
        st.failed = true;
        return rc;
    }
    if (gen_slot >= 0) end_production(st, s, gen_slot);
    st.pdirty[unit % 3] = false;                 // the two launches consumed and reset its claims
    st.pair_dirty[unit % 2] = false;             // and its overflow accumulators
    st.pair_dirty[u1 % 2] = true;
    st.paired = u1;
    st.paired_in = *next;
    if (next2) {
        st.pdirty[u2 % 3] = true;
        st.hot_prepped = u2;
        st.hot_in = *next2;
    } else {
        st.hot_prepped = -1;
    }
    st.set = 1 - st.set;
    return RG_OK;
}

// ---------------------------------------------------------------- overlapped step
int ensure_stamps(Stepper &st) {
    if (st.stamp[0]) return RG_OK;
    const rg_mf_tables_t &t = st.cfg.tables[0];
    const size_t bytes = (size_t)(t.num_users + t.num_items) * sizeof(int32_t);
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = hipMalloc(&st.stamp[k], bytes);
        if (e == hipSuccess) e = hipMemset(st.stamp[k], 0, bytes);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? RG_OK : hip_fail("stepper: stamps", e);
}

rg_mf_mark_t mark_of(const Stepper &st, int arr, int32_t serial) {
    rg_mf_mark_t m{};
    m.stamp = st.stamp[arr];
    m.num_users = st.cfg.tables[0].num_users;
    m.serial = serial;
    return m;
}

int32_t next_serial(Stepper &st) {
    st.serial = st.serial == 0x7fffffff ? 1 : st.serial + 1;
    return st.serial;
}

// the touched rows of the hot pass: a stamp scan (RG_HOT_SCAN=1, default) or the owner flags
const rg_mf_mark_t *hot_mark(const Stepper &st, const rg_mf_mark_t &m) { return st.hot_scan ? &m : nullptr; }

int train_fused(Stepper &st, hipStream_t s, const rg_mf_step_in_t &cur, const rg_mf_step_in_t *next,
                float *loss_out, void *ev0, void *ev1) {
    int rc = ensure_stamps(st);
    if (rc) return rc;
    const int64_t unit = st.taken;
    if ((rc = keep_ahead(st, unit))) return rc;
    rg_mf_work_t w = work_for(st, cur);
    const rg_mf_batch_t batch = make_batch(st, cur, unit);
    if (!(st.prepared && st.prep_unit == unit && st.prep_serial != 0 && same_input(st.prep_in, cur))) {
        // first step, or the prefetched pairs were for another input: marked prepare here
        if ((rc = wait_side(st, s, (int)(unit % 2)))) return rc;
        if ((rc = wait_words(st, s, unit))) return rc;
        st.prep_arr = 1 - st.prep_arr;
        st.prep_serial = next_serial(st);
        const rg_mf_mark_t m = mark_of(st, st.prep_arr, st.prep_serial);
        if ((rc = rg_mf_prepare_marked(s, &batch, &w, &m))) return rc;
        st.prepared = true;
        st.prep_unit = unit;
        st.prep_in = cur;
    }
    const rg_mf_mark_t cur_mark = mark_of(st, st.prep_arr, st.prep_serial);
    const rg_mf_tables_t *tb = &st.cfg.tables[st.set];
    const int64_t U = tb->num_users, R = tb->num_users + tb->num_items;
    const int64_t cold_end = st.cfg.item_grad ? U : R;    // DP: items go through the exchange
    st.cfg.step += 1;
    const rg_opt_t o = opt_at(st, st.cfg.step);
    const rg_mf_loss_t l = loss_of(st, cur.global_pos, loss_out);

    rg_mf_batch_t nbatch{};
    rg_mf_work_t nw{};
    rg_mf_mark_t nmark{};
    const int narr = 1 - st.prep_arr;
    if (next) {
        if ((rc = keep_ahead(st, unit + 1))) return rc;
        if ((rc = wait_side(st, s, (int)((unit + 1) % 2)))) return rc;
        if ((rc = wait_words(st, s, unit + 1))) return rc;
        nbatch = make_batch(st, *next, unit + 1);
        nw = work_for(st, *next);
        nmark = mark_of(st, narr, next_serial(st));
    }
    if ((rc = record(ev0, s))) return rc;
    if ((rc = rg_mf_step_front(s, tb, &batch, &w, &cur_mark, &o, 0, cold_end, next ? &nbatch : nullptr,
                               next ? &nw : nullptr, next ? &nmark : nullptr)))
        return rc;
    if ((rc = release(st, s))) return rc;               // clears `prepared` for this unit
    if (next) {
        st.prepared = true;
        st.prep_unit = unit + 1;
        st.prep_in = *next;
        st.prep_serial = nmark.serial;
        st.prep_arr = narr;
    }
    if (st.cfg.item_grad) {
        if ((rc = rg_mf_grads(s, tb, &w, st.cfg.item_grad, U, R, &l))) return rc;
        if (st.cfg.comm && (rc = rg::comm_begin(st.cfg.comm, s, st.cfg.item_grad,
                                                tb->num_items * (int64_t)(tb->dim + 1) + 1)))
            return rc;
        if ((rc = rg_mf_step_hot(s, tb, &batch, &w, hot_mark(st, cur_mark), &o, 0, U, nullptr))) return rc;
        if ((rc = record(ev1, s))) return rc;
        if (st.cfg.comm && (rc = rg::comm_end(st.cfg.comm, s))) return rc;
        if ((rc = rg_mf_apply_dense(s, tb, st.cfg.item_grad, &o, U, R, loss_out))) return rc;
    } else {
        if ((rc = rg_mf_step_hot(s, tb, &batch, &w, hot_mark(st, cur_mark), &o, 0, R, &l))) return rc;
        if ((rc = record(ev1, s))) return rc;
    }
    st.set = 1 - st.set;
    return RG_OK;
}

// ---------------------------------------------------------------- buffers
int alt_create(Stepper &st) {
    const rg_mf_stepper_config_t *cfg = &st.cfg;
    hipError_t e = hipSuccess;
    if (st.lazy) {
        const size_t ub = (size_t)cfg->tables[0].num_users * sizeof(int32_t);
        e = hipMalloc(&st.last_rel, ub);
        if (e == hipSuccess) e = hipMalloc(&st.umark, ub);
        if (e == hipSuccess) e = hipMemset(st.umark, 0, ub);
        if (e == hipSuccess) e = hipMemset(st.last_rel, 0, ub);
        if (e == hipSuccess) e = hipMalloc(&st.rows_done, sizeof(uint64_t));
        if (e == hipSuccess) e = hipMemset(st.rows_done, 0, sizeof(uint64_t));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_fail("rg_mf_stepper_create: lazy state", e);
        st.lazy_base = cfg->step;
    }
    const rg_mf_tables_t &t0 = cfg->tables[0];
    // pipelined step (rg_mf_pipe_step): single rank, claimed slots, pointwise / bpr / hinge, a
    // float4 row layout of >= 8 lanes (dim a multiple of 4, 32..256)
    st.pipe = ab_flag("RG_PIPE", false) && st.claim && cfg->dp_mode == 0 && !st.prep_in_pairs &&
               (cfg->loss == RG_LOSS_POINTWISE || cfg->loss == RG_LOSS_BPR || cfg->loss == RG_LOSS_HINGE) &&
               t0.dim % 4 == 0 && t0.dim >= 32 && t0.dim <= 256 && cfg->work.part_row && cfg->work.part_bias &&
               cfg->work.loss_partials && cfg->n_partials > 0;
    if (st.pipe) {
        // the pair workgroups wait inside the launch: keep them at most half of what the chip
        // holds (>= 4 workgroups per CU at the launch's register count), so the rows they wait
        // for always have room to run whatever the dispatch order
        const int64_t upb = rg_mf_plan_units_per_block(t0.dim);
        st.pipe = upb > 0 && (cfg->cols + upb - 1) / upb <= 2 * (int64_t)rg::num_cus() &&
                   std::max(t0.num_users, t0.num_items) * (int64_t)t0.dim * 4 < ((int64_t)1 << 31);
    }
    // two-launch pipelined step (rg_mf_pipe2_hot / _cold) for the single-rank losses with claimed
    // slots: RG_PIPE2=1 selects it; the default is the split step, which measures faster
    st.pipe2 = !st.pipe && ab_flag("RG_PIPE2", false) && st.claim && cfg->dp_mode == 0 && !st.prep_in_pairs &&
                (cfg->loss == RG_LOSS_POINTWISE || cfg->loss == RG_LOSS_BPR || cfg->loss == RG_LOSS_HINGE) &&
                cfg->work.part_row && cfg->work.part_bias && cfg->work.loss_partials && cfg->n_partials > 0;
    if (st.pipe || st.pipe2) {
        const int64_t rows = t0.num_users + t0.num_items;
        const int64_t hot_len = std::min<int64_t>(t0.num_users, (int64_t)(1 + cfg->n_neg) * cfg->cols);
        e = hipMalloc(&st.p_counts2, (size_t)rows * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemset(st.p_counts2, 0, (size_t)rows * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc(&st.p_list1, (size_t)rows * RG_MF_LIST_CAP * 2 * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc(&st.p_hg1, (size_t)rows * t0.dim * sizeof(int64_t));
        if (e == hipSuccess) e = hipMemset(st.p_hg1, 0, (size_t)rows * t0.dim * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc(&st.p_hbg1, (size_t)rows * sizeof(int64_t));
        if (e == hipSuccess) e = hipMemset(st.p_hbg1, 0, (size_t)rows * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc(&st.p_part1, (size_t)cfg->n_partials * 2 * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(&st.p_prow1, (size_t)cfg->cols * t0.dim * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(&st.p_pbias1, (size_t)cfg->cols * sizeof(float));
        for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipMalloc(&st.hot[k], (size_t)hot_len * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc(&st.pint, 8 * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemset(st.pint, 0, 8 * sizeof(int32_t));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_fail("rg_mf_stepper_create: pipelined step buffers", e);
        st.pcounts[0] = st.counts[0];
        st.pcounts[1] = st.counts[1];
        st.pcounts[2] = st.p_counts2;
    }
    return RG_OK;
}

void alt_destroy(Stepper &st) {
    for (int i = 0; i < 2; ++i)
        if (st.stamp[i]) hipFree(st.stamp[i]);
    if (st.last_rel) hipFree(st.last_rel);
    if (st.umark) hipFree(st.umark);
    if (st.consts) hipFree(st.consts);
    if (st.rows_done) hipFree(st.rows_done);
    for (void *p : {(void *)st.p_counts2, (void *)st.p_list1, (void *)st.p_hg1, (void *)st.p_hbg1,
                    (void *)st.p_part1, (void *)st.p_prow1, (void *)st.p_pbias1, (void *)st.hot[0],
                    (void *)st.hot[1], (void *)st.hot[2], (void *)st.pint})
        if (p) hipFree(p);
}

}  // namespace stepper
}  // namespace rg
#pragma GCC visibility pop

using namespace rg::stepper;

extern "C" int rg_mf_stepper_pipelined(void *h) {
    Stepper *st = static_cast<Stepper *>(h);
    if (!st) return rg::fail_arg("rg_mf_stepper_pipelined: null handle");
    return st->pipe ? 1 : st->pipe2 ? 2 : 0;
}

extern "C" int rg_mf_stepper_pipe_error(void *h, int32_t *err_out) {
    Stepper *st = static_cast<Stepper *>(h);
    if (!st || !err_out) return rg::fail_arg("rg_mf_stepper_pipe_error: null argument");
    *err_out = 0;
    if (!st->pipe) return RG_OK;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(err_out, st->pint + 5, sizeof(int32_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? RG_OK : hip_fail("rg_mf_stepper_pipe_error", e);
}

extern "C" int rg_mf_stepper_flush(void *h, void *stream) {
    Stepper *st = static_cast<Stepper *>(h);
    if (!st) return rg::fail_arg("rg_mf_stepper_flush: null handle");
    return lazy_flush(*st, (hipStream_t)stream);
}

extern "C" int rg_mf_stepper_lazy_count(void *h, int32_t enable, uint64_t *rows_out) {
    Stepper *st = static_cast<Stepper *>(h);
    if (!st) return rg::fail_arg("rg_mf_stepper_lazy_count: null handle");
    if (rows_out) {
        *rows_out = 0;
        if (st->rows_done) {
            hipError_t e = hipDeviceSynchronize();
            if (e == hipSuccess) e = hipMemcpy(rows_out, st->rows_done, sizeof(uint64_t), hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemset(st->rows_done, 0, sizeof(uint64_t));
            if (e != hipSuccess) return hip_fail("rg_mf_stepper_lazy_count", e);
        }
    }
    st->count_rows = enable != 0 && st->rows_done != nullptr;
    return st->lazy ? 1 : 0;
}
