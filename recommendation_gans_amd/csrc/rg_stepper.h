// The MF stepper's state and the helpers its two halves share (internal to the library).
//
//   rg_stepper.cpp      the product's steps (split, data-parallel, owner-sharded), the word
//                       ring / generator and prefetch machinery, create / destroy and the
//                       dispatch in rg_mf_stepper_train
//   rg_stepper_alt.cpp  the measured-slower whole-step alternatives of the A/B build
//                       (pipelined, two-launch pipelined, lazy, overlapped: DESIGN §4.1, §9),
//                       their buffers and the C entries that only serve them
//
// Declared here: the Stepper struct, the slot constants, and exactly the functions one file
// defines and the other calls.  Everything is hidden from the library's dynamic symbols.
#pragma once
#include <hip/hip_runtime.h>

#include "rg_common.h"

#pragma GCC visibility push(hidden)
namespace rg {
namespace stepper {

constexpr int kSlots = 3;        // word slots in the ring
constexpr int kAheadSlots = 2;   // slots generated ahead of the one being consumed

struct Stepper {
    rg_mf_stepper_config_t cfg;
    bool failed = false;          // a step stopped half applied (pipe2's cold launch refused): unusable
    hipStream_t gen = nullptr, prep = nullptr;
    int64_t W = 0;                        // words per unit
    int64_t G = 1;                        // units per ring slot
    uint32_t *words[kSlots] = {nullptr, nullptr, nullptr};
    uint32_t *start_state[kSlots] = {nullptr, nullptr, nullptr};   // [625] state before the slot
    hipEvent_t gen_done[kSlots] = {nullptr, nullptr, nullptr};
    hipEvent_t consumed[kSlots] = {nullptr, nullptr, nullptr};     // after the slot's last consumer
    // Who produced / has seen / last consumed each slot.  Events are recorded lazily,
    // only when a DIFFERENT stream has to be ordered after that work (same-stream
    // order is free): the single-GPU split step then issues no event at all.
    // (a null hipStream_t is the legacy default stream, a real consumer: validity is tracked
    // by flags, never by null handles)
    hipStream_t prod[kSlots] = {nullptr, nullptr, nullptr};        // producing stream
    bool gen_rec[kSlots] = {false, false, false};                  // gen_done recorded after the production
    hipStream_t seen[kSlots] = {nullptr, nullptr, nullptr};        // a stream ordered after the production
    bool seen_ok[kSlots] = {false, false, false};
    hipStream_t cons_on[kSlots] = {nullptr, nullptr, nullptr};     // stream of the last consumer
    bool cons_ok[kSlots] = {false, false, false};                  // the slot was consumed since its production
    bool cons_rec[kSlots] = {false, false, false};                 // consumed recorded after that consumer
    bool inline_gen = false;              // split step: the walk of unit t+2 rides in step t's dense pass
    hipEvent_t ready[2] = {nullptr, nullptr};                      // side-stream prepared pairs buffers
    bool side_pending[2] = {false, false};                         // ready[b] not yet waited by the consumer
    hipEvent_t mark = nullptr;                                     // consumer-stream point a side prepare follows
    int64_t unit_base = 0;                // unit of relative slot 0 (reset when the state is loaded)
    int64_t gen_slots = 0;                // relative slots generated
    int64_t taken = 0;                    // units consumed
    // prepared pairs of unit prep_unit for input prep_in, in pairs buffer prep_unit % 2
    bool prepared = false;
    int64_t prep_unit = -1;
    rg_mf_step_in_t prep_in{};
    int32_t prep_serial = 0;              // nonzero: prepared with row marks (stamp array prep_arr)
    int prep_arr = 0;
    int32_t serial = 0;                   // last mark serial issued
    int32_t *stamp[2] = {nullptr, nullptr};   // [U + I] each, lazily allocated
    int set = 0;                          // ping-pong set holding the current tables
    bool fused = false;
    bool hot_scan = true;
    // MT jump-ahead path: the device state is in window form after a jump slot;
    // cp_pos tracks CPython's position-in-block of the same stream point
    rg::MtJumpPlan *jump = nullptr;
    bool window_form = false;
    int32_t cp_pos = 624;
    bool win_at[kSlots] = {false, false, false};   // form / position at each slot's start
    int32_t pos_at[kSlots] = {624, 624, 624};
    // owner step over a communicator (dp_mode 2, world > 1; opt-in RG_OWNER_MT_SLICE=1 -- the
    // emulated rank 0 of 8 measured 75.0 us per step with it, 74.6 without: the jump launches cost
    // the same either way, and the slot's MT work already hides beside the step): each rank
    // walks only ITS slice of every unit's words (L = W / world words at offset rank * L): a slot's
    // G slices come from one head walk, one jump launch and G parallel segments, the device state
    // ending G * W ahead; the slices are all-gathered on the generator stream
    // (rg::comm_words_allgather), and gstate -- the global stream's state at the start of the next
    // slot to produce, what the CPython state exports read -- is advanced by a jump of G * W per
    // slot.  One rank's MT work per slot: G * L words walked G-wide and two jump launches, instead
    // of the whole global draw's G * W words
    bool slice = false;
    int64_t L = 0;
    rg::MtJumpPlan *slice_plan = nullptr, *gjump = nullptr, *rjump = nullptr;
    uint32_t *gstate = nullptr, *jscratch = nullptr;
    // owner-sharded step (dp_mode 2) between its parts
    rg_mf_step_in_t own_in{};
    int64_t own_unit = -1;
    int own_stage = 0;                    // 0 idle, 1 after begin, 2 after mid
    hipEvent_t own_back = nullptr;        // after the owner backward (the item gradient may start)
    hipEvent_t own_grads = nullptr;       // train_owner: the lists are pulled (the user update may start)
    hipEvent_t own_users = nullptr;       // train_owner: the user update is done (the next step may start)
    // lazy dense pass (single-rank split step): deferred cold user-row updates
    bool lazy = false;
    bool lazy_pending = false;            // some user rows lag the current step
    int64_t lazy_base = 0;                // absolute step of last_rel == 0
    int32_t *last_rel = nullptr;          // [U]
    int32_t *umark = nullptr;             // [U]
    float *consts = nullptr;              // [2 * n_consts] Adam constants per absolute step
    int64_t n_consts = 0;
    uint64_t *rows_done = nullptr;        // diagnostic counter (rg_mf_stepper_lazy_count)
    bool count_rows = false;
    // claimed list slots (single-rank split step, rg_mf_work_t claim_num_users): the prepare of
    // unit u claims in counts[u % 2] (cfg.work.row_count and a second array owned here), so the
    // next unit's claims never meet the dense pass that reads and resets this unit's counts
    bool claim = false;
    int32_t *counts[2] = {nullptr, nullptr};
    int32_t *own_counts = nullptr;
    bool count_dirty[2] = {false, false};  // counts[b] hold claims no dense pass consumed yet
    bool prep_claimed = false;             // the prepared pairs carry claimed slots
    bool prep_in_pairs = false;            // split step: the next prepare rides in the pair pass
    // pipelined step (rg_mf_pipe_step; single rank, claimed slots, pointwise / bpr / hinge):
    // launch t updates step t's rows, runs step t+1's pair pass and step t+2's prepare.  A unit's
    // scratch by its parity -- claims in pcounts[u % 3], lists / overflow accumulators / partials
    // / planned partials in set u % 2 ([0] the caller's cfg.work, [1] owned here) -- and the
    // users its pair pass reads in hot[u % 3] (length pint[u % 3]).
    bool pipe = false;
    int32_t *pcounts[3] = {nullptr, nullptr, nullptr};
    int32_t *p_counts2 = nullptr;          // owned: pcounts[2]
    bool pdirty[3] = {false, false, false};   // pcounts[k] hold claims no dense pass consumed
    int32_t *p_list1 = nullptr;
    int64_t *p_hg1 = nullptr, *p_hbg1 = nullptr;
    float *p_part1 = nullptr, *p_prow1 = nullptr, *p_pbias1 = nullptr;
    int32_t *hot[3] = {nullptr, nullptr, nullptr};
    int32_t *pint = nullptr;               // [0..3) hot-list lengths, [3..5) gates, [5] error flag
    bool pair_dirty[2] = {false, false};   // overflow accumulators of set k hold a pair pass's adds
    int64_t paired = -1;                   // unit whose pair pass has run (its lists ready)
    rg_mf_step_in_t paired_in{};
    int64_t hot_prepped = -1;              // unit prepared with claims and a hot list, pair pending
    rg_mf_step_in_t hot_in{};
    int64_t last_pipe = -1;                // unit of the last pipelined launch (its counter resets)
    // two-launch pipelined step (train_pipe2, the single-GPU default): the same per-unit scratch
    // parities as `pipe`, no gate
    bool pipe2 = false;
};

// ---------------------------------------------------------------- rg_stepper.cpp
int hip_fail(const char *what, hipError_t e);
int64_t rel_slot(const Stepper &st, int64_t unit);
rg_mf_batch_t make_batch(const Stepper &st, const rg_mf_step_in_t &in, int64_t unit);
rg_mf_work_t work_for(const Stepper &st, const rg_mf_step_in_t &in);
bool same_input(const rg_mf_step_in_t &a, const rg_mf_step_in_t &b);
int begin_production(Stepper &st, hipStream_t p, int slot);
void end_production(Stepper &st, hipStream_t p, int slot);
int generate_upto(Stepper &st, int64_t unit, int ahead);
int keep_ahead(Stepper &st, int64_t unit);
int wait_words(Stepper &st, hipStream_t stream, int64_t unit);
int wait_side(Stepper &st, hipStream_t stream, int b);
int release(Stepper &st, hipStream_t stream);
rg_mf_loss_t loss_of(const Stepper &st, int64_t global_pos, float *out);
rg_opt_t opt_at(const Stepper &st, int64_t t);
bool ab_flag(const char *name, bool dflt);
int record(void *ev, hipStream_t s);

// ---------------------------------------------------------------- rg_stepper_alt.cpp
// buffers of the alternatives the configuration selects (st.lazy is set by the caller; sets
// st.pipe / st.pipe2); on failure the error is set and the caller destroys the stepper
int alt_create(Stepper &st);
void alt_destroy(Stepper &st);
// every lazily skipped user row up to the current step (no-op unless st.lazy and rows lag)
int lazy_flush(Stepper &st, hipStream_t s);
// drop every pipelined unit not trained yet (no-op unless st.pipe / st.pipe2)
int pipe_abandon(Stepper &st, hipStream_t s);
int train_pipe(Stepper &st, hipStream_t s, const rg_mf_step_in_t &cur, const rg_mf_step_in_t *next,
               const rg_mf_step_in_t *next2, float *loss_out, void *ev0, void *ev1);
int train_pipe2(Stepper &st, hipStream_t s, const rg_mf_step_in_t &cur, const rg_mf_step_in_t *next,
                const rg_mf_step_in_t *next2, float *loss_out, void *ev0, void *ev1);
int train_lazy(Stepper &st, hipStream_t s, const rg_mf_step_in_t &cur, const rg_mf_step_in_t *next,
               float *loss_out, void *ev0, void *ev1);
int train_fused(Stepper &st, hipStream_t s, const rg_mf_step_in_t &cur, const rg_mf_step_in_t *next,
                float *loss_out, void *ev0, void *ev1);

}  // namespace stepper
}  // namespace rg
#pragma GCC visibility pop
