// icp_run.hip — icp_run: the registration loop of GPU::ICP::find_corresponding_opti
// (src/GPU/gpu.cc:52-83) over the engine's resident clouds (icp_engine.hip), host code only.
//
//   icp_run -> run_loop: run_setup, then per iteration enqueue_canon (a scene in slot order: the
//              canonical schedule) or enqueue_launches (every other scene: the launch loop),
//              wait_one for the ring's oldest iteration, the drain and finish_run
//   run_setup hands over to run_kept (icp_set_metric, icp_set_max_distance, icp_set_robust, icp_set_trim,
//   icp_set_one_to_one)
//              or run_persistent (the one-launch loops of small clouds) where they apply
//   run_knobs / run_test_knobs: every environment switch of the run path (the table in icp_engine.h)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "icp_engine.h"
#include "icp_horn.h"

namespace {

#ifndef ICP_ITER2_DBG
#define ICP_ITER2_DBG 0 // (1: the diagnostic build, icp_grid.hip)
#endif
// (the diagnostic build's wave records behind ICP_ITER_DEBUG's 16 counters: four words a block)
constexpr size_t kIterDbgRec = ICP_ITER2_DBG ? 4 * (size_t)icp::kCanonStrandsMax : 0;

bool env_not0(const char *name) // on unless atoi(value) == 0
{
    const char *e = getenv(name);
    return !(e && atoi(e) == 0);
}
bool env_first_not0(const char *name) // on unless the value starts with '0'
{
    const char *e = getenv(name);
    return !(e && e[0] == '0');
}
bool env_first1(const char *name) // on if the value starts with '1'
{
    const char *e = getenv(name);
    return e && e[0] == '1';
}

RunKnobs read_run_knobs()
{
    RunKnobs k{};
    const char *e = getenv("ICP_GRID_BUDGET");
    k.grid_budget = e ? std::max(1, atoi(e)) : 0;
    k.grid_auto = env_not0("ICP_GRID_AUTO");
    k.grid_iter = env_not0("ICP_GRID_ITER");
    e = getenv("ICP_GRID_XCD");
    k.grid_xcd = e ? atoi(e) : 1;
    k.bundle_order_off = !env_not0("ICP_BUNDLE_ORDER");
    k.scene_order_off = !env_not0("ICP_SCENE_ORDER");
    k.cell_seed = env_not0("ICP_CELL_SEED");
    e = getenv("ICP_FIRST_K1");
    k.first_k1 = e && atoi(e) == 1;
    e = getenv("ICP_RUN_MODE");
    k.run_mode = !e ? -1
                 : std::strcmp(e, "launches") == 0   ? ICP_RUN_LAUNCHES
                 : std::strcmp(e, "persistent") == 0 ? ICP_RUN_PERSISTENT
                                                     : -1;
    e = getenv("ICP_PERSIST_MID");
    k.persist_mid_off = e && std::strcmp(e, "0") == 0;
    k.persist_stamps = getenv("ICP_PERSIST_STAMPS") != nullptr;
    e = getenv("ICP_PERSIST_NN");
    k.persist_cull = e && std::strcmp(e, "all") == 0 ? 0 : 1;
    k.mid_prepass = env_first1("ICP_MID_PREPASS");
    k.transform_records = env_not0("ICP_TRANSFORM_RECORDS");
    e = getenv("ICP_GRID_FAR_SHIFT");
    const int shift = e ? atoi(e) : 5;
    k.far_shift = shift >= 0 && shift <= 20 ? shift : 5;
    e = getenv("ICP_GRID_FAR");
    k.far_dist = e && std::string(e) == "dist";
    e = getenv("ICP_FUSED_STEPS");
    k.fused_steps = e ? atoi(e) & 3 : 0;
    k.err_pair = env_first_not0("ICP_ERR_PAIR");
    e = getenv("ICP_NN_TIMING_STRIDE");
    k.timing_stride = e ? std::max(1, atoi(e)) : 0;
    k.canon = env_first_not0("ICP_CANON");
    k.cert = env_first_not0("ICP_CERT");
    k.cert_two = env_first_not0("ICP_CERT_TWO") ? 1 : 0;
    e = getenv("ICP_CERT_SKIN");
    const double skin = e ? atof(e) : 0.25;
    k.cert_skin = skin >= 0.0 && skin <= 4.0 ? skin : 0.25;
    e = getenv("ICP_CERT_SKIN1");
    const double skin1 = e ? atof(e) : -1.0;
    k.cert_skin1 = skin1 >= 0.0 && skin1 <= 4.0 ? skin1 : k.cert_skin;
    e = getenv("ICP_ITER2_ORDER");
    k.iter2_order = !e ? 2 : atoi(e) >= 1 && atoi(e) <= 7 && atoi(e) != 4 ? atoi(e) : 0;
    e = getenv("ICP_ITER_DEBUG");
    k.iter_debug = !e ? 0 : atoi(e) == 2 ? 2 : 1;
    k.tail_split_err = getenv("ICP_TAIL_SPLIT_ERR") != nullptr;
    k.debug_policy = getenv("ICP_DEBUG_POLICY") != nullptr;
    return k;
}

// The knobs and what lives as long as they do: ICP_ITER_DEBUG's counters (device memory, allocated
// at the first run that fills them and kept until the process ends)
struct KnobOwner {
    RunKnobs knobs;
    unsigned long long *iter_dbg;
};
KnobOwner &knob_owner()
{
    static KnobOwner o{read_run_knobs(), nullptr};
    return o;
}

} // namespace

const RunKnobs &icp::engine::run_knobs() { return knob_owner().knobs; }

RunTestKnobs icp::engine::run_test_knobs()
{
    RunTestKnobs t{};
    const char *e = getenv("ICP_TEST_ENQUEUE_DELAY_US");
    t.enqueue_delay_us = e ? std::max(0, atoi(e)) : 0;
    t.tail_test_abort = env_first1("ICP_TAIL_TEST_ABORT");
    t.persist_test_abort = env_first1("ICP_PERSIST_TEST_ABORT");
    return t;
}

// Spin until err_step has written `ticket` (system-scope release after (done, iter)).  No
// event per iteration: an event marker costs the stream a ~6 us bubble.  If the stream
// drains without the ticket (an earlier failure), report instead of spinning forever.
int icp::engine::wait_flag(icp_ctx *ctx, const int *flag, int ticket)
{
    // The stream is queried (a drained stream without the flag is a failure) only once a wait has
    // lasted 20 ms, then every 20 ms: hipStreamQuery puts a marker at the stream's tail, right
    // behind the last error step enqueued, and the next search then started 5.6 us late -- every
    // iteration, with the spin's query every 1,024 pauses (profiles/r04z/gaps*)
    auto next = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
    for (unsigned spin = 1;; ++spin) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket) return ICP_OK;
        if ((spin & 1023u) == 0 && std::chrono::steady_clock::now() >= next) {
            next = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
            const hipError_t q = hipStreamQuery(ctx->st);
            if (q == hipErrorNotReady) continue;
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket) return ICP_OK;
            if (q != hipSuccess) return fail(ctx, ICP_E_HIP, std::string("icp_run: ") + hipGetErrorString(q));
            return fail(ctx, ICP_E_HIP, "icp_run: the stream drained without the iteration's flag");
        }
        __builtin_ia32_pause();
    }
}

namespace {

constexpr int kAhead = 1, kRing = 4; // iterations in flight beyond the one waited on; the flag ring's slots

// icp_set_progress: iterations [progress_next, upto) of the running icp_run, from the mapped
// error trace (each entry written before its iteration's ticket was released)
void report_progress(icp_ctx *ctx, int upto)
{
    if (!ctx->progress_fn) return;
    for (; ctx->progress_next < upto; ++ctx->progress_next)
        ctx->progress_fn(ctx->progress_next, ctx->h_trace[ctx->progress_next], ctx->progress_user);
}

// The run's result from the mapped host mirror of the last recorded iteration (both loops).
int finish_run(icp_ctx *ctx, double threshold, double *err_trace, icp_result *res,
               std::chrono::steady_clock::time_point wall0)
{
    const IterState &hs = *ctx->h_iter; // mirrored by the last recorded err step
    report_progress(ctx, hs.iter); // (the rest: a one-launch run reports here)
    icp_result r{};
    r.iterations = hs.iter;
    r.s = 1.0; // GPU::ICP ctor state (gpu.hh:53-55) when no iteration ran
    r.R[0] = r.R[4] = r.R[8] = 1.0;
    if (hs.iter > 0) {
        const double *tr = ctx->h_trace;
        if (err_trace) std::memcpy(err_trace, tr, sizeof(double) * (size_t)hs.iter);
        r.err = tr[hs.iter - 1];
        r.converged = r.err < threshold ? 1 : 0;
        r.s = hs.srt[0];
        for (int k = 0; k < 9; ++k) r.R[k] = hs.srt[1 + k];
        for (int k = 0; k < 3; ++k) r.t[k] = hs.srt[10 + k];
    }
    // (the run's applied steps into the context's total; a run that recorded nothing mirrored nothing)
    if (hs.iter > 0 && hs.tot_n > 0) compose_srt(hs.tot, ctx->tot, &ctx->tot_n);
    ctx->stats.iterations += hs.iter;
    if (ctx->nn_mode == ICP_NN_CERTIFIED) {
        ctx->stats.ambiguous += hs.nn_counts[0];
        ctx->stats.grid_fallback += hs.nn_counts[1];
        ctx->stats.level1_queued += hs.nn_counts[2];
        ctx->stats.level1_unrecovered += hs.nn_counts[3];
    }
    ctx->stats.iter_ms +=
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (res) *res = r;
    return ICP_OK;
}

// the run all-reduces its sums (ranks > 1 or a communicator): error test one iteration late
bool lag_run(const icp_ctx *ctx) { return ctx->comm != nullptr || ctx->world > 1; }

// entries of a run's mapped trace (the error's; the kept-pairs loop's K, W, K+ and C): at least
// max_iter, 64 to begin with (the previous run ended with a sync, so a trace too short may go)
size_t trace_entries(int max_iter) { return (size_t)std::max(max_iter, 64); }

// What one icp_run keeps from its set-up and across its iterations (run_setup builds it; both
// schedules, the wait side and the drain take it)
struct LoopRun {
    icp_ctx *ctx = nullptr;
    size_t n = 0;     // this rank's points
    double N = 0.0;   // all ranks'
    double threshold = 0.0;
    int max_iter = 0;
    std::chrono::steady_clock::time_point wall0;
    RunTestKnobs tk{};
    bool need_p32 = false;   // the scene's fp32 copy has a reader: every transform keeps it
    bool fuse_seeds = false; // seeded f16 searches: each transform writes the next search's seeds
    bool lag = false;        // lag_run: the error test one iteration late
    bool canon = false;      // the canonical schedule (a scene in slot order)
    // the search policy (run_setup_policy)
    bool grid_policy = false, carry = false, hold_first = false;
    int far_thr = 0;
    int far_obs = -1;       // far_acc of the last iteration the host has seen
    int q2_obs = -1;        // queued2 of the last iteration the host has seen
    int hold_far = -1;      // transform 0's far count, read by hold_first
    std::vector<int> fold_far; // [j]: the far count mirrored with iteration j's (lagged) error step
    bool grid_next = false; // the launch loop: the path of the next search
    // the launch loop's steps (run_setup_steps)
    bool fused_moments = false, fused_steps = false, err_pair = false, fused_tail = false, seeds_at_start = false;
    int tail_blocks = 0;
    unsigned tail_epoch = 0;
    const int *digest_order = nullptr;
    unsigned long long *iter_dbg = nullptr;
    SeedArgs sa;      // a transform before a bundle / f16 search
    SeedArgs sa_grid; // a transform before a grid search: its seed distances only
    // What the last enqueued transform wrote for the next search (nn_search_begin uses each part
    // only in the form it was written in).  A carried-over run starts from the last run's seed
    // distances (seedd_valid); everything else is rebuilt by the first search.
    SeedState ws;
    CanonStep cs;
    // The fused grid iteration's exclusion certificate (icp_grid.hip): the state one fused
    // iteration writes is read by the next one of this run only (cert_prev); any other search
    // leaves it stale.
    CertArgs cert;
    bool cert_prev = false;
    // The fused iteration's dispatch order (IterOrder): the table the fold builds from one fused
    // launch's walker counts is the next fused launch's, and only that one's -- walk_written: the
    // last launch left counts worth sorting (one-strand workgroups, a certificate state read: in a
    // run's first fused launch every query walks); order_ok: the fold since built the table.  Any
    // other search, and the run's end, drop both, so a table never outlives its scene
    // (icp_set_scene), its size or its path.
    IterOrder order;
    bool walk_written = false, order_ok = false;
    bool xf_pending = false; // (canon: the last Horn step's transform is still to be applied)
    int rows_strands = 0;    // (> 0: the last fused launch wrote the canonical rows as this many strands)
    int slot_ticket[kRing] = {};
    bool ar_timed[kRing] = {};
    int enqueued = 0, waited = 0, recorded = 0;
    bool stop = false;
    int timing_stride = 0, timing_phase = 0; // (stride 0: no iteration is timed -- run_kept)
};

// The O(N*M) kernel is timed (two events; on multi-rank runs two more around the
// all-reduce) every 8th iteration: each event marker leaves a ~4.4 us gap in the stream,
// which at the bundle filter's C4 iteration (~0.25 ms) is 3.5% per iteration for the filter's
// pair and ~11% of a W = 8 shard's 0.15 ms iteration for all four (profiles/r03bf/ kernel
// trace).  stats.nn_ms / nn_launches stays the mean of the timed launches.
// ICP_NN_TIMING_STRIDE overrides (1: every iteration, as before for searches of >= 2^32 pairs).
// The sampled iterations rotate from run to run (run r: those = r mod the stride), so that over
// a stride's worth of registrations every iteration index is timed once -- the mean of the timed
// launches is then the mean of all of them, as a kernel trace of the same runs gives it (a fixed
// phase sampled iterations 1, 9, 17, 25 only, the slower early ones among them); iteration 0
// (its search unseeded) is never sampled
bool is_timed(const LoopRun &r, int it)
{
    return r.timing_stride > 0 && it % r.timing_stride == r.timing_phase && (it > 0 || r.timing_stride == 1);
}

// The wait side of the ring (both loops): the oldest iteration in flight's flag, the far count and
// second-pass queue its error step mirrored (the policy's runs), progress, its timed events.
int wait_one(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    const int slot = r.waited % kRing;
    TRY(wait_flag(ctx, ctx->h_flags + 4 * slot + 2, r.slot_ticket[slot]));
    ++r.waited;
    if (r.grid_policy) { // (mirrored by the error step of that iteration)
        r.far_obs = ctx->h_iter->far_acc;
        if (r.waited - 1 < (int)r.fold_far.size()) r.fold_far[r.waited - 1] = r.far_obs;
        r.q2_obs = ctx->h_iter->queued2;
        if (run_knobs().debug_policy)
            fprintf(stderr, "[policy] waited %d far %d thr %d next_grid %d\n", r.waited, r.far_obs, r.far_thr, (int)r.grid_next);
    }
    const int done = ctx->h_flags[4 * slot], iters = ctx->h_flags[4 * slot + 1];
    report_progress(ctx, iters); // (the iterations recorded so far, as they end)
    if (iters > r.recorded) { // this iteration counted: its NN kernel time (if timed)
        float ms = 0.f;
        if (r.n && is_timed(r, r.waited - 1)) {
            // (an empty shard records no events)
            if (hipEventElapsedTime(&ms, ctx->iter_ev[5 * slot], ctx->iter_ev[5 * slot + 1]) == hipSuccess) {
                ctx->stats.nn_ms += ms;
                ctx->stats.nn_launches += 1;
            } else {
                (void)hipGetLastError(); // a failed query must not surface at the next launch check
            }
        }
        if (r.ar_timed[slot]) { // the all-reduce rode on this slot's iteration
            if (hipEventElapsedTime(&ms, ctx->iter_ev[5 * slot + 3], ctx->iter_ev[5 * slot + 4]) == hipSuccess) {
                ctx->stats.allreduce_ms += ms;
                ctx->stats.allreduce_calls += 1;
            } else {
                (void)hipGetLastError();
            }
        }
        ctx->stats.nn_pairs += (long long)r.n * (long long)ctx->nm;
        r.recorded = iters;
    }
    r.stop = done != 0;
    return ICP_OK;
}

// What every loop does after search `it` is enqueued: the filter counters and path bits, the
// correspondences' validity, the CPU rule's host fix-up, the index digest.  fused: the search was
// a fused grid iteration's (the grid's, y written, no kd positions; its condition excludes the CPU
// rule, so no fix-up).  slot: the ring slot whose all-reduce timing is cleared (-1: none, run_kept).
int after_search(LoopRun &r, int it, bool fused, int slot)
{
    icp_ctx *ctx = r.ctx;
    if (fused) {
        ctx->stats.last_filter = ICP_FILTER_GRID;
        ctx->kpos_valid = false;
        ctx->y_ready = true;
    }
    if (ctx->stats.last_filter == ICP_FILTER_BUNDLE) ctx->stats.run_bundle_searches += 1;
    else if (ctx->stats.last_filter == ICP_FILTER_GRID) ctx->stats.run_grid_searches += 1;
    if (ctx->stats.last_filter == ICP_FILTER_GRID && it < 64) ctx->stats.run_path_bits |= 1ull << it;
    ctx->seeds_valid = true; // idx pairs every point of the resident scene
    if (!fused) TRY(cpu_rule_fixup(ctx, ctx->scene, r.n, &ctx->iter_state->done)); // (ICP_NN_RULE_CPU_SQRT only: host near ties)
    if (slot >= 0) r.ar_timed[slot] = false;
    if ((size_t)it < ctx->digest_cap) {
        launch_idx_digest(ctx->idx, (int)r.n, &ctx->iter_state->done, ctx->digest + 3 * (size_t)it, ctx->st, r.digest_order);
        LAUNCHCHK("idx_digest");
    }
    return ICP_OK;
}

// what a transform run with `sa_t` leaves for the next search
SeedState seed_state_of(const SeedArgs &sa_t)
{
    SeedState ws;
    ws.seedd = sa_t.seedd != nullptr; // (every form writes the seed distances)
    ws.seed16 = !sa_t.seed16 ? 0 : sa_t.qop && sa_t.local_r >= 0.0 ? 2 : 1;
    ws.records = sa_t.qop != nullptr;
    ws.rec_local = sa_t.qop ? sa_t.local_r : -1.0;
    return ws;
}

// The transform before a bundle search writes that search's slot records (the prep's output,
// in order) once the images exist and a bundle search of this size has sized the buffers --
// decided per transform, in the form the next search will run: the local pair test's with the
// current frames' R, else the global one.  (It was decided once at the start of the run:
// after icp_set_model the images are pending, b_rlmax is -1, and a run whose policy turned to
// the bundle mid-run then wrote global-form records for a search that, its images built in
// between, ran the local form -- the C5 registration stall)
void records_args(const LoopRun &r, SeedArgs &s)
{
    const icp_ctx *ctx = r.ctx;
    if (!run_knobs().transform_records || !ctx->scene_slot || !r.fuse_seeds || !s.seed16 || !s.seedd ||
        ctx->bundle_pending || ctx->nb_pad <= 0 || level1_kind(ctx, r.n) != 3 || !bundle_v2())
        return;
    const size_t nslots = bundle2_slots(plan_nn_bundle2(r.n, ctx->nb_pad));
    if (!ctx->b_qop || ctx->b_qop.capacity() < nslots * 64 || ctx->b_gop.capacity() < nslots ||
        ctx->b_gctr.capacity() < nslots / 32)
        return;
    s.qop = ctx->b_qop;
    s.gop = ctx->b_gop;
    s.gctr = ctx->b_gctr;
    s.nslots = (int)nslots;
    s.local_r = ctx->b_rlmax >= 0.0 && bundle_local() ? ctx->b_rlmax : -1.0; // (as the search decides)
}

// The state a run with the fused tail starts from (n <= kTailMaxBlocks * kBlock points: a few MB)
// into tail_backup, for the separate-launch rerun should a tail barrier time out; restore: back.
int tail_snapshot(icp_ctx *ctx, size_t n, bool with_idx, bool restore)
{
    DevCloud &P = ctx->scene;
    char *bk = ctx->tail_backup;
    const auto copy = [&](void *live, size_t off, size_t bytes) {
        return restore ? hipMemcpyAsync(live, bk + off, bytes, hipMemcpyDeviceToDevice, ctx->st)
                       : hipMemcpyAsync(bk + off, live, bytes, hipMemcpyDeviceToDevice, ctx->st);
    };
    HIPCHK(copy(P.x, 0, n * sizeof(double)));
    HIPCHK(copy(P.y, n * 8, n * sizeof(double)));
    HIPCHK(copy(P.z, n * 16, n * sizeof(double)));
    if (P.f) HIPCHK(copy(P.f, n * 24, n * sizeof(float4)));
    if (with_idx) HIPCHK(copy(ctx->idx, n * 40, n * sizeof(int)));
    return ICP_OK;
}

// (partials: the residual's unreduced rows, folded in the same launch)
// (horn: this iteration's Horn step in the same single-thread launch, right after it)
int enqueue_err_step(LoopRun &r, int it, const double *partials = nullptr, bool horn = false)
{
    icp_ctx *ctx = r.ctx;
    IterState *sd = ctx->iter_state;
    const int sl = it % kRing;
    // (done, iter) straight into mapped host memory, then the slot's ticket
    r.slot_ticket[sl] = ++ctx->flag_ticket;
    if (horn)
        launch_err_horn_step(ctx->sums, r.N, r.threshold, r.max_iter, ctx->err_trace_dev, sd, ctx->h_flags.dev() + 4 * sl,
                             r.slot_ticket[sl], ctx->h_iter.dev(), ctx->h_trace.dev(), ctx->c, 1, ctx->amb_count, ctx->st);
    else
        launch_err_step(ctx->sums, r.N, r.threshold, r.max_iter, ctx->err_trace_dev, sd, ctx->h_flags.dev() + 4 * sl,
                        r.slot_ticket[sl], ctx->h_iter.dev(), ctx->h_trace.dev(), ctx->st, partials, red_blocks(r.n));
    LAUNCHCHK("err_step");
    return ICP_OK;
}

// Workgroups of the one-launch registration for this run, or 0 if it does not apply: one
// rank, no communicator, no per-iteration instrumentation, and either
//  - n <= kRedSingle (the single-workgroup passes it reproduces bit for bit), the model in
//    LDS, >= 64 co-resident workgroups (icp_persistent_kernel), or
//  - kRedSingle < n <= kTailMaxBlocks * 256, red_blocks(n) workgroups co-resident with a
//    quarter of the CUs to spare, nm <= kPersistMidMaxModel (icp_persistent_mid_kernel; *mid_out).
int persistent_grid(const icp_ctx *ctx, size_t n, int max_iter, size_t *lds_out, bool *mid_out)
{
    *mid_out = false;
    const int forced = run_knobs().run_mode; // ICP_RUN_MODE=launches|persistent (A/B runs)
    const int mode = forced >= 0 ? forced : ctx->run_mode;
    if (mode == ICP_RUN_LAUNCHES) return 0;
    if (mode == ICP_RUN_AUTO && ctx->nn_variant != ICP_NN_VARIANT_AUTO) return 0; // explicit variants run their cascade
    if (ctx->world != 1 || ctx->comm || ctx->host_reduce || ctx->digest_cap || max_iter < 1) return 0;
    if (ctx->nn_rule != ICP_NN_RULE_SQUARED) return 0; // (the host resolves the CPU rule's near ties)
    if (n > (size_t)kRedSingle) {
        // (ICP_PERSIST_MID=0: mid-size runs keep the launch loop, A/B)
        if (run_knobs().persist_mid_off || n > (size_t)kTailMaxBlocks * kBlock || ctx->nm < 1 || ctx->nm > (size_t)kPersistMidMaxModel ||
            !ctx->pm_img)
            return 0;
        // the classic red_blocks(n) workgroups, widened to the whole co-resident grid: the extra
        // ones own no point and only search (their partial rows are +0.0, which leaves
        // reduce_kernel's tree bit for bit unchanged)
        const int classic = red_blocks(n), wide = std::min(kTailMaxBlocks, ctx->n_cu * 3 / 4);
        const int grid = std::max(classic, wide);
        if (grid > ctx->n_cu * 3 / 4 || grid > kTailMaxBlocks || (size_t)classic * kBlock < n) return 0;
        const size_t lds = 24 * (ctx->pm_blocks + (ctx->nm + 15) / 16);
        if (lds > kPersistMidLdsMax || lds + persistent_mid_static_lds() > ctx->lds_per_cu) return 0;
        *lds_out = lds;
        *mid_out = true;
        return grid;
    }
    if (n < 4 || ctx->nm < 1 || ctx->nm > (size_t)kPersistMaxModel) return 0;
    const size_t lds = 24 * ctx->nm + 48 * ctx->pm_blocks, statics = persistent_static_lds();
    if (!ctx->pm_img) return 0;
    if (lds + statics > ctx->lds_per_cu) return 0; // (gfx950: one workgroup may take the whole 160 KiB)
    const int per_cu = (int)std::min<size_t>(2, ctx->lds_per_cu / (lds + statics)); // (<= 2: 199 VGPRs)
    // residency margin: a quarter of the admissible slots left free (a barrier over a grid that
    // is not fully resident would only time out, but it would be an error, not a slow run);
    // 256 / 128 / 64 workgroups, so that every one owns the same number of virtual threads
    const int slots = ctx->n_cu * per_cu * 3 / 4;
    const int grid = slots >= kBlock ? kBlock : slots >= kBlock / 2 ? kBlock / 2 : kBlock / 4;
    if (grid < 64) return 0;
    *lds_out = lds;
    return grid;
}

// ICP_PERSIST_STAMPS: phase durations of workgroup 0 (tags: 0 NN begin, 1 NN end, 2 published,
// 3 barrier passed, 8 partials loaded, 4 folded, 5 Horn done, 6 transformed, 7 end), to stderr
int persist_stamps_report(icp_ctx *ctx, int grid, size_t lds, bool mid)
{
    std::vector<unsigned long long> h(2 * kPersistMaxStamps + 2 * kBlock + 8 * kBlock + 2 * kBlock);
    HIPCHK(hipMemcpy(h.data(), ctx->pers_stamps, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    double acc[9] = {0}, cntp[9] = {0};
    for (int k = 1; k < kPersistMaxStamps && h[2 * k + 1]; ++k) {
        const int tag = (int)h[2 * k];
        acc[tag] += (double)(h[2 * k + 1] - h[2 * k - 1]) * 0.01; // 100 MHz -> us
        cntp[tag] += 1;
    }
    if (mid) { // workgroup 0's NN phase (tag 0 -> 1, its barrier wait included) per iteration
        fprintf(stderr, "[persist-mid] NN per iteration (us):");
        for (int k = 1; k < kPersistMaxStamps && h[2 * k + 1]; ++k)
            if (h[2 * k] == 1 && h[2 * k - 2] == 0) fprintf(stderr, " %.0f", (double)(h[2 * k + 1] - h[2 * k - 1]) * 0.01);
        fprintf(stderr, "\n");
    }
    fprintf(stderr, "[persist] grid %d lds %zu: us ending at tag (calls):", grid, lds);
    for (int t = 0; t < 9; ++t) fprintf(stderr, " %d:%.2f(%g)", t, acc[t], cntp[t]);
    double nmin = 1e30, nmax = 0, nsum = 0, bmin = 1e30, bmax = 0, bsum = 0;
    for (int w = 0; w < grid; ++w) {
        const double tn = h[2 * kPersistMaxStamps + 2 * w] * 0.01, tb = h[2 * kPersistMaxStamps + 2 * w + 1] * 0.01;
        nmin = std::min(nmin, tn), nmax = std::max(nmax, tn), nsum += tn;
        bmin = std::min(bmin, tb), bmax = std::max(bmax, tb), bsum += tb;
    }
    fprintf(stderr, " | per-wg NN min/mean/max %.1f/%.1f/%.1f barrier %.1f/%.1f/%.1f us\n", nmin, nsum / grid, nmax,
            bmin, bsum / grid, bmax);
    if (mid) { // per workgroup: NN us (all iterations, first), superblocks / tile rounds / blocks per query
        const unsigned long long *w = h.data() + 2 * kPersistMaxStamps + 2 * kBlock;
        double mx[5] = {0}, sm[5] = {0};
        for (int g = 0; g < grid; ++g) {
            const double q = std::max<double>(1.0, (double)w[8 * g + 5]);
            const double v[5] = {w[8 * g] * 0.01, w[8 * g + 1] * 0.01, w[8 * g + 2] / q, w[8 * g + 3] / q, w[8 * g + 4] / q};
            for (int k = 0; k < 5; ++k) mx[k] = std::max(mx[k], v[k]), sm[k] += v[k];
        }
        double tph[4] = {0, 0, 0, 0}, cnt[3] = {0, 0, 0};
        for (int g = 0; g < grid; ++g) {
            tph[0] += (double)(w[8 * g + 6] & 0xffffffffu) * 0.01;
            tph[1] += (double)(w[8 * g + 6] >> 32) * 0.01;
            tph[2] += (double)(w[8 * g + 7] & 0xffffffffu) * 0.01;
            tph[3] += (double)(w[8 * g + 7] >> 32) * 0.01;
            for (int k = 0; k < 3; ++k) cnt[k] += (double)w[8 * g + 2 + k];
        }
        const double nbat = (double)((ctx->scene.n + 3) / 4) * std::max(1, ctx->h_iter->iter);
        double wsum = 0, wmax = 0; // per-wave busy time, summed over the iterations (max: of one iteration)
        for (int g = 0; g < grid; ++g) {
            wsum += (double)w[8 * kBlock + 2 * g] * 0.01;
            wmax = std::max(wmax, (double)w[8 * kBlock + 2 * g + 1] * 0.01);
        }
        const int iters = std::max(1, ctx->h_iter->iter);
        fprintf(stderr, "[persist-mid] wave busy per NN: mean %.1f us, slowest wave of any NN %.1f us\n",
                wsum / (grid * 8.0 * iters), wmax);
        fprintf(stderr, "[persist-mid] per wg NN mean/max %.1f/%.1f us (first %.1f/%.1f) | per batch: superblocks %.2f "
                        "tile rounds %.2f blocks %.2f | per batch us: query loads %.2f tests %.2f gathers %.2f reduce+store %.2f\n",
                sm[0] / grid, mx[0], sm[1] / grid, mx[1], cnt[0] / nbat, cnt[1] / nbat, cnt[2] / nbat, tph[0] / nbat,
                tph[1] / nbat, tph[2] / nbat, tph[3] / nbat);
    }
    return ICP_OK;
}

// icp_run as ONE launch (launch_icp_persistent): same results, bit for bit, as the loop below.
// kPersistFallback: the launch gave up at its first grid barrier, before writing any state
// (some workgroups were not co-resident); the caller runs the launch loop instead.
constexpr int kPersistFallback = 1;
int run_persistent(icp_ctx *ctx, int grid, size_t lds, bool mid, int max_iter, double threshold,
                   double *err_trace, icp_result *res, std::chrono::steady_clock::time_point wall0)
{
    static_assert(2 * kTailMaxBlocks <= 2 * kBlock, "pers_part holds the mid kernel's rows");
    const size_t n = ctx->scene.n;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    TRY(ctx->idx.grow(ctx, n)); // (a fresh context has run no search yet)
    TRY(ctx->pers_part.grow(ctx, (size_t)2 * kBlock * kNumSums));
    const bool stamps = run_knobs().persist_stamps; // (ICP_PERSIST_STAMPS)
    if (stamps) {
        const size_t ns = (size_t)2 * kPersistMaxStamps + 2 * kBlock + 8 * kBlock + 2 * kBlock;
        TRY(ctx->pers_stamps.grow(ctx, ns));
        HIPCHK(hipMemsetAsync(ctx->pers_stamps, 0, sizeof(unsigned long long) * ns, ctx->st));
    }
    TRY(ctx->pers_sync.grow(ctx, kPersistSyncWords));
    // the barrier words count on from the previous launch of the same grid (no memset launch);
    // zeroed on the first launch, when the grid changes and after an aborted launch
    if (!ctx->pers_sync_valid || ctx->pers_grid != grid) {
        HIPCHK(hipMemsetAsync(ctx->pers_sync, 0, kPersistSyncWords * sizeof(unsigned), ctx->st));
        ctx->pers_epoch_base = 0;
        ctx->pers_grid = grid;
    }
    ctx->pers_sync_valid = false; // (until this launch has completed cleanly)
    ctx->h_flags[3] = 0; // abort word (mapped host)
    ctx->h_flags[7] = 0; // barriers used (mapped host)
    PersistArgs a{};
    a.img = ctx->pm_img;
    a.nblk = (int)ctx->pm_blocks;
    a.nm = (int)ctx->nm;
    a.n = (int)n;
    a.px = P.x;
    a.py = P.y;
    a.pz = P.z;
    a.yx = Y.x;
    a.yy = Y.y;
    a.yz = Y.z;
    a.p32 = P.f;
    a.idx = ctx->idx;
    a.part = ctx->pers_part;
    a.sync = ctx->pers_sync;
    a.h_abort = ctx->h_flags.dev() + 3;
    a.N = (double)ctx->np_total;
    a.c0 = ctx->c[0];
    a.c1 = ctx->c[1];
    a.c2 = ctx->c[2];
    a.threshold = threshold;
    a.max_iter = max_iter;
    a.err_trace = ctx->err_trace_dev;
    a.s_glob = ctx->iter_state;
    a.h_state = ctx->h_iter.dev();
    a.h_trace = ctx->h_trace.dev();
    a.stamps = stamps ? ctx->pers_stamps : nullptr;
    a.cull = run_knobs().persist_cull; // (ICP_PERSIST_NN=all: every model point for every query, A/B)
    a.epoch_base = ctx->pers_epoch_base;
    a.h_epochs = ctx->h_flags.dev() + 7;
    // (tests: ICP_PERSIST_TEST_ABORT=1 makes the first barrier fail as if a workgroup never came)
    a.test_abort = run_test_knobs().persist_test_abort;
    for (int k = 0; k < 3; ++k) a.m0[k] = ctx->model_host[k];
    if (mid) {
        // the first search is seeded by the resident correspondences if they pair this scene
        // already; else every query descends to its nearest-box block (ICP_MID_PREPASS=1: one
        // pass of the exact cascade instead, for A/B runs)
        const bool prepass = run_knobs().mid_prepass;
        if (!ctx->seeds_valid && prepass) {
            launch_run_init(ctx->iter_state, ctx->amb_count, ctx->st);
            TRY(nn_search_begin(ctx, P, n, false, nullptr, nullptr, false, nullptr, &ctx->iter_state->done));
        }
        TRY(ctx->mid_q4.grow(ctx, 4 * n));
        TRY(ctx->mid_res.grow(ctx, n));
        TRY(ctx->mid_perm.grow(ctx, n));
        const size_t ob = mid_order_scratch_bytes((int)n);
        TRY(ctx->mid_cnt.grow(ctx, ob));
        if (launch_mid_order(P.x, P.y, P.z, (int)n, ctx->m_lo, ctx->m_hi, ctx->mid_cnt, ob, ctx->mid_perm, ctx->st))
            return fail(ctx, ICP_E_HIP, "icp_run: the mid-size search order (radix sort) failed");
        LAUNCHCHK("mid_order");
        a.perm = ctx->mid_perm;
        a.seed_big = ctx->pm_seed_big;
        a.seed_idx = ctx->seeds_valid || prepass ? ctx->idx : nullptr;
        a.m4 = ctx->m4;
        a.q4 = ctx->mid_q4;
        a.res = ctx->mid_res;
        launch_icp_persistent_mid(a, grid, lds, ctx->st);
    } else {
        launch_icp_persistent(a, grid, lds, ctx->st);
    }
    LAUNCHCHK("icp_persistent");
    if (stamps) { // (the timers of every workgroup: the whole grid must have finished)
        HIPCHK(hipStreamSynchronize(ctx->st));
    } else { // workgroup 0's last store (h_flags[7] = barriers used, a release after the run's
             // mirrored state); an aborted launch never writes it and ends with the stream
        // (the stream queried after 2 ms, then every 2 ms: each query leaves a marker behind the
        // launch, which the next launch waits for -- see wait_flag)
        auto next = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
        for (unsigned spin = 1; __atomic_load_n(ctx->h_flags + 7, __ATOMIC_ACQUIRE) == 0; ++spin) {
            if ((spin & 1023u) == 0 && std::chrono::steady_clock::now() >= next) {
                next = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
                const hipError_t q = hipStreamQuery(ctx->st);
                if (q == hipErrorNotReady) continue;
                if (q != hipSuccess) return fail(ctx, ICP_E_HIP, std::string("icp_run: ") + hipGetErrorString(q));
                break; // (finished: aborted, or the word landed just now)
            }
            __builtin_ia32_pause();
        }
    }
    if (stamps) TRY(persist_stamps_report(ctx, grid, lds, mid));
    const int aborted = __atomic_load_n(ctx->h_flags + 3, __ATOMIC_ACQUIRE);
    if (aborted == 1) { // at the first barrier: not co-resident, nothing written -> the launch loop
        ctx->stats.persistent_fallbacks += 1;
        return kPersistFallback;
    }
    if (aborted != 0)
        return fail(ctx, ICP_E_HIP, "icp_run: a grid barrier of the one-launch loop timed out (workgroups not co-resident)");
    ctx->pers_epoch_base += (unsigned)__atomic_load_n(ctx->h_flags + 7, __ATOMIC_ACQUIRE);
    ctx->pers_sync_valid = true;
    ctx->seeds_valid = true;
    ctx->seedd_valid = false; // (the one-launch loop keeps no seed distances)
    const int iters = ctx->h_iter->iter;
    ctx->stats.nn_pairs += (long long)iters * (long long)n * (long long)ctx->nm;
    ctx->stats.persistent_runs += 1;
    ctx->stats.last_filter = ICP_FILTER_ONE_LAUNCH;
    return finish_run(ctx, threshold, err_trace, res, wall0);
}

// icp_run over the kept pairs: the max-correspondence-distance gate (icp_set_max_distance; kernels
// in icp_gated.hip), the point-to-plane metric (icp_set_metric; icp_plane.hip), robust weights
// (icp_set_robust; both files), or any of them together.
// run_setup_buffers has prepared the loop state, the mapped mirrors and the flag ring.
// Per iteration: the search as the launch loop's generic path runs it (seeded by the previous
// correspondences, nothing carried from a transform); the moments (gate, mask, and the metric's
// sums: 18 for Horn's closed form with N = K, 28 for the 6 x 6 normal equations); their fold and
// the metric's step; the transform of every point with the kept points' residual (along the normal
// for the plane metric); its fold and the error step with N = K.  With ranks or a communicator the
// sums and the residual are each all-reduced before their step (two all-reduces an iteration; the
// error test is not lagged).  The scene keeps the order it is in (file or slot); on one rank the
// host does not synchronise inside an iteration.
// The metrics differ in: the normals (plane), the least K (4 / 6, in the step kernels), D (the
// plane metric runs ungated with D = +inf), the first iteration's pre-pass (point-to-point only:
// the plane sums need no shifts), the kernels behind the launchers, and the closing messages.
// A gated run leaves icp_get_inliers its last gate and K trace; an ungated one leaves the last
// gated run's.
// With robust weights (icp_set_robust) the moments and the fold + step are their weighted
// instantiations (rows of 20 and 30: the sums, K, W = sum w, K+ = #{w > 0}; the pre-pass's shifts
// divide by W; the step stops on K+ as on K and writes W and K+ to their mapped traces); the
// transform, the residual and the error step, hence err = (e + e) / K, are the unweighted loop's.
// With a trim (icp_set_trim) the iteration's gate is min(D, C), C the T-th smallest d2 over all
// ranks, selected on the device (icp_select.hip) between the search and the moments: a keys pass
// gathers and stores y and writes each point's d2 key, kSelectPasses passes of count + pick (one
// launch of one workgroup up to kRedSingle points on one rank) leave C in device memory, and every
// moments pass then runs in its streamed form with the cut's address.  With ranks each pass's bins are all-reduced before its pick (kSelectPasses more all-reduces an
// iteration).  T below the metric's least count stops the run as K below it does.  A trimmed run
// counts as a gated one for icp_get_inliers, and leaves icp_get_trim_trace its C trace.
// With icp_set_one_to_one a pair is kept only when it is its model point's closest: between the search
// (and the trim's selection) and the moments, the table best (one 64-bit key a model point, all ones
// from a memset on the run's stream at every iteration's start) takes the unsigned minimum of the d2
// keys that chose each model point (icp_unique.hip: unique_min_kernel gathers and stores y like the
// keys pass; with a trim it scatters the keys that pass wrote), and every moments pass then runs in
// its streamed form with the table's address and keeps d2 <= min(D, C) && key(d2) == best[idx].  The
// minimum is over this rank's points, so more than one rank is refused (run_setup).  A one-to-one run
// counts as a gated one for icp_get_inliers.
// With icp_set_plane_symmetric the plane metric's three launches are their symmetric instantiations
// (icp_plane.hip: SYMM), which also read the scene's normals u0 in the scene's current order and the
// total since icp_set_scene* (SymmArgs: the context's at the run's start, the run's own from the loop
// state); everything else of the loop, the sums' width and the all-reduces included, is the plane metric's.
// With icp_set_plane_to_plane the moments and the transform are icp_gicp.hip's (each kept pair enters
// with a 3 x 3 information matrix from both clouds' normals; the same SymmArgs and 1 - epsilon), and
// the fold and step between them are the one-sided plane metric's as they stand.
int run_kept(icp_ctx *ctx, int max_iter, double threshold, double *err_trace, icp_result *res, bool need_p32,
             std::chrono::steady_clock::time_point wall0)
{
    const bool plane = ctx->metric == ICP_METRIC_POINT_TO_PLANE;
    if (plane && !ctx->has_normals)
        return fail(ctx, ICP_E_NO_MODEL, "icp_run: the point-to-plane metric needs the model's normals (icp_set_model_normals)");
    const bool symm = plane && ctx->plane_symmetric;
    if (symm && !ctx->has_scene_normals)
        return fail(ctx, ICP_E_NO_MODEL, "icp_run: the symmetric point-to-plane iteration needs the scene's normals "
                                         "(icp_set_scene_normals, icp_estimate_scene_normals)");
    const bool gicp = plane && ctx->plane_to_plane > 0.0; // (never with symm: run_setup refused both)
    if (gicp && !ctx->has_scene_normals)
        return fail(ctx, ICP_E_NO_MODEL, "icp_run: the plane-to-plane iteration needs the scene's normals "
                                         "(icp_set_scene_normals, icp_estimate_scene_normals)");
    if (max_iter < 1) return finish_run(ctx, threshold, err_trace, res, wall0); // (no gate evaluated: the last one stays)
    const size_t n = ctx->scene.n;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    const bool trim = ctx->trim_fraction < 1.0;
    const bool uniq = ctx->one_to_one;
    const bool gated = ctx->gate_dmax > 0.0 || trim || uniq; // (what icp_get_inliers reports)
    const double D = ctx->gate_dmax > 0.0 ? ctx->gate_dmax * ctx->gate_dmax : HUGE_VAL; // (fp64, once)
    // the trim's count, PCL's rule: the product in fp64 as written, truncated, once
    const long long T = trim ? std::max(1LL, (long long)(ctx->trim_fraction * (double)ctx->np_total)) : 0;
    const bool trim_few = trim && T < (ctx->metric == ICP_METRIC_POINT_TO_PLANE ? 6 : 4);
    const int robust = ctx->robust_kind; // (ICP_ROBUST_*; 0: the unweighted kernels, as without the setting)
    const int width = kept_width(plane, robust != 0);
    const bool ranks = lag_run(ctx);
    const int nb = red_blocks(n);
    TRY(ctx->kept_mask.grow(ctx, (n + 63) / 64));
    if (gated) TRY(ctx->gate_flags.grow(ctx, n));
    TRY(ctx->kept_part.grow(ctx, (size_t)kRedMaxBlocksCap * kRobustPlaneSums));
    TRY(ctx->kept_state.grow(ctx, 1));
    TRY(ctx->h_kept.grow(ctx, 1));
    TRY(ctx->h_ktrace.grow(ctx, trace_entries(max_iter)));
    if (robust) {
        TRY(ctx->h_wtrace.grow(ctx, trace_entries(max_iter)));
        TRY(ctx->h_ptrace.grow(ctx, trace_entries(max_iter)));
    }
    if (trim) {
        TRY(ctx->h_ctrace.grow(ctx, trace_entries(max_iter)));
        TRY(ctx->trim_keys.grow(ctx, n));
        TRY(ctx->trim_bins.grow(ctx, kSelectBins));
        TRY(ctx->trim_bins_d.grow(ctx, kSelectBins));
        TRY(ctx->trim_state.grow(ctx, 1));
        TRY(ctx->trim_cut.grow(ctx, 1));
        HIPCHK(hipMemsetAsync(ctx->trim_bins, 0, sizeof(unsigned) * kSelectBins, ctx->st)); // (each pick leaves them zero)
    }
    if (uniq) TRY(ctx->uniq_best.grow(ctx, ctx->nm));
    std::memset(ctx->h_kept, 0, sizeof(GateState));
    HIPCHK(hipMemsetAsync(ctx->kept_state, 0, sizeof(GateState), ctx->st));
    IterState *sd = ctx->iter_state;
    launch_run_init(sd, ctx->amb_count, ctx->st, ctx->c); // (the first gated iteration's pre-pass sums around the model's centre)
    if (ctx->digest_cap) HIPCHK(hipMemsetAsync(ctx->digest, 0, sizeof(unsigned long long) * 3 * ctx->digest_cap, ctx->st));
    const int *digest_order = ctx->scene_slot ? ctx->s_order : nullptr;
    ctx->stats.run_path_bits = 0;
    // The metric's launches: the moments' pass with its fold, and the fold of the moments' partial
    // rows and / or the step on the folded (all ranks') sums.  Their arguments hold for the run, but
    // for what a search leaves (it may allocate idx and the kd-ordered form): taken at each pass.
    // The symmetric form: u0 in the scene's current order (a scene in slot order: its copy in that
    // order, made once per order), and the context's total at the run's start, which the kernels
    // compose the run's own onto.
    SymmArgs sy = {};
    if (symm || gicp) {
        const DevCloud *U = nullptr;
        TRY(scene_normals_current(ctx, &U));
        sy.ux = U->x, sy.uy = U->y, sy.uz = U->z;
        sy.st = sd;
        sy.have_q0 = ctx->tot_n > 0 ? 1 : 0;
        for (int k = 0; k < 9; ++k) sy.q0[k] = sy.have_q0 ? ctx->tot[1 + k] : (k % 4 == 0 ? 1.0 : 0.0);
    }
    GicpArgs ga = {}; // (the plane-to-plane form: the same u0 and total; read by its two launchers alone)
    if (gicp) ga = {sy, 1.0 - ctx->plane_to_plane};
    KeptPass pass = {};
    pass.plane = plane;
    pass.symm = symm ? &sy : nullptr;
    pass.gicp = gicp ? &ga : nullptr;
    pass.robust_kind = robust;
    pass.k = ctx->robust_k, pass.k2 = ctx->robust_k2;
    pass.m4 = ctx->m4, pass.n4 = ctx->n4;
    pass.px = P.x, pass.py = P.y, pass.pz = P.z, pass.n = (int)n;
    pass.yx = Y.x, pass.yy = Y.y, pass.yz = Y.z;
    pass.st_dev = sd;
    pass.D = D;
    pass.cut = trim ? ctx->trim_cut : nullptr;
    pass.best = uniq ? ctx->uniq_best : nullptr;
    pass.mask = ctx->kept_mask, pass.partials = ctx->kept_part;
    pass.st = ctx->st;
    KeptStep fold = {};
    fold.plane = plane, fold.robust = robust != 0, fold.trim_few = trim_few;
    fold.symm = symm;
    fold.sums = ctx->sums, fold.amb_count = ctx->amb_count;
    fold.st_dev = sd, fold.h_state = ctx->h_iter.dev();
    fold.gate = ctx->kept_state, fold.h_gate = ctx->h_kept.dev();
    fold.h_wtrace = ctx->h_wtrace.dev(), fold.h_ptrace = ctx->h_ptrace.dev();
    fold.st = ctx->st;
    for (int k = 0; k < 3; ++k) pass.c[k] = fold.c[k] = ctx->c[k];
    const auto moments = [&](bool y_ready, bool do_step) {
        pass.idx = ctx->idx;
        pass.kpos = ctx->kpos_valid ? ctx->kpos : nullptr;
        pass.m4kd = ctx->m4kd;
        if (gicp) launch_gicp_moments(pass, y_ready);
        else launch_kept_moments(pass, y_ready);
        launch_kept_step(fold, ctx->kept_part, nb, do_step);
    };
    LoopRun r; // (the ring and the after-search bookkeeping only: no timing, no policy)
    r.ctx = ctx;
    r.n = n;
    r.digest_order = digest_order;
    while (!r.stop && r.waited < max_iter) {
        if (r.enqueued < max_iter && r.enqueued - r.waited <= kAhead) {
            // 1. correspondences (a search queued behind the iteration that froze the run returns at once)
            const SeedState ws;
            ctx->second_pass_items = 0;
            TRY(nn_search_begin(ctx, P, n, ctx->seeds_valid, nullptr, nullptr, false, &ws, &sd->done, ctx->scene_slot,
                                false, nullptr));
            TRY(after_search(r, r.enqueued, false, -1));
            // Point-to-point, the first iteration's shifts: a pre-pass of the same moments around c
            // gives the kept pairs' centroids (all ranks'), and the pass below sums around those --
            // around c a scan D from the model's centre cancels (D / sigma)^2 of the moments'
            // precision.  Later iterations get their shifts from the Horn step before them.
            const bool pre_pass = !plane && r.enqueued == 0;
            // The trim's cut: the keys pass (y stored, each point's d2 key), then the selection of
            // the T-th smallest key over all ranks into *cut; the moments below stream the stored y.
            if (trim) {
                launch_select_keys(ctx->idx, ctx->m4, P.x, P.y, P.z, (int)n, Y.x, Y.y, Y.z, &sd->done, ctx->trim_keys, ctx->st,
                                   ctx->kpos_valid ? ctx->kpos : nullptr, ctx->m4kd, ctx->y_ready);
                LAUNCHCHK("select_keys");
                if (!ranks) {
                    launch_select_kth(ctx->trim_keys, (int)n, (unsigned long long)T, ctx->trim_state, &sd->done, ctx->trim_bins,
                                      ctx->trim_cut, sd, ctx->h_ctrace.dev(), ctx->st);
                    LAUNCHCHK("select_kth");
                }
                for (int pass = 0; ranks && pass < kSelectPasses; ++pass) { // (each pass's bins all-reduced before its pick)
                    launch_select_count(ctx->trim_keys, (int)n, pass, ctx->trim_state, &sd->done, ctx->trim_bins, ctx->st);
                    launch_select_bins(ctx->trim_bins, ctx->trim_bins_d, &sd->done, ctx->st);
                    LAUNCHCHK("select_bins");
                    TRY(allreduce(ctx, ctx->trim_bins_d, kSelectBins));
                    launch_select_pick(ctx->trim_bins, ctx->trim_bins_d, pass, (unsigned long long)T, ctx->trim_state, &sd->done,
                                       ctx->trim_cut, sd, ctx->h_ctrace.dev(), ctx->st);
                    LAUNCHCHK("select_pick");
                }
            }
            // One-to-one: each model point's smallest d2 key into best (all ones before); with a trim
            // the keys pass above has stored y and the keys, else this pass stores y.
            if (uniq) {
                HIPCHK(hipMemsetAsync(ctx->uniq_best, 0xff, sizeof(unsigned long long) * ctx->nm, ctx->st));
                if (trim)
                    launch_unique_min_keys(ctx->idx, ctx->trim_keys, (int)n, &sd->done, ctx->uniq_best, (int)ctx->nm, ctx->st);
                else
                    launch_unique_min(ctx->idx, ctx->m4, P.x, P.y, P.z, (int)n, Y.x, Y.y, Y.z, &sd->done, ctx->uniq_best,
                                      (int)ctx->nm, ctx->st, ctx->kpos_valid ? ctx->kpos : nullptr, ctx->m4kd, ctx->y_ready);
                LAUNCHCHK("unique_min");
            }
            const bool y_stored = ctx->y_ready || trim || uniq;
            if (pre_pass) {
                moments(y_stored, false); // (the fold alone)
                LAUNCHCHK("gated_moments (first shifts)");
                if (ranks) TRY(allreduce(ctx, ctx->sums, width));
                launch_kept_first_shift(sd, ctx->sums, robust ? kRobustGateW : kGateCount, ctx->st);
                LAUNCHCHK("gated_first_shift");
            }
            // 2-4. the gate, the kept pairs' sums and count, the metric's step
            // (after the pre-pass y = m[idx] is stored: the pass streams it)
            moments(y_stored || pre_pass, !ranks);
            LAUNCHCHK(plane ? "plane_moments" : "gated_moments");
            if (ranks) {
                TRY(allreduce(ctx, ctx->sums, width));
                launch_kept_step(fold, nullptr, 0, true);
                LAUNCHCHK(plane ? "plane_solve" : "gated_horn");
            }
            // 5-6. every point moves; the kept points' residual; err = (e + e) / K
            if (gicp)
                launch_gicp_transform(P.x, P.y, P.z, Y.x, Y.y, Y.z, (int)n, &sd->xf, &sd->done, need_p32 ? P.f : nullptr,
                                      ctx->kept_mask, ctx->idx, ctx->n4, ctx->partials, ctx->st, ga);
            else
                launch_kept_transform(P.x, P.y, P.z, Y.x, Y.y, Y.z, (int)n, &sd->xf, &sd->done, need_p32 ? P.f : nullptr,
                                      ctx->kept_mask, ctx->idx, plane ? ctx->n4 : nullptr, ctx->partials, ctx->st,
                                      symm ? &sy : nullptr);
            if (!need_p32) ctx->p32_stale = true;
            const int sl = r.enqueued % kRing;
            r.slot_ticket[sl] = ++ctx->flag_ticket;
            const auto err = [&](const double *part, int nblocks, bool do_step) {
                launch_gated_err(part, nblocks, ctx->sums, do_step, threshold, max_iter, ctx->err_trace_dev, sd, ctx->kept_state,
                                 ctx->h_ktrace.dev(), ctx->h_flags.dev() + 4 * sl, r.slot_ticket[sl], ctx->h_iter.dev(), ctx->h_trace.dev(),
                                 ctx->st);
            };
            err(ctx->partials, nb, !ranks);
            LAUNCHCHK(plane ? "plane_transform" : "gated_transform");
            if (ranks) {
                TRY(allreduce(ctx, ctx->sums + kSumErr, 1));
                err(nullptr, 0, true);
                LAUNCHCHK(plane ? "plane_err" : "gated_err");
            }
            ++r.enqueued;
            continue;
        }
        TRY(wait_one(r));
    }
    // with the gate on: the last gate evaluated, as flags in the caller's point order (icp_get_inliers)
    if (gated && r.enqueued > 0) {
        launch_gated_unpack(ctx->kept_mask, digest_order, (int)n, ctx->gate_flags, ctx->st);
        LAUNCHCHK("gated_unpack");
    }
    HIPCHK(hipStreamSynchronize(ctx->st)); // (the iteration queued behind the last one drains)
    // nothing of a transform is carried to the next run: it starts from the correspondences alone
    ctx->seedd_valid = false;
    ctx->last_far = -1;
    ctx->last_q2 = -1;
    ctx->second_pass_items = 0;
    const GateState hk = *ctx->h_kept;
    if (gated && r.enqueued > 0) { // (the mapped buffers are the next run's, gated or not)
        ctx->gate_have = true;
        ctx->gate_K = hk.K;
        ctx->gate_ktrace.assign(ctx->h_ktrace.get(), ctx->h_ktrace + ctx->h_iter->iter);
    }
    if (trim && r.enqueued > 0) { // (icp_get_trim_trace: the recorded iterations' C)
        ctx->trim_have = true;
        ctx->trim_ctrace.assign(ctx->h_ctrace.get(), ctx->h_ctrace + ctx->h_iter->iter);
    }
    if (robust && r.enqueued > 0) { // (icp_get_robust_trace: the recorded iterations' W and K+)
        ctx->robust_have = true;
        ctx->robust_wtrace.assign(ctx->h_wtrace.get(), ctx->h_wtrace + ctx->h_iter->iter);
        ctx->robust_ptrace.assign(ctx->h_ptrace.get(), ctx->h_ptrace + ctx->h_iter->iter);
    }
    TRY(finish_run(ctx, threshold, err_trace, res, wall0));
    const std::string trimmed = (trim ? " (the trim keeps T = " + std::to_string(T) + " of " + std::to_string(ctx->np_total) +
                                            " pairs, ties at the cut included)"
                                      : std::string()) +
                                (uniq ? " (one-to-one is on: a model point keeps its closest pair alone)" : "");
    if (hk.status == kGateTooFew && robust)
        return fail(ctx, ICP_E_TOO_FEW_POINTS,
                    "icp_run: iteration " + std::to_string(hk.fail_iter) + " kept K = " + std::to_string(hk.K) +
                        " pairs, K+ = " + std::to_string(hk.Kpos) + " of them with a robust weight > 0; " +
                        (plane ? "the point-to-plane metric needs at least 6 of both" : "need at least 4 of both") + trimmed);
    if (hk.status == kGateTooFew)
        return fail(ctx, ICP_E_TOO_FEW_POINTS,
                    "icp_run: iteration " + std::to_string(hk.fail_iter) + " kept K = " + std::to_string(hk.K) +
                        (plane ? " pairs; the point-to-plane metric needs at least 6"
                               : trim || (uniq && D == HUGE_VAL) ? " pairs; need at least 4"
                                      : " pairs within the max correspondence distance; need at least 4") +
                        trimmed);
    if (hk.status == kPlaneDegenerate) {
        char piv[32];
        std::snprintf(piv, sizeof(piv), "%.3g", hk.min_pivot);
        return fail(ctx, ICP_E_DEGENERATE,
                    "icp_run: iteration " + std::to_string(hk.fail_iter) +
                        " has a degenerate " + (gicp ? "plane-to-plane" : "point-to-plane") + " system (smallest pivot " +
                        piv + ", K = " +
                        std::to_string(hk.K) + ")");
    }
    return ICP_OK;
}

// ---- the set-up ------------------------------------------------------------------------

// The argument checks, the loop state, the mapped mirrors and the flag ring, the seed arguments,
// the timing events and the scene's fp32 copy: what every loop of icp_run needs (run_kept and
// run_persistent too)
int run_setup_buffers(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    TRY(check_ready(ctx, true));
    TRY(scene_revert_now(ctx));
    // alignement_check (gpu.cc:54-62)
    if (ctx->np_total != ctx->nm && !ctx->allow_unequal)
        return fail(ctx, ICP_E_SIZE_MISMATCH, "Point sets need to have the same number of points.");
    if (ctx->np_total < 4) return fail(ctx, ICP_E_TOO_FEW_POINTS, "Need at least 4 point pairs");

    r.wall0 = std::chrono::steady_clock::now();
    const size_t n = r.n = ctx->scene.n;
    r.N = (double)ctx->np_total;
    r.lag = lag_run(ctx);
    r.tk = run_test_knobs();
    DevCloud &P = ctx->scene;
    TRY(ctx->iter_state.grow(ctx, 1));
    TRY(ctx->h_iter.grow(ctx, 1));
    TRY(ctx->h_trace.grow(ctx, trace_entries(r.max_iter)));
    std::memset(ctx->h_iter, 0, sizeof(IterState));
    if (!ctx->h_flags) {
        TRY(ctx->h_flags.grow(ctx, 4 * kRing));
        std::memset(ctx->h_flags, 0, sizeof(int) * 4 * kRing);
    }
    // seeded f16 searches: each transform writes the next search's seeds (no seed kernel)
    r.fuse_seeds = ctx->nn_mode == ICP_NN_CERTIFIED && level1_kind(ctx, n) >= 2;
    if (r.fuse_seeds) {
        TRY(ctx->seed16.grow(ctx, n));
        r.sa.seed16 = ctx->seed16;
        for (int a = 0; a < 3; ++a) r.sa.c[a] = ctx->c[a];
        r.sa.scale = ctx->scale16;
        if (level1_kind(ctx, n) == 3 && bundle_v2()) { // the bundle filter's seed distances too
            TRY(ctx->b_seedd.grow(ctx, n));
            r.sa.seedd = ctx->b_seedd;
        }
    }
    TRY(ctx->err_trace_dev.grow(ctx, (size_t)(r.max_iter > 0 ? r.max_iter : 1)));
    while (ctx->iter_ev.size() < 5 * (size_t)kRing) { // (nn begin, nn end, -, all-reduce begin, end) per slot
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
        ctx->iter_ev.push_back(e);
    }
    // the scene's fp32 copy is read only by the fp32 filters (level 1 VALU / f32 MFMA), their
    // windowed resolve and the one-launch paths: other runs let the transform skip it (16 B a
    // point) and leave it to be refreshed here when a later run needs it
    r.need_p32 = (ctx->nn_mode == ICP_NN_CERTIFIED && level1_kind(ctx, n) <= 1 &&
                  ctx->nn_variant != ICP_NN_VARIANT_GRID) ||
                 n <= (size_t)kTailMaxBlocks * kBlock;
    if (r.need_p32 && ctx->p32_stale) {
        if (n) launch_make_f32(P.x, P.y, P.z, n, ctx->c[0], ctx->c[1], ctx->c[2], P.f, ctx->st);
        LAUNCHCHK("make_f32");
        ctx->p32_stale = false;
    }
    return ICP_OK;
}

// The scene into slot order where it applies, and the search policy of AUTO at the bundle filter's
// sizes (the scene in slot order): a seeded search takes the grid (grid_seeded_search) instead of
// the bundle cascade when the last transform the host has seen left at most n/32 points farther
// than 1.5 grid cells from their correspondence (the queries whose box exceeds kSeededBox cells:
// the second, per-wave pass).  The decision for iteration k + 1 is taken when k is enqueued (k's
// transform writes the bundle's records and seeds only if k + 1 is a bundle search), on the count
// of an iteration one or two behind.  Before any count is seen: the count the last run ended with
// when this run continues it (carry), else the grid while the bundle images are still unbuilt
// (bundle_pending: the first search is then the unseeded grid search, nn_search_begin), else the
// bundle cascade.  A far count above the threshold builds the bundle images (ensure_bundle).  Both
// paths return the exact first minimum, so the trajectory is the same whichever runs.
// ICP_GRID_AUTO=0: always the bundle.
int run_setup_policy(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    const size_t n = r.n;
    const RunKnobs &k = run_knobs();
    if (want_slot_order(ctx, n)) TRY(scene_to_slot_order(ctx));
    if (ctx->scene_slot && ctx->nn_variant == ICP_NN_VARIANT_GRID && ctx->nn_mode == ICP_NN_CERTIFIED && !r.sa.seedd) {
        // the grid variant's seeded searches read the transform's seed distances too
        TRY(ctx->b_seedd.grow(ctx, n));
        r.sa.seedd = ctx->b_seedd;
    }
    r.digest_order = ctx->scene_slot ? ctx->s_order : nullptr;
    r.grid_policy = ctx->scene_slot && ctx->nn_mode == ICP_NN_CERTIFIED && ctx->nn_variant == ICP_NN_VARIANT_AUTO &&
                    level1_kind(ctx, n) == 3 && k.grid_auto;
    r.far_thr = std::max(16, (int)(n >> k.far_shift));
    // a run that continues the last one (the same resident scene, its seed distances written by
    // that run's last transform) starts from that run's last far count: its first searches need
    // not be the bundle cascade's
    r.carry = r.grid_policy && ctx->seeds_valid && ctx->seedd_valid;
    r.far_obs = r.carry ? ctx->last_far : -1;
    r.q2_obs = r.carry ? ctx->last_q2 : -1;
    r.grid_next = r.carry && r.far_obs >= 0 && r.far_obs <= r.far_thr;
    // The far count's rule: a moved point whose complete box around its seed distance, clamped to
    // the grid, exceeds kSeededBox cells -- the queries the seeded grid search could not take in
    // its walk.  Round 4 counted points farther than 1.5 cells from their correspondence, which
    // also counted the points outside the model's box whose clamped box is small: a C5 shard (3.9%
    // of its points outside, 0.9% with a big box) then built the bundle images for its first
    // iterations (15 ms of a 31 ms registration).  ICP_GRID_FAR=dist: the distance rule (A/B).
    if (r.grid_policy) {
        const double h = 1.0 / ctx->grid.inv_h;
        r.sa.far_acc = r.sa_grid.far_acc = &ctx->iter_state->far_acc;
        r.sa.far_d2 = r.sa_grid.far_d2 = 2.25 * h * h;
        if (!k.far_dist) {
            r.sa.far_gv = r.sa_grid.far_gv = grid_view(ctx);
            r.sa.far_box = r.sa_grid.far_box = kSeededBox;
        }
        r.sa_grid.seedd = r.sa.seedd; // (grid_seeded_search reads them: no gather of the seed point)
    }
    r.ws.seedd = r.carry;
    // A run that starts with the bundle images pending and nothing carried over has no far count
    // until its first iteration completes: the host waits for it before enqueuing the second, so
    // that the second search's path is decided on a count (a blind grid search right after the
    // first alignment scans boxes as big as the first transform's moves)
    // (only a shard against a model of at least twice its points, whose first transform leaves more
    // than n/32 points far -- C5's shards: 40,739 of 2^20 by a CPU model; a scene of
    // the model's size goes straight on to the grid -- C4: 107 big boxes, searched in the fused
    // kernel -- without the synchronisation)
    r.hold_first = r.grid_policy && !r.carry && ctx->bundle_pending && ctx->nm >= 2 * n;
    // the canonical schedule's path rule (canon_path): fold_far[j] = the far count mirrored with
    // iteration j's (lagged) error step -- transform j's, counted by iteration j + 1's search kernel
    // (all ranks'); hold_far = transform 0's, read by hold_first
    r.fold_far = std::vector<int>((size_t)std::max(r.max_iter, 1), -1);
    return ICP_OK;
}

// How the launch loop's steps are fused, the fused tail's snapshot, the digests, the timing sample.
int run_setup_steps(LoopRun &r, bool no_tail)
{
    icp_ctx *ctx = r.ctx;
    const size_t n = r.n;
    const RunKnobs &k = run_knobs();
    // partials over several workgroups: the moments and / or the transform may fold their
    // partials in their own last workgroup (StepFold), and on one rank go on there to the Horn
    // step / the error step -- one launch fewer each, bit-identical.  ICP_FUSED_STEPS = bit 0:
    // the moments, bit 1: the transform; 0 (the default): the separate launches.  Measured at C4
    // (profiles/r04r): both fused 0.183 ms per iteration against 0.164 separate -- the last
    // workgroup's fold reads the rows coherently (sc1: past L2), and the moments kernel with the
    // Horn solve inlined holds 128 VGPRs
    r.fused_moments = (k.fused_steps & 1) && red_blocks(n) > 1;
    r.fused_steps = (k.fused_steps & 2) && red_blocks(n) > 1; // (the transform's)
    // multi-rank runs: the transform's residual partials wait in err_part, and the next
    // iteration's moments fold folds them too (launch_reduce_pair: one launch fewer an iteration,
    // the same bits); the last iteration folds its own before the final all-reduce
    r.err_pair = k.err_pair && r.lag && red_blocks(n) > 1 && !r.fused_steps && !r.fused_moments;
    if (r.err_pair) TRY(ctx->err_part.grow(ctx, (size_t)kRedMaxBlocksCap));
    if ((r.fused_steps || r.fused_moments) && !ctx->fold_ticket) {
        TRY(ctx->fold_ticket.grow(ctx, 2));
        HIPCHK(hipMemsetAsync(ctx->fold_ticket, 0, 2 * sizeof(unsigned), ctx->st));
    }
    // mid-size single-rank runs: iterations >= 2 end in ONE fused launch (moments ... error step)
    // (ICP_RUN_MODE=launches forces the separate launches here; =persistent leaves icp_set_run_mode's)
    r.tail_blocks = red_blocks(n);
    r.fused_tail = !no_tail && k.run_mode != ICP_RUN_LAUNCHES && ctx->run_mode != ICP_RUN_LAUNCHES && !r.lag &&
                   n > (size_t)kRedSingle && r.tail_blocks <= kTailMaxBlocks && r.tail_blocks <= ctx->n_cu * 3 / 4;
    r.seeds_at_start = ctx->seeds_valid;
    if (r.fused_tail) {
        TRY(ctx->tail_part.grow(ctx, (size_t)19 * kTailMaxBlocks));
        TRY(ctx->tail_sync.grow(ctx, kPersistSyncWords));
        HIPCHK(hipMemsetAsync(ctx->tail_sync, 0, kPersistSyncWords * sizeof(unsigned), ctx->st));
        ctx->h_flags[11] = 0; // its barriers' abort word (mapped host)
        TRY(ctx->tail_backup.grow(ctx, n * (3 * sizeof(double) + sizeof(float4) + sizeof(int))));
        TRY(tail_snapshot(ctx, n, r.seeds_at_start, false));
    }
    if (ctx->digest_cap) HIPCHK(hipMemsetAsync(ctx->digest, 0, sizeof(unsigned long long) * 3 * ctx->digest_cap, ctx->st));
    r.timing_stride = k.timing_stride ? k.timing_stride : 8; // (is_timed)
    r.timing_phase = r.timing_stride > 1 ? (int)(ctx->runs++ % (unsigned)r.timing_stride) : 0;
    ctx->stats.run_path_bits = 0;
    return ICP_OK;
}

// A scene in slot order (C4, C5, their shards): the canonical schedule (icp_canon.h).  The
// transform of iteration k - 1 is enqueued at the start of iteration k, right before its
// search, in the form that search reads; its residual and k's moments go to the canonical
// rows, and ONE fold launch ends iteration k with k - 1's error step and k's Horn step (with
// ranks: the fold, the all-reduce of the 18 sums, the error + Horn step) -- the error test
// runs one iteration late, as the multi-rank loop's always did, and the scene freezes at the
// same point.  Every search path adds to the same rows in the same order, so the NN variants'
// trajectories stay bitwise equal.  ICP_CANON=0: the round-4 schedule (A/B).
// Here: its rows, the first shift of p, the certificate's buffers, the fold's arguments.
int run_setup_canon(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    const size_t n = r.n;
    const RunKnobs &k = run_knobs();
    DevCloud &P = ctx->scene;
    IterState *sd = ctx->iter_state;
    r.canon = k.canon && ctx->scene_slot && n > 0;
    if (r.canon) {
        TRY(ctx->canon_rowbuf.grow(ctx, (size_t)canon_strands(n) * kCanonCols)); // (rows, or strands)
        TRY(ctx->h_far.grow(ctx, 1));
        // the first iteration's shift of p: the scene's centroid (all ranks'), where run_init put the
        // model's centre c -- a scene far from the model would otherwise cancel (D / sigma)^2 of the
        // one-pass moments' precision (the shift of y follows the first search: the mean of a sample
        // of its correspondences, launch_first_shift_y_sample in enqueue_canon_search)
        launch_sum3(P.x, P.y, P.z, (int)n, red_target(ctx, n, ctx->sums + kSumScene), ctx->st, 1);
        red_finish(ctx, n, 3, ctx->sums + kSumScene);
        LAUNCHCHK("scene_sum");
        TRY(allreduce(ctx, ctx->sums + kSumScene, 3));
        // (set with the shift of y, after the first search; ICP_FIRST_K1=1 sums its first moments
        // inside that search's launch and needs it now: its shift of y stays c)
        if (k.first_k1) {
            launch_first_shift(sd, ctx->sums + kSumScene, r.N, ctx->st);
            LAUNCHCHK("first_shift");
        }
    }
    // ICP_CERT=0: every query walks (A/B); ICP_CERT_TWO=0: the one-point form;
    // ICP_CERT_SKIN: the walk's extra radius in grid cells (default 0.25).
    if (r.canon && k.cert && k.grid_iter && ctx->g_pts32) {
        TRY(ctx->cert_state.grow(ctx, n));
        // the counts accumulate on the device over the runs of one scene size (64-bit: no wrap),
        // read when the stats are; another size folds them into the stats first (a synchronisation
        // the runs of a registration loop do not pay: 60 us a run at C4, profiles/r06/r06fold3)
        const int crows = canon_strands(n); // (rows or strands: nn_grid_iter2_kernel NWG)
        // (3 words a strand: the two counts, then walk_last and the order table, an int each)
        if (ctx->cert_counts_rows != crows) {
            TRY(fold_cert_counts(ctx));
            TRY(ctx->cert_counts.grow(ctx, 3 * (size_t)crows));
            HIPCHK(hipMemsetAsync(ctx->cert_counts, 0, 3 * (size_t)crows * sizeof(ctx->cert_counts[0]), ctx->st));
            ctx->cert_counts_rows = crows;
        }
        r.cert.state = ctx->cert_state;
        r.cert.two = k.cert_two;
        r.cert.skin = k.cert_skin / ctx->grid.inv_h;
        r.cert.counts = ctx->cert_counts;
        if (k.iter2_order) {
            r.cert.walk_last = (int *)(ctx->cert_counts + 2 * (size_t)crows);
            r.order.walk_last = r.cert.walk_last;
            r.order.order = r.cert.walk_last + crows;
            r.order.S = crows;
            r.order.L = nn_grid_iter_strand_run((int)n);
            r.order.form = k.iter2_order;
        }
    }
    // ICP_ITER_DEBUG=1: nn_grid_iter_kernel's phase clocks and counts, summed over the run, to stderr
    if (k.iter_debug && r.canon) {
        unsigned long long *&buf = knob_owner().iter_dbg;
        // (the diagnostic build, -DICP_ITER2_DBG=1: + four words a wave, nn_grid_iter2_kernel's records)
        if (!buf) HIPCHK(hipMalloc((void **)&buf, (16 + kIterDbgRec) * sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(buf, 0, 16 * sizeof(unsigned long long), ctx->st));
        r.iter_dbg = buf;
    }
    r.cs.N = r.N;
    r.cs.threshold = r.threshold;
    r.cs.max_iter = r.max_iter;
    r.cs.err_trace = ctx->err_trace_dev;
    r.cs.s = sd;
    r.cs.h_state = ctx->h_iter.dev();
    r.cs.h_trace = ctx->h_trace.dev();
    for (int a = 0; a < 3; ++a) r.cs.c[a] = ctx->c[a];
    r.cs.cnt = ctx->amb_count;
    if (!ctx->canon_ticket) {
        TRY(ctx->canon_ticket.grow(ctx, 1));
        HIPCHK(hipMemsetAsync(ctx->canon_ticket, 0, sizeof(int), ctx->st));
    }
    r.cs.fold_ticket = ctx->canon_ticket;
    return ICP_OK;
}

// Everything before the loop.  *handed: the run was another loop's (run_kept, run_persistent) and
// is over, with the returned code.
int run_setup(LoopRun &r, icp_ctx *ctx, int max_iter, double threshold, double *err_trace, icp_result *res,
              bool no_tail, bool *handed)
{
    r.ctx = ctx;
    r.max_iter = max_iter;
    r.threshold = threshold;
    // the two switches on the plane metric exclude each other: refused before anything changes
    if (ctx && ctx->metric == ICP_METRIC_POINT_TO_PLANE && ctx->plane_symmetric && ctx->plane_to_plane > 0.0)
        return fail(ctx, ICP_E_ARG, "icp_run: icp_set_plane_symmetric and icp_set_plane_to_plane are both on; the "
                                    "point-to-plane metric takes one form at a time");
    // one-to-one: the table's minimum is over one rank's points (a min-reduction over ranks is not
    // the engine's sum all-reduce): refused before anything is enqueued
    if (ctx && ctx->one_to_one && ctx->world > 1)
        return fail(ctx, ICP_E_ARG, "icp_run: icp_set_one_to_one is on with world_size > 1; the closest pair of a model "
                                    "point is chosen on one rank (ranks are not supported)");
    TRY(run_setup_buffers(r));
    *handed = true;
    // icp_set_metric, icp_set_max_distance, icp_set_robust, icp_set_trim, icp_set_one_to_one: the kept-pairs loop (never
    // the one-launch kernels or the fused iterations)
    if (ctx->metric == ICP_METRIC_POINT_TO_PLANE || ctx->gate_dmax > 0.0 || ctx->robust_kind != 0 || ctx->trim_fraction < 1.0 ||
        ctx->one_to_one)
        return run_kept(ctx, max_iter, threshold, err_trace, res, r.need_p32, r.wall0);
    {
        size_t lds = 0;
        bool mid = false;
        const int grid = persistent_grid(ctx, r.n, max_iter, &lds, &mid);
        if (grid) {
            const int rc = run_persistent(ctx, grid, lds, mid, max_iter, threshold, err_trace, res, r.wall0);
            if (rc != kPersistFallback) return rc;
        }
    }
    *handed = false;
    TRY(run_setup_policy(r));
    launch_run_init(ctx->iter_state, ctx->amb_count, ctx->st, ctx->c);
    TRY(run_setup_steps(r, no_tail));
    return run_setup_canon(r);
}

// ---- the canonical schedule (a scene in slot order) ---------------------------------------

// the canonical transform of the last Horn step's (s, R, t), in the form sa_t (its residual into
// the rows' kSumErr column, and what the next search reads)
int canon_transform(LoopRun &r, const SeedArgs &sa_t)
{
    icp_ctx *ctx = r.ctx;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    IterState *sd = ctx->iter_state;
    launch_canon_transform(P.x, P.y, P.z, Y.x, Y.y, Y.z, (int)r.n, &sd->xf, &sd->done, r.need_p32 ? P.f : nullptr,
                           ctx->canon_rowbuf, sa_t, ctx->st);
    LAUNCHCHK("canon_transform");
    if (!r.need_p32) ctx->p32_stale = true;
    r.ws = seed_state_of(sa_t);
    r.xf_pending = false;
    return ICP_OK;
}

// the table the fold after a fused launch is to build (IterOrder), or none; consumes walk_written
IterOrder fold_order(LoopRun &r)
{
    const bool build = r.walk_written;
    r.walk_written = false;
    return build ? r.order : IterOrder{};
}

// canon: the error step of iteration `it` (ticket of its slot) after the fold of the rows --
// with the Horn step of the current iteration (horn) or alone (the run's last residual)
int canon_end(LoopRun &r, int it, bool horn, int slot)
{
    icp_ctx *ctx = r.ctx;
    IterState *sd = ctx->iter_state;
    CanonStep &cs = r.cs;
    const int sl = it % kRing;
    r.slot_ticket[sl] = ++ctx->flag_ticket;
    cs.hflag = ctx->h_flags.dev() + 4 * sl;
    cs.ticket = r.slot_ticket[sl];
    const int strands = r.rows_strands; // (the fused kernel wrote the rows as strands)
    r.rows_strands = 0;
    const IterOrder ord = fold_order(r);
    if (!r.lag) {
        r.order_ok = launch_canon_fold(ctx->canon_rowbuf, (int)r.n, ctx->sums, horn ? 1 : 2, cs, ctx->st, strands, ord);
        LAUNCHCHK("canon_fold");
        return ICP_OK;
    }
    r.order_ok = launch_canon_fold(ctx->canon_rowbuf, (int)r.n, ctx->sums, horn ? 0 : 3, cs, ctx->st, strands, ord);
    LAUNCHCHK("canon_fold");
    const bool tm = horn && slot >= 0 && r.ar_timed[slot];
    if (tm) HIPCHK(hipEventRecord(ctx->iter_ev[5 * slot + 3], ctx->st));
    // (the policy's runs: the far count rides along as a 19th sum, so every rank decides on the
    // same global count -- canon_path's rule)
    TRY(horn ? allreduce(ctx, ctx->sums, r.grid_policy ? kNumSums + 1 : kNumSums)
             : allreduce(ctx, ctx->sums + kSumErr, 1));
    if (tm) HIPCHK(hipEventRecord(ctx->iter_ev[5 * slot + 4], ctx->st));
    if (horn)
        launch_err_horn_step(ctx->sums, r.N, r.threshold, r.max_iter, ctx->err_trace_dev, sd, cs.hflag, cs.ticket,
                             ctx->h_iter.dev(), ctx->h_trace.dev(), ctx->c, 1, ctx->amb_count, ctx->st,
                             r.grid_policy ? 1 : 0);
    else
        launch_err_step(ctx->sums, r.N, r.threshold, r.max_iter, ctx->err_trace_dev, sd, cs.hflag, cs.ticket,
                        ctx->h_iter.dev(), ctx->h_trace.dev(), ctx->st, nullptr, 0);
    LAUNCHCHK("err_step");
    return ICP_OK;
}

// canon: a run's first iteration ends in the Horn step alone -- its moments in one pass
// around the shifts run_init set (c), no error step before it (round 4: the reference's two
// passes and an unshifted Horn step, four more launches)
int canon_first(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    const int strands = r.rows_strands;
    r.rows_strands = 0;
    const IterOrder ord = fold_order(r);
    if (!r.lag) {
        r.order_ok = launch_canon_fold(ctx->canon_rowbuf, (int)r.n, ctx->sums, 4, r.cs, ctx->st, strands, ord);
        LAUNCHCHK("canon_fold");
        return ICP_OK;
    }
    r.order_ok = launch_canon_fold(ctx->canon_rowbuf, (int)r.n, ctx->sums, 0, r.cs, ctx->st, strands, ord);
    LAUNCHCHK("canon_fold");
    TRY(allreduce(ctx, ctx->sums, kNumSums));
    launch_horn_step(ctx->sums, r.N, ctx->c, true, ctx->amb_count, ctx->iter_state, ctx->st);
    LAUNCHCHK("horn_step");
    return ICP_OK;
}

// the end of a canonical run: the last transform and its residual's error step
int finish_canon(LoopRun &r)
{
    TRY(canon_transform(r, r.grid_policy ? r.sa_grid : SeedArgs{}));
    return canon_end(r, r.enqueued - 1, false, -1);
}

// What every form of the canonical iteration ends in, its moments in the rows: the fold with the
// previous iteration's error step and this one's Horn step (the first iteration: the Horn step
// alone), then the run's end if this was the last iteration.
int canon_tail(LoopRun &r, int slot, bool timed)
{
    if (r.enqueued == 0) {
        TRY(canon_first(r));
    } else {
        r.ar_timed[slot] = timed && r.lag;
        TRY(canon_end(r, r.enqueued - 1, true, slot));
    }
    r.xf_pending = true;
    ++r.enqueued;
    if (r.enqueued == r.max_iter) TRY(finish_canon(r));
    return ICP_OK;
}

// The path of search k: on the far count of transform k - 3 (counted by iteration
// k - 2's search kernel, mirrored with iteration k - 3's lagged error step; all
// ranks' on several: kSumFar), which the host has waited for before enqueuing k
// (run_loop: iteration k - 1 may still run meanwhile) -- the same count whatever the
// host's lead over the device, and on every rank.  Before that count exists:
// transform 0's count when hold_first read it, else the count the last run ended
// with (carry), else the grid while the bundle images are pending.
int canon_path(LoopRun &r, bool *grid_out)
{
    icp_ctx *ctx = r.ctx;
    const int far_dec = r.enqueued >= 3 ? r.fold_far[r.enqueued - 3] : r.hold_far >= 0 ? r.hold_far : r.carry ? ctx->last_far : -1;
    bool grid_c = r.grid_policy && (far_dec >= 0 ? far_dec <= r.far_thr : r.enqueued == 0 ? r.grid_next : ctx->bundle_pending);
    if (r.xf_pending && r.hold_first && r.enqueued == 1 && far_dec < 0) {
        // the images pending and no count yet: the first transform, then its far count
        // (all ranks'), before the second search's path is chosen (one synchronisation a run)
        TRY(canon_transform(r, r.sa_grid));
        HIPCHK(hipMemcpyAsync(ctx->h_far, &ctx->iter_state->far_acc, sizeof(int), hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
        r.hold_far = *ctx->h_far;
        if (r.lag) TRY(global_count(ctx, &r.hold_far));
        r.far_obs = r.hold_far;
        grid_c = r.hold_far <= r.far_thr;
    }
    *grid_out = grid_c;
    return ICP_OK;
}

// The diagnostic build (-DICP_ITER2_DBG=1) with ICP_ITER_DEBUG=2 and ICP_ITER_TAIL_DUMP=<file>:
// the last fused launch's wave records (entry time, exit time at 100 MHz, strand << 32 | XCD << 16
// | walkers, tasks << 48 | walk batches << 32 | pair tests -- four words a block) appended to the
// file after a header (magic, iteration, blocks, n); tools/iter_tail.py reads it.  The launch's
// counts, which one-strand workgroups leave in their records, are added to cnt.  The stream is
// idle here (ICP_ITER_DEBUG=2 synchronises).
int dump_wave_records(LoopRun &r, unsigned long long cnt[4])
{
    if (!ICP_ITER2_DBG || r.rows_strands <= 0) return ICP_OK;
    icp_ctx *ctx = r.ctx;
    const size_t nb = (size_t)r.rows_strands;
    std::vector<unsigned long long> h(4 + 4 * nb);
    h[0] = 0x4c494154524554ull; // ("ITERTAIL")
    h[1] = (unsigned long long)r.enqueued;
    h[2] = nb;
    h[3] = r.n;
    HIPCHK(hipMemcpy(h.data() + 4, r.iter_dbg + 16, 4 * nb * sizeof(h[0]), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < nb; ++b) {
        const unsigned long long w = h[4 + 4 * b + 2], c = h[4 + 4 * b + 3];
        cnt[0] += c >> 48;
        cnt[1] += w & 0xffffull;
        cnt[2] += (c >> 32) & 0xffffull;
        cnt[3] += c & 0xffffffffull;
    }
    const char *path = getenv("ICP_ITER_TAIL_DUMP");
    if (!path) return ICP_OK;
    FILE *f = fopen(path, "ab");
    if (!f) return fail(ctx, ICP_E_HIP, "ICP_ITER_TAIL_DUMP: cannot open the file");
    fwrite(h.data(), sizeof(h[0]), h.size(), f);
    fclose(f);
    return ICP_OK;
}

// the fused grid iteration's launch (nn_grid_iter_kernel); xform 0: no pending transform
void launch_fused_iter(LoopRun &r, int xform)
{
    icp_ctx *ctx = r.ctx;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    IterState *sd = ctx->iter_state;
    r.cert.order = r.order_ok ? r.order.order : nullptr;
    r.order_ok = false; // (the table was this launch's: the next fold builds the next one)
    r.cert_prev = launch_nn_grid_iter((int)r.n, P.x, P.y, P.z, Y.x, Y.y, Y.z, ctx->idx, sd, r.need_p32 ? P.f : nullptr,
                                      grid_view(ctx), kSeededBox, grid_budget(ctx), (int)ctx->nm, ctx->m4,
                                      ctx->canon_rowbuf, r.grid_policy ? &sd->far_acc : nullptr,
                                      r.sa_grid.far_box > 0 ? -1.0 : r.sa_grid.far_d2, ctx->amb_count + 2, ctx->st,
                                      r.iter_dbg, xform, r.cert, &r.rows_strands);
    r.walk_written = r.cert_prev && r.cert.valid && r.cert.walk_last && r.rows_strands == r.order.S;
}

// a fresh run's first iteration on the grid as ONE launch too: cell seeds (their
// coordinates as the correspondences), then the fused kernel with no pending
// transform -- the search nn_search_begin would run (its unseeded grid path) and the
// one-pass moments, into the same rows
// (ICP_FIRST_K1=1; measured slower: the cell seeds' big boxes, 0.4% of the queries, are
// each the whole owning wave's serial work there, where the seeded pass queues them for
// a second pass of one wave each -- first iteration 0.53 against 0.37 ms, profiles/r05ab)
int enqueue_canon_first_k1(LoopRun &r, int slot, bool timed)
{
    icp_ctx *ctx = r.ctx;
    const size_t n = r.n;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    TRY(ctx->idx.grow(ctx, n));
    launch_nn_grid_cell_seed((int)n, P.x, P.y, P.z, grid_view(ctx), (int)ctx->nm, ctx->idx, nullptr, ctx->st, Y.x, Y.y,
                             Y.z);
    LAUNCHCHK("nn_grid_cell_seed");
    if (timed) HIPCHK(hipEventRecord(ctx->iter_ev[5 * slot], ctx->st));
    r.cert.valid = 0;
    r.cert.skin = run_knobs().cert_skin1 / ctx->grid.inv_h;
    launch_fused_iter(r, 0);
    LAUNCHCHK("nn_grid_iter (first)");
    if (timed) HIPCHK(hipEventRecord(ctx->iter_ev[5 * slot + 1], ctx->st));
    r.ws = SeedState{};
    TRY(after_search(r, r.enqueued, true, slot));
    return canon_tail(r, slot, false); // (the first iteration: no all-reduce is timed)
}

// the grid's iterations as ONE launch: the pending transform, the seeded search
// of every point and the moments (nn_grid_iter_kernel)
int enqueue_canon_fused(LoopRun &r, int slot, bool timed)
{
    icp_ctx *ctx = r.ctx;
    const RunKnobs &k = run_knobs();
    if (timed) HIPCHK(hipEventRecord(ctx->iter_ev[5 * slot], ctx->st));
    r.cert.valid = r.cert_prev ? 1 : 0;
    r.cert.skin = (r.cert_prev ? k.cert_skin : k.cert_skin1) / ctx->grid.inv_h;
    launch_fused_iter(r, 1);
    if (r.iter_dbg && k.iter_debug == 2) { // (ICP_ITER_DEBUG=2: each launch's counts, synchronising)
        unsigned long long h[16];
        HIPCHK(hipStreamSynchronize(ctx->st));
        HIPCHK(hipMemcpy(h, r.iter_dbg, sizeof(h), hipMemcpyDeviceToHost));
        TRY(dump_wave_records(r, h));
        fprintf(stderr, "[iter2_debug] it %d tasks %llu walkers %llu batches %llu pair tests %llu (lane 0's)\n",
                r.enqueued, h[0], h[1], h[2], h[3]);
        HIPCHK(hipMemset(r.iter_dbg, 0, sizeof(h)));
    }
    LAUNCHCHK("nn_grid_iter");
    if (timed) HIPCHK(hipEventRecord(ctx->iter_ev[5 * slot + 1], ctx->st));
    if (!r.need_p32) ctx->p32_stale = true;
    r.ws = SeedState{}; // (no seed distances written: the next grid iteration computes its own)
    r.xf_pending = false;
    TRY(after_search(r, r.enqueued, true, slot));
    return canon_tail(r, slot, timed);
}

// the generic form: the pending transform in the form this search reads, the search
// (nn_search_begin), the moments into the rows (canon_moments)
int enqueue_canon_search(LoopRun &r, int slot, bool timed, bool grid_c)
{
    icp_ctx *ctx = r.ctx;
    const size_t n = r.n;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    IterState *sd = ctx->iter_state;
    r.cert_prev = false; // (any other search: the certificate's state is stale)
    r.walk_written = r.order_ok = false; // (and so is the dispatch order)
    if (r.xf_pending) { // the last Horn step's transform, in the form this search reads
        SeedArgs sa_t = grid_c ? r.sa_grid : r.sa;
        if (!grid_c) records_args(r, sa_t);
        TRY(canon_transform(r, sa_t));
    }
    const double *gs = r.ws.seedd && (grid_c || ctx->nn_variant == ICP_NN_VARIANT_GRID) ? r.sa.seedd : nullptr;
    ctx->second_pass_items = r.grid_policy && r.q2_obs >= 0 ? std::max(256, 4 * r.q2_obs) : 0;
    TRY(nn_search_begin(ctx, P, n, ctx->seeds_valid, timed ? ctx->iter_ev[5 * slot] : nullptr,
                        timed ? ctx->iter_ev[5 * slot + 1] : nullptr, false, &r.ws, &sd->done, ctx->scene_slot, grid_c,
                        gs));
    TRY(after_search(r, r.enqueued, false, slot));
    if (r.enqueued == 0) { // the first moments in one pass around the first shifts, then the Horn step
        // the shift of y: the mean of a sample of these correspondences (all ranks'), where
        // run_init put the model's centre c -- matched points that are a small part of the
        // model, D from c, would otherwise cancel (D / sigma)^2 of the y moments' precision
        launch_first_shift_y_sample(ctx->idx, ctx->m4, Y.x, Y.y, Y.z, (int)n, ctx->kpos_valid ? ctx->kpos : nullptr,
                                    ctx->m4kd, ctx->y_ready, ctx->sums + kSumYSample, r.lag ? nullptr : sd,
                                    ctx->sums + kSumScene, r.N, ctx->st);
        LAUNCHCHK("first_shift_y_sample");
        if (r.lag) {
            TRY(allreduce(ctx, ctx->sums + kSumYSample, 4));
            launch_first_shifts(sd, ctx->sums + kSumYSample, ctx->sums + kSumScene, r.N, ctx->st);
            LAUNCHCHK("first_shifts");
        }
    }
    launch_canon_moments(ctx->idx, ctx->m4, P.x, P.y, P.z, (int)n, Y.x, Y.y, Y.z, sd, ctx->canon_rowbuf, ctx->st,
                         ctx->kpos_valid ? ctx->kpos : nullptr, ctx->m4kd, ctx->y_ready);
    LAUNCHCHK("canon_moments");
    return canon_tail(r, slot, timed);
}

// One iteration of the canonical schedule: the path of its search, then one of its three forms.
int enqueue_canon(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    const RunKnobs &k = run_knobs();
    const int slot = r.enqueued % kRing;
    // 1. correspondences: compute_Y_w_opti(m, new_p, Y)  (gpu.cc:69)
    const bool timed = is_timed(r, r.enqueued);
    bool grid_c = false;
    TRY(canon_path(r, &grid_c));
    const bool k1_first =
        k.first_k1 && k.grid_iter && r.enqueued == 0 && !r.xf_pending && !ctx->seeds_valid && k.cell_seed &&
        ctx->nn_mode == ICP_NN_CERTIFIED && ctx->nn_rule == ICP_NN_RULE_SQUARED && ctx->g_pts32 &&
        (ctx->nn_variant == ICP_NN_VARIANT_GRID ||
         (ctx->nn_variant == ICP_NN_VARIANT_AUTO && ctx->bundle_pending && level1_kind(ctx, r.n) == 3));
    if (k1_first) return enqueue_canon_first_k1(r, slot, timed);
    const bool k1 = k.grid_iter && r.xf_pending && ctx->seeds_valid && r.enqueued > 0 &&
                    ctx->nn_mode == ICP_NN_CERTIFIED && ctx->nn_rule == ICP_NN_RULE_SQUARED &&
                    (grid_c || ctx->nn_variant == ICP_NN_VARIANT_GRID) && ctx->g_pts32;
    if (k1) return enqueue_canon_fused(r, slot, timed);
    return enqueue_canon_search(r, slot, timed, grid_c);
}

// ---- the launch loop (every scene that is not in slot order; ICP_CANON=0) ---------------------

// small cloud, one rank: steps 2-6 in one workgroup, the same arithmetic in the
// same order as the separate launches (launch latency dominates there)
int enqueue_tail_small(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    const int sl = r.enqueued % kRing;
    r.slot_ticket[sl] = ++ctx->flag_ticket;
    launch_iteration_tail_small(ctx->idx, ctx->m4, P.x, P.y, P.z, (int)r.n, Y.x, Y.y, Y.z, P.f, ctx->sums, r.N, ctx->c,
                                ctx->amb_count, ctx->iter_state, r.threshold, r.max_iter, ctx->err_trace_dev,
                                ctx->h_flags.dev() + 4 * sl, r.slot_ticket[sl], ctx->h_iter.dev(), ctx->h_trace.dev(), ctx->st);
    LAUNCHCHK("iteration_tail_small");
    r.ws = SeedState{}; // (it writes no seeds)
    ++r.enqueued;
    return ICP_OK;
}

// mid-size single-rank runs: steps 2-6 in one launch of the same workgroups (bit-identical; see
// icp_iter.hip)
int enqueue_tail_fused(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    const int sl = r.enqueued % kRing;
    r.slot_ticket[sl] = ++ctx->flag_ticket;
    TailArgs ta{};
    ta.idx = ctx->idx;
    ta.m4 = ctx->m4;
    ta.px = P.x;
    ta.py = P.y;
    ta.pz = P.z;
    ta.n = (int)r.n;
    ta.yx = Y.x;
    ta.yy = Y.y;
    ta.yz = Y.z;
    ta.p32 = P.f;
    ta.sa = r.sa;
    ta.part17 = ctx->tail_part;
    ta.part1 = ctx->tail_part + (size_t)18 * kTailMaxBlocks;
    ta.sync = ctx->tail_sync;
    ta.epoch_base = r.tail_epoch;
    ta.h_abort = ctx->h_flags.dev() + 11;
    ta.N = r.N;
    ta.c0 = ctx->c[0];
    ta.c1 = ctx->c[1];
    ta.c2 = ctx->c[2];
    ta.cnt = ctx->amb_count;
    ta.s = ctx->iter_state;
    ta.threshold = r.threshold;
    ta.max_iter = r.max_iter;
    ta.err_trace = ctx->err_trace_dev;
    ta.hflag = ctx->h_flags.dev() + 4 * sl;
    ta.ticket = r.slot_ticket[sl];
    ta.h_state = ctx->h_iter.dev();
    ta.h_trace = ctx->h_trace.dev();
    const bool split_err = run_knobs().tail_split_err; // (A/B)
    ta.sums_out = split_err ? ctx->sums : nullptr;
    ta.test_abort = r.tk.tail_test_abort; // (tests: fails the tail's first barrier -- the rerun path)
    launch_iteration_tail_grid(ta, r.tail_blocks, ctx->st);
    LAUNCHCHK("iteration_tail_grid");
    r.ws = SeedState{}; // (its transform: the f16 seeds and the seed distances, no records)
    r.ws.seed16 = r.sa.seed16 ? 1 : 0;
    r.ws.seedd = r.sa.seedd != nullptr;
    if (split_err) TRY(enqueue_err_step(r, r.enqueued));
    r.tail_epoch += 2;
    ++r.enqueued;
    return ICP_OK;
}

// steps 2-6 as their own launches: the moments (with ranks: their all-reduce and the lagged error
// step), the Horn step, the transform + residual, the error step
int enqueue_steps(LoopRun &r, int slot, bool timed)
{
    icp_ctx *ctx = r.ctx;
    const size_t n = r.n;
    const bool lag = r.lag;
    DevCloud &P = ctx->scene, &Y = ctx->Y;
    IterState *sd = ctx->iter_state;
    bool horn_fused = false; // (reduce_horn: the Horn step rode on the moments' fold)
    // 2-3. centroids, centred cross-covariance and norms (gpu.cc:98-104, :142): the first
    // iteration two-pass (the reference's order); later ones in one pass around the shifts
    // the previous Horn step left (its transformed centroid, its correspondence centroid)
    if (r.enqueued == 0) {
        TRY(moments_phase(ctx, n));
    } else {
        StepFold mf;
        if (r.fused_moments) { // (+ the fold, and on one rank the Horn step, in the last workgroup)
            mf.ticket = ctx->fold_ticket;
            mf.sums = ctx->sums;
            mf.step = !lag;
            mf.N = r.N;
            for (int a = 0; a < 3; ++a) mf.c[a] = ctx->c[a];
            mf.cnt = ctx->amb_count;
            mf.s = sd;
        }
        launch_shifted_moments(ctx->idx, ctx->m4, P.x, P.y, P.z, (int)n, Y.x, Y.y, Y.z, sd,
                               red_target(ctx, n, ctx->sums), ctx->st, ctx->kpos_valid ? ctx->kpos : nullptr,
                               ctx->m4kd, ctx->y_ready, mf);
        if (r.fused_moments) {
            horn_fused = !lag; // (multi-rank: the all-reduce, then the lagged error + Horn step below)
        } else if (!lag && red_blocks(n) > 1) { // the fold and the Horn step in one launch
            launch_reduce_horn(ctx->partials, red_blocks(n), ctx->sums, r.N, ctx->c, 1, ctx->amb_count, sd, ctx->st);
            horn_fused = true;
        } else if (r.err_pair) { // (+ the previous transform's residual, into sums[kSumErr])
            launch_reduce_pair(ctx->partials, ctx->err_part, red_blocks(n), ctx->sums, ctx->st);
        } else {
            red_finish(ctx, n, 17, ctx->sums);
        }
        LAUNCHCHK("shifted_moments");
        // With an all-reduce (ranks > 1, or a 1-rank communicator) each iteration has ONE: the
        // moments' 17 sums plus the previous iteration's residual e, whose err_step therefore runs
        // one iteration late (before this iteration's Horn solve, so a converged state is still
        // frozen at the same point).  Without one, err_step follows its own transform.
        if (lag) { // + the previous iteration's residual (sums[kSumErr], local until now)
            if (timed) HIPCHK(hipEventRecord(ctx->iter_ev[5 * slot + 3], ctx->st));
            TRY(allreduce(ctx, ctx->sums, kNumSums));
            if (timed) HIPCHK(hipEventRecord(ctx->iter_ev[5 * slot + 4], ctx->st));
            r.ar_timed[slot] = timed;
            // (enqueued > 0 here: the Horn step is the shifted one)
            TRY(enqueue_err_step(r, r.enqueued - 1, nullptr, true));
            horn_fused = true;
        }
    }
    // 4. Horn solve (gpu.cc:106-146) on the device
    if (!horn_fused) launch_horn_step(ctx->sums, r.N, ctx->c, r.enqueued > 0, ctx->amb_count, sd, ctx->st);
    // 5. apply + residual (gpu.cc:71-74): new_p <- sR new_p + t; e = sum ||Y - new_p||^2
    SeedArgs sa_t = r.grid_next ? r.sa_grid : r.sa;
    if (!r.grid_next) records_args(r, sa_t); // (a bundle search next: its slot records, when they can be)
    r.ws = seed_state_of(sa_t);
    StepFold ef;
    const bool err_fused = r.fused_steps && !sa_t.qop; // (the slot-record form keeps its own launch)
    if (err_fused && lag) { // (the fold only: the residual rides on the next all-reduce)
        ef.ticket = ctx->fold_ticket + 1;
        ef.sums = ctx->sums;
        ef.step = false;
    } else if (err_fused) { // (+ reduce_err_kernel's fold and error step, in the last workgroup)
        const int sl = r.enqueued % kRing;
        r.slot_ticket[sl] = ++ctx->flag_ticket;
        ef.ticket = ctx->fold_ticket + 1;
        ef.sums = ctx->sums;
        ef.N = r.N;
        ef.s = sd;
        ef.threshold = r.threshold;
        ef.max_iter = r.max_iter;
        ef.err_trace = ctx->err_trace_dev;
        ef.hflag = ctx->h_flags.dev() + 4 * sl;
        ef.hticket = r.slot_ticket[sl];
        ef.h_state = ctx->h_iter.dev();
        ef.h_trace = ctx->h_trace.dev();
    }
    launch_transform_err_dev(P.x, P.y, P.z, Y.x, Y.y, Y.z, (int)n, &sd->xf, &sd->done, r.need_p32 ? P.f : nullptr,
                             r.err_pair ? ctx->err_part : red_target(ctx, n, ctx->sums + kSumErr), sa_t, ctx->st, ef);
    if (!r.need_p32) ctx->p32_stale = true;
    const bool fold_err = !lag && red_blocks(n) > 1; // (folded by the error step's launch)
    if (!fold_err && !err_fused && !r.err_pair) red_finish(ctx, n, 1, ctx->sums + kSumErr);
    LAUNCHCHK("transform_err");
    // 6. err = (e + e) / np; stop after the iteration with err < threshold (gpu.cc:76-80)
    if (!lag && !err_fused) TRY(enqueue_err_step(r, r.enqueued, fold_err ? ctx->partials : nullptr));
    ++r.enqueued;
    if (lag && r.enqueued == r.max_iter) { // the last residual has no next iteration to ride on
        if (r.err_pair) launch_reduce(ctx->err_part, red_blocks(n), 1, ctx->sums + kSumErr, ctx->st);
        TRY(allreduce(ctx, ctx->sums + kSumErr, 1));
        TRY(enqueue_err_step(r, r.enqueued - 1));
    }
    return ICP_OK;
}

// One iteration of the launch loop: the search, then steps 2-6 in one of three forms.
int enqueue_launches(LoopRun &r)
{
    icp_ctx *ctx = r.ctx;
    const size_t n = r.n;
    const int slot = r.enqueued % kRing;
    // 1. correspondences: compute_Y_w_opti(m, new_p, Y)  (gpu.cc:69)
    const bool timed = is_timed(r, r.enqueued);
    // the path of this search: on the last count the host has seen (the previous transform
    // wrote for the path predicted when it was enqueued; a different decision here just
    // rebuilds what this path reads, nn_search_begin), else as predicted (carried over,
    // or the grid while the bundle images are still pending)
    const bool grid_cur = r.grid_policy && (r.far_obs >= 0 ? r.far_obs <= r.far_thr : r.grid_next);
    r.grid_next = r.grid_policy && (r.far_obs >= 0 ? r.far_obs <= r.far_thr : ctx->bundle_pending);
    // (the search of an iteration queued behind the converged one returns at once)
    // (the seed distances the last transform wrote -- of this run, or of the last one when
    // carried over -- for a grid search)
    const double *gseedd = r.ws.seedd && (grid_cur || ctx->nn_variant == ICP_NN_VARIANT_GRID) ? r.sa.seedd : nullptr;
    // (the second pass's grid: for four times the last queue seen, at least 256 queries)
    ctx->second_pass_items = r.grid_policy && r.q2_obs >= 0 ? std::max(256, 4 * r.q2_obs) : 0;
    TRY(nn_search_begin(ctx, ctx->scene, n, ctx->seeds_valid, timed ? ctx->iter_ev[5 * slot] : nullptr,
                        timed ? ctx->iter_ev[5 * slot + 1] : nullptr, false, &r.ws, &ctx->iter_state->done,
                        ctx->scene_slot, grid_cur, gseedd)); // (run_init zeroed the counters)
    TRY(after_search(r, r.enqueued, false, slot));
    if (!r.lag && r.enqueued > 0 && n > 0 && n <= (size_t)kRedSingle) return enqueue_tail_small(r);
    if (r.enqueued > 0 && r.fused_tail) return enqueue_tail_fused(r);
    return enqueue_steps(r, slot, timed);
}

constexpr int kTailAborted = -1000; // run_loop: a fused tail's grid barrier timed out (state restored)

// The loop of GPU::ICP::find_corresponding_opti (gpu.cc:52-83), device-resident: every
// iteration is enqueued without waiting on the previous one -- NN search, moments and their
// all-reduces, the Horn solve (horn_step, the host's own code), transform + residual and its
// all-reduce, the error test (err_step).  The host runs one iteration ahead: it enqueues
// iteration i+1, then waits for iteration i's completion event and its (done, iter) flag.
// After the iteration whose err < threshold the device flag freezes the state (the one
// iteration already enqueued behind it changes nothing), which is exactly where the
// reference's loop breaks (gpu.cc:79-80).
int run_loop(icp_ctx *ctx, int max_iter, double threshold, double *err_trace, icp_result *res, bool no_tail)
{
    LoopRun r;
    bool handed = false;
    const int rc = run_setup(r, ctx, max_iter, threshold, err_trace, res, no_tail, &handed);
    if (rc != ICP_OK || handed) return rc;
    const size_t n = r.n;
    while (!r.stop && r.waited < max_iter) {
        if (r.tk.enqueue_delay_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(r.tk.enqueue_delay_us));
        if (r.enqueued < max_iter && r.enqueued - r.waited <= kAhead + (r.lag || r.canon ? 1 : 0) &&
            !(!r.canon && r.hold_first && r.enqueued == 1 && r.waited == 0) &&
            !(r.canon && r.grid_policy && r.enqueued >= 3 && r.waited < r.enqueued - 2)) { // (fold_far[enqueued - 3] known)
            TRY(r.canon ? enqueue_canon(r) : enqueue_launches(r));
            continue;
        }
        const int wr = wait_one(r);
        if (wr != ICP_OK) {
            if (r.fused_tail && __atomic_load_n(ctx->h_flags + 11, __ATOMIC_ACQUIRE) != 0) break; // (rerun below)
            return wr;
        }
    }
    HIPCHK(hipStreamSynchronize(ctx->st)); // (the iterations queued behind the last one drain)
    if (r.fused_tail && __atomic_load_n(ctx->h_flags + 11, __ATOMIC_ACQUIRE) != 0) {
        TRY(tail_snapshot(ctx, n, r.seeds_at_start, true));
        HIPCHK(hipStreamSynchronize(ctx->st));
        ctx->seeds_valid = r.seeds_at_start;
        ctx->seedd_valid = false;
        return kTailAborted;
    }
    if (r.iter_dbg) {
        unsigned long long h[16];
        HIPCHK(hipMemcpy(h, r.iter_dbg, sizeof(h), hipMemcpyDeviceToHost));
        fprintf(stderr, "[iter_debug] tasks %llu staged %llu pts %llu big %llu flushes %llu rows_over %llu pts_over %llu "
                        "| wave-us A %.1f BC %.1f D %.1f E %.1f FG %.1f\n",
                h[0], h[1], h[2], h[3], h[4], h[10], h[11], h[5] * 0.01, h[6] * 0.01, h[7] * 0.01, h[8] * 0.01,
                h[9] * 0.01);
        // (four-wave workgroups only: one-strand workgroups count into their records, read a launch
        // at a time by ICP_ITER_DEBUG=2)
        fprintf(stderr, "[iter2_debug] (nn_grid_iter2_kernel, an ICP_ITER2_DBG build) tasks %llu walkers %llu batches %llu "
                        "pair tests %llu (lane 0's)\n",
                h[0], h[1], h[2], h[3]);
    }
    // (every transform of a policy run wrote the seed distances, whatever its form; the next run
    // may start from them)
    // (cert_counts: read with the stats, or folded into them when a run of another size starts)
    ctx->seedd_valid = r.grid_policy && r.ws.seedd;
    ctx->last_far = r.far_obs;
    ctx->last_q2 = r.q2_obs;
    ctx->second_pass_items = 0;
    return finish_run(ctx, threshold, err_trace, res, r.wall0);
}

} // namespace

extern "C" int icp_run(icp_ctx *ctx, int max_iter, double threshold, double *err_trace, icp_result *res)
{
    // (icp_set_progress: reset once per icp_run -- a rerun below replays the same iterations bit for
    // bit, and report_progress skips the ones the aborted attempt already reported)
    if (ctx) ctx->progress_next = 0;
    if (ctx) ctx->scene_pristine = false; // (icp_estimate_scene_normals: the scene as icp_set_scene* received it only)
    const int r = run_loop(ctx, max_iter, threshold, err_trace, res, false);
    if (r != kTailAborted) return r;
    // A grid barrier of the fused mid-size tail timed out (its workgroups were not all resident:
    // another process's persistent kernel on the same GPU).  The scene and correspondences the
    // run started from were restored; the same registration again with the separate launches
    // (bit-identical, icp_iter.hip) -- the stats count both attempts.
    return run_loop(ctx, max_iter, threshold, err_trace, res, true);
}
