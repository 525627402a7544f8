// icp_engine.h — private to the engine's translation units: icp_engine.hip (the context, the
// model and scene set-up, the searches, the per-operation surface), icp_run.hip (icp_run's
// loops), icp_cloud.hip (the normals, the k-NN lists and the temporary grid of a cloud),
// icp_global.hip (global registration's four calls), icp_filter.hip (the outlier filters) and
// icp_eval.hip (a registration's evaluation).  The
// context, the few types they share, the error macros, the run path's knob table and the
// declarations of the helpers one file calls in another.  The helpers are icp::engine
// and hidden: the shared library exports the C ABI (include/icp_capi.h) and nothing of this.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "icp_canon.h"
#include "icp_kernels.h"

namespace icp {
namespace engine {

// Every block of device or pinned host memory the engine keeps is one of these two owning types: the
// pointer, its capacity and its release travel together, and a struct that holds them frees them with
// itself.  Movable and swappable, not copyable -- so passing the object itself to a kernel does not
// compile; it converts to its pointer wherever one is expected.  live_blocks: the blocks both types hold
// now, process-wide (icp_debug_live_buffers).
extern std::atomic<long long> live_blocks;

// Device memory.  grow never shrinks and does not preserve the contents: a block too small is freed
// first; a count of 0 allocates one element.  When it fails the buffer is empty and the context's error
// is set (ctx may be null, as for fail).
template <class T> class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { (void)release(); }
    operator T *() const { return p; }
    T *get() const { return p; } // (where the pointer is cast on to another type)
    T *operator->() const { return p; }
    size_t capacity() const { return cap; } // in elements
    int grow(icp_ctx *ctx, size_t count);
    hipError_t release();

private:
    T *p = nullptr;
    size_t cap = 0;
};

// Pinned host memory: mapped and coherent with its device address (dev()), or plain pinned.  grow as
// DevBuf's: pointer, device address and capacity change together or not at all.
template <class T, bool Mapped> class HostBuf {
public:
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { (void)release(); }
    operator T *() const { return h; }
    T *get() const { return h; }
    T *operator->() const { return h; }
    T *dev() const
    {
        static_assert(Mapped, "plain pinned memory has no device address");
        return d;
    }
    size_t capacity() const { return cap; }
    int grow(icp_ctx *ctx, size_t count);
    hipError_t release();

private:
    T *h = nullptr, *d = nullptr;
    size_t cap = 0;
};
template <class T> using MappedBuf = HostBuf<T, true>;
template <class T> using PinnedBuf = HostBuf<T, false>;

struct DevCloud {
    DevBuf<double> x, y, z;
    DevBuf<float4> f;
    size_t n = 0;
    size_t cap() const { return x.capacity(); } // (grow_cloud keeps the four at one capacity)
};

// device memory the context keeps for the Scratch objects over it: want = the last call's total
struct KeptBlock {
    DevBuf<char> base;
    size_t want = 0;
};

} // namespace engine
} // namespace icp

// (a private header: the files that include it work in these namespaces)
using namespace icp;
using namespace icp::engine;

struct icp_ctx {
    int device = 0;
    int nn_mode = ICP_NN_CERTIFIED;
    int rank = 0, world = 1;
    bool allow_unequal = false;
    hipStream_t st = nullptr;
    ncclComm_t comm = nullptr;
    icp_allreduce_fn host_reduce = nullptr; // alternative to RCCL (icp_ctx_create_sharded)
    void *host_reduce_user = nullptr;
    icp_progress_fn progress_fn = nullptr; // (icp_set_progress: each recorded iteration's error, as it ends)
    void *progress_user = nullptr;
    int progress_next = 0; // (the next iteration of the current run to report)

    // model (replicated)
    DevCloud model;
    DevBuf<float4> m32;      // centred fp32 model, padded to nm_pad with far points
    DevBuf<float4> mperm;    // same, (mm, x, y, z) permuted for the MFMA operands
    DevBuf<float> mm;        // |m~|^2 rounded to fp32 (the MFMA's k = 0 operand)
    DevBuf<char> mimg16;     // f16 split image for the 32x32x16 f16 MFMA (1 KiB / 32 points)
    bool mimg16_pending = false; // (built at the first search that reads it: ensure_mimage16)
    bool m32_pending = false;    // (m32, mperm, mm: built at their first reader, ensure_m32)
    DevBuf<float> mms16;     // |b_s|^2 (scaled) per model point, fp32
    double scale16 = 1.0;    // power of two: max |b_s| in [2^11, 2^12)
    size_t nm = 0, nm_pad = 0;
    int nn_variant = ICP_NN_VARIANT_AUTO;
    double c[3] = {0, 0, 0}; // centring point = model centroid
    // host copy of the model (AoS): kept when the one-launch paths can take it (small models),
    // downloaded on demand for the CPU rule's host fix-up, else empty (0.2 GB at 2^23 points)
    std::vector<double> model_host;
    double rm = 0.0;         // max |centred fp32 model coordinate|
    // the model's preparation on the device (icp_model.hip): stats scratch, results (device and
    // pinned host), the kd builder's plan and scratch, the compare counter of icp_ensure_model
    DevBuf<double> mstat_part, mstat_out;
    PinnedBuf<double> h_mstat;
    DevBuf<int> cmp_diff;
    KdPlan kd_plan;
    DevBuf<char> kd_scratch;
    bool has_model = false;

    // scene (this rank's shard), its correspondences
    DevCloud scene, Y;
    size_t np_total = 0;
    bool has_scene = false;
    // icp_get_transform: (s, R row-major, t) mapping the scene as icp_set_scene* received it onto the
    // resident one -- every finished run's total (IterState::tot, finish_run) and every
    // icp_transform_scene, composed on the host (compose_srt); tot_n == 0: the identity
    double tot[13] = {0};
    int tot_n = 0;

    // scratch clouds for the per-operation surface
    DevCloud qa, qb;

    // NN workspace
    DevBuf<int> idx;
    DevBuf<char> part, part2;
    DevBuf<int> amb1;              // queue of the MFMA certificate
    DevBuf<int> amb_count, amb_list;
    DevBuf<double> amb_T;          // (amb_list and amb_T: one capacity, ensure_queue)
    // exact grid resolver (icp_grid.hip): model grid + the queues around it
    GridParams grid{};
    DevBuf<int> g_start;
    DevBuf<char> g_sort;     // the build's sort scratch (launch_grid_build)
    DevBuf<double4> g_pts;
    DevBuf<float4> g_pts32;  // (the fp32 image of g_pts: the seeded grid search's prefilter)
    DevBuf<IterState> iter_state; // device-resident loop state (icp_iter.hip)
    MappedBuf<IterState> h_iter;  // mapped host mirror of the last recorded iteration's state
    MappedBuf<double> h_trace;    // mapped host error trace
    MappedBuf<int> h_sig;         // mapped completion word of the per-operation calls
    int sig_ticket = 0;
    MappedBuf<double> h_few;      // mapped host staging of the few-query path: q (3 x kFewQueries),
                                  //   y (3 x kFewQueries), idx (kFewQueries ints)
    MappedBuf<int> h_flags;       // mapped host (done, iter, ticket, -) per in-flight iteration
                                  // (err_step writes it directly, through its device address)
    int flag_ticket = 0;          // last ticket handed to an iteration
    DevBuf<double> err_trace_dev;
    std::vector<hipEvent_t> iter_ev; // per ring slot: (nn begin, nn end, -, all-reduce begin, all-reduce end)
    DevBuf<unsigned long long> digest; // icp_set_index_digest: 3 x digest_cap per-iteration digests
    DevBuf<unsigned> cert_audit;       // icp_set_cert_audit: (max err ratio, min margin) float bits, count
    size_t digest_cap = 0;             // (the iterations asked for; 0: off)
    DevBuf<double4> m4;         // model as (x, y, z, 0) doubles: one read per random gather
    // the next model's SoA copy and double4 rows, built while its checks are read back and
    // swapped with model / m4 when they pass (set_model_staged)
    DevCloud model_alt;
    DevBuf<double4> m4_alt;
    hipEvent_t mstat_ev = nullptr; // (the checks' read-back)
    DevBuf<unsigned> seed16;    // seeded f16 filter: per-query shift (icp_run iterations >= 2)
    bool last_search_timed = false; // the per-operation search recorded its events
    bool seeds_valid = false;   // idx holds the previous search over the resident scene
    // seedd_valid: b_seedd holds D64(p_j, m[idx_j]) of the resident scene (the last icp_run took
    // the search policy, whose every transform writes it), and last_far that run's last far count
    // (SeedArgs::far_acc): the next run's policy starts from them instead of two bundle searches
    bool seedd_valid = false;
    int last_far = -1;
    // second_pass_items (icp_run's policy searches): the grid of the seeded search's second pass
    // is sized for this many queued queries (0: min(n, 4096)) -- the far count the host last saw
    int second_pass_items = 0;
    int last_q2 = -1; // the last run's last observed second-pass queue (IterState::queued2)
    DevBuf<int> amb1_hint, amb_hint;                  // candidates of the level-1 / level-2 queues
    DevBuf<int> fb_list;                              // queries the grid hands back
    DevBuf<double> fb_T;

    // reductions
    DevBuf<double> partials;
    DevBuf<double> err_part;     // (multi-rank icp_run: the transform's residual partials, icp_run.hip)
    DevBuf<double> canon_rowbuf; // (icp_run over a scene in slot order: the canonical rows, icp_canon.h)
    DevBuf<int> canon_ticket;    // (the fold's workgroup ticket, CanonStep::fold_ticket)
    PinnedBuf<int> h_far; // (a far count read back once, canon_path's hold_first)
    DevBuf<double> sums;
    PinnedBuf<double> h_sums;
    PinnedBuf<int> h_amb;
    DevBuf<double> stage;
    // small host <-> device transfers: a mapped pinned buffer the conversion kernels read and
    // write directly (no pageable-copy staging); bump-allocated, recycled after a sync
    MappedBuf<double> h_io;
    size_t io_off = 0;
    bool io_pending = false; // a queued kernel may still read h_io

    // ICP_NN_RULE_CPU_SQRT: the near-tie window of every search (launch_nn_cpu_rule_window)
    int nn_rule = ICP_NN_RULE_SQUARED;
    DevBuf<CpuRuleEntry> cr_entries;
    DevBuf<int> cr_count;
    DevBuf<int> cr_fix; // the fix-up's (query, index) pairs

    // one-launch registration of small clouds (icp_iter.hip, launch_icp_persistent)
    int run_mode = ICP_RUN_AUTO;
    int n_cu = 0;                    // compute units
    size_t lds_per_cu = 0, lds_per_block = 0;
    DevBuf<double> pers_part;        // 2 x kBlock x kNumSums published partials
    DevBuf<unsigned> pers_sync;      // arrival counter, abort word (+ padding to 16 B)
    DevBuf<double> tail_part;        // fused mid-size tail: published partials (18 x kTailMaxBlocks)
    DevBuf<unsigned> tail_sync;      // its barrier words
    DevBuf<double> mid_q4;           // mid-size one-launch loop: published queries (4 per point)
    DevBuf<int> mid_res;             // and their correspondences
    DevBuf<int> mid_perm;            // its search order (each point's row)
    DevBuf<char> mid_cnt;            // the order's scratch (radix sort)
    double m_lo[3] = {0, 0, 0}, m_hi[3] = {0, 0, 0}; // the model's box
    double pm_seed_big = 0.0;        // PersistArgs::seed_big for this model
    bool pers_sync_valid = false;    // the barrier words hold pers_epoch_base barriers of grid pers_grid
    unsigned pers_epoch_base = 0;
    int pers_grid = 0;
    DevBuf<unsigned long long> pers_stamps; // ICP_PERSIST_STAMPS=1: phase stamps
    // the model in Morton order for the one-launch NN (models <= kPersistMaxModel points):
    // x[nm] | y[nm] | z[nm] | 64-point block boxes (lo xyz, hi xyz) | original index (int32)
    DevBuf<double> pm_img;
    size_t pm_blocks = 0;
    // bundle-bound filter (icp_bundle.hip): the model's kd-ordered bundle and pair images, built
    // per model of >= kBundleMinModel points; the query order of the scene it searches
    DevBuf<char> b_img, b_pimg;               // 1 KiB per 32 bundles; 1 KiB per bundle
    DevBuf<int> b_kd_orig;                    // original index per kd position (nm: padding)
    DevBuf<double4> b_bctr, b_blk;            // per bundle / per 32-bundle block: centre, radius
    DevBuf<int> b_kd;                         // the kd order (upload staging)
    int nb_pad = 0;                           // bundles (whole LDS tiles)
    // the bundle filter's kd order and images are built at their first use (ensure_bundle):
    // pending from icp_set_model on until then (a run whose searches all take the grid never
    // builds them)
    bool bundle_pending = false;
    DevBuf<int> q_order;                      // the bundle filter's query order (launch_query_order)
    DevBuf<int> q_pos;                        // its inverse (query j's slot)
    DevBuf<char> q_order_tmp;
    const double *q_order_src = nullptr;      // the cloud q_order was computed for (its x array)
    size_t q_order_n = 0;
    DevBuf<unsigned long long> b_counters;    // icp_set_bundle_counters: the filter's executed work
    DevBuf<char> b_qop, b_gop;                // v2: per-slot query operands, per-group bounds
    DevBuf<double4> b_qraw;                   // v2: per-slot query coordinates, index, seed
    DevBuf<int> b_glist;                      // v2: fired-block list overflow
    DevBuf<double> b_seedd;                   // v2: per point, D64 to its seed (icp_run's transform)
    // the fused grid iteration's exclusion certificate (CertArgs): per point in slot order the
    // bound and the pair; counts = (certified, walked) summed over the run (device)
    hipEvent_t order_ev = nullptr; // icp_set_*_device_stream: the producer stream's point to wait for
    DevBuf<int4> cert_state;
    DevBuf<unsigned long long> cert_counts;    // (2 per strand: certified, walked -- CertArgs::counts;
                                               //  then, in the same allocation, a strand's last walker count and the
                                               //  dispatch order built from it, an int each: CertArgs::walk_last, IterOrder)
    int cert_counts_rows = 0; // (strands the runs since the last fold counted into cert_counts, not yet in stats)
    DevBuf<char> tail_backup;                 // icp_run with the fused tail: the starting scene / idx
    DevBuf<double4> b_gctr;                   // v2: per-group (centre, D)
    DevBuf<int> b_cand, b_cand_n;             // v2: per filter workgroup, its candidate blocks
    DevBuf<int> b_wsplit, b_tctl;             // v2: per filter workgroup its tasks; (count, counter)
    DevBuf<int2> b_tasks;                     // v2: the task list
    size_t b_counters_rows = 0;
    // The resident scene in slot order (scene_in_slot_order): point s of the scene (and idx[s]
    // while seeds_valid) is the caller's point s_order[s].  icp_get_scene / icp_get_indices and
    // the index digests map back; every other per-point pass is order-agnostic.
    // the local pair test (icp_bundle_rec.h): the pair image in block frames, the frames (c_B,
    // R_B) and max R_B (-1: not built)
    DevBuf<char> b_pimg_l;
    DevBuf<float4> b_frame;
    double b_rlmax = -1.0;
    // the model in kd order and the kd order's inverse (launch_build_kd_tables), and per query
    // its correspondence's kd position (kpos_valid: the last search over the resident scene kept it)
    DevBuf<double4> m4kd;
    DevBuf<int> kd_of, kpos;
    bool kpos_valid = false;
    // y_ready: the last search over the resident scene also wrote Y = m[idx] (the shifted moments
    // then stream it instead of gathering)
    bool y_ready = false;
    // arrival counters of the passes that end in their own last workgroup (StepFold): [0] the
    // moments + Horn step, [1] the transform + error step; zero between launches
    DevBuf<unsigned> fold_ticket;
    bool scene_slot = false;
    unsigned runs = 0; // (icp_run calls: the timing sample's phase)
    // scene_revert: the scene is in the slot order of a model since replaced -- icp_run puts it
    // back into file order (and sorts it by the new model's box) unless a new scene comes first
    bool scene_revert = false;
    bool p32_stale = false; // the scene's fp32 copy was not kept by the last icp_run (its path never read it)
    DevBuf<int> s_order;
    DevCloud s_tmp;                           // the permutation's second buffer
    DevBuf<int> s_tmp_idx;

    // The kept-pairs loop (run_kept: the max-correspondence-distance gate, icp_set_max_distance and
    // icp_gated.hip, and the point-to-plane metric, icp_set_metric and icp_plane.hip).  Scoped to one
    // run, whichever metric: the mask words (the scene's order), the moments' partial rows (kRobustPlaneSums
    // a workgroup, the widest), the device state with its mapped host mirror, the mapped K trace.
    DevBuf<unsigned long long> kept_mask;
    DevBuf<double> kept_part;
    DevBuf<GateState> kept_state;
    MappedBuf<GateState> h_kept;
    MappedBuf<long long> h_ktrace;
    // The gate: dmax (0: off), and what icp_get_inliers / icp_get_inlier_trace report, saved at the
    // end of the last gated run (a later ungated plane run leaves it): the flags in the caller's
    // order, K of the last gate evaluated, the recorded iterations' K.
    double gate_dmax = 0.0;
    DevBuf<unsigned char> gate_flags;
    bool gate_have = false; // a gated run has evaluated a gate since icp_set_scene
    long long gate_K = 0;
    std::vector<long long> gate_ktrace;
    // The trim (icp_set_trim): the fraction (1: off); per run the scene's d2 keys, the selection's
    // bins (integers; as doubles on their way through the all-reduce), its state and the
    // iteration's cut C (icp_select.hip), the mapped C trace beside the K trace; and what
    // icp_get_trim_trace reports, saved at the end of the last trimmed run (dropped with the scene).
    double trim_fraction = 1.0;
    DevBuf<unsigned long long> trim_keys;
    DevBuf<unsigned> trim_bins;
    DevBuf<double> trim_bins_d, trim_cut;
    DevBuf<SelectState> trim_state;
    MappedBuf<double> h_ctrace;
    bool trim_have = false;
    std::vector<double> trim_ctrace;
    // One-to-one rejection (icp_set_one_to_one): the switch, and per run the table of each model
    // point's smallest d2 key (icp_unique.hip; nm words, all ones at every iteration's start).
    bool one_to_one = false;
    DevBuf<unsigned long long> uniq_best;
    // Robust weights (icp_set_robust): the kind (ICP_ROBUST_*; 0: off), k and k2 = k * k (fp64, once),
    // the mapped W / K+ traces beside the K trace (grown with it), and what icp_get_robust_trace
    // reports, saved at the end of the last robust run (dropped with the scene).
    int robust_kind = 0;
    double robust_k = 0.0, robust_k2 = 0.0;
    MappedBuf<double> h_wtrace;
    MappedBuf<long long> h_ptrace;
    bool robust_have = false;
    std::vector<double> robust_wtrace;
    std::vector<long long> robust_ptrace;

    // the point-to-plane metric: the model's normals as (nx, ny, nz, 0) by model index (dropped with
    // the model)
    int metric = 0; // ICP_METRIC_*
    DevBuf<double4> n4;
    bool has_normals = false;
    // The symmetric form (icp_set_plane_symmetric): the scene's normals u0 as given, in the caller's
    // order (sn; dropped with the scene, kept across icp_transform_scene), and for a scene in slot
    // order their copy in that order (sn_slot, made at the first symmetric run that needs it;
    // sn_slot_valid falls with every change of the scene's order).  scene_pristine: no icp_run or
    // icp_transform_scene since icp_set_scene* (icp_estimate_scene_normals' condition).
    bool plane_symmetric = false;
    double plane_to_plane = 0.0; // icp_set_plane_to_plane's epsilon (0: off); reads the same sn / sn_slot
    DevCloud sn, sn_slot;
    bool has_scene_normals = false, sn_slot_valid = false;
    bool scene_pristine = false;
    // icp_model_knn's nm x k lists and the estimator's counters (icp_normals.hip): scratch of those two
    // calls alone, so that they leave everything a run reads as they found it
    DevBuf<int> knn_idx;
    DevBuf<double> knn_d2;
    DevBuf<unsigned long long> knn_counters;

    // icp_voxel_downsample* (icp_voxel.hip): scratch of those calls alone -- the keys, orders, run
    // heads and box rows (vox_buf), the host form's staged input and output clouds (vox_io: 6 n
    // doubles) and counts (vox_cnt)
    DevBuf<char> vox_buf;
    DevBuf<double> vox_io;
    DevBuf<int> vox_cnt;
    // icp_filter_* (icp_filter.hip): every device array of a call -- the temporary grid's, the filter's
    // own, the staged clouds -- is a part of this one block (Scratch's kept mode), kept between calls: a
    // call's dozen allocations cost as much as its kernels
    KeptBlock filt_block;
    // icp_evaluate* (icp_eval.hip): likewise, a block of its own -- the per-point pairs, the sums' terms,
    // the queries' rows and, with `both`, the scene's temporary grid
    KeptBlock eval_block;

    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    icp_stats stats{};
    std::string err;
};

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, ICP_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

#define LAUNCHCHK(what)                                                                       \
    do {                                                                                      \
        hipError_t e_ = hipGetLastError();                                                    \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, ICP_E_HIP, std::string(what) + ": " + hipGetErrorString(e_));    \
    } while (0)

#define TRY(expr)                                                                             \
    do {                                                                                      \
        int rc_ = (expr);                                                                     \
        if (rc_ != ICP_OK) return rc_;                                                        \
    } while (0)

#pragma GCC visibility push(hidden)
namespace icp {
namespace engine {

// What icp_run's last enqueued transform wrote for the next search (transform_err_kernel, SeedArgs).
// The next search may use each output only in the form it was written in: the bundle filter's
// slot records exist in a global and a local pair-test form (local_r, icp_bundle_rec.h), and
// seed16 holds either the f16 seed (mfma16_seed_value) or the local form's shift s0.
struct SeedState {
    bool seedd = false;      // b_seedd: each point's seed distance D64(p', y)
    int seed16 = 0;          // seed16: 0 not written, 1 the f16 seeds, 2 the local shifts s0
    bool records = false;    // b_qop / b_gop / b_gctr: the slot records and group bounds
    double rec_local = -1.0; // the records' local_r (-1: the global form)
};

// The run path's environment switches, each read ONCE per process (run_knobs, icp_run.hip: at the
// first call that asks for any of them).  Parse: "!=0" on unless atoi(value) == 0; "=1" on only if
// atoi(value) == 1; "[0]" by the value's first character; "set" on if the variable exists.
//
//   field              variable                default  parse / clamp          what it switches
//   grid_budget        ICP_GRID_BUDGET         0        max(1, atoi); 0: the   cells a query box may span (grid_budget)
//                                                       rule of grid_budget
//   grid_auto          ICP_GRID_AUTO           on       !=0                    icp_run's search policy for AUTO at the bundle
//                                                                              filter's sizes; 0: every seeded search on the
//                                                                              bundle cascade (A/B)
//   grid_iter          ICP_GRID_ITER           on       !=0                    the grid iterations over a scene in slot order as
//                                                                              ONE launch each (nn_grid_iter_kernel: the
//                                                                              transform, the seeded search with the task's boxes
//                                                                              staged in LDS, the moments); 0: the separate
//                                                                              passes (A/B; measured at C4 0.167 against 0.162 ms
//                                                                              an iteration, the W = 8 shard 0.058 against 0.055,
//                                                                              profiles/r05g)
//   grid_xcd           ICP_GRID_XCD            1        atoi                   the seeded grid search of a sparse scene in slot
//                                                                              order, each XCD on a contiguous eighth of it
//                                                                              (launch_nn_grid_resolve_all); 0: the plain block
//                                                                              order, 2: every scene (A/B)
//   bundle_order_off   ICP_BUNDLE_ORDER        off      set and atoi == 0      the bundle filter's queries in file order (A/B)
//   scene_order_off    ICP_SCENE_ORDER         off      set and atoi == 0      the resident scene stays in file order (A/B)
//   cell_seed          ICP_CELL_SEED           on       !=0                    an unseeded search of a scene in slot order takes
//                                                                              the seeded grid pass from cell seeds
//                                                                              (grid_unseeded_slot); 0: the ring search (A/B)
//   first_k1           ICP_FIRST_K1            off      =1                     the canonical first iteration's search and moments
//                                                                              as one fused launch (A/B; measured slower,
//                                                                              enqueue_canon_first_k1)
//   run_mode           ICP_RUN_MODE            -1       "launches" |           forces the run mode over icp_set_run_mode (A/B);
//                                                       "persistent", else -1  the fused tail obeys "launches" only
//   persist_mid_off    ICP_PERSIST_MID         off      value == "0"           mid-size runs keep the launch loop (A/B)
//   persist_stamps     ICP_PERSIST_STAMPS      off      set                    the one-launch loop's phase stamps, to stderr
//   persist_cull       ICP_PERSIST_NN          1        "all": 0               0: every model point for every query (A/B)
//   mid_prepass        ICP_MID_PREPASS         off      [0] == '1'             the mid-size loop's first search seeded by one pass
//                                                                              of the exact cascade (A/B)
//   transform_records  ICP_TRANSFORM_RECORDS   on       !=0                    0: the prep kernel writes the slot records (A/B)
//   far_shift          ICP_GRID_FAR_SHIFT      5        atoi in [0, 20]        the far threshold n >> shift (A/B)
//   far_dist           ICP_GRID_FAR            off      value == "dist"        the far count by the round-4 distance rule (A/B)
//   fused_steps        ICP_FUSED_STEPS         0        atoi & 3               bit 0: the moments, bit 1: the transform fold their
//                                                                              partials in their own last workgroup (run_setup_steps)
//   err_pair           ICP_ERR_PAIR            on       [0] != '0'             0: the separate residual fold (A/B)
//   timing_stride      ICP_NN_TIMING_STRIDE    0        max(1, atoi); 0: 8     every how many iterations the search is timed
//   canon              ICP_CANON               on       [0] != '0'             0: the round-4 schedule for a scene in slot order (A/B)
//   cert               ICP_CERT                on       [0] != '0'             the fused grid iteration's exclusion certificate;
//                                                                              0: every query walks (A/B)
//   cert_two           ICP_CERT_TWO            1        [0] == '0': 0          0: the certificate's one-point form
//   cert_skin          ICP_CERT_SKIN           0.25     atof in [0, 4]         the walk's extra radius in grid cells
//   cert_skin1         ICP_CERT_SKIN1          = skin   atof in [0, 4]         the skin of a launch with no state to read (A/B)
//   iter2_order        ICP_ITER2_ORDER         2        atoi in 1 .. 7 but 4,  the fused iteration's dispatch order (IterOrder,
//                                                       else 0                 icp_kernels.h): 0 xcd_row; 1 / 2 / 3 the heavy
//                                                                              strands first (2: runs, then strands -- C4 10,676
//                                                                              against 10,379 it/s; 1 level, 3 -9.8%,
//                                                                              profiles/r10/ab_forms.txt); 5 / 6 / 7 light-first (tests)
//   iter_debug         ICP_ITER_DEBUG          0        set: 1; atoi == 2: 2   nn_grid_iter_kernel's phase clocks and counts, summed
//                                                                              over the run, to stderr; 2: each launch's (synchronises)
//   tail_split_err     ICP_TAIL_SPLIT_ERR      off      set                    the fused tail's error step as its own launch (A/B)
//   debug_policy       ICP_DEBUG_POLICY        off      set                    the policy's far counts, to stderr
struct RunKnobs {
    int grid_budget;
    bool grid_auto, grid_iter;
    int grid_xcd;
    bool bundle_order_off, scene_order_off, cell_seed, first_k1;
    int run_mode;
    bool persist_mid_off, persist_stamps;
    int persist_cull;
    bool mid_prepass, transform_records;
    int far_shift;
    bool far_dist;
    int fused_steps;
    bool err_pair;
    int timing_stride;
    bool canon, cert;
    int cert_two;
    double cert_skin, cert_skin1;
    int iter2_order;
    int iter_debug;
    bool tail_split_err, debug_policy;
};
const RunKnobs &run_knobs();

// The switches the tests set between two runs of one process: read again at every run (run_test_knobs).
//   enqueue_delay_us    ICP_TEST_ENQUEUE_DELAY_US  0    max(0, atoi)   the host sleeps this long before each enqueue attempt
//                                                                      (the path sequence must not depend on the host's lead)
//   tail_test_abort     ICP_TAIL_TEST_ABORT        off  [0] == '1'     fails the fused tail's first barrier (the rerun path)
//   persist_test_abort  ICP_PERSIST_TEST_ABORT     off  [0] == '1'     makes the one-launch loop's first barrier fail as if a
//                                                                      workgroup never came
struct RunTestKnobs {
    int enqueue_delay_us;
    bool tail_test_abort, persist_test_abort;
};
RunTestKnobs run_test_knobs();

// ---- icp_engine.hip --------------------------------------------------------------------
constexpr int kSeededBox = 125; // cells of the box a seeded grid search walks with a few lanes (grid_seeded_search)

int fail(icp_ctx *ctx, int code, const std::string &msg);

template <class T> hipError_t DevBuf<T>::release()
{
    if (!p) return hipSuccess;
    live_blocks.fetch_sub(1, std::memory_order_relaxed);
    T *old = p;
    p = nullptr;
    cap = 0;
    return hipFree(old);
}

template <class T> int DevBuf<T>::grow(icp_ctx *ctx, size_t count)
{
    if (cap >= count && p) return ICP_OK;
    HIPCHK(release());
    T *fresh = nullptr;
    HIPCHK(hipMalloc((void **)&fresh, sizeof(T) * (count ? count : 1)));
    live_blocks.fetch_add(1, std::memory_order_relaxed);
    p = fresh;
    cap = count;
    return ICP_OK;
}

template <class T, bool Mapped> hipError_t HostBuf<T, Mapped>::release()
{
    if (!h) return hipSuccess;
    live_blocks.fetch_sub(1, std::memory_order_relaxed);
    T *old = h;
    h = d = nullptr;
    cap = 0;
    return hipHostFree(old);
}

template <class T, bool Mapped> int HostBuf<T, Mapped>::grow(icp_ctx *ctx, size_t count)
{
    if (cap >= count && h) return ICP_OK;
    HIPCHK(release()); // (the caller has synchronised: no kernel still writes the old block)
    T *fresh = nullptr;
    HIPCHK(hipHostMalloc((void **)&fresh, sizeof(T) * (count ? count : 1),
                         Mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault));
    live_blocks.fetch_add(1, std::memory_order_relaxed);
    h = fresh;
    if (Mapped) {
        const hipError_t e = hipHostGetDevicePointer((void **)&d, h, 0);
        if (e != hipSuccess) {
            (void)release();
            return fail(ctx, ICP_E_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
        }
    }
    cap = count;
    return ICP_OK;
}

int check_ready(icp_ctx *ctx, bool need_scene);
int allreduce(icp_ctx *ctx, double *buf, size_t count);
int global_count(icp_ctx *ctx, int *v);
double *red_target(icp_ctx *ctx, size_t n, double *out);
void red_finish(icp_ctx *ctx, size_t n, int K, double *out);
int level1_kind(const icp_ctx *ctx, size_t n);
GridView grid_view(const icp_ctx *ctx);
int grid_budget(const icp_ctx *ctx);
bool want_slot_order(const icp_ctx *ctx, size_t n);
int scene_revert_now(icp_ctx *ctx);
int scene_to_slot_order(icp_ctx *ctx);
int scene_normals_current(icp_ctx *ctx, const DevCloud **out);
int fold_cert_counts(icp_ctx *ctx);
int nn_search_begin(icp_ctx *ctx, const DevCloud &q, size_t n, bool seeded, hipEvent_t ev0, hipEvent_t ev1,
                    bool zero_counts = true, const SeedState *ws = nullptr, const int *stop = nullptr,
                    bool slot_order = false, bool grid_seeded = false, const double *seedd = nullptr);
int cpu_rule_fixup(icp_ctx *ctx, const DevCloud &q, size_t n, const int *stop);
int moments_phase(icp_ctx *ctx, size_t n);
int grow_cloud(icp_ctx *ctx, DevCloud &c, size_t n, bool with_f32);
int download_cloud(icp_ctx *ctx, const DevCloud &c, size_t n, double *xyz);
int ensure_model_stats(icp_ctx *ctx);
GridView grid_view_of(const GridParams &p, const int *start, const double4 *pts, const float4 *pts32);
int grid_budget_for(size_t n);

// ---- icp_cloud.hip ---------------------------------------------------------------------
// The device arrays of one call on a cloud that is not the resident model; they go, or may be handed out
// again, with the object.  Owning (kept null): every get is a hipMalloc, freed with the object.  Kept,
// over a block of the context's: a get is a 256-byte-aligned part of the block while it fits and an
// allocation of the object's own when it does not; as it goes, the object leaves the call's total in the
// block and, when the call did not fit, grows the block to that total (should that fail, the next object
// over it does, once, before it hands anything out) -- so the second call at a size, and every call at the
// size of the one before it, allocates nothing.  A count of 0 yields a valid pointer.
class Scratch {
public:
    explicit Scratch(icp_ctx *ctx, KeptBlock *kept = nullptr) : ctx(ctx), kept(kept) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch();
    template <class T> int get(T **out, size_t count) { return get_bytes((void **)out, sizeof(T) * (count ? count : 1)); }

private:
    int get_bytes(void **out, size_t bytes);
    icp_ctx *ctx;
    KeptBlock *kept;
    size_t off = 0, total = 0;
    bool begun = false;
    std::vector<DevBuf<char>> own;
};

// A temporary grid over a cloud that is not the model: the cloud's double4 rows, the grid as the kernels
// take it, its cell budget.  The arrays are the Scratch's that it was built from.
struct TempGrid {
    double4 *rows = nullptr;
    GridView gv{};
    int budget = 0;
};

// tg = the grid of the n points in aos (device memory, 3 x n col-major), built as the scene estimator's,
// its arrays and the cloud's SoA streams taken from mem.  Asynchronous on the context's stream but for the
// box's read-back; the caller synchronises before mem goes.  ICP_E_RANGE for a non-finite coordinate.
int cloud_grid(icp_ctx *ctx, const std::string &who, const double *aos, size_t n, Scratch &mem, TempGrid &tg);
// icp_fpfh's grid half: cloud_grid in memory of its own, freed before the call returns; rows = the points'
// double4 rows; with k_normals > 0 nrm = their normals by the estimator's kernels; row j of idx / d2 =
// launch_model_knn's k lists: the caller's device arrays of n (rows, nrm) and n x k entries.  Synchronous.
int cloud_knn(icp_ctx *ctx, const std::string &who, const double *aos, size_t n, int k_normals, const double *viewpoint,
              int k, double4 *rows, double4 *nrm, int *idx, double *d2);

// the checks and the unpack loop these calls share; each caller words its own refusal
constexpr size_t kAllFinite = ~(size_t)0;
inline size_t first_nonfinite(const double *v, size_t count) // the first non-finite entry's index, or kAllFinite
{
    for (size_t k = 0; k < count; ++k)
        if (!std::isfinite(v[k])) return k;
    return kAllFinite;
}
// name = k within [kKnnMinK, kKnnMaxK] and at most the `word`'s n points (ICP_E_ARG)
int knn_k_check(icp_ctx *ctx, const std::string &who, const char *name, int k, const std::string &word, size_t n);
inline void rows4_to_xyz(const double *rows4, size_t n, double *xyz) // n (x, y, z, -) rows -> 3 x n col-major
{
    for (size_t j = 0; j < n; ++j)
        for (int a = 0; a < 3; ++a) xyz[3 * j + a] = rows4[4 * j + a];
}

// ---- icp_run.hip -----------------------------------------------------------------------
int wait_flag(icp_ctx *ctx, const int *flag, int ticket);

} // namespace engine
} // namespace icp
#pragma GCC visibility pop
