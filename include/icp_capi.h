/*
 * icp_capi.h — C-ABI of the MI355X-native ICP engine (libicp_hip.so).
 *
 * Drop-in boundary for the reference's src/GPU layer (yassram/iterative-closest-point).
 * The reference exposes C++ free functions over Eigen matrices (src/GPU/gpu.hh:110-116)
 * and the GPU::ICP class (src/GPU/gpu.hh:41-104).  This header replaces them with plain
 * pointers + sizes; INTEGRATION.md shows the shim a maintainer adds to src/GPU so that
 * host code written against gpu.hh relinks unchanged.
 *
 * Data layout at the boundary: a cloud of n points is 3 x n column-major doubles, i.e.
 * interleaved xyz (Eigen MatrixXd::data() of the reference's 3 x n matrices):
 * point j = (a[3j], a[3j+1], a[3j+2]).  Device layout is private to the engine.
 *
 * Errors: every entry point returns ICP_OK (0) or a negative ICP_E_* code; the library
 * never calls exit().  icp_last_error(ctx) gives a message.  Calls are synchronous
 * (results are on the host when the call returns) and not re-entrant per context.
 */
#ifndef ICP_CAPI_H
#define ICP_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
#define ICP_OK 0
#define ICP_E_ARG (-1)            /* bad argument / null pointer                    */
#define ICP_E_HIP (-2)            /* HIP runtime failure (message in icp_last_error) */
#define ICP_E_SIZE_MISMATCH (-3)  /* np != nm      (src/cpu.cc:44-47, src/GPU/gpu.cc:54-57) */
#define ICP_E_TOO_FEW_POINTS (-4) /* np < 4        (src/cpu.cc:49-52, src/GPU/gpu.cc:59-62) */
#define ICP_E_NO_MODEL (-5)       /* icp_set_model / icp_set_scene not called        */
#define ICP_E_RCCL (-6)           /* RCCL failure                                   */
#define ICP_E_NO_DEVICE (-7)      /* no HIP device / bad device ordinal             */
#define ICP_E_IO (-8)             /* file could not be opened (src/load.cc:11-14)   */
#define ICP_E_RANGE (-9)          /* coordinates outside the engine's domain        */
#define ICP_E_DEGENERATE (-10)    /* point-to-plane: an iteration's 6 x 6 system is singular;
                                     icp_ransac_pose: no hypothesis passed the edge check */

/* ---- nearest-neighbour arithmetic -------------------------------------- */
/* Both modes return the SAME indices: the first (lowest-index) minimum of the fp64
 * squared distance ((dx*dx + dy*dy) + dz*dz) — the reference's opti GPU rule
 * (src/GPU/compute.cu:112-117,137) == CPU minCoeff first-min (src/cpu.cc:22).       */
#define ICP_NN_CERTIFIED 0 /* fp32 filter + per-query certificate + fp64 resolution (fast) */
#define ICP_NN_FP64 1      /* fp64 brute force (reference-faithful cross-check)           */

/* Filter used by ICP_NN_CERTIFIED (results identical; speed differs):
 * VALU:   direct-form fp32 distances on the vector ALUs (8 VALU ops per pair);
 * MFMA:   expanded form |m|^2 - 2 p.m on v_mfma_f32_16x16x4_f32 (256 pairs / instruction);
 * MFMA16: the same form on v_mfma_f32_32x32x16_f16 with hi/lo f16 splits (1024 pairs /
 *         instruction, co-executes with the VALU);
 * All filters send uncertified queries to an exact fp64 search on a uniform model grid,
 * then (boxes over budget) to the VALU filter and fp64 brute force.
 * GRID:   no brute-force filter: exact fp64 search on the model grid for every query
 *         (same first-minimum rule, same results); O(N) instead of
 *         O(N*M) for clouds whose nearest neighbours are local.
 * BUNDLE: MFMA16 behind an exact MFMA bound per (query, 32-point kd bundle of the model):
 *         every query is tested against every bundle (N x M/32 bound evaluations, 32 x 32 per
 *         instruction) and only the bundles that may hold a point as close as the query's
 *         seed run the pair test (icp_bundle.hip).  Same results.
 * AUTO:   MFMA16 when both clouds have >= 8192 points, else VALU. */
#define ICP_NN_VARIANT_AUTO 0
#define ICP_NN_VARIANT_VALU 1
#define ICP_NN_VARIANT_MFMA 2
#define ICP_NN_VARIANT_MFMA16 3
#define ICP_NN_VARIANT_GRID 4
#define ICP_NN_VARIANT_BUNDLE 5

typedef struct icp_ctx icp_ctx;

typedef struct icp_result {
    int iterations; /* ICP iterations executed                                       */
    int converged;  /* 1 if err < threshold stopped the loop (src/GPU/gpu.cc:79-80)   */
    double err;     /* last err = (e_align + e_apply) / np, as printed (gpu.cc:76);
                       with icp_set_plane_symmetric the residual is along a sum of two
                       normals: up to four times the one-sided metric's; with
                       icp_set_plane_to_plane it is the mean squared Mahalanobis residual,
                       which carries the tangential distance with weight 1/2 and does
                       not fall to zero between two samplings of a surface           */
    double s;       /* last increment's scale       (GPU::ICP::s, gpu.hh:91); 1 with
                       ICP_METRIC_POINT_TO_PLANE                                      */
    double R[9];    /* last increment's rotation, row-major (GPU::ICP::r, gpu.hh:93)  */
    double t[3];    /* last increment's translation (GPU::ICP::t, gpu.hh:92)          */
} icp_result;

typedef struct icp_stats {
    double nn_ms;          /* summed device time of the timed NN searches' O(N*M)-class kernel (HIP
                              events).  icp_run times iterations 1, 9, 17, ... of each run (an event
                              pair costs the stream ~9 us; ICP_NN_TIMING_STRIDE changes the 8), the
                              per-operation surface every search of >= 2^32 pairs               */
    long long nn_launches; /* number of NN searches timed (samples, not every search)       */
    long long nn_pairs;    /* sum over searches of np_local * nm                        */
    long long ambiguous;   /* queries the fp32 certificate sent to fp64 resolution      */
    long long level1_queued; /* queries the MFMA certificate sent to the VALU filter     */
    long long level1_unrecovered; /* ... of which the MFMA filter proposed no candidate      */
    double iter_ms;        /* host wall time inside icp_run                             */
    long long iterations;  /* iterations executed by icp_run                            */
    long long grid_fallback; /* near ties the grid resolver handed back to brute force     */
    double allreduce_ms;   /* summed device time of icp_run's per-iteration all-reduce
                              (HIP events around the collective on the engine stream; timed
                              iterations only, like nn_ms)                                   */
    long long allreduce_calls; /* number of all-reduces timed                              */
    /* f16 certificate audit (icp_set_cert_audit; -1 / 0 when off), over every query the f16
     * filter certified since the last reset: the largest |filter value - fp64 value| of the
     * winner over its error bound delta_b (< 1 means the bound held with room), the smallest
     * (second - T) / (T - best) margin, and the number of certified queries audited.          */
    double cert_max_err_ratio;
    double cert_min_margin;
    long long cert_audited;
    long long persistent_runs; /* icp_run calls that ran as ONE launch (icp_set_run_mode)      */
    long long cpu_rule_ties;   /* ICP_NN_RULE_CPU_SQRT: near ties evaluated on the host       */
    long long cpu_rule_changed; /* ... whose CPU-rule answer differs from the squared rule's   */
    long long persistent_fallbacks; /* one-launch runs that found their grid not co-resident at
                                       the first barrier and ran the launch loop instead         */
    int last_filter; /* ICP_FILTER_* of the last NN search's O(N*M)-class level (-1: none since the
                        context was created or its stats reset)                                    */
    long long bundle_builds;     /* builds of the bundle filter's images (set_model leaves them
                                    pending; the first search that needs them builds them)         */
    long long bundle_builds_in_run; /* ... of which between two iterations of an icp_run          */
    long long run_bundle_searches;  /* icp_run searches that ran the bundle cascade                */
    long long run_grid_searches;    /* icp_run searches that ran the exact grid search             */
    long long run_certified; /* queries of icp_run's fused grid iterations that kept their
                                correspondence by the exclusion certificate, without a walk    */
    long long run_walked;    /* ... and those that walked their box (or were taken by a wave)  */
    unsigned long long run_path_bits; /* the last icp_run: bit k set when iteration k's search was the
                                         exact grid search (k < 64); the rest ran the bundle cascade or
                                         another filter.  The same on every rank of a job.           */
} icp_stats;
/* icp_stats.last_filter: the search level that decided most queries */
#define ICP_FILTER_VALU 0    /* fp32 direct-form filter on the vector ALUs */
#define ICP_FILTER_MFMA 1    /* f32 MFMA expanded-form filter               */
#define ICP_FILTER_MFMA16 2  /* f16 hi/lo MFMA filter over all N x M pairs  */
#define ICP_FILTER_BUNDLE 3  /* f16 MFMA bundle bound + pair filter (nn_bundle2_kernel) */
#define ICP_FILTER_GRID 4    /* exact fp64 grid search of every query       */
#define ICP_FILTER_FP64 5    /* fp64 brute force                            */
#define ICP_FILTER_ONE_LAUNCH 6 /* the one-launch registration's culled fp64 search */

/* ---- context ------------------------------------------------------------ */
/* Single-GPU context on HIP device `device` (replaces the stateless wrappers of
 * src/GPU/compute.cu, which re-allocate and re-upload everything per call). */
int icp_ctx_create(int device, int nn_mode, icp_ctx **out);

/* One rank of a world_size-rank job (one process per GPU).  The scene is sharded,
 * the model replicated; per iteration the partial centroid / cross-covariance / error
 * sums are all-reduced with RCCL.  `rccl_id` = 128 bytes from icp_rccl_unique_id() on
 * rank 0, broadcast to all ranks by the caller.  With world_size 1 and a non-null id the
 * context still creates a (1-rank) communicator and every sum goes through ncclAllReduce:
 * the RCCL data path of a multi-GPU job, runnable on a single GPU. */
int icp_ctx_create_dist(int device, int nn_mode, int rank, int world_size, const void *rccl_id,
                        icp_ctx **out);
int icp_rccl_unique_id(void *out128);
/* Same sharded engine, but the per-iteration sums are combined by a caller-supplied
 * host all-reduce instead of RCCL: `fn(buf, count, user)` must replace buf[0..count) by
 * its element-wise sum over all ranks (identically on every rank) and return 0.  Used to
 * run several ranks on ONE device (RCCL refuses duplicate GPUs) and by embedders that
 * own their communicator. */
typedef int (*icp_allreduce_fn)(double *buf, size_t count, void *user);
int icp_ctx_create_sharded(int device, int nn_mode, int rank, int world_size, icp_allreduce_fn fn,
                           void *user, icp_ctx **out);
void icp_ctx_destroy(icp_ctx *ctx);
const char *icp_last_error(const icp_ctx *ctx);
const char *icp_strerror(int code);
int icp_device_count(int *count);

/* ---- resident clouds (GPU::ICP constructor, src/GPU/gpu.hh:44-56) -------- */
/* Model ("ref", m) is uploaded once and replicated on every rank. */
int icp_set_model(icp_ctx *ctx, const double *m_xyz, size_t nm);
/* Scene ("transform", p): this rank's np_local points of an np_total-point cloud.
 * Resets new_p = p (gpu.hh:47).  Single-GPU: np_local == np_total. */
int icp_set_scene(icp_ctx *ctx, const double *p_xyz, size_t np_local, size_t np_total);
/* The same two calls for clouds already in device memory (AoS fp64, 3 x n col-major, on the
 * context's device, e.g. the output of an earlier GPU stage): no PCIe copy -- the model's images
 * and the scene's SoA copies are built from the caller's array on the context's stream.  The
 * array is read after all work enqueued before the call on ANY stream of the device (the call
 * synchronises the device first), and must stay valid and unmodified until the call returns. */
int icp_set_model_device(icp_ctx *ctx, const double *m_xyz_dev, size_t nm);
int icp_set_scene_device(icp_ctx *ctx, const double *p_xyz_dev, size_t np_local, size_t np_total);
/* ... reading the array after the work enqueued so far on `producer` only (a hipStream_t of the
 * context's device; NULL = the legacy default stream): the context's stream waits for an event
 * recorded there, with no device synchronisation.  Work on other streams is not waited for.
 * These two are stream-ordered: they may return before the array has been read (the model
 * setter still waits for its bounding box; the scene setter does not wait at all), so the array
 * must stay valid and unmodified until a synchronising call on the context returns (icp_run,
 * icp_get_*); errors of the enqueued work surface there. */
int icp_set_model_device_stream(icp_ctx *ctx, const double *m_xyz_dev, size_t nm, void *producer);
int icp_set_scene_device_stream(icp_ctx *ctx, const double *p_xyz_dev, size_t np_local, size_t np_total,
                                void *producer);
/* Copy this rank's current new_p (gpu.hh:88) back to the host. */
int icp_get_scene(icp_ctx *ctx, double *p_xyz_out);
/* icp_set_model, unless the resident model already holds exactly these nm points, bit for bit
 * (models of <= 64k points: memcmp against the engine's host copy; larger ones: the upload is
 * compared with the resident device copy, and becomes the new model if it differs): the safe
 * form of "upload the model once" for wrappers that receive the model on every call
 * (compute_Y_w_opti, compute.cu:154-160, re-uploads per call).  *uploaded (nullable) = 1 if
 * the model changed. */
int icp_ensure_model(icp_ctx *ctx, const double *m_xyz, size_t nm, int *uploaded);
/* Progress of icp_run (the reference prints "[ICP] iteration number i | error value = e" as each
 * iteration ends, src/GPU/gpu.cc:65,77): fn(i, err_i, user) is called on the calling thread, in
 * order, once per recorded iteration, while the run waits for the device (from the mapped error
 * trace: no extra synchronisation); a one-launch registration reports when its launch ends.
 * fn = NULL switches it off. */
typedef void (*icp_progress_fn)(int iteration, double err, void *user);
int icp_set_progress(icp_ctx *ctx, icp_progress_fn fn, void *user);
/* Reference behaviour is to refuse np != nm (gpu.cc:54-57); 1 lifts that check. */
int icp_set_allow_unequal(icp_ctx *ctx, int allow);
/* ICP_NN_VARIANT_* (default AUTO). */
int icp_set_nn_variant(icp_ctx *ctx, int variant);
/* How icp_run executes (results are bit-identical either way):
 * LAUNCHES:   the device-resident loop of a few launches per iteration (any size, any rank count);
 * PERSISTENT: the whole run in ONE launch of co-resident workgroups -- taken when the run is
 *             eligible: one rank without a communicator, the squared NN rule, no index digest,
 *             and either 4 <= np <= 4096 with nm <= ~6,400 points (the model in LDS, one grid
 *             barrier per iteration) or 4096 < np <= 49,152 with nm <= 65,536 (the model in
 *             global memory, its block boxes in LDS, three grid barriers per iteration);
 * AUTO:       PERSISTENT for eligible runs with the AUTO NN variant (an explicitly chosen NN
 *             variant runs its own search cascade), else LAUNCHES.  The default.
 * The environment variable ICP_RUN_MODE=launches|persistent overrides (A/B runs). */
/* Which distance the first minimum is taken over (default SQUARED):
 * SQUARED:  (dx*dx + dy*dy) + dz*dz -- the reference's GPU path (compute.cu:112-117,137);
 * CPU_SQRT: sqrt((pow(dx,2) + pow(dy,2)) + pow(dz,2)) with libm pow -- the reference's CPU path
 *           (src/cpu.cc:17-22, the `icp` binary).  The two differ only at near ties (sqrt merges
 *           squared distances an ulp apart; libm pow is not always x*x).  The device finds the
 *           queries with a near tie and the host evaluates those candidates with libm (the run
 *           then synchronises once per search; the one-launch loop is not used). */
#define ICP_NN_RULE_SQUARED 0
#define ICP_NN_RULE_CPU_SQRT 1
int icp_set_nn_rule(icp_ctx *ctx, int rule);

#define ICP_RUN_AUTO 0
#define ICP_RUN_LAUNCHES 1
#define ICP_RUN_PERSISTENT 2
int icp_set_run_mode(icp_ctx *ctx, int mode);

/* ---- partial overlap: the max-correspondence-distance gate --------------- */
/* dmax > 0 and finite (the clouds' units): icp_run drops, in every iteration, the pairs farther
 * apart than dmax (PCL / Open3D max_correspondence_distance).  With D = dmax * dmax in fp64 and
 * d2_j = (dx*dx + dy*dy) + dz*dz between scene point j and its correspondence, pair j is kept
 * when d2_j <= D; K = the pairs kept over all ranks.  Horn's closed form runs over the kept
 * pairs with N = K, EVERY point is transformed (the outliers move with the cloud), and
 * err = (e + e) / K with e the kept pairs' residual.  An iteration with K < 4 stops the run
 * before it changes anything: icp_run returns ICP_E_TOO_FEW_POINTS with res and err_trace
 * filled for the completed iterations and the scene as the last completed one left it.
 * A gated run always takes the launch loop (ICP_RUN_LAUNCHES), whatever icp_set_run_mode says.
 * 0 or +inf switches the gate off (the default: icp_run exactly as without this call); a
 * negative value or NaN is ICP_E_ARG.  The setting survives icp_set_scene / icp_set_model. */
int icp_set_max_distance(icp_ctx *ctx, double dmax);
/* The last gate the last gated icp_run evaluated: the last recorded iteration's, or the failing
 * one's after ICP_E_TOO_FEW_POINTS.  mask_out (nullable): this rank's np_local flags (0 / 1) in
 * the caller's point order; count_out (nullable): K over all ranks.  ICP_E_NO_MODEL if no gated
 * run has happened since icp_set_scene. */
int icp_get_inliers(icp_ctx *ctx, uint8_t *mask_out, long long *count_out);
/* K of each recorded iteration of the last gated icp_run: writes min(cap, iterations) entries
 * (counts_out may be NULL when cap is 0) and returns the number of recorded iterations (>= 0),
 * or ICP_E_NO_MODEL as icp_get_inliers. */
int icp_get_inlier_trace(icp_ctx *ctx, long long *counts_out, size_t cap);

/* ---- the point-to-plane metric ------------------------------------------- */
/* ICP_METRIC_POINT_TO_PLANE: icp_run minimises, in every iteration, the kept pairs' squared
 * distance along the model's normal (Chen-Medioni; Low 2004) instead of Horn's point-to-point
 * closed form.  With y_j = m[idx_j] and n_j = N[idx_j] the correspondence and its normal,
 * c the model's centroid, a_j = [(p_j - c) x n_j ; n_j] and r_j = (p_j - y_j) . n_j, the iteration
 * solves (sum a_j a_j^T) x = -sum a_j r_j in fp64 (Cholesky of the system scaled to a unit
 * diagonal) on the device, and moves EVERY point by q = R p + t with R = exp([x[0..2]]x) (Rodrigues)
 * and t = (c + x[3..5]) - R c; err = (e + e) / K with e = sum ((q_j - y_j) . n_j)^2 over the K kept
 * pairs.  There is no scale: res->s is 1 in this mode.  The pairs kept are those of
 * icp_set_max_distance (all of them when the gate is off; icp_get_inliers / icp_get_inlier_trace
 * then keep reporting the last GATED run).  An iteration with K < 6 stops the run before it
 * changes anything with ICP_E_TOO_FEW_POINTS, as the gate's K < 4 does; one whose system has a
 * diagonal entry not > 0 or, scaled, a Cholesky pivot not > 1e-12 (a planar model, a surface of
 * revolution with exact normals) stops it the same way with ICP_E_DEGENERATE, and icp_last_error
 * names the iteration and the smallest pivot.  A point-to-plane run always takes the launch loop
 * (ICP_RUN_LAUNCHES), whatever icp_set_run_mode says; without normals it returns ICP_E_NO_MODEL.
 * ICP_METRIC_POINT_TO_POINT (the default): icp_run exactly as without this call.  Another value is
 * ICP_E_ARG.  The setting survives icp_set_scene / icp_set_model. */
#define ICP_METRIC_POINT_TO_POINT 0
#define ICP_METRIC_POINT_TO_PLANE 1
int icp_set_metric(icp_ctx *ctx, int metric);
/* The resident model's normals: n_xyz is a host array, 3 x nm column-major like a cloud, normal j
 * belonging to model point j.  They are used AS GIVEN: the engine does not renormalise them, and a
 * zero normal makes its pairs contribute nothing to the system or the error.  ICP_E_NO_MODEL
 * without a model, ICP_E_SIZE_MISMATCH if nm differs from the resident model's, ICP_E_ARG for a
 * null pointer or a non-finite value.  Every icp_set_model* call that changes the model drops
 * them; icp_ensure_model keeps them when it did not upload. */
int icp_set_model_normals(icp_ctx *ctx, const double *n_xyz, size_t nm);
/* The same array already in device memory, read like icp_set_model_device's (after the work of any
 * stream; valid until the call returns); its values are not checked for finiteness. */
int icp_set_model_normals_device(icp_ctx *ctx, const double *n_xyz_dev, size_t nm);

/* ---- robust weights: iteratively re-weighted least squares ------------------ */
/* With a kind other than ICP_ROBUST_NONE, every pair the gate keeps enters the iteration's sums
 * multiplied by a weight w_j of its residual at the current pose (PCL / Open3D robust kernels).
 * With d = p_j - y_j the residual is r2_j = (dx*dx + dy*dy) + dz*dz, the gate's own d2, under
 * ICP_METRIC_POINT_TO_POINT, and r2_j = r_j * r_j with r_j = (dx*nx + dy*ny) + dz*nz under
 * ICP_METRIC_POINT_TO_PLANE (with icp_set_plane_to_plane: the squared Mahalanobis residual d^T M d
 * of that iteration, so k is in those units: for a residual along both normals, 1 / sqrt(2 epsilon)
 * times the distance).  With k in the clouds' units and k2 = k * k (fp64, once, on the host):
 *   ICP_ROBUST_HUBER   w = r2 <= k2 ? 1 : k / sqrt(r2)
 *   ICP_ROBUST_TUKEY   w = r2 < k2 ? (1 - r2/k2)^2 : 0
 *   ICP_ROBUST_CAUCHY  w = 1 / (1 + r2/k2)
 * in fp64 as written; a NaN residual weighs 0.  Each of the pair's terms t of the unweighted
 * iteration (the 17 shifted moments, or the 21 + 6 entries of A and b) is summed as w * t, and two
 * sums join the kept count K: W = sum w and K+ = #{w > 0}, over all ranks.  Point-to-point: Horn's
 * closed form on the weighted sums with N = W (weighted centroids, S, and scale).  Point-to-plane:
 * (sum w a a^T) x = -sum w a r, solved as the unweighted system.  An iteration with K or K+ below
 * the metric's least count (4 / 6) stops the run before it changes anything with
 * ICP_E_TOO_FEW_POINTS, and icp_last_error names the iteration, K and K+.  Everything else is the
 * unweighted loop's: every point moves, err = (e + e) / K stays the kept pairs' UNWEIGHTED
 * residual (Open3D's inlier_rmse; a threshold keeps its meaning), and icp_get_inliers /
 * icp_get_inlier_trace keep reporting the gate.  A robust run always takes the launch loop
 * (ICP_RUN_LAUNCHES), whatever icp_set_run_mode says; it combines with the gate (off: every pair is
 * kept and weighted), both metrics, ranks and communicators.
 * k must be finite and > 0 with k * k finite and > 0, and the kind one of the four: anything else
 * is ICP_E_ARG and leaves the earlier setting.  With ICP_ROBUST_NONE (the default: icp_run exactly
 * as without this call) k is ignored.  The setting survives icp_set_scene / icp_set_model. */
#define ICP_ROBUST_NONE 0
#define ICP_ROBUST_HUBER 1
#define ICP_ROBUST_TUKEY 2
#define ICP_ROBUST_CAUCHY 3
int icp_set_robust(icp_ctx *ctx, int kind, double k);
/* W and K+ of each recorded iteration of the last robust icp_run: writes min(cap, iterations)
 * entries to each array that is not NULL and returns the number of recorded iterations (>= 0), or
 * ICP_E_NO_MODEL if no robust run has happened since icp_set_scene. */
int icp_get_robust_trace(icp_ctx *ctx, double *wsum_out, long long *active_out, size_t cap);

/* ---- partial overlap without a length: the trimmed fraction ----------------- */
/* 0 < fraction < 1: every iteration of icp_run keeps the T pairs with the smallest d2 (trimmed
 * ICP, Chetverikov et al.; PCL's CorrespondenceRejectorTrimmed), the expected overlap fraction
 * instead of a length in the clouds' units.  T = max(1, (long long)(fraction * (double)np_total)):
 * the product in fp64 as written, truncated, once on the host.  With d2_j = (dx*dx + dy*dy) + dz*dz
 * between scene point j and its correspondence (the gate's own value, under either metric), C is
 * the T-th smallest d2 over all ranks (1-based), selected on the device, and pair j is kept when
 * d2_j <= min(D, C), D = dmax * dmax of icp_set_max_distance or +inf when the gate is off.  Ties at
 * C are all kept: K >= T when the trim binds, K does not depend on the points' order or the number
 * of ranks, and no index breaks a tie.  Everything after the cut is the gated loop's: N = K (W with
 * robust weights, which apply to the kept pairs), every point moves, err = (e + e) / K, and K below
 * the metric's least count (4 / 6) stops the run before it changes anything with
 * ICP_E_TOO_FEW_POINTS; so does T below it, and icp_last_error names the iteration, K and T.  A
 * trimmed run counts as a gated one for icp_get_inliers / icp_get_inlier_trace (the mask and K of
 * min(D, C)), and always takes the launch loop (ICP_RUN_LAUNCHES), whatever icp_set_run_mode says.
 * fraction == 1 switches the trim off (the default: icp_run exactly as without this call);
 * fraction <= 0, > 1 or NaN is ICP_E_ARG and leaves the earlier setting.  The setting survives
 * icp_set_scene / icp_set_model. */
int icp_set_trim(icp_ctx *ctx, double fraction);
/* C of each recorded iteration of the last trimmed icp_run, the selected d2 itself (before the
 * min with the gate; every rank reports the same bits): writes min(cap, iterations) entries
 * (cut_d2_out may be NULL when cap is 0) and returns the number of recorded iterations (>= 0), or
 * ICP_E_NO_MODEL if no trimmed run has happened since icp_set_scene. */
int icp_get_trim_trace(icp_ctx *ctx, double *cut_d2_out, size_t cap);

/* ---- partial overlap without a parameter: one-to-one correspondences -------- */
/* on == 1: of all the scene points that chose model point j, only the closest is a pair (PCL's
 * CorrespondenceRejectorOneToOne, libpointmatcher's unique-match filter).  With
 * d2_i = (dx*dx + dy*dy) + dz*dz between scene point i and its correspondence idx_i (the gate's own
 * value, under either metric) and B_j = min{ d2_i : idx_i = j }, found on the device, pair i is kept
 * when d2_i == B_{idx_i} and d2_i <= min(D, C), D and C the gate's and the trim's exactly as without
 * this call: C is still selected over all pairs and T is unchanged.  The gate and the trim cannot
 * change the winner: a model point's winner has its smallest d2, so if the winner fails the gate or
 * the cut every other pair of that point fails too; "the winner among all pairs" and "the winner
 * among the kept" are the same set, and the three rejectors are independent predicates.  Ties are
 * kept whole, as at the trim's cut: two scene points at the same smallest d2 of a model point (two
 * identical points, say) are both pairs, no index breaks a tie, and the mask and K do not depend on
 * the points' order or on the schedule.  A NaN d2 never wins and is never kept.  Everything after
 * the mask is the gated loop's: N = K (W with robust weights, which apply to the kept pairs), every
 * point moves, err = (e + e) / K, and K below the metric's least count (4 / 6) stops the run before
 * it changes anything with ICP_E_TOO_FEW_POINTS; icp_last_error names the iteration and K and says
 * that one-to-one is on.  A one-to-one run counts as a gated one for icp_get_inliers /
 * icp_get_inlier_trace, and always takes the launch loop (ICP_RUN_LAUNCHES), whatever
 * icp_set_run_mode says.  It combines with the gate, the trim, robust weights, every metric
 * (point-to-point, point-to-plane and its symmetric and plane-to-plane forms), icp_run_pyramid and
 * icp_set_allow_unequal.  Ranks are not supported: B_j over ranks is a min-reduction, which the
 * engine's sum all-reduce cannot express, and with world_size > 1 icp_run returns ICP_E_ARG before
 * it enqueues anything.
 * on == 0 switches it off (the default: icp_run exactly as without this call); any other value is
 * ICP_E_ARG and leaves the earlier setting.  The setting survives icp_set_scene / icp_set_model. */
int icp_set_one_to_one(icp_ctx *ctx, int on);

/* ---- normals estimated from the model itself: grid k-NN and PCA ------------ */
/* The k nearest model points of every point of the resident model, searched over the model's grid.
 * 1. Neighbour set.  With d = m_j - m_i and d2 = (dx*dx + dy*dy) + dz*dz in fp64 exactly as written,
 *    N_j is the first k model indices i in ascending (d2, i) order: ties go to the lower index, the
 *    first-minimum rule extended to k.  The point itself is a candidate like any other (with
 *    duplicate points it need not come first).  Row j of idx (host, nm x k) is N_j in that order;
 *    d2 (nullable, host, nm x k) the matching distances.
 * icp_estimate_model_normals makes the normals of the resident model from those neighbourhoods:
 * 2. Covariance, two passes in the order of N_j: mu = (sum m_i) / k, C = sum (m_i - mu)(m_i - mu)^T
 *    (six entries, fp64, the difference taken before any product).  The order is fixed, so two calls,
 *    and every rank of a job (the model is replicated; there is no communication), give the same bits.
 * 3. Normal.  With l0 <= l1 <= l2 the eigenvalues of C (cyclic Jacobi, fp64, a fixed number of
 *    sweeps), the direction is undetermined when !(l2 > 0) or l1 - l0 <= 1e-12 * l2 (all points
 *    equal, collinear neighbours, a neighbourhood symmetric about an axis): the normal is then
 *    (0, 0, 0) -- icp_run's point-to-plane metric gives such a point's pairs no weight -- and the
 *    point is counted in *degenerate (nullable).  The 1e-12 is a condition, not a measurement: below
 *    it the eigenvector has lost 12 of fp64's 16 digits.  Otherwise the normal is the unit
 *    eigenvector of l0.
 * 4. Sign.  With a viewpoint v (nullable, 3 doubles): flipped so that n . (v - m_j) >= 0; without:
 *    so that its component of largest magnitude is positive (ties: the lowest axis).  The sign is
 *    immaterial to icp_run: a_j a_j^T and a_j r_j are even in n.
 * 5. The normals become the context's, exactly as icp_set_model_normals_device leaves them: every
 *    icp_set_model* call that changes the model drops them, icp_ensure_model keeps them when it did
 *    not upload.  The metric setting is not touched, and nothing else a run depends on changes: an
 *    icp_run after an estimate is bit-identical to that run on a fresh context.
 * Errors: ICP_E_NO_MODEL without a model; ICP_E_ARG for a null required pointer, k < 3, k > 64,
 * k > nm or a non-finite viewpoint (icp_last_error names the value; nothing has run, so earlier
 * normals stay).  icp_get_model_normals copies the context's normals, however they were set, to a
 * host array (3 x nm column-major like a cloud); ICP_E_NO_MODEL without a model or without normals. */
int icp_model_knn(icp_ctx *ctx, int k, int32_t *idx, double *d2);
int icp_estimate_model_normals(icp_ctx *ctx, int k, const double *viewpoint, long long *degenerate);
int icp_get_model_normals(icp_ctx *ctx, double *n_xyz);

/* ---- the symmetric point-to-plane iteration: the scene's normals too -------- */
/* icp_set_plane_symmetric(ctx, 1): with ICP_METRIC_POINT_TO_PLANE every iteration of icp_run minimises
 * the symmetric objective (Rusinkiewicz, "A Symmetric Objective Function for ICP", SIGGRAPH 2019):
 * the plane iteration with a second normal, the scene's.  It is exact to second order where
 * point-to-plane is exact only on a flat model, and converges from larger rotations.  One iteration,
 * with N the model's normals, u0 the scene's as given, c the model's centroid and Q the rotation of
 * icp_get_transform at the iteration's start:
 * 1. The search, y_j = m[idx_j], d = p_j - y_j, the gate, the trim, the mask and K: unchanged.
 * 2. N_j = N[idx_j], u_j = Q u0_j (each row summed as ((Q0 u0 + Q1 u1) + Q2 u2)), h = (Nx ux + Ny uy)
 *    + Nz uz.  If N_j is all zero or u0_j is all zero, n_j = 0: the pair counts in K and adds nothing
 *    else.  Otherwise n_j = h < 0 ? N_j - u_j : N_j + u_j, so the sign of any normal of either cloud
 *    changes no bit of a run (estimated normals have no consistent orientation).
 * 3. v_j = (p_j - c) + (y_j - c), a_j = [v_j x n_j ; n_j], r_j = (dx nx + dy ny) + dz nz; A = sum a a^T,
 *    b = -sum a r, the count, and with robust weights w(r * r), W and K+: the plane metric's sums.
 * 4. The least counts (K, K+, the trim's T >= 6), the scaled Cholesky, the 1e-12 pivot,
 *    ICP_E_TOO_FEW_POINTS and ICP_E_DEGENERATE: the plane metric's.
 * 5. With a~ = x[0..2], t~ = x[3..5]: aa = (a~0^2 + a~1^2) + a~2^2, g = 1 / sqrt(1 + aa), k2 = g g / (1 + g),
 *    R_h = I + g [a~]x + k2 [a~]x^2 (the half rotation; g is the half angle's cosine: no trigonometry),
 *    R = R_h R_h, t = ((R_h (g t~)) + c) - R c, s = 1: q = c + R_h (R_h (p - c) + g t~) -- the scene turns
 *    half way towards the model and the model, implicitly, half way back.
 * 6. Every point moves by (R, t); the step is composed into icp_get_transform's total.
 * 7. err = (e + e) / K with e = sum over the kept pairs of ((q_j - y_j) . n'_j)^2, n'_j formed by rule 2
 *    from N_j and u'_j = Q' u0_j, Q' the total's rotation with this step composed.  n is a sum of two
 *    unit normals, so this err -- icp_result.err, the error trace, and what the threshold of icp_run
 *    is compared with -- is up to FOUR TIMES the one-sided metric's for the same pose.
 * It works with the gate, the trim, robust weights, ranks and communicators as the plane metric
 * does, in the same launch loop.  on = 0 (the default), or the point-to-point metric: icp_run
 * exactly as without this call, whether or not scene normals are resident.  A value other than 0
 * or 1 is ICP_E_ARG.  The setting survives icp_set_scene / icp_set_model, like the metric.  With it on,
 * icp_run without model normals or without scene normals returns ICP_E_NO_MODEL, and icp_last_error
 * names the missing setter. */
int icp_set_plane_symmetric(icp_ctx *ctx, int on);
/* The resident scene's normals: n_xyz is a host array, 3 x np_local column-major like a cloud, row j
 * belonging to point j of this rank's scene as icp_set_scene* received it, in that scene's frame.
 * The context keeps them AS GIVEN (u0): never renormalised, never rewritten.  The CURRENT normal of
 * point j is u_j = Q u0_j with Q the rotation of icp_get_transform, so the normals follow every applied
 * iteration of every icp_run (whatever its loop or metric) and every icp_transform_scene; a frozen
 * iteration does not move them.  ICP_E_NO_MODEL without a scene, ICP_E_SIZE_MISMATCH if np_local
 * differs from the resident scene's, ICP_E_ARG for a null pointer or a non-finite value.  Every
 * icp_set_scene* call drops them, and icp_voxel_downsample* does not carry them. */
int icp_set_scene_normals(icp_ctx *ctx, const double *n_xyz, size_t np_local);
/* The same array already in device memory, read like icp_set_scene_device's (after the work of any
 * stream; valid until the call returns); its values are not checked for finiteness. */
int icp_set_scene_normals_device(icp_ctx *ctx, const double *n_xyz_dev, size_t np_local);
/* The CURRENT normals Q u0, in the caller's point order, to a host array (3 x np_local);
 * ICP_E_NO_MODEL without a scene or without scene normals. */
int icp_get_scene_normals(icp_ctx *ctx, double *n_xyz);
/* The normals of the resident scene, estimated from the scene itself with icp_estimate_model_normals'
 * kernels over a temporary grid of the scene: steps 1-4 of that contract with "model" read as
 * "scene", ties going to the lower index in the caller's point order.  The result is bit for bit
 * what icp_estimate_model_normals(k, viewpoint) gives on a fresh context whose model is these scene
 * points, and becomes the context's scene normals as icp_set_scene_normals_device leaves them.
 * Allowed only on an unsharded scene (np_local == np_total) that no icp_run or icp_transform_scene
 * has touched since icp_set_scene*: otherwise ICP_E_ARG, and icp_last_error says which.  k as the
 * model's estimator checks it (3 <= k <= 64, k <= np_local); ICP_E_NO_MODEL without a scene;
 * ICP_E_RANGE for a scene with a non-finite coordinate.  It touches nothing a run depends on except
 * the scene normals, and needs no model. */
int icp_estimate_scene_normals(icp_ctx *ctx, int k, const double *viewpoint, long long *degenerate);

/* ---- the plane-to-plane iteration (generalised ICP) from both clouds' normals ---- */
/* icp_set_plane_to_plane(ctx, epsilon) with 0 < epsilon <= 1: with ICP_METRIC_POINT_TO_PLANE every
 * iteration of icp_run minimises the plane-to-plane objective of generalised ICP (Segal, Haehnel and
 * Thrun, RSS 2009) in the regularised form of PCL's GeneralizedIterativeClosestPoint and Open3D's
 * registration_generalized_icp, whose default epsilon is 1e-3: a point's covariance has the eigenvalues
 * (epsilon, 1, 1), epsilon along its normal, C = I - (1 - epsilon) n n^T.  The covariances are a function
 * of the normals the context holds, and the scene's turn with the scene because its normals do.  One
 * iteration, with N the model's normals, u0 the scene's as given, c the model's centroid, Q the rotation
 * of icp_get_transform at the iteration's start and k1 = 1 - epsilon (fp64, once):
 * 1. The search, y_j = m[idx_j], d = p_j - y_j, the gate, the trim, the mask and K: unchanged.
 * 2. N_j = N[idx_j], u_j = Q u0_j (rows summed as ((Q0 u0 + Q1 u1) + Q2 u2)).  S = 2 I - k1 (N_j N_j^T +
 *    u_j u_j^T), six entries s_ab = [a == b ? 2 : 0] - k1 * (N_a * N_b + u_a * u_b).  A zero normal gives
 *    that cloud's covariance as I; the sign of a normal changes no bit.  Normals are used as given and are
 *    expected to be unit or zero: when S is not positive definite (s00 > 0, s00 s11 - s01 s01 > 0 and
 *    det S > 0, each false for a NaN) the pair counts in K and adds nothing else.  M_j = adj(S) * (1 / det S)
 *    in fp64; the condition number of S is at most 1 / epsilon.
 * 3. v = p_j - c, g = M_j d, r2 = d . g (the squared Mahalanobis residual), w = the robust weight of r2 (1
 *    without).  With J = [-[v]x | I]: A = sum w J^T M_j J, b = -sum w [v x g ; g], the count, and with
 *    weights W and K+: the plane metric's 28 (30) sums in its columns.  For M = n n^T they are the plane
 *    metric's own.
 * 4. The fold, the all-reduce, the least counts (6), the scaled Cholesky with the 1e-12 pivot and the
 *    step R = exp([omega]x), t = (c + tau) - R c, s = 1 are the one-sided plane metric's: one
 *    Gauss-Newton step a search, as Open3D does.
 * 5. Every point moves; err = (e + e) / K with e = sum over the kept pairs of (q_j - y_j)^T M'_j (q_j -
 *    y_j), M' from Q' u0, Q' the total's rotation with this step composed.  This err -- icp_result.err,
 *    the trace, what the threshold is compared with -- carries the tangential distance with weight 1/2:
 *    between different samplings of one surface it does not fall to zero.
 * The tangential term of weight epsilon also registers a planar model, where both other forms stop with
 * ICP_E_DEGENERATE.  It works with the gate, the trim, robust weights, ranks (with given scene normals)
 * and communicators as the plane metric does.  epsilon = 0 (the default) is off: icp_run exactly as
 * without this call; with the point-to-point metric the switch has no effect.  A NaN, a negative value
 * or one above 1 is ICP_E_ARG and leaves the earlier setting.  The setting survives icp_set_scene /
 * icp_set_model.  On together with icp_set_plane_symmetric(1), icp_run returns ICP_E_ARG before it
 * changes anything; without model normals or scene normals it returns ICP_E_NO_MODEL, and
 * icp_last_error names the missing setter. */
int icp_set_plane_to_plane(icp_ctx *ctx, double epsilon);

/* ---- coarse-to-fine: the total transform, a pose for the scene, a voxel downsample -- */
/* icp_get_transform: the similarity q = s R p + t (R row-major) that maps the scene as icp_set_scene*
 * received it onto the resident scene now: every APPLIED iteration of every icp_run since then and
 * every icp_transform_scene, composed as (s2, R2, t2) o (s1, R1, t1) = (s2 s1, R2 R1, s2 R2 t1 + t2)
 * in fp64, each 3-term sum as ((a + b) + c); the first step is copied, so after one iteration it has
 * icp_result's bits.  The identity after icp_set_scene*; s stays 1 under ICP_METRIC_POINT_TO_PLANE.
 * The step of an iteration that stopped the run before it changed anything (ICP_E_TOO_FEW_POINTS,
 * ICP_E_DEGENERATE) is not part of it.  The steps come from all-reduced sums, so every rank of a job
 * reports the same bits.  ICP_E_NO_MODEL without a scene, ICP_E_ARG for a null pointer.
 * icp_transform_scene: moves this rank's resident scene by q = sR p + t, with sR = s * R formed once
 * on the host and q = ((sR0 p0 + sR1 p1) + sR2 p2) + t per row, the iterations' own arithmetic; R is
 * used as given.  The transform is composed into the total, and the context is left exactly as
 * icp_set_scene of the moved points would leave it (the correspondences, the gate's and the robust
 * weights' reports are dropped; the scene is prepared again by the set-up's own passes): an icp_run
 * after it is bit-identical to that run on a fresh context given icp_get_scene's points.
 * ICP_E_ARG for a null pointer, a non-finite value or s <= 0; ICP_E_NO_MODEL without a scene. */
int icp_get_transform(icp_ctx *ctx, double *s, double R[9], double t[3]);
int icp_transform_scene(icp_ctx *ctx, double s, const double R[9], const double t[3]);
/* One point per occupied cell of a cubic lattice of side `voxel`: the mean of the cell's points.
 * 1. Cell.  With lo_a = origin ? origin[a] : min_i x_a, a point's cell per axis is
 *    c_a = floor((x_a - lo_a) / voxel) in fp64 exactly as written (IEEE division, no reciprocal), and
 *    g_a = 1 + max_i c_a.  Two clouds downsampled with the same origin share the lattice.
 * 2. Key.  (c_z * g_y + c_y) * g_x + c_x, 64 bits.
 * 3. Output.  Point v of xyz_out is the mean (sum x_i) / L_v of the L_v points of the v-th occupied cell
 *    in ascending key order, count_out[v] (nullable) = L_v, *n_out the number of occupied cells.
 *    xyz_out and count_out have room for n entries.
 * 4. Order of the sum: a pure function of the input (no floating-point atomics; two calls give the
 *    same bits, the host and the device form too).  A cell's points in input order are cut into
 *    chunks of 1,024; in a chunk 64 partial sums start from +0 and take the points l, l + 64, ... in
 *    order, and are combined by the butterfly a_l += a_(l xor 32), 16, 8, 4, 2, 1; the chunk sums are
 *    added, from +0, in chunk order.  Any order satisfies
 *    |mean - exact mean| <= (L + 1) 2^-53 max_i |x_i| per axis.
 * xyz: 3 x n column-major like a cloud; origin (nullable): 3 host doubles.  The device form takes
 * xyz, xyz_out and count_out in device memory, read like icp_set_model_device's array (after the work
 * of any stream; valid until the call returns).  Both calls are synchronous (*n_out is on the host)
 * and touch neither the resident clouds nor anything a run depends on: an icp_run after one is
 * bit-identical to that run without it.
 * ICP_E_ARG: a null required pointer, n == 0, n > INT_MAX, voxel not finite or not > 0, a non-finite
 * origin or (host form) a non-finite coordinate.  ICP_E_RANGE: some c_a < 0 (a point below an explicit
 * origin) or some g_a > 2^21 (icp_last_error names the axis and the value); the device form: a
 * non-finite coordinate, as icp_set_model_device.  Nothing is written to the outputs on an error. */
int icp_voxel_downsample(icp_ctx *ctx, const double *xyz, size_t n, double voxel, const double *origin,
                         double *xyz_out, int32_t *count_out, size_t *n_out);
int icp_voxel_downsample_device(icp_ctx *ctx, const double *xyz_dev, size_t n, double voxel, const double *origin,
                                double *xyz_out_dev, int32_t *count_out_dev, size_t *n_out);

/* ---- outlier removal: the statistical and the radius filter ------------------ */
/* What a raw scan needs before normals, descriptors, a downsample or icp_run: its isolated returns
 * (flying pixels, dust, multipath) removed.  PCL's StatisticalOutlierRemoval / RadiusOutlierRemoval and
 * Open3D's remove_statistical_outlier / remove_radius_outlier, over a temporary grid of the cloud built
 * as icp_estimate_scene_normals builds the scene's (its device memory and the filters' own are scratch
 * of the context, kept for the next filter call and freed with the context).  xyz: n points,
 * 3 x n column-major like a cloud.  d2 between two points is (dx*dx + dy*dy) + dz*dz in fp64 exactly
 * as written.
 *
 * icp_filter_statistical(k, std_ratio):
 * 1. Neighbour list.  L_j is the first k + 1 indices i in ascending (d2, i) order of point j's distances
 *    to every point of the cloud: icp_model_knn's rule 1 with k + 1, the same search; the point itself is
 *    a candidate like any other.
 * 2. Mean distance.  dbar_j = (sum over the k + 1 entries of L_j, in list order from +0, of sqrt(d2)) / k:
 *    PCL's mean over the k other points, the self entry adding 0.  With k + 2 or more equal points every
 *    entry is 0 and dbar_j = 0.  mean_dist_out (nullable, n) = dbar.
 * 3. Moments, two passes: mu = S(dbar) / n, then sigma = sqrt(S((dbar_j - mu) * (dbar_j - mu)) / (n - 1)).
 *    S sums a sequence of L terms in an order that depends on L alone: the sequence is cut into chunks of
 *    1,024; in a chunk 64 partial sums start from +0 and take the terms l, l + 64, l + 128, ... in order
 *    and are combined by the butterfly a_l += a_(l xor 32), 16, 8, 4, 2, 1; a single chunk's sum is S;
 *    otherwise the chunk sums in chunk order are a sequence of ceil(L / 1024) terms and S is that
 *    sequence's S.  No floating-point atomics: two calls, and the host and the device form, give the
 *    same bits.
 * 4. T = mu + std_ratio * sigma (the product rounded, then the sum).  Point j is kept iff dbar_j <= T.
 * 5. stats_out (nullable) = (mu, sigma, T).
 *
 * icp_filter_radius(radius, min_neighbors):
 * 1. c_j = #{ i : d2(j, i) <= radius * radius }, the product taken once on the host.  The point itself is
 *    counted, so c_j >= 1.
 * 2. Point j is kept iff c_j > min_neighbors: at least min_neighbors OTHER points within the radius
 *    (PCL's and Open3D's rule).
 * 3. count_out (nullable, n) = c_j, the full counts.  Without it the scan of a point may stop at
 *    min_neighbors + 1; the mask is the same either way.
 *
 * Both: the kept points go to out_xyz (nullable, room for n points) in their input order, mask_out
 * (nullable, n) holds 1 for a kept point and 0 for a removed one, *n_out (required) the number kept; 0
 * is a valid result and ICP_OK.  The calls are synchronous, write their outputs only once everything
 * has run, and touch neither the resident clouds, the normals nor any setting: an icp_run after one is
 * bit-identical to that run on a fresh context.  The device forms take xyz, out_xyz, mask_out and the
 * per-point mean_dist_out / count_out in device memory, read like icp_set_model_device's array (after
 * the work of any stream; valid until the call returns); n_out and stats_out stay host pointers.
 * Errors (icp_last_error names the value; nothing has run and nothing is written): ICP_E_ARG for a null
 * xyz or n_out, n == 0 or n > INT_MAX, k outside [2, 63] (the list of k + 1 entries must fit
 * icp_model_knn's 3 to 64), k + 1 > n, std_ratio negative or not finite, radius not finite or <= 0,
 * min_neighbors < 0; ICP_E_RANGE for a non-finite coordinate. */
int icp_filter_statistical(icp_ctx *ctx, const double *xyz, size_t n, int k, double std_ratio,
                           double *out_xyz, uint8_t *mask_out, size_t *n_out, double *mean_dist_out,
                           double stats_out[3]);
int icp_filter_statistical_device(icp_ctx *ctx, const double *xyz_dev, size_t n, int k, double std_ratio,
                                  double *out_xyz_dev, uint8_t *mask_out_dev, size_t *n_out,
                                  double *mean_dist_out_dev, double stats_out[3]);
int icp_filter_radius(icp_ctx *ctx, const double *xyz, size_t n, double radius, int min_neighbors,
                      double *out_xyz, uint8_t *mask_out, size_t *n_out, int32_t *count_out);
int icp_filter_radius_device(icp_ctx *ctx, const double *xyz_dev, size_t n, double radius, int min_neighbors,
                             double *out_xyz_dev, uint8_t *mask_out_dev, size_t *n_out, int32_t *count_out_dev);

/* ---- a registration evaluated: fitness, inlier RMSE, the information matrix --- */
/* How good the pose reached is: Open3D's evaluate_registration and
 * get_information_matrix_from_point_clouds, PCL's getFitnessScore.  The call works on the resident model
 * and the resident scene AS IT LIES NOW: after every applied iteration of an icp_run and every
 * icp_transform_scene; the coordinates are the caller's.  (icp_run's err is the kept pairs' error of its
 * last iteration BEFORE the last step is applied, under that run's gate, trim and weights; this call
 * applies none of them.)
 *
 * 1. Distance.  d2(a, b) = (dx*dx + dy*dy) + dz*dz in fp64, exactly as written: the gate's own d2.  The
 *    nearest-neighbour rule is always the squared-distance first minimum, whatever icp_set_nn_rule and
 *    the context's nn_mode say.
 * 2. Forward pair.  D = max_dist * max_dist, the product taken once on the host; max_dist = +inf gives
 *    D = +inf.  For scene point j, i_j is the lowest index among the model points that minimise d2 and
 *    d2_j that minimum.  Pair j is kept iff d2_j <= D.  A kept point has idx_out[j] = i_j and
 *    d2_out[j] = d2_j; a point that is not kept has idx_out[j] = -1 and d2_out[j] = +inf (Open3D's
 *    correspondence set: a point with nothing within max_dist has no pair).  Both arrays are nullable,
 *    hold np entries and are in the caller's point order.
 *    With a finite max_dist a point far from the model costs the scan of a small box of cells.  With
 *    max_dist = +inf a point far outside the model's box scans every model point (its completeness box is
 *    over the cell budget): a scene of a million points with a far clump is far too slow at +inf; give
 *    such a scene a finite max_dist.
 * 3. Forward summary.  K is the number of kept pairs; fitness = K / np, one fp64 division;
 *    inlier_rmse = sqrt(S(t) / K) with t_j = d2_j for a kept pair and +0 otherwise; max_inlier_d2 is the
 *    maximum of the kept d2.  With K == 0 the last two are 0.
 * 4. Information matrix (Open3D's).  With y = m[i_j] = (x, y, z) as the caller gave it,
 *    A = sum over the kept pairs of G_j^T G_j, the rows of G_j being (0, z, -y, 1, 0, 0),
 *    (-z, 0, x, 0, 1, 0) and (y, -x, 0, 0, 0, 1).  It is formed from nine S-sums over the caller's order:
 *    Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz; each product is rounded first and a pair that is not kept
 *    contributes +0.  A00 = Syy + Szz, A11 = Sxx + Szz, A22 = Sxx + Syy; A01 = -Sxy, A02 = -Sxz,
 *    A12 = -Syz; A04 = -Sz, A05 = Sy, A13 = Sz, A15 = -Sx, A23 = -Sy, A24 = Sx; A33 = A44 = A55 = K.  A is
 *    symmetric and every other entry is 0.  information[] is row-major, the rotation block first.
 * 5. Sum order.  S is the filters' sum rule (icp_filter_statistical's rule 3 above), over the np (or nm)
 *    terms in the caller's point order.  No floating-point atomics: two calls give the same bits, and so
 *    do the host and the device form.  (K and the maximum are integer atomics: a non-negative double
 *    orders as its bit pattern.)
 * 6. Reverse direction (both != 0): the same with the roles exchanged.  For model point i the lowest
 *    caller's-order index among the scene points that minimise d2; model_idx_out and model_d2_out
 *    (nullable, nm entries, the model's order), K_m, model_fitness = K_m / nm, model_rmse and
 *    model_max_inlier_d2.  In partial overlap the scene can sit wholly on the model with fitness 1; the
 *    model's fitness says how much of the model it covers.  There is no second information matrix.  With
 *    both == 0 the five model fields are 0 and a non-null model_* array is ICP_E_ARG.
 * 7. Effects.  The call is synchronous, writes its outputs only once everything has run and changes
 *    nothing that a run or a report depends on: an icp_run after it returns the same bits as that run
 *    without it (the result, the error trace, icp_get_scene, icp_get_transform), and icp_get_indices,
 *    icp_get_inliers and the traces answer as before.  Its device memory is scratch of the context, kept
 *    for the next evaluation (a second call at the same sizes allocates nothing) and freed with it.
 * 8. Errors.  Nothing has run and nothing is written; icp_last_error names the value.  ICP_E_ARG: a null
 *    context; a null out; max_dist that is NaN or not > 0; rule 6's case; a context of more than one rank
 *    (the reverse minimum over shards would be a min-reduction: refused, as the one-to-one rejection
 *    refuses ranks).  ICP_E_NO_MODEL: no model or no scene.  The clouds' sizes need not be equal and no
 *    minimum count applies: those are icp_run's checks, not this call's.
 * The device form takes the four per-point arrays in device memory; out stays a host pointer. */
typedef struct icp_evaluation {
    long long scene_points;          /* np */
    long long correspondences;       /* K */
    double fitness;                  /* K / np */
    double inlier_rmse;              /* sqrt(S(d2 of the kept) / K); 0 when K == 0 */
    double max_inlier_d2;            /* the largest kept d2; 0 when K == 0 */
    double information[36];          /* row-major 6 x 6, rotation block first */
    long long model_points;          /* nm; this and the four below are 0 unless both != 0 */
    long long model_correspondences; /* K_m */
    double model_fitness, model_rmse, model_max_inlier_d2;
} icp_evaluation;

int icp_evaluate(icp_ctx *ctx, double max_dist, int both, icp_evaluation *out, int32_t *idx_out, double *d2_out,
                 int32_t *model_idx_out, double *model_d2_out);
int icp_evaluate_device(icp_ctx *ctx, double max_dist, int both, icp_evaluation *out, int32_t *idx_out_dev,
                        double *d2_out_dev, int32_t *model_idx_out_dev, double *model_d2_out_dev);

/* ---- global registration: FPFH descriptors, feature matches, a RANSAC pose ---- */
/* What a scene that does NOT start near its answer needs before icp_run: a pose from local shape
 * descriptors (Rusu, Blodow and Beetz, "Fast Point Feature Histograms (FPFH) for 3D Registration", ICRA
 * 2009; PCL's FPFHEstimation, Open3D's compute_fpfh_feature / registration_ransac_based_on_correspondence).
 * The four calls take host arrays, are synchronous, work on any context (a sharded one too: nothing is
 * communicated), need no resident cloud and touch neither the resident clouds nor anything a run
 * depends on: an icp_run after any of them is bit-identical to that run on a fresh context.
 *
 * icp_fpfh: the descriptors of the n points xyz (3 x n column-major like a cloud): fpfh_out is n x 33
 * row-major, spfh_out (nullable) the simplified histograms of rule 3, normals_out (nullable, 3 x n)
 * the normals used.
 * 1. Grid, normals, neighbours.  A temporary grid of the cloud is built as icp_estimate_scene_normals
 *    builds the scene's and freed before the call returns.  normals == NULL: they are estimated on that
 *    grid by the estimator's own kernels, bit for bit what icp_estimate_model_normals(k_normals,
 *    viewpoint) gives on a fresh context whose model is these points; else normals (3 x n) are used as
 *    given and k_normals and viewpoint are ignored.  N_i is icp_model_knn's list of point i for k: the
 *    same kernel, ascending (d2, index), the point itself a candidate.
 * 2. Pair feature of point i and list entry j (PCL's computePairFeatures); every dot product and 3-term
 *    sum is ((a + b) + c), a cross product a x b is (ay bz - az by, az bx - ax bz, ax by - ay bx).  With
 *    d = x_j - x_i and L2 = (dx dx + dy dy) + dz dz the pair is SKIPPED when j == i, L2 == 0 or either
 *    normal is all zero.  L = sqrt(L2), a1 = (N_i . d) / L, a2 = (N_j . d) / L.  If |a1| < |a2|:
 *    (n1, n2, e, f3) = (N_j, N_i, -d, -a2), else (N_i, N_j, d, a1) -- the frame on the point whose normal
 *    is closer to the line, as a comparison (no acos).  v = e x n1, vl2 = (vx vx + vy vy) + vz vz; vl2 == 0
 *    skips the pair, else each component of v is divided by sqrt(vl2).  w = n1 x v, f2 = v . n2,
 *    f1 = atan2(w . n2, n1 . n2).  Bins: b1 = clamp(floor(11 * ((f1 + pi) / (2 pi))), 0, 10), b2 the same
 *    of (f2 + 1) / 2, b3 of (f3 + 1) / 2; pi is M_PI, 2 pi is 2.0 * M_PI, a NaN goes to bin 0.
 * 3. SPFH_i[b] = (double)cnt_b * (100.0 / (double)c_i) with c_i the counted pairs of point i and cnt_b
 *    those in bin b (b1 in 0-10, 11 + b2, 22 + b3); all 0 when c_i = 0.  Integer counts: no order.
 * 4. FPFH (Open3D's form).  A[b] from +0; for the entries j of N_i in list order with j != i and
 *    d2_ij > 0 (the list's d2): A[b] += (1.0 / d2_ij) * SPFH_j[b].  Per third (bins 0-10, 11-21, 22-32): T
 *    = the sum of its A in ascending bin order from +0, A[b] = T > 0 ? A[b] * (100.0 / T) : 0.
 *    FPFH_i[b] = A[b] + SPFH_i[b].
 * Everything but atan2 is IEEE arithmetic as written; two calls give the same bits.
 * Errors: ICP_E_ARG for a null required pointer, n == 0, n > INT_MAX, k < 3, k > 64, k > n (and the
 * same for k_normals when normals == NULL), a non-finite viewpoint or given normal; ICP_E_RANGE for a
 * non-finite coordinate.  Nothing is written to the outputs on an error. */
#define ICP_FPFH_DIM 33
int icp_fpfh(icp_ctx *ctx, const double *xyz, size_t n, const double *normals, int k_normals,
             const double *viewpoint, int k, double *fpfh_out, double *spfh_out, double *normals_out);
/* For every row a of fa (na x 33) the nearest row of fb (nb x 33): D(a, b) = sum over c = 0..32 of
 * (fa[a][c] - fb[b][c])^2, summed from +0 in ascending c, the difference taken before the product;
 * idx_out[a] = the LOWEST b among the minimisers of D (the first-minimum rule in 33 dimensions),
 * dist_out[a] (nullable) its D.  A NaN D never wins: idx_out[a] = -1 (and dist_out[a] a NaN) when every
 * D is a NaN.  Brute force: na * nb * 33 subtract-multiply-adds in fp64 -- meant for downsampled clouds.
 * The mutual filter is two calls: keep a when idx_ba[idx_ab[a]] == a (icp_global_pose does that).
 * ICP_E_ARG for a null required pointer, na == 0, nb == 0 or either above INT_MAX.
 * icp_match_features_plan: how the search cuts fb for these sizes -- rows staged at a time (tile), rows a
 * workgroup's range (chunk, a multiple of tile) and the number of ranges (splits); for tests and tools. */
int icp_match_features(icp_ctx *ctx, const double *fa, size_t na, const double *fb, size_t nb,
                       int32_t *idx_out, double *dist_out);
int icp_match_features_plan(size_t na, size_t nb, int *tile, int *chunk, int *splits);
/* A rigid pose q = R p + t from C putative pairs p_c -> q_c (both 3 x C column-major) by RANSAC over 3-pair
 * samples.  Hypothesis h = 0 .. hypotheses - 1:
 * 1. Draw.  z_r = splitmix64(seed + (3 h + r + 1) * 0x9E3779B97F4A7C15) for r = 0, 1, 2, where
 *    splitmix64(x) is x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB;
 *    x ^= x >> 31, all mod 2^64.  i0 = z_0 % C; i1 = z_1 % (C - 1), then + 1 if >= i0; i2 = z_2 % (C - 2),
 *    then + 1 if >= min(i0, i1), then + 1 if >= max(i0, i1): three distinct pairs, a pure function of
 *    (seed, h, C).
 * 2. Edge check over the sample's index pairs (0, 1), (1, 2), (2, 0): with lp and lq the squared lengths
 *    ((dx dx + dy dy) + dz dz) in p and in q, the hypothesis is kept when min(lp, lq) >= e2 * max(lp, lq)
 *    for all three, e2 = edge_ratio * edge_ratio formed once.  A rejected hypothesis has count -1.
 * 3. Pose.  Centroids ((x0 + x1) + x2) / 3 per axis; p' = p - mu_p, q' = q - mu_q; S = sum p' q'^T (nine
 *    entries), d_caps = sum ((q'x q'x + q'y q'y) + q'z q'z) and sp likewise of p', each from +0 in the
 *    order r = 0, 1, 2; R = the rotation of icp_horn_solve(S, mu_p, mu_q, d_caps, sp) -- the same code, on
 *    the device; the scale is discarded: t = mu_q - R mu_p, rows as ((R0 m0 + R1 m1) + R2 m2).
 * 4. Count: the pairs with (dx dx + dy dy) + dz dz <= max_dist * max_dist (formed once), d = (((R0 p0 +
 *    R1 p1) + R2 p2) + t) - q per row: the iterations' arithmetic.
 * 5. Winner: the largest count, ties to the lowest h, decided on the device by an unsigned 64-bit atomic
 *    maximum over (count << 32) | (0xFFFFFFFF - h): an integer key, so no schedule changes the result.
 * Outputs: R (row-major), t, *inliers (the winner's count), *best_h, *evaluated (nullable: how many
 * passed the edge check), counts_out (nullable, one per hypothesis), mask_out (nullable, C: the
 * winner's inliers).  Hypotheses run in batches of 65,536, so device memory does not grow with them.
 * ICP_E_ARG: a null required pointer, C < 3, C > INT_MAX, hypotheses < 1 or >= 2^32, max_dist not finite
 * or not > 0, edge_ratio outside [0, 1], a non-finite point.  ICP_E_DEGENERATE: no hypothesis passed the
 * edge check (icp_last_error names H and the seed).  Nothing is written on an error. */
int icp_ransac_pose(icp_ctx *ctx, const double *p_xyz, const double *q_xyz, size_t C, long long hypotheses,
                    uint64_t seed, double max_dist, double edge_ratio, double R[9], double t[3],
                    long long *inliers, long long *best_h, long long *evaluated, int32_t *counts_out,
                    uint8_t *mask_out);
/* The chain, bit for bit what the public calls give when chained by hand: both clouds through
 * icp_voxel_downsample(voxel), each from its own origin; icp_fpfh of each with estimated normals
 * (k_normals, no viewpoint) and k_fpfh; icp_match_features scene -> model, and with mutual != 0 model ->
 * scene and the mutual filter; the surviving pairs in ascending (downsampled) scene index through
 * icp_ransac_pose.  q = R p + t maps the scene onto the model: ready for icp_transform_scene(1, R, t).
 * Zero fields of prm take defaults: k_normals 16, k_fpfh 32, hypotheses 100000 (Open3D's), max_dist
 * 1.5 * voxel, edge_ratio 0.9; seed 0 is used as it is and mutual as given.  ICP_E_ARG, before anything
 * runs: a null required pointer, nm or np outside [1, INT_MAX], voxel not finite or not > 0, and with the
 * defaults filled in a k outside [3, 64], hypotheses outside [1, 2^32), max_dist not finite or not > 0,
 * edge_ratio outside [0, 1].  ICP_E_TOO_FEW_POINTS: a downsampled cloud has fewer than max(k_normals, k_fpfh) points
 * (before any descriptor kernel runs), or fewer than 3 matches survive.  rep is nullable. */
typedef struct icp_global_params {
    double voxel;
    int k_normals, k_fpfh, mutual;
    long long hypotheses;
    uint64_t seed;
    double max_dist, edge_ratio;
} icp_global_params;
typedef struct icp_global_report {
    long long model_points, scene_points, matches, evaluated, inliers, best_h;
} icp_global_report;
int icp_global_pose(icp_ctx *ctx, const double *m_xyz, size_t nm, const double *p_xyz, size_t np,
                    const icp_global_params *prm, double R[9], double t[3], icp_global_report *rep);

/* ---- the ICP loop: GPU::ICP::find_corresponding_opti (src/GPU/gpu.cc:52-83) -- */
/* Runs up to max_iter iterations on the resident clouds; stops after the iteration
 * whose err < threshold (pass threshold < 0 to run exactly max_iter iterations).
 * err_trace (nullable, length max_iter) receives every iteration's err.
 * Returns ICP_E_SIZE_MISMATCH / ICP_E_TOO_FEW_POINTS like the reference's checks. */
int icp_run(icp_ctx *ctx, int max_iter, double threshold, double *err_trace, icp_result *res);

/* ---- per-operation surface (src/GPU/gpu.hh:110-116) ---------------------- */
/* compute_Y_w_opti (compute.cu:154-245): Y[:, j] = m[:, NN(p_j)] on the resident model.
 * y_xyz_out and idx_out are each nullable. */
int icp_closest_matrix(icp_ctx *ctx, const double *p_xyz, size_t np, double *y_xyz_out,
                       int32_t *idx_out);
/* rowwise().mean() + substract_col_w (gpu.cc:98-102, compute.cu:381-416):
 * mu = mean of the n points; centred_out (nullable) = points - mu. */
int icp_compute_centroid(icp_ctx *ctx, const double *xyz, size_t n, double mu[3],
                         double *centred_out);
/* substract_col_w (compute.cu:381-416): out[:, j] = xyz[:, j] - m for ANY 3-vector m
 * (gpu.cc:101-102 passes the host means rowwise().mean()).  out may alias xyz. */
int icp_subtract_col(icp_ctx *ctx, const double *xyz, size_t n, const double m[3], double *out);
/* y_p_norm_w (compute.cu:418-469): d_caps = sum ||y_j||^2, sp = sum ||p_j||^2 */
int icp_y_p_norm(icp_ctx *ctx, const double *y_xyz, const double *p_xyz, size_t n,
                 double *d_caps, double *sp);
/* compute_err_w (compute.cu:315-379): q_j = sR p_j + t; returns sum ||y_j - q_j||^2;
 * if in_place, p_xyz is overwritten with q (the reference writes p back, :367-368).
 * sR is the row-major 3x3 product s*R, t a 3-vector. */
int icp_err_compute(icp_ctx *ctx, const double *y_xyz, double *p_xyz, size_t n, int in_place,
                    const double sR[9], const double t[3], double *err);
/* ICP::find_alignment (gpu.cc:95-151): Horn's closed form aligning p onto y.
 * Outputs s, R (row-major), t and err = sum ||y - (sRp + t)||^2 (p is not modified). */
int icp_find_alignment(icp_ctx *ctx, const double *p_xyz, const double *y_xyz, size_t n,
                       double *s, double R[9], double t[3], double *err);

/* ---- host-only helpers (no device work) --------------------------------- */
/* The host half of find_alignment (gpu.cc:104-146) from the reduced sums:
 * S = sum p' y'^T (row-major), mu_p, mu_y, d_caps = sum ||y'||^2, sp = sum ||p'||^2. */
int icp_horn_solve(const double S[9], const double mu_p[3], const double mu_y[3], double d_caps,
                   double sp, double *s, double R[9], double t[3]);
/* max_element_index (gpu.cc:85-93) exactly as the reference writes it. */
int icp_max_element_index(const double ev[4]);
/* Contiguous shard of the scene for `rank` of `world_size` (first n % w ranks get +1). */
int icp_shard_range(size_t n_total, int rank, int world_size, size_t *begin, size_t *count);
/* Synthetic pair: n model points uniform in [-1,1]^3 from
 * std::mt19937_64(seed), rounded to fp32-representable doubles; scene = R(axis,angle) m + t
 * (computed in fp64, then rounded to fp32), same point order. */
int icp_synthetic_pair(uint64_t seed, size_t n, double angle_deg, const double axis[3],
                       const double t[3], double *model_xyz_out, double *scene_xyz_out);
/* load_matrix (src/load.cc:3-33): n = #lines - 1, header skipped, "%lf,%lf,%lf" per row.
 * *xyz_out is allocated with malloc; release with icp_free.  ICP_E_IO if unopenable. */
int icp_load_matrix(const char *path, double **xyz_out, size_t *n_out);
/* write_matrix (src/load.cc:68-81): header + 6-significant-digit rows. */
int icp_write_matrix(const char *path, const double *xyz, size_t n);
void icp_free(void *p);

/* ---- instrumentation ----------------------------------------------------- */
/* Correspondences of the last NN search over the resident scene (the last icp_run
 * iteration's compute_Y_w_opti, gpu.cc:69): idx_out[j] = model index of this rank's scene
 * point j (np_local entries).  ICP_E_NO_MODEL if no search has run since icp_set_scene.
 * A run with an all-reduce (ranks > 1 or a communicator) tests the error one iteration late;
 * when it stops on the threshold, the search of the iteration after the converged one has
 * already run, and these are its correspondences (of the final cloud). */
int icp_get_indices(icp_ctx *ctx, int32_t *idx_out);
/* Test instrumentation: with cap > 0, every icp_run iteration k < cap records a digest of its
 * correspondence indices (this rank's shard, local j): (sum idx[j], sum (j+1) idx[j],
 * #{idx[j] == j}), all mod 2^64, order-independent.  Each icp_run restarts at k = 0.
 * cap = 0 disables (the default: no extra launch). */
int icp_set_index_digest(icp_ctx *ctx, size_t cap);
/* Test instrumentation: 1 = audit every f16-certified query (extra fp64 work per query and
 * three atomics; results in icp_stats.cert_*), 0 = off (the default). */
int icp_set_cert_audit(icp_ctx *ctx, int enable);
/* Test instrumentation of the bundle filter's exclusions (a model with its bundle images, a
 * resident scene with correspondences): `groups` 32-query groups of the scene, each query's
 * correspondence as its seed, against every bundle.  max_err_ratio = max over the evaluated
 * (query, bundle) pairs of |V^ - (V - mu_q - mu_c)| / (mu_q + mu_c) (the exclusion is sound
 * while < 1); over the excluded pairs near the bound, violations counts a bundle holding a
 * point at least as close as the seed (0 when sound) and min_gap the smallest relative D64 gap
 * (D64 min - D_seed) / D_seed.  Synchronous; ICP_E_NO_MODEL without bundle images or seeds. */
typedef struct icp_bundle_audit_result {
    double max_err_ratio;
    double min_gap;
    long long pairs, excluded, checked, violations;
} icp_bundle_audit_result;
int icp_bundle_audit(icp_ctx *ctx, int groups, icp_bundle_audit_result *out);
int icp_get_index_digest(icp_ctx *ctx, uint64_t *out, size_t cap);

/* The counters since the context was created or icp_reset_stats.  run_certified / run_walked are
 * kept on the device while the runs' scene size stays the same (no synchronisation at a run's
 * start), so icp_get_stats synchronises the context's stream to read them. */
int icp_get_stats(const icp_ctx *ctx, icp_stats *out);
int icp_reset_stats(icp_ctx *ctx);
/* Instrumentation of the bundle filter (ICP_NN_VARIANT_BUNDLE): with enable = 1 its searches
 * count, from zero, the executed f16 MFMAs behind the roofline -- (out[8]) the stream's bound
 * tests, (out[0]) the 32-bundle blocks whose stream test fired in a wave (each re-issues its
 * stream test), (out[1]) the per-query bound tests run on the groups they fired for, (out[2])
 * the pair tests (32 queries x 32 points each) -- and, summed over the wave tasks (out[7] of
 * them), the 100 MHz clock ticks each spent in its prologue (out[3]), bundle stream (out[4]),
 * deferred fired blocks (out[5]) and epilogue (out[6]), and (out[9]) the largest total of one
 * wave task over all the launches counted; within the deferred phase (v2, which waits for each
 * step's memory while counting) the per-query bound tests (out[10]), the waits for the pair
 * blocks (out[11]) and the pair tests (out[12]); 0 = off (the default; no counting). */
int icp_set_bundle_counters(icp_ctx *ctx, int enable);
int icp_get_bundle_counters(icp_ctx *ctx, uint64_t out[16]);
/* Who this context talks to (evidence for multi-GPU runs): *comm_count / *comm_rank =
 * ncclCommCount / ncclCommUserRank of its RCCL communicator, or -1 / the context's rank when
 * it has none (plain or host all-reduce contexts); bus_id (nullable, len >= 16) = the PCI bus
 * id of its HIP device (hipDeviceGetPCIBusId), NUL-terminated. */
int icp_get_comm_info(icp_ctx *ctx, int *comm_count, int *comm_rank, char *bus_id, int len);
/* The bundle filter's kd order of the resident model (models of >= 8,192 points; built on the
 * device by icp_set_model): kd_out[P] = the original index of kd position P (nm entries); 32
 * consecutive positions form a bundle.  ICP_E_NO_MODEL if the model has no bundle images. */
int icp_get_model_order(icp_ctx *ctx, int32_t *kd_out);
/* The engine's stable LSD radix sort (icp_sort.hip: the grid build's cell lists and the scene's
 * slot order), exposed for its tests: order_out[k] = the input position of the k-th pair when
 * the n keys are sorted by their low `bits` bits (ties in input order); keys_out (nullable) =
 * the keys in that order.  Host arrays; runs on `device` (synchronous).  ICP_E_ARG for bits
 * outside [0, 32] or n > INT_MAX. */
int icp_sort_pairs(int device, const uint32_t *keys, size_t n, int bits, uint32_t *keys_out, int32_t *order_out);
/* The engine's radix select (icp_select.hip: the cut of a trimmed icp_run; the same kernels),
 * exposed for its tests: *out = the k-th smallest (1-based) of the n host doubles v in the total
 * order -inf < ... < -0 < +0 < ... < +inf < NaN; every NaN is equal and last, and is returned as a
 * quiet NaN.  Runs on `device` (synchronous).  ICP_E_ARG for a null pointer, n == 0, n > INT_MAX,
 * k == 0 or k > n. */
int icp_select_kth(int device, const double *v, size_t n, size_t k, double *out);
/* The resident model's uniform grid (icp_grid.hip: launch_grid_build), exposed for its tests:
 * g = the cells per axis, lo = the grid's origin, *inv_h = 1 / cell size (a point's cell per axis is
 * clamp(floor((x - lo) * inv_h), 0, g - 1), its id (cz * g[1] + cy) * g[0] + cx); start (nullable,
 * g[0] g[1] g[2] + 1 entries) = each cell's first position in the sorted point list; order
 * (nullable, nm entries) = each sorted position's model index.  Call once with start = order =
 * NULL for the sizes.  ICP_E_NO_MODEL without a model. */
int icp_get_grid(icp_ctx *ctx, int g[3], double lo[3], double *inv_h, int32_t *start, int32_t *order);
/* The blocks of device and pinned host memory the library holds now, over every context of the process
 * (exposed for its tests: the count returns to what it was once the contexts made since are destroyed). */
long /* (the type's second word begins the line that names the function, as every declaration here does) */
long icp_debug_live_buffers(void);

#ifdef __cplusplus
}
#endif
#endif /* ICP_CAPI_H */
