// icp_eval.hip -- a registration evaluated on the device: icp_evaluate and icp_evaluate_device (DESIGN
// §3.22; include/icp_capi.h states the rules).  The resident scene as it lies now against the resident
// model: each scene point's closest model point (the squared-distance first minimum), the pairs within
// max_dist kept, their count, fitness, RMSE and largest d2, Open3D's 6 x 6 information matrix, and with
// `both` the same with the roles exchanged.  Every device array of a call is a part of the context's
// eval_block (a kept Scratch, icp_engine.h); the call reads the resident clouds and the model's grid and
// writes nothing a run or a report depends on.
//
//   eval_rows_kernel    the forward queries of a call without `both`: the scene's rows (x, y, z, caller's
//                       index) in its resident order (for a large scene the slot order: cell-coherent)
//   eval_aos_kernel     with `both`: the scene interleaved in the caller's order, from which cloud_grid
//                       (icp_cloud.hip) builds its temporary grid -- the reverse direction's target, and
//                       its cell-sorted points (w = the caller's index) the forward queries
//   eval_nn_kernel      ONE cross-cloud 1-NN kernel, both directions: a lane a query, the best (d2, index)
//                       under knn_less in registers (icp_knn.h's nn1_* helpers).  Finite D and the box of
//                       complete_box_r(q, max_dist) within the cell budget: that box alone is scanned --
//                       everything within D lies in it, so one scan decides whether the point is kept and
//                       which point is its pair.  Else nn1_search: the ring, the completeness box of the
//                       distance found, the scan of every point.  A query outside the target's box gets
//                       clamped cells; both modes stop by the completeness box alone.  The result goes to
//                       the caller's index: (i, d2) when d2 <= D, else (-1, +inf).
//   eval_terms_kernel   one pass in the caller's order: the d2 term, and forward the nine terms of the
//                       information matrix from y = m[i] (each product rounded; +0 for a pair not kept),
//                       column c at terms + c * n; K by an integer atomic, the largest kept d2 by an
//                       integer atomicMax on its bit pattern (a non-negative double orders as its bits),
//                       one pair of atomics a workgroup of 4,096 points
//   filter_sum_kernel   (icp_sum.h) the filters' sum rule S over the ten columns, a launch a level
//   eval_pack_kernel    one thread: the sums into the call's record beside the counts
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "icp_engine.h"
#include "icp_knn.h"
#include "icp_sum.h"

namespace icp {
namespace {

using namespace icp::engine;

constexpr int kEvalCols = 10; // t = d2, x, y, z, xx, yy, zz, xy, xz, yz
constexpr int kEvalTile = 4096; // points a workgroup of eval_terms_kernel (16 a thread)

// what a call reads back: the forward sums, the reverse d2 sum, (K, max bits, K_m, max_m bits)
struct EvalRecord {
    double s[kEvalCols + 1];
    unsigned long long k[4];
};

__global__ __launch_bounds__(kBlock) void eval_rows_kernel(const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ z, const int *__restrict__ order,
                                                           int n, double4 *__restrict__ rows)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    rows[s] = make_double4(x[s], y[s], z[s], (double)(order ? order[s] : s));
}

__global__ __launch_bounds__(kBlock) void eval_aos_kernel(const double *__restrict__ x, const double *__restrict__ y,
                                                          const double *__restrict__ z, const int *__restrict__ order,
                                                          int n, double *__restrict__ aos)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const size_t j = (size_t)(order ? order[s] : s);
    aos[3 * j] = x[s];
    aos[3 * j + 1] = y[s];
    aos[3 * j + 2] = z[s];
}

// queries q4s[0 .. nq) (w: where the result goes) against the grid gv over nt points (w: the index reported)
__global__ __launch_bounds__(kBlock) void eval_nn_kernel(GridView gv, int nt, const double4 *__restrict__ q4s, int nq,
                                                         double R, double D, int bounded, int budget,
                                                         int *__restrict__ idx, double *__restrict__ d2)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nq) return;
    const double4 q4 = q4s[t];
    const double q[3] = {q4.x, q4.y, q4.z};
    double bd = INFINITY;
    int bi = INT_MAX;
    int c0[3], c1[3];
    if (bounded && complete_box_r(q, R, gv, budget, c0, c1)) nn1_scan_box<false>(gv, c0, c1, c0, c1, q4.x, q4.y, q4.z, bd, bi);
    else nn1_search(gv, nt, budget, q4.x, q4.y, q4.z, bd, bi);
    const bool kept = bi != INT_MAX && bd <= D;
    const int j = (int)q4.w;
    idx[j] = kept ? bi : -1;
    d2[j] = kept ? bd : INFINITY;
}

// kInfo: the forward direction's ten columns; else the d2 column alone.  acc: (K, the largest kept d2's bits).
// A workgroup takes kEvalTile points, a thread every kBlock-th of them, and ends in ONE pair of atomics:
// a pair a wave of 64 points serialised on the two words (0.39 ms at 2^20 points, as long as the ten columns'
// writes: profiles/eval/)
template <bool kInfo>
__global__ __launch_bounds__(kBlock) void eval_terms_kernel(const int *__restrict__ idx, const double *__restrict__ d2,
                                                            const double4 *__restrict__ m4, int n,
                                                            double *__restrict__ terms, unsigned long long *__restrict__ acc)
{
    __shared__ int sh_cnt[kBlock / 64];
    __shared__ double sh_max[kBlock / 64];
    const long long base = (long long)blockIdx.x * kEvalTile + threadIdx.x;
    const size_t s = (size_t)n;
    int cnt = 0;
    double mx = 0.0; // (a kept d2 is >= +0 and never a NaN: it passed d2 <= D)
#pragma unroll 4
    for (int u = 0; u < kEvalTile / kBlock; ++u) {
        const long long j = base + (long long)u * kBlock;
        if (j >= n) break;
        const int i = idx[j];
        const bool kept = i >= 0;
        const double t = kept ? d2[j] : 0.0;
        terms[j] = t;
        cnt += kept ? 1 : 0;
        mx = t > mx ? t : mx;
        if (kInfo) {
            double4 y = make_double4(0.0, 0.0, 0.0, 0.0);
            if (kept) y = m4[i];
            terms[s + j] = y.x;
            terms[2 * s + j] = y.y;
            terms[3 * s + j] = y.z;
            terms[4 * s + j] = y.x * y.x;
            terms[5 * s + j] = y.y * y.y;
            terms[6 * s + j] = y.z * y.z;
            terms[7 * s + j] = y.x * y.y;
            terms[8 * s + j] = y.x * y.z;
            terms[9 * s + j] = y.y * y.z;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        const double other = __shfl_xor(mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        sh_cnt[threadIdx.x >> 6] = cnt;
        sh_max[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) {
            cnt += sh_cnt[w];
            mx = sh_max[w] > mx ? sh_max[w] : mx;
        }
        if (cnt) {
            atomicAdd(&acc[0], (unsigned long long)cnt);
            atomicMax(&acc[1], (unsigned long long)__double_as_longlong(mx));
        }
    }
}

__global__ void eval_pack_kernel(const double *__restrict__ sums, size_t stride, int cols, int at, EvalRecord *__restrict__ rec)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int c = 0; c < cols; ++c) rec->s[at + c] = sums[(size_t)c * stride];
}

// ICP_EVAL_DEBUG: a call's phases timed by events on the context's stream, one line to stderr
// (tools/eval_probe.py): the queries and the scene's grid, the forward search, the reverse search, the
// terms and sums
struct EvalClock {
    bool on;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int marks = 0;
    EvalClock()
    {
        static const bool debug = getenv("ICP_EVAL_DEBUG") != nullptr;
        on = debug;
        if (on)
            for (hipEvent_t &e : ev)
                if (hipEventCreate(&e) != hipSuccess) on = false;
    }
    ~EvalClock()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(hipStream_t st)
    {
        if (on && marks < 5) (void)hipEventRecord(ev[marks++], st);
    }
    void report(size_t np, size_t nm, double max_dist, int both, long long K) // (after the stream's last synchronise)
    {
        float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!on || marks != 5) return;
        for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        std::fprintf(stderr,
                     "[evaluate] np=%zu nm=%zu max_dist=%g both=%d K=%lld queries/grid %.3f ms, forward search %.3f ms, "
                     "reverse search %.3f ms, terms/sums %.3f ms\n",
                     np, nm, max_dist, both, K, ms[0], ms[1], ms[2], ms[3]);
    }
};

double bits_double(unsigned long long b)
{
    double d;
    std::memcpy(&d, &b, sizeof(d));
    return d;
}

// rule 4: A from the nine sums and K
void information_from_sums(const double *s, long long K, double A[36])
{
    const double Sx = s[1], Sy = s[2], Sz = s[3], Sxx = s[4], Syy = s[5], Szz = s[6], Sxy = s[7], Sxz = s[8], Syz = s[9];
    for (int k = 0; k < 36; ++k) A[k] = 0.0;
    auto set = [&](int r, int c, double v) { A[6 * r + c] = A[6 * c + r] = v; };
    set(0, 0, Syy + Szz);
    set(1, 1, Sxx + Szz);
    set(2, 2, Sxx + Syy);
    set(0, 1, -Sxy);
    set(0, 2, -Sxz);
    set(1, 2, -Syz);
    set(0, 4, -Sz);
    set(0, 5, Sy);
    set(1, 3, Sz);
    set(1, 5, -Sx);
    set(2, 3, -Sy);
    set(2, 4, Sx);
    for (int d = 3; d < 6; ++d) set(d, d, (double)K);
}

// both forms: the checks, the kernels, the read-back; then alone the outputs, the per-point arrays to
// host (host) or device memory
int evaluate(icp_ctx *ctx, double max_dist, int both, icp_evaluation *out, int32_t *idx_out, double *d2_out,
             int32_t *model_idx_out, double *model_d2_out, bool host)
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_evaluate";
    if (!out) return fail(ctx, ICP_E_ARG, who + ": out is null");
    if (!(max_dist > 0.0)) // (a NaN fails it)
        return fail(ctx, ICP_E_ARG, who + ": max_dist = " + std::to_string(max_dist) + " is not > 0");
    if (!both && (model_idx_out || model_d2_out))
        return fail(ctx, ICP_E_ARG, who + ": both = 0 with a model_idx_out or model_d2_out array");
    if (ctx->world > 1)
        return fail(ctx, ICP_E_ARG, who + ": a context of " + std::to_string(ctx->world) +
                                        " ranks (the reverse minimum over shards is not built)");
    if (!ctx->has_model || !ctx->g_start || !ctx->g_pts || !ctx->m4)
        return fail(ctx, ICP_E_NO_MODEL, who + ": no model (icp_set_model)");
    if (!ctx->has_scene || ctx->scene.n == 0) return fail(ctx, ICP_E_NO_MODEL, who + ": no scene (icp_set_scene)");
    HIPCHK(hipSetDevice(ctx->device));

    const size_t np = ctx->scene.n, nm = ctx->nm;
    const double D = max_dist * max_dist; // (once, here)
    const int bounded = std::isfinite(D) ? 1 : 0;
    const double R = bounded ? std::max(max_dist, std::sqrt(D)) : 0.0;
    const DevCloud &P = ctx->scene;
    const int *order = ctx->scene_slot ? ctx->s_order : nullptr; // (slot s holds the caller's point order[s])

    Scratch tmp(ctx, &ctx->eval_block); // (kept for the next evaluation)
    int *idx = nullptr, *midx = nullptr;
    double *d2 = nullptr, *md2 = nullptr, *terms = nullptr, *part = nullptr;
    EvalRecord *rec = nullptr;
    TRY(tmp.get(&idx, np));
    TRY(tmp.get(&d2, np));
    TRY(tmp.get(&terms, (size_t)kEvalCols * np));
    TRY(tmp.get(&part, sum_part_doubles(np, kEvalCols)));
    TRY(tmp.get(&rec, 1));
    EvalClock clock;
    clock.mark(ctx->st);
    HIPCHK(hipMemsetAsync(rec, 0, sizeof(EvalRecord), ctx->st));

    const GridView mg = grid_view(ctx);
    const double4 *queries = nullptr;
    TempGrid tg;
    if (both) {
        double *aos = nullptr;
        TRY(tmp.get(&aos, 3 * np));
        eval_aos_kernel<<<blocks_for(np, kBlock), kBlock, 0, ctx->st>>>(P.x, P.y, P.z, order, (int)np, aos);
        LAUNCHCHK("eval_aos");
        TRY(cloud_grid(ctx, who, aos, np, tmp, tg));
        queries = tg.gv.pts;
    } else {
        double4 *rows = nullptr;
        TRY(tmp.get(&rows, np));
        eval_rows_kernel<<<blocks_for(np, kBlock), kBlock, 0, ctx->st>>>(P.x, P.y, P.z, order, (int)np, rows);
        LAUNCHCHK("eval_rows");
        queries = rows;
    }
    clock.mark(ctx->st);
    eval_nn_kernel<<<blocks_for(np, kBlock), kBlock, 0, ctx->st>>>(mg, (int)nm, queries, (int)np, R, D, bounded,
                                                                    grid_budget(ctx), idx, d2);
    LAUNCHCHK("eval_nn_forward");
    clock.mark(ctx->st);
    if (both) {
        TRY(tmp.get(&midx, nm));
        TRY(tmp.get(&md2, nm));
        eval_nn_kernel<<<blocks_for(nm, kBlock), kBlock, 0, ctx->st>>>(tg.gv, (int)np, mg.pts, (int)nm, R, D, bounded,
                                                                        tg.budget, midx, md2);
        LAUNCHCHK("eval_nn_reverse");
    }
    clock.mark(ctx->st);
    eval_terms_kernel<true><<<blocks_for(np, kEvalTile), kBlock, 0, ctx->st>>>(idx, d2, ctx->m4, (int)np, terms, rec->k);
    const double *s = sum_levels<false>(terms, (int)np, nullptr, part, ctx->st, kEvalCols, np);
    eval_pack_kernel<<<1, 1, 0, ctx->st>>>(s, sum_part_stride(np), kEvalCols, 0, rec);
    LAUNCHCHK("eval_sums");
    if (both) {
        double *mterms = nullptr, *mpart = nullptr;
        TRY(tmp.get(&mterms, nm));
        TRY(tmp.get(&mpart, sum_part_doubles(nm)));
        eval_terms_kernel<false><<<blocks_for(nm, kEvalTile), kBlock, 0, ctx->st>>>(midx, md2, nullptr, (int)nm, mterms,
                                                                                 rec->k + 2);
        const double *sm = sum_levels<false>(mterms, (int)nm, nullptr, mpart, ctx->st);
        eval_pack_kernel<<<1, 1, 0, ctx->st>>>(sm, 0, 1, kEvalCols, rec);
        LAUNCHCHK("eval_model_sums");
    }
    EvalRecord h;
    HIPCHK(hipMemcpyAsync(&h, rec, sizeof(h), hipMemcpyDeviceToHost, ctx->st));
    clock.mark(ctx->st);
    HIPCHK(hipStreamSynchronize(ctx->st));

    // everything has run: the outputs
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (idx_out) HIPCHK(hipMemcpyAsync(idx_out, idx, sizeof(int32_t) * np, kind, ctx->st));
    if (d2_out) HIPCHK(hipMemcpyAsync(d2_out, d2, sizeof(double) * np, kind, ctx->st));
    if (model_idx_out) HIPCHK(hipMemcpyAsync(model_idx_out, midx, sizeof(int32_t) * nm, kind, ctx->st));
    if (model_d2_out) HIPCHK(hipMemcpyAsync(model_d2_out, md2, sizeof(double) * nm, kind, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    icp_evaluation e{};
    const long long K = (long long)h.k[0];
    e.scene_points = (long long)np;
    e.correspondences = K;
    e.fitness = (double)K / (double)np;
    e.inlier_rmse = K ? std::sqrt(h.s[0] / (double)K) : 0.0;
    e.max_inlier_d2 = K ? bits_double(h.k[1]) : 0.0;
    information_from_sums(h.s, K, e.information);
    if (both) {
        const long long Km = (long long)h.k[2];
        e.model_points = (long long)nm;
        e.model_correspondences = Km;
        e.model_fitness = (double)Km / (double)nm;
        e.model_rmse = Km ? std::sqrt(h.s[kEvalCols] / (double)Km) : 0.0;
        e.model_max_inlier_d2 = Km ? bits_double(h.k[3]) : 0.0;
    }
    clock.report(np, nm, max_dist, both ? 1 : 0, K);
    *out = e;
    return ICP_OK;
}

} // namespace
} // namespace icp

using namespace icp;

extern "C" {

int icp_evaluate(icp_ctx *ctx, double max_dist, int both, icp_evaluation *out, int32_t *idx_out, double *d2_out,
                 int32_t *model_idx_out, double *model_d2_out)
{
    return evaluate(ctx, max_dist, both, out, idx_out, d2_out, model_idx_out, model_d2_out, true);
}

int icp_evaluate_device(icp_ctx *ctx, double max_dist, int both, icp_evaluation *out, int32_t *idx_out_dev,
                        double *d2_out_dev, int32_t *model_idx_out_dev, double *model_d2_out_dev)
{
    return evaluate(ctx, max_dist, both, out, idx_out_dev, d2_out_dev, model_idx_out_dev, model_d2_out_dev, false);
}

} // extern "C"
