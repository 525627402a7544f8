// icp_gated.hip — the kernels of icp_run's gated iteration (icp_set_max_distance): the moments,
// the transform + residual and their folds and steps over the pairs no farther apart than dmax.
//
// One gated iteration on the scene p (n points on this rank), after the search has left idx:
//   y_j = m[idx_j];  d2_j = (dx*dx + dy*dy) + dz*dz in fp64 as written (the searches' own
//   arithmetic);  keep_j = d2_j <= D (false for a NaN);  K = #kept over all ranks;
//   K < 4: the run stops before the iteration changes anything;  else Horn's closed form over the
//   kept pairs with N = K, every point moved by it (the outliers travel with the cloud), and
//   err = (e + e) / K with e the kept pairs' residual.
// The gate of an iteration is kept bit-packed, one 64-bit word per wave of points (__ballot), for
// the transform's residual and for icp_get_inliers.
// The loop over the pairs with the gate and its mask, the transform's body, the fold and the freeze
// of a stopped run are icp_kept.h's, shared with the point-to-plane kernels (icp_plane.hip); the
// residual's fold and error step here (launch_gated_err) and the mask's unpacking serve both.
// Robust weights (icp_set_robust) are a template parameter of the moments and of the fold + step:
// each kept pair's terms enter as w * t, w a function of the pair's d2, beside W = sum w and
// K+ = #{w > 0}.  The launchers of both metrics' loops are here (launch_kept_*).
// Compiled with IEEE semantics like icp_step.hip (the error step's `err < threshold` and the
// gate's `d2 <= D` must stay false for a NaN).
#include <hip/hip_runtime.h>

#include "icp_canon.h"
#include "icp_device.h"
#include "icp_fold.h"
#include "icp_kept.h"
#include "icp_kernels.h"

namespace icp {
namespace {

// Modelled on shifted_moments_kernel: the 17 one-pass moment terms around the shifts of *st, of
// the kept pairs only (kept_pairs_pass: the gate and its mask), and the kept count as an 18th sum
// (a double: exact below 2^53).
// KIND, a robust weight (icp_set_robust; kk = k, k2): each kept pair's 17 terms (moment_leaves:
// shifted_moment_terms' arithmetic) enter as a += w * t with w = robust_weight<KIND>(d2), d2 the
// gate's own, and W = sum w and K+ = #{w > 0} are the 19th and 20th sums (doubles: K+ exact below
// 2^53).  A weight of exactly 1.0 adds the unweighted kind's bits.
// A frozen iteration (st->done) returns at once: neither its sums nor the mask are written.
template <bool YIN, int KIND, class CUT, class... K>
__global__ __launch_bounds__(kBlock) void gated_moments_kernel(
    const int *__restrict__ idx, const double4 *__restrict__ m4, const double *__restrict__ px,
    const double *__restrict__ py, const double *__restrict__ pz, int n, double *__restrict__ yx,
    double *__restrict__ yy, double *__restrict__ yz, const IterState *__restrict__ st, double D,
    unsigned long long *__restrict__ mask, double *__restrict__ partials, const int *__restrict__ kpos,
    const double4 *__restrict__ m4kd, K... kk, CUT cut)
{
    constexpr bool kRobust = KIND != kRobustNone;
    constexpr int WIDTH = kept_width(false, kRobust);
    if (st->done != 0) return;
    const double cp[3] = {st->shift_p[0], st->shift_p[1], st->shift_p[2]};
    const double cy[3] = {st->shift_y[0], st->shift_y[1], st->shift_y[2]};
    // (unweighted: shifted_moment_terms' 17 sums and the count beside them, joined for the store --
    // summed as one row of 18 the same pass compiles to another instruction stream)
    double a[kRobust ? WIDTH : 17];
#pragma unroll
    for (double &v : a) v = 0.0;
    double kept = 0.0;
    kept_pairs_pass<YIN, kKeptUnique<CUT>>(idx, m4, px, py, pz, n, yx, yy, yz, kept_cut(D, cut_of(cut)), mask, kpos, m4kd, best_of(cut),
                         [&](long long, double q0, double q1, double q2, const double4 &m, double dx, double dy, double dz)
                             __attribute__((always_inline)) {
                                 if constexpr (kRobust) {
                                     const double w = robust_weight<KIND>((dx * dx + dy * dy) + dz * dz, kk...);
                                     double t[17];
                                     moment_leaves(q0, q1, q2, m.x, m.y, m.z, cp, cy, t);
#pragma unroll
                                     for (int j = 0; j < 17; ++j) a[j] += w * t[j];
                                     a[kGateCount] += 1.0;
                                     a[kRobustGateW] += w;
                                     a[kRobustGateKpos] += w > 0.0 ? 1.0 : 0.0;
                                 } else {
                                     shifted_moment_terms(q0, q1, q2, m, cp[0], cp[1], cp[2], cy[0], cy[1], cy[2], a);
                                     kept += 1.0;
                                 }
                             });
    if constexpr (kRobust) {
        block_sum_store<WIDTH>(a, partials + (size_t)blockIdx.x * WIDTH);
    } else {
        double b[WIDTH];
#pragma unroll
        for (int j = 0; j < 17; ++j) b[j] = a[j];
        b[kGateCount] = kept;
        block_sum_store<WIDTH>(b, partials + (size_t)blockIdx.x * WIDTH);
    }
}

// The fold of the moments' partial rows into sums[0..width) (nblocks > 0) and / or the gated Horn
// step on sums (step; nblocks = 0: the sums as they are, all-reduced).  The step decides from the
// global count K = sums[kGateCount], identical on every rank: K < 4 freezes the run with the
// too-few status (kept_stop); else Horn's closed form over the kept pairs, N = K.
// ROBUST, the weighted rows: K+ < 4 freezes the run as well, N = W, and a solved iteration's W and
// K+ join their mapped traces (the error step records that iteration's K and error).
// trim_few: the trim's T is below the least count (icp_set_trim), which stops the run like K.
template <bool ROBUST>
__device__ __forceinline__ void gated_horn_body(
    const double *__restrict__ partials, int nblocks, double *__restrict__ sums, int step, double c0, double c1, double c2,
    int *__restrict__ cnt, IterState *__restrict__ s, GateState *__restrict__ g, GateState *__restrict__ h_g,
    IterState *__restrict__ h_state, double *__restrict__ h_wtrace, long long *__restrict__ h_ptrace, int trim_few)
{
    constexpr int WIDTH = kept_width(false, ROBUST);
    __shared__ double res[WIDTH];
    if (nblocks > 0) {
        fold_to<WIDTH>(partials, nblocks, sums, res);
    } else {
        if (threadIdx.x < WIDTH) res[threadIdx.x] = sums[threadIdx.x];
        __syncthreads();
    }
    if (!step || threadIdx.x != 0) return;
    const double K = res[kGateCount];
    if (!s->done) { // (a frozen iteration's sums are stale: its gate was not evaluated)
        g->K = (long long)K;
        h_g->K = (long long)K;
        bool few = !(K >= 4.0) || trim_few != 0;
        if constexpr (ROBUST) {
            const double W = res[kRobustGateW], Kpos = res[kRobustGateKpos];
            g->W = W;
            g->Kpos = (long long)Kpos;
            h_g->W = W;
            h_g->Kpos = (long long)Kpos;
            few = few || !(Kpos >= 4.0);
            if (!few) {
                h_wtrace[s->iter] = W;
                h_ptrace[s->iter] = (long long)Kpos;
            }
        }
        if (few) kept_stop(s, g, h_g, h_state, kGateTooFew, 0.0);
    }
    horn_step_body(res, ROBUST ? res[kRobustGateW] : K, c0, c1, c2, 1, cnt, s); // (done: the search's counters only)
}

// (The step is an inlined function under the kernel, not the kernel's own body: written straight
// into the kernel the same text compiles to another instruction stream.)
template <bool ROBUST>
__global__ __launch_bounds__(kBlock) void gated_horn_kernel(
    const double *__restrict__ partials, int nblocks, double *__restrict__ sums, int step, double c0, double c1, double c2,
    int *__restrict__ cnt, IterState *__restrict__ s, GateState *__restrict__ g, GateState *__restrict__ h_g,
    IterState *__restrict__ h_state, double *__restrict__ h_wtrace, long long *__restrict__ h_ptrace, int trim_few)
{
    gated_horn_body<ROBUST>(partials, nblocks, sums, step, c0, c1, c2, cnt, s, g, h_g, h_state, h_wtrace, h_ptrace, trim_few);
}

// The first gated iteration's shifts, from a pre-pass of the moments around the model's centre c
// (where run_init put both shifts): the kept pairs' centroids, c + sum (p - c) / K and
// c + sum (y - c) / K, K = sums[slot = kGateCount]; or from the weighted pre-pass their weighted
// centroids, c + sum w (p - c) / W and c + sum w (y - c) / W, W = sums[slot = kRobustGateW] (the
// weights do not depend on the shifts, so the pass that follows computes the same ones).  A
// partial-overlap scan D from c would otherwise cancel (D / sigma)^2 of the one-pass moments'
// precision; sums of differences from c give the centroids to D eps, far closer than a shift has
// to be.  sums: the folded (all ranks') pre-pass.  A divisor not > 0 leaves c (the step that follows
// stops the run on K or K+); K is an integer-valued double, so K > 0 is K >= 1.
__global__ void kept_first_shift_kernel(IterState *__restrict__ s, const double *__restrict__ sums, int slot)
{
    const double v = sums[slot];
    if (threadIdx.x >= 3 || s->done || !(v > 0.0)) return;
    s->shift_p[threadIdx.x] += sums[kSumP + threadIdx.x] / v;
    s->shift_y[threadIdx.x] += sums[kSumY + threadIdx.x] / v;
}

// Modelled on the plain branch of transform_err_kernel: every point moves, the residual is
// summed over the kept points (kept_transform).
__global__ __launch_bounds__(kBlock) void gated_transform_kernel(
    double *__restrict__ px, double *__restrict__ py, double *__restrict__ pz, const double *__restrict__ yx,
    const double *__restrict__ yy, const double *__restrict__ yz, int n, const Xform *__restrict__ xfd,
    const int *__restrict__ done, float4 *__restrict__ p32, const unsigned long long *__restrict__ mask,
    double *__restrict__ partials)
{
    kept_transform(px, py, pz, n, xfd, done, p32, mask, partials,
                   [&](long long i, double q0, double q1, double q2) __attribute__((always_inline)) {
                       return residual2(yx[i], yy[i], yz[i], q0, q1, q2);
                   });
}

// The fold of the residual's partial rows into sums[kSumErr] (nblocks > 0) and / or the error
// step with N = K (step): the iteration's K joins the mapped K trace as its error is recorded.
__global__ __launch_bounds__(kBlock) void gated_err_kernel(const double *__restrict__ partials, int nblocks,
                                                           double *__restrict__ sums, int step, double threshold,
                                                           int max_iter, double *__restrict__ err_trace,
                                                           IterState *__restrict__ s, const GateState *__restrict__ g,
                                                           long long *__restrict__ h_ktrace, int *hflag, int ticket,
                                                           IterState *h_state, double *h_trace)
{
    __shared__ double res[1];
    if (nblocks > 0) fold_to<1>(partials, nblocks, sums + kSumErr, res);
    if (!step || threadIdx.x != 0) return;
    const long long K = g->K;
    if (!s->done) h_ktrace[s->iter] = K;
    err_step_body(sums, (double)K, threshold, max_iter, err_trace, s, hflag, ticket, h_state, h_trace);
}

// out[caller's index of point i] = bit i of the mask (order: point i is the caller's order[i])
__global__ __launch_bounds__(kBlock) void gated_unpack_kernel(const unsigned long long *__restrict__ mask,
                                                              const int *__restrict__ order, int n,
                                                              unsigned char *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[order ? order[i] : i] = (unsigned char)((mask[i >> 6] >> (i & 63)) & 1ull);
}

} // namespace

void launch_kept_moments(const KeptPass &a, bool y_ready)
{
    if (a.plane) return plane_moments(a, y_ready);
    kept_dispatch(y_ready, a.robust_kind, [&](auto yin, auto kind) {
        const auto go = [&](auto... kk) {
            kept_tail(yin, a, [&](auto cut) {
                gated_moments_kernel<yin(), kind(), decltype(cut), decltype(kk)...><<<red_blocks(a.n), kBlock, 0, a.st>>>(
                    a.idx, a.m4, a.px, a.py, a.pz, a.n, a.yx, a.yy, a.yz, a.st_dev, a.D, a.mask, a.partials, a.kpos, a.m4kd,
                    kk..., cut);
            });
        };
        if constexpr (kind() == kRobustNone) go();
        else go(a.k, a.k2);
    });
}

void launch_kept_step(const KeptStep &a, const double *partials, int nblocks, bool step)
{
    if (a.plane) return plane_step(a, partials, nblocks, step);
    const auto kernel = a.robust ? gated_horn_kernel<true> : gated_horn_kernel<false>;
    kernel<<<1, kBlock, 0, a.st>>>(partials, nblocks, a.sums, step ? 1 : 0, a.c[0], a.c[1], a.c[2], a.amb_count, a.st_dev,
                                   a.gate, a.h_gate, a.h_state, a.h_wtrace, a.h_ptrace, a.trim_few ? 1 : 0);
}

void launch_kept_first_shift(IterState *st_dev, const double *sums, int slot, hipStream_t st)
{
    kept_first_shift_kernel<<<1, 64, 0, st>>>(st_dev, sums, slot);
}

void launch_kept_transform(double *px, double *py, double *pz, const double *yx, const double *yy, const double *yz,
                           int n, const Xform *xf, const int *done, float4 *p32, const unsigned long long *mask,
                           const int *idx, const double4 *n4, double *partials, hipStream_t st, const SymmArgs *symm)
{
    if (n4) return plane_transform(px, py, pz, yx, yy, yz, n, xf, done, p32, mask, idx, n4, partials, st, symm);
    gated_transform_kernel<<<red_blocks(n), kBlock, 0, st>>>(px, py, pz, yx, yy, yz, n, xf, done, p32, mask, partials);
}

void launch_gated_err(const double *partials, int nblocks, double *sums, bool step, double threshold, int max_iter,
                      double *err_trace, IterState *st_dev, const GateState *gate, long long *h_ktrace, int *hflag_dev,
                      int ticket, IterState *h_state_dev, double *h_trace_dev, hipStream_t st)
{
    gated_err_kernel<<<1, kBlock, 0, st>>>(partials, nblocks, sums, step ? 1 : 0, threshold, max_iter, err_trace, st_dev,
                                           gate, h_ktrace, hflag_dev, ticket, h_state_dev, h_trace_dev);
}

void launch_gated_unpack(const unsigned long long *mask, const int *order, int n, unsigned char *out, hipStream_t st)
{
    if (n <= 0) return;
    gated_unpack_kernel<<<(n + kBlock - 1) / kBlock, kBlock, 0, st>>>(mask, order, n, out);
}

} // namespace icp
