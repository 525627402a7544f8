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
// With robust weights (icp_set_robust) the moments and the fold + step have weighted twins here
// (robust_gated_moments_kernel, robust_gated_horn_kernel, robust_first_shift_kernel): each kept
// pair's terms enter as w * t, w a function of the pair's d2, beside W = sum w and K+ = #{w > 0}.
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
// A frozen iteration (st->done) returns at once: neither its sums nor the mask are written.
template <bool YIN>
__global__ __launch_bounds__(kBlock) void gated_moments_kernel(
    const int *__restrict__ idx, const double4 *__restrict__ m4, const double *__restrict__ px,
    const double *__restrict__ py, const double *__restrict__ pz, int n, double *__restrict__ yx,
    double *__restrict__ yy, double *__restrict__ yz, const IterState *__restrict__ st, double D,
    unsigned long long *__restrict__ mask, double *__restrict__ partials, const int *__restrict__ kpos,
    const double4 *__restrict__ m4kd, const double *__restrict__ cut)
{
    if (st->done != 0) return;
    const double cp0 = st->shift_p[0], cp1 = st->shift_p[1], cp2 = st->shift_p[2];
    const double cy0 = st->shift_y[0], cy1 = st->shift_y[1], cy2 = st->shift_y[2];
    double a[17];
#pragma unroll
    for (int k = 0; k < 17; ++k) a[k] = 0.0;
    double kept = 0.0;
    kept_pairs_pass<YIN>(idx, m4, px, py, pz, n, yx, yy, yz, kept_cut(D, cut), mask, kpos, m4kd,
                         [&](long long, double q0, double q1, double q2, const double4 &m, double, double, double)
                             __attribute__((always_inline)) {
                                 shifted_moment_terms(q0, q1, q2, m, cp0, cp1, cp2, cy0, cy1, cy2, a);
                                 kept += 1.0;
                             });
    double b[kGateSums];
#pragma unroll
    for (int k = 0; k < 17; ++k) b[k] = a[k];
    b[kGateCount] = kept;
    block_sum_store<kGateSums>(b, partials + (size_t)blockIdx.x * kGateSums);
}

// gated_moments_kernel with robust weights (icp_set_robust): each kept pair's 17 terms (moment_leaves:
// shifted_moment_terms' arithmetic) enter as a += w * t with w = robust_weight<KIND>(d2), d2 the
// gate's own; the kept count stays the 18th sum, W = sum w and K+ = #{w > 0} are the 19th and 20th
// (doubles: K+ exact below 2^53).  A weight of exactly 1.0 adds the unweighted kernel's bits.
template <bool YIN, int KIND>
__global__ __launch_bounds__(kBlock) void robust_gated_moments_kernel(
    const int *__restrict__ idx, const double4 *__restrict__ m4, const double *__restrict__ px,
    const double *__restrict__ py, const double *__restrict__ pz, int n, double *__restrict__ yx,
    double *__restrict__ yy, double *__restrict__ yz, const IterState *__restrict__ st, double D,
    unsigned long long *__restrict__ mask, double *__restrict__ partials, const int *__restrict__ kpos,
    const double4 *__restrict__ m4kd, double k, double k2, const double *__restrict__ cut)
{
    if (st->done != 0) return;
    const double cp[3] = {st->shift_p[0], st->shift_p[1], st->shift_p[2]};
    const double cy[3] = {st->shift_y[0], st->shift_y[1], st->shift_y[2]};
    double a[kRobustGateSums];
#pragma unroll
    for (int j = 0; j < kRobustGateSums; ++j) a[j] = 0.0;
    kept_pairs_pass<YIN>(idx, m4, px, py, pz, n, yx, yy, yz, kept_cut(D, cut), mask, kpos, m4kd,
                         [&](long long, double q0, double q1, double q2, const double4 &m, double dx, double dy, double dz)
                             __attribute__((always_inline)) {
                                 const double w = robust_weight<KIND>((dx * dx + dy * dy) + dz * dz, k, k2);
                                 double t[17];
                                 moment_leaves(q0, q1, q2, m.x, m.y, m.z, cp, cy, t);
#pragma unroll
                                 for (int j = 0; j < 17; ++j) a[j] += w * t[j];
                                 a[kGateCount] += 1.0;
                                 a[kRobustGateW] += w;
                                 a[kRobustGateKpos] += w > 0.0 ? 1.0 : 0.0;
                             });
    block_sum_store<kRobustGateSums>(a, partials + (size_t)blockIdx.x * kRobustGateSums);
}

// The fold of the moments' partial rows into sums[0..WIDTH) (nblocks > 0) and / or the gated Horn
// step on sums (step; nblocks = 0: the sums as they are, all-reduced).  The step decides from the
// global count K = sums[kGateCount], identical on every rank: K < 4 freezes the run with the
// too-few status (kept_stop); else Horn's closed form over the kept pairs, N = K.
// WIDTH = kRobustGateSums, the weighted rows: K+ < 4 freezes the run as well, N = W, and a solved
// iteration's W and K+ join their mapped traces (the error step records that iteration's K and error).
// trim_few: the trim's T is below the least count (icp_set_trim), which stops the run like K.
template <int WIDTH>
__device__ __forceinline__ void gated_horn_body(const double *__restrict__ partials, int nblocks,
                                                double *__restrict__ sums, int step, double c0, double c1, double c2,
                                                int *__restrict__ cnt, IterState *__restrict__ s,
                                                GateState *__restrict__ g, GateState *__restrict__ h_g,
                                                IterState *__restrict__ h_state, double *__restrict__ h_wtrace,
                                                long long *__restrict__ h_ptrace, int trim_few)
{
    constexpr bool kRobust = WIDTH == kRobustGateSums;
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
        if constexpr (kRobust) {
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
    horn_step_body(res, kRobust ? res[kRobustGateW] : K, c0, c1, c2, 1, cnt, s); // (done: the search's counters only)
}

__global__ __launch_bounds__(kBlock) void gated_horn_kernel(const double *__restrict__ partials, int nblocks,
                                                            double *__restrict__ sums, int step, double c0, double c1,
                                                            double c2, int *__restrict__ cnt, IterState *__restrict__ s,
                                                            GateState *__restrict__ g, GateState *__restrict__ h_g,
                                                            IterState *__restrict__ h_state, int trim_few)
{
    gated_horn_body<kGateSums>(partials, nblocks, sums, step, c0, c1, c2, cnt, s, g, h_g, h_state, nullptr, nullptr,
                               trim_few);
}

__global__ __launch_bounds__(kBlock) void robust_gated_horn_kernel(
    const double *__restrict__ partials, int nblocks, double *__restrict__ sums, int step, double c0, double c1, double c2,
    int *__restrict__ cnt, IterState *__restrict__ s, GateState *__restrict__ g, GateState *__restrict__ h_g,
    IterState *__restrict__ h_state, double *__restrict__ h_wtrace, long long *__restrict__ h_ptrace, int trim_few)
{
    gated_horn_body<kRobustGateSums>(partials, nblocks, sums, step, c0, c1, c2, cnt, s, g, h_g, h_state, h_wtrace,
                                     h_ptrace, trim_few);
}

// The first gated iteration's shifts, from a pre-pass of the moments around the model's centre c
// (where run_init put both shifts): the kept pairs' centroids, c + sum (p - c) / K and
// c + sum (y - c) / K.  A partial-overlap scan D from c would otherwise cancel (D / sigma)^2 of the
// one-pass moments' precision; sums of differences from c give the centroids to D eps, far closer
// than a shift has to be.  sums: the folded (all ranks') pre-pass.  K = 0 leaves c (the step that
// follows stops the run on the same count).
__global__ void gated_first_shift_kernel(IterState *__restrict__ s, const double *__restrict__ sums)
{
    const double K = sums[kGateCount];
    if (threadIdx.x >= 3 || s->done || !(K >= 1.0)) return;
    s->shift_p[threadIdx.x] += sums[kSumP + threadIdx.x] / K;
    s->shift_y[threadIdx.x] += sums[kSumY + threadIdx.x] / K;
}

// gated_first_shift_kernel for the weighted pre-pass (rows of 20): the weighted centroids,
// c + sum w (p - c) / W and c + sum w (y - c) / W.  The weights do not depend on the shifts, so the
// pass that follows computes the same ones.  W not > 0 leaves c (K+ = 0: the step stops the run).
__global__ void robust_first_shift_kernel(IterState *__restrict__ s, const double *__restrict__ sums)
{
    const double W = sums[kRobustGateW];
    if (threadIdx.x >= 3 || s->done || !(W > 0.0)) return;
    s->shift_p[threadIdx.x] += sums[kSumP + threadIdx.x] / W;
    s->shift_y[threadIdx.x] += sums[kSumY + threadIdx.x] / W;
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

void launch_gated_moments(const int *idx, const double4 *m4, const double *px, const double *py, const double *pz,
                          int n, double *yx, double *yy, double *yz, const IterState *st_dev, double D,
                          unsigned long long *mask, double *partials, hipStream_t st, const int *kpos,
                          const double4 *m4kd, bool y_ready, const double *cut)
{
    if (y_ready)
        gated_moments_kernel<true><<<red_blocks(n), kBlock, 0, st>>>(idx, m4, px, py, pz, n, yx, yy, yz, st_dev, D, mask,
                                                                     partials, kpos, m4kd, cut);
    else
        gated_moments_kernel<false><<<red_blocks(n), kBlock, 0, st>>>(idx, m4, px, py, pz, n, yx, yy, yz, st_dev, D, mask,
                                                                      partials, kpos, m4kd, cut);
}

void launch_gated_horn(const double *partials, int nblocks, double *sums, bool step, const double c[3], int *amb_count,
                       IterState *st_dev, GateState *gate, GateState *h_gate, IterState *h_state, hipStream_t st,
                       bool trim_few)
{
    gated_horn_kernel<<<1, kBlock, 0, st>>>(partials, nblocks, sums, step ? 1 : 0, c[0], c[1], c[2], amb_count, st_dev,
                                            gate, h_gate, h_state, trim_few ? 1 : 0);
}

void launch_gated_first_shift(IterState *st_dev, const double *sums, hipStream_t st)
{
    gated_first_shift_kernel<<<1, 64, 0, st>>>(st_dev, sums);
}

template <int KIND>
static void robust_gated_moments_of(double k, double k2, const int *idx, const double4 *m4, const double *px,
                                    const double *py, const double *pz, int n, double *yx, double *yy, double *yz,
                                    const IterState *st_dev, double D, unsigned long long *mask, double *partials,
                                    hipStream_t st, const int *kpos, const double4 *m4kd, bool y_ready, const double *cut)
{
    if (y_ready)
        robust_gated_moments_kernel<true, KIND><<<red_blocks(n), kBlock, 0, st>>>(idx, m4, px, py, pz, n, yx, yy, yz, st_dev,
                                                                                  D, mask, partials, kpos, m4kd, k, k2, cut);
    else
        robust_gated_moments_kernel<false, KIND><<<red_blocks(n), kBlock, 0, st>>>(idx, m4, px, py, pz, n, yx, yy, yz, st_dev,
                                                                                   D, mask, partials, kpos, m4kd, k, k2, cut);
}

void launch_robust_gated_moments(int kind, double k, double k2, const int *idx, const double4 *m4, const double *px,
                                 const double *py, const double *pz, int n, double *yx, double *yy, double *yz,
                                 const IterState *st_dev, double D, unsigned long long *mask, double *partials,
                                 hipStream_t st, const int *kpos, const double4 *m4kd, bool y_ready, const double *cut)
{
    const auto go = kind == kRobustHuber   ? robust_gated_moments_of<kRobustHuber>
                    : kind == kRobustTukey ? robust_gated_moments_of<kRobustTukey>
                                           : robust_gated_moments_of<kRobustCauchy>;
    go(k, k2, idx, m4, px, py, pz, n, yx, yy, yz, st_dev, D, mask, partials, st, kpos, m4kd, y_ready, cut);
}

void launch_robust_gated_horn(const double *partials, int nblocks, double *sums, bool step, const double c[3],
                              int *amb_count, IterState *st_dev, GateState *gate, GateState *h_gate, IterState *h_state,
                              double *h_wtrace, long long *h_ptrace, hipStream_t st, bool trim_few)
{
    robust_gated_horn_kernel<<<1, kBlock, 0, st>>>(partials, nblocks, sums, step ? 1 : 0, c[0], c[1], c[2], amb_count,
                                                   st_dev, gate, h_gate, h_state, h_wtrace, h_ptrace, trim_few ? 1 : 0);
}

void launch_robust_first_shift(IterState *st_dev, const double *sums, hipStream_t st)
{
    robust_first_shift_kernel<<<1, 64, 0, st>>>(st_dev, sums);
}

void launch_gated_transform(double *px, double *py, double *pz, const double *yx, const double *yy, const double *yz,
                            int n, const Xform *xf, const int *done, float4 *p32, const unsigned long long *mask,
                            double *partials, hipStream_t st)
{
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
