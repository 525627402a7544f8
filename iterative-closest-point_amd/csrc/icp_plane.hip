// icp_plane.hip — the kernels of icp_run's point-to-plane iteration (icp_set_metric with
// ICP_METRIC_POINT_TO_PLANE): the moments of the 6 x 6 normal equations, their fold and solve, the
// transform with the residual along the normal.
//
// One iteration on the scene p (n points on this rank), after the search has left idx; N = the
// model's normals as given, c = the model's centre, D = dmax * dmax (+inf: no gate):
//   y_j = m[idx_j], n_j = N[idx_j];  d_j = p_j - y_j;  d2_j = (dx*dx + dy*dy) + dz*dz as written;
//   keep_j = d2_j <= D (false for a NaN);  K = #kept over all ranks;
//   K < 6: the run stops before the iteration changes anything;  else over the kept pairs
//   a_j = [(p_j - c) x n_j ; n_j], r_j = d_j . n_j,  A = sum a_j a_j^T (21 entries, upper triangle
//   by rows), b = -sum a_j r_j (summed as sum a_j r_j and negated by the solve: exact);
//   g_k = sqrt(A_kk), A^ = A / (g g^T), b^ = b / g, Cholesky, x = solve(A^, b^) / g; an A_kk not > 0
//   or a pivot not > 1e-12 stops the run like too-few (degenerate);
//   omega = x[0..2], tau = x[3..5]: R = exp([omega]x), s = 1, t = (c + tau) - R c; every point
//   moves by q = R p + t, and err = (e + e) / K with e = sum over the kept pairs of ((q - y) . n)^2.
// The loop over the pairs with the gate and its mask (one 64-bit word per wave of points), the
// transform's body, the fold and the freeze of a stopped run are icp_kept.h's, shared with
// icp_gated.hip; the residual's fold and error step are that file's launch_gated_err, and its
// launch_kept_* reach the kernels here through plane_moments, plane_step and plane_transform.
// Robust weights (icp_set_robust) are a template parameter of the moments and of the fold + solve:
// A = sum w a a^T, b = -sum w a r with w a function of r * r, beside W = sum w and K+ = #{w > 0}.
// The symmetric form (icp_set_plane_symmetric; Rusinkiewicz 2019) is the same iteration with a second
// normal, the scene's: u0 as given, in the scene's current order, u_j = Q u0_j with Q the rotation of
// the total since icp_set_scene* (the run's IterState::tot composed onto the context's, SymmArgs):
//   h = N_j . u_j;  n_j = 0 if N_j or u0_j is all zero, else h < 0 ? N_j - u_j : N_j + u_j;
//   a_j = [((p_j - c) + (y_j - c)) x n_j ; n_j], r_j = d_j . n_j, the same 21 + 6 + 1 sums (a pair with
//   n_j = 0 counts in K and adds nothing else) and the same solve; with a~ = x[0..2], t~ = x[3..5]:
//   g = 1 / sqrt(1 + |a~|^2), k2 = g g / (1 + g), R_h = I + g [a~]x + k2 [a~]x^2 (the half rotation: g is
//   the half angle's cosine), R = R_h R_h, t = ((R_h (g t~)) + c) - R c, s = 1;
//   err = (e + e) / K with e = sum over the kept pairs of ((q - y) . n')^2, n' from u' = Q' u0, Q' the
//   total's rotation with this step composed.
// It is a template parameter of the three kernels (the moments and the transform take SymmArgs behind
// their one-sided arguments): under `if constexpr`, so the one-sided instantiations carry none of it.
// Compiled with IEEE semantics like icp_gated.hip (`d2 <= D`, `A_kk > 0` and `pivot > 1e-12` must
// stay false for a NaN).
#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_fold.h"
#include "icp_kept.h"
#include "icp_kernels.h"

namespace icp {
namespace {

// n4[i] = (n_i, 0) from the caller's interleaved xyz array
__global__ __launch_bounds__(kBlock) void plane_normals4_kernel(const double *__restrict__ aos, int nm,
                                                                double4 *__restrict__ n4)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nm) return;
    n4[i] = make_double4(aos[3 * i], aos[3 * i + 1], aos[3 * i + 2], 0.0);
}

// ---- the symmetric form's pairs (icp_set_plane_symmetric) ---------------------------------------
// Q = the rotation of the total since icp_set_scene*, by one thread: the run's so far (st->tot,
// composed by every applied step) onto the context's at the run's start (sy.q0), in compose_srt's
// arithmetic, so that it is the rotation icp_get_transform reports when the run ends here.
__device__ __forceinline__ void symm_total_rotation(const IterState *__restrict__ st, const SymmArgs &sy, double *q)
{
    if (st->tot_n == 0) {
        for (int k = 0; k < 9; ++k) q[k] = sy.q0[k]; // (the identity without one)
    } else if (!sy.have_q0) {
        for (int k = 0; k < 9; ++k) q[k] = st->tot[1 + k];
    } else {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double a = st->tot[1 + 3 * r] * sy.q0[c], b = st->tot[2 + 3 * r] * sy.q0[3 + c],
                             d = st->tot[3 + 3 * r] * sy.q0[6 + c];
                q[3 * r + c] = (a + b) + d;
            }
    }
}

// v, which every lane of the wave holds alike, as a value the compiler knows to be wave-uniform
__device__ __forceinline__ double wave_uniform(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// The pair's normal from the model's N and the scene's u0 (as given): false, and n = 0, when either is
// all zero; else u = Q u0 and n = N - u or N + u by the sign of N . u, so that the sign of either
// normal changes no bit of n but its own sign, and none of n n^T or (d . n) n.
__device__ __forceinline__ bool symm_normal(const double4 &N, double a0, double a1, double a2, const double *Q, double &n0,
                                            double &n1, double &n2)
{
    n0 = n1 = n2 = 0.0;
    if ((N.x == 0.0 && N.y == 0.0 && N.z == 0.0) || (a0 == 0.0 && a1 == 0.0 && a2 == 0.0)) return false;
    const double u0 = (Q[0] * a0 + Q[1] * a1) + Q[2] * a2;
    const double u1 = (Q[3] * a0 + Q[4] * a1) + Q[5] * a2;
    const double u2 = (Q[6] * a0 + Q[7] * a1) + Q[8] * a2;
    const double h = (N.x * u0 + N.y * u1) + N.z * u2;
    n0 = h < 0.0 ? N.x - u0 : N.x + u0;
    n1 = h < 0.0 ? N.y - u1 : N.y + u1;
    n2 = h < 0.0 ? N.z - u2 : N.z + u2;
    return true;
}

// What a moments kernel's trailing arguments ([SymmArgs,] [k, k2]) hold: the symmetric form's, and the
// pair's weight.
template <class... K> __device__ __forceinline__ const SymmArgs &symm_of(const SymmArgs &sy, K...) { return sy; }
template <int KIND> __device__ __forceinline__ double plane_weight(double r2, double k, double k2)
{
    return robust_weight<KIND>(r2, k, k2);
}
template <int KIND> __device__ __forceinline__ double plane_weight(double r2, const SymmArgs &, double k, double k2)
{
    return robust_weight<KIND>(r2, k, k2);
}

// The sums over the kept pairs (kept_pairs_pass: the gate and its mask, as the gated moments): the
// 21 + 6 of the normal equations and the kept count as the 28th (a double: exact below 2^53).  No
// shifts: r is a difference of near points, and (p - c) is taken before any product.
// KIND, a robust weight (icp_set_robust; k, k2): each of the pair's 27 terms enters as
// a += w * t with w = robust_weight<KIND>(r * r), r the residual along the normal, and W = sum w and
// K+ = #{w > 0} are the 29th and 30th sums.
// SYMM, the symmetric form: the pair's normal (symm_normal) and the sum of both lever arms, the same
// columns in the same order; Q goes through LDS, read from the loop state by one thread of the
// workgroup.  A pair without a normal counts in K and adds nothing else.
// X, what the form and the kind add to the arguments: [SymmArgs,] [k, k2] (an unused one costs the
// pairs' loop instructions).
// A frozen iteration (st->done) returns at once: neither its sums nor the mask are written.
template <bool YIN, int KIND, bool SYMM, class CUT, class... X>
__global__ __launch_bounds__(kBlock) void plane_moments_kernel(
    const int *__restrict__ idx, const double4 *__restrict__ m4, const double4 *__restrict__ n4,
    const double *__restrict__ px, const double *__restrict__ py, const double *__restrict__ pz, int n,
    double *__restrict__ yx, double *__restrict__ yy, double *__restrict__ yz, const IterState *__restrict__ st, double D,
    double c0, double c1, double c2, unsigned long long *__restrict__ mask, double *__restrict__ partials,
    const int *__restrict__ kpos, const double4 *__restrict__ m4kd, X... xx, CUT cut)
{
    constexpr bool kRobust = KIND != kRobustNone;
    constexpr int WIDTH = kept_width(true, kRobust);
    if (st->done != 0) return;
    [[maybe_unused]] double Q[SYMM ? 9 : 1]; // (the same in every lane: kept in scalar registers)
    if constexpr (SYMM) {
        __shared__ double sq[9];
        if (threadIdx.x == 0) symm_total_rotation(st, symm_of(xx...), sq);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 9; ++k) Q[k] = wave_uniform(sq[k]);
    }
    double a[WIDTH];
#pragma unroll
    for (int j = 0; j < WIDTH; ++j) a[j] = 0.0;
    kept_pairs_pass<YIN, kKeptUnique<CUT>>(
        idx, m4, px, py, pz, n, yx, yy, yz, kept_cut(D, cut_of(cut)), mask, kpos, m4kd, best_of(cut),
        [&](long long i, double q0, double q1, double q2, const double4 &y, double dx, double dy, double dz)
            __attribute__((always_inline)) {
                double v[6];
                if constexpr (SYMM) {
                    const SymmArgs &sy = symm_of(xx...);
                    a[kPlaneCount] += 1.0;
                    if (!symm_normal(n4[idx[i]], sy.ux[i], sy.uy[i], sy.uz[i], Q, v[3], v[4], v[5])) return;
                    const double l0 = (q0 - c0) + (y.x - c0), l1 = (q1 - c1) + (y.y - c1), l2 = (q2 - c2) + (y.z - c2);
                    v[0] = l1 * v[5] - l2 * v[4];
                    v[1] = l2 * v[3] - l0 * v[5];
                    v[2] = l0 * v[4] - l1 * v[3];
                } else {
                    const double4 nn = n4[idx[i]]; // (idx is final here whichever search ran: kpos rides beside it)
                    const double u0 = q0 - c0, u1 = q1 - c1, u2 = q2 - c2;
                    v[0] = u1 * nn.z - u2 * nn.y;
                    v[1] = u2 * nn.x - u0 * nn.z;
                    v[2] = u0 * nn.y - u1 * nn.x;
                    v[3] = nn.x;
                    v[4] = nn.y;
                    v[5] = nn.z;
                }
                const double r = (dx * v[3] + dy * v[4]) + dz * v[5];
                double w = 1.0; // (unweighted: not multiplied)
                if constexpr (kRobust) w = plane_weight<KIND>(r * r, xx...);
                const auto add = [&](double &sum, double t) __attribute__((always_inline)) {
                    if constexpr (kRobust) sum += w * t;
                    else sum += t;
                };
#pragma unroll
                for (int row = 0; row < 6; ++row)
#pragma unroll
                    for (int col = row; col < 6; ++col) add(a[6 * row - row * (row - 1) / 2 + (col - row)], v[row] * v[col]);
#pragma unroll
                for (int row = 0; row < 6; ++row) add(a[kPlaneB + row], v[row] * r);
                if constexpr (!SYMM) a[kPlaneCount] += 1.0;
                if constexpr (kRobust) {
                    a[kRobustPlaneW] += w;
                    a[kRobustPlaneKpos] += w > 0.0 ? 1.0 : 0.0;
                }
            });
    block_sum_store<WIDTH>(a, partials + (size_t)blockIdx.x * WIDTH);
}

// The 6 x 6 solve of one thread.  sums: the 28 folded sums; A (36) and w (12: g, then x) are the
// thread's arrays, in LDS so that no index turns into a private-memory access.  Returns whether the
// system is regular; *piv = the smallest Cholesky pivot met (0 when a diagonal entry is not > 0).
__device__ __forceinline__ bool plane_solve(const double *sums, double *A, double *w, double *piv)
{
    double *g = w, *x = w + 6;
    int k = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) A[6 * r + c] = A[6 * c + r] = sums[k++];
    *piv = 0.0;
    for (int r = 0; r < 6; ++r) {
        if (!(A[7 * r] > 0.0)) return false;
        g[r] = sqrt(A[7 * r]);
    }
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) A[6 * r + c] = A[6 * r + c] / (g[r] * g[c]);
        x[r] = -sums[kPlaneB + r] / g[r];
    }
    // Cholesky by rows, L in the lower triangle; the pivot of row r is its Schur complement
    double pmin = 1.0 / 0.0;
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < r; ++c) {
            double v = A[6 * r + c];
            for (int j = 0; j < c; ++j) v -= A[6 * r + j] * A[6 * c + j];
            A[6 * r + c] = v / A[7 * c];
        }
        double d = A[7 * r];
        for (int j = 0; j < r; ++j) d -= A[6 * r + j] * A[6 * r + j];
        pmin = d < pmin || !(d == d) ? d : pmin;
        *piv = pmin;
        if (!(d > 1e-12)) return false;
        A[7 * r] = sqrt(d);
    }
    for (int r = 0; r < 6; ++r) { // L z = b^
        double v = x[r];
        for (int j = 0; j < r; ++j) v -= A[6 * r + j] * x[j];
        x[r] = v / A[7 * r];
    }
    for (int r = 5; r >= 0; --r) { // L^T x^ = z
        double v = x[r];
        for (int j = r + 1; j < 6; ++j) v -= A[6 * j + r] * x[j];
        x[r] = v / A[7 * r];
    }
    for (int r = 0; r < 6; ++r) x[r] = x[r] / g[r];
    return true;
}

// The symmetric step from the solve's x = (a~, t~): R_h = I + g [a~]x + k2 [a~]x^2 entry by entry,
// R = R_h R_h, t = ((R_h (g t~)) + c) - R c, s = 1, composed into the run's total.  One thread.
__device__ __forceinline__ void symm_step(const double *x, double c0, double c1, double c2, IterState *__restrict__ s)
{
    const double a0 = x[0], a1 = x[1], a2 = x[2];
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double g = 1.0 / sqrt(1.0 + aa), k2 = g * g / (1.0 + g);
    double H[9];
    H[0] = 1.0 - k2 * (a1 * a1 + a2 * a2);
    H[1] = k2 * (a0 * a1) - g * a2;
    H[2] = k2 * (a0 * a2) + g * a1;
    H[3] = k2 * (a0 * a1) + g * a2;
    H[4] = 1.0 - k2 * (a0 * a0 + a2 * a2);
    H[5] = k2 * (a1 * a2) - g * a0;
    H[6] = k2 * (a0 * a2) - g * a1;
    H[7] = k2 * (a1 * a2) + g * a0;
    H[8] = 1.0 - k2 * (a0 * a0 + a1 * a1);
    const double tau[3] = {g * x[3], g * x[4], g * x[5]};
    const double c[3] = {c0, c1, c2};
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) R[3 * r + k] = (H[3 * r] * H[k] + H[3 * r + 1] * H[3 + k]) + H[3 * r + 2] * H[6 + k];
    s->srt[0] = 1.0;
    for (int k = 0; k < 9; ++k) {
        s->srt[1 + k] = R[k];
        s->xf.sR[k] = R[k];
    }
    for (int k = 0; k < 3; ++k) {
        const double Ht = (H[3 * k] * tau[0] + H[3 * k + 1] * tau[1]) + H[3 * k + 2] * tau[2];
        const double Rc = (R[3 * k] * c0 + R[3 * k + 1] * c1) + R[3 * k + 2] * c2;
        const double t = (Ht + c[k]) - Rc;
        s->srt[10 + k] = t;
        s->xf.t[k] = t;
        s->xf.c[k] = c[k];
    }
    double inc[13];
    for (int k = 0; k < 13; ++k) inc[k] = s->srt[k];
    compose_srt(inc, s->tot, &s->tot_n);
}

// The fold of the moments' partial rows into sums[0..width) (nblocks > 0; one row in flight: 28 columns
// leave no registers for four) and / or the solve and step on sums (step; nblocks = 0: the sums as
// they are, all-reduced).  The step decides from the global sums, identical on every rank: K < 6 or
// a degenerate system freezes the run with its status (kept_stop); else s = 1, R, t of the solve.
// ROBUST, the weighted rows: K+ < 6 freezes the run as well, the system solved is the weighted one,
// and a solved iteration's W and K+ join their mapped traces.
// trim_few: the trim's T is below the least count (icp_set_trim), which stops the run like K.
// SYMM, the symmetric form: the same fold, counts and solve; the step is the half rotation applied
// twice about c (the file's head), with no trigonometry.
template <bool ROBUST, bool SYMM = false>
__device__ __forceinline__ void plane_solve_body(
    const double *__restrict__ partials, int nblocks, double *__restrict__ sums, int step, double c0, double c1, double c2,
    int *__restrict__ cnt, IterState *__restrict__ s, GateState *__restrict__ g, GateState *__restrict__ h_g,
    IterState *__restrict__ h_state, double *__restrict__ h_wtrace, long long *__restrict__ h_ptrace, int trim_few)
{
    constexpr int WIDTH = kept_width(true, ROBUST);
    __shared__ double res[WIDTH];
    __shared__ double A[36], w[12];
    if (nblocks > 0) {
        fold_to<WIDTH, 1>(partials, nblocks, sums, res);
    } else {
        if (threadIdx.x < WIDTH) res[threadIdx.x] = sums[threadIdx.x];
        __syncthreads();
    }
    if (!step || threadIdx.x != 0) return;
    if (!s->done) { // (a frozen iteration's sums are stale: its gate was not evaluated)
        const double K = res[kPlaneCount];
        g->K = (long long)K;
        h_g->K = (long long)K;
        int status = 0;
        double piv = 0.0;
        bool few = !(K >= 6.0) || trim_few != 0;
        if constexpr (ROBUST) {
            const double W = res[kRobustPlaneW], Kpos = res[kRobustPlaneKpos];
            g->W = W;
            g->Kpos = (long long)Kpos;
            h_g->W = W;
            h_g->Kpos = (long long)Kpos;
            few = few || !(Kpos >= 6.0);
        }
        if (few) status = kGateTooFew;
        else if (!plane_solve(res, A, w, &piv)) status = kPlaneDegenerate;
        if (status) kept_stop(s, g, h_g, h_state, status, piv);
        if constexpr (ROBUST) {
            if (!status) {
                h_wtrace[s->iter] = res[kRobustPlaneW];
                h_ptrace[s->iter] = (long long)res[kRobustPlaneKpos];
            }
        }
    }
    if (!step_counters(cnt, s)) return; // (done: the search's counters only)
    if constexpr (SYMM) {
        symm_step(w + 6, c0, c1, c2, s);
        return;
    }
    // R = exp([omega]x) by Rodrigues: I + (sin th / th) W + (2 sin^2(th / 2) / th^2) W^2
    const double o0 = w[6], o1 = w[7], o2 = w[8];
    const double th2 = (o0 * o0 + o1 * o1) + o2 * o2;
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (th2 > 0.0) {
        const double th = sqrt(th2);
        const double sa = sin(th) / th, h = sin(0.5 * th) / th, sb = 2.0 * (h * h);
        R[0] = 1.0 - sb * (o1 * o1 + o2 * o2);
        R[1] = sb * (o0 * o1) - sa * o2;
        R[2] = sb * (o0 * o2) + sa * o1;
        R[3] = sb * (o0 * o1) + sa * o2;
        R[4] = 1.0 - sb * (o0 * o0 + o2 * o2);
        R[5] = sb * (o1 * o2) - sa * o0;
        R[6] = sb * (o0 * o2) - sa * o1;
        R[7] = sb * (o1 * o2) + sa * o0;
        R[8] = 1.0 - sb * (o0 * o0 + o1 * o1);
    }
    const double c[3] = {c0, c1, c2};
    s->srt[0] = 1.0;
    for (int k = 0; k < 9; ++k) {
        s->srt[1 + k] = R[k];
        s->xf.sR[k] = R[k];
    }
    for (int k = 0; k < 3; ++k) {
        const double Rc = (R[3 * k] * c0 + R[3 * k + 1] * c1) + R[3 * k + 2] * c2;
        const double t = (c[k] + w[9 + k]) - Rc;
        s->srt[10 + k] = t;
        s->xf.t[k] = t;
        s->xf.c[k] = c[k];
    }
    double inc[13]; // (the step is applied: a frozen iteration returned above)
    for (int k = 0; k < 13; ++k) inc[k] = s->srt[k];
    compose_srt(inc, s->tot, &s->tot_n);
}

// (The step is an inlined function under the kernel, not the kernel's own body: written straight
// into the kernel the same text compiles to another instruction stream.)
template <bool ROBUST, bool SYMM>
__global__ __launch_bounds__(kBlock) void plane_solve_kernel(
    const double *__restrict__ partials, int nblocks, double *__restrict__ sums, int step, double c0, double c1, double c2,
    int *__restrict__ cnt, IterState *__restrict__ s, GateState *__restrict__ g, GateState *__restrict__ h_g,
    IterState *__restrict__ h_state, double *__restrict__ h_wtrace, long long *__restrict__ h_ptrace, int trim_few)
{
    plane_solve_body<ROBUST, SYMM>(partials, nblocks, sums, step, c0, c1, c2, cnt, s, g, h_g, h_state, h_wtrace, h_ptrace,
                                   trim_few);
}

// Every point moves, and the squared residual along the normal, gathered again through idx, is
// summed over the kept points (kept_transform).  S, the symmetric form's SymmArgs or nothing: with it
// the pair's normal is formed again from Q', the total's rotation with the step just composed (the
// step kernel ran before this one; a frozen run returns before Q' is used).
template <class... S>
__global__ __launch_bounds__(kBlock) void plane_transform_kernel(
    double *__restrict__ px, double *__restrict__ py, double *__restrict__ pz, const double *__restrict__ yx,
    const double *__restrict__ yy, const double *__restrict__ yz, int n, const Xform *__restrict__ xfd,
    const int *__restrict__ done, float4 *__restrict__ p32, const unsigned long long *__restrict__ mask,
    const int *__restrict__ idx, const double4 *__restrict__ n4, double *__restrict__ partials, S... sy)
{
    constexpr bool SYMM = sizeof...(S) != 0;
    [[maybe_unused]] double Q[SYMM ? 9 : 1]; // (the same in every lane: kept in scalar registers)
    if constexpr (SYMM) {
        __shared__ double sq[9];
        if (threadIdx.x == 0) symm_total_rotation(symm_of(sy...).st, symm_of(sy...), sq);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 9; ++k) Q[k] = wave_uniform(sq[k]);
    }
    kept_transform(px, py, pz, n, xfd, done, p32, mask, partials,
                   [&](long long i, double q0, double q1, double q2) __attribute__((always_inline)) {
                       double n0, n1, n2;
                       if constexpr (SYMM) {
                           const SymmArgs &u = symm_of(sy...);
                           symm_normal(n4[idx[i]], u.ux[i], u.uy[i], u.uz[i], Q, n0, n1, n2);
                       } else {
                           const double4 nn = n4[idx[i]];
                           n0 = nn.x, n1 = nn.y, n2 = nn.z;
                       }
                       const double e0 = q0 - yx[i], e1 = q1 - yy[i], e2 = q2 - yz[i];
                       const double rn = (e0 * n0 + e1 * n1) + e2 * n2;
                       return rn * rn;
                   });
}

// (x, y, z)[i] = the first three of rows[i] (estimated normals into the scene normals' streams)
__global__ __launch_bounds__(kBlock) void rows4_to_soa_kernel(const double4 *__restrict__ rows, int n, double *__restrict__ x,
                                                              double *__restrict__ y, double *__restrict__ z)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double4 r = rows[i];
    x[i] = r.x;
    y[i] = r.y;
    z[i] = r.z;
}

} // namespace

void launch_rows4_to_soa(const double4 *rows, int n, double *x, double *y, double *z, hipStream_t st)
{
    if (n <= 0) return;
    rows4_to_soa_kernel<<<(n + kBlock - 1) / kBlock, kBlock, 0, st>>>(rows, n, x, y, z);
}

void launch_plane_normals4(const double *aos, int nm, double4 *n4, hipStream_t st)
{
    if (nm <= 0) return;
    plane_normals4_kernel<<<(nm + kBlock - 1) / kBlock, kBlock, 0, st>>>(aos, nm, n4);
}

void plane_moments(const KeptPass &a, bool y_ready)
{
    kept_dispatch(y_ready, a.robust_kind, [&](auto yin, auto kind) {
        // the kernel of (yin, kind, the form) with what these add to its arguments: [SymmArgs,] [k, k2]
        const auto go = [&](auto symm, auto... xx) {
            kept_tail(yin, a, [&](auto cut) {
                plane_moments_kernel<yin(), kind(), symm(), decltype(cut), decltype(xx)...>
                    <<<red_blocks(a.n), kBlock, 0, a.st>>>(a.idx, a.m4, a.n4, a.px, a.py, a.pz, a.n, a.yx, a.yy, a.yz, a.st_dev,
                                                           a.D, a.c[0], a.c[1], a.c[2], a.mask, a.partials, a.kpos, a.m4kd,
                                                           xx..., cut);
            });
        };
        const auto of_form = [&](auto... kk) {
            if (a.symm) go(std::true_type(), *a.symm, kk...);
            else go(std::false_type(), kk...);
        };
        if constexpr (kind() == kRobustNone) of_form();
        else of_form(a.k, a.k2);
    });
}

void plane_step(const KeptStep &a, const double *partials, int nblocks, bool step)
{
    static constexpr decltype(&plane_solve_kernel<false, false>) kernels[2][2] = {
        {plane_solve_kernel<false, false>, plane_solve_kernel<false, true>},
        {plane_solve_kernel<true, false>, plane_solve_kernel<true, true>}};
    kernels[a.robust][a.symm]<<<1, kBlock, 0, a.st>>>(partials, nblocks, a.sums, step ? 1 : 0, a.c[0], a.c[1], a.c[2],
                                                      a.amb_count, a.st_dev, a.gate, a.h_gate, a.h_state, a.h_wtrace,
                                                      a.h_ptrace, a.trim_few ? 1 : 0);
}

void plane_transform(double *px, double *py, double *pz, const double *yx, const double *yy, const double *yz, int n,
                     const Xform *xf, const int *done, float4 *p32, const unsigned long long *mask, const int *idx,
                     const double4 *n4, double *partials, hipStream_t st, const SymmArgs *symm)
{
    const auto go = [&](auto... sy) {
        plane_transform_kernel<<<red_blocks(n), kBlock, 0, st>>>(px, py, pz, yx, yy, yz, n, xf, done, p32, mask, idx, n4,
                                                                 partials, sy...);
    };
    if (symm) go(*symm);
    else go();
}

} // namespace icp
