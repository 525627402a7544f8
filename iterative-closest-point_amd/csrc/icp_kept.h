// icp_kept.h — what the kept-pairs iterations share on the device (icp_gated.hip: point-to-point
// under the max-distance gate; icp_plane.hip: point-to-plane, gated or not; icp_gicp.hip: its
// plane-to-plane form).  Private to those three files, which hold each metric's own arithmetic and
// are compiled with IEEE semantics (`d2 <= D` must stay false for a NaN):
//   kept_pairs_pass   the moments kernels' loop: y, the gate, the mask word, a callable per kept pair
//   kept_cut          a trimmed iteration's gate: the smaller of D and the cut selected on the device
//   robust_weight     a kept pair's weight from its squared residual (icp_set_robust)
//   kept_dispatch     the moments kernels' instantiation for a pass: <stored y or gathered, robust kind>
//   kept_transform    the transform kernels' body: every point moves, a callable gives a kept
//                     point's squared residual
//   fold_to           the fold of per-workgroup partial rows (reduce_kernel's tree)
//   kept_stop         the freeze of a run whose iteration cannot be solved
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "icp_device.h"
#include "icp_kernels.h"

namespace icp {

// icp_plane.hip's side of launch_kept_moments, launch_kept_step and launch_kept_transform (icp_gated.hip);
// with KeptPass::symm / KeptStep::symm / symm set, the kernels' symmetric instantiations (icp_set_plane_symmetric)
void plane_moments(const KeptPass &a, bool y_ready);
void plane_step(const KeptStep &a, const double *partials, int nblocks, bool step);
void plane_transform(double *px, double *py, double *pz, const double *yx, const double *yy, const double *yz, int n,
                     const Xform *xf, const int *done, float4 *p32, const unsigned long long *mask, const int *idx,
                     const double4 *n4, double *partials, hipStream_t st, const SymmArgs *symm);

namespace {

// For every point i of this thread's grid stride: y_i = m[idx_i] (YIN: streamed from the copy the
// search or a pre-pass stored; else gathered and stored), d = p_i - y_i, keep = d2 <= D with
// d2 = (dx*dx + dy*dy) + dz*dz as written, and kept(i, p, y, d) for a kept pair.
// The loop runs whole waves (its bound is the wave's first point), so that every lane takes part
// in the ballot; word w of the mask holds points 64 w .. 64 w + 63 and is stored by lane 0.
// UNIQ (icp_set_one_to_one; a template flag: the other instantiations carry no argument, register
// or branch for it): best is the min pass's table (icp_unique.hip), and a pair within D is kept only
// when key(d2) == best[idx_i], d2 being the bits that pass scattered (the same p, the stored y, the
// same expression).
template <bool YIN, bool UNIQ, class Kept>
__device__ __forceinline__ void kept_pairs_pass(const int *__restrict__ idx, const double4 *__restrict__ m4,
                                                const double *__restrict__ px, const double *__restrict__ py,
                                                const double *__restrict__ pz, int n, double *__restrict__ yx,
                                                double *__restrict__ yy, double *__restrict__ yz, double D,
                                                unsigned long long *__restrict__ mask, const int *__restrict__ kpos,
                                                const double4 *__restrict__ m4kd,
                                                const unsigned long long *__restrict__ best, Kept &&kept)
{
    const int lane = threadIdx.x & 63;
    const long long G = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i - lane < n; i += G) {
        bool keep = false;
        if (i < n) {
            double4 m;
            if constexpr (YIN) { // (the search wrote y = m[idx]: the same values, streamed)
                m = make_double4(yx[i], yy[i], yz[i], 0.0);
            } else {
                m = kpos ? m4kd[kpos[i]] : m4[idx[i]]; // (kpos: the same point, kd-ordered copy)
                yx[i] = m.x;
                yy[i] = m.y;
                yz[i] = m.z;
            }
            const double q0 = px[i], q1 = py[i], q2 = pz[i];
            const double dx = q0 - m.x, dy = q1 - m.y, dz = q2 - m.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            keep = d2 <= D;
            if constexpr (UNIQ) {
                if (keep) keep = select_key(d2) == best[idx[i]];
            }
            if (keep) kept(i, q0, q1, q2, m, dx, dy, dz);
        }
        const unsigned long long word = __ballot(keep);
        if (lane == 0) mask[i >> 6] = word;
    }
}

// A moments kernel's last argument, CUT: the trim's nullable cut alone (const double *: the kernel
// as it is without one-to-one), or with one-to-one on (KeptCutBest) the cut and the table.
struct KeptCutBest {
    const double *cut;
    const unsigned long long *best;
};
template <class CUT> constexpr bool kKeptUnique = std::is_same<CUT, KeptCutBest>::value;
__device__ __forceinline__ const double *cut_of(const double *c) { return c; }
__device__ __forceinline__ const double *cut_of(const KeptCutBest &c) { return c.cut; }
__device__ __forceinline__ const unsigned long long *best_of(const double *) { return nullptr; }
__device__ __forceinline__ const unsigned long long *best_of(const KeptCutBest &c) { return c.best; }

// D of an iteration: the gate's, or with a trim (icp_set_trim; cut not null) the smaller of it and
// the cut the selection left in device memory (icp_select.hip).  A NaN cut leaves D.
__device__ __forceinline__ double kept_cut(double D, const double *__restrict__ cut)
{
    if (!cut) return D;
    const double C = *cut;
    return C < D ? C : D;
}

// The robust weight of a kept pair from its squared residual r2 (icp_set_robust; k2 = k * k from the
// host), fp64 as written.  KIND is a template parameter: the pairs' loop carries no switch.  Every
// comparison is false for a NaN, so a NaN residual weighs 0; Huber is exactly 1.0 within k.
template <int KIND>
__device__ __forceinline__ double robust_weight(double r2, double k, double k2)
{
    if constexpr (KIND == kRobustHuber) {
        return r2 <= k2 ? 1.0 : (r2 > k2 ? k / sqrt(r2) : 0.0);
    } else if constexpr (KIND == kRobustTukey) {
        const double u = 1.0 - r2 / k2;
        return r2 < k2 ? u * u : 0.0;
    } else {
        static_assert(KIND == kRobustCauchy, "robust_weight: unknown kind");
        return r2 == r2 ? 1.0 / (1.0 + r2 / k2) : 0.0;
    }
}

// g(a.cut) or, with one-to-one on, g(KeptCutBest): a moments kernel's last argument and its type.
// The one-to-one kernels exist in the streamed form alone (yin: the min pass has stored y).
template <class YIN, class Pass, class G> void kept_tail(YIN, const Pass &a, G &&g)
{
    if constexpr (YIN::value) {
        if (a.best) return g(KeptCutBest{a.cut, a.best});
    }
    g(a.cut);
}

// f(YIN, KIND) with the pass's (y_ready, robust kind) as integral constants: a moments kernel's
// template arguments.  A weighted KIND's kernel takes k and k2 behind m4kd, the unweighted one does
// not (an unused pair costs its pairs' loop instructions).
template <class F> void kept_dispatch(bool y_ready, int kind, F &&f)
{
    const auto of_kind = [&](auto yin) {
        switch (kind) {
        case kRobustNone: return f(yin, std::integral_constant<int, kRobustNone>());
        case kRobustHuber: return f(yin, std::integral_constant<int, kRobustHuber>());
        case kRobustTukey: return f(yin, std::integral_constant<int, kRobustTukey>());
        default: return f(yin, std::integral_constant<int, kRobustCauchy>());
        }
    };
    if (y_ready) of_kind(std::true_type());
    else of_kind(std::false_type());
}

// A transform kernel's body: p <- sR p + t for every point (p32 nullable), and this workgroup's
// partial [sum over the kept points (the gate's mask words) of residual(i, p')].  A no-op once *done.
template <class Residual>
__device__ __forceinline__ void kept_transform(double *__restrict__ px, double *__restrict__ py, double *__restrict__ pz,
                                               int n, const Xform *__restrict__ xfd, const int *__restrict__ done,
                                               float4 *__restrict__ p32, const unsigned long long *__restrict__ mask,
                                               double *__restrict__ partials, Residual &&residual)
{
    __shared__ Xform sxf;
    __shared__ int sdone;
    if (threadIdx.x == 0) {
        sdone = *done;
        sxf = *xfd;
    }
    __syncthreads();
    if (sdone) return;
    const Xform xf = sxf;
    double a[1] = {0.0};
    const long long G = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += G) {
        double q0, q1, q2;
        transform_point(xf, px[i], py[i], pz[i], q0, q1, q2);
        if ((mask[i >> 6] >> (i & 63)) & 1ull) a[0] += residual(i, q0, q1, q2);
        px[i] = q0;
        py[i] = q1;
        pz[i] = q2;
        if (p32) p32[i] = make_float4((float)(q0 - xf.c[0]), (float)(q1 - xf.c[1]), (float)(q2 - xf.c[2]), 0.0f);
    }
    block_sum_store<1>(a, partials + blockIdx.x);
}

// reduce_kernel<K>'s tree over nblocks rows of K doubles: out[k] (global) and res[k] (LDS) for
// k < K; every thread of the workgroup must call it.  One row folds to itself.  ROWS: fold_rows'
// rows in flight.
template <int K, int ROWS = 4>
__device__ __forceinline__ void fold_to(const double *__restrict__ partials, int nblocks, double *__restrict__ out,
                                        double *res)
{
    __shared__ double sh[kBlock / 64][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    fold_rows<K, ROWS>(partials, nblocks, a);
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wave][k] = a[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double r = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) r += sh[w][threadIdx.x];
        out[threadIdx.x] = r;
        res[threadIdx.x] = r;
    }
    __syncthreads();
}

// An iteration that cannot be solved freezes the run (done) before anything of it is applied: the
// status, the iteration and the pivot go to the device state and its host mirror, and the loop
// state of the last completed iteration is mirrored to the host.  One thread.
__device__ __forceinline__ void kept_stop(IterState *__restrict__ s, GateState *__restrict__ g, GateState *__restrict__ h_g,
                                          IterState *__restrict__ h_state, int status, double min_pivot)
{
    s->done = 1;
    g->status = status;
    g->fail_iter = s->iter;
    g->min_pivot = min_pivot;
    h_g->status = status;
    h_g->fail_iter = s->iter;
    h_g->min_pivot = min_pivot;
    const int *src = (const int *)s;
    int *dst = (int *)h_state;
    for (size_t k = 0; k < sizeof(IterState) / sizeof(int); ++k) dst[k] = src[k];
}

} // namespace
} // namespace icp
