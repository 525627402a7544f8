// icp_fold.h — device pieces shared by the kernels that end an ICP iteration on the device
// (icp_iter.hip's tails and one-launch loops, icp_kernels.hip's fused moments / transform
// passes): the Horn step and the error step on the folded sums, and the write-through hand-off
// of per-workgroup partials (publish, coherent loads, reduce_kernel's fold tree).
#pragma once
#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_horn.h"
#include "icp_kernels.h"

namespace icp {
namespace {

// The counters every step kernel keeps for the loop, whatever its metric: the search's queue sizes
// into the statistics, then zeroed for the next search (always: the next search appends to these
// counters even after the loop has converged or stopped).  Returns whether the loop still runs.
__device__ __forceinline__ bool step_counters(int *__restrict__ cnt, IterState *__restrict__ s)
{
    const int qc[4] = {cnt[0], cnt[1], cnt[2], cnt[3]};
    for (int k = 0; k < 4; ++k) cnt[k] = 0;
    s->far_acc = 0; // (this iteration's transform counts afresh)
    s->queued2 = qc[2];
    if (s->done) return false;
    for (int k = 0; k < 4; ++k) s->nn_counts[k] += qc[k];
    return true;
}

// early_total (a compile-time constant at every call): the first and the last word of the run's total
// are loaded before the solve, which brings its two cache lines near while the solve runs (the
// canonical fold, where the step is on every iteration's critical path and the state is in global
// memory); the rest is loaded where it is composed.  Loading all of it early cost the fold 27 VGPRs
// and the benchmark 2 % (profiles/voxel/bench_ab.txt).
__device__ __forceinline__ void horn_step_body(const double *__restrict__ sums, double N, double c0, double c1, double c2,
                               int shifted, int *__restrict__ cnt, IterState *__restrict__ s, bool early_total = false)
{
    if (!step_counters(cnt, s)) return;
    double tot_first = 0.0, tot_last = 0.0;
    if (early_total) {
        tot_first = s->tot[0];
        tot_last = s->tot[12];
    }
    double mu_p[3], mu_y[3], S[9], d_caps, sp;
    if (!shifted) { // two-pass sums (moments_phase): Σp, Σy, then centred S, d_caps, sp
        for (int k = 0; k < 3; ++k) {
            mu_p[k] = sums[kSumP + k] / N; // rowwise().mean() (gpu.cc:98-99)
            mu_y[k] = sums[kSumY + k] / N;
        }
        for (int k = 0; k < 9; ++k) S[k] = sums[kSumS + k];
        d_caps = sums[kSumDcaps];
        sp = sums[kSumSp];
    } else { // one pass around (cp, cy): remove the shift
        double dp[3], dy[3];
        for (int k = 0; k < 3; ++k) {
            dp[k] = sums[kSumP + k] / N;
            dy[k] = sums[kSumY + k] / N;
            mu_p[k] = s->shift_p[k] + dp[k];
            mu_y[k] = s->shift_y[k] + dy[k];
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) S[3 * r + c] = sums[kSumS + 3 * r + c] - sums[kSumP + r] * dy[c];
        d_caps = sums[kSumDcaps] - ((sums[kSumY] * dy[0] + sums[kSumY + 1] * dy[1]) + sums[kSumY + 2] * dy[2]);
        sp = sums[kSumSp] - ((sums[kSumP] * dp[0] + sums[kSumP + 1] * dp[1]) + sums[kSumP + 2] * dp[2]);
    }
    double sc, R[9], t[3];
    horn_solve(S, mu_p, mu_y, d_caps, sp, &sc, R, t);
    double step[13];
    step[0] = sc;
    for (int k = 0; k < 9; ++k) step[1 + k] = R[k];
    for (int k = 0; k < 3; ++k) step[10 + k] = t[k];
    for (int k = 0; k < 13; ++k) s->srt[k] = step[k];
    for (int k = 0; k < 9; ++k) s->xf.sR[k] = sc * R[k];
    for (int k = 0; k < 3; ++k) s->xf.t[k] = t[k];
    // the run's total (icp_get_transform): this step's transform follows, so it is applied
    if (early_total) {
        double tot[13];
        tot[0] = tot_first;
        for (int k = 1; k < 12; ++k) tot[k] = s->tot[k];
        tot[12] = tot_last;
        int tot_n = s->tot_n;
        compose_srt(step, tot, &tot_n);
        for (int k = 0; k < 13; ++k) s->tot[k] = tot[k];
        s->tot_n = tot_n;
    } else {
        compose_srt(step, s->tot, &s->tot_n);
    }
    s->xf.c[0] = c0;
    s->xf.c[1] = c1;
    s->xf.c[2] = c2;
    // the next iteration's shifts: the transformed scene's centroid (exactly sR mu_p + t in
    // real arithmetic) and this iteration's correspondence centroid
    double smu[3];
    matvec3(s->xf.sR, mu_p, smu);
    for (int k = 0; k < 3; ++k) {
        s->shift_p[k] = smu[k] + t[k];
        s->shift_y[k] = mu_y[k];
    }
}

__device__ __forceinline__ void err_step_body(const double *__restrict__ sums, double N, double threshold, int max_iter,
                              double *__restrict__ err_trace, IterState *__restrict__ s, int *hflag, int ticket,
                              IterState *h_state, double *h_trace, bool far_coherent = false, int far_global = -1,
                              bool running_published = false)
{
    // The state's four words the step reads, loaded together: one memory round trip when s is
    // global, not three dependent ones (done; then iter; then, the run going on, the two counts)
    // (far_coherent: s is global and this launch's workgroups added to s->far_acc -- a fused
    // transform -- so its count is read at agent scope; s may be an LDS copy otherwise)
    int done = s->done, iter = s->iter;
    const int queued2 = s->queued2;
    const int far_acc = far_coherent ? __hip_atomic_load(&s->far_acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : s->far_acc;
    asm volatile("" ::"v"(queued2), "v"(far_acc)); // (here: the compiler sinks a load used under one condition below it)
    if (!done) {
        const double e = sums[kSumErr];
        const double err = (e + e) / N; // gpu.cc:71-76: find_alignment's residual is the same sum
        err_trace[iter] = err;
        iter += 1;
        s->iter = iter;
        if (err < threshold || iter >= max_iter) s->done = done = 1; // gpu.cc:79-80
        if (running_published && !done) return; // (the host side is err_publish_running's, on another wave)
        h_trace[iter - 1] = err; // mapped host copies: the run's result needs no copy back
        // the mirror: every field once the run is done (the result: iter, srt, nn_counts); before
        // that only what the host reads while the run goes on (the policy's far_acc and queued2) --
        // each field is a posted write over the host link that the ticket's release waits for
        if (done) {
            const int *src = (const int *)s;
            int *dst = (int *)h_state;
            for (size_t k = 0; k < sizeof(IterState) / sizeof(int); ++k) dst[k] = src[k];
            if (far_coherent) h_state->far_acc = far_acc;
        } else {
            h_state->iter = iter;
            h_state->far_acc = far_acc;
            h_state->queued2 = queued2;
        }
        if (far_global >= 0) h_state->far_acc = far_global; // (all ranks' count: sums[kSumFar] after the all-reduce)
    }
    // (done, iter) to the host (mapped memory), then the ticket the host spins on
    __hip_atomic_store(hflag, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(hflag + 1, iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(hflag + 2, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The host side of an error step that leaves the run going, from the values the step will read
// (the state's words loaded before any thread steps it, the residual's sum): what err_step_body
// writes to the host then, bit for bit, and nothing on the device.  A step that ends the run, or
// finds it ended, is published by the thread that steps it (running_published), whole mirror
// and all; both take the decision by the same arithmetic from the same values.
__device__ __forceinline__ void err_publish_running(double e, double N, double threshold, int max_iter, int done, int iter,
                                                    int far_acc, int queued2, int *hflag, int ticket,
                                                    IterState *h_state, double *h_trace)
{
    if (done) return;
    const double err = (e + e) / N;
    if (err < threshold || iter + 1 >= max_iter) return;
    h_trace[iter] = err;
    h_state->iter = iter + 1;
    h_state->far_acc = far_acc;
    h_state->queued2 = queued2;
    __hip_atomic_store(hflag, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(hflag + 1, iter + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(hflag + 2, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Hand-off (guide §6 Guideline 16, R1): partials are stored write-through (relaxed agent-scope
// atomic stores = sc1), every storing wave drains (s_waitcnt vmcnt(0)) before the workgroup
// barrier, and every load of a partial is an agent-scope atomic load or an sc1 buffer load.
__device__ __forceinline__ void pub_store(double *p, double v)
{
    __hip_atomic_store((unsigned long long *)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double pub_load(const double *p)
{
    return __longlong_as_double((long long)__hip_atomic_load((unsigned long long *)p, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}

// Row b (K of its S doubles) of the published partials, with write-through-coherent (sc1)
// loads issued together: 16-byte buffer loads when the row is 16-byte aligned (S even), else
// agent-scope atomic loads.
template <int K, int S> __device__ __forceinline__ void load_row(const double *part, int nblocks, int b, double (&v)[K])
{
    if constexpr (S % 2 == 0) {
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void *)part, (short)0, (int)((size_t)nblocks * S * sizeof(double)), 0x00020000);
        const int base = (int)((size_t)b * S * sizeof(double));
        constexpr int G = (K + 1) / 2;
        decltype(__builtin_amdgcn_raw_buffer_load_b128(rsrc, 0, 0, 0)) g[G];
#pragma unroll
        for (int j = 0; j < G; ++j) g[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, base + 16 * j, 0, 16 /* sc1 */);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const auto &q = g[k / 2];
            const unsigned lo = (k & 1) ? q[2] : q[0], hi = (k & 1) ? q[3] : q[1];
            v[k] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = pub_load(part + (size_t)b * S + k);
    }
}

// reduce_kernel<K>'s result from the published partials (rows of S >= K doubles), into LDS out[0..K)
template <int K, int S = K> __device__ __forceinline__ void tail_fold(const double *part, int nblocks, double *out)
{
    __shared__ double sh[kBlock / 64][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    constexpr int kRows = K <= 2 ? 4 : 1; // (narrow rows: four rows' loads in flight, the same sums in order)
    for (int b0 = threadIdx.x; b0 < nblocks; b0 += kRows * kBlock) {
        double v[kRows][K];
#pragma unroll
        for (int u = 0; u < kRows; ++u)
            if (b0 + u * kBlock < nblocks) load_row<K, S>(part, nblocks, b0 + u * kBlock, v[u]);
#pragma unroll
        for (int u = 0; u < kRows; ++u)
            if (b0 + u * kBlock < nblocks)
#pragma unroll
                for (int k = 0; k < K; ++k) a[k] += v[u][k];
    }
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
    }
    __syncthreads();
}

// block_sum_store<K>'s tree with the row published write-through (pub_store): the same bits
template <int K> __device__ __forceinline__ void block_sum_publish(double (&a)[K], double *out)
{
    __shared__ double sh[kBlock / 64][K];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += __shfl_down(a[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wave][k] = a[k];
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        pub_store(out + k, ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k]);
    }
}

// The last-arrival hand-off of a launch whose workgroups each published a partial row
// (block_sum_publish): true in the one workgroup that arrives last, which may then read every
// row (tail_fold's coherent loads).  Every workgroup of the launch must call it.  The arrival
// counter is back at zero when the launch ends (the last arrival resets it), so one counter
// serves every launch of its kernel on a stream.
__device__ __forceinline__ bool last_arrival(unsigned *ticket)
{
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's write-through stores have landed
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old + 1 == gridDim.x;
        if (s_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return s_last != 0;
}

} // namespace
} // namespace icp
