// icp_select.hip — the k-th smallest of n doubles on the device: the cut of a trimmed iteration
// (icp_set_trim) and icp_select_kth.
//
// An exact MSB-first radix select over 64-bit keys.  The key is the monotone map of the fp64 bit
// pattern (select_key): the sign bit flipped for non-negatives, every bit flipped for negatives,
// every NaN mapped to all ones, so that the keys' unsigned order is
//   -inf < ... < -0 < +0 < ... < +inf < NaN.
// Six passes over digits of 11, 11, 11, 11, 11 and 9 bits (kSelectShift), most significant first.
// One pass is two launches:
//   select_count_kernel  red_blocks(n) workgroups; each builds the histogram of the pass's digit in
//                        LDS with integer LDS atomics, over the keys whose higher bits equal the
//                        prefix chosen so far, and adds its non-empty bins to the 2,048 global
//                        ones with one integer atomic each;
//   select_pick_kernel   one workgroup scans the bins, finds the digit that holds the remaining
//                        rank, updates {prefix, remaining} in the device state and zeroes the bins.
// Up to kRedSingle keys on one rank, where every pass is one workgroup's anyway, the six passes are
// one launch of one workgroup with the bins and the state in LDS (select_small_kernel).
// With ranks the bins travel between the two as doubles (select_bins_kernel; exact below 2^53)
// through the all-reduce, like the sums.  Counts are integers, so every schedule and every split
// of the keys over ranks gives the same answer; there is no floating-point atomic.  The last pick
// writes the value of the selected key to *cut and, in a run, to the mapped trace.
// A frozen run (*done) skips every kernel, as the moments do.
// select_keys_kernel is the trimmed iteration's keys pass: y = m[idx] (stored unless the search
// wrote it), and the key of d2 = (dx*dx + dy*dy) + dz*dz, the gate's own value as written.
// Compiled with IEEE semantics like icp_gated.hip.
#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_kernels.h"

namespace icp {
namespace {

// (select_key, the map itself: icp_device.h, shared with the one-to-one rejector)
__device__ __forceinline__ double select_value(unsigned long long key)
{
    if (key == ~0ull) return __longlong_as_double(0x7ff8000000000000ll); // (a quiet NaN)
    return __longlong_as_double((long long)((key & kSignBit) ? (key ^ kSignBit) : ~key));
}

__global__ __launch_bounds__(kBlock) void select_map_kernel(const double *__restrict__ v, int n,
                                                            unsigned long long *__restrict__ keys)
{
    const long long G = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += G) keys[i] = select_key(v[i]);
}

// kept_pairs_pass's y and d2 (icp_kept.h), without the gate: the moments that follow stream the
// stored y and recompute d2 from the same p and y, hence its bits.
template <bool YIN>
__global__ __launch_bounds__(kBlock) void select_keys_kernel(
    const int *__restrict__ idx, const double4 *__restrict__ m4, const double *__restrict__ px,
    const double *__restrict__ py, const double *__restrict__ pz, int n, double *__restrict__ yx,
    double *__restrict__ yy, double *__restrict__ yz, const int *__restrict__ done,
    unsigned long long *__restrict__ keys, const int *__restrict__ kpos, const double4 *__restrict__ m4kd)
{
    if (*done != 0) return;
    const long long G = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += G) {
        double4 m;
        if constexpr (YIN) {
            m = make_double4(yx[i], yy[i], yz[i], 0.0);
        } else {
            m = kpos ? m4kd[kpos[i]] : m4[idx[i]];
            yx[i] = m.x;
            yy[i] = m.y;
            yz[i] = m.z;
        }
        const double dx = px[i] - m.x, dy = py[i] - m.y, dz = pz[i] - m.z;
        keys[i] = select_key((dx * dx + dy * dy) + dz * dz);
    }
}

// himask: the bits above the pass's digit (0 in the first pass: every key counts)
__global__ __launch_bounds__(kBlock) void select_count_kernel(const unsigned long long *__restrict__ keys, int n,
                                                              int shift, unsigned dmask, unsigned long long himask,
                                                              const SelectState *__restrict__ state,
                                                              const int *__restrict__ done, unsigned *__restrict__ bins)
{
    if (done && *done != 0) return;
    __shared__ unsigned h[kSelectBins];
    for (int b = threadIdx.x; b < kSelectBins; b += kBlock) h[b] = 0u;
    __syncthreads();
    const unsigned long long prefix = himask ? state->prefix : 0ull;
    const long long G = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += G) {
        const unsigned long long k = keys[i];
        if (((k ^ prefix) & himask) == 0ull) atomicAdd(&h[(unsigned)(k >> shift) & dmask], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kSelectBins; b += kBlock) {
        const unsigned c = h[b];
        if (c) __hip_atomic_fetch_add(bins + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the bins as doubles for the all-reduce; the integer bins are zeroed for the next pass
__global__ __launch_bounds__(kBlock) void select_bins_kernel(unsigned *__restrict__ bins, double *__restrict__ out,
                                                             const int *__restrict__ done)
{
    if (done && *done != 0) return;
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= kSelectBins) return;
    out[b] = (double)bins[b];
    bins[b] = 0u;
}

// The pick of one workgroup, every thread of it: thread t brings the counts of bins 8 t .. 8 t + 7.
// The digit whose bin holds rank `rem` (1-based, among the keys that carry `prefix`) joins the prefix:
// the one thread whose bins hold it writes sel[0] = the new prefix, sel[1] = the rank within that bin,
// and returns true.
__device__ __forceinline__ bool select_pick(const unsigned long long (&c)[8], int shift, unsigned long long prefix,
                                            unsigned long long rem, unsigned long long *sel)
{
    static_assert(kSelectBins == 8 * kBlock, "select_pick: eight bins a thread");
    __shared__ unsigned long long wave_sum[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long sum = 0ull;
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += c[j];
    unsigned long long incl = sum; // (inclusive scan of the thread sums: within the wave, then over the waves)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    __syncthreads(); // (the wave sums of the pass before are read no more)
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned long long before = incl - sum;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (!(before < rem && rem <= before + sum)) return false; // (one thread's bins hold the rank)
    bool mine = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (!mine && before < rem && rem <= before + c[j]) {
            sel[0] = prefix | ((unsigned long long)(8 * threadIdx.x + j) << shift);
            sel[1] = rem - before;
            mine = true;
        }
        before += c[j];
    }
    return mine;
}

// One workgroup.  rank: the rank sought (1-based), read in the first pass (first != 0); later
// passes take what the pass before left in the state.  last: the prefix is the whole key; its
// value goes to *cut and, with a run's state s, to h_trace[s->iter].
template <class Bin>
__global__ __launch_bounds__(kBlock) void select_pick_kernel(Bin *__restrict__ bins, int shift, int first, int last,
                                                             unsigned long long rank, SelectState *__restrict__ state,
                                                             const int *__restrict__ done, double *__restrict__ cut,
                                                             const IterState *__restrict__ s, double *__restrict__ h_trace)
{
    if (done && *done != 0) return;
    unsigned long long c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        c[j] = (unsigned long long)bins[8 * threadIdx.x + j];
        if constexpr (sizeof(Bin) == sizeof(unsigned)) bins[8 * threadIdx.x + j] = 0;
    }
    const unsigned long long rem = first ? rank : state->remaining;
    const unsigned long long prefix = first ? 0ull : state->prefix;
    unsigned long long sel[2]; // (select_pick's barriers: every thread has read the state before one writes it)
    if (!select_pick(c, shift, prefix, rem, sel)) return;
    state->prefix = sel[0];
    state->remaining = sel[1];
    if (last) {
        const double v = select_value(sel[0]);
        *cut = v;
        if (h_trace) h_trace[s->iter] = v;
    }
}

// The whole selection of n <= kRedSingle keys, the sizes at which every pass is one workgroup's: the
// six passes in one launch of one workgroup, the histogram and {prefix, remaining} in LDS.  The same
// counts and the same pick as the launches above, hence the same answer.
__global__ __launch_bounds__(kBlock) void select_small_kernel(const unsigned long long *__restrict__ keys, int n,
                                                              unsigned long long rank, SelectState *__restrict__ state,
                                                              const int *__restrict__ done, double *__restrict__ cut,
                                                              const IterState *__restrict__ s, double *__restrict__ h_trace)
{
    if (done && *done != 0) return;
    __shared__ unsigned h[kSelectBins];
    __shared__ unsigned long long sel[2];
    if (threadIdx.x == 0) {
        sel[0] = 0ull;
        sel[1] = rank;
    }
    for (int pass = 0; pass < kSelectPasses; ++pass) {
        const int shift = pass < kSelectPasses - 1 ? 53 - 11 * pass : 0, width = pass < kSelectPasses - 1 ? 11 : 9;
        const unsigned dmask = (1u << width) - 1u;
        const unsigned long long himask = pass == 0 ? 0ull : ~0ull << (shift + width);
        for (int b = threadIdx.x; b < kSelectBins; b += kBlock) h[b] = 0u;
        __syncthreads();
        const unsigned long long prefix = sel[0], rem = sel[1];
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const unsigned long long k = keys[i];
            if (((k ^ prefix) & himask) == 0ull) atomicAdd(&h[(unsigned)(k >> shift) & dmask], 1u);
        }
        __syncthreads();
        unsigned long long c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = h[8 * threadIdx.x + j];
        select_pick(c, shift, prefix, rem, sel);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        state->prefix = sel[0];
        state->remaining = sel[1];
        const double v = select_value(sel[0]);
        *cut = v;
        if (h_trace) h_trace[s->iter] = v;
    }
}

} // namespace

void launch_select_map(const double *v, int n, unsigned long long *keys, hipStream_t st)
{
    if (n <= 0) return;
    select_map_kernel<<<red_blocks(n), kBlock, 0, st>>>(v, n, keys);
}

void launch_select_keys(const int *idx, const double4 *m4, const double *px, const double *py, const double *pz, int n,
                        double *yx, double *yy, double *yz, const int *done, unsigned long long *keys, hipStream_t st,
                        const int *kpos, const double4 *m4kd, bool y_ready)
{
    if (n <= 0) return;
    if (y_ready)
        select_keys_kernel<true><<<red_blocks(n), kBlock, 0, st>>>(idx, m4, px, py, pz, n, yx, yy, yz, done, keys, kpos, m4kd);
    else
        select_keys_kernel<false><<<red_blocks(n), kBlock, 0, st>>>(idx, m4, px, py, pz, n, yx, yy, yz, done, keys, kpos, m4kd);
}

void launch_select_count(const unsigned long long *keys, int n, int pass, const SelectState *state, const int *done,
                         unsigned *bins, hipStream_t st)
{
    if (n <= 0) return; // (an empty shard adds nothing to the bins)
    const int shift = kSelectShift[pass], width = pass == 0 ? 64 - shift : kSelectShift[pass - 1] - shift;
    const unsigned long long himask = pass == 0 ? 0ull : ~0ull << (shift + width);
    select_count_kernel<<<red_blocks(n), kBlock, 0, st>>>(keys, n, shift, (1u << width) - 1u, himask, state, done, bins);
}

void launch_select_bins(unsigned *bins, double *out, const int *done, hipStream_t st)
{
    select_bins_kernel<<<kSelectBins / kBlock, kBlock, 0, st>>>(bins, out, done);
}

void launch_select_pick(unsigned *bins, const double *bins_reduced, int pass, unsigned long long rank, SelectState *state,
                        const int *done, double *cut, const IterState *s, double *h_trace, hipStream_t st)
{
    const int shift = kSelectShift[pass], first = pass == 0, last = pass == kSelectPasses - 1;
    if (bins_reduced)
        select_pick_kernel<const double><<<1, kBlock, 0, st>>>(bins_reduced, shift, first, last, rank, state, done, cut, s,
                                                               h_trace);
    else
        select_pick_kernel<unsigned><<<1, kBlock, 0, st>>>(bins, shift, first, last, rank, state, done, cut, s, h_trace);
}

void launch_select_kth(const unsigned long long *keys, int n, unsigned long long rank, SelectState *state, const int *done,
                       unsigned *bins, double *cut, const IterState *s, double *h_trace, hipStream_t st)
{
    if (n <= 0) return;
    if (red_blocks(n) == 1) {
        select_small_kernel<<<1, kBlock, 0, st>>>(keys, n, rank, state, done, cut, s, h_trace);
        return;
    }
    for (int pass = 0; pass < kSelectPasses; ++pass) {
        launch_select_count(keys, n, pass, state, done, bins, st);
        launch_select_pick(bins, nullptr, pass, rank, state, done, cut, s, h_trace, st);
    }
}

} // namespace icp
