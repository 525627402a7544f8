// icp_sum.h -- the fixed-order sum rule S of icp_filter.hip (stated at that file's head and in
// include/icp_capi.h's filter section), as the kernel and the level loop that icp_filter.hip (one column)
// and icp_eval.hip (several columns of one length, a launch for all of them) share.  Compiled with
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icp_internal.h"

namespace icp {

constexpr int kFilterChunk = 1024; // terms of a chunk of the sum rule

inline int blocks_for(size_t n, int per) { return (int)((std::max<size_t>(n, 1) + per - 1) / per); }

// level 0 of a pass reads v (with kDev: (v - *mu)^2), a later level the sums of the level before.
// Column blockIdx.y: its terms at v + y * vstride, its chunk sums to part + y * pstride.
template <bool kDev>
__global__ __launch_bounds__(kBlock) void filter_sum_kernel(const double *__restrict__ v, int len, size_t vstride,
                                                            const double *__restrict__ mu, double *__restrict__ part,
                                                            size_t pstride)
{
    v += (size_t)blockIdx.y * vstride;
    part += (size_t)blockIdx.y * pstride;
    const int lane = threadIdx.x & 63;
    const long long chunk = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const long long b = chunk * kFilterChunk;
    if (b >= len) return; // (a whole wave: no barrier below)
    const int e = (int)std::min<long long>(len, b + kFilterChunk);
    const double m = kDev ? *mu : 0.0;
    double a = 0.0;
    for (int i = (int)b + lane; i < e; i += 64) {
        if (kDev) {
            const double d = v[i] - m;
            a += d * d;
        } else {
            a += v[i];
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) part[chunk] = a;
}

// a column's stride in part, and part's doubles for `cols` columns of n terms (two halves)
inline size_t sum_part_stride(size_t n) { return (size_t)blocks_for(n, kFilterChunk) + 1; }
inline size_t sum_part_doubles(size_t n, int cols = 1) { return 2 * (size_t)cols * sum_part_stride(n); }

// The sum rule over the cols columns of v (column c: the n terms at v + c * vstride; kDev: over
// (v - *mu)^2): level after level into the two halves of part (sum_part_doubles); -> the device address
// of column 0's S, column c's at + c * sum_part_stride(n)
template <bool kDev>
const double *sum_levels(const double *v, int n, const double *mu, double *part, hipStream_t st, int cols = 1,
                         size_t vstride = 0)
{
    const size_t pst = sum_part_stride(n), half = (size_t)cols * pst;
    const double *src = v;
    size_t sst = vstride;
    int len = n, level = 0;
    for (;;) { // (at most four levels: len falls by 1,024 a level)
        const int chunks = blocks_for(len, kFilterChunk);
        double *dst = part + (level & 1 ? half : 0);
        const dim3 nb(blocks_for(chunks, kBlock / 64), cols);
        if (level == 0 && kDev) filter_sum_kernel<true><<<nb, kBlock, 0, st>>>(src, len, sst, mu, dst, pst);
        else filter_sum_kernel<false><<<nb, kBlock, 0, st>>>(src, len, sst, nullptr, dst, pst);
        if (chunks == 1) return dst;
        src = dst;
        sst = pst;
        len = chunks;
        ++level;
    }
}

} // namespace icp
