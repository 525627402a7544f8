// icp_unique.hip — the one-to-one rejector's min pass (icp_set_one_to_one): for every model point
// j the smallest d2 over the scene points whose correspondence is j, left in device memory as the
// selection's 64-bit key (select_key, icp_device.h: the keys' unsigned order is the doubles', every
// NaN is all ones), so that the minimum is an unsigned integer minimum:
//   best[j] = min{ key(d2_i) : idx_i = j },   all ones where nobody chose j (the run's memset).
// An integer minimum is associative and commutative, so the table does not depend on the points'
// order or on the schedule, and there is no floating-point atomic.  The moments that follow
// (kept_pairs_pass, icp_kept.h) keep pair i when key(d2_i) == best[idx_i], d2_i recomputed from the
// same p and the stored y with the same expression: the value that was scattered, bit for bit.
//   unique_min_kernel<YIN>   y = m[idx] (stored unless the search wrote it) and d2 = (dx*dx + dy*dy)
//                            + dz*dz as select_keys_kernel has them, then the scatter;
//   unique_min_keys_kernel   with a trim on: the keys pass has stored y and every point's key, and
//                            this pass scatters those (y is gathered once, the key computed once).
// The scatter: a relaxed agent-scope load of best[j] first, and no atomic when the entry is
// already <= the key.  Entries only decrease within a pass, so a skipped atomic would have changed
// nothing: the table is exactly the one every atomic would leave.  Under contention (many points on
// one model point) a point's key is a new minimum only log-many times, and the rest are loads of
// one L2 line.  -DICP_UNIQUE_ALWAYS_ATOMIC builds the form without the skip (tools/unique_probe.py's
// comparison); the table is the same.
// A frozen run (*done) skips both kernels, as the moments do.  Compiled with IEEE semantics like
// icp_gated.hip and icp_select.hip.
#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_kernels.h"

namespace icp {
namespace {

// best[j] = min(best[j], key); j outside the table (no search leaves one) writes nothing
__device__ __forceinline__ void unique_scatter(unsigned long long *__restrict__ best, int nm, int j, unsigned long long key)
{
    if ((unsigned)j >= (unsigned)nm) return;
#ifndef ICP_UNIQUE_ALWAYS_ATOMIC
    if (__hip_atomic_load(best + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
#endif
    (void)__hip_atomic_fetch_min(best + j, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool YIN>
__global__ __launch_bounds__(kBlock) void unique_min_kernel(
    const int *__restrict__ idx, const double4 *__restrict__ m4, const double *__restrict__ px,
    const double *__restrict__ py, const double *__restrict__ pz, int n, double *__restrict__ yx,
    double *__restrict__ yy, double *__restrict__ yz, const int *__restrict__ done,
    unsigned long long *__restrict__ best, int nm, const int *__restrict__ kpos, const double4 *__restrict__ m4kd)
{
    if (*done != 0) return;
    const long long G = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += G) {
        const int j = idx[i];
        double4 m;
        if constexpr (YIN) {
            m = make_double4(yx[i], yy[i], yz[i], 0.0);
        } else {
            m = kpos ? m4kd[kpos[i]] : m4[j];
            yx[i] = m.x;
            yy[i] = m.y;
            yz[i] = m.z;
        }
        const double dx = px[i] - m.x, dy = py[i] - m.y, dz = pz[i] - m.z;
        unique_scatter(best, nm, j, select_key((dx * dx + dy * dy) + dz * dz));
    }
}

__global__ __launch_bounds__(kBlock) void unique_min_keys_kernel(const int *__restrict__ idx,
                                                                 const unsigned long long *__restrict__ keys, int n,
                                                                 const int *__restrict__ done,
                                                                 unsigned long long *__restrict__ best, int nm)
{
    if (*done != 0) return;
    const long long G = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += G) unique_scatter(best, nm, idx[i], keys[i]);
}

} // namespace

void launch_unique_min(const int *idx, const double4 *m4, const double *px, const double *py, const double *pz, int n,
                       double *yx, double *yy, double *yz, const int *done, unsigned long long *best, int nm, hipStream_t st,
                       const int *kpos, const double4 *m4kd, bool y_ready)
{
    if (n <= 0) return;
    if (y_ready)
        unique_min_kernel<true><<<red_blocks(n), kBlock, 0, st>>>(idx, m4, px, py, pz, n, yx, yy, yz, done, best, nm, kpos, m4kd);
    else
        unique_min_kernel<false><<<red_blocks(n), kBlock, 0, st>>>(idx, m4, px, py, pz, n, yx, yy, yz, done, best, nm, kpos, m4kd);
}

void launch_unique_min_keys(const int *idx, const unsigned long long *keys, int n, const int *done, unsigned long long *best,
                            int nm, hipStream_t st)
{
    if (n <= 0) return;
    unique_min_keys_kernel<<<red_blocks(n), kBlock, 0, st>>>(idx, keys, n, done, best, nm);
}

} // namespace icp
