// icp_voxel.hip — the voxel downsample behind icp_voxel_downsample* (DESIGN §3.13), and the kernel
// of icp_transform_scene.  A cloud's points are binned into cubic cells of side `voxel` on a lattice
// through `lo`; every occupied cell gives one output point, the mean of its points, in ascending
// order of the cell's 64-bit key (include/icp_capi.h states the cell, the key and the mean).
//
//   voxel_box_kernel      per workgroup, the cloud's min / max per axis and a non-finite flag (the
//                         host folds the rows: min and max do not depend on the order)
//   voxel_keys_kernel     per point, c_a = floor((x_a - lo_a) / voxel) in fp64 as written and the
//                         key's two 32-bit words
//   sort_pairs_u32        the engine's stable sort (icp_sort.hip) over the low word, `bits` = what
//                         g_x g_y g_z needs; a key of more than 32 bits takes voxel_gather_kernel (the
//                         high words in the first pass's order) and a second stable pass over them
//   voxel_head_count / voxel_head_scan / voxel_head_place
//                         a sorted position is a run's head when its key differs from the one before
//                         it; the heads of each 1,024-position tile are counted, the counts scanned by
//                         one workgroup (integers: any order), and every head's position written to
//                         start[v], v = its rank -- the compaction; start[n_out] = n
//   voxel_means_kernel    a wave per eight consecutive cells (a grid-stride loop over the cells: the
//                         count stays on the device): a cell of at most eight points is summed by eight
//                         lanes, a longer one by the whole wave, both by the order rule below; the mean
//                         and the count; a cell of more than kVoxelLong points is appended to a list
//   voxel_long_kernel     a workgroup of 16 waves per listed cell: 16 chunks at a time, the same rule
//
// The order rule (the result is a pure function of the input: no floating-point atomics, and the
// sort is stable, so a cell's points come in input order): the cell's points p_0 .. p_{L-1} in
// input order are cut into chunks of kVoxelChunk = 1,024.  In a chunk, lane l of 64 starts from +0
// and adds the chunk's points l, l + 64, l + 128, ... in that order; the 64 lane sums are combined by
// the xor butterfly a_l += a_{l ^ 32}, then 16, 8, 4, 2, 1 (every lane ends with the same bits).  The
// cell's sum starts from +0 and adds the chunk sums in chunk order; the mean is sum / L.  Each axis
// on its own; -ffp-contract=off, IEEE division.  Both kernels call chunk_sum, so a cell's bits do not
// depend on which of them took it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icp_device.h"
#include "icp_kernels.h"

namespace icp {
namespace {

constexpr int kVoxelChunk = 1024;    // points of a chunk of the order rule
constexpr int kVoxelLong = 4096;     // cells of more points go to voxel_long_kernel
constexpr int kVoxelTile = 1024;     // sorted positions per workgroup of the head passes (4 a thread)
constexpr int kVoxelLongWaves = 16;  // waves of a voxel_long_kernel workgroup
constexpr int kVoxelBoxMaxBlocks = 1024;

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

__global__ __launch_bounds__(kBlock) void voxel_box_kernel(const double *__restrict__ aos, int n,
                                                           double *__restrict__ part)
{
    __shared__ double sh[kBlock / 64][8];
    double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    int bad = 0;
    for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kBlock) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = aos[3 * i + a];
            bad |= !isfinite(v);
            mn[a] = v < mn[a] ? v : mn[a];
            mx[a] = v > mx[a] ? v : mx[a];
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double u = __shfl_xor(mn[a], o, 64), w = __shfl_xor(mx[a], o, 64);
            mn[a] = u < mn[a] ? u : mn[a];
            mx[a] = w > mx[a] ? w : mx[a];
        }
        bad |= __shfl_xor(bad, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int a = 0; a < 3; ++a) {
            sh[wave][a] = mn[a];
            sh[wave][3 + a] = mx[a];
        }
        sh[wave][6] = bad ? 1.0 : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int k = threadIdx.x;
        double r = sh[0][k];
        for (int w = 1; w < kBlock / 64; ++w) {
            const double u = sh[w][k];
            r = k < 3 ? (u < r ? u : r) : (u > r ? u : r); // (the flag: a max too)
        }
        part[8 * (size_t)blockIdx.x + k] = r;
    }
}

__global__ __launch_bounds__(kBlock) void voxel_keys_kernel(const double *__restrict__ aos, int n, VoxelGrid vg,
                                                            unsigned *__restrict__ klo, unsigned *__restrict__ khi)
{
    const size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x;
    if (i >= (size_t)n) return;
    long long c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = (long long)floor((aos[3 * i + a] - vg.lo[a]) / vg.voxel);
    const unsigned long long key =
        ((unsigned long long)c[2] * (unsigned long long)vg.g[1] + (unsigned long long)c[1]) * (unsigned long long)vg.g[0] +
        (unsigned long long)c[0];
    klo[i] = (unsigned)key;
    if (khi) khi[i] = (unsigned)(key >> 32);
}

__global__ __launch_bounds__(kBlock) void voxel_gather_kernel(const unsigned *__restrict__ src, const int *__restrict__ order,
                                                              int n, unsigned *__restrict__ dst)
{
    const size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x;
    if (i < (size_t)n) dst[i] = src[order[i]];
}

// sorted position i starts a run: its key differs from position i - 1's.  k1: the sorted words of
// the last pass (the whole key, or its high word); lo / order: the low words by input position and
// the final order (a wide key only, else null)
__device__ __forceinline__ bool voxel_is_head(int i, const unsigned *__restrict__ k1, const unsigned *__restrict__ lo,
                                              const int *__restrict__ order)
{
    if (i == 0) return true;
    if (k1[i] != k1[i - 1]) return true;
    return lo && lo[order[i]] != lo[order[i - 1]];
}

__global__ __launch_bounds__(kBlock) void voxel_head_count_kernel(const unsigned *__restrict__ k1,
                                                                  const unsigned *__restrict__ lo,
                                                                  const int *__restrict__ order, int n,
                                                                  int *__restrict__ bcount)
{
    __shared__ int sh[kBlock / 64];
    const long long base = (long long)blockIdx.x * kVoxelTile + 4 * (int)threadIdx.x;
    int c = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (base + u < n) c += voxel_is_head((int)(base + u), k1, lo, order) ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) bcount[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// exclusive scan of bcount[0 .. nblk) in place, one workgroup; the total to *n_out and the sentinel
// start[total] = n
__global__ __launch_bounds__(1024) void voxel_head_scan_kernel(int *__restrict__ bcount, int nblk, int n,
                                                               int *__restrict__ start, int *__restrict__ n_out)
{
    __shared__ int sh[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblk; b0 += 1024) {
        const int b = b0 + (int)threadIdx.x;
        const int v = b < nblk ? bcount[b] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) { // (Hillis-Steele, inclusive)
            const int t = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        const int c0 = carry;
        if (b < nblk) bcount[b] = c0 + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c0 + sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *n_out = carry;
        start[carry] = n;
    }
}

__global__ __launch_bounds__(kBlock) void voxel_head_place_kernel(const unsigned *__restrict__ k1,
                                                                  const unsigned *__restrict__ lo,
                                                                  const int *__restrict__ order, int n,
                                                                  const int *__restrict__ bcount, int *__restrict__ start)
{
    __shared__ int sh[kBlock / 64];
    const long long base = (long long)blockIdx.x * kVoxelTile + 4 * (int)threadIdx.x;
    bool h[4];
    int c = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        h[u] = base + u < n && voxel_is_head((int)(base + u), k1, lo, order);
        c += h[u] ? 1 : 0;
    }
    // the heads before this thread's in the tile: an inclusive scan over the wave's lanes, then the
    // earlier waves' totals
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int pos = bcount[blockIdx.x] + inc - c;
    for (int w = 0; w < wave; ++w) pos += sh[w];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (h[u]) start[pos++] = (int)(base + u);
}

// the order rule's chunk sum: the sorted positions [s, e) (e - s <= kVoxelChunk) of one cell, by the
// 64 lanes of the calling wave; every lane returns the same three sums
__device__ __forceinline__ void chunk_sum(const double *__restrict__ aos, const int *__restrict__ order, int s, int e,
                                          int lane, double (&a)[3])
{
    a[0] = a[1] = a[2] = 0.0;
    for (int i = s + lane; i < e; i += 64) {
        const size_t j = (size_t)order[i];
        a[0] += aos[3 * j];
        a[1] += aos[3 * j + 1];
        a[2] += aos[3 * j + 2];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] += __shfl_xor(a[k], o, 64);
    }
}

__device__ __forceinline__ void voxel_write(double *__restrict__ out, int *__restrict__ count, int v, int L,
                                            const double (&t)[3])
{
    const double d = (double)L;
    out[3 * (size_t)v] = t[0] / d;
    out[3 * (size_t)v + 1] = t[1] / d;
    out[3 * (size_t)v + 2] = t[2] / d;
    if (count) count[v] = L;
}

// long_list[0]: the number of listed cells (zeroed before the launch), then their ranks
__global__ __launch_bounds__(kBlock) void voxel_means_kernel(const double *__restrict__ aos, const int *__restrict__ order,
                                                             const int *__restrict__ start, const int *__restrict__ n_out,
                                                             double *__restrict__ out, int *__restrict__ count,
                                                             int *__restrict__ long_list)
{
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * (kBlock / 64);
    const int cells = *n_out;
    // A wave takes eight consecutive cells at a time, eight lanes a cell.  A cell of at most eight
    // points is summed by its own eight lanes: lane l holds +0 + p_l (or +0), and the butterfly's
    // stages 4, 2, 1 stay inside the group.  These are the rule's bits: in the 64-lane form the
    // stages 32, 16, 8 would add +0 to a value that is never -0, which changes nothing.  The longer
    // cells of the eight then take the whole wave, one after the other.
    for (long long v0 = 8LL * (blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)); v0 < cells; v0 += 8LL * waves) {
        const int sub = lane & 7;
        const long long vg = v0 + (lane >> 3);
        int s = 0, L = 0;
        if (vg < cells) {
            s = start[vg];
            L = start[vg + 1] - s;
        }
        const bool small = L > 0 && L <= 8;
        double a[3] = {0.0, 0.0, 0.0};
        if (small && sub < L) {
            const size_t j = (size_t)order[s + sub];
            a[0] += aos[3 * j];
            a[1] += aos[3 * j + 1];
            a[2] += aos[3 * j + 2];
        }
#pragma unroll
        for (int o = 4; o >= 1; o >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] += __shfl_xor(a[k], o, 64);
        }
        if (small && sub == 0) {
            const double t[3] = {0.0 + a[0], 0.0 + a[1], 0.0 + a[2]}; // (the cell's sum: +0, then its one chunk)
            voxel_write(out, count, (int)vg, L, t);
        }
        unsigned long long big = __ballot(L > 8);
        while (big) {
            const int src = __ffsll((long long)big) - 1; // (a lane of the group: they all hold the cell's s and L)
            big &= ~(0xffULL << (src & ~7));
            const int v = (int)(v0 + (src >> 3));
            const int bs = __shfl(s, src, 64), bL = __shfl(L, src, 64), be = bs + bL;
            if (bL > kVoxelLong) {
                if (lane == 0) long_list[1 + atomicAdd(long_list, 1)] = v;
                continue;
            }
            double t[3] = {0.0, 0.0, 0.0};
            for (int c = bs; c < be; c += kVoxelChunk) {
                double b[3];
                chunk_sum(aos, order, c, min(be, c + kVoxelChunk), lane, b);
                t[0] += b[0];
                t[1] += b[1];
                t[2] += b[2];
            }
            if (lane == 0) voxel_write(out, count, v, bL, t);
        }
    }
}

__global__ __launch_bounds__(64 * kVoxelLongWaves) void voxel_long_kernel(const double *__restrict__ aos,
                                                                          const int *__restrict__ order,
                                                                          const int *__restrict__ start,
                                                                          double *__restrict__ out, int *__restrict__ count,
                                                                          const int *__restrict__ long_list)
{
    __shared__ double sh[2][kVoxelLongWaves][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int listed = long_list[0];
    for (int k = blockIdx.x; k < listed; k += gridDim.x) {
        const int v = long_list[1 + k];
        const int s = start[v], e = start[v + 1], L = e - s;
        const int nchunk = (L + kVoxelChunk - 1) / kVoxelChunk;
        double t[3] = {0.0, 0.0, 0.0};
        int buf = 0;
        for (int c0 = 0; c0 < nchunk; c0 += kVoxelLongWaves, buf ^= 1) {
            const int c = c0 + wave;
            if (c < nchunk) {
                double a[3];
                const int cs = s + c * kVoxelChunk; // (c * 1,024 < L: no overflow)
                chunk_sum(aos, order, cs, min(e, cs + kVoxelChunk), lane, a);
                if (lane == 0) {
                    sh[buf][wave][0] = a[0];
                    sh[buf][wave][1] = a[1];
                    sh[buf][wave][2] = a[2];
                }
            }
            __syncthreads(); // (the other buffer is the next round's: one barrier a round)
            const int m = min(kVoxelLongWaves, nchunk - c0);
            for (int w = 0; w < m; ++w) { // every thread the same sums, in chunk order
                t[0] += sh[buf][w][0];
                t[1] += sh[buf][w][1];
                t[2] += sh[buf][w][2];
            }
        }
        if (threadIdx.x == 0) voxel_write(out, count, v, L, t);
        __syncthreads(); // (the next cell's first round reuses buffer 0)
    }
}

// icp_transform_scene: the resident scene (SoA, point s the caller's point order[s]; order null: the
// caller's order) moved by transform_point into an AoS array in the caller's order
__global__ __launch_bounds__(kBlock) void transform_to_aos_kernel(const double *__restrict__ x, const double *__restrict__ y,
                                                                  const double *__restrict__ z, int n,
                                                                  const int *__restrict__ order, Xform xf,
                                                                  double *__restrict__ aos)
{
    const size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x;
    if (i >= (size_t)n) return;
    double q0, q1, q2;
    transform_point(xf, x[i], y[i], z[i], q0, q1, q2);
    const size_t j = order ? (size_t)order[i] : i;
    aos[3 * j] = q0;
    aos[3 * j + 1] = q1;
    aos[3 * j + 2] = q2;
}

int blocks_for(int n, int per) { return (int)(((size_t)std::max(n, 1) + per - 1) / per); }

// the scratch's parts, in order (each 256-byte aligned)
struct VoxelScratch {
    unsigned *klo, *khi, *ka, *kb, *kc;
    int *oa, *ob, *bcount, *start, *long_list;
    void *sort_temp;
    size_t sort_bytes, total;
};

VoxelScratch voxel_scratch(void *base, int n)
{
    VoxelScratch s{};
    char *p = (char *)base;
    size_t off = 0;
    const auto take = [&](size_t bytes) {
        char *q = p ? p + off : nullptr;
        off += al256(bytes);
        return q;
    };
    const size_t w = (size_t)std::max(n, 1) * 4;
    s.klo = (unsigned *)take(w);
    s.khi = (unsigned *)take(w);
    s.ka = (unsigned *)take(w);
    s.kb = (unsigned *)take(w);
    s.kc = (unsigned *)take(w);
    s.oa = (int *)take(w);
    s.ob = (int *)take(w);
    s.bcount = (int *)take(((size_t)blocks_for(n, kVoxelTile) + 1) * 4);
    s.start = (int *)take(w + 4);
    s.long_list = (int *)take(((size_t)n / (kVoxelLong + 1) + 2) * 4);
    size_t sb = 0;
    (void)sort_pairs_u32(nullptr, sb, nullptr, nullptr, nullptr, nullptr, std::max(n, 1), 32, nullptr);
    s.sort_bytes = sb;
    s.sort_temp = take(sb);
    s.total = off;
    return s;
}

int bits_for(unsigned long long cells) // the bits of the largest key, cells - 1
{
    int b = 0;
    while (b < 64 && ((cells - 1) >> b) != 0) ++b;
    return b;
}

} // namespace

int voxel_box_blocks(int n) { return std::min(kVoxelBoxMaxBlocks, blocks_for(n, 4 * kBlock)); }

void launch_voxel_box(const double *aos, int n, double *part, hipStream_t st)
{
    voxel_box_kernel<<<voxel_box_blocks(n), kBlock, 0, st>>>(aos, n, part);
}

size_t voxel_scratch_bytes(int n) { return voxel_scratch(nullptr, n).total; }

hipError_t launch_voxel_downsample(const double *aos, int n, const VoxelGrid &vg, void *scratch, size_t bytes,
                                   double *xyz_out, int *count_out, int *n_out_dev, hipStream_t st)
{
    const VoxelScratch s = voxel_scratch(scratch, n);
    if (!scratch || bytes < s.total || n <= 0) return hipErrorInvalidValue;
    // (g_a <= 2^21: the product fits 63 bits)
    const unsigned long long cells = (unsigned long long)vg.g[0] * (unsigned long long)vg.g[1] * (unsigned long long)vg.g[2];
    const int bits = bits_for(cells);
    const bool wide = bits > 32;
    const int nb = blocks_for(n, kBlock);
    voxel_keys_kernel<<<nb, kBlock, 0, st>>>(aos, n, vg, s.klo, wide ? s.khi : nullptr);
    size_t sb = s.sort_bytes;
    hipError_t e = sort_pairs_u32(s.sort_temp, sb, s.klo, s.ka, nullptr, s.oa, n, std::min(bits, 32), st);
    if (e != hipSuccess) return e;
    const unsigned *k1 = s.ka;
    const int *order = s.oa;
    if (wide) { // the high words in the first pass's order, and a second stable pass over them
        voxel_gather_kernel<<<nb, kBlock, 0, st>>>(s.khi, s.oa, n, s.kb);
        e = sort_pairs_u32(s.sort_temp, sb, s.kb, s.kc, s.oa, s.ob, n, bits - 32, st);
        if (e != hipSuccess) return e;
        k1 = s.kc;
        order = s.ob;
    }
    const unsigned *lo = wide ? s.klo : nullptr;
    const int nt = blocks_for(n, kVoxelTile);
    voxel_head_count_kernel<<<nt, kBlock, 0, st>>>(k1, lo, order, n, s.bcount);
    voxel_head_scan_kernel<<<1, 1024, 0, st>>>(s.bcount, nt, n, s.start, n_out_dev);
    voxel_head_place_kernel<<<nt, kBlock, 0, st>>>(k1, lo, order, n, s.bcount, s.start);
    e = hipMemsetAsync(s.long_list, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    // (a wave a cell, eight workgroups a CU's worth of them at the most: the loop strides)
    const int mb = std::min(blocks_for(n, kBlock / 64), 2048);
    voxel_means_kernel<<<mb, kBlock, 0, st>>>(aos, order, s.start, n_out_dev, xyz_out, count_out, s.long_list);
    const int lb = std::min(n / (kVoxelLong + 1), 256);
    if (lb > 0)
        voxel_long_kernel<<<lb, 64 * kVoxelLongWaves, 0, st>>>(aos, order, s.start, xyz_out, count_out, s.long_list);
    return hipGetLastError();
}

void launch_transform_to_aos(const double *x, const double *y, const double *z, int n, const int *order, const Xform &xf,
                             double *aos, hipStream_t st)
{
    if (n <= 0) return;
    transform_to_aos_kernel<<<blocks_for(n, kBlock), kBlock, 0, st>>>(x, y, z, n, order, xf, aos);
}

} // namespace icp
