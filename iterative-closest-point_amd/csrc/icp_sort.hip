// icp_sort.hip — the stable LSD radix sort of (u32 key, int value) pairs behind the grid build
// (launch_grid_build: model points by cell id) and the scene's slot order (launch_slot_order_aos,
// launch_query_order, launch_mid_order: queries by Morton cell).  The order it must produce is
// fixed: ascending key, ties in input order -- every search result is independent of it, but the
// slot order decides which queries share a wave, and the grid's cell lists decide the walk order.
//
// rocprim's onesweep (what this replaces, rounds 4-5) spends ~92 us and ~8 buffer fills (~5 us
// each, its look-back state resets) per 2^20-pair sort on gfx950: its tuned tile is 16K items, so a
// pass over 2^20 pairs runs 64 workgroups on a 256-CU chip.  Here each pass is three launches with
// no state to reset:
//   sort_hist_kernel     per 4,096-item tile, the count of each digit (digit-major table hist)
//   sort_rows_kernel     one workgroup per digit: the exclusive scan of the digit's row of hist
//                        (its count in each tile) and the digit's total -- only for tables of more
//                        than kSortPrefixTiles tiles: below, hist is written tile-major and each
//                        scatter workgroup sums the digits' columns itself (the counts of the
//                        earlier tiles, and of all: coalesced reads of an L2-resident table that
//                        grow with ntile^2, so the launch stays for large sorts)
//   sort_scatter_kernel  per tile, each item's stable rank among its tile's items of the same
//                        digit, the tile staged in LDS in digit order, written out in runs at
//                        (scan of the digit totals) + (row prefix) -- the tile's output slots
// A workgroup is W waves (4, 8 or 16: ICP_SORT_WAVES) over one 4,096-item tile, each wave a run of
// 4,096 / W consecutive items in 64 / W rounds; the ranks do not depend on W (stable rank = the
// digit's items in earlier waves' runs + in earlier rounds + in lower lanes).
// Ranks come from wave ballots (the lanes holding the same digit, popcount below the lane) and a
// per-wave running count in LDS, so no atomics and no ordering across workgroups: the result is a
// pure function of the input.  Digits are <= 8 bits: ceil(bits / 8) passes of equal width (the
// grid's 19-21-bit cell ids and the 24-bit Morton keys: three).
// Algorithmic traffic per pass: keys read twice, values once, both written once (20 B per pair).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "icp_kernels.h"

namespace icp {
namespace {

constexpr int kSortTile = 4096;       // items a workgroup: W waves, each a run of 4,096 / W in 64 / W rounds
constexpr int kSortBins = 256;
constexpr int kRowThreads = 256;      // a row of 1,024 tiles (2^22 pairs) in one sweep
constexpr int kSortPrefixTiles = 256; // (default bound of the in-scatter prefix: n <= 2^20)
constexpr int kSortWavesDefault = 16;

// the lanes of this wave whose (valid) digit equals this lane's
__device__ __forceinline__ unsigned long long digit_peers(unsigned d, bool valid, int width)
{
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        if (b < width) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
    }
    return peers;
}

template <int W> __device__ __forceinline__ int tile_item(int tile, int w, int r, int l)
{
    return tile * kSortTile + w * (kSortTile / W) + r * 64 + l;
}

// tile_major: hist[tile][digit] (the in-scatter prefix), else hist[digit][tile] (sort_rows_kernel)
template <int W>
__global__ __launch_bounds__(64 * W) void sort_hist_kernel(const unsigned *__restrict__ keys, int n, int shift,
                                                           int width, int ntile, int tile_major,
                                                           int *__restrict__ hist)
{
    constexpr int kRounds = 64 / W;
    __shared__ int cnt[W][kSortBins];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, tile = blockIdx.x;
    const unsigned mask = (1u << width) - 1u;
    for (int i = tid; i < W * kSortBins; i += 64 * W) (&cnt[0][0])[i] = 0;
    unsigned k[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int i = tile_item<W>(tile, w, r, l);
        k[r] = i < n ? keys[i] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const bool valid = tile_item<W>(tile, w, r, l) < n;
        const unsigned d = (k[r] >> shift) & mask;
        const unsigned long long peers = digit_peers(d, valid, width);
        if (valid && (peers >> l) == 1ull) cnt[w][d] += __popcll(peers); // (the highest peer lane)
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (tid < kSortBins) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) c += cnt[j][tid];
        hist[tile_major ? tile * kSortBins + tid : tid * ntile + tile] = c;
    }
}

__device__ __forceinline__ int wave_incl_scan(int v, int l)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (l >= o) v += u;
    }
    return v;
}

// one workgroup per digit: the exclusive scan of the digit's row of hist (its count in each tile)
// in place, and the row's total -> totals[digit]
__global__ __launch_bounds__(kRowThreads) void sort_rows_kernel(int *__restrict__ hist, int ntile,
                                                                 int *__restrict__ totals)
{
    __shared__ int wsum[kRowThreads / 64];
    __shared__ int carry_s;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    int *row = hist + (size_t)blockIdx.x * ntile;
    int carry = 0;
    for (int base = 0; base < ntile; base += 4 * kRowThreads) {
        const int i = base + 4 * tid;
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < ntile ? row[i + j] : 0;
        const int t = v[0] + v[1] + v[2] + v[3];
        const int incl = wave_incl_scan(t, l);
        if (l == 63) wsum[w] = incl;
        __syncthreads();
        if (w == 0) {
            const int s = l < kRowThreads / 64 ? wsum[l] : 0;
            const int si = wave_incl_scan(s, l);
            if (l < kRowThreads / 64) wsum[l] = si - s;
            if (l == kRowThreads / 64 - 1) carry_s = si;
        }
        __syncthreads();
        int run = carry + wsum[w] + incl - t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < ntile) row[i + j] = run;
            run += v[j];
        }
        carry += carry_s;
        __syncthreads();
    }
    if (tid == 0) totals[blockIdx.x] = carry;
}

// vin == nullptr: the values are the input positions (the first pass of an index sort)
// totals == nullptr: hist is tile-major and holds counts -- each digit's prefix over the earlier
// tiles and its total are summed here: wave w takes the rows of tiles w, w + W, ... (1 KiB each, four
// digits a lane: 16-byte loads, independent, so a whole table of <= 16 W tiles is one round trip),
// the W partial sums meet in LDS (the staging arrays, not yet in use)
template <int W>
__global__ __launch_bounds__(64 * W) void sort_scatter_kernel(const unsigned *__restrict__ kin,
                                                              const int *__restrict__ vin, int n, int shift, int width,
                                                              int ntile, const int *__restrict__ hist,
                                                              const int *__restrict__ totals,
                                                              unsigned *__restrict__ kout, int *__restrict__ vout)
{
    constexpr int kRounds = 64 / W;
    __shared__ unsigned skey[kSortTile];
    __shared__ int sval[kSortTile];
    __shared__ int cnt[W][kSortBins];
    __shared__ int goff[kSortBins];
    static_assert(W * kSortBins <= kSortTile, "the prefix partials fit the staging arrays");
    int *const ppre = (int *)skey, *const ptot = sval; // ([W][kSortBins] each, until the digit step)
    __shared__ int wtot[4], wbase[4];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, tile = blockIdx.x;
    const unsigned mask = (1u << width) - 1u;
    for (int i = tid; i < W * kSortBins; i += 64 * W) (&cnt[0][0])[i] = 0;
    unsigned k[kRounds];
    int v[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int i = tile_item<W>(tile, w, r, l);
        k[r] = i < n ? kin[i] : 0u;
        v[r] = i < n ? (vin ? vin[i] : i) : 0;
    }
    if (!totals) {
        const int4 *rows = (const int4 *)hist;
        int4 pre = make_int4(0, 0, 0, 0), tot = pre;
#pragma unroll 16
        for (int t = w; t < ntile; t += W) {
            const int4 h = rows[t * (kSortBins / 4) + l];
            const int m = t < tile ? -1 : 0;
            tot.x += h.x, tot.y += h.y, tot.z += h.z, tot.w += h.w;
            pre.x += h.x & m, pre.y += h.y & m, pre.z += h.z & m, pre.w += h.w & m;
        }
        ((int4 *)ppre)[w * (kSortBins / 4) + l] = pre;
        ((int4 *)ptot)[w * (kSortBins / 4) + l] = tot;
    }
    __syncthreads();
    // each item's rank among the earlier items of its wave's run holding its digit
    int rank[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const bool valid = tile_item<W>(tile, w, r, l) < n;
        const unsigned d = (k[r] >> shift) & mask;
        const unsigned long long peers = digit_peers(d, valid, width);
        const int below = __popcll(peers & ((1ull << l) - 1ull));
        const int before = cnt[w][d];
        rank[r] = before + below;
        if (valid && (peers >> l) == 1ull) cnt[w][d] = before + below + 1; // (the highest peer lane)
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // thread = digit (the first four waves): the runs' offsets within the tile, the tile's digit
    // starts, the digits' first output slots (the scan of the totals), this tile's output slots
    int c[W], tot = 0, gt = 0, hp = 0, incl = 0, gincl = 0;
    if (tid < kSortBins) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            c[j] = cnt[j][tid];
            tot += c[j];
        }
        if (totals) {
            gt = totals[tid];
            hp = hist[tid * ntile + tile];
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                gt += ptot[j * kSortBins + tid];
                hp += ppre[j * kSortBins + tid];
            }
        }
        incl = wave_incl_scan(tot, l);
        gincl = wave_incl_scan(gt, l);
        if (l == 63) {
            wtot[w] = incl;
            wbase[w] = gincl;
        }
    }
    __syncthreads();
    if (tid < kSortBins) {
        int start = incl - tot, gbase = gincl - gt;
        for (int j = 0; j < w; ++j) {
            start += wtot[j];
            gbase += wbase[j];
        }
        goff[tid] = gbase + hp - start;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            cnt[j][tid] = start;
            start += c[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        if (tile_item<W>(tile, w, r, l) < n) {
            const int p = cnt[w][(k[r] >> shift) & mask] + rank[r];
            skey[p] = k[r];
            sval[p] = v[r];
        }
    }
    __syncthreads();
    const int count = min(kSortTile, n - tile * kSortTile);
#pragma unroll 4
    for (int s = tid; s < count; s += 64 * W) {
        const unsigned key = skey[s];
        const int o = goff[(key >> shift) & mask] + s;
        kout[o] = key;
        vout[o] = sval[s];
    }
}

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// ICP_SORT_WAVES = 4 | 8 | 16: waves a workgroup (read once; 4 is the form before the sweep)
int sort_waves()
{
    static const int w = [] {
        const char *e = getenv("ICP_SORT_WAVES");
        const int v = e ? atoi(e) : 0;
        return v == 4 || v == 8 || v == 16 ? v : kSortWavesDefault;
    }();
    return w;
}

// ICP_SORT_PREFIX = the largest table (tiles) whose prefix the scatter sums itself; 0: every sort
// launches sort_rows_kernel (the form before)
int sort_prefix_tiles()
{
    static const int t = [] {
        const char *e = getenv("ICP_SORT_PREFIX");
        return e ? std::max(0, atoi(e)) : kSortPrefixTiles;
    }();
    return t;
}

template <int W>
void sort_pass(const unsigned *ki, const int *vi, int n, int shift, int wd, int ntile, bool prefix, int *hist,
               int *totals, unsigned *ko, int *vo, hipStream_t st)
{
    sort_hist_kernel<W><<<ntile, 64 * W, 0, st>>>(ki, n, shift, wd, ntile, prefix ? 1 : 0, hist);
    if (!prefix) sort_rows_kernel<<<kSortBins, kRowThreads, 0, st>>>(hist, ntile, totals);
    sort_scatter_kernel<W><<<ntile, 64 * W, 0, st>>>(ki, vi, n, shift, wd, ntile, hist, prefix ? nullptr : totals, ko,
                                                     vo);
}

} // namespace

hipError_t sort_pairs_u32(void *temp, size_t &temp_bytes, const unsigned *k0, unsigned *k1, const int *v0, int *v1,
                          int n, int bits, hipStream_t st)
{
    const int ntile = (std::max(n, 1) + kSortTile - 1) / kSortTile;
    const size_t need = 2 * al256((size_t)std::max(n, 1) * sizeof(int)) + al256((size_t)kSortBins * ntile * sizeof(int)) +
                        al256(kSortBins * sizeof(int));
    if (!temp) {
        temp_bytes = need;
        return hipSuccess;
    }
    if (temp_bytes < need || bits < 0 || bits > 32) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int npass = std::max(1, (bits + 7) / 8); // (bits = 0: one pass of 0-bit digits, a stable copy)
    char *p = (char *)temp;
    unsigned *tk = (unsigned *)p;
    int *tv = (int *)(p + al256((size_t)n * sizeof(int)));
    int *hist = (int *)(p + 2 * al256((size_t)n * sizeof(int)));
    int *totals = (int *)((char *)hist + al256((size_t)kSortBins * ntile * sizeof(int)));
    const int width = (bits + npass - 1) / npass;
    const int W = sort_waves();
    const bool prefix = ntile <= sort_prefix_tiles();
    // ping-pong so that the last pass lands in (k1, v1)
    const unsigned *ki = k0;
    const int *vi = v0;
    for (int pass = 0; pass < npass; ++pass) {
        const bool to_out = ((npass - 1 - pass) & 1) == 0;
        unsigned *ko = to_out ? k1 : tk;
        int *vo = to_out ? v1 : tv;
        const int shift = pass * width, wd = std::min(width, bits - shift);
        if (W == 16) sort_pass<16>(ki, vi, n, shift, wd, ntile, prefix, hist, totals, ko, vo, st);
        else if (W == 8) sort_pass<8>(ki, vi, n, shift, wd, ntile, prefix, hist, totals, ko, vo, st);
        else sort_pass<4>(ki, vi, n, shift, wd, ntile, prefix, hist, totals, ko, vo, st);
        ki = ko;
        vi = vo;
    }
    return hipGetLastError();
}

} // namespace icp
