// icp_engine.hip — the device-resident ICP engine behind include/icp_capi.h.
//
// Replaces the reference's src/GPU layer: GPU::ICP::find_corresponding_opti
// (src/GPU/gpu.cc:52-83), GPU::ICP::find_alignment (gpu.cc:95-151) and the wrappers of
// src/GPU/compute.cu.  Differences in structure (same results):
//  * clouds live in HBM for the context's lifetime (the reference re-allocates and
//    re-uploads the model every call, compute.cu:160);
//  * the NN search is one fused pass + a tiny exact-resolution pass, no N x M matrix
//    (compute.cu:176-203 materialises batch x M fp64 distances);
//  * per iteration only 18 fp64 sums cross PCIe (the reference round-trips whole clouds
//    ~30 times per iteration);
//  * multi-GPU: the scene is sharded across ranks, the sums are all-reduced with RCCL.
// icp_run's loops are icp_run.hip, the normals, the k-NN lists and a cloud's temporary grid icp_cloud.hip;
// what the files share is icp_engine.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "icp_horn.h"
#include "icp_engine.h"

// The one-launch loops' model image: points in the order of a kd split -- a range of more
// than 1,024 points splits at a multiple of 1,024, one of more than 64 at a multiple of 64, one
// of more than 16 at a multiple of 16, each at about its middle along the widest axis of its
// box (nth_element; ties: original index) -- so that every 16-point block, 64-point tile and
// 1,024-point superblock is a kd cell and their boxes barely overlap.  Layout (doubles):
// x[nm] | y[nm] | z[nm] | 64-point blocks x (lo x, lo y, lo z, hi x, hi y, hi z) | int32
// original index per sorted position (packed two per double) | superblocks (16 consecutive
// blocks) x their boxes, the same six doubles | the 64-point blocks' then the 16-point blocks'
// boxes as six floats each, rounded outward (the mid-size kernel's LDS copy).
std::vector<double> icp::persist_model_image(const double *m, size_t nm, size_t *blocks_out)
{
    std::vector<uint32_t> ord(nm);
    for (size_t j = 0; j < nm; ++j) ord[j] = (uint32_t)j;
    std::vector<std::pair<size_t, size_t>> stack{{0, nm}};
    while (!stack.empty()) {
        const auto [lo, hi] = stack.back();
        stack.pop_back();
        const size_t cnt = hi - lo;
        const size_t unit = cnt > 1024 ? 1024 : cnt > 64 ? 64 : cnt > 16 ? 16 : 0;
        if (!unit) continue;
        double bl[3] = {INFINITY, INFINITY, INFINITY}, bh[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t k = lo; k < hi; ++k)
            for (int a = 0; a < 3; ++a) {
                bl[a] = std::min(bl[a], m[3 * ord[k] + a]);
                bh[a] = std::max(bh[a], m[3 * ord[k] + a]);
            }
        int ax = 0;
        for (int a = 1; a < 3; ++a)
            if (bh[a] - bl[a] > bh[ax] - bl[ax]) ax = a;
        const size_t units = (cnt + unit - 1) / unit, mid = lo + unit * ((units + 1) / 2);
        if (mid >= hi) continue; // (one unit: a leaf at this level, split below)
        std::nth_element(ord.begin() + lo, ord.begin() + mid, ord.begin() + hi, [&](uint32_t x, uint32_t y) {
            const double vx = m[3 * x + ax], vy = m[3 * y + ax];
            return vx < vy || (vx == vy && x < y);
        });
        stack.push_back({lo, mid});
        stack.push_back({mid, hi});
    }
    const size_t nb = (nm + 63) / 64;
    const size_t nsb = (nb + 15) / 16, nb16 = (nm + 15) / 16;
    const size_t nf32 = 6 * (nb + nb16);
    std::vector<double> img(3 * nm + 6 * nb + (nm + 1) / 2 + 6 * nsb + (nf32 + 1) / 2);
    int32_t *orig = (int32_t *)(img.data() + 3 * nm + 6 * nb);
    for (size_t k = 0; k < nm; ++k) {
        const size_t j = ord[k];
        for (int a = 0; a < 3; ++a) img[a * nm + k] = m[3 * j + a];
        orig[k] = (int32_t)j;
    }
    for (size_t b = 0; b < nb; ++b) {
        double *box = img.data() + 3 * nm + 6 * b;
        for (int a = 0; a < 3; ++a) {
            box[a] = img[a * nm + 64 * b];
            box[3 + a] = box[a];
        }
        for (size_t k = 64 * b + 1; k < std::min(nm, 64 * b + 64); ++k)
            for (int a = 0; a < 3; ++a) {
                box[a] = std::min(box[a], img[a * nm + k]);
                box[3 + a] = std::max(box[3 + a], img[a * nm + k]);
            }
    }
    double *sbox = img.data() + 3 * nm + 6 * nb + (nm + 1) / 2;
    for (size_t s = 0; s < nsb; ++s) {
        const double *first = img.data() + 3 * nm + 6 * (16 * s);
        for (int a = 0; a < 6; ++a) sbox[6 * s + a] = first[a];
        for (size_t b = 16 * s + 1; b < std::min(nb, 16 * s + 16); ++b) {
            const double *box = img.data() + 3 * nm + 6 * b;
            for (int a = 0; a < 3; ++a) {
                sbox[6 * s + a] = std::min(sbox[6 * s + a], box[a]);
                sbox[6 * s + 3 + a] = std::max(sbox[6 * s + 3 + a], box[3 + a]);
            }
        }
    }
    // fp32 boxes rounded outward: each contains its exact box, so its distance is a lower bound
    float *f32 = (float *)(sbox + 6 * nsb);
    auto down = [](double v) {
        float f = (float)v;
        return (double)f > v ? std::nextafter(f, -INFINITY) : f;
    };
    auto up = [](double v) {
        float f = (float)v;
        return (double)f < v ? std::nextafter(f, INFINITY) : f;
    };
    for (size_t b = 0; b < nb; ++b)
        for (int a = 0; a < 3; ++a) {
            f32[6 * b + a] = down(img[3 * nm + 6 * b + a]);
            f32[6 * b + 3 + a] = up(img[3 * nm + 6 * b + 3 + a]);
        }
    float *f16b = f32 + 6 * nb;
    for (size_t b = 0; b < nb16; ++b)
        for (int a = 0; a < 3; ++a) {
            double lo = img[a * nm + 16 * b], hi = lo;
            for (size_t k = 16 * b + 1; k < std::min(nm, 16 * b + 16); ++k) {
                lo = std::min(lo, img[a * nm + k]);
                hi = std::max(hi, img[a * nm + k]);
            }
            f16b[6 * b + a] = down(lo);
            f16b[6 * b + 3 + a] = up(hi);
        }
    *blocks_out = nb;
    return img;
}

namespace icp {
namespace engine {

int fail(icp_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

#define RCCLCHK(expr)                                                                         \
    do {                                                                                      \
        ncclResult_t r_ = (expr);                                                             \
        if (r_ != ncclSuccess)                                                                \
            return fail(ctx, ICP_E_RCCL, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

std::atomic<long long> live_blocks{0};

// the four arrays at one capacity: all of them anew whenever one is missing or too small, and none
// of them when an allocation fails
int grow_cloud(icp_ctx *ctx, DevCloud &c, size_t n, bool with_f32)
{
    if (c.cap() < n || !c.x || (with_f32 && !c.f)) {
        HIPCHK(c.x.release());
        HIPCHK(c.y.release());
        HIPCHK(c.z.release());
        HIPCHK(c.f.release());
        const size_t m = n ? n : 1;
        int rc = c.x.grow(ctx, m);
        if (rc == ICP_OK) rc = c.y.grow(ctx, m);
        if (rc == ICP_OK) rc = c.z.grow(ctx, m);
        if (rc == ICP_OK) rc = c.f.grow(ctx, m);
        if (rc != ICP_OK) {
            c = DevCloud{};
            return rc;
        }
    }
    c.n = n;
    return ICP_OK;
}

// Clouds up to this many doubles (3 x 64k points, 1.5 MiB) move through the mapped buffer.
constexpr size_t kMappedIo = 3 * 65536;
constexpr int kBundleMinModel = 8192; // models from this size get the bundle filter's images

// `count` (<= 2 x kMappedIo) doubles of the mapped buffer: host pointer (*h) and device pointer
// (*d).  When the buffer is used up it is recycled from the start, after a sync if a kernel
// may still read it.
static int io_take(icp_ctx *ctx, size_t count, double **h, double **d)
{
    if (count > 2 * kMappedIo) // callers gate on this; a larger region would run past the buffer
        return fail(ctx, ICP_E_ARG, "io_take: " + std::to_string(count) + " doubles exceed the mapped buffer");
    if (ctx->io_off + count > ctx->h_io.capacity()) {
        if (ctx->io_pending) HIPCHK(hipStreamSynchronize(ctx->st));
        ctx->io_pending = false;
        ctx->io_off = 0;
        TRY(ctx->h_io.grow(ctx, 2 * kMappedIo));
    }
    *h = ctx->h_io + ctx->io_off;
    *d = ctx->h_io.dev() + ctx->io_off;
    ctx->io_off += count;
    return ICP_OK;
}

// host AoS (3 x n col-major) -> device SoA fp64 (+ centred fp32 copy)
static int upload_cloud(icp_ctx *ctx, DevCloud &c, const double *xyz, size_t n, bool make_f32)
{
    TRY(grow_cloud(ctx, c, n, true));
    if (!n) return ICP_OK;
    if (3 * n <= kMappedIo) { // small: the conversion kernel reads the host copy directly
        double *h, *d;
        TRY(io_take(ctx, 3 * n, &h, &d));
        std::memcpy(h, xyz, sizeof(double) * 3 * n);
        ctx->io_pending = true;
        if (make_f32) {
            launch_aos_to_soa_f32(d, n, c.x, c.y, c.z, ctx->c, c.f, ctx->st);
            LAUNCHCHK("upload_cloud");
            return ICP_OK;
        }
        launch_aos_to_soa(d, n, c.x, c.y, c.z, ctx->st);
    } else {
        TRY(ctx->stage.grow(ctx, 3 * n));
        HIPCHK(hipMemcpyAsync(ctx->stage, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->st));
        launch_aos_to_soa(ctx->stage, n, c.x, c.y, c.z, ctx->st);
    }
    if (make_f32) launch_make_f32(c.x, c.y, c.z, n, ctx->c[0], ctx->c[1], ctx->c[2], c.f, ctx->st);
    LAUNCHCHK("upload_cloud");
    return ICP_OK;
}

int download_cloud(icp_ctx *ctx, const DevCloud &c, size_t n, double *xyz)
{
    if (!n) return ICP_OK;
    if (3 * n <= kMappedIo) { // small: the conversion kernel writes the host copy directly
        double *h, *d;
        TRY(io_take(ctx, 3 * n, &h, &d));
        launch_soa_to_aos(c.x, c.y, c.z, n, d, ctx->st);
        LAUNCHCHK("download_cloud");
        HIPCHK(hipStreamSynchronize(ctx->st));
        ctx->io_pending = false;
        std::memcpy(xyz, h, sizeof(double) * 3 * n);
        return ICP_OK;
    }
    TRY(ctx->stage.grow(ctx, 3 * n));
    launch_soa_to_aos(c.x, c.y, c.z, n, ctx->stage, ctx->st);
    LAUNCHCHK("download_cloud");
    HIPCHK(hipMemcpyAsync(xyz, ctx->stage, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return ICP_OK;
}

// The model's host copy (AoS), downloaded once if set_model did not keep it.
static int model_host_copy(icp_ctx *ctx, const double **out)
{
    if (ctx->model_host.size() != 3 * ctx->nm) {
        ctx->model_host.resize(3 * ctx->nm);
        TRY(download_cloud(ctx, ctx->model, ctx->nm, ctx->model_host.data()));
    }
    *out = ctx->model_host.data();
    return ICP_OK;
}

static int ensure_reduction_space(icp_ctx *ctx)
{
    if (ctx->partials) return ICP_OK;
    TRY(ctx->partials.grow(ctx, (size_t)kRedMaxBlocksCap * kRedMaxK));
    TRY(ctx->sums.grow(ctx, 32));
    TRY(ctx->h_sums.grow(ctx, 32));
    TRY(ctx->h_amb.grow(ctx, 4));
    // NN queue counters: present even for an empty shard (horn_step folds and resets them
    // every iteration, whether or not this rank searched anything)
    TRY(ctx->amb_count.grow(ctx, 4));
    HIPCHK(hipMemsetAsync(ctx->amb_count, 0, sizeof(int) * 4, ctx->st)); // (ordered before the stream's kernels)
    return ICP_OK;
}

// A streaming reduction writes per-workgroup partials, then launch_reduce folds them; a
// single-workgroup pass (small clouds) writes its K sums straight to `out` instead.
double *red_target(icp_ctx *ctx, size_t n, double *out) { return red_blocks(n) == 1 ? out : ctx->partials; }
void red_finish(icp_ctx *ctx, size_t n, int K, double *out)
{
    if (red_blocks(n) > 1) launch_reduce(ctx->partials, red_blocks(n), K, out, ctx->st);
}

// queue of queries the fp32 certificate could not settle (list + window T + counter)
static int ensure_queue(icp_ctx *ctx, size_t n)
{
    if (ctx->amb_list.capacity() >= n && ctx->amb_list) return ICP_OK;
    HIPCHK(ctx->amb_list.release()); // (both or neither)
    HIPCHK(ctx->amb_T.release());
    const size_t m = n ? n : 1;
    int rc = ctx->amb_list.grow(ctx, m);
    if (rc == ICP_OK && (rc = ctx->amb_T.grow(ctx, m)) != ICP_OK) (void)ctx->amb_list.release();
    return rc;
}

static int ensure_bundle(icp_ctx *ctx); // (the bundle filter's images at their first use; below)

// level-1 filter of a certified search: 0 = none (VALU filter only), 1 = f32 MFMA, 2 = f16 MFMA
int level1_kind(const icp_ctx *ctx, size_t n)
{
    if (ctx->nn_variant == ICP_NN_VARIANT_MFMA) return 1;
    if (ctx->nn_variant == ICP_NN_VARIANT_MFMA16) return 2;
    const bool bundle = ctx->nb_pad > 0 || ctx->bundle_pending; // (built, or built at first use)
    if (ctx->nn_variant == ICP_NN_VARIANT_BUNDLE) return bundle ? 3 : 2;
    if (ctx->nn_variant == ICP_NN_VARIANT_VALU || ctx->nn_variant == ICP_NN_VARIANT_GRID) return 0;
    // measured crossover (tools/configs_probe.py, 50-iteration registrations of synthetic n x n
    // pairs): VALU wins at 4,096 (2.4 vs 8.9 ms), the f16 MFMA filter from 8,192 (3.3 vs 3.7
    // ms) and by 2.2-2.6x at bunny / horse size, 8x at 65,536.  Behind the bundle bound
    // (icp_bundle.hip) it is 35x faster again at C4 (0.78 against 27.6 ms per search, the same
    // indices bit for bit) and 14x at a W = 8 shard; the two break even near 40,000 x 40,000
    // (16,384 x 16,384: 73 against 25 us), so the bundle filter takes searches from 2^31 pairs
    // (tools/bundle_probe.py, profiles/r03f/)
    if (n >= 8192 && ctx->nm >= 8192)
        return bundle && (double)n * (double)ctx->nm >= 2147483648.0 ? 3 : 2;
    return 0;
}

// launch_model_stats' scratch, its 16 outputs and their host copy, at the first use
int ensure_model_stats(icp_ctx *ctx)
{
    TRY(ctx->mstat_part.grow(ctx, model_stats_scratch_doubles()));
    TRY(ctx->mstat_out.grow(ctx, 16));
    return ctx->h_mstat.grow(ctx, 16);
}

// a built grid as the kernels take it: its geometry, offsets, points and their fp32 image
GridView grid_view_of(const GridParams &p, const int *start, const double4 *pts, const float4 *pts32)
{
    GridView gv{};
    gv.pts = pts;
    gv.start = start;
    for (int a = 0; a < 3; ++a) {
        gv.g[a] = p.g[a];
        gv.lo[a] = p.lo[a];
        gv.c32[a] = p.c32[a];
    }
    gv.inv_h = p.inv_h;
    gv.pts32 = pts32;
    gv.em32 = p.em32;
    return gv;
}

GridView grid_view(const icp_ctx *ctx)
{
    return grid_view_of(ctx->grid, ctx->g_start, ctx->g_pts, ctx->g_pts32);
}

// Cells a query box may span before the query goes to the brute-force levels.  A box costs
// at most about 2 point evaluations per cell (the grid holds ~2 model points per cell of the
// bounding box; far fewer on surface clouds, whose cells are mostly empty), a brute-force
// fallback nm.  Measured (profiles/r01dr/, cells): horse (48,485 points, 25,840 cells) 1,024 ->
// 6,060 -> 12,000 took the grid variant 3,700 -> 4,277 -> 5,003 it/s and the default 5,560 ->
// 5,977 -> 6,012, with no gain beyond; bunny likewise.  ICP_GRID_BUDGET overrides.
// (n: the points the grid holds.)
int grid_budget_for(size_t n)
{
    if (run_knobs().grid_budget) return run_knobs().grid_budget;
    return (int)std::min<size_t>(std::max<size_t>(kGridBudget, n / 4), (size_t)1 << 16);
}

int grid_budget(const icp_ctx *ctx)
{
    return grid_budget_for(ctx->nm);
}

// The bundle filter's processing order of the n queries in q (a Morton order over the model's
// box, launch_query_order): computed once per cloud -- an icp_run's scene moves rigidly, so its
// first order stays spatially coherent -- and again after set_scene / closest_matrix uploads.
// ICP_BUNDLE_ORDER=0: file order (A/B).
static int query_order(icp_ctx *ctx, const DevCloud &q, size_t n, const int **order)
{
    *order = nullptr;
    if (run_knobs().bundle_order_off) return ICP_OK;
    if (ctx->q_order_src != q.x || ctx->q_order_n != n) {
        TRY(ctx->q_order.grow(ctx, n));
        TRY(ctx->q_pos.grow(ctx, n));
        const size_t bytes = query_order_scratch_bytes((int)n);
        TRY(ctx->q_order_tmp.grow(ctx, bytes));
        if (launch_query_order(q.x, q.y, q.z, (int)n, ctx->m_lo, ctx->m_hi, ctx->q_order_tmp, bytes, ctx->q_order,
                               ctx->st, ctx->q_pos) != 0)
            return fail(ctx, ICP_E_HIP, "query_order: radix sort failed");
        LAUNCHCHK("query_order");
        ctx->q_order_src = q.x;
        ctx->q_order_n = n;
    }
    *order = ctx->q_order;
    return ICP_OK;
}

// icp_run keeps a resident scene of this size in slot order: the bundle filter's Morton order
// over the model's box (launch_query_order), so that its per-query records and the
// certificate's reads and index writes stream in order instead of scattering, and neighbouring
// queries share cells in the grid levels.  The condition depends on the sizes only, not on the
// NN variant, so that every variant runs the same per-point order and the same reductions
// (their trajectories stay bitwise equal); below it (n <= 49,152) the one-launch paths keep
// their own orders.  ICP_SCENE_ORDER=0: file order (A/B).
bool want_slot_order(const icp_ctx *ctx, size_t n)
{
    return !run_knobs().scene_order_off && n > (size_t)kTailMaxBlocks * kBlock && ctx->nm >= (size_t)kBundleMinModel &&
           (double)n * (double)ctx->nm >= 2147483648.0;
}

// A pending scene_revert (set_model while the scene was in slot order): the scene back into
// file order, its fp32 copy around the new model's c
int scene_revert_now(icp_ctx *ctx)
{
    if (!ctx->scene_revert) return ICP_OK;
    DevCloud &P = ctx->scene;
    TRY(grow_cloud(ctx, ctx->s_tmp, P.n, true));
    launch_permute_cloud(ctx->s_order, (int)P.n, 1, P.x, P.y, P.z, nullptr, nullptr, ctx->s_tmp.x, ctx->s_tmp.y,
                         ctx->s_tmp.z, nullptr, nullptr, ctx->st);
    std::swap(ctx->scene, ctx->s_tmp);
    launch_make_f32(ctx->scene.x, ctx->scene.y, ctx->scene.z, ctx->scene.n, ctx->c[0], ctx->c[1], ctx->c[2],
                    ctx->scene.f, ctx->st);
    LAUNCHCHK("scene_to_file_order");
    ctx->scene_slot = false;
    ctx->scene_revert = false;
    ctx->p32_stale = false;
    ctx->sn_slot_valid = false;
    return ICP_OK;
}

// The resident scene (and its correspondences while seeds_valid) into slot order, once per
// uploaded scene: gathered into the second buffer, which then becomes the scene.
int scene_to_slot_order(icp_ctx *ctx)
{
    if (ctx->scene_slot || !ctx->scene.n) return ICP_OK;
    DevCloud &P = ctx->scene;
    const size_t n = P.n;
    TRY(ctx->s_order.grow(ctx, n));
    const size_t bytes = query_order_scratch_bytes((int)n);
    TRY(ctx->q_order_tmp.grow(ctx, bytes));
    if (launch_query_order(P.x, P.y, P.z, (int)n, ctx->m_lo, ctx->m_hi, ctx->q_order_tmp, bytes, ctx->s_order,
                           ctx->st) != 0)
        return fail(ctx, ICP_E_HIP, "scene order: radix sort failed");
    TRY(grow_cloud(ctx, ctx->s_tmp, n, true));
    const bool with_idx = ctx->seeds_valid;
    if (with_idx) TRY(ctx->s_tmp_idx.grow(ctx, n));
    launch_permute_cloud(ctx->s_order, (int)n, 0, P.x, P.y, P.z, P.f, with_idx ? ctx->idx : nullptr, ctx->s_tmp.x,
                         ctx->s_tmp.y, ctx->s_tmp.z, ctx->s_tmp.f, with_idx ? ctx->s_tmp_idx : nullptr, ctx->st);
    LAUNCHCHK("scene_to_slot_order");
    std::swap(ctx->scene, ctx->s_tmp);
    if (with_idx) std::swap(ctx->idx, ctx->s_tmp_idx);
    ctx->scene_slot = true;
    ctx->sn_slot_valid = false;
    return ICP_OK;
}

// u0 in the scene's current order: the caller's, or for a scene in slot order its copy in that
// order, permuted as the scene was (once per order: sn_slot_valid)
int scene_normals_current(icp_ctx *ctx, const DevCloud **out)
{
    *out = &ctx->sn;
    const size_t n = ctx->scene.n;
    if (!ctx->scene_slot || !n) return ICP_OK;
    if (!ctx->sn_slot_valid) {
        TRY(grow_cloud(ctx, ctx->sn_slot, n, false));
        launch_permute_cloud(ctx->s_order, (int)n, 0, ctx->sn.x, ctx->sn.y, ctx->sn.z, nullptr, nullptr, ctx->sn_slot.x,
                             ctx->sn_slot.y, ctx->sn_slot.z, nullptr, nullptr, ctx->st);
        LAUNCHCHK("scene_normals_to_slot_order");
        ctx->sn_slot_valid = true;
    }
    *out = &ctx->sn_slot;
    return ICP_OK;
}

constexpr size_t kInlineFallbackModel = 8192; // (16 lanes scan it; a larger model: nn_resolve, 256 per query)

// The seeded grid search of a scene stored in slot order: every query walks the complete box
// around its seed (the previous correspondence) with a few lanes, if it has at most kSeededBox
// cells; the queries with a bigger box go to the resolver with a whole wave each (flattened scan,
// loads in flight: a big box is one query's long chain of dependent loads in the first pass),
// which scans what is over the cell budget over every model point in place.  Every level returns
// the exact first minimum.  With the seed distances (seedd) the passes also write each query's
// correspondence y (the moments stream it); without them kpos is kept when the bundle's kd tables
// exist (the moments then gather from the kd-ordered model).
// The fused iteration's per-row certificate counts of the last run (CertArgs::counts) summed:
// (certified, walked); cert_counts_rows = 0: none pending
static int sum_cert_counts(const icp_ctx *ctx, long long out[2])
{
    out[0] = out[1] = 0;
    if (ctx->cert_counts_rows <= 0 || !ctx->cert_counts) return ICP_OK;
    std::vector<unsigned long long> h(2 * (size_t)ctx->cert_counts_rows);
    if (hipStreamSynchronize(ctx->st) != hipSuccess ||
        hipMemcpy(h.data(), ctx->cert_counts, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost) != hipSuccess)
        return ICP_E_HIP;
    for (size_t r = 0; r < h.size(); r += 2) {
        out[0] += h[r];
        out[1] += h[r + 1];
    }
    return ICP_OK;
}

int fold_cert_counts(icp_ctx *ctx)
{
    long long c[2];
    TRY(sum_cert_counts(ctx, c));
    ctx->stats.run_certified += c[0];
    ctx->stats.run_walked += c[1];
    ctx->cert_counts_rows = 0;
    return ICP_OK;
}

static int grid_seeded_search(icp_ctx *ctx, const DevCloud &q, size_t n, const int *stop, const double *seedd,
                              hipEvent_t ev1)
{
    TRY(ctx->amb1.grow(ctx, n));
    TRY(ctx->amb1_hint.grow(ctx, n));
    TRY(ctx->fb_list.grow(ctx, n));
    TRY(ctx->fb_T.grow(ctx, n));
    int *kpos_out = nullptr;
    // (kd tables of the current model only: nb_pad > 0 -- set_model resets it, and pending bundle
    // images leave the last model's tables in place)
    if (ctx->nn_rule == ICP_NN_RULE_SQUARED && ctx->m4kd && ctx->kd_of && ctx->nb_pad > 0) {
        TRY(ctx->kpos.grow(ctx, n));
        kpos_out = ctx->kpos;
    }
    // (an XCD a contiguous eighth of the slot order: measured faster for sparse shards, slower
    // for a whole scene -- C4 W = 8 shard 36.8 against 41.5 us, W = 1 140 against 126 us, r04k)
    const bool xcd = run_knobs().grid_xcd == 2 || (run_knobs().grid_xcd == 1 && 4 * n <= ctx->nm);
    // with the seed distances (the policy's searches): every level also writes each answered
    // query's correspondence y = m[idx] (the moments then stream y: no gather)
    const DevCloud &Y = ctx->Y;
    const bool y_out = seedd && Y.x && Y.cap() >= n;
    double *yx = y_out ? Y.x : nullptr, *yy = y_out ? Y.y : nullptr, *yz = y_out ? Y.z : nullptr;
    if (y_out) {
        kpos_out = nullptr;
        launch_nn_grid_seeded((int)n, q.x, q.y, q.z, grid_view(ctx), kSeededBox, seedd, ctx->m4, ctx->idx, yx, yy,
                              yz, ctx->amb_count + 2, ctx->amb1, ctx->amb1_hint, stop, xcd, ctx->st,
                              (long long)ctx->nm);
    } else {
        launch_nn_grid_resolve_all((int)n, q.x, q.y, q.z, ctx->m4, grid_view(ctx), kSeededBox, ctx->idx,
                                   ctx->amb_count + 1, ctx->fb_list, ctx->fb_T, ctx->st, stop, 0, xcd,
                                   ctx->amb_count + 2, ctx->amb1, ctx->amb1_hint, kpos_out, ctx->kd_of, seedd);
    }
    if (ev1) HIPCHK(hipEventRecord(ev1, ctx->st)); // (the timed kernel: the pass over every query)
    // the second pass: a whole wave per queued query, grid-striding over the device-side count
    // (sized for a few thousand -- the policy keeps the queue short; a launch of 4,096 idle
    // workgroups cost ~6 us a search, r04q)
    // A box over the budget (grid_budget: 65,536 cells at C4 -- a non-finite query, or one about a
    // model extent away) is scanned in place over every model point by its wave (the exact fp64
    // first minimum), instead of a brute-force launch that nearly always finds nothing to do
    // (~5 us a search)
    // (sized by the queue the host last saw when icp_run's policy runs the search -- at C4 it is
    // empty after the first seeded search (profiles/r04z/far_counts.log): an empty queue then costs
    // ~1.5 us instead of the ~4 us of 1,024 idle workgroups; more queries than the grid's waves
    // are taken in turns)
    const int sp_items = ctx->second_pass_items > 0 ? std::min(ctx->second_pass_items, 4096) : 4096;
    launch_nn_grid_resolve(ctx->amb_count + 2, (int)std::min<size_t>(n, sp_items), ctx->amb1, ctx->amb1_hint, q.x, q.y, q.z, ctx->m4,
                           grid_view(ctx), grid_budget(ctx), ctx->idx, ctx->amb_count + 1, ctx->fb_list, nullptr,
                           ctx->fb_T, ctx->st, stop, (int)ctx->nm, kpos_out, ctx->kd_of, 64, yx, yy, yz);
    LAUNCHCHK("grid_seeded_search");
    static const bool dbg_far = getenv("ICP_DEBUG_FAR") != nullptr; // (diagnostics: synchronises)
    if (dbg_far) {
        int h[4];
        HIPCHK(hipMemcpy(h, ctx->amb_count, sizeof(h), hipMemcpyDeviceToHost));
        fprintf(stderr, "[far] second pass %d fallback %d\n", h[2], h[1]);
    }
    ctx->kpos_valid = kpos_out != nullptr;
    ctx->y_ready = y_out;
    return ICP_OK;
}

// The f16 split image and its norms (the f16 filter's operands, the f16 / bundle finalize's
// certificate) at the first search that reads them: a registration the grid serves from its
// first search never builds them (13 us at C4, profiles/r05h)
static int ensure_mimage16(icp_ctx *ctx)
{
    if (!ctx->mimg16_pending) return ICP_OK;
    TRY(ctx->mimg16.grow(ctx, ctx->nm_pad * 32));
    TRY(ctx->mms16.grow(ctx, ctx->nm_pad));
    launch_build_mimage16(ctx->model.x, ctx->model.y, ctx->model.z, (int)ctx->nm, (int)ctx->nm_pad, ctx->c,
                          ctx->scale16, ctx->mimg16, ctx->mms16, ctx->st);
    LAUNCHCHK("build_mimage16");
    ctx->mimg16_pending = false;
    return ICP_OK;
}

// The fp32 operand images (m32, its MFMA permutation mperm, the norms mm: the fp32 brute-force
// filters and the brute-force resolver) at their first reader, from the resident SoA model -- the
// caller's array is only promised until icp_run returns; the values are the same (one rounded
// subtraction of c, one rounding to fp32, the same padding).  A registration the grid serves from
// its first search never builds them (12 us at C4).
static int ensure_m32(icp_ctx *ctx)
{
    if (!ctx->m32_pending) return ICP_OK;
    TRY(ctx->m32.grow(ctx, ctx->nm_pad));
    TRY(ctx->mperm.grow(ctx, ctx->nm_pad));
    TRY(ctx->mm.grow(ctx, ctx->nm_pad));
    launch_model_f32_images_soa(ctx->model.x, ctx->model.y, ctx->model.z, (int)ctx->nm, (int)ctx->nm_pad, ctx->c,
                                ctx->m32, (float *)ctx->mperm.get(), ctx->mm, ctx->st);
    LAUNCHCHK("model_f32_images");
    ctx->m32_pending = false;
    return ICP_OK;
}

// An unseeded search of a scene in slot order takes the seeded grid pass from cell seeds
// (launch_nn_grid_cell_seed: the first minimum over the query's own cell, or the empty cell's
// stand-in) instead of the ring search (nn_grid_search_kernel: rings of cells until one holds a
// point, then the complete box).  Both end in the exact first minimum over a complete box; the
// seeded pass is the tuned one (its lanes, loads in flight, y written for the moments).
// ICP_CELL_SEED=0: the ring search (A/B).
static int grid_unseeded_slot(icp_ctx *ctx, const DevCloud &q, size_t n, const int *stop, hipEvent_t ev1)
{
    TRY(ctx->b_seedd.grow(ctx, n));
    launch_nn_grid_cell_seed((int)n, q.x, q.y, q.z, grid_view(ctx), (int)ctx->nm, ctx->idx, ctx->b_seedd, ctx->st);
    LAUNCHCHK("nn_grid_cell_seed");
    return grid_seeded_search(ctx, q, n, stop, ctx->b_seedd, ev1);
}

// Launches the complete NN search of the n queries in q against the resident model ->
// ctx->idx, with no host synchronisation: every level is sized on the device.  Queue sizes:
// amb_count [0] queue of the VALU certificate, [1] grid -> fp64 brute-force fallback,
// [2] level-1 (MFMA) queue, [3] level-1 queries without a candidate.  ev0..ev1 brackets the
// O(N*M) kernel.  seeded: ctx->idx holds a previous correspondence of each query (icp_run).
// zero_counts = false: amb_count is already zero (icp_run: horn_step clears it).  ws (nullable):
// what icp_run's previous transform wrote (SeedState); each part is used only if its form is
// the one this search runs, else rebuilt here.
int nn_search_begin(icp_ctx *ctx, const DevCloud &q, size_t n, bool seeded, hipEvent_t ev0, hipEvent_t ev1,
                    bool zero_counts, const SeedState *ws, const int *stop, bool slot_order, bool grid_seeded,
                    const double *seedd)
{
    const SeedState none;
    const SeedState &w = ws ? *ws : none;
    TRY(ctx->idx.grow(ctx, n));
    ctx->kpos_valid = false;
    ctx->y_ready = false;
    if (!n) return ICP_OK;
    int *kpos_out = nullptr; // (the local bundle filter: each writer of idx also writes kpos)
    // small models: the grid resolver scans its rare leftovers exactly in place (no fp64
    // brute-force launch, which would almost always find an empty queue)
    const int inline_nm = ctx->nm <= (size_t)kInlineFallbackModel ? (int)ctx->nm : 0;
    TRY(ensure_queue(ctx, n));
    if (zero_counts) HIPCHK(hipMemsetAsync(ctx->amb_count, 0, sizeof(int) * 4, ctx->st));
    if (ctx->nn_mode == ICP_NN_FP64) {
        ctx->stats.last_filter = ICP_FILTER_FP64;
        const NNPlan pl = plan_nn64(n, ctx->nm);
        const size_t need = (size_t)pl.splits * n * (sizeof(double) + sizeof(int));
        TRY(ctx->part.grow(ctx, need));
        double *pb = (double *)ctx->part.get();
        int *pi = (int *)(pb + (size_t)pl.splits * n);
        if (ev0) HIPCHK(hipEventRecord(ev0, ctx->st));
        launch_nn_fp64(q.x, q.y, q.z, (int)n, ctx->model.x, ctx->model.y, ctx->model.z, (int)ctx->nm,
                       pl, pb, pi, ctx->st, stop);
        if (ev1) HIPCHK(hipEventRecord(ev1, ctx->st));
        launch_nn_finalize64(pb, pi, pl.splits, (int)n, ctx->idx, ctx->st, stop);
        LAUNCHCHK("nn_fp64");
    } else if (seeded && slot_order && (grid_seeded || ctx->nn_variant == ICP_NN_VARIANT_GRID)) {
        // (icp_run's seeded search of a scene in slot order; AUTO takes it by icp_run's policy,
        // icp_run.hip)
        ctx->stats.last_filter = ICP_FILTER_GRID;
        if (ev0) HIPCHK(hipEventRecord(ev0, ctx->st));
        // (seedd: the last transform wrote each point's seed distance -- the policy's searches, and
        // the grid variant's after its first iteration)
        TRY(grid_seeded_search(ctx, q, n, stop, seedd, ev1));
        return ICP_OK;
    } else if (ctx->nn_variant == ICP_NN_VARIANT_GRID) {
        // exact grid search for every query; over-budget boxes -> fp64 brute force per query
        ctx->stats.last_filter = ICP_FILTER_GRID;
        TRY(ctx->fb_list.grow(ctx, n));
        TRY(ctx->fb_T.grow(ctx, n));
        const bool cell_seeds = !seeded && slot_order && run_knobs().cell_seed;
        if (!cell_seeds) TRY(ensure_m32(ctx)); // (launch_nn_resolve below reads m32)
        if (ev0) HIPCHK(hipEventRecord(ev0, ctx->st));
        if (cell_seeds) return grid_unseeded_slot(ctx, q, n, stop, ev1);
        if (seeded) // (icp_run: the previous correspondence is each query's candidate; no ring search)
            launch_nn_grid_resolve_all((int)n, q.x, q.y, q.z, ctx->m4, grid_view(ctx), grid_budget(ctx), ctx->idx,
                                       ctx->amb_count + 1, ctx->fb_list, ctx->fb_T, ctx->st, stop, 0,
                                       slot_order && run_knobs().grid_xcd != 0);
        else
            launch_nn_grid_search((int)n, q.x, q.y, q.z, grid_view(ctx), grid_budget(ctx), ctx->idx,
                                  ctx->amb_count + 1, ctx->fb_list, ctx->fb_T, ctx->st);
        if (ev1) HIPCHK(hipEventRecord(ev1, ctx->st));
        launch_nn_resolve(ctx->amb_count + 1, ctx->fb_list, ctx->fb_T, q.f, q.x, q.y, q.z, ctx->m32,
                          ctx->model.x, ctx->model.y, ctx->model.z, (int)ctx->nm, (int)n, ctx->idx, ctx->st,
                          stop);
        LAUNCHCHK("nn_grid_search");
    } else if (int l1 = level1_kind(ctx, n)) {
        // level 1: MFMA expanded-form filter over every query.  An unseeded f16 search is
        // seeded from the model grid first (a near point per query; ICP_GRID_SEED=0 disables):
        // the full N x M pass then runs the seeded kernel, 35.9 -> ~28 ms at C4
        static const bool grid_seed = [] {
            const char *e = getenv("ICP_GRID_SEED");
            return !(e && atoi(e) == 0);
        }();
        // (the bundle bound needs every query's seed: without the grid, the full f16 pass)
        if (l1 == 3 && !seeded && !(grid_seed && ctx->g_pts)) l1 = 2;
        if (l1 == 3 && !seeded && slot_order && ctx->bundle_pending && ctx->nn_variant == ICP_NN_VARIANT_AUTO) {
            // an icp_run's unseeded first search while the bundle images are still pending: the
            // exact grid search (ring seed, then the complete box), as the grid variant runs it.
            // The run's policy then keeps to the grid until its far count says otherwise, and a
            // registration that stays near the model never builds the bundle images (§3.6)
            ctx->stats.last_filter = ICP_FILTER_GRID;
            TRY(ctx->fb_list.grow(ctx, n));
            TRY(ctx->fb_T.grow(ctx, n));
            if (!run_knobs().cell_seed) TRY(ensure_m32(ctx)); // (launch_nn_resolve below reads m32)
            if (ev0) HIPCHK(hipEventRecord(ev0, ctx->st));
            if (run_knobs().cell_seed) return grid_unseeded_slot(ctx, q, n, stop, ev1);
            launch_nn_grid_search((int)n, q.x, q.y, q.z, grid_view(ctx), grid_budget(ctx), ctx->idx, ctx->amb_count + 1,
                                  ctx->fb_list, ctx->fb_T, ctx->st);
            if (ev1) HIPCHK(hipEventRecord(ev1, ctx->st));
            launch_nn_resolve(ctx->amb_count + 1, ctx->fb_list, ctx->fb_T, q.f, q.x, q.y, q.z, ctx->m32, ctx->model.x,
                              ctx->model.y, ctx->model.z, (int)ctx->nm, (int)n, ctx->idx, ctx->st, stop);
            LAUNCHCHK("nn_grid_search (first)");
            return ICP_OK;
        }
        if (l1 >= 2) TRY(ensure_mimage16(ctx));
        // (the fp32 MFMA filter's mperm and mm; the brute-force resolver's m32)
        if (l1 == 1 || !inline_nm) TRY(ensure_m32(ctx));
        if (l1 == 3 && ctx->bundle_pending && ws) ctx->stats.bundle_builds_in_run += 1; // (icp_run, mid-run)
        if (l1 == 3) TRY(ensure_bundle(ctx)); // (built at their first use)
        const bool gseed = l1 >= 2 && !seeded && grid_seed && ctx->g_pts;
        if (gseed) {
            launch_nn_grid_seed((int)n, q.x, q.y, q.z, grid_view(ctx), (int)ctx->nm, ctx->idx, ctx->st);
            LAUNCHCHK("nn_grid_seed");
        }
        // (gseed: the seeds come from these candidates, below -- nothing the transform wrote)
        const SeedState &wu = gseed ? none : w;
        const bool sd = (seeded || gseed) && l1 >= 2;
        const bool v2 = l1 == 3 && bundle_v2();
        ctx->stats.last_filter = l1 == 3 ? ICP_FILTER_BUNDLE : l1 == 2 ? ICP_FILTER_MFMA16 : ICP_FILTER_MFMA;
        const NNPlan pl = l1 == 3   ? (v2 ? plan_nn_bundle2(n, ctx->nb_pad) : plan_nn_bundle(n, ctx->nb_pad))
                          : l1 == 2 ? plan_nn_mfma16(n, ctx->nm_pad, sd)
                                    : plan_nn_mfma(n, ctx->nm_pad);
        // the local pair test (icp_bundle_rec.h): with the queries in slot order (no scattered
        // records) and the model's block frames built; ICP_BUNDLE_LOCAL=0 keeps the global one
        const bool local = v2 && slot_order && ctx->b_rlmax >= 0.0 && bundle_local();
        // (local: the partials carry kd positions; every writer of idx below then keeps kpos too,
        // unless the CPU rule's host fix-up may rewrite idx after the search)
        if (local && ctx->nn_rule == ICP_NN_RULE_SQUARED && ctx->m4kd) {
            TRY(ctx->kpos.grow(ctx, n));
            kpos_out = ctx->kpos;
        }
        // the transform's records serve only the form this search runs: the local pair test's
        // with the current frames' R (b_rlmax, set by the build of the images), else the global
        // one.  A run that started while the images were pending wrote no records before they
        // were built, and a form written for other images is rebuilt by the prep.
        const bool records_ready = v2 && wu.records && sd &&
                                   (local ? wu.rec_local >= 0.0 && wu.rec_local == ctx->b_rlmax : wu.rec_local < 0.0);
        // seed16 ready in this search's form: the shifts come with local records (else the prep
        // writes them), the f16 seeds from a transform that wrote them
        const bool seeds_ready = local ? records_ready && wu.seed16 == 2 : wu.seed16 == 1;
        if (sd && !seeds_ready) { // (icp_run: the previous iteration's transform wrote them)
            TRY(ctx->seed16.grow(ctx, n));
            if (!local) // (local: the prep writes each query's shift there)
                launch_mfma16_seed(q.x, q.y, q.z, (int)n, ctx->idx, ctx->m4, ctx->c, ctx->scale16, ctx->seed16,
                                   ctx->st);
        }
        const unsigned *seeds = sd ? ctx->seed16 : nullptr;
        TRY(ctx->part.grow(ctx, (size_t)pl.splits * n * (2 * sizeof(float) + sizeof(int))));
        float *pb = (float *)ctx->part.get();
        float *ps = pb + (size_t)pl.splits * n;
        int *pi = (int *)(ps + (size_t)pl.splits * n);
        TRY(ctx->amb1.grow(ctx, n));
        TRY(ctx->amb1_hint.grow(ctx, n));
        TRY(ctx->fb_list.grow(ctx, n));
        TRY(ctx->fb_T.grow(ctx, n));
        const int *order = nullptr;
        // (slot_order: q is the resident scene, already stored in the filter's order)
        if (l1 == 3 && !slot_order) TRY(query_order(ctx, q, n, &order));
        if (v2) { // every query's operands, once, in the filter's slot order
            const size_t nslots = bundle2_slots(pl);
            TRY(ctx->b_qop.grow(ctx, nslots * 64));
            TRY(ctx->b_qraw.grow(ctx, nslots));
            TRY(ctx->b_gop.grow(ctx, nslots));
            TRY(ctx->b_glist.grow(ctx, bundle2_list_ints(pl, ctx->nb_pad)));
            TRY(ctx->b_cand.grow(ctx, (size_t)pl.qblocks * (ctx->nb_pad >> 5)));
            TRY(ctx->b_cand_n.grow(ctx, (size_t)pl.qblocks));
            TRY(ctx->b_wsplit.grow(ctx, (size_t)pl.qblocks));
            TRY(ctx->b_tasks.grow(ctx, bundle2_task_count(pl)));
            if (ctx->b_tctl.capacity() < (size_t)kBundleTctlInts || !ctx->b_tctl) { // (the done counter starts at zero)
                TRY(ctx->b_tctl.grow(ctx, kBundleTctlInts));
                HIPCHK(hipMemsetAsync(ctx->b_tctl, 0, sizeof(int) * kBundleTctlInts, ctx->st));
            }
            TRY(ctx->b_gctr.grow(ctx, nslots / 32));
            if (ctx->b_counters && ctx->b_counters_rows < bundle2_counter_rows(pl)) { // (per-wave rows)
                ctx->b_counters_rows = bundle2_counter_rows(pl);
                TRY(ctx->b_counters.grow(ctx, kBundleCounterFields * ctx->b_counters_rows));
                HIPCHK(hipMemsetAsync(ctx->b_counters, 0,
                                      sizeof(unsigned long long) * kBundleCounterFields * ctx->b_counters_rows,
                                      ctx->st));
            }
            // (wu.seedd: icp_run's previous transform wrote each point's seed distance,
            // SeedArgs::seedd, which the prep would otherwise gather; records_ready: the records
            // and group bounds themselves, SeedArgs::qop)
            if (!records_ready) launch_bundle_prep(q.x, q.y, q.z, (int)n, order ? ctx->q_pos : nullptr, ctx->idx, ctx->m4,
                               sd && wu.seedd && ctx->b_seedd ? ctx->b_seedd : nullptr, ctx->c, ctx->scale16, sd ? ctx->seed16 : nullptr, nslots, ctx->b_qop,
                               order ? ctx->b_qraw : nullptr, ctx->st, stop, order ? nullptr : ctx->b_gop,
                               order ? nullptr : ctx->b_gctr, local ? ctx->b_rlmax : -1.0);
            if (order && !records_ready) launch_bundle_groups(ctx->b_qop, nslots, ctx->b_gop, ctx->b_gctr, ctx->st, stop);
            launch_bundle_candidates(pl, ctx->b_gctr, ctx->b_blk, ctx->nb_pad, ctx->b_cand, ctx->b_cand_n,
                                     ctx->b_wsplit, ctx->b_tasks, ctx->b_tctl, ctx->st, stop);
        }
        if (ev0) HIPCHK(hipEventRecord(ev0, ctx->st));
        if (v2)
            launch_nn_bundle2(ctx->b_qop, ctx->b_gop, (int)n, ctx->b_img, ctx->nb_pad, ctx->b_cand, ctx->b_cand_n,
                              ctx->b_tasks, ctx->b_tctl, local ? ctx->b_pimg_l : ctx->b_pimg, ctx->b_kd_orig,
                              ctx->b_glist, pl, pb, ps, pi, ctx->st, stop, ctx->b_counters,
                              local ? ctx->b_frame : nullptr);
        else if (l1 == 3)
            launch_nn_bundle(q.x, q.y, q.z, (int)n, order, ctx->idx, ctx->m4, ctx->c, ctx->scale16, seeds, ctx->b_img,
                             ctx->nb_pad, ctx->b_pimg, ctx->b_kd_orig, (int)ctx->nm, pl, pb, ps, pi, ctx->st, stop,
                             ctx->b_counters);
        else if (l1 == 2)
            launch_nn_mfma16(q.x, q.y, q.z, (int)n, ctx->c, ctx->scale16, seeds, ctx->mimg16, (int)ctx->nm_pad,
                             pl, pb, ps, pi, ctx->st, stop);
        else
            launch_nn_mfma(q.f, (int)n, ctx->mperm, (int)ctx->nm_pad, pl, pb, ps, pi, ctx->st);
        if (ev1) HIPCHK(hipEventRecord(ev1, ctx->st));
        if (l1 >= 2)
            launch_nn_finalize_mfma16(pb, ps, pi, pl.splits, q.x, q.y, q.z, (int)n, (int)ctx->nm, ctx->c,
                                      ctx->scale16, seeds, ctx->mms16, ctx->idx, ctx->amb_count + 2, ctx->amb1,
                                      ctx->amb1_hint, ctx->st, stop, ctx->m4, ctx->cert_audit,
                                      v2 && order ? ctx->b_qraw : nullptr, // (slot s = query s: p read in order)
                                      v2 ? ctx->b_wsplit : nullptr, v2 ? 4 * pl.q_per_lane * 32 : 0,
                                      local ? ctx->b_rlmax : -1.0, local ? ctx->b_kd_orig : nullptr, kpos_out);
        else
            launch_nn_finalize_mfma(pb, ps, pi, pl.splits, q.f, (int)n, ctx->mm, (int)ctx->nm, ctx->idx, ctx->amb_count + 2,
                                    ctx->amb1, ctx->amb1_hint, ctx->st);
        // exact resolution of the near ties through the model grid, around each candidate;
        // what it cannot take (none at C4): fp64 over every model point, one workgroup each
        launch_nn_grid_resolve(ctx->amb_count + 2, (int)n, ctx->amb1, ctx->amb1_hint, q.x, q.y, q.z, ctx->m4,
                               grid_view(ctx), grid_budget(ctx), ctx->idx, ctx->amb_count + 1, ctx->fb_list, nullptr,
                               ctx->fb_T, ctx->st, stop, inline_nm, kpos_out, ctx->kd_of);
        if (!inline_nm)
            launch_nn_resolve(ctx->amb_count + 1, ctx->fb_list, ctx->fb_T, q.f, q.x, q.y, q.z, ctx->m32,
                              ctx->model.x, ctx->model.y, ctx->model.z, (int)ctx->nm, (int)n, ctx->idx, ctx->st,
                              stop, kpos_out, ctx->kd_of);
        LAUNCHCHK("nn_mfma");
        ctx->kpos_valid = kpos_out != nullptr;
    } else {
        ctx->stats.last_filter = ICP_FILTER_VALU;
        const NNPlan pl = plan_nn32(n, ctx->nm_pad);
        const size_t need = (size_t)pl.splits * n * (2 * sizeof(float) + sizeof(int));
        TRY(ctx->part.grow(ctx, need));
        float *pb = (float *)ctx->part.get();
        float *ps = pb + (size_t)pl.splits * n;
        int *pi = (int *)(ps + (size_t)pl.splits * n);
        TRY(ctx->amb_hint.grow(ctx, n));
        TRY(ctx->fb_list.grow(ctx, n));
        TRY(ctx->fb_T.grow(ctx, n));
        TRY(ensure_m32(ctx)); // (the fp32 filter and the brute-force resolver read m32)
        if (ev0) HIPCHK(hipEventRecord(ev0, ctx->st));
        launch_nn_filter(q.f, (int)n, ctx->m32, (int)ctx->nm_pad, pl, pb, ps, pi, ctx->st, stop);
        if (ev1) HIPCHK(hipEventRecord(ev1, ctx->st));
        CertParams cp{ctx->rm, (int)ctx->nm};
        launch_nn_finalize(pb, ps, pi, pl.splits, q.f, (int)n, cp, ctx->idx, ctx->amb_count, ctx->amb_list,
                           ctx->amb_T, ctx->amb_hint, ctx->st, stop);
        // near ties: exact through the model grid; what it cannot take, fp64 brute force
        // (sized on the device: no host round trip on this path)
        launch_nn_grid_resolve(ctx->amb_count, (int)n, ctx->amb_list, ctx->amb_hint, q.x, q.y, q.z, ctx->m4,
                               grid_view(ctx), grid_budget(ctx), ctx->idx, ctx->amb_count + 1, ctx->fb_list,
                               ctx->amb_T, ctx->fb_T, ctx->st, stop, inline_nm);
        if (!inline_nm)
            launch_nn_resolve(ctx->amb_count + 1, ctx->fb_list, ctx->fb_T, q.f, q.x, q.y, q.z, ctx->m32,
                              ctx->model.x, ctx->model.y, ctx->model.z, (int)ctx->nm, (int)n, ctx->idx, ctx->st,
                              stop);
        LAUNCHCHK("nn_certified");
    }
    return ICP_OK;
}

// queue sizes of the last search -> pinned h_amb (the caller synchronises)
static int nn_counts_to_host(icp_ctx *ctx)
{
    HIPCHK(hipMemcpyAsync(ctx->h_amb, ctx->amb_count, sizeof(int) * 4, hipMemcpyDeviceToHost, ctx->st));
    return ICP_OK;
}

// NN search for the per-operation surface: queues the counts to h_amb; the caller
// synchronises, then calls account_nn.
// searches below this many pairs are not timed: two event markers cost the stream ~9 us
constexpr double kTimedPairs = 4294967296.0;

static int nn_search(icp_ctx *ctx, const DevCloud &q, size_t n)
{
    ctx->last_search_timed = n && (double)n * (double)ctx->nm >= kTimedPairs;
    TRY(nn_search_begin(ctx, q, n, false, ctx->last_search_timed ? ctx->ev[0] : nullptr,
                        ctx->last_search_timed ? ctx->ev[1] : nullptr));
    return n ? nn_counts_to_host(ctx) : ICP_OK;
}

// The reference CPU path's distance (src/cpu.cc:17-19): (pow(dx,2) + pow(dy,2)) + pow(dz,2),
// then sqrt, with libm's pow -- called through a volatile pointer so that the compiler cannot
// turn pow(x, 2.0) into x*x (libm's pow is not always correctly rounded; the reference, built
// without optimisation, calls it: benchmark/callgrind.out.76685).
static double (*volatile g_libm_pow)(double, double) = std::pow;
static double cpu_rule_distance(const double q[3], const double *m)
{
    const double dx = q[0] - m[0], dy = q[1] - m[1], dz = q[2] - m[2];
    const double t = (g_libm_pow(dx, 2.0) + g_libm_pow(dy, 2.0)) + g_libm_pow(dz, 2.0);
    return std::sqrt(t);
}

// ICP_NN_RULE_CPU_SQRT: after a search has left the squared-rule first minimum in idx, find the
// queries with another point inside their near-tie window on the device, evaluate the
// reference's CPU arithmetic on the host for exactly those candidates (minCoeff's first
// minimum, cpu.cc:22), and write the changed correspondences back.  Synchronises the stream.
int cpu_rule_fixup(icp_ctx *ctx, const DevCloud &q, size_t n, const int *stop)
{
    if (ctx->nn_rule != ICP_NN_RULE_CPU_SQRT || n == 0) return ICP_OK;
    TRY(ctx->cr_count.grow(ctx, 1));
    size_t want = std::min<size_t>(n, 4096);
    for (int pass = 0; pass < 2; ++pass) {
        TRY(ctx->cr_entries.grow(ctx, want));
        HIPCHK(hipMemsetAsync(ctx->cr_count, 0, sizeof(int), ctx->st));
        launch_nn_cpu_rule_window((int)n, q.x, q.y, q.z, ctx->m4, grid_view(ctx), grid_budget(ctx), ctx->idx,
                                  ctx->cr_count, ctx->cr_entries, (int)ctx->cr_entries.capacity(), ctx->st, stop);
        LAUNCHCHK("nn_cpu_rule_window");
        int cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, ctx->cr_count, sizeof(int), hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
        if ((size_t)cnt > ctx->cr_entries.capacity()) { // more near ties than entries: once more with room for all
            want = (size_t)cnt;
            continue;
        }
        if (cnt == 0) return ICP_OK;
        std::vector<CpuRuleEntry> h((size_t)cnt);
        HIPCHK(hipMemcpyAsync(h.data(), ctx->cr_entries, sizeof(CpuRuleEntry) * (size_t)cnt,
                              hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
        const double *m = nullptr;
        TRY(model_host_copy(ctx, &m));
        std::vector<int> cand;
        std::vector<int> changed; // (j, best) pairs, sent in one copy and scattered on ctx->st
        for (const CpuRuleEntry &e : h) {
            cand.clear();
            if (e.n >= 0) {
                cand.assign(e.cand, e.cand + e.n);
                std::sort(cand.begin(), cand.end());
            } else { // a window the grid could not bound: every model point, in order
                cand.resize(ctx->nm);
                for (size_t k = 0; k < ctx->nm; ++k) cand[k] = (int)k;
            }
            int best = cand.empty() ? e.h : cand[0];
            double bd = cand.empty() ? 0.0 : cpu_rule_distance(e.q, m + 3 * (size_t)best);
            for (size_t c = 1; c < cand.size(); ++c) {
                const double d = cpu_rule_distance(e.q, m + 3 * (size_t)cand[c]);
                if (d < bd) { // minCoeff: strict, so the lowest index of the minimum
                    bd = d;
                    best = cand[c];
                }
            }
            ctx->stats.cpu_rule_ties += 1;
            if (best != e.h) {
                ctx->stats.cpu_rule_changed += 1;
                changed.push_back(e.j);
                changed.push_back(best);
            }
        }
        if (!changed.empty()) {
            const size_t npairs = changed.size() / 2;
            TRY(ctx->cr_fix.grow(ctx, changed.size()));
            HIPCHK(hipMemcpyAsync(ctx->cr_fix, changed.data(), sizeof(int) * changed.size(), hipMemcpyHostToDevice,
                                  ctx->st));
            launch_scatter_pairs(ctx->cr_fix, (int)npairs, ctx->idx, ctx->st);
            LAUNCHCHK("scatter_pairs");
            HIPCHK(hipStreamSynchronize(ctx->st)); // `changed` is pageable and local
        }
        return ICP_OK;
    }
    return fail(ctx, ICP_E_HIP, "cpu_rule_fixup: the near-tie list kept growing");
}

// after the stream has been synchronised (h_amb holds the last search's final counts): fold
// the NN events and queue sizes into the stats
static void account_nn(icp_ctx *ctx, size_t n)
{
    float ms = 0.f;
    if (ctx->last_search_timed) {
        if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) {
            ctx->stats.nn_ms += ms;
            ctx->stats.nn_launches += 1;
        } else {
            (void)hipGetLastError(); // a failed query must not surface at the next launch check
        }
    }
    ctx->stats.nn_pairs += (long long)n * (long long)ctx->nm;
    if (ctx->nn_mode == ICP_NN_CERTIFIED && n) {
        ctx->stats.ambiguous += ctx->h_amb[0];
        ctx->stats.grid_fallback += ctx->h_amb[1];
        ctx->stats.level1_queued += ctx->h_amb[2];
        ctx->stats.level1_unrecovered += ctx->h_amb[3];
    }
}

// Sum `count` device doubles over the ranks: RCCL on the context stream, or the caller's
// host all-reduce (device -> host, fn, host -> device).
int allreduce(icp_ctx *ctx, double *buf, size_t count)
{
    if (ctx->comm) { // also a 1-rank communicator (icp_ctx_create_dist with world_size 1)
        RCCLCHK(ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, ctx->comm, ctx->st));
        return ICP_OK;
    }
    if (ctx->world <= 1) return ICP_OK;
    if (!ctx->host_reduce) return fail(ctx, ICP_E_ARG, "world_size > 1 without a communicator");
    double few[32];
    std::vector<double> many(count > 32 ? count : 0); // (the selection's bins: kSelectBins doubles)
    double *tmp = count > 32 ? many.data() : few;
    HIPCHK(hipMemcpyAsync(tmp, buf, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (ctx->host_reduce(tmp, count, ctx->host_reduce_user) != 0)
        return fail(ctx, ICP_E_RCCL, "host all-reduce callback failed");
    HIPCHK(hipMemcpyAsync(buf, tmp, sizeof(double) * count, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return ICP_OK;
}

// an int summed over the ranks (several ranks: through the all-reduce; one: as it is), synchronous
int global_count(icp_ctx *ctx, int *v)
{
    if (!ctx->comm && ctx->world <= 1) return ICP_OK;
    double x = (double)*v;
    HIPCHK(hipMemcpyAsync(ctx->sums + kSumFar + 1, &x, sizeof(double), hipMemcpyHostToDevice, ctx->st));
    TRY(allreduce(ctx, ctx->sums + kSumFar + 1, 1));
    HIPCHK(hipMemcpyAsync(&x, ctx->sums + kSumFar + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *v = (int)x;
    return ICP_OK;
}

int check_ready(icp_ctx *ctx, bool need_scene)
{
    if (!ctx) return ICP_E_ARG;
    if (!ctx->has_model || (need_scene && !ctx->has_scene))
        return fail(ctx, ICP_E_NO_MODEL, "model/scene not set (icp_set_model / icp_set_scene)");
    HIPCHK(hipSetDevice(ctx->device));
    return ensure_reduction_space(ctx);
}

// The bundle filter's kd order, images, block frames and kd tables for the resident model (§3.6),
// with kd_h (nullable) a host-built kd order (ICP_KD_HOST).  Synchronous (the frames' max R_B).
// nm: the model's point count -- passed, not read from ctx->nm, which set_model assigns only after
// every image is built (ICP_KD_HOST builds these before that)
static int build_bundle(icp_ctx *ctx, size_t nm, const int *kd_h)
{
    const int nb_pad = bundle_pad(nm);
    TRY(ctx->b_kd.grow(ctx, nm));
    if (kd_h) {
        HIPCHK(hipMemcpyAsync(ctx->b_kd, kd_h, sizeof(int) * nm, hipMemcpyHostToDevice, ctx->st));
    } else {
        kd_plan(nm, ctx->kd_plan); // (ctx-owned: outlives the stream's copy of it)
        TRY(ctx->kd_scratch.grow(ctx, kd_order_scratch_bytes(ctx->kd_plan)));
        if (launch_kd_order(ctx->model.x, ctx->model.y, ctx->model.z, ctx->kd_plan, ctx->kd_scratch,
                            ctx->kd_scratch.capacity(), ctx->b_kd, ctx->st) != 0)
            return fail(ctx, ICP_E_HIP, "the bundle kd order's build failed");
    }
    const size_t nbx = (size_t)nb_pad + 32; // + the null block (icp_bundle.hip)
    TRY(ctx->b_img.grow(ctx, nbx * 32));
    TRY(ctx->b_pimg.grow(ctx, nbx * 1024));
    TRY(ctx->b_kd_orig.grow(ctx, nbx * 32));
    TRY(ctx->b_bctr.grow(ctx, nbx));
    TRY(ctx->b_blk.grow(ctx, nbx / 32));
    launch_build_bundle_images(ctx->model.x, ctx->model.y, ctx->model.z, (int)nm, ctx->b_kd, nb_pad, ctx->c,
                               ctx->scale16, ctx->b_img, ctx->b_pimg, ctx->b_kd_orig, ctx->b_bctr, ctx->b_blk, ctx->st);
    LAUNCHCHK("build_bundle_images");
    // the local pair test's image and block frames, and max R_B (the certificate's R)
    const size_t nfr = nbx / 32;
    TRY(ctx->b_pimg_l.grow(ctx, nbx * 1024));
    TRY(ctx->b_frame.grow(ctx, nfr));
    launch_build_local_images(ctx->model.x, ctx->model.y, ctx->model.z, (int)nm, ctx->b_kd, nb_pad, ctx->c,
                              ctx->scale16, ctx->b_pimg_l, ctx->b_frame, ctx->st);
    LAUNCHCHK("build_local_images");
    TRY(ctx->m4kd.grow(ctx, nm));
    TRY(ctx->kd_of.grow(ctx, nm));
    launch_build_kd_tables(ctx->m4, ctx->b_kd_orig, (int)nm, ctx->m4kd, ctx->kd_of, ctx->st);
    LAUNCHCHK("build_kd_tables");
    std::vector<float4> fr(nfr);
    HIPCHK(hipMemcpyAsync(fr.data(), ctx->b_frame, sizeof(float4) * nfr, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    double rl = 0.0;
    for (const float4 &f : fr) rl = std::max(rl, (double)f.w);
    ctx->b_rlmax = rl;
    ctx->nb_pad = nb_pad;
    ctx->bundle_pending = false;
    ctx->stats.bundle_builds += 1;
    return ICP_OK;
}

// the bundle filter's images, built now if they are pending (the first search that needs them)
static int ensure_bundle(icp_ctx *ctx)
{
    return ctx->bundle_pending ? build_bundle(ctx, ctx->nm, nullptr) : ICP_OK;
}

// moments of one iteration, all on the device: Y = m[idx]; sum p, sum y [all-reduce 6];
// centred S, d_caps, sp around the all-reduced centroids [all-reduce 11]
int moments_phase(icp_ctx *ctx, size_t n)
{
    const DevCloud &P = ctx->scene, &Y = ctx->Y;
    launch_gather_moments(ctx->idx, ctx->m4, P.x, P.y, P.z, (int)n, Y.x, Y.y, Y.z, red_target(ctx, n, ctx->sums + kSumP),
                          ctx->st, ctx->kpos_valid ? ctx->kpos : nullptr, ctx->m4kd);
    red_finish(ctx, n, 6, ctx->sums + kSumP);
    LAUNCHCHK("moments");
    TRY(allreduce(ctx, ctx->sums + kSumP, 6));
    launch_centred_moments(P.x, P.y, P.z, Y.x, Y.y, Y.z, (int)n, ctx->sums, (double)ctx->np_total, red_target(ctx, n, ctx->sums + kSumS),
                           ctx->st);
    red_finish(ctx, n, 11, ctx->sums + kSumS);
    LAUNCHCHK("centred_moments");
    return allreduce(ctx, ctx->sums + kSumS, 11);
}

} // namespace engine
} // namespace icp

// ===================================================================================
extern "C" {

int icp_device_count(int *count)
{
    if (!count) return ICP_E_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return ICP_OK;
}

static int ctx_init(icp_ctx *ctx)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(ctx, ICP_E_NO_DEVICE, "no HIP device visible");
    if (ctx->device < 0 || ctx->device >= ndev)
        return fail(ctx, ICP_E_NO_DEVICE, "device ordinal out of range");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamCreateWithFlags(&ctx->st, hipStreamNonBlocking));
    // timing-only events: no system-scope fence (an L2 writeback + invalidate per record);
    // data always reaches the host through a stream synchronisation or the mapped flags
    for (auto &e : ctx->ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, ctx->device));
    ctx->n_cu = prop.multiProcessorCount;
    ctx->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
    ctx->lds_per_block = prop.sharedMemPerBlock;
    ctx->stats.last_filter = -1;
    return ensure_reduction_space(ctx);
}

int icp_ctx_create(int device, int nn_mode, icp_ctx **out)
{
    if (!out || (nn_mode != ICP_NN_CERTIFIED && nn_mode != ICP_NN_FP64)) return ICP_E_ARG;
    *out = nullptr;
    icp_ctx *ctx = new icp_ctx();
    ctx->device = device;
    ctx->nn_mode = nn_mode;
    int rc = ctx_init(ctx);
    if (rc != ICP_OK) {
        icp_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return ICP_OK;
}

int icp_rccl_unique_id(void *out128)
{
    if (!out128) return ICP_E_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return ICP_E_RCCL;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(out128, &id, sizeof(id));
    return ICP_OK;
}

int icp_ctx_create_dist(int device, int nn_mode, int rank, int world_size, const void *rccl_id,
                        icp_ctx **out)
{
    if (!out || world_size < 1 || rank < 0 || rank >= world_size ||
        (nn_mode != ICP_NN_CERTIFIED && nn_mode != ICP_NN_FP64) || (world_size > 1 && !rccl_id))
        return ICP_E_ARG;
    *out = nullptr;
    icp_ctx *ctx = new icp_ctx();
    ctx->device = device;
    ctx->nn_mode = nn_mode;
    ctx->rank = rank;
    ctx->world = world_size;
    int rc = ctx_init(ctx);
    if (rc == ICP_OK && rccl_id) { // world_size 1 + an id: a 1-rank communicator (exercises RCCL on one GPU)
        ncclUniqueId id;
        std::memcpy(&id, rccl_id, sizeof(id));
        ncclResult_t r = ncclCommInitRank(&ctx->comm, world_size, id, rank);
        if (r != ncclSuccess) rc = fail(ctx, ICP_E_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    }
    if (rc != ICP_OK) {
        icp_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return ICP_OK;
}

int icp_ctx_create_sharded(int device, int nn_mode, int rank, int world_size, icp_allreduce_fn fn,
                           void *user, icp_ctx **out)
{
    if (!out || world_size < 1 || rank < 0 || rank >= world_size || (world_size > 1 && !fn) ||
        (nn_mode != ICP_NN_CERTIFIED && nn_mode != ICP_NN_FP64))
        return ICP_E_ARG;
    *out = nullptr;
    icp_ctx *ctx = new icp_ctx();
    ctx->device = device;
    ctx->nn_mode = nn_mode;
    ctx->rank = rank;
    ctx->world = world_size;
    ctx->host_reduce = fn;
    ctx->host_reduce_user = user;
    int rc = ctx_init(ctx);
    if (rc != ICP_OK) {
        icp_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return ICP_OK;
}

int icp_set_bundle_counters(icp_ctx *ctx, int enable)
{
    if (!ctx) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (!enable) {
        HIPCHK(ctx->b_counters.release());
        ctx->b_counters_rows = 0;
        return ICP_OK;
    }
    // (rows: one for v1's shared counters, per wave task for v2; sized at the next search)
    if (!ctx->b_counters) {
        ctx->b_counters_rows = 1;
        TRY(ctx->b_counters.grow(ctx, kBundleCounterFields));
    }
    HIPCHK(hipMemsetAsync(ctx->b_counters, 0, kBundleCounterFields * sizeof(unsigned long long) * ctx->b_counters_rows,
                          ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return ICP_OK;
}

int icp_get_bundle_counters(icp_ctx *ctx, uint64_t out[16])
{
    if (!ctx || !out) return ICP_E_ARG;
    for (int k = 0; k < 16; ++k) out[k] = 0;
    if (!ctx->b_counters) return ICP_OK;
    HIPCHK(hipSetDevice(ctx->device));
    constexpr int F = kBundleCounterFields;
    std::vector<unsigned long long> v(F * ctx->b_counters_rows);
    HIPCHK(hipMemcpyAsync(v.data(), ctx->b_counters, sizeof(unsigned long long) * v.size(), hipMemcpyDeviceToHost,
                          ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    for (size_t r = 0; r < ctx->b_counters_rows; ++r) {
        for (int k = 0; k < 9; ++k) out[k] += v[F * r + k];
        for (int k = 9; k < F; ++k) out[k + 1] += v[F * r + k]; // (out[9]: the slowest task)
        const uint64_t t = v[F * r + 3] + v[F * r + 4] + v[F * r + 5] + v[F * r + 6];
        out[9] = std::max<uint64_t>(out[9], t); // the slowest wave task's clock ticks
    }
    return ICP_OK;
}

int icp_get_comm_info(icp_ctx *ctx, int *comm_count, int *comm_rank, char *bus_id, int len)
{
    if (!ctx || !comm_count || !comm_rank || (bus_id && len < 16)) return ICP_E_ARG;
    *comm_count = -1;
    *comm_rank = ctx->rank;
    if (ctx->comm) {
        RCCLCHK(ncclCommCount(ctx->comm, comm_count));
        RCCLCHK(ncclCommUserRank(ctx->comm, comm_rank));
    }
    if (bus_id) HIPCHK(hipDeviceGetPCIBusId(bus_id, len, ctx->device));
    return ICP_OK;
}

void icp_ctx_destroy(icp_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->st) (void)hipStreamSynchronize(ctx->st);
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    for (auto e : ctx->iter_ev) (void)hipEventDestroy(e);
    if (ctx->order_ev) (void)hipEventDestroy(ctx->order_ev);
    if (ctx->mstat_ev) (void)hipEventDestroy(ctx->mstat_ev);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->st) (void)hipStreamDestroy(ctx->st);
    // The members free themselves, here: after the stream was synchronised above (no kernel still
    // uses a block) and with the context's device current (a process may hold contexts on several).
    delete ctx;
}

long long icp_debug_live_buffers(void) { return live_blocks.load(std::memory_order_relaxed); }

const char *icp_last_error(const icp_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int icp_set_nn_variant(icp_ctx *ctx, int variant)
{
    if (!ctx || variant < ICP_NN_VARIANT_AUTO || variant > ICP_NN_VARIANT_BUNDLE) return ICP_E_ARG;
    ctx->nn_variant = variant;
    return ICP_OK;
}

int icp_set_nn_rule(icp_ctx *ctx, int rule)
{
    if (!ctx || (rule != ICP_NN_RULE_SQUARED && rule != ICP_NN_RULE_CPU_SQRT)) return ICP_E_ARG;
    ctx->nn_rule = rule;
    return ICP_OK;
}

int icp_set_run_mode(icp_ctx *ctx, int mode)
{
    if (!ctx || mode < ICP_RUN_AUTO || mode > ICP_RUN_PERSISTENT) return ICP_E_ARG;
    ctx->run_mode = mode;
    return ICP_OK;
}

int icp_set_progress(icp_ctx *ctx, icp_progress_fn fn, void *user)
{
    if (!ctx) return ICP_E_ARG;
    ctx->progress_fn = fn;
    ctx->progress_user = user;
    return ICP_OK;
}

int icp_set_allow_unequal(icp_ctx *ctx, int allow)
{
    if (!ctx) return ICP_E_ARG;
    ctx->allow_unequal = allow != 0;
    return ICP_OK;
}

int icp_set_max_distance(icp_ctx *ctx, double dmax)
{
    if (!ctx || std::isnan(dmax) || dmax < 0.0) return ICP_E_ARG;
    ctx->gate_dmax = std::isinf(dmax) ? 0.0 : dmax; // (0 and +inf: off -- every pair is kept)
    return ICP_OK;
}

int icp_get_inliers(icp_ctx *ctx, uint8_t *mask_out, long long *count_out)
{
    if (!ctx) return ICP_E_ARG;
    if (!ctx->has_scene || !ctx->gate_have)
        return fail(ctx, ICP_E_NO_MODEL, "no gated icp_run since icp_set_scene (icp_set_max_distance)");
    HIPCHK(hipSetDevice(ctx->device));
    if (mask_out && ctx->scene.n) {
        HIPCHK(hipMemcpyAsync(mask_out, ctx->gate_flags, ctx->scene.n, hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
    }
    if (count_out) *count_out = ctx->gate_K;
    return ICP_OK;
}

int icp_get_inlier_trace(icp_ctx *ctx, long long *counts_out, size_t cap)
{
    if (!ctx || (!counts_out && cap)) return ICP_E_ARG;
    if (!ctx->has_scene || !ctx->gate_have)
        return fail(ctx, ICP_E_NO_MODEL, "no gated icp_run since icp_set_scene (icp_set_max_distance)");
    const size_t k = std::min(cap, ctx->gate_ktrace.size());
    if (k) std::memcpy(counts_out, ctx->gate_ktrace.data(), sizeof(long long) * k);
    return (int)ctx->gate_ktrace.size();
}

int icp_set_trim(icp_ctx *ctx, double fraction)
{
    if (!ctx || !(fraction > 0.0) || !(fraction <= 1.0)) return ICP_E_ARG; // (a NaN fails both)
    ctx->trim_fraction = fraction;
    return ICP_OK;
}

int icp_set_one_to_one(icp_ctx *ctx, int on)
{
    if (!ctx || (on != 0 && on != 1)) return ICP_E_ARG;
    ctx->one_to_one = on == 1;
    return ICP_OK;
}

int icp_get_trim_trace(icp_ctx *ctx, double *cut_d2_out, size_t cap)
{
    if (!ctx || (!cut_d2_out && cap)) return ICP_E_ARG;
    if (!ctx->has_scene || !ctx->trim_have)
        return fail(ctx, ICP_E_NO_MODEL, "no trimmed icp_run since icp_set_scene (icp_set_trim)");
    const size_t k = std::min(cap, ctx->trim_ctrace.size());
    if (k) std::memcpy(cut_d2_out, ctx->trim_ctrace.data(), sizeof(double) * k);
    return (int)ctx->trim_ctrace.size();
}

int icp_set_robust(icp_ctx *ctx, int kind, double k)
{
    if (!ctx || kind < ICP_ROBUST_NONE || kind > ICP_ROBUST_CAUCHY) return ICP_E_ARG;
    if (kind == ICP_ROBUST_NONE) { // (k is ignored)
        ctx->robust_kind = kind;
        return ICP_OK;
    }
    const double k2 = k * k; // (fp64, once: what every kernel of the run compares against)
    if (!std::isfinite(k) || !(k > 0.0) || !std::isfinite(k2) || !(k2 > 0.0)) return ICP_E_ARG;
    ctx->robust_kind = kind;
    ctx->robust_k = k;
    ctx->robust_k2 = k2;
    return ICP_OK;
}

int icp_get_robust_trace(icp_ctx *ctx, double *wsum_out, long long *active_out, size_t cap)
{
    if (!ctx) return ICP_E_ARG;
    if (!ctx->has_scene || !ctx->robust_have)
        return fail(ctx, ICP_E_NO_MODEL, "no robust icp_run since icp_set_scene (icp_set_robust)");
    const size_t k = std::min(cap, ctx->robust_wtrace.size());
    if (k && wsum_out) std::memcpy(wsum_out, ctx->robust_wtrace.data(), sizeof(double) * k);
    if (k && active_out) std::memcpy(active_out, ctx->robust_ptrace.data(), sizeof(long long) * k);
    return (int)ctx->robust_wtrace.size();
}

int icp_set_metric(icp_ctx *ctx, int metric)
{
    if (!ctx || (metric != ICP_METRIC_POINT_TO_POINT && metric != ICP_METRIC_POINT_TO_PLANE)) return ICP_E_ARG;
    ctx->metric = metric;
    return ICP_OK;
}

int icp_set_plane_symmetric(icp_ctx *ctx, int on)
{
    if (!ctx || (on != 0 && on != 1)) return ICP_E_ARG;
    ctx->plane_symmetric = on == 1;
    return ICP_OK;
}

int icp_set_plane_to_plane(icp_ctx *ctx, double epsilon)
{
    if (!ctx || !(epsilon >= 0.0 && epsilon <= 1.0)) return ICP_E_ARG; // (false for a NaN)
    ctx->plane_to_plane = epsilon;
    return ICP_OK;
}

// The model's AoS copy -> ctx->stage (pageable host memory: the runtime's staged copy).
static int stage_model(icp_ctx *ctx, const double *m_xyz, size_t nm)
{
    TRY(ctx->stage.grow(ctx, 3 * nm));
    HIPCHK(hipMemcpyAsync(ctx->stage, m_xyz, sizeof(double) * 3 * nm, hipMemcpyHostToDevice, ctx->st));
    return ICP_OK;
}

// ICP_KD_HOST=1: the bundle filter's kd order from the host statement of the rule
// (bundle_kd_order, threaded nth_element) instead of the device build (A/B runs)
static bool kd_host()
{
    static const bool on = [] {
        const char *e = getenv("ICP_KD_HOST");
        return e && atoi(e) == 1;
    }();
    return on;
}

// icp_set_model from the staged AoS copy: every image of the model is built on the device
// (icp_model.hip); the host reads back 13 doubles and, for models that fit the one-launch
// loops (<= 64k points), builds their Morton image.  Nothing of the context changes before the
// model has passed its checks.
// aos_dev (nullable): the model's AoS copy in device memory (icp_set_model_device), else ctx->stage.
// m_xyz: the host copy, for the host-side images (small models, ICP_KD_HOST, the CPU rule)
// stream_ordered (icp_set_model_device_stream): no closing synchronisation when no host buffer
// feeds the device work -- the images are built on the context's stream, which every later call
// uses, and the caller's array is read there (its contract: unchanged until icp_run returns)
static int set_model_staged(icp_ctx *ctx, const double *m_xyz, size_t nm, const double *aos_dev = nullptr,
                            bool stream_ordered = false)
{
    const double *aos = aos_dev ? aos_dev : ctx->stage;
    TRY(ensure_model_stats(ctx));
    // 1. sum, box, finiteness; the centring point c = the model's centroid (any c is valid for
    // the certificate; the centroid keeps |coordinates| and hence the fp32 error bound small)
    launch_model_stats(aos, (int)nm, ctx->mstat_part, ctx->mstat_out, ctx->st);
    LAUNCHCHK("model_stats");
    HIPCHK(hipMemcpyAsync(ctx->h_mstat, ctx->mstat_out, sizeof(double) * 10, hipMemcpyDeviceToHost, ctx->st));
    if (!ctx->mstat_ev) HIPCHK(hipEventCreateWithFlags(&ctx->mstat_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ctx->mstat_ev, ctx->st));
    // the SoA fp64 copy and the double4 rows need no statistic: built into the spare buffers while
    // the host waits for the checks (the wait was an idle gap of ~20 us at C4), swapped in below
    TRY(grow_cloud(ctx, ctx->model_alt, nm, true));
    TRY(ctx->m4_alt.grow(ctx, nm));
    launch_aos_to_soa4(aos, nm, ctx->model_alt.x, ctx->model_alt.y, ctx->model_alt.z, ctx->m4_alt, ctx->st);
    LAUNCHCHK("aos_to_soa4");
    HIPCHK(hipEventSynchronize(ctx->mstat_ev)); // (the checks only: the copy above runs on)
    if (ctx->h_mstat[9] != 0.0) return fail(ctx, ICP_E_RANGE, "model has non-finite coordinates");
    double c[3], lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        c[k] = ctx->h_mstat[k] / (double)nm;
        lo[k] = ctx->h_mstat[3 + k];
        hi[k] = ctx->h_mstat[6 + k];
    }
    // 2. the fp32 range around c (the certificate's rm: max |fl32(m - c)|) and the fp64 one (the
    // f16 image's scale: max |m - c|), over every point and axis.  Both are monotone in each
    // coordinate (one rounded subtraction, then a rounding to fp32), so their maxima are taken at
    // the box's faces: lo and hi give exactly the values a pass over the points would (the pass
    // and its synchronisation before round 5)
    double rm = 0.0, rm64 = 0.0;
    for (int k = 0; k < 3; ++k)
        for (const double v : {lo[k], hi[k]}) {
            const double d = v - c[k];
            const float f = (float)d;
            if (!std::isfinite(f)) return fail(ctx, ICP_E_RANGE, "model has non-finite coordinates");
            rm = std::max(rm, std::fabs((double)f));
            rm64 = std::max(rm64, std::fabs(d));
        }
    if (rm > 1e15) return fail(ctx, ICP_E_RANGE, "model coordinates exceed 1e15 around the centroid");
    ctx->has_model = false; // (until every image below is built)
    ctx->has_normals = false; // (the normals belong to the model they were given for)
    for (int k = 0; k < 3; ++k) ctx->c[k] = c[k];
    ctx->rm = rm;
    // 3. the images: SoA fp64, the centred fp32 copy padded to whole LDS tiles with far points
    // and its MFMA operand order, the f16 split image at S = 2^e with max |m - c| S in
    // [2^11, 2^12), the double4 rows, the grid
    const size_t nm_pad = (nm + kTile32 - 1) / kTile32 * kTile32;
    std::swap(ctx->model, ctx->model_alt);
    std::swap(ctx->m4, ctx->m4_alt);
    // ICP_M32_LAZY=0 (A/B, read once): the fp32 images here, from the uploaded copy; else at
    // their first reader (ensure_m32)
    static const bool m32_lazy = [] {
        const char *e = getenv("ICP_M32_LAZY");
        return !(e && atoi(e) == 0);
    }();
    ctx->m32_pending = m32_lazy;
    if (!m32_lazy) {
        TRY(ctx->m32.grow(ctx, nm_pad));
        TRY(ctx->mperm.grow(ctx, nm_pad));
        TRY(ctx->mm.grow(ctx, nm_pad));
        launch_model_f32_images(aos, (int)nm, (int)nm_pad, ctx->c, ctx->m32, (float *)ctx->mperm.get(), ctx->mm, ctx->st);
        LAUNCHCHK("model_f32_images");
    }
    ctx->scale16 = rm64 > 0.0 ? std::ldexp(1.0, (int)std::floor(std::log2(4096.0 / rm64))) : 1.0;
    while (rm64 * ctx->scale16 >= 4096.0) ctx->scale16 *= 0.5;
    ctx->mimg16_pending = true; // (the f16 image: at the first f16 / bundle search, ensure_mimage16)
    // uniform grid over the fp64 model for the exact resolver (its box: step 1's)
    ctx->grid = grid_params_box(lo, hi, nm);
    const long long ncell = grid_cells(ctx->grid);
    TRY(ctx->g_start.grow(ctx, (size_t)ncell + 1));
    TRY(ctx->g_pts.grow(ctx, nm));
    TRY(ctx->g_pts32.grow(ctx, nm));
    const size_t gbytes = grid_build_scratch_bytes((int)nm, ncell);
    TRY(ctx->g_sort.grow(ctx, gbytes));
    if (launch_grid_build(ctx->model.x, ctx->model.y, ctx->model.z, ctx->m4, (int)nm, ctx->grid, ctx->g_sort, gbytes,
                          ctx->g_start, ctx->g_pts, ctx->g_pts32, ctx->st) != 0)
        return fail(ctx, ICP_E_HIP, "grid build: radix sort failed");
    LAUNCHCHK("grid_build");
    for (int k = 0; k < 3; ++k) { // the model's box (the query orders: mid-size loop, bundle filter)
        ctx->m_lo[k] = lo[k];
        ctx->m_hi[k] = hi[k];
    }
    ctx->nb_pad = 0;
    ctx->b_rlmax = -1.0;
    std::vector<int> kd_h; // (ICP_KD_HOST: alive until the closing sync)
    ctx->bundle_pending = false;
    if (nm >= (size_t)kBundleMinModel) { // the bundle filter's kd images (icp_bundle.hip): at first use
        if (kd_host()) {
            kd_h = bundle_kd_order(m_xyz, nm); // (the host build needs the caller's array: now)
            TRY(build_bundle(ctx, nm, kd_h.data()));
        } else {
            ctx->bundle_pending = true;
        }
    }
    std::vector<double> pm;
    if (nm <= (size_t)std::max(kPersistMaxModel, kPersistMidMaxModel)) { // the one-launch loops' model image
        pm = persist_model_image(m_xyz, nm, &ctx->pm_blocks);
        TRY(ctx->pm_img.grow(ctx, pm.size()));
        HIPCHK(hipMemcpyAsync(ctx->pm_img, pm.data(), sizeof(double) * pm.size(), hipMemcpyHostToDevice, ctx->st));
        { // the mid-size search's stale-seed scale: a move beyond 2 diagonals of a median 16-point block
            const size_t nb16 = (nm + 15) / 16;
            std::vector<double> d2(nb16);
            for (size_t b = 0; b < nb16; ++b) {
                double acc = 0.0;
                for (int k = 0; k < 3; ++k) {
                    double blo = pm[k * nm + 16 * b], bhi = blo;
                    for (size_t j = 16 * b + 1; j < std::min(nm, 16 * b + 16); ++j) {
                        blo = std::min(blo, pm[k * nm + j]);
                        bhi = std::max(bhi, pm[k * nm + j]);
                    }
                    acc += (bhi - blo) * (bhi - blo);
                }
                d2[b] = acc;
            }
            std::nth_element(d2.begin(), d2.begin() + nb16 / 2, d2.end());
            ctx->pm_seed_big = 4.0 * d2[nb16 / 2];
        }
    }
    if (!stream_ordered || !pm.empty() || !kd_h.empty()) HIPCHK(hipStreamSynchronize(ctx->st));
    if (nm <= (size_t)std::max(kPersistMaxModel, kPersistMidMaxModel) || ctx->nn_rule == ICP_NN_RULE_CPU_SQRT)
        ctx->model_host.assign(m_xyz, m_xyz + 3 * nm);
    else
        std::vector<double>().swap(ctx->model_host);
    ctx->nm = nm;
    ctx->nm_pad = nm_pad;
    ctx->has_model = true;
    ctx->seeds_valid = false;
    ctx->seedd_valid = false;
    // a scene in slot order (the last model's box) goes back to file order before the next run
    // sorts it by the new box (scene_revert_now), as after set_model then set_scene -- the same
    // order, hence the same reductions, whichever call came first.  Not here: a set_scene that
    // replaces it (every registration of the bench) would make the permutation wasted work
    if (ctx->has_scene && ctx->scene.n && ctx->scene_slot) ctx->scene_revert = true;
    // the scene's fp32 copy depends on c: refresh it (a pending revert refreshes it then)
    if (ctx->has_scene && ctx->scene.n && !ctx->scene_revert) {
        launch_make_f32(ctx->scene.x, ctx->scene.y, ctx->scene.z, ctx->scene.n, ctx->c[0], ctx->c[1],
                        ctx->c[2], ctx->scene.f, ctx->st);
        LAUNCHCHK("make_f32");
        ctx->p32_stale = false;
        if (!stream_ordered) HIPCHK(hipStreamSynchronize(ctx->st));
    }
    return ICP_OK;
}

int icp_set_model(icp_ctx *ctx, const double *m_xyz, size_t nm)
{
    if (!ctx || (!m_xyz && nm) || nm == 0) return ICP_E_ARG;
    if (nm > (size_t)0x7fffffff - kTile32) return fail(ctx, ICP_E_ARG, "model too large");
    HIPCHK(hipSetDevice(ctx->device));
    TRY(stage_model(ctx, m_xyz, nm));
    return set_model_staged(ctx, m_xyz, nm);
}

// a host copy of the model is needed only for the host-side images: the one-launch loops' model
// image (small models), the host kd order (ICP_KD_HOST) and the CPU rule's host fix-up
static bool model_needs_host(const icp_ctx *ctx, size_t nm)
{
    return nm <= (size_t)std::max(kPersistMaxModel, kPersistMidMaxModel) || kd_host() ||
           ctx->nn_rule == ICP_NN_RULE_CPU_SQRT;
}

// The caller's device array is read on the context's stream (non-blocking: nothing orders it after
// other streams' work by itself).  producer: the stream whose work so far wrote the array -- the
// context's stream waits for it (an event, no host synchronisation); nullptr (icp_set_*_device):
// every stream of the device, by a device synchronisation.
static int order_after_producer(icp_ctx *ctx, void *producer, bool any_stream)
{
    if (any_stream) {
        HIPCHK(hipDeviceSynchronize());
        return ICP_OK;
    }
    if (!ctx->order_ev) HIPCHK(hipEventCreateWithFlags(&ctx->order_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ctx->order_ev, (hipStream_t)producer));
    HIPCHK(hipStreamWaitEvent(ctx->st, ctx->order_ev, 0));
    return ICP_OK;
}

static int set_model_device_impl(icp_ctx *ctx, const double *m_xyz_dev, size_t nm, void *producer, bool any_stream)
{
    if (!ctx || !m_xyz_dev || nm == 0) return ICP_E_ARG;
    if (nm > (size_t)0x7fffffff - kTile32) return fail(ctx, ICP_E_ARG, "model too large");
    HIPCHK(hipSetDevice(ctx->device));
    TRY(order_after_producer(ctx, producer, any_stream));
    std::vector<double> host; // (only when a host-side image needs the points)
    if (model_needs_host(ctx, nm)) {
        host.resize(3 * nm);
        HIPCHK(hipMemcpyAsync(host.data(), m_xyz_dev, sizeof(double) * 3 * nm, hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
    }
    return set_model_staged(ctx, host.empty() ? nullptr : host.data(), nm, m_xyz_dev, !any_stream);
}

int icp_set_model_device(icp_ctx *ctx, const double *m_xyz_dev, size_t nm)
{
    return set_model_device_impl(ctx, m_xyz_dev, nm, nullptr, true);
}

int icp_set_model_device_stream(icp_ctx *ctx, const double *m_xyz_dev, size_t nm, void *producer)
{
    return set_model_device_impl(ctx, m_xyz_dev, nm, producer, false);
}

int icp_ensure_model(icp_ctx *ctx, const double *m_xyz, size_t nm, int *uploaded)
{
    if (!ctx || !m_xyz || nm == 0) return ICP_E_ARG;
    if (uploaded) *uploaded = 0;
    if (nm > (size_t)0x7fffffff - kTile32) return fail(ctx, ICP_E_ARG, "model too large");
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->has_model && ctx->nm == nm) {
        if (ctx->model_host.size() == 3 * nm) { // the kept host copy compares exactly
            if (std::memcmp(ctx->model_host.data(), m_xyz, sizeof(double) * 3 * nm) == 0) return ICP_OK;
        } else { // a large model: its upload compared bit for bit with the resident copy on the device
            TRY(ctx->cmp_diff.grow(ctx, 1));
            TRY(stage_model(ctx, m_xyz, nm));
            HIPCHK(hipMemsetAsync(ctx->cmp_diff, 0, sizeof(int), ctx->st));
            launch_model_compare(ctx->stage, (int)nm, ctx->model.x, ctx->model.y, ctx->model.z, ctx->cmp_diff,
                                 ctx->st);
            LAUNCHCHK("model_compare");
            int diff = 0;
            HIPCHK(hipMemcpyAsync(&diff, ctx->cmp_diff, sizeof(int), hipMemcpyDeviceToHost, ctx->st));
            HIPCHK(hipStreamSynchronize(ctx->st));
            if (diff == 0) return ICP_OK;
            TRY(set_model_staged(ctx, m_xyz, nm)); // (staged already)
            if (uploaded) *uploaded = 1;
            return ICP_OK;
        }
    }
    TRY(icp_set_model(ctx, m_xyz, nm));
    if (uploaded) *uploaded = 1;
    return ICP_OK;
}

static int set_scene_common(icp_ctx *ctx, size_t np_local, size_t np_total, bool slot);

// The scene's resident copies from its AoS array in device memory (the caller's, or the staged
// upload).  A scene icp_run keeps in slot order (want_slot_order, against the current model) is
// sorted here and gathered straight from the AoS array into the SoA fp64 streams and the fp32
// copy -- one 24-byte read a point, where the run's scene_to_slot_order moves the four SoA
// streams at random (a cache line each: 76 us at C4, profiles/r05h); the order is the same
// (stable sort of the same keys from file order).  Returns whether the scene is in slot order.
static int scene_from_aos(icp_ctx *ctx, const double *aos, size_t n, bool *slot)
{
    *slot = false;
    if (!n) return ICP_OK;
    DevCloud &P = ctx->scene;
    if (ctx->has_model && want_slot_order(ctx, n)) {
        TRY(ctx->s_order.grow(ctx, n));
        const size_t bytes = query_order_scratch_bytes((int)n);
        TRY(ctx->q_order_tmp.grow(ctx, bytes));
        if (launch_slot_order_aos(aos, (int)n, ctx->m_lo, ctx->m_hi, ctx->q_order_tmp, bytes, ctx->s_order, ctx->c,
                                  P.x, P.y, P.z, P.f, ctx->st) != 0)
            return fail(ctx, ICP_E_HIP, "scene order: radix sort failed");
        LAUNCHCHK("scene_slot_order_aos");
        *slot = true;
        return ICP_OK;
    }
    launch_aos_to_soa_f32(aos, n, P.x, P.y, P.z, ctx->c, P.f, ctx->st);
    LAUNCHCHK("scene_from_aos");
    return ICP_OK;
}

int icp_set_scene(icp_ctx *ctx, const double *p_xyz, size_t np_local, size_t np_total)
{
    if (!ctx || (!p_xyz && np_local) || np_local > np_total) return ICP_E_ARG;
    if (np_total > (size_t)0x7fffffff) return fail(ctx, ICP_E_ARG, "scene too large");
    HIPCHK(hipSetDevice(ctx->device));
    TRY(ensure_reduction_space(ctx));
    TRY(grow_cloud(ctx, ctx->Y, np_local, false));
    bool slot = false;
    if (3 * np_local <= kMappedIo) { // small: through the mapped staging buffer (host-copied: the
        // caller's array is free again when this returns)
        TRY(upload_cloud(ctx, ctx->scene, p_xyz, np_local, true));
    } else { // large: a pageable copy into the stage, then as icp_set_scene_device
        TRY(grow_cloud(ctx, ctx->scene, np_local, true));
        TRY(ctx->stage.grow(ctx, 3 * np_local));
        HIPCHK(hipMemcpyAsync(ctx->stage, p_xyz, sizeof(double) * 3 * np_local, hipMemcpyHostToDevice, ctx->st));
        TRY(scene_from_aos(ctx, ctx->stage, np_local, &slot));
        HIPCHK(hipStreamSynchronize(ctx->st));
    }
    return set_scene_common(ctx, np_local, np_total, slot);
}

static int set_scene_device_impl(icp_ctx *ctx, const double *p_xyz_dev, size_t np_local, size_t np_total,
                                 void *producer, bool any_stream)
{
    if (!ctx || (!p_xyz_dev && np_local) || np_local > np_total) return ICP_E_ARG;
    if (np_total > (size_t)0x7fffffff) return fail(ctx, ICP_E_ARG, "scene too large");
    HIPCHK(hipSetDevice(ctx->device));
    if (np_local) TRY(order_after_producer(ctx, producer, any_stream));
    TRY(ensure_reduction_space(ctx));
    TRY(grow_cloud(ctx, ctx->Y, np_local, false));
    TRY(grow_cloud(ctx, ctx->scene, np_local, true));
    bool slot = false;
    TRY(scene_from_aos(ctx, p_xyz_dev, np_local, &slot)); // (the caller's array: no copy)
    // the caller's array is read on the context's stream: done before icp_set_scene_device returns;
    // icp_set_scene_device_stream is stream-ordered (the array unchanged until icp_run returns)
    if (np_local && any_stream) HIPCHK(hipStreamSynchronize(ctx->st));
    return set_scene_common(ctx, np_local, np_total, slot);
}

int icp_set_scene_device(icp_ctx *ctx, const double *p_xyz_dev, size_t np_local, size_t np_total)
{
    return set_scene_device_impl(ctx, p_xyz_dev, np_local, np_total, nullptr, true);
}

int icp_set_scene_device_stream(icp_ctx *ctx, const double *p_xyz_dev, size_t np_local, size_t np_total,
                                void *producer)
{
    return set_scene_device_impl(ctx, p_xyz_dev, np_local, np_total, producer, false);
}

static int set_scene_common(icp_ctx *ctx, size_t np_local, size_t np_total, bool slot)
{
    ctx->np_total = np_total;
    ctx->has_scene = true;
    ctx->tot_n = 0; // (icp_get_transform: the identity)
    ctx->seeds_valid = false;
    ctx->seedd_valid = false;
    ctx->gate_have = false;
    ctx->robust_have = false;
    ctx->trim_have = false;
    ctx->q_order_src = nullptr; // new contents: a new query order
    ctx->scene_slot = slot;     // (else in the caller's order)
    ctx->scene_revert = false;
    ctx->p32_stale = false;
    ctx->has_scene_normals = false; // (the scene's normals belong to the scene they were given for)
    ctx->sn_slot_valid = false;
    ctx->scene_pristine = true;
    // ICP_EAGER_BUNDLE=1: a shard against a model of at least twice its points (C5's 8-way shards)
    // gets the bundle images here instead of at their first use.  Round 4 built them here always:
    // its far rule sent a C5 shard's first searches to the bundle cascade.  With the box rule
    // (icp_run.hip run_setup_policy: the queries whose clamped box the grid walk cannot take) the same shard stays on
    // the grid (0.9% of its points against the n/32 threshold), and a scene that does need the
    // cascade builds the images between two iterations (the same results, tests/test_gpu_lazy_bundle.py).
    // Only for a scene the bundle filter would search (level1_kind == 3, the slot order)
    const char *eager_env = getenv("ICP_EAGER_BUNDLE"); // (read per call: tests toggle it)
    const bool eager = eager_env && eager_env[0] == '1';
    if (eager && ctx->bundle_pending && np_local > 0 && ctx->nm >= 2 * np_local &&
        ctx->nn_variant == ICP_NN_VARIANT_AUTO && ctx->nn_mode == ICP_NN_CERTIFIED && level1_kind(ctx, np_local) == 3 &&
        want_slot_order(ctx, np_local))
        TRY(ensure_bundle(ctx));
    return ICP_OK;
}

int icp_get_scene(icp_ctx *ctx, double *p_xyz_out)
{
    if (!ctx || (!p_xyz_out && ctx->scene.n)) return ICP_E_ARG;
    if (!ctx->has_scene) return fail(ctx, ICP_E_NO_MODEL, "scene not set");
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->scene_slot && ctx->scene.n) { // back to the caller's order, in the second buffer
        const DevCloud &P = ctx->scene;
        TRY(grow_cloud(ctx, ctx->s_tmp, P.n, true));
        launch_permute_cloud(ctx->s_order, (int)P.n, 1, P.x, P.y, P.z, nullptr, nullptr, ctx->s_tmp.x, ctx->s_tmp.y,
                             ctx->s_tmp.z, nullptr, nullptr, ctx->st);
        LAUNCHCHK("scene_to_file_order");
        return download_cloud(ctx, ctx->s_tmp, P.n, p_xyz_out);
    }
    return download_cloud(ctx, ctx->scene, ctx->scene.n, p_xyz_out);
}

// ---- the total transform, a pose for the resident scene, the voxel downsample -----------

int icp_get_transform(icp_ctx *ctx, double *s, double R[9], double t[3])
{
    if (!ctx || !s || !R || !t) return ICP_E_ARG;
    if (!ctx->has_scene) return fail(ctx, ICP_E_NO_MODEL, "icp_get_transform: scene not set");
    *s = 1.0;
    for (int k = 0; k < 9; ++k) R[k] = k % 4 == 0 ? 1.0 : 0.0;
    for (int k = 0; k < 3; ++k) t[k] = 0.0;
    if (ctx->tot_n > 0) {
        *s = ctx->tot[0];
        for (int k = 0; k < 9; ++k) R[k] = ctx->tot[1 + k];
        for (int k = 0; k < 3; ++k) t[k] = ctx->tot[10 + k];
    }
    return ICP_OK;
}

int icp_transform_scene(icp_ctx *ctx, double s, const double R[9], const double t[3])
{
    if (!ctx) return ICP_E_ARG;
    if (!R || !t) return fail(ctx, ICP_E_ARG, "icp_transform_scene: R or t is null");
    bool finite = std::isfinite(s);
    for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(R[k]);
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(t[k]);
    if (!finite) return fail(ctx, ICP_E_ARG, "icp_transform_scene: s, R or t is not finite");
    if (!(s > 0.0)) return fail(ctx, ICP_E_ARG, "icp_transform_scene: s = " + std::to_string(s) + " is not > 0");
    if (!ctx->has_scene) return fail(ctx, ICP_E_NO_MODEL, "icp_transform_scene: scene not set");
    HIPCHK(hipSetDevice(ctx->device));
    double step[13];
    Xform xf{};
    step[0] = s;
    for (int k = 0; k < 9; ++k) {
        step[1 + k] = R[k];
        xf.sR[k] = s * R[k]; // (once, as the Horn step forms it)
    }
    for (int k = 0; k < 3; ++k) {
        step[10 + k] = t[k];
        xf.t[k] = t[k];
        xf.c[k] = ctx->c[k];
    }
    // The moved points, in the caller's order, into the stage; from there the scene is prepared as
    // icp_set_scene prepares an upload of them: the same kernels on the same values, so the slot
    // order, the fp32 copy and every flag are those of a fresh icp_set_scene.
    const size_t n = ctx->scene.n;
    bool slot = false;
    if (n) {
        DevCloud &P = ctx->scene;
        TRY(ctx->stage.grow(ctx, 3 * n));
        launch_transform_to_aos(P.x, P.y, P.z, (int)n, ctx->scene_slot ? ctx->s_order : nullptr, xf, ctx->stage, ctx->st);
        LAUNCHCHK("transform_to_aos");
        if (3 * n <= kMappedIo) {
            launch_aos_to_soa_f32(ctx->stage, n, P.x, P.y, P.z, ctx->c, P.f, ctx->st);
            LAUNCHCHK("transform_scene");
        } else {
            TRY(scene_from_aos(ctx, ctx->stage, n, &slot));
        }
        HIPCHK(hipStreamSynchronize(ctx->st));
    }
    double tot[13];
    const int tot_n = ctx->tot_n;
    const bool normals = ctx->has_scene_normals; // (u0 stays as given: the total turns it)
    std::memcpy(tot, ctx->tot, sizeof(tot));
    TRY(set_scene_common(ctx, n, ctx->np_total, slot));
    std::memcpy(ctx->tot, tot, sizeof(tot));
    ctx->tot_n = tot_n;
    ctx->has_scene_normals = normals;
    ctx->scene_pristine = false;
    compose_srt(step, ctx->tot, &ctx->tot_n);
    return ICP_OK;
}

// the box rows folded: lo / hi per axis; ICP_E_RANGE for a non-finite coordinate (as icp_set_model_device)
static int voxel_box(icp_ctx *ctx, const double *xyz_dev, size_t n, double lo[3], double hi[3])
{
    const int rows = voxel_box_blocks((int)n);
    double *part = (double *)ctx->vox_buf.get(); // (the head of the scratch: read back before the passes write it)
    launch_voxel_box(xyz_dev, (int)n, part, ctx->st);
    LAUNCHCHK("voxel_box");
    std::vector<double> h(8 * (size_t)rows);
    HIPCHK(hipMemcpyAsync(h.data(), part, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    bool bad = false;
    for (int a = 0; a < 3; ++a) {
        lo[a] = h[a];
        hi[a] = h[3 + a];
    }
    for (int r = 0; r < rows; ++r) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], h[8 * (size_t)r + a]);
            hi[a] = std::max(hi[a], h[8 * (size_t)r + 3 + a]);
        }
        bad = bad || h[8 * (size_t)r + 6] != 0.0;
    }
    if (bad) return fail(ctx, ICP_E_RANGE, "icp_voxel_downsample: the cloud has non-finite coordinates");
    return ICP_OK;
}

// both forms, the cloud and the outputs in device memory; *n_out on the host when it returns
static int voxel_downsample_dev(icp_ctx *ctx, const double *xyz_dev, size_t n, double voxel, const double *origin,
                                double *xyz_out_dev, int32_t *count_out_dev, size_t *n_out)
{
    const size_t bytes = std::max(voxel_scratch_bytes((int)n), sizeof(double) * 8 * (size_t)voxel_box_blocks((int)n)) + 256;
    TRY(ctx->vox_buf.grow(ctx, bytes));
    double lo[3], hi[3];
    TRY(voxel_box(ctx, xyz_dev, n, lo, hi));
    VoxelGrid vg{};
    vg.voxel = voxel;
    static const char axis[3] = {'x', 'y', 'z'};
    for (int a = 0; a < 3; ++a) {
        vg.lo[a] = origin ? origin[a] : lo[a];
        // floor((x - lo) / voxel) does not decrease with x: the least and the largest cell of the axis
        const double c_min = std::floor((lo[a] - vg.lo[a]) / voxel), c_max = std::floor((hi[a] - vg.lo[a]) / voxel);
        if (c_min < 0.0)
            return fail(ctx, ICP_E_RANGE, std::string("icp_voxel_downsample: a point's ") + axis[a] + " = " +
                                              std::to_string(lo[a]) + " lies below the origin's " +
                                              std::to_string(vg.lo[a]));
        if (!(c_max + 1.0 <= 2097152.0))
            return fail(ctx, ICP_E_RANGE, std::string("icp_voxel_downsample: the ") + axis[a] + " axis needs " +
                                              std::to_string(c_max + 1.0) + " cells, more than 2^21 (voxel = " +
                                              std::to_string(voxel) + ")");
        vg.g[a] = (long long)c_max + 1;
    }
    int *n_dev = (int *)(ctx->vox_buf + bytes - 256);
    if (launch_voxel_downsample(xyz_dev, (int)n, vg, ctx->vox_buf, bytes - 256, xyz_out_dev, count_out_dev, n_dev, ctx->st) !=
        hipSuccess)
        return fail(ctx, ICP_E_HIP, "icp_voxel_downsample: a launch failed");
    int cells = 0;
    HIPCHK(hipMemcpyAsync(&cells, n_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *n_out = (size_t)cells;
    return ICP_OK;
}

static int voxel_args(icp_ctx *ctx, const void *xyz, size_t n, double voxel, const double *origin, const void *xyz_out,
                      const size_t *n_out)
{
    if (!ctx) return ICP_E_ARG;
    if (!xyz || !xyz_out || !n_out) return fail(ctx, ICP_E_ARG, "icp_voxel_downsample: xyz, xyz_out or n_out is null");
    if (n == 0 || n > (size_t)INT_MAX)
        return fail(ctx, ICP_E_ARG, "icp_voxel_downsample: n = " + std::to_string(n) + " is outside [1, INT_MAX]");
    if (!std::isfinite(voxel) || !(voxel > 0.0))
        return fail(ctx, ICP_E_ARG, "icp_voxel_downsample: voxel = " + std::to_string(voxel) + " is not finite and > 0");
    if (origin)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(origin[a]))
                return fail(ctx, ICP_E_ARG, "icp_voxel_downsample: origin[" + std::to_string(a) + "] is not finite");
    HIPCHK(hipSetDevice(ctx->device));
    return ICP_OK;
}

int icp_voxel_downsample_device(icp_ctx *ctx, const double *xyz_dev, size_t n, double voxel, const double *origin,
                                double *xyz_out_dev, int32_t *count_out_dev, size_t *n_out)
{
    TRY(voxel_args(ctx, xyz_dev, n, voxel, origin, xyz_out_dev, n_out));
    HIPCHK(hipDeviceSynchronize()); // (the array is read after the work of any stream, as icp_set_model_device's)
    return voxel_downsample_dev(ctx, xyz_dev, n, voxel, origin, xyz_out_dev, count_out_dev, n_out);
}

int icp_voxel_downsample(icp_ctx *ctx, const double *xyz, size_t n, double voxel, const double *origin, double *xyz_out,
                         int32_t *count_out, size_t *n_out)
{
    TRY(voxel_args(ctx, xyz, n, voxel, origin, xyz_out, n_out));
    const size_t bad = first_nonfinite(xyz, 3 * n);
    if (bad != kAllFinite) return fail(ctx, ICP_E_ARG, "icp_voxel_downsample: point " + std::to_string(bad / 3) + " is not finite");
    TRY(ctx->vox_io.grow(ctx, 6 * n));
    if (count_out) TRY(ctx->vox_cnt.grow(ctx, n));
    double *in = ctx->vox_io, *out = ctx->vox_io + 3 * n;
    HIPCHK(hipMemcpyAsync(in, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->st));
    size_t cells = 0;
    TRY(voxel_downsample_dev(ctx, in, n, voxel, origin, out, count_out ? ctx->vox_cnt : nullptr, &cells));
    HIPCHK(hipMemcpyAsync(xyz_out, out, sizeof(double) * 3 * cells, hipMemcpyDeviceToHost, ctx->st));
    if (count_out)
        HIPCHK(hipMemcpyAsync(count_out, ctx->vox_cnt, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *n_out = cells;
    return ICP_OK;
}

// ---- per-operation surface ------------------------------------------------------------

// Few queries (the per-point API: compute_distance_w_naive, GPU::ICP::compute_y_naive): one
// exact fp64 launch per call with mapped host I/O, instead of the certified cascade's ~10
// launches and two pageable copies.  Same rule (first minimum of D64), same indices.  Taken
// by the automatic variant choice (and the fp64 mode).
constexpr size_t kFewQueries = 32;

// The end of a per-operation call's work on the stream, without the runtime's synchronisation:
// a one-thread kernel stores a ticket into mapped host memory and the host spins on it
// (wait_flag: it still reports a failed stream).  Saves ~5-10 us per call, which is what the
// per-point API's thousands of calls (compute_distance_w_naive) pay.
static int sync_by_flag(icp_ctx *ctx)
{
    if (!ctx->h_sig) {
        TRY(ctx->h_sig.grow(ctx, 64 / sizeof(int)));
        std::memset(ctx->h_sig, 0, 64);
    }
    const int ticket = ++ctx->sig_ticket;
    launch_signal(ctx->h_sig.dev(), ticket, ctx->st);
    LAUNCHCHK("signal");
    return wait_flag(ctx, ctx->h_sig, ticket);
}

static int closest_few(icp_ctx *ctx, const double *p_xyz, size_t np, double *y_xyz_out, int32_t *idx_out)
{
    TRY(ctx->h_few.grow(ctx, 7 * kFewQueries));
    double *hq = ctx->h_few, *hy = ctx->h_few + 3 * kFewQueries;
    int *hi = (int *)(ctx->h_few + 6 * kFewQueries);
    std::memcpy(hq, p_xyz, sizeof(double) * 3 * np);
    launch_nn_exact_few(ctx->h_few.dev(), (int)np, ctx->m4, (int)ctx->nm, (int *)(ctx->h_few.dev() + 6 * kFewQueries),
                        ctx->h_few.dev() + 3 * kFewQueries, ctx->st);
    LAUNCHCHK("nn_exact_few");
    TRY(sync_by_flag(ctx));
    if (y_xyz_out) std::memcpy(y_xyz_out, hy, sizeof(double) * 3 * np);
    if (idx_out) std::memcpy(idx_out, hi, sizeof(int32_t) * np);
    ctx->stats.nn_pairs += (long long)np * (long long)ctx->nm;
    return ICP_OK;
}

// A model image that fits in LDS, and a query count the mapped buffer holds: one launch
// (launch_nn_lds), queries and results through mapped host memory.
static int closest_lds(icp_ctx *ctx, const double *p_xyz, size_t np, double *y_xyz_out, int32_t *idx_out)
{
    double *h, *d; // queries, y, idx
    TRY(io_take(ctx, 6 * np + (np + 1) / 2, &h, &d));
    std::memcpy(h, p_xyz, sizeof(double) * 3 * np);
    static const int cull = [] { // ICP_PERSIST_NN=all: every model point for every query (A/B)
        const char *e = getenv("ICP_PERSIST_NN");
        return e && std::strcmp(e, "all") == 0 ? 0 : 1;
    }();
    const size_t lds = 24 * ctx->nm + 48 * ctx->pm_blocks;
    launch_nn_lds(ctx->pm_img, (int)ctx->nm, (int)ctx->pm_blocks, d, (int)np, cull, ctx->model_host.data(),
                  (int *)(d + 6 * np), d + 3 * np, lds, ctx->st);
    LAUNCHCHK("nn_lds");
    TRY(sync_by_flag(ctx));
    ctx->io_pending = false;
    if (y_xyz_out) std::memcpy(y_xyz_out, h + 3 * np, sizeof(double) * 3 * np);
    if (idx_out) std::memcpy(idx_out, h + 6 * np, sizeof(int32_t) * np);
    ctx->stats.nn_pairs += (long long)np * (long long)ctx->nm;
    return ICP_OK;
}

int icp_closest_matrix(icp_ctx *ctx, const double *p_xyz, size_t np, double *y_xyz_out,
                       int32_t *idx_out)
{
    TRY(check_ready(ctx, false));
    if (!p_xyz && np) return ICP_E_ARG;
    // (an explicitly chosen NN variant always runs its own cascade, as the tests of it expect)
    const bool auto_rule = (ctx->nn_variant == ICP_NN_VARIANT_AUTO || ctx->nn_mode == ICP_NN_FP64) &&
                           ctx->nn_rule == ICP_NN_RULE_SQUARED;
    if (np && np <= kFewQueries && auto_rule) return closest_few(ctx, p_xyz, np, y_xyz_out, idx_out);
    // (closest_lds takes queries, y and the int32 indices from the mapped buffer: 6.5 doubles a query)
    if (np && auto_rule && ctx->pm_img && ctx->nm <= (size_t)kPersistMaxModel &&
        6 * np + (np + 1) / 2 <= 2 * kMappedIo && 24 * ctx->nm + 48 * ctx->pm_blocks + 4096 <= ctx->lds_per_cu)
        return closest_lds(ctx, p_xyz, np, y_xyz_out, idx_out);
    TRY(upload_cloud(ctx, ctx->qa, p_xyz, np, true));
    ctx->seeds_valid = false; // idx is about to hold other queries' correspondences
    ctx->seedd_valid = false;
    ctx->q_order_src = nullptr;
    TRY(nn_search(ctx, ctx->qa, np));
    TRY(cpu_rule_fixup(ctx, ctx->qa, np, nullptr));
    if (np && y_xyz_out) {
        TRY(grow_cloud(ctx, ctx->qb, np, false));
        launch_gather_moments(ctx->idx, ctx->m4, ctx->qa.x,
                              ctx->qa.y, ctx->qa.z, (int)np, ctx->qb.x, ctx->qb.y, ctx->qb.z,
                              ctx->partials, ctx->st);
        LAUNCHCHK("gather");
        TRY(download_cloud(ctx, ctx->qb, np, y_xyz_out));
    }
    if (np && idx_out)
        HIPCHK(hipMemcpyAsync(idx_out, ctx->idx, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (np) account_nn(ctx, np);
    return ICP_OK;
}

int icp_compute_centroid(icp_ctx *ctx, const double *xyz, size_t n, double mu[3], double *centred_out)
{
    if (!ctx || !mu || (!xyz && n) || n == 0) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    TRY(ensure_reduction_space(ctx));
    if (n <= (size_t)kRedSingle) { // one launch on mapped host memory (icp_iter.hip)
        double *hin, *din; // one region: input, the centred output, the three sums
        TRY(io_take(ctx, 6 * n + 4, &hin, &din));
        double *hout = hin + 3 * n, *dout = din + 3 * n, *hsum = hin + 6 * n, *dsum = din + 6 * n;
        std::memcpy(hin, xyz, sizeof(double) * 3 * n);
        launch_small_centroid(din, (int)n, (double)n, dsum, centred_out ? dout : nullptr, ctx->st);
        LAUNCHCHK("centroid");
        TRY(sync_by_flag(ctx));
        ctx->io_pending = false;
        for (int k = 0; k < 3; ++k) mu[k] = hsum[k] / (double)n; // rowwise().mean()
        if (centred_out) std::memcpy(centred_out, hout, sizeof(double) * 3 * n);
        return ICP_OK;
    }
    if (3 * n <= kMappedIo) { // mid-size: sum and centre straight from / into mapped host memory
        double *hin, *din; // one region: input, then the centred output (<= the buffer's 2 x kMappedIo)
        TRY(io_take(ctx, (centred_out ? 6 : 3) * n, &hin, &din));
        double *hout = hin + 3 * n, *dout = din + 3 * n;
        std::memcpy(hin, xyz, sizeof(double) * 3 * n);
        launch_sum3(din, din + 1, din + 2, (int)n, red_target(ctx, n, ctx->sums), ctx->st, 3);
        red_finish(ctx, n, 3, ctx->sums);
        if (centred_out) launch_centre_aos(din, (int)n, ctx->sums, dout, ctx->st);
        LAUNCHCHK("centroid");
        HIPCHK(hipMemcpyAsync(ctx->h_sums, ctx->sums, sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
        ctx->io_pending = false;
        for (int k = 0; k < 3; ++k) mu[k] = ctx->h_sums[k] / (double)n; // rowwise().mean()
        if (centred_out) std::memcpy(centred_out, hout, sizeof(double) * 3 * n);
        return ICP_OK;
    }
    TRY(upload_cloud(ctx, ctx->qa, xyz, n, false));
    launch_sum3(ctx->qa.x, ctx->qa.y, ctx->qa.z, (int)n, red_target(ctx, n, ctx->sums), ctx->st);
    red_finish(ctx, n, 3, ctx->sums);
    LAUNCHCHK("sum3");
    HIPCHK(hipMemcpyAsync(ctx->h_sums, ctx->sums, sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    for (int k = 0; k < 3; ++k) mu[k] = ctx->h_sums[k] / (double)n;
    if (centred_out) {
        launch_subtract(ctx->qa.x, ctx->qa.y, ctx->qa.z, (int)n, mu[0], mu[1], mu[2], ctx->st);
        LAUNCHCHK("subtract");
        TRY(download_cloud(ctx, ctx->qa, n, centred_out));
    }
    return ICP_OK;
}

int icp_subtract_col(icp_ctx *ctx, const double *xyz, size_t n, const double m[3], double *out)
{
    if (!ctx || !m || ((!xyz || !out) && n)) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    TRY(ensure_reduction_space(ctx));
    if (!n) return ICP_OK;
    if (3 * n <= kMappedIo) { // small: straight from / into mapped host memory
        double *hin, *din;
        TRY(io_take(ctx, 6 * n, &hin, &din));
        std::memcpy(hin, xyz, sizeof(double) * 3 * n);
        launch_subtract_aos(din, (int)n, m, din + 3 * n, ctx->st);
        LAUNCHCHK("subtract_col");
        TRY(sync_by_flag(ctx));
        ctx->io_pending = false;
        std::memcpy(out, hin + 3 * n, sizeof(double) * 3 * n);
        return ICP_OK;
    }
    TRY(upload_cloud(ctx, ctx->qa, xyz, n, false));
    launch_subtract(ctx->qa.x, ctx->qa.y, ctx->qa.z, (int)n, m[0], m[1], m[2], ctx->st);
    LAUNCHCHK("subtract_col");
    return download_cloud(ctx, ctx->qa, n, out);
}

int icp_y_p_norm(icp_ctx *ctx, const double *y_xyz, const double *p_xyz, size_t n, double *d_caps,
                 double *sp)
{
    if (!ctx || !d_caps || !sp || ((!y_xyz || !p_xyz) && n)) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    TRY(ensure_reduction_space(ctx));
    TRY(upload_cloud(ctx, ctx->qa, y_xyz, n, false));
    TRY(upload_cloud(ctx, ctx->qb, p_xyz, n, false));
    launch_norms(ctx->qa.x, ctx->qa.y, ctx->qa.z, ctx->qb.x, ctx->qb.y, ctx->qb.z, (int)n,
                 red_target(ctx, n, ctx->sums), ctx->st);
    red_finish(ctx, n, 2, ctx->sums);
    LAUNCHCHK("norms");
    HIPCHK(hipMemcpyAsync(ctx->h_sums, ctx->sums, sizeof(double) * 2, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *d_caps = ctx->h_sums[0];
    *sp = ctx->h_sums[1];
    return ICP_OK;
}

int icp_err_compute(icp_ctx *ctx, const double *y_xyz, double *p_xyz, size_t n, int in_place,
                    const double sR[9], const double t[3], double *err)
{
    if (!ctx || !sR || !t || !err || ((!y_xyz || !p_xyz) && n)) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    TRY(ensure_reduction_space(ctx));
    if (n && n <= (size_t)kRedSingle) { // one launch on mapped host memory (icp_iter.hip)
        double *h, *d; // y, p, the sum
        TRY(io_take(ctx, 6 * n + 2, &h, &d));
        std::memcpy(h, y_xyz, sizeof(double) * 3 * n);
        std::memcpy(h + 3 * n, p_xyz, sizeof(double) * 3 * n);
        Xform xf;
        std::memcpy(xf.sR, sR, sizeof(xf.sR));
        std::memcpy(xf.t, t, sizeof(xf.t));
        std::memcpy(xf.c, ctx->c, sizeof(xf.c));
        launch_small_err(d, d + 3 * n, (int)n, xf, in_place ? 1 : 0, d + 6 * n, ctx->st);
        LAUNCHCHK("err_compute");
        TRY(sync_by_flag(ctx));
        ctx->io_pending = false;
        *err = h[6 * n];
        if (in_place) std::memcpy(p_xyz, h + 3 * n, sizeof(double) * 3 * n);
        return ICP_OK;
    }
    TRY(upload_cloud(ctx, ctx->qa, y_xyz, n, false));
    TRY(upload_cloud(ctx, ctx->qb, p_xyz, n, false));
    Xform xf;
    std::memcpy(xf.sR, sR, sizeof(xf.sR));
    std::memcpy(xf.t, t, sizeof(xf.t));
    std::memcpy(xf.c, ctx->c, sizeof(xf.c));
    launch_transform_err(ctx->qb.x, ctx->qb.y, ctx->qb.z, ctx->qa.x, ctx->qa.y, ctx->qa.z, (int)n, xf,
                         in_place ? 1 : 0, nullptr, red_target(ctx, n, ctx->sums), ctx->st);
    red_finish(ctx, n, 1, ctx->sums);
    LAUNCHCHK("transform_err");
    HIPCHK(hipMemcpyAsync(ctx->h_sums, ctx->sums, sizeof(double), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *err = ctx->h_sums[0];
    if (in_place) TRY(download_cloud(ctx, ctx->qb, n, p_xyz));
    return ICP_OK;
}

int icp_find_alignment(icp_ctx *ctx, const double *p_xyz, const double *y_xyz, size_t n, double *s,
                       double R[9], double t[3], double *err)
{
    if (!ctx || !s || !R || !t || !err || !p_xyz || !y_xyz || n == 0) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    TRY(ensure_reduction_space(ctx));
    if (n <= (size_t)kRedSingle) { // one launch on mapped host memory, Horn on the device (icp_iter.hip)
        double *h, *d; // p, y, the results
        TRY(io_take(ctx, 6 * n + 32, &h, &d));
        std::memcpy(h, p_xyz, sizeof(double) * 3 * n);
        std::memcpy(h + 3 * n, y_xyz, sizeof(double) * 3 * n);
        launch_small_alignment(d, d + 3 * n, (int)n, d + 6 * n, ctx->st);
        LAUNCHCHK("find_alignment");
        TRY(sync_by_flag(ctx));
        ctx->io_pending = false;
        const double *o = h + 6 * n;
        *s = o[18];
        for (int k = 0; k < 9; ++k) R[k] = o[19 + k];
        for (int k = 0; k < 3; ++k) t[k] = o[28 + k];
        *err = o[kSumErr];
        return ICP_OK;
    }
    TRY(upload_cloud(ctx, ctx->qb, p_xyz, n, false));
    TRY(upload_cloud(ctx, ctx->qa, y_xyz, n, false));
    launch_sum3(ctx->qb.x, ctx->qb.y, ctx->qb.z, (int)n, red_target(ctx, n, ctx->sums + kSumP), ctx->st);
    red_finish(ctx, n, 3, ctx->sums + kSumP);
    launch_sum3(ctx->qa.x, ctx->qa.y, ctx->qa.z, (int)n, red_target(ctx, n, ctx->sums + kSumY), ctx->st);
    red_finish(ctx, n, 3, ctx->sums + kSumY);
    launch_centred_moments(ctx->qb.x, ctx->qb.y, ctx->qb.z, ctx->qa.x, ctx->qa.y, ctx->qa.z, (int)n,
                           ctx->sums, (double)n, red_target(ctx, n, ctx->sums + kSumS), ctx->st);
    red_finish(ctx, n, 11, ctx->sums + kSumS);
    LAUNCHCHK("find_alignment moments");
    HIPCHK(hipMemcpyAsync(ctx->h_sums, ctx->sums, sizeof(double) * kSumErr, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    const double N = (double)n;
    const double *h = ctx->h_sums;
    const double mu_p[3] = {h[kSumP] / N, h[kSumP + 1] / N, h[kSumP + 2] / N};
    const double mu_y[3] = {h[kSumY] / N, h[kSumY + 1] / N, h[kSumY + 2] / N};
    horn_solve(h + kSumS, mu_p, mu_y, h[kSumDcaps], h[kSumSp], s, R, t);
    double sR[9];
    for (int k = 0; k < 9; ++k) sR[k] = *s * R[k];
    Xform xf;
    std::memcpy(xf.sR, sR, sizeof(sR));
    std::memcpy(xf.t, t, sizeof(xf.t));
    std::memcpy(xf.c, ctx->c, sizeof(xf.c));
    launch_transform_err(ctx->qb.x, ctx->qb.y, ctx->qb.z, ctx->qa.x, ctx->qa.y, ctx->qa.z, (int)n, xf,
                         0, nullptr, red_target(ctx, n, ctx->sums + kSumErr), ctx->st);
    red_finish(ctx, n, 1, ctx->sums + kSumErr);
    LAUNCHCHK("find_alignment err");
    HIPCHK(hipMemcpyAsync(ctx->h_sums + kSumErr, ctx->sums + kSumErr, sizeof(double),
                          hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    *err = ctx->h_sums[kSumErr];
    return ICP_OK;
}

int icp_get_indices(icp_ctx *ctx, int32_t *idx_out)
{
    if (!ctx || (!idx_out && ctx->scene.n)) return ICP_E_ARG;
    if (!ctx->has_scene || !ctx->seeds_valid)
        return fail(ctx, ICP_E_NO_MODEL, "no NN search over the resident scene since icp_set_scene");
    HIPCHK(hipSetDevice(ctx->device));
    const int *src = ctx->idx;
    if (ctx->scene_slot && ctx->scene.n) { // back to the caller's order
        TRY(ctx->s_tmp_idx.grow(ctx, ctx->scene.n));
        launch_permute_cloud(ctx->s_order, (int)ctx->scene.n, 1, nullptr, nullptr, nullptr, nullptr, ctx->idx, nullptr,
                             nullptr, nullptr, nullptr, ctx->s_tmp_idx, ctx->st);
        LAUNCHCHK("indices_to_file_order");
        src = ctx->s_tmp_idx;
    }
    if (ctx->scene.n)
        HIPCHK(hipMemcpyAsync(idx_out, src, sizeof(int32_t) * ctx->scene.n, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return ICP_OK;
}

int icp_set_index_digest(icp_ctx *ctx, size_t cap)
{
    if (!ctx) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    if (cap) {
        TRY(ctx->digest.grow(ctx, 3 * cap));
        // (on the engine stream: a null-stream hipMemset is not ordered against the non-blocking
        // engine stream and may land in the middle of the next run's digests -- seen once in
        // the 8-context C5 test, a digest 9% short)
        HIPCHK(hipMemsetAsync(ctx->digest, 0, sizeof(unsigned long long) * 3 * cap, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
    }
    ctx->digest_cap = cap;
    return ICP_OK;
}

int icp_get_index_digest(icp_ctx *ctx, uint64_t *out, size_t cap)
{
    if (!ctx || !out || cap > ctx->digest_cap) return ICP_E_ARG;
    if (!cap) return ICP_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out, ctx->digest, sizeof(uint64_t) * 3 * cap, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return ICP_OK;
}

static int cert_audit_reset(icp_ctx *ctx)
{
    const unsigned init[3] = {0u, 0x7f800000u, 0u}; // max ratio 0, min margin +inf, count 0
    // on the engine stream (non-blocking: the null-stream hipMemcpy is not ordered against it),
    // then waited for, since `init` lives on this frame
    HIPCHK(hipMemcpyAsync(ctx->cert_audit, init, sizeof(init), hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return ICP_OK;
}

int icp_set_cert_audit(icp_ctx *ctx, int enable)
{
    if (!ctx) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (!enable) {
        HIPCHK(ctx->cert_audit.release());
        return ICP_OK;
    }
    TRY(ctx->cert_audit.grow(ctx, 4));
    return cert_audit_reset(ctx);
}

int icp_bundle_audit(icp_ctx *ctx, int groups, icp_bundle_audit_result *out)
{
    if (!ctx || !out || groups < 1) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const DevCloud &P = ctx->scene;
    TRY(ensure_bundle(ctx));
    if (!ctx->b_img || !ctx->b_bctr || !ctx->b_kd_orig || ctx->nb_pad <= 0 || !P.n || !ctx->seeds_valid)
        return fail(ctx, ICP_E_NO_MODEL, "icp_bundle_audit: needs the bundle images and a scene with correspondences");
    DevBuf<unsigned long long> buf;
    TRY(buf.grow(ctx, 6));
    const double inf = INFINITY;
    unsigned long long init[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    std::memcpy(&init[1], &inf, sizeof(double));
    int rc = ICP_OK;
    if (hipMemcpyAsync(buf, init, sizeof(init), hipMemcpyHostToDevice, ctx->st) != hipSuccess) rc = ICP_E_HIP;
    if (rc == ICP_OK) {
        launch_bundle_audit(P.x, P.y, P.z, ctx->idx, ctx->m4, (int)P.n, groups, ctx->b_img, ctx->b_bctr, ctx->b_kd_orig,
                            (int)ctx->nm, ctx->nb_pad, ctx->c, ctx->scale16, buf, buf + 2, ctx->st);
        unsigned long long h[6];
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(h, buf, sizeof(h), hipMemcpyDeviceToHost, ctx->st) != hipSuccess ||
            hipStreamSynchronize(ctx->st) != hipSuccess) {
            rc = ICP_E_HIP;
        } else {
            std::memcpy(&out->max_err_ratio, &h[0], sizeof(double));
            std::memcpy(&out->min_gap, &h[1], sizeof(double));
            out->pairs = (long long)h[2];
            out->excluded = (long long)h[3];
            out->violations = (long long)h[4];
            out->checked = (long long)h[5];
        }
    }
    return rc == ICP_OK ? ICP_OK : fail(ctx, rc, "icp_bundle_audit: HIP error");
}

int icp_get_model_order(icp_ctx *ctx, int32_t *kd_out)
{
    if (!ctx || !kd_out) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->has_model) TRY(ensure_bundle(ctx));
    if (!ctx->has_model || ctx->nb_pad <= 0 || !ctx->b_kd) return fail(ctx, ICP_E_NO_MODEL, "no bundle kd order");
    HIPCHK(hipMemcpyAsync(kd_out, ctx->b_kd, sizeof(int32_t) * ctx->nm, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return ICP_OK;
}

int icp_sort_pairs(int device, const uint32_t *keys, size_t n, int bits, uint32_t *keys_out, int32_t *order_out)
{
    if (bits < 0 || bits > 32 || n > (size_t)INT_MAX || (n && (!keys || !order_out))) return ICP_E_ARG;
    if (n == 0) return ICP_OK;
    if (hipSetDevice(device) != hipSuccess) return ICP_E_HIP;
    size_t temp = 0;
    (void)icp::sort_pairs_u32(nullptr, temp, nullptr, nullptr, nullptr, nullptr, (int)n, bits, nullptr);
    DevBuf<char> mem;
    const size_t kb = ((n * 4 + 255) & ~(size_t)255);
    if (mem.grow(nullptr, 3 * kb + temp) != ICP_OK) return ICP_E_HIP;
    char *buf = mem;
    unsigned *k0 = (unsigned *)buf, *k1 = (unsigned *)(buf + kb);
    int *v1 = (int *)(buf + 2 * kb);
    bool ok = hipMemcpy(k0, keys, n * 4, hipMemcpyHostToDevice) == hipSuccess &&
              icp::sort_pairs_u32(buf + 3 * kb, temp, k0, k1, nullptr, v1, (int)n, bits, nullptr) == hipSuccess &&
              hipMemcpy(order_out, v1, n * 4, hipMemcpyDeviceToHost) == hipSuccess &&
              (!keys_out || hipMemcpy(keys_out, k1, n * 4, hipMemcpyDeviceToHost) == hipSuccess);
    ok = mem.release() == hipSuccess && ok;
    return ok ? ICP_OK : ICP_E_HIP;
}

int icp_select_kth(int device, const double *v, size_t n, size_t k, double *out)
{
    if (!v || !out || n == 0 || n > (size_t)INT_MAX || k == 0 || k > n) return ICP_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return ICP_E_HIP;
    // one allocation: the values, their keys, the bins, the state, the result
    const size_t vb = (n * 8 + 255) & ~(size_t)255, bb = sizeof(unsigned) * icp::kSelectBins;
    DevBuf<char> mem;
    if (mem.grow(nullptr, 2 * vb + bb + 256 + 256) != ICP_OK) return ICP_E_HIP;
    char *buf = mem;
    double *dv = (double *)buf;
    unsigned long long *keys = (unsigned long long *)(buf + vb);
    unsigned *bins = (unsigned *)(buf + 2 * vb);
    icp::SelectState *state = (icp::SelectState *)(buf + 2 * vb + bb);
    double *cut = (double *)(buf + 2 * vb + bb + 256);
    bool ok = hipMemcpy(dv, v, n * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemset(bins, 0, bb) == hipSuccess;
    if (ok) {
        icp::launch_select_map(dv, (int)n, keys, nullptr);
        icp::launch_select_kth(keys, (int)n, (unsigned long long)k, state, nullptr, bins, cut, nullptr, nullptr, nullptr);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(out, cut, sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
    ok = mem.release() == hipSuccess && ok;
    return ok ? ICP_OK : ICP_E_HIP;
}

int icp_get_grid(icp_ctx *ctx, int g[3], double lo[3], double *inv_h, int32_t *start, int32_t *order)
{
    if (!ctx || !g || !lo || !inv_h) return ICP_E_ARG;
    if (!ctx->has_model || !ctx->g_start || !ctx->g_pts) return fail(ctx, ICP_E_NO_MODEL, "no model grid");
    HIPCHK(hipSetDevice(ctx->device));
    for (int a = 0; a < 3; ++a) {
        g[a] = ctx->grid.g[a];
        lo[a] = ctx->grid.lo[a];
    }
    *inv_h = ctx->grid.inv_h;
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (start)
        HIPCHK(hipMemcpy(start, ctx->g_start, sizeof(int32_t) * ((size_t)grid_cells(ctx->grid) + 1),
                         hipMemcpyDeviceToHost));
    if (order) { // (each sorted point's record carries its model index in w)
        std::vector<double> pts(4 * ctx->nm);
        HIPCHK(hipMemcpy(pts.data(), ctx->g_pts, sizeof(double) * 4 * ctx->nm, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < ctx->nm; ++k) order[k] = (int32_t)pts[4 * k + 3];
    }
    return ICP_OK;
}

int icp_get_stats(const icp_ctx *ctx, icp_stats *out)
{
    if (!ctx || !out) return ICP_E_ARG;
    *out = ctx->stats;
    long long cc[2]; // (the runs' certificate counts still on the device)
    if (sum_cert_counts(ctx, cc) != ICP_OK) return ICP_E_HIP;
    out->run_certified += cc[0];
    out->run_walked += cc[1];
    out->cert_max_err_ratio = -1.0;
    out->cert_min_margin = -1.0;
    out->cert_audited = 0;
    if (ctx->cert_audit) {
        unsigned a[3] = {0, 0, 0};
        if (hipStreamSynchronize(ctx->st) != hipSuccess ||
            hipMemcpy(a, ctx->cert_audit, sizeof(a), hipMemcpyDeviceToHost) != hipSuccess)
            return ICP_E_HIP;
        float r, mg;
        std::memcpy(&r, &a[0], 4);
        std::memcpy(&mg, &a[1], 4);
        out->cert_max_err_ratio = r;
        out->cert_min_margin = mg;
        out->cert_audited = a[2];
    }
    return ICP_OK;
}

int icp_reset_stats(icp_ctx *ctx)
{
    if (!ctx) return ICP_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->cert_audit) TRY(cert_audit_reset(ctx));
    ctx->stats = icp_stats{};
    ctx->cert_counts_rows = 0; // (the device's certificate counts go with the rest: zeroed at the next run)
    ctx->stats.last_filter = -1;
    return ICP_OK;
}

} // extern "C"
