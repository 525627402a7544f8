// icp_cloud.hip -- the calls on a cloud's neighbourhoods, none of them on icp_run's path, host code only:
// the model's and the scene's normals set, read and estimated, icp_model_knn, and the temporary grid of a
// cloud that is not the resident model (the scene's estimator, icp_fpfh, the outlier filters).  Scratch, a
// call's device memory, and the checks these files share (icp_engine.h) are here too; no kernel is.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "icp_engine.h"

namespace icp {
namespace engine {

Scratch::~Scratch()
{
    own.clear(); // (the object's own allocations go first, as they always did)
    if (!kept || !begun) return;
    kept->want = total;
    // The call did not fit: the block grown to its total now, not at the next call's start, so that the
    // next call at these sizes allocates nothing.  (Every caller has synchronised, or the frees above have; a
    // failure leaves an empty block, which the next object grows again, and the call's own status and message.)
    if (kept->base.capacity() < total) {
        const std::string err = ctx->err;
        if (kept->base.grow(ctx, total) != ICP_OK) ctx->err = err;
    }
}

int Scratch::get_bytes(void **out, size_t bytes)
{
    *out = nullptr;
    if (kept) {
        if (!begun && kept->base.capacity() < kept->want) TRY(kept->base.grow(ctx, kept->want)); // (once)
        begun = true;
        const size_t part = (bytes + 255) & ~(size_t)255;
        total += part;
        if (off + part <= kept->base.capacity()) {
            *out = kept->base + off;
            off += part;
            return ICP_OK;
        }
    }
    DevBuf<char> mine;
    TRY(mine.grow(ctx, bytes));
    *out = mine;
    own.push_back(std::move(mine));
    return ICP_OK;
}

int knn_k_check(icp_ctx *ctx, const std::string &who, const char *name, int k, const std::string &word, size_t n)
{
    if (k < kKnnMinK || k > kKnnMaxK)
        return fail(ctx, ICP_E_ARG, who + ": " + name + " = " + std::to_string(k) + " is outside [" +
                                        std::to_string(kKnnMinK) + ", " + std::to_string(kKnnMaxK) + "]");
    if ((size_t)k > n)
        return fail(ctx, ICP_E_ARG, who + ": " + name + " = " + std::to_string(k) + " exceeds the " + word + "'s " +
                                        std::to_string(n) + " points");
    return ICP_OK;
}

// What icp_set_{model,scene}_normals[_device] share: the checks (who: the host function's name, which
// its _device form reports under too; word: the cloud's; present, count: the cloud's) and, of a host
// array, the finite check and the upload to the stage.  *aos_dev: the interleaved array in device memory.
static int normals_upload(icp_ctx *ctx, const std::string &who, const std::string &word, bool present, size_t count,
                          const double *n_xyz, size_t n, bool host, const double **aos_dev)
{
    if (!present) return fail(ctx, ICP_E_NO_MODEL, who + ": no " + word + " (icp_set_" + word + ")");
    if (n != count)
        return fail(ctx, ICP_E_SIZE_MISMATCH, who + ": " + std::to_string(n) + " normals for a " + word + " of " +
                                                  std::to_string(count) + " points");
    HIPCHK(hipSetDevice(ctx->device));
    *aos_dev = n_xyz;
    if (!host) {
        HIPCHK(hipDeviceSynchronize()); // (as icp_set_model_device / icp_set_scene_device: after the work of any stream)
        return ICP_OK;
    }
    const size_t bad = first_nonfinite(n_xyz, 3 * n);
    if (bad != kAllFinite) return fail(ctx, ICP_E_ARG, who + ": normal " + std::to_string(bad / 3) + " is not finite");
    TRY(ctx->stage.grow(ctx, 3 * n));
    HIPCHK(hipMemcpyAsync(ctx->stage, n_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->st));
    *aos_dev = ctx->stage;
    return ICP_OK;
}

// the model's normals as double4 rows, from its interleaved array (host or device memory)
static int set_model_normals(icp_ctx *ctx, const double *n_xyz, size_t nm, bool host)
{
    if (!ctx || !n_xyz) return ICP_E_ARG;
    const double *aos_dev = nullptr;
    TRY(normals_upload(ctx, "icp_set_model_normals", "model", ctx->has_model, ctx->nm, n_xyz, nm, host, &aos_dev));
    TRY(ctx->n4.grow(ctx, nm));
    launch_plane_normals4(aos_dev, (int)nm, ctx->n4, ctx->st);
    LAUNCHCHK("plane_normals4");
    HIPCHK(hipStreamSynchronize(ctx->st)); // (the caller's array, or the stage, is free again)
    ctx->has_normals = true;
    return ICP_OK;
}

// u0 (the caller's order) from the scene's interleaved normals (host or device memory)
static int set_scene_normals(icp_ctx *ctx, const double *n_xyz, size_t n, bool host)
{
    if (!ctx || !n_xyz) return ICP_E_ARG;
    const double *aos_dev = nullptr;
    TRY(normals_upload(ctx, "icp_set_scene_normals", "scene", ctx->has_scene, ctx->scene.n, n_xyz, n, host, &aos_dev));
    ctx->has_scene_normals = false; // (until the new ones are complete)
    ctx->sn_slot_valid = false;
    TRY(grow_cloud(ctx, ctx->sn, n, false));
    if (n) launch_aos_to_soa(aos_dev, n, ctx->sn.x, ctx->sn.y, ctx->sn.z, ctx->st);
    LAUNCHCHK("scene_normals");
    HIPCHK(hipStreamSynchronize(ctx->st)); // (the caller's array, or the stage, is free again)
    ctx->has_scene_normals = true;
    return ICP_OK;
}

// the checks of a k-NN call over a cloud (word, present, count: the model or the scene) and of an
// estimator's viewpoint (nullable); nothing has run when they fail
static int knn_args(icp_ctx *ctx, const std::string &who, const std::string &word, bool present, size_t count, int k,
                    const double *viewpoint)
{
    if (!present) return fail(ctx, ICP_E_NO_MODEL, who + ": no " + word + " (icp_set_" + word + ")");
    TRY(knn_k_check(ctx, who, "k", k, word, count));
    const size_t a = viewpoint ? first_nonfinite(viewpoint, 3) : kAllFinite;
    if (a != kAllFinite)
        return fail(ctx, ICP_E_ARG, who + ": viewpoint[" + std::to_string(a) + "] = " + std::to_string(viewpoint[a]) +
                                        " is not finite");
    HIPCHK(hipSetDevice(ctx->device));
    return ICP_OK;
}

static bool model_gridded(const icp_ctx *ctx) { return ctx->has_model && ctx->g_start && ctx->g_pts && ctx->m4; }

static bool normals_debug()
{
    static const bool debug = getenv("ICP_NORMALS_DEBUG") != nullptr;
    return debug;
}

// An estimator's first half on a grid gv over the n rows: the counters zeroed, the k-NN + PCA kernel (the
// rows' normals into out).  label: "model", "scene" or "cloud".
static int normals_launch(icp_ctx *ctx, const GridView &gv, const double4 *rows, size_t n, int k, int budget,
                          const double *viewpoint, double4 *out, const std::string &label)
{
    TRY(ctx->knn_counters.grow(ctx, (size_t)kKnnCounters));
    HIPCHK(hipMemsetAsync(ctx->knn_counters, 0, sizeof(unsigned long long) * kKnnCounters, ctx->st));
    launch_model_normals(gv, rows, (int)n, k, budget, viewpoint, out, ctx->knn_counters, normals_debug(), ctx->st);
    LAUNCHCHK(label + "_normals");
    return ICP_OK;
}

// Its second, behind whatever the caller enqueued in between: the counters read back (synchronises):
// *degenerate and, with ICP_NORMALS_DEBUG set, the search's counts to stderr (tools/normals_probe.py).
static int normals_finish(icp_ctx *ctx, size_t n, int k, const std::string &label, long long *degenerate)
{
    unsigned long long c[kKnnCounters];
    HIPCHK(hipMemcpyAsync(c, ctx->knn_counters, sizeof(c), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (degenerate) *degenerate = (long long)c[0];
    if (normals_debug())
        std::fprintf(stderr, "[normals] %s=%zu k=%d degenerate=%llu second_scans=%llu full_scans=%llu candidates=%llu\n",
                     label == "model" ? "nm" : (label == "scene" ? "scene n" : "cloud n"), n, k, c[0], c[1], c[2], c[3]);
    return ICP_OK;
}

// A temporary grid over n points that are not the model: the one place where it is built, so that every
// caller gets what icp_set_model makes of a model's upload.  The cloud comes as its SoA streams and its
// interleaved copy (aos), both in device memory: the box and the finiteness check from aos (ICP_E_RANGE
// names `word`), the grid's size from the box, the double4 rows, the build.  The five arrays are mem's.
static int temp_grid_build(icp_ctx *ctx, const std::string &who, const std::string &word, const double *x, const double *y,
                           const double *z, const double *aos, size_t n, Scratch &mem, TempGrid &tg)
{
    TRY(ensure_model_stats(ctx));
    launch_model_stats(aos, (int)n, ctx->mstat_part, ctx->mstat_out, ctx->st);
    LAUNCHCHK(word + "_stats");
    HIPCHK(hipMemcpyAsync(ctx->h_mstat, ctx->mstat_out, sizeof(double) * 10, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (ctx->h_mstat[9] != 0.0) return fail(ctx, ICP_E_RANGE, who + ": the " + word + " has non-finite coordinates");
    const GridParams gp = grid_params_box(ctx->h_mstat + 3, ctx->h_mstat + 6, n);
    const long long ncell = grid_cells(gp);
    const size_t gbytes = grid_build_scratch_bytes((int)n, ncell);
    // the cloud's rows, the grid's offsets, its points, their fp32 image, the build's sort scratch
    const size_t bytes[5] = {sizeof(double4) * n, sizeof(int) * ((size_t)ncell + 1), sizeof(double4) * n, sizeof(float4) * n,
                             gbytes};
    char *q[5];
    for (int i = 0; i < 5; ++i) TRY(mem.get(&q[i], bytes[i]));
    tg.rows = (double4 *)q[0];
    launch_make_aos4(x, y, z, (int)n, tg.rows, ctx->st);
    if (launch_grid_build(x, y, z, tg.rows, (int)n, gp, q[4], gbytes, (int *)q[1], (double4 *)q[2], (float4 *)q[3], ctx->st) != 0)
        return fail(ctx, ICP_E_HIP, who + ": grid build: radix sort failed");
    LAUNCHCHK(word + "_grid_build");
    tg.gv = grid_view_of(gp, (const int *)q[1], (const double4 *)q[2], (const float4 *)q[3]);
    tg.budget = grid_budget_for(n);
    return ICP_OK;
}

int cloud_grid(icp_ctx *ctx, const std::string &who, const double *aos, size_t n, Scratch &mem, TempGrid &tg)
{
    double *x = nullptr; // the cloud's SoA streams
    TRY(mem.get(&x, 3 * n));
    double *y = x + n, *z = y + n;
    launch_aos_to_soa(aos, n, x, y, z, ctx->st);
    return temp_grid_build(ctx, who, "cloud", x, y, z, aos, n, mem, tg);
}

int cloud_knn(icp_ctx *ctx, const std::string &who, const double *aos, size_t n, int k_normals, const double *viewpoint,
              int k, double4 *rows, double4 *nrm, int *idx, double *d2)
{
    Scratch mem(ctx); // (freed before the call returns, whatever it returns)
    TempGrid tg;
    TRY(cloud_grid(ctx, who, aos, n, mem, tg));
    if (k_normals > 0) {
        TRY(normals_launch(ctx, tg.gv, tg.rows, n, k_normals, tg.budget, viewpoint, nrm, "cloud"));
        TRY(normals_finish(ctx, n, k_normals, "cloud", nullptr));
    }
    launch_model_knn(tg.gv, tg.rows, (int)n, k, tg.budget, idx, d2, ctx->st);
    LAUNCHCHK("cloud_knn");
    HIPCHK(hipMemcpyAsync(rows, tg.rows, sizeof(double4) * n, hipMemcpyDeviceToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st)); // (the grid is freed on return)
    return ICP_OK;
}

} // namespace engine
} // namespace icp

extern "C" {

int icp_set_model_normals(icp_ctx *ctx, const double *n_xyz, size_t nm) { return set_model_normals(ctx, n_xyz, nm, true); }

int icp_set_model_normals_device(icp_ctx *ctx, const double *n_xyz_dev, size_t nm)
{
    return set_model_normals(ctx, n_xyz_dev, nm, false);
}

int icp_model_knn(icp_ctx *ctx, int k, int32_t *idx, double *d2)
{
    if (!ctx) return ICP_E_ARG;
    if (!idx) return fail(ctx, ICP_E_ARG, "icp_model_knn: idx is null");
    TRY(knn_args(ctx, "icp_model_knn", "model", model_gridded(ctx), ctx->nm, k, nullptr));
    const size_t cnt = ctx->nm * (size_t)k;
    TRY(ctx->knn_idx.grow(ctx, cnt));
    if (d2) TRY(ctx->knn_d2.grow(ctx, cnt));
    launch_model_knn(grid_view(ctx), ctx->m4, (int)ctx->nm, k, grid_budget(ctx), ctx->knn_idx, d2 ? ctx->knn_d2 : nullptr,
                     ctx->st);
    LAUNCHCHK("model_knn");
    HIPCHK(hipMemcpyAsync(idx, ctx->knn_idx, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, ctx->st));
    if (d2) HIPCHK(hipMemcpyAsync(d2, ctx->knn_d2, sizeof(double) * cnt, hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    return ICP_OK;
}

int icp_estimate_model_normals(icp_ctx *ctx, int k, const double *viewpoint, long long *degenerate)
{
    if (!ctx) return ICP_E_ARG;
    TRY(knn_args(ctx, "icp_estimate_model_normals", "model", model_gridded(ctx), ctx->nm, k, viewpoint));
    TRY(ctx->n4.grow(ctx, ctx->nm));
    ctx->has_normals = false; // (until the new ones are complete)
    TRY(normals_launch(ctx, grid_view(ctx), ctx->m4, ctx->nm, k, grid_budget(ctx), viewpoint, ctx->n4, "model"));
    TRY(normals_finish(ctx, ctx->nm, k, "model", degenerate));
    ctx->has_normals = true;
    return ICP_OK;
}

int icp_get_model_normals(icp_ctx *ctx, double *n_xyz)
{
    if (!ctx) return ICP_E_ARG;
    if (!n_xyz) return fail(ctx, ICP_E_ARG, "icp_get_model_normals: n_xyz is null");
    if (!ctx->has_model || !ctx->has_normals || !ctx->n4)
        return fail(ctx, ICP_E_NO_MODEL, "icp_get_model_normals: the model has no normals (icp_set_model_normals, "
                                         "icp_estimate_model_normals)");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->st));
    std::vector<double> rows(4 * ctx->nm);
    HIPCHK(hipMemcpy(rows.data(), ctx->n4, sizeof(double) * 4 * ctx->nm, hipMemcpyDeviceToHost));
    rows4_to_xyz(rows.data(), ctx->nm, n_xyz);
    return ICP_OK;
}

int icp_set_scene_normals(icp_ctx *ctx, const double *n_xyz, size_t np_local)
{
    return set_scene_normals(ctx, n_xyz, np_local, true);
}

int icp_set_scene_normals_device(icp_ctx *ctx, const double *n_xyz_dev, size_t np_local)
{
    return set_scene_normals(ctx, n_xyz_dev, np_local, false);
}

int icp_get_scene_normals(icp_ctx *ctx, double *n_xyz)
{
    if (!ctx) return ICP_E_ARG;
    if (!n_xyz && ctx->scene.n) return fail(ctx, ICP_E_ARG, "icp_get_scene_normals: n_xyz is null");
    if (!ctx->has_scene || !ctx->has_scene_normals)
        return fail(ctx, ICP_E_NO_MODEL, "icp_get_scene_normals: the scene has no normals (icp_set_scene_normals, "
                                         "icp_estimate_scene_normals)");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = ctx->scene.n;
    TRY(download_cloud(ctx, ctx->sn, n, n_xyz)); // u0, the caller's order
    if (ctx->tot_n == 0) return ICP_OK;
    const double *Q = ctx->tot + 1; // u = Q u0, each row ((Q0 u0 + Q1 u1) + Q2 u2) as the kernels sum it
    for (size_t j = 0; j < n; ++j) {
        const double a0 = n_xyz[3 * j], a1 = n_xyz[3 * j + 1], a2 = n_xyz[3 * j + 2];
        for (int r = 0; r < 3; ++r) n_xyz[3 * j + r] = (Q[3 * r] * a0 + Q[3 * r + 1] * a1) + Q[3 * r + 2] * a2;
    }
    return ICP_OK;
}

int icp_estimate_scene_normals(icp_ctx *ctx, int k, const double *viewpoint, long long *degenerate)
{
    if (!ctx) return ICP_E_ARG;
    const std::string who = "icp_estimate_scene_normals";
    const size_t n = ctx->scene.n;
    // (these two refusals come before the checks on k; with no scene knn_args' first check answers)
    if (ctx->has_scene && n != ctx->np_total)
        return fail(ctx, ICP_E_ARG, who + ": the scene is sharded (" + std::to_string(n) + " of " +
                                        std::to_string(ctx->np_total) + " points on this rank)");
    if (ctx->has_scene && !ctx->scene_pristine)
        return fail(ctx, ICP_E_ARG, who + ": an icp_run or icp_transform_scene has moved the scene since icp_set_scene");
    TRY(knn_args(ctx, who, "scene", ctx->has_scene, n, k, viewpoint));
    // the scene in the caller's order (a copy when it is resident in slot order), its interleaved
    // copy for the box, its double4 rows: what icp_set_model makes of a model's upload
    const DevCloud *P = &ctx->scene;
    if (ctx->scene_slot) {
        TRY(grow_cloud(ctx, ctx->s_tmp, n, true));
        launch_permute_cloud(ctx->s_order, (int)n, 1, ctx->scene.x, ctx->scene.y, ctx->scene.z, nullptr, nullptr,
                             ctx->s_tmp.x, ctx->s_tmp.y, ctx->s_tmp.z, nullptr, nullptr, ctx->st);
        LAUNCHCHK("scene_to_file_order");
        P = &ctx->s_tmp;
    }
    TRY(ctx->stage.grow(ctx, 3 * n));
    launch_soa_to_aos(P->x, P->y, P->z, n, ctx->stage, ctx->st);
    Scratch mem(ctx); // (freed before the call returns, whatever it returns)
    TempGrid tg;
    double4 *nrm = nullptr; // the normals' rows
    TRY(temp_grid_build(ctx, who, "scene", P->x, P->y, P->z, ctx->stage, n, mem, tg));
    TRY(mem.get(&nrm, n));
    TRY(normals_launch(ctx, tg.gv, tg.rows, n, k, tg.budget, viewpoint, nrm, "scene"));
    ctx->has_scene_normals = false; // (until the new ones are complete)
    ctx->sn_slot_valid = false;
    TRY(grow_cloud(ctx, ctx->sn, n, false));
    launch_rows4_to_soa(nrm, (int)n, ctx->sn.x, ctx->sn.y, ctx->sn.z, ctx->st);
    LAUNCHCHK("scene_normals_rows");
    TRY(normals_finish(ctx, n, k, "scene", degenerate));
    ctx->has_scene_normals = true;
    return ICP_OK;
}

} // extern "C"
