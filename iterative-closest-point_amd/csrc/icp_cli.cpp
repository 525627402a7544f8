// icp_cli.cpp — `icp-gpu` / `icp` command line (src/GPU/main.cc:3-21, src/main.cc:6-25).
//
//   icp-gpu <path_to_ref_cloud> <path_to_transform_cloud> <nb_iter> [options]
//
// Same positional contract, stderr lines ([load] / [ICP] / [output]), ./output.txt and
// exit codes as the reference.  Both binaries run the HIP engine (there is no CPU
// fallback in the product).  `icp` keeps the reference CPU path's NN rule (src/main.cc ->
// cpu.cc:17-22: first minimum of sqrt(pow() sums), ICP_NN_RULE_CPU_SQRT) and `icp-gpu` the GPU
// path's (compute.cu:112-117: squared distances); they differ only at near ties.
// Options (after the positionals):
//   --rule cpu|squared override the binary's NN rule
//   --allow-unequal    run even when the clouds differ in size (reference: exit 255)
//   --nn fp64|certified  NN arithmetic (default certified; identical results)
//   --threshold X      convergence threshold (default 1e-5, src/cpu.hh:113)
//   --max-dist X       max correspondence distance: pairs farther apart than X are left out of
//                      each iteration's alignment and error (partial overlap; default: none)
//   --normals FILE     the model's normals, a CSV in the clouds' format with one row per model point:
//                      selects the point-to-plane metric (combines with --max-dist; no scale)
//   --estimate-normals K  the model's normals estimated from its own K nearest neighbours (3 <= K <= 64,
//                      K <= the model's size; icp_estimate_model_normals): the same metric as --normals,
//                      which it excludes
//   --robust huber|tukey|cauchy  robust weights on the kept pairs (icp_set_robust): needs --robust-k
//   --robust-k K       the weights' scale, in the clouds' units (> 0); needs --robust
//   --write-normals FILE  writes the normals the run used (either option's) in the clouds' format
//   --out PATH         output file (default output.txt, src/load.cc:71)
//   --device D         HIP device ordinal (default 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/icp_capi.h"

static double *load_or_exit(const char *path, size_t *n)
{
    std::fprintf(stderr, "[load] opening %s\n", path); // load.cc:8
    double *xyz = nullptr;
    if (icp_load_matrix(path, &xyz, n) != ICP_OK) {
        std::fprintf(stderr, "[load] %s could not be opened\n", path); // load.cc:11-13
        std::exit(2);
    }
    std::fprintf(stderr, "[load] loading file into matrix\n"); // load.cc:19
    return xyz;
}

int main(int argc, char **argv)
{
    const char *prog = std::strrchr(argv[0], '/') ? std::strrchr(argv[0], '/') + 1 : argv[0];
    if (argc < 4) { // main.cc:5-8
        std::printf("Usage: ./%s [path_to_ref_cloud] [path_to_transform_cloud] [nb_iter]\n", prog);
        std::printf("       options: [--max-dist X] [--normals FILE | --estimate-normals K] [--write-normals FILE] "
                    "[--robust huber|tukey|cauchy --robust-k K] [--threshold X] [--out PATH]\n");
        return -1;
    }
    const int max_iter = std::atoi(argv[3]);
    bool allow_unequal = false;
    int nn_mode = ICP_NN_CERTIFIED, device = 0;
    int rule = std::strcmp(prog, "icp") == 0 ? ICP_NN_RULE_CPU_SQRT : ICP_NN_RULE_SQUARED;
    double threshold = 1e-5, max_dist = 0.0;
    const char *out = "output.txt", *normals = nullptr, *estimate = nullptr, *write_normals = nullptr;
    const char *robust = nullptr, *robust_k = nullptr;
    for (int a = 4; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--allow-unequal")) allow_unequal = true;
        else if (!std::strcmp(argv[a], "--nn") && a + 1 < argc) {
            ++a;
            nn_mode = !std::strcmp(argv[a], "fp64") ? ICP_NN_FP64 : ICP_NN_CERTIFIED;
        } else if (!std::strcmp(argv[a], "--rule") && a + 1 < argc) {
            ++a;
            rule = !std::strcmp(argv[a], "cpu") ? ICP_NN_RULE_CPU_SQRT : ICP_NN_RULE_SQUARED;
        } else if (!std::strcmp(argv[a], "--threshold") && a + 1 < argc) threshold = std::atof(argv[++a]);
        else if (!std::strcmp(argv[a], "--max-dist") && a + 1 < argc) max_dist = std::atof(argv[++a]);
        else if (!std::strcmp(argv[a], "--normals") && a + 1 < argc) normals = argv[++a];
        else if (!std::strcmp(argv[a], "--estimate-normals") && a + 1 < argc) estimate = argv[++a];
        else if (!std::strcmp(argv[a], "--write-normals") && a + 1 < argc) write_normals = argv[++a];
        else if (!std::strcmp(argv[a], "--robust") && a + 1 < argc) robust = argv[++a];
        else if (!std::strcmp(argv[a], "--robust-k") && a + 1 < argc) robust_k = argv[++a];
        else if (!std::strcmp(argv[a], "--out") && a + 1 < argc) out = argv[++a];
        else if (!std::strcmp(argv[a], "--device") && a + 1 < argc) device = std::atoi(argv[++a]);
        else {
            std::fprintf(stderr, "[error] unknown option %s\n", argv[a]);
            return -1;
        }
    }

    // the normals' options, checked before any file or device is touched
    int est_k = 0;
    if (estimate) {
        char *end = nullptr;
        const long v = std::strtol(estimate, &end, 10);
        if (end == estimate || *end || v < 3 || v > 64) {
            std::fprintf(stderr, "[error] --estimate-normals: K = %s is not an integer in [3, 64]\n", estimate);
            return -1;
        }
        est_k = (int)v;
        if (normals) {
            std::fprintf(stderr, "[error] --estimate-normals and --normals exclude each other\n");
            return -1;
        }
    }
    if (write_normals && !normals && !estimate) {
        std::fprintf(stderr, "[error] --write-normals needs --normals or --estimate-normals\n");
        return -1;
    }

    // the robust weights' options: a kind and its scale come together
    int robust_kind = ICP_ROBUST_NONE;
    double robust_scale = 0.0;
    if (robust || robust_k) {
        if (!robust || !robust_k) {
            std::fprintf(stderr, "[error] --robust and --robust-k need each other\n");
            return -1;
        }
        robust_kind = !std::strcmp(robust, "huber")    ? ICP_ROBUST_HUBER
                      : !std::strcmp(robust, "tukey")  ? ICP_ROBUST_TUKEY
                      : !std::strcmp(robust, "cauchy") ? ICP_ROBUST_CAUCHY
                                                       : ICP_ROBUST_NONE;
        char *end = nullptr;
        robust_scale = std::strtod(robust_k, &end);
        if (robust_kind == ICP_ROBUST_NONE) {
            std::fprintf(stderr, "[error] --robust: %s is not huber, tukey or cauchy\n", robust);
            return -1;
        }
        if (end == robust_k || *end) {
            std::fprintf(stderr, "[error] --robust-k: %s is not a number\n", robust_k);
            return -1;
        }
    }

    size_t nm = 0, np = 0;
    double *m = load_or_exit(argv[1], &nm);
    double *p = load_or_exit(argv[2], &np);

    size_t nn = 0;
    double *nrm = normals ? load_or_exit(normals, &nn) : nullptr;
    if (normals && nn != nm) {
        std::fprintf(stderr, "[error] --normals: %zu rows for a model of %zu points\n", nn, nm);
        return -1;
    }

    if (estimate && (size_t)est_k > nm) {
        std::fprintf(stderr, "[error] --estimate-normals: K = %d exceeds the model's %zu points\n", est_k, nm);
        return -1;
    }

    // alignement_check (cpu.cc:42-53 / gpu.cc:54-62): message + exit(-1)
    if (np != nm && !allow_unequal) {
        std::fprintf(stderr, "[error] Point sets need to have the same number of points.\n");
        return -1;
    }
    if (np < 4) {
        std::fprintf(stderr, "[error] Need at least 4 point pairs\n");
        return -1;
    }

    icp_ctx *ctx = nullptr;
    int rc = icp_ctx_create(device, nn_mode, &ctx);
    if (rc != ICP_OK) {
        std::fprintf(stderr, "[error] %s\n", icp_strerror(rc));
        return 3;
    }
    icp_set_allow_unequal(ctx, allow_unequal ? 1 : 0);
    icp_set_nn_rule(ctx, rule);
    if ((rc = icp_set_max_distance(ctx, max_dist)) != ICP_OK) {
        std::fprintf(stderr, "[error] --max-dist: %s\n", icp_strerror(rc));
        return 3;
    }
    if ((rc = icp_set_robust(ctx, robust_kind, robust_scale)) != ICP_OK) {
        std::fprintf(stderr, "[error] --robust-k: %s\n", icp_strerror(rc));
        return 3;
    }
    if ((rc = icp_set_model(ctx, m, nm)) != ICP_OK || (rc = icp_set_scene(ctx, p, np, np)) != ICP_OK) {
        std::fprintf(stderr, "[error] %s: %s\n", icp_strerror(rc), icp_last_error(ctx));
        return 3;
    }
    if (normals && ((rc = icp_set_model_normals(ctx, nrm, nn)) != ICP_OK ||
                    (rc = icp_set_metric(ctx, ICP_METRIC_POINT_TO_PLANE)) != ICP_OK)) {
        std::fprintf(stderr, "[error] --normals: %s: %s\n", icp_strerror(rc), icp_last_error(ctx));
        return 3;
    }
    if (estimate) {
        long long degenerate = 0;
        if ((rc = icp_estimate_model_normals(ctx, est_k, nullptr, &degenerate)) != ICP_OK ||
            (rc = icp_set_metric(ctx, ICP_METRIC_POINT_TO_PLANE)) != ICP_OK) {
            std::fprintf(stderr, "[error] --estimate-normals: %s: %s\n", icp_strerror(rc), icp_last_error(ctx));
            return 3;
        }
        std::fprintf(stderr, "[normals] estimated from %d neighbours; %lld of %zu undetermined (zero)\n", est_k,
                     degenerate, nm);
    }
    if (write_normals) {
        double *nout = (double *)std::malloc(sizeof(double) * 3 * nm);
        if (!nout || (rc = icp_get_model_normals(ctx, nout)) != ICP_OK) {
            std::fprintf(stderr, "[error] --write-normals: %s: %s\n", icp_strerror(rc), icp_last_error(ctx));
            return 3;
        }
        if (icp_write_matrix(write_normals, nout, nm) != ICP_OK) {
            std::fprintf(stderr, "[error] cannot write %s\n", write_normals);
            return 2;
        }
        std::free(nout);
    }
    double *errs = (double *)std::calloc(max_iter > 0 ? (size_t)max_iter : 1, sizeof(double));
    icp_result res{};
    // each iteration's line as it ends (gpu.cc:65,77), from the engine's progress callback
    icp_set_progress(
        ctx, [](int i, double e, void *) { std::fprintf(stderr, "[ICP] iteration number %d | error value = %g\n", i, e); },
        nullptr);
    rc = icp_run(ctx, max_iter, threshold, errs, &res);
    if (rc != ICP_OK) {
        std::fprintf(stderr, "[error] %s: %s\n", icp_strerror(rc), icp_last_error(ctx));
        return 3;
    }
    if ((rc = icp_get_scene(ctx, p)) != ICP_OK) {
        std::fprintf(stderr, "[error] %s: %s\n", icp_strerror(rc), icp_last_error(ctx));
        return 3;
    }
    if (icp_write_matrix(out, p, np) != ICP_OK) { // load.cc:68-81
        std::fprintf(stderr, "[error] cannot write %s\n", out);
        return 2;
    }
    std::fprintf(stderr, "[output] output file \"%s\" was generated.\n", out);
    icp_ctx_destroy(ctx);
    std::free(errs);
    icp_free(m);
    icp_free(p);
    icp_free(nrm);
    return 0;
}
