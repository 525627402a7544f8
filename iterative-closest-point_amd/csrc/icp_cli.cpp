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
//   --trim F           trimmed ICP (icp_set_trim): each iteration keeps the fraction F (0 < F <= 1) of the
//                      pairs with the smallest distances, the expected overlap; combines with --max-dist,
//                      --normals, --robust and --pyramid (each level trimmed by the same fraction)
//   --one-to-one       one-to-one correspondences (icp_set_one_to_one): of the scene points that chose one model
//                      point only the closest is a pair (ties whole); no parameter; combines with --max-dist,
//                      --trim, --robust, every metric and --pyramid
//   --normals FILE     the model's normals, a CSV in the clouds' format with one row per model point:
//                      selects the point-to-plane metric (combines with --max-dist; no scale)
//   --estimate-normals K  the model's normals estimated from its own K nearest neighbours (3 <= K <= 64,
//                      K <= the model's size; icp_estimate_model_normals): the same metric as --normals,
//                      which it excludes
//   --symmetric        the symmetric point-to-plane iteration (icp_set_plane_symmetric): needs one source of
//                      model normals (--normals | --estimate-normals) and one of scene normals
//                      (--scene-normals | --estimate-scene-normals); its error is along a sum of two normals,
//                      up to four times the one-sided metric's (--threshold compares with it)
//   --gicp             the plane-to-plane iteration of generalised ICP (icp_set_plane_to_plane): the same normals
//                      options as --symmetric, which it excludes; its error is the mean squared Mahalanobis
//                      residual (--threshold compares with it); works under --pyramid
//   --gicp-epsilon E   the covariances' eigenvalue along the normal, 0 < E <= 1 (default 1e-3, PCL's and
//                      Open3D's); needs --gicp
//   --scene-normals FILE  the scene's normals, a CSV in the clouds' format with one row per scene point, in
//                      the frame of the scene file; excludes --estimate-scene-normals and --pyramid
//   --estimate-scene-normals K  the scene's normals estimated from its own K nearest neighbours (3 <= K <= 64,
//                      K <= the scene's size; icp_estimate_scene_normals); with --pyramid per level
//   --write-scene-normals FILE  writes the scene's current normals after the run (icp_get_scene_normals)
//   --robust huber|tukey|cauchy  robust weights on the kept pairs (icp_set_robust): needs --robust-k
//   --robust-k K       the weights' scale, in the clouds' units (> 0); needs --robust
//   --write-normals FILE  writes the normals the run used (either option's) in the clouds' format
//   --pyramid H1[,H2,...]  coarse-to-fine: for each voxel size in the order given, both clouds are
//                      downsampled (icp_voxel_downsample), set with the unequal-size check lifted, the scene
//                      moved by the pose so far (icp_transform_scene), registered with the run's own settings
//                      and the total taken (icp_get_transform); then the full clouds from that pose.  One
//                      "[pyramid] level ..." line per level and a "[pyramid] total ..." line go to stderr.
//                      With --estimate-normals the normals are estimated per level; excludes --normals
//   --pyramid-iters K  iterations per level (default nb_iter)
//   --global H         global registration first (icp_global_pose): both clouds downsampled to voxel H, FPFH
//                      descriptors, mutual feature matches and a RANSAC pose, applied to the scene with
//                      icp_transform_scene before the first run (so it is part of --write-transform's total);
//                      for a scene that does not start near its answer.  One "[global] model ... scene ...
//                      matches ... evaluated ... inliers ... hypothesis ..." line goes to stderr.  Combines
//                      with every other option; under --pyramid it is the pyramid's initial pose
//   --global-k K       neighbours of a descriptor (default 32), --global-normals-k K of a normal (default 16):
//                      integers in [3, 64]
//   --global-hyp N     RANSAC hypotheses (default 100000), --global-seed S their seed (default 0)
//   --global-dist X    a pair counts as an inlier within X (default 1.5 H)
//   --sor K,RATIO      statistical outlier removal (icp_filter_statistical) of the model and of the scene right
//                      after loading, before --global, --pyramid and any normal estimation: a point stays when
//                      its mean distance to its K nearest neighbours (2 <= K <= 63) is at most mu + RATIO sigma
//                      of those means (RATIO >= 0).  The clouds' sizes will differ afterwards, so it needs
//                      --allow-unequal.  Rows of --normals / --scene-normals files follow their clouds: the rows
//                      of removed points are dropped.  One "[sor] model|scene N points, kept M, mu .. sigma .. T .."
//                      line per cloud goes to stderr.  The output file holds the kept scene points as
//                      registered; --write-transform is unchanged, so the pose can be applied to the full scan
//   --ror RADIUS,MIN   radius outlier removal (icp_filter_radius), likewise and after --sor when both are given:
//                      a point stays when at least MIN other points lie within RADIUS (RADIUS > 0, MIN >= 0);
//                      one "[ror] model|scene N points, kept M" line per cloud
//   --evaluate DIST    after the run (and after --global / --pyramid) the registration evaluated (icp_evaluate): the
//                      scene points with a model point within DIST (> 0, or inf) are the inliers; one "[evaluate]
//                      scene K of N within DIST, fitness .. inlier RMSE .. largest kept distance .." line goes to stderr
//   --evaluate-both    the model's side too: a second "[evaluate] model ..." line (needs --evaluate)
//   --write-information FILE  the 6 x 6 information matrix of the kept pairs (rotation block first), six
//                      comma-separated rows of 6 significant digits (needs --evaluate)
//   --write-transform FILE  the total transform q = s R p + t (icp_get_transform) as a 4 x 4 matrix
//                      [sR t; 0 0 0 1], four comma-separated rows of 6 significant digits
//   --out PATH         output file (default output.txt, src/load.cc:71)
//   --device D         HIP device ordinal (default 0)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

// K of --estimate-normals / --estimate-scene-normals: an integer in [3, 64], else the message and false
static bool parse_k(const char *option, const char *text, int *k)
{
    char *end = nullptr;
    const long v = std::strtol(text, &end, 10);
    if (end == text || *end || v < 3 || v > 64) {
        std::fprintf(stderr, "[error] %s: K = %s is not an integer in [3, 64]\n", option, text);
        return false;
    }
    *k = (int)v;
    return true;
}

int main(int argc, char **argv)
{
    const char *prog = std::strrchr(argv[0], '/') ? std::strrchr(argv[0], '/') + 1 : argv[0];
    if (argc < 4) { // main.cc:5-8
        std::printf("Usage: ./%s [path_to_ref_cloud] [path_to_transform_cloud] [nb_iter]\n", prog);
        std::printf("       options: [--max-dist X] [--trim F] [--one-to-one] [--normals FILE | --estimate-normals K] [--write-normals FILE] "
                    "[--symmetric | --gicp [--gicp-epsilon E]] [--scene-normals FILE | --estimate-scene-normals K] [--write-scene-normals FILE] "
                    "[--robust huber|tukey|cauchy --robust-k K] [--threshold X] [--pyramid H1[,H2,...]] "
                    "[--pyramid-iters K] [--global H [--global-k K] [--global-normals-k K] [--global-hyp N] [--global-seed S] "
                    "[--global-dist X]] [--sor K,RATIO] [--ror RADIUS,MIN] [--evaluate DIST [--evaluate-both] [--write-information FILE]] "
                    "[--write-transform FILE] [--out PATH]\n");
        return -1;
    }
    const int max_iter = std::atoi(argv[3]);
    bool allow_unequal = false;
    int nn_mode = ICP_NN_CERTIFIED, device = 0;
    int rule = std::strcmp(prog, "icp") == 0 ? ICP_NN_RULE_CPU_SQRT : ICP_NN_RULE_SQUARED;
    double threshold = 1e-5, max_dist = 0.0;
    const char *out = "output.txt", *normals = nullptr, *estimate = nullptr, *write_normals = nullptr;
    const char *robust = nullptr, *robust_k = nullptr, *trim = nullptr;
    const char *scene_normals = nullptr, *estimate_scene = nullptr, *write_scene_normals = nullptr;
    bool symmetric = false, gicp = false, one_to_one = false;
    const char *gicp_epsilon = nullptr;
    const char *pyramid = nullptr, *pyramid_iters = nullptr, *write_transform = nullptr;
    const char *global = nullptr, *global_k = nullptr, *global_nk = nullptr, *global_hyp = nullptr, *global_seed = nullptr;
    const char *global_dist = nullptr, *sor = nullptr, *ror = nullptr;
    const char *evaluate = nullptr, *write_information = nullptr;
    bool evaluate_both = false;
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
        else if (!std::strcmp(argv[a], "--trim") && a + 1 < argc) trim = argv[++a];
        else if (!std::strcmp(argv[a], "--one-to-one")) one_to_one = true;
        else if (!std::strcmp(argv[a], "--normals") && a + 1 < argc) normals = argv[++a];
        else if (!std::strcmp(argv[a], "--estimate-normals") && a + 1 < argc) estimate = argv[++a];
        else if (!std::strcmp(argv[a], "--write-normals") && a + 1 < argc) write_normals = argv[++a];
        else if (!std::strcmp(argv[a], "--symmetric")) symmetric = true;
        else if (!std::strcmp(argv[a], "--gicp")) gicp = true;
        else if (!std::strcmp(argv[a], "--gicp-epsilon") && a + 1 < argc) gicp_epsilon = argv[++a];
        else if (!std::strcmp(argv[a], "--scene-normals") && a + 1 < argc) scene_normals = argv[++a];
        else if (!std::strcmp(argv[a], "--estimate-scene-normals") && a + 1 < argc) estimate_scene = argv[++a];
        else if (!std::strcmp(argv[a], "--write-scene-normals") && a + 1 < argc) write_scene_normals = argv[++a];
        else if (!std::strcmp(argv[a], "--robust") && a + 1 < argc) robust = argv[++a];
        else if (!std::strcmp(argv[a], "--robust-k") && a + 1 < argc) robust_k = argv[++a];
        else if (!std::strcmp(argv[a], "--pyramid") && a + 1 < argc) pyramid = argv[++a];
        else if (!std::strcmp(argv[a], "--pyramid-iters") && a + 1 < argc) pyramid_iters = argv[++a];
        else if (!std::strcmp(argv[a], "--global") && a + 1 < argc) global = argv[++a];
        else if (!std::strcmp(argv[a], "--global-k") && a + 1 < argc) global_k = argv[++a];
        else if (!std::strcmp(argv[a], "--global-normals-k") && a + 1 < argc) global_nk = argv[++a];
        else if (!std::strcmp(argv[a], "--global-hyp") && a + 1 < argc) global_hyp = argv[++a];
        else if (!std::strcmp(argv[a], "--global-seed") && a + 1 < argc) global_seed = argv[++a];
        else if (!std::strcmp(argv[a], "--global-dist") && a + 1 < argc) global_dist = argv[++a];
        else if (!std::strcmp(argv[a], "--sor") && a + 1 < argc) sor = argv[++a];
        else if (!std::strcmp(argv[a], "--ror") && a + 1 < argc) ror = argv[++a];
        else if (!std::strcmp(argv[a], "--evaluate") && a + 1 < argc) evaluate = argv[++a];
        else if (!std::strcmp(argv[a], "--evaluate-both")) evaluate_both = true;
        else if (!std::strcmp(argv[a], "--write-information") && a + 1 < argc) write_information = argv[++a];
        else if (!std::strcmp(argv[a], "--write-transform") && a + 1 < argc) write_transform = argv[++a];
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
        if (!parse_k("--estimate-normals", estimate, &est_k)) return -1;
        if (normals) {
            std::fprintf(stderr, "[error] --estimate-normals and --normals exclude each other\n");
            return -1;
        }
    }
    if (write_normals && !normals && !estimate) {
        std::fprintf(stderr, "[error] --write-normals needs --normals or --estimate-normals\n");
        return -1;
    }

    // the scene normals' options and the symmetric switch, likewise
    int est_scene_k = 0;
    if (estimate_scene) {
        if (!parse_k("--estimate-scene-normals", estimate_scene, &est_scene_k)) return -1;
        if (scene_normals) {
            std::fprintf(stderr, "[error] --estimate-scene-normals and --scene-normals exclude each other\n");
            return -1;
        }
    }
    if (symmetric && (!(normals || estimate) || !(scene_normals || estimate_scene))) {
        std::fprintf(stderr, "[error] --symmetric needs the model's normals (--normals or --estimate-normals) and the "
                             "scene's (--scene-normals or --estimate-scene-normals)\n");
        return -1;
    }
    // the plane-to-plane switch: the same normals, never with --symmetric
    double gicp_eps = 1e-3;
    if (gicp_epsilon) {
        char *end = nullptr;
        gicp_eps = std::strtod(gicp_epsilon, &end);
        if (end == gicp_epsilon || *end || !(gicp_eps > 0.0 && gicp_eps <= 1.0)) {
            std::fprintf(stderr, "[error] --gicp-epsilon: %s is not a number in (0, 1]\n", gicp_epsilon);
            return -1;
        }
        if (!gicp) {
            std::fprintf(stderr, "[error] --gicp-epsilon needs --gicp\n");
            return -1;
        }
    }
    if (gicp && symmetric) {
        std::fprintf(stderr, "[error] --gicp and --symmetric exclude each other\n");
        return -1;
    }
    if (gicp && (!(normals || estimate) || !(scene_normals || estimate_scene))) {
        std::fprintf(stderr, "[error] --gicp needs the model's normals (--normals or --estimate-normals) and the "
                             "scene's (--scene-normals or --estimate-scene-normals)\n");
        return -1;
    }
    if (write_scene_normals && !scene_normals && !estimate_scene) {
        std::fprintf(stderr, "[error] --write-scene-normals needs --scene-normals or --estimate-scene-normals\n");
        return -1;
    }

    double trim_fraction = 1.0;
    if (trim) {
        char *end = nullptr;
        trim_fraction = std::strtod(trim, &end);
        if (end == trim || *end) {
            std::fprintf(stderr, "[error] --trim: %s is not a number\n", trim);
            return -1;
        }
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

    // the pyramid's options: the list of voxel sizes (each a number > 0, no empty entry), the levels'
    // iterations; --normals' rows belong to the full model
    std::vector<double> voxels;
    int level_iter = max_iter;
    if (pyramid) {
        for (const char *q = pyramid;;) {
            char *end = nullptr;
            const double h = std::strtod(q, &end);
            if (end == q || (*end && *end != ',') || !(h > 0.0) || h > 1.7e308) {
                std::fprintf(stderr, "[error] --pyramid: %s is not a list of voxel sizes > 0\n", pyramid);
                return -1;
            }
            voxels.push_back(h);
            if (!*end) break;
            q = end + 1;
        }
        if (normals) {
            std::fprintf(stderr, "[error] --pyramid and --normals exclude each other (the file's rows belong to the "
                                 "full model): use --estimate-normals\n");
            return -1;
        }
        if (scene_normals) {
            std::fprintf(stderr, "[error] --pyramid and --scene-normals exclude each other (the file's rows belong to the "
                                 "full scene): use --estimate-scene-normals\n");
            return -1;
        }
    }
    if (pyramid_iters) {
        char *end = nullptr;
        const long v = std::strtol(pyramid_iters, &end, 10);
        if (!pyramid || end == pyramid_iters || *end || v < 0 || v > 1000000) {
            std::fprintf(stderr, "[error] --pyramid-iters: needs --pyramid and an integer >= 0\n");
            return -1;
        }
        level_iter = (int)v;
    }

    // the global registration's options: the voxel and what goes with it
    icp_global_params gprm{};
    gprm.mutual = 1;
    if (!global && (global_k || global_nk || global_hyp || global_seed || global_dist)) {
        std::fprintf(stderr, "[error] --global-k, --global-normals-k, --global-hyp, --global-seed and --global-dist need --global\n");
        return -1;
    }
    if (global) {
        char *end = nullptr;
        gprm.voxel = std::strtod(global, &end);
        if (end == global || *end || !(gprm.voxel > 0.0) || gprm.voxel > 1.7e308) {
            std::fprintf(stderr, "[error] --global: %s is not a voxel size > 0\n", global);
            return -1;
        }
        if (global_k && !parse_k("--global-k", global_k, &gprm.k_fpfh)) return -1;
        if (global_nk && !parse_k("--global-normals-k", global_nk, &gprm.k_normals)) return -1;
        if (global_hyp) {
            gprm.hypotheses = std::strtoll(global_hyp, &end, 10);
            if (end == global_hyp || *end || gprm.hypotheses < 1 || gprm.hypotheses >= (1LL << 32)) {
                std::fprintf(stderr, "[error] --global-hyp: %s is not an integer in [1, 2^32)\n", global_hyp);
                return -1;
            }
        }
        if (global_seed) {
            gprm.seed = std::strtoull(global_seed, &end, 10);
            if (end == global_seed || *end || global_seed[0] == '-') {
                std::fprintf(stderr, "[error] --global-seed: %s is not an unsigned integer\n", global_seed);
                return -1;
            }
        }
        if (global_dist) {
            gprm.max_dist = std::strtod(global_dist, &end);
            if (end == global_dist || *end || !(gprm.max_dist > 0.0) || gprm.max_dist > 1.7e308) {
                std::fprintf(stderr, "[error] --global-dist: %s is not a distance > 0\n", global_dist);
                return -1;
            }
        }
    }

    // the outlier filters' options: two values each, and the clouds' sizes will differ afterwards
    int sor_k = 0, ror_min = 0;
    double sor_ratio = 0.0, ror_radius = 0.0;
    if (sor) {
        char *end = nullptr, *end2 = nullptr;
        const long v = std::strtol(sor, &end, 10);
        if (end != sor && *end == ',') sor_ratio = std::strtod(end + 1, &end2);
        if (end == sor || *end != ',' || end2 == end + 1 || *end2 || v < 2 || v > 63 || !(sor_ratio >= 0.0) ||
            sor_ratio > 1.7e308) {
            std::fprintf(stderr, "[error] --sor: %s is not K,RATIO with an integer K in [2, 63] and a RATIO >= 0\n", sor);
            return -1;
        }
        sor_k = (int)v;
    }
    if (ror) {
        char *end = nullptr, *end2 = nullptr;
        ror_radius = std::strtod(ror, &end);
        long v = -1;
        if (end != ror && *end == ',') v = std::strtol(end + 1, &end2, 10);
        if (end == ror || *end != ',' || end2 == end + 1 || *end2 || !(ror_radius > 0.0) || ror_radius > 1.7e308 || v < 0 ||
            v > 2147483647L) {
            std::fprintf(stderr, "[error] --ror: %s is not RADIUS,MIN with a RADIUS > 0 and an integer MIN >= 0\n", ror);
            return -1;
        }
        ror_min = (int)v;
    }
    if ((sor || ror) && !allow_unequal) {
        std::fprintf(stderr, "[error] --sor and --ror remove points from each cloud on its own, so the clouds' sizes will "
                             "differ: they need --allow-unequal\n");
        return -1;
    }

    // the evaluation's options: a distance > 0 (inf: every pair), and what needs it
    double eval_dist = 0.0;
    if (evaluate) {
        char *end = nullptr;
        eval_dist = std::strtod(evaluate, &end);
        if (end == evaluate || *end || !(eval_dist > 0.0)) {
            std::fprintf(stderr, "[error] --evaluate: %s is not a distance > 0 (or inf)\n", evaluate);
            return -1;
        }
    } else if (evaluate_both || write_information) {
        std::fprintf(stderr, "[error] --evaluate-both and --write-information need --evaluate\n");
        return -1;
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

    size_t nsn = 0;
    double *snrm = scene_normals ? load_or_exit(scene_normals, &nsn) : nullptr;
    if (scene_normals && nsn != np) {
        std::fprintf(stderr, "[error] --scene-normals: %zu rows for a scene of %zu points\n", nsn, np);
        return -1;
    }
    if (estimate_scene && (size_t)est_scene_k > np) {
        std::fprintf(stderr, "[error] --estimate-scene-normals: K = %d exceeds the scene's %zu points\n", est_scene_k, np);
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
    if ((rc = icp_set_trim(ctx, trim_fraction)) != ICP_OK) {
        std::fprintf(stderr, "[error] --trim: %s (a fraction in (0, 1])\n", icp_strerror(rc));
        return 3;
    }
    if ((rc = icp_set_one_to_one(ctx, one_to_one ? 1 : 0)) != ICP_OK) {
        std::fprintf(stderr, "[error] --one-to-one: %s\n", icp_strerror(rc));
        return 3;
    }
    if ((rc = icp_set_robust(ctx, robust_kind, robust_scale)) != ICP_OK) {
        std::fprintf(stderr, "[error] --robust-k: %s\n", icp_strerror(rc));
        return 3;
    }
    const auto die = [&](const char *what) {
        std::fprintf(stderr, "[error] %s: %s: %s\n", what, icp_strerror(rc), icp_last_error(ctx));
        return 3;
    };
    if ((rc = icp_set_plane_symmetric(ctx, symmetric ? 1 : 0)) != ICP_OK) return die("--symmetric");
    if ((rc = icp_set_plane_to_plane(ctx, gicp ? gicp_eps : 0.0)) != ICP_OK) return die("--gicp");
    // --write-normals / --write-scene-normals: a cloud's current normals, the clouds' format
    const auto write_normals_file = [&](const char *option, int (*get)(icp_ctx *, double *), size_t rows, const char *path) {
        std::vector<double> nout(3 * rows);
        if ((rc = get(ctx, nout.data())) != ICP_OK) return die(option);
        if (icp_write_matrix(path, nout.data(), rows) != ICP_OK) {
            std::fprintf(stderr, "[error] cannot write %s\n", path);
            return 2;
        }
        return 0;
    };
    const auto write_total = [&]() { // --write-transform: [sR t; 0 0 0 1] in the CSV style
        double s = 1.0, R[9], t[3];
        if ((rc = icp_get_transform(ctx, &s, R, t)) != ICP_OK) return die("--write-transform");
        FILE *f = std::fopen(write_transform, "w");
        if (!f) {
            std::fprintf(stderr, "[error] cannot write %s\n", write_transform);
            return 2;
        }
        for (int r = 0; r < 3; ++r)
            std::fprintf(f, "%g,%g,%g,%g\n", s * R[3 * r], s * R[3 * r + 1], s * R[3 * r + 2], t[r]);
        std::fprintf(f, "0,0,0,1\n");
        std::fclose(f);
        return 0;
    };
    // --evaluate: the registration as it ends, its line(s) and --write-information's matrix in the CSV style
    const auto evaluate_now = [&]() {
        icp_evaluation ev{};
        if ((rc = icp_evaluate(ctx, eval_dist, evaluate_both ? 1 : 0, &ev, nullptr, nullptr, nullptr, nullptr)) != ICP_OK)
            return die("--evaluate");
        std::fprintf(stderr, "[evaluate] scene %lld of %lld within %g, fitness %g inlier RMSE %g largest kept distance %g\n",
                     ev.correspondences, ev.scene_points, eval_dist, ev.fitness, ev.inlier_rmse, std::sqrt(ev.max_inlier_d2));
        if (evaluate_both)
            std::fprintf(stderr, "[evaluate] model %lld of %lld within %g, fitness %g inlier RMSE %g largest kept distance %g\n",
                         ev.model_correspondences, ev.model_points, eval_dist, ev.model_fitness, ev.model_rmse,
                         std::sqrt(ev.model_max_inlier_d2));
        if (write_information) {
            FILE *f = std::fopen(write_information, "w");
            bool ok = f != nullptr;
            for (int r = 0; ok && r < 6; ++r) {
                const double *a = ev.information + 6 * r;
                ok = std::fprintf(f, "%g,%g,%g,%g,%g,%g\n", a[0], a[1], a[2], a[3], a[4], a[5]) > 0;
            }
            if (f && std::fclose(f) != 0) ok = false; // (a full disk shows here at the latest)
            if (!ok) {
                std::fprintf(stderr, "[error] cannot write %s\n", write_information);
                return 2;
            }
        }
        return 0;
    };
    // What a run ends with: the files asked for, the moved scene, the [output] line.  get_scene: how a
    // failing icp_get_scene is named (null: not at all).
    const auto finish = [&](double *errs, const char *get_scene) {
        int w = 0;
        if (evaluate && (w = evaluate_now()) != 0) return w;
        if (write_scene_normals &&
            (w = write_normals_file("--write-scene-normals", icp_get_scene_normals, np, write_scene_normals)) != 0)
            return w;
        if (write_transform && (w = write_total()) != 0) return w;
        if ((rc = icp_get_scene(ctx, p)) != ICP_OK) {
            if (get_scene) return die(get_scene);
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
        icp_free(snrm);
        return 0;
    };
    // --sor, then --ror: each cloud on its own, right after loading; a normals file's rows follow the mask
    if (sor || ror) {
        const auto filter_cloud = [&](const char *word, double *xyz, size_t *n, double *rows) {
            for (int pass = 0; pass < 2; ++pass) {
                if (!(pass == 0 ? sor : ror)) continue;
                std::vector<double> kept_xyz(3 * *n);
                std::vector<uint8_t> mask(*n);
                size_t kept = 0;
                double st[3] = {0.0, 0.0, 0.0};
                rc = pass == 0 ? icp_filter_statistical(ctx, xyz, *n, sor_k, sor_ratio, kept_xyz.data(), mask.data(), &kept,
                                                        nullptr, st)
                               : icp_filter_radius(ctx, xyz, *n, ror_radius, ror_min, kept_xyz.data(), mask.data(), &kept,
                                                   nullptr);
                if (rc != ICP_OK) return false;
                if (pass == 0)
                    std::fprintf(stderr, "[sor] %s %zu points, kept %zu, mu %g sigma %g T %g\n", word, *n, kept, st[0], st[1],
                                 st[2]);
                else std::fprintf(stderr, "[ror] %s %zu points, kept %zu\n", word, *n, kept);
                std::memcpy(xyz, kept_xyz.data(), sizeof(double) * 3 * kept);
                if (rows) {
                    size_t w = 0;
                    for (size_t j = 0; j < *n; ++j)
                        if (mask[j]) {
                            for (int a = 0; a < 3; ++a) rows[3 * w + a] = rows[3 * j + a];
                            ++w;
                        }
                }
                *n = kept;
                if (kept == 0) break; // (the size check below answers)
            }
            return true;
        };
        if (!filter_cloud("model", m, &nm, nrm)) return die("--sor / --ror (model)");
        if (!filter_cloud("scene", p, &np, snrm)) return die("--sor / --ror (scene)");
        if (normals) nn = nm;
        if (scene_normals) nsn = np;
        if (np < 4 || nm < 1) {
            std::fprintf(stderr, "[error] --sor / --ror left %zu model and %zu scene points: need at least 4 point pairs\n", nm,
                         np);
            return -1;
        }
    }
    // --global: the pose of the full clouds' global registration, before anything is resident
    double g_R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, g_t[3] = {0, 0, 0};
    if (global) {
        icp_global_report rep{};
        if ((rc = icp_global_pose(ctx, m, nm, p, np, &gprm, g_R, g_t, &rep)) != ICP_OK) return die("--global");
        std::fprintf(stderr, "[global] model %lld scene %lld points, matches %lld, evaluated %lld, inliers %lld, hypothesis %lld\n",
                     rep.model_points, rep.scene_points, rep.matches, rep.evaluated, rep.inliers, rep.best_h);
    }
    if (pyramid) {
        // The calls of icp_amd.register_pyramid, in its order: every level's clouds first, then per
        // level (and for the full clouds) set_allow_unequal, set_model, [estimate], set_scene,
        // transform_scene by the pose so far, run, get_transform.
        struct Level {
            double h;
            std::vector<double> m, p;
        };
        std::vector<Level> levels(voxels.size());
        for (size_t l = 0; l < voxels.size(); ++l) {
            Level &L = levels[l];
            L.h = voxels[l];
            L.m.resize(3 * nm);
            L.p.resize(3 * np);
            size_t cm = 0, cp = 0;
            if ((rc = icp_voxel_downsample(ctx, m, nm, L.h, nullptr, L.m.data(), nullptr, &cm)) != ICP_OK ||
                (rc = icp_voxel_downsample(ctx, p, np, L.h, nullptr, L.p.data(), nullptr, &cp)) != ICP_OK)
                return die("--pyramid");
            L.m.resize(3 * cm);
            L.p.resize(3 * cp);
        }
        // an estimator's K against every level's cloud
        const auto k_fits = [&](const char *option, int k, const char *word, std::vector<double> Level::*cloud) {
            for (const Level &L : levels)
                if ((L.*cloud).size() / 3 < (size_t)k) {
                    std::fprintf(stderr, "[error] %s: K = %d exceeds the %zu %s points of the level h=%g\n", option, k,
                                 (L.*cloud).size() / 3, word, L.h);
                    return false;
                }
            return true;
        };
        if (estimate && !k_fits("--estimate-normals", est_k, "model", &Level::m)) return -1;
        if (estimate_scene && !k_fits("--estimate-scene-normals", est_scene_k, "scene", &Level::p)) return -1;
        if (estimate && (rc = icp_set_metric(ctx, ICP_METRIC_POINT_TO_PLANE)) != ICP_OK) return die("--estimate-normals");
        double s = 1.0, R[9], t[3]; // (the identity, or --global's pose)
        std::memcpy(R, g_R, sizeof(R));
        std::memcpy(t, g_t, sizeof(t));
        double *errs = (double *)std::calloc((size_t)(max_iter > level_iter ? max_iter : level_iter) + 1, sizeof(double));
        icp_result res{};
        for (size_t l = 0; l <= levels.size(); ++l) {
            const bool full = l == levels.size();
            const double *lm = full ? m : levels[l].m.data(), *lp = full ? p : levels[l].p.data();
            const size_t lnm = full ? nm : levels[l].m.size() / 3, lnp = full ? np : levels[l].p.size() / 3;
            icp_set_allow_unequal(ctx, full ? (allow_unequal ? 1 : 0) : 1);
            if ((rc = icp_set_model(ctx, lm, lnm)) != ICP_OK) return die("--pyramid");
            if (estimate && (rc = icp_estimate_model_normals(ctx, est_k, nullptr, nullptr)) != ICP_OK)
                return die("--estimate-normals");
            if ((rc = icp_set_scene(ctx, lp, lnp, lnp)) != ICP_OK) return die("--pyramid");
            if (estimate_scene && (rc = icp_estimate_scene_normals(ctx, est_scene_k, nullptr, nullptr)) != ICP_OK)
                return die("--estimate-scene-normals");
            if ((rc = icp_transform_scene(ctx, s, R, t)) != ICP_OK) return die("--pyramid");
            if (full) // the fine run's lines, as a plain run prints them
                icp_set_progress(
                    ctx,
                    [](int i, double e, void *) { std::fprintf(stderr, "[ICP] iteration number %d | error value = %g\n", i, e); },
                    nullptr);
            if ((rc = icp_run(ctx, full ? max_iter : level_iter, threshold, errs, &res)) != ICP_OK) return die("icp_run");
            if ((rc = icp_get_transform(ctx, &s, R, t)) != ICP_OK) return die("--pyramid");
            if (!full)
                std::fprintf(stderr, "[pyramid] level h=%g model %zu scene %zu points, %d iterations, err %g\n", levels[l].h,
                             lnm, lnp, res.iterations, res.err);
        }
        std::fprintf(stderr, "[pyramid] total s=%.17g R=%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g t=%.17g,%.17g,%.17g\n", s,
                     R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], t[0], t[1], t[2]);
        if (write_normals) {
            const int w = write_normals_file("--write-normals", icp_get_model_normals, nm, write_normals);
            if (w) return w;
        }
        return finish(errs, "icp_get_scene");
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
    if (scene_normals && (rc = icp_set_scene_normals(ctx, snrm, nsn)) != ICP_OK) return die("--scene-normals");
    if (estimate_scene) {
        long long degenerate = 0;
        if ((rc = icp_estimate_scene_normals(ctx, est_scene_k, nullptr, &degenerate)) != ICP_OK)
            return die("--estimate-scene-normals");
        std::fprintf(stderr, "[normals] the scene's estimated from %d neighbours; %lld of %zu undetermined (zero)\n",
                     est_scene_k, degenerate, np);
    }
    if (write_normals) {
        const int w = write_normals_file("--write-normals", icp_get_model_normals, nm, write_normals);
        if (w) return w;
    }
    // (after the estimates: icp_estimate_scene_normals needs the scene as icp_set_scene received it)
    if (global && (rc = icp_transform_scene(ctx, 1.0, g_R, g_t)) != ICP_OK) return die("--global");
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
    return finish(errs, nullptr);
}
