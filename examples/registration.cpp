// registration.cpp — the reference's first example (examples/registration.cpp: two 640 x 480 8-D clouds, "T" = register, report,
// show the result) as a command-line program over the MI355X engine: no window, no GL buffers — the transformed cloud goes to a
// file instead of a vertex buffer.
//
//   registration                          a synthetic pair (the data files of the reference are not distributed: .MISSING_LARGE_BLOBS)
//   registration NAME                     data/NAME_1.bin, data/NAME_2.bin      (the reference's argument convention, :299-329)
//   registration A B                      data/A.bin, data/B.bin — or A and B themselves when they name existing files
//   ... [--out FILE] [--device N] [--reference-order] [--svd] [--reject-invalid] [--max-dist MM] [--trim FRACTION]
//       [--point-to-plane MU] [--colored KAPPA] [--robust KIND:SCALE] [--plane-to-plane EPS] [--symmetric] [--one-to-one]
//       [--median-factor F] [--adaptive-trim [MIN:MAX[:Q]]] [--reciprocal [GAP]] [--projective [RADIUS]] [--evaluate MAXDIST] [--pyramid LEVELS[:MAXDZ]]
//
// --reject-invalid / --max-dist: correspondence rejection (icp_set_rejection: pairs with a pixel without depth at either end / pairs
// farther apart than MM get weight 0).  --trim: trimmed ICP (icp_set_trimming: every iteration keeps the closest FRACTION in (0, 1] of the
// pairs).  --point-to-plane: point-to-plane ICP plus MU (>= 0) times the point-to-point error (icp_set_error_metric), the normals from the
// fixed 128 x 128 landmark grid (ICP_NORMALS_GRID).  --colored: colored ICP (ICP_METRIC_COLORED): point-to-plane plus KAPPA (>= 0) times
// the photometric term (icp_set_color_weight), grid normals and intensity gradients; MU of --point-to-plane when given, else 0.
// --robust: a robust loss (icp_set_robust_loss) of KIND huber, cauchy or tukey with the scale SCALE (> 0, mm), e.g. tukey:50.
// --plane-to-plane: Generalized ICP (icp_set_plane_to_plane) with the covariance parameter EPS in (0, 1], e.g. 0.001: point-to-plane with
// every pair weighed by both frames' grid normals; implies --point-to-plane 0 when no MU is given.
// --symmetric: symmetric ICP (icp_set_symmetric; Rusinkiewicz 2019): point-to-plane along the mean of both frames' grid normals, the
// rotation split between the frames; implies --point-to-plane 0 when no MU is given.
// --one-to-one: one-to-one correspondences (icp_set_unique): of the pairs that share a fixed point only the closest keeps its weight.
// --median-factor: median-distance rejection (icp_set_median_rejection): every iteration gives the pairs farther apart than F (> 0)
// times that iteration's median pair distance weight 0.
// --adaptive-trim: adaptive trimming (icp_set_adaptive_trimming): every iteration chooses the kept fraction itself, between MIN and MAX,
// by minimising the fractional RMSD with lambda = (Q - 1) / 2, Q in 2 .. 8 (default 0.05:0.95:4); in --trim's place, not together with it.
// --reciprocal: reciprocal correspondences (icp_set_reciprocal): a pair keeps its weight only if its fixed point, searching the moving
// frame, finds the pair's moving point again, or one within GAP mm of it (default 0: exactly that point).
// --projective: projective data association (icp_set_projective): every moving landmark is paired with the closest fixed landmark of the
// (2 RADIUS + 1)^2 window around the cell of the fixed landmark grid it projects to, instead of searching (RADIUS in [0, 8], default 1).
// The intrinsics are those of the landmarks of a 640 x 480 frame (column 65 + 4 i, row 49 + 3 j), for files and the synthetic pair alike.
// --evaluate: after the run, the registration's quality at the final transform (icp_evaluate): fitness, inlier RMSE and the inlier
// count for pairs no farther apart than MAXDIST mm (0: no distance test).
// --pyramid: coarse-to-fine registration (icp_pyramid_*): LEVELS landmark grids 128, 64, 32, .. wide with 256, 64, 64, .. representatives,
// coarsest first, each level made of 2 x 2 means of the one below it (points within MAXDZ mm in z of the block's first valid point,
// doubling per level; default 0: no band); the other options apply to every level, with the level's own grid width.
// Not the reference's behaviour; off by default.
//
// A cloud file is 640 x 480 points of 8 floats [x y z 1 r g b 1], little endian, row-major (src/kinect_frame_grabber.cpp:252-272).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <ocl_icp_reg.hpp>

namespace {

const size_t kPoints = 640u * 480u;
struct AdaptiveTrim { float lo = 0.f, hi = 0.f; uint32_t q = 0; };      // --adaptive-trim (q 0: off)
// the pinhole model of the 128 x 128 landmarks of a 640 x 480 frame, in grid units (include/icp_amd.h: icp_set_projective)
const float kLmFx = 595.f / 4.f, kLmFy = 595.f / 3.f, kLmCx = (319.5f - 65.f) / 4.f, kLmCy = (239.5f - 49.f) / 3.f;

bool exists (const std::string &p) { std::ifstream f (p, std::ios::binary); return f.good (); }

void read_cloud (const std::string &path, std::vector<icp_float8> &pc)
{
    std::ifstream f (path, std::ios::binary);
    if (!f) throw std::runtime_error ("cannot open " + path);
    pc.resize (kPoints);
    f.read (reinterpret_cast<char *> (pc.data ()), (std::streamsize) (kPoints * sizeof (icp_float8)));
    if ((size_t) f.gcount () != kPoints * sizeof (icp_float8)) throw std::runtime_error (path + ": expected 640 x 480 x 8 floats");
}

std::string data_path (const std::string &name) { return exists (name) ? name : "../data/" + name + ".bin"; }

template <cl_algo::ICP::ICPStepConfigT RC>
int run (int device, icp::Mode mode, const std::vector<icp_float8> &pc1, const std::vector<icp_float8> &pc2, const std::string &out,
         int reject_flags, float max_dist, float trim, float p2pl_mu, float kappa, icp::RobustLoss robust, float gicp_eps, bool symmetric, bool one_to_one, float median_factor, AdaptiveTrim adaptive,
         float reciprocal, int projective, float evaluate)
{
    ICPReg<RC, cl_algo::ICP::ICPStepConfigW::WEIGHTED> app (device, mode);
    if (reject_flags || max_dist > 0.f) app.setRejection (reject_flags, max_dist);
    if (reciprocal >= 0.f) app.setReciprocal (true, reciprocal);
    if (projective >= 0) app.setProjective (true, 128, kLmFx, kLmFy, kLmCx, kLmCy, (uint32_t) projective);
    if (one_to_one) app.setUnique (true);
    if (median_factor > 0.f) app.setMedianRejection (median_factor);
    if (trim != 1.f) app.setTrimming (trim);
    if (adaptive.q) app.setAdaptiveTrimming (adaptive.lo, adaptive.hi, adaptive.q);
    if (robust.loss != icp::RobustLoss::NONE) app.setRobustLoss (robust);
    if (gicp_eps > 0.f) app.setPlaneToPlane (gicp_eps);
    if (symmetric) app.setSymmetric (true);
    if (kappa >= 0.f) {
        app.setNormals (ICP_NORMALS_GRID, 128); app.setColorWeight (kappa);
        app.setErrorMetric (ICP_METRIC_COLORED, p2pl_mu >= 0.f ? p2pl_mu : 0.f);
    }
    else if (p2pl_mu >= 0.f) { app.setNormals (ICP_NORMALS_GRID, 128); app.setErrorMetric (ICP_METRIC_POINT_TO_PLANE, p2pl_mu); }
    app.init (pc1, pc2);
    app.registerPC ();                                        // buildRBC + run + transform + the reference's report
    auto &reg = app.registration ();
    std::printf ("\n    q = (%.9g, %.9g, %.9g, %.9g)   t = (%.9g, %.9g, %.9g)   s = %.9g   k = %u\n",
                 reg.q.x (), reg.q.y (), reg.q.z (), reg.q.w (), reg.t (0), reg.t (1), reg.t (2), reg.s, reg.k);
    if (evaluate >= 0.f) {
        const icp_quality_t q = reg.evaluate (evaluate);
        std::printf ("    fitness = %.6f   inlier RMSE = %.6f mm   inliers = %u of %u\n", q.fitness, q.inlier_rmse, q.n_inliers, q.n_moving);
    }
    if (!out.empty ()) {
        std::ofstream f (out, std::ios::binary);
        f.write (reinterpret_cast<const char *> (app.transformed ().data ()), (std::streamsize) (kPoints * sizeof (icp_float8)));
        if (!f) throw std::runtime_error ("cannot write " + out);
        std::printf ("    transformed cloud     :    %s\n", out.c_str ());
    }
    return 0;
}

void check_level (icp_handle h, int rc) { if (rc != ICP_OK) throw std::runtime_error (std::string ("level: ") + icp_last_error (h)); }

// the same registration through cl_algo::ICP::ICPPyramid: the options on every level's handle, the level's own grid width
template <cl_algo::ICP::ICPStepConfigT RC>
int run_pyramid (int device, icp::Mode mode, unsigned levels, float max_dz, const std::vector<icp_float8> &pc1, const std::vector<icp_float8> &pc2, const std::string &out,
                 int reject_flags, float max_dist, float trim, float p2pl_mu, float kappa, icp::RobustLoss robust, float gicp_eps, bool symmetric, bool one_to_one, float median_factor, AdaptiveTrim adaptive,
                 float reciprocal, int projective, float evaluate)
{
    cl_algo::ICP::ICPPyramid<RC, cl_algo::ICP::ICPStepConfigW::WEIGHTED> pyr (icp::Env (device), mode);
    std::vector<uint32_t> nr (levels, 64u); nr[0] = 256u;
    pyr.init (16384, nr, 2e2f, 1e-6f);                       // (the demo's parameters: src/ocl_icp_reg.cpp:82-88)
    pyr.setReduction (ICP_PYRAMID_MEAN, max_dz);
    for (unsigned l = 0; l < levels; ++l) {
        icp_handle h = pyr.level (l);
        const uint32_t gw = 128u >> l;
        if (reject_flags || max_dist > 0.f) check_level (h, icp_set_rejection (h, reject_flags, max_dist));
        if (reciprocal >= 0.f) check_level (h, icp_set_reciprocal (h, 1, reciprocal));
        if (projective >= 0) {                               // (a level's cell is the mean of 2^l x 2^l finest cells: centred on finest column 2^l i + (2^l - 1) / 2)
            const float f = (float) (1u << l), half = (f - 1.f) / 2.f;
            check_level (h, icp_set_projective (h, 1, gw, kLmFx / f, kLmFy / f, (kLmCx - half) / f, (kLmCy - half) / f, (uint32_t) projective));
        }
        if (one_to_one) check_level (h, icp_set_unique (h, 1));
        if (median_factor > 0.f) check_level (h, icp_set_median_rejection (h, median_factor));
        if (trim != 1.f) check_level (h, icp_set_trimming (h, trim));
        if (adaptive.q) check_level (h, icp_set_adaptive_trimming (h, adaptive.lo, adaptive.hi, adaptive.q));
        if (robust.loss != icp::RobustLoss::NONE) check_level (h, icp_set_robust_loss (h, robust.loss, robust.scale));
        if (gicp_eps > 0.f) check_level (h, icp_set_plane_to_plane (h, gicp_eps));
        if (symmetric) check_level (h, icp_set_symmetric (h, 1));
        if (kappa >= 0.f) {
            check_level (h, icp_set_normals (h, ICP_NORMALS_GRID, gw)); check_level (h, icp_set_color_weight (h, kappa));
            check_level (h, icp_set_error_metric (h, ICP_METRIC_COLORED, p2pl_mu >= 0.f ? p2pl_mu : 0.f));
        }
        else if (p2pl_mu >= 0.f) { check_level (h, icp_set_normals (h, ICP_NORMALS_GRID, gw)); check_level (h, icp_set_error_metric (h, ICP_METRIC_POINT_TO_PLANE, p2pl_mu)); }
    }
    pyr.writeCloud (ICP_MEM_F, pc1.data ());
    pyr.writeCloud (ICP_MEM_M, pc2.data ());
    pyr.buildRBC ();
    pyr.sync ();
    pyr.run ();
    std::printf ("\n    q = (%.9g, %.9g, %.9g, %.9g)   t = (%.9g, %.9g, %.9g)   s = %.9g   k =",
                 pyr.q.x (), pyr.q.y (), pyr.q.z (), pyr.q.w (), pyr.t (0), pyr.t (1), pyr.t (2), pyr.s);
    for (unsigned l = 0; l < levels; ++l) std::printf (" %u", pyr.k[l]);
    std::printf ("   (per level, finest first)\n");
    if (evaluate >= 0.f) {
        const icp_quality_t q = pyr.evaluate (evaluate);
        std::printf ("    fitness = %.6f   inlier RMSE = %.6f mm   inliers = %u of %u\n", q.fitness, q.inlier_rmse, q.n_inliers, q.n_moving);
    }
    if (!out.empty ()) {
        std::vector<icp_float8> moved (kPoints);
        check_level (pyr.level (0), icp_transform_cloud (pyr.level (0), pc2.data (), moved.data (), (uint32_t) kPoints));
        std::ofstream f (out, std::ios::binary);
        f.write (reinterpret_cast<const char *> (moved.data ()), (std::streamsize) (kPoints * sizeof (icp_float8)));
        if (!f) throw std::runtime_error ("cannot write " + out);
        std::printf ("    transformed cloud     :    %s\n", out.c_str ());
    }
    return 0;
}

}  // namespace

int main (int argc, char **argv)
{
    std::vector<std::string> names;
    std::string out;
    int device = 0; bool svd = false, symmetric = false, one_to_one = false;
    int reject_flags = 0; float max_dist = 0.f, trim = 1.f, p2pl_mu = -1.f, kappa = -1.f, gicp_eps = 0.f, evaluate = -1.f, reciprocal = -1.f, median_factor = 0.f; int projective = -1;     // (p2pl_mu < 0: point-to-point; kappa < 0: not colored; gicp_eps 0: off; evaluate < 0: no quality report; reciprocal < 0: off)
    icp::RobustLoss robust;
    AdaptiveTrim adaptive;
    unsigned pyramid_levels = 0; float pyramid_dz = 0.f;       // (0 levels: one level, no pyramid object)
    icp::Mode mode = icp::Mode::FAST;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--out" && i + 1 < argc) out = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = std::atoi (argv[++i]);
        else if (a == "--reference-order") mode = icp::Mode::REFERENCE_ORDER;
        else if (a == "--svd") svd = true;
        else if (a == "--reject-invalid") reject_flags |= ICP_REJECT_INVALID;
        else if (a == "--max-dist" && i + 1 < argc) max_dist = std::strtof (argv[++i], nullptr);
        else if (a == "--trim" && i + 1 < argc) {
            trim = std::strtof (argv[++i], nullptr);
            if (!(trim > 0.f && trim <= 1.f)) { std::fprintf (stderr, "--trim: FRACTION must be in (0, 1]\n"); return 2; }
        }
        else if (a == "--point-to-plane" && i + 1 < argc) {
            p2pl_mu = std::strtof (argv[++i], nullptr);
            if (!(p2pl_mu >= 0.f && std::isfinite (p2pl_mu))) { std::fprintf (stderr, "--point-to-plane: MU must be finite and >= 0\n"); return 2; }
        }
        else if (a == "--colored" && i + 1 < argc) {
            kappa = std::strtof (argv[++i], nullptr);
            if (!(kappa >= 0.f && std::isfinite (kappa))) { std::fprintf (stderr, "--colored: KAPPA must be finite and >= 0\n"); return 2; }
        }
        else if (a == "--plane-to-plane" && i + 1 < argc) {
            gicp_eps = std::strtof (argv[++i], nullptr);
            if (!(gicp_eps > 0.f && gicp_eps <= 1.f)) { std::fprintf (stderr, "--plane-to-plane: EPS must be in (0, 1]\n"); return 2; }
        }
        else if (a == "--evaluate" && i + 1 < argc) {
            evaluate = std::strtof (argv[++i], nullptr);
            if (!(evaluate >= 0.f)) { std::fprintf (stderr, "--evaluate: MAXDIST must be >= 0\n"); return 2; }
        }
        else if (a == "--pyramid" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t c = v.find (':');
            char *end = nullptr;
            const long n = std::strtol (v.c_str (), &end, 10);
            const bool levels_ok = end != v.c_str () && (*end == 0 || *end == ':') && n >= 1 && n <= ICP_PYRAMID_MAX_LEVELS;
            char *dend = nullptr;
            pyramid_dz = c == std::string::npos ? 0.f : std::strtof (v.c_str () + c + 1, &dend);
            if (!levels_ok || (c != std::string::npos && (dend == v.c_str () + c + 1 || *dend)) || !(pyramid_dz >= 0.f && std::isfinite (pyramid_dz))) {
                std::fprintf (stderr, "--pyramid: LEVELS[:MAXDZ] with LEVELS in [1, 5] and MAXDZ finite and >= 0\n"); return 2;
            }
            pyramid_levels = (unsigned) n;
        }
        else if (a == "--symmetric") symmetric = true;
        else if (a == "--one-to-one") one_to_one = true;
        else if (a == "--median-factor" && i + 1 < argc) {
            median_factor = std::strtof (argv[++i], nullptr);
            if (!(median_factor > 0.f && std::isfinite (median_factor))) { std::fprintf (stderr, "--median-factor: F must be finite and > 0\n"); return 2; }
        }
        else if (a == "--adaptive-trim") {                        // (MIN:MAX[:Q] is optional: taken when the next argument is no option and holds a colon)
            adaptive.lo = 0.05f; adaptive.hi = 0.95f; adaptive.q = 4u;
            if (i + 1 < argc && argv[i + 1][0] != '-' && std::strchr (argv[i + 1], ':')) {
                const char *v = argv[++i];
                char *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
                long q = 4;
                adaptive.lo = std::strtof (v, &e1);
                const bool lo_ok = e1 != v && *e1 == ':';
                if (lo_ok) adaptive.hi = std::strtof (e1 + 1, &e2);
                const bool hi_ok = lo_ok && e2 != e1 + 1 && (*e2 == 0 || *e2 == ':');
                if (hi_ok && *e2 == ':') q = std::strtol (e2 + 1, &e3, 10);
                const bool q_ok = hi_ok && (*e2 == 0 || (e3 != e2 + 1 && *e3 == 0));
                if (!q_ok || !(adaptive.lo > 0.f && adaptive.lo <= adaptive.hi && adaptive.hi <= 1.f) || q < 2 || q > 8) {
                    std::fprintf (stderr, "--adaptive-trim: MIN:MAX[:Q] with 0 < MIN <= MAX <= 1 and Q in 2 .. 8\n"); return 2;
                }
                adaptive.q = (uint32_t) q;
            }
        }
        else if (a == "--reciprocal") {                           // (GAP is optional: taken when the next argument is a number)
            reciprocal = 0.f;
            if (i + 1 < argc) {
                char *end = nullptr;
                const float g = std::strtof (argv[i + 1], &end);
                if (end != argv[i + 1] && *end == 0) {
                    if (!(g >= 0.f && std::isfinite (g))) { std::fprintf (stderr, "--reciprocal: GAP must be finite and >= 0\n"); return 2; }
                    reciprocal = g; ++i;
                }
            }
        }
        else if (a == "--projective") {                           // (RADIUS is optional: taken when the next argument is a number)
            projective = 1;
            if (i + 1 < argc) {
                char *end = nullptr;
                const long r = std::strtol (argv[i + 1], &end, 10);
                if (end != argv[i + 1] && *end == 0) {
                    if (r < 0 || r > 8) { std::fprintf (stderr, "--projective: RADIUS must be in [0, 8]\n"); return 2; }
                    projective = (int) r; ++i;
                }
            }
        }
        else if (a == "--robust" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t c = v.find (':');
            const std::string kind = v.substr (0, c);
            robust.loss = kind == "huber" ? icp::RobustLoss::HUBER : kind == "cauchy" ? icp::RobustLoss::CAUCHY : kind == "tukey" ? icp::RobustLoss::TUKEY : -1;
            char *end = nullptr;
            robust.scale = c == std::string::npos ? 0.f : std::strtof (v.c_str () + c + 1, &end);
            if (robust.loss < 0 || c == std::string::npos || end == v.c_str () + c + 1 || *end || !(robust.scale > 0.f && std::isfinite (robust.scale))) {
                std::fprintf (stderr, "--robust: KIND:SCALE with KIND huber, cauchy or tukey and SCALE finite and > 0\n"); return 2;
            }
        }
        else if (a.rfind ("--", 0) == 0) { std::fprintf (stderr, "unknown option %s\n", a.c_str ()); return 2; }
        else names.push_back (a);
    }
    if (adaptive.q && trim != 1.f) { std::fprintf (stderr, "--adaptive-trim and --trim exclude each other\n"); return 2; }
    if ((gicp_eps > 0.f || symmetric) && p2pl_mu < 0.f) p2pl_mu = 0.f;   // (plane-to-plane and symmetric act in the point-to-plane metric)
    try
    {
        std::vector<icp_float8> pc1, pc2;
        if (names.empty ()) {
            pc1.resize (kPoints); pc2.resize (kPoints);
            if (icp_synth_cloud_vga (0x1C9D5EEDull, 0, pc1[0].data ()) || icp_synth_cloud_vga (0x1C9D5EEDull, 1, pc2[0].data ())) return 2;
            std::printf ("(no files given: a synthetic pair)\n");
        } else if (names.size () == 1) {
            read_cloud ("../data/" + names[0] + "_1.bin", pc1); read_cloud ("../data/" + names[0] + "_2.bin", pc2);
        } else {
            read_cloud (data_path (names[0]), pc1); read_cloud (data_path (names[1]), pc2);
        }
        if (pyramid_levels)
            return svd ? run_pyramid<cl_algo::ICP::ICPStepConfigT::EIGEN> (device, mode, pyramid_levels, pyramid_dz, pc1, pc2, out, reject_flags, max_dist, trim, p2pl_mu, kappa, robust, gicp_eps, symmetric, one_to_one, median_factor, adaptive, reciprocal, projective, evaluate)
                       : run_pyramid<cl_algo::ICP::ICPStepConfigT::POWER_METHOD> (device, mode, pyramid_levels, pyramid_dz, pc1, pc2, out, reject_flags, max_dist, trim, p2pl_mu, kappa, robust, gicp_eps, symmetric, one_to_one, median_factor, adaptive, reciprocal, projective, evaluate);
        return svd ? run<cl_algo::ICP::ICPStepConfigT::EIGEN> (device, mode, pc1, pc2, out, reject_flags, max_dist, trim, p2pl_mu, kappa, robust, gicp_eps, symmetric, one_to_one, median_factor, adaptive, reciprocal, projective, evaluate)
                   : run<cl_algo::ICP::ICPStepConfigT::POWER_METHOD> (device, mode, pc1, pc2, out, reject_flags, max_dist, trim, p2pl_mu, kappa, robust, gicp_eps, symmetric, one_to_one, median_factor, adaptive, reciprocal, projective, evaluate);
    }
    catch (const std::exception &e)
    {
        std::fprintf (stderr, "%s\n", e.what ());
        return 1;
    }
}
