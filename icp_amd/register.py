"""`python -m icp_amd.register fixed.bin moving.bin [-o out.bin]` — what the reference's `ICPReg::registerPC`
does (src/ocl_icp_reg.cpp:165-210) without the GL window: landmarks (getLMs), buildRBC, ICP::run, full-cloud
transform of the moving cloud, and the same printout."""
import argparse
import inspect
import math
import time
import types

import numpy as np

from . import landmark_intrinsics, ICP, ErrorMetric, ICPPyramid, Memory, Normals, Pairs, PowerMode, PyramidReduction, ReduceMode, RobustLoss
from .io import load_pc8d, save_pc8d


def register_clouds(fixed, moving, device=0, a=2e2, c=1e-6, max_iterations=40, angle_threshold=0.001,
                    translation_threshold=0.01, reduce_mode=ReduceMode.FUSED, reject_invalid=False, max_dist=None, trim=1.0,
                    point_to_plane=None, colored=None, robust=None, plane_to_plane=None, symmetric=False, one_to_one=False,
                    normal_angle=None, reject_boundary=False, pyramid=None, reciprocal=None, projective=None, median_factor=None,
                    adaptive_trim=None):
    """Returns (T[8], k, latency_ms, transformed moving cloud).  reject_invalid / max_dist: correspondence rejection
    (ICPStep.set_rejection), trim: the fraction of pairs trimmed ICP keeps (ICPStep.set_trimming; 1.0: off), point_to_plane: mu of
    point-to-plane ICP with the fixed frame's normals from its 128 x 128 landmark grid (ICPStep.set_error_metric; None: off),
    colored: kappa of colored ICP, with grid normals and intensity gradients and mu = point_to_plane or 0 (ICPStep.set_color_weight;
    None: off), robust: (RobustLoss kind, scale) of a robust loss (ICPStep.set_robust_loss; None: off), plane_to_plane: epsilon of
    Generalized ICP, with both frames' grid normals and mu = point_to_plane or 0 (ICPStep.set_plane_to_plane; None: off), symmetric:
    the symmetric objective, with both frames' grid normals and mu = point_to_plane or 0 (ICPStep.set_symmetric), one_to_one: of the
    pairs that share a fixed point only the closest keeps its weight (ICPStep.set_unique), normal_angle: the largest angle in degrees
    between the two normals of a pair, with both frames' grid normals (ICPStep.set_normal_rejection with its cosine; None: off),
    reject_boundary: pairs whose fixed point lies at the boundary of the 128 wide landmark grid get weight 0
    (ICPStep.set_boundary_rejection), reciprocal: max_gap in mm of reciprocal correspondences — a pair keeps its weight only if its fixed
    point finds the pair's moving point again, or one within max_gap of it (ICPStep.set_reciprocal; 0: exact only, None: off), projective: the window radius in [0, 8] of projective data association — the pairs
    come from projecting the moving landmarks onto the fixed landmark grid with the frame's pinhole model (landmark_intrinsics) instead
    of from the RBC search (ICPStep.set_projective; None: off), median_factor: every iteration rejects the pairs farther apart than
    median_factor times that iteration's median pair distance (ICPStep.set_median_rejection; None: off), adaptive_trim: (min_fraction,
    max_fraction, power) of adaptive trimming — every iteration chooses the kept fraction itself (ICPStep.set_adaptive_trimming; None:
    off; not together with trim < 1); pyramid: (levels, max_dz) of a coarse-to-fine registration (ICPPyramid: 128, 64, 32, .. wide
    levels with 256, 64, 64, .. representatives, 2 x 2 means within a z band of max_dz mm, 0: no band; every option above applies to
    every level with the level's own grid width; k is then the list of the levels' counts, finest first; None: one level); none is
    the reference's behaviour, all are off by default."""
    return _run(False, None, types.SimpleNamespace(**locals()))[:4]


def register_and_evaluate(fixed, moving, evaluate, **options):
    """register_clouds (its options) with the registration's quality at the final transform: returns (T[8], k, latency_ms,
    transformed moving cloud, Quality record) — fitness, inlier RMSE, information matrix and counts for pairs no farther apart than
    `evaluate` mm (ICPStep.evaluate; 0 or None: no distance test)."""
    return _run(False, 0.0 if evaluate is None else evaluate, _bind(fixed, moving, options))[:5]


def register_with_pairs(fixed, moving, evaluate=None, **options):
    """register_clouds (its options) with the registration's correspondence set at the final transform: returns (T[8], k, latency_ms,
    transformed moving cloud, Quality record or None, pairs) — pairs the Pairs.EVALUATED set (ICPStep.correspondences: a structured
    array of moving index, fixed landmark index, squared distance, weight) for pairs no farther apart than `evaluate` mm (None or 0:
    no distance test); the Quality record is None when `evaluate` is None."""
    return _run(True, evaluate, _bind(fixed, moving, options))


def _bind(fixed, moving, options):
    """The record register_clouds makes of its arguments — one field per parameter, its defaults filled in —, for the functions that
    take its options by name; TypeError for a name it does not have."""
    bound = inspect.signature(register_clouds).bind(fixed, moving, **options)
    bound.apply_defaults()
    return types.SimpleNamespace(**bound.arguments)


def pyramid_nr(levels):
    """Representatives per level of the 128 wide landmark grid, finest first: 256, 64, 64, .."""
    return [256] + [64] * (levels - 1)


def level_intrinsics(intr, factor):
    """(fx, fy, cx, cy) of a pyramid level whose cells are `factor` x `factor` means of the finest grid's (PyramidReduction.MEAN): cell i
    of the level is centred on finest column factor i + (factor - 1) / 2, so f / factor and (c - (factor - 1) / 2) / factor."""
    fx, fy, cx, cy = intr
    h = (factor - 1) / 2.0
    return fx / factor, fy / factor, (cx - h) / factor, (cy - h) / factor


def _apply_options(reg, side, o):
    """The options of register_clouds' record `o` on one handle whose landmark grid is `side` wide (640 x 480 clouds -> 128 x 128
    landmarks, row-major; a pyramid level l: 128 >> l)."""
    if o.projective is not None:
        reg.set_projective(side, *level_intrinsics(landmark_intrinsics(), 128 // side), radius=o.projective)
    reg.setPowerMode(PowerMode.SQUARED)
    reg.setReduceMode(o.reduce_mode)
    if o.reject_invalid or o.max_dist:
        reg.set_rejection(o.reject_invalid, o.max_dist)
    if o.reject_boundary:
        reg.set_boundary_rejection(side)
    if o.normal_angle is not None:
        reg.set_normals(Normals.GRID, side)
        reg.set_normal_rejection(normal_cosine(o.normal_angle))
    if o.reciprocal is not None:
        reg.set_reciprocal(True, o.reciprocal)
    if o.one_to_one:
        reg.set_unique(True)
    if o.median_factor is not None:
        reg.set_median_rejection(o.median_factor)
    if o.trim != 1.0:
        reg.set_trimming(o.trim)
    if o.adaptive_trim is not None:
        reg.set_adaptive_trimming(*o.adaptive_trim)
    if o.robust is not None:
        reg.set_robust_loss(*o.robust)
    point_to_plane = o.point_to_plane
    if o.plane_to_plane is not None:
        reg.set_plane_to_plane(o.plane_to_plane)
        if point_to_plane is None:
            point_to_plane = 0.0                               # (plane-to-plane acts in the point-to-plane metric)
    if o.symmetric:
        reg.set_symmetric(True)
        if point_to_plane is None:
            point_to_plane = 0.0                               # (the symmetric objective acts in the point-to-plane metric)
    if o.colored is not None:
        reg.set_normals(Normals.GRID, side)
        reg.set_color_weight(o.colored)
        reg.set_error_metric(ErrorMetric.COLORED, 0.0 if point_to_plane is None else point_to_plane)
    elif point_to_plane is not None:
        reg.set_normals(Normals.GRID, side)
        reg.set_error_metric(ErrorMetric.POINT_TO_PLANE, point_to_plane)


def _run(pairs, evaluate, o):
    """(T[8], k, latency_ms, transformed moving cloud, Quality record or None, pairs or None) for register_clouds' record `o`: the
    quality at max_dist = evaluate (None: no evaluation), with `pairs` the Pairs.EVALUATED correspondence set at the same max_dist (None:
    0, no distance test).  `o` has one field per parameter of register_clouds."""
    if o.pyramid is not None:
        levels, max_dz = o.pyramid
        reg = ICPPyramid(o.device)
        reg.init(16384, pyramid_nr(levels), o.a, o.c, o.max_iterations, o.angle_threshold, o.translation_threshold)
        reg.set_reduction(PyramidReduction.MEAN, max_dz)
        for l in range(levels):
            _apply_options(reg.level(l), 128 >> l, o)
        result = reg.level(0)
    else:
        reg = result = ICP(o.device)
        reg.init(16384, 256, o.a, o.c, o.max_iterations, o.angle_threshold, o.translation_threshold)   # src/ocl_icp_reg.cpp:81-88
        _apply_options(reg, 128, o)
    reg.write_cloud(Memory.F, o.fixed)
    reg.write_cloud(Memory.M, o.moving)
    reg.buildRBC()
    reg.sync()
    t0 = time.perf_counter()
    k = reg.run()
    ms = (time.perf_counter() - t0) * 1e3
    T = result.read(Memory.T)
    quality = result.evaluate(evaluate)[0] if evaluate is not None else None
    members = result.correspondences(Pairs.EVALUATED, evaluate or 0.0) if pairs else None
    out = result.transform_cloud(o.moving)
    reg.close()
    return T, k, ms, out, quality, members


def track(frames, device=0, a=2e2, c=1e-6, warm_start=False, **kw):
    """Frame-to-frame registration (README.md:4 of the reference): frame i is the fixed set of frame i+1.
    Yields (T_i, k_i) mapping frame i+1 onto frame i.  One handle; every frame is uploaded once, its landmarks are
    extracted on the device and stay there to serve as the next hop's fixed set (icp_track_next); warm_start: each hop
    starts from the previous hop's transform instead of the identity."""
    reg = ICP(device)
    reg.init(16384, 256, a, c, kw.get("max_iterations", 40), kw.get("angle_threshold", 0.001), kw.get("translation_threshold", 0.01))
    reg.setPowerMode(PowerMode.SQUARED)
    reg.setReduceMode(kw.get("reduce_mode", ReduceMode.FUSED))
    for f in frames:
        k = reg.track_next(f, warm_start)
        if k is not None:
            yield reg.read(Memory.T), k
    reg.close()


def _fraction(s):
    v = float(s)
    if not 0.0 < v <= 1.0:
        raise argparse.ArgumentTypeError("must be in (0, 1], got %s" % s)
    return v


def _point_weight(s):
    v = float(s)
    if not (v >= 0.0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError("must be finite and >= 0, got %s" % s)
    return v


def normal_cosine(degrees):
    """The min_cos of ICPStep.set_normal_rejection for a largest angle in degrees (the engine's rule takes the cosine)."""
    return min(1.0, max(-1.0, math.cos(math.radians(float(degrees)))))


def _angle(s):
    v = float(s)
    if not 0.0 <= v <= 180.0:
        raise argparse.ArgumentTypeError("must be an angle in [0, 180] degrees, got %s" % s)
    return v


def _radius(s):
    try:
        v = int(s)
    except ValueError:
        raise argparse.ArgumentTypeError("must be an integer in [0, 8], got %s" % s)
    if not 0 <= v <= 8:
        raise argparse.ArgumentTypeError("must be in [0, 8], got %s" % s)
    return v


def _robust(s):
    """KIND:SCALE, e.g. tukey:50 -> (RobustLoss kind, scale); KIND is huber, cauchy or tukey, SCALE finite and > 0."""
    kind, sep, scale = s.partition(":")
    if kind.lower() not in ("huber", "cauchy", "tukey") or not sep:
        raise argparse.ArgumentTypeError("must be KIND:SCALE with KIND huber, cauchy or tukey, got %s" % s)
    try:
        v = float(scale)
    except ValueError:
        raise argparse.ArgumentTypeError("SCALE must be a number, got %s" % s)
    if not (v > 0.0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError("SCALE must be finite and > 0, got %s" % s)
    return RobustLoss.NAMES[kind.lower()], v


def _median_factor(s):
    """a finite factor > 0"""
    v = float(s)
    if not (v > 0.0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError("must be finite and > 0, got %s" % s)
    return v


def _adaptive_trim(s):
    """MIN:MAX[:Q], e.g. 0.05:0.95 or 0.4:1:3 -> (min_fraction, max_fraction, power); 0 < MIN <= MAX <= 1, Q in 2 .. 8 (default 4)."""
    parts = s.split(":")
    try:
        lo, hi, q = float(parts[0]), float(parts[1]), int(parts[2]) if len(parts) == 3 else 4
    except (ValueError, IndexError):
        raise argparse.ArgumentTypeError("must be MIN:MAX[:Q], got %s" % s)
    if len(parts) > 3 or not (0.0 < lo <= hi <= 1.0) or not 2 <= q <= 8:
        raise argparse.ArgumentTypeError("must be MIN:MAX[:Q] with 0 < MIN <= MAX <= 1 and Q in 2 .. 8, got %s" % s)
    return lo, hi, q


def _pyramid(s):
    """LEVELS[:MAXDZ], e.g. 3 or 3:24 -> (levels, max_dz); LEVELS in [1, 5], MAXDZ finite and >= 0 (mm; 0: no band)."""
    levels, sep, dz = s.partition(":")
    try:
        n, v = int(levels), float(dz) if sep else 0.0
    except ValueError:
        raise argparse.ArgumentTypeError("must be LEVELS[:MAXDZ], got %s" % s)
    if not 1 <= n <= 5 or not (v >= 0.0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError("LEVELS must be in [1, 5] and MAXDZ finite and >= 0, got %s" % s)
    return n, v


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("fixed")
    ap.add_argument("moving")
    ap.add_argument("-o", "--output", help="write the transformed moving cloud (raw 640x480 float8)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-a", "--alpha", dest="a", metavar="ALPHA", type=float, default=2e2)
    ap.add_argument("--reject-invalid", action="store_true",
                    help="give pairs with an invalid endpoint (a pixel without depth) weight 0 (not reference behaviour)")
    ap.add_argument("--max-dist", type=float, default=None,
                    help="give pairs farther apart than this geometric distance (mm) weight 0 (not reference behaviour)")
    ap.add_argument("--trim", type=_fraction, default=1.0, metavar="FRACTION",
                    help="trimmed ICP: keep the closest FRACTION in (0, 1] of the pairs in every iteration (not reference behaviour)")
    ap.add_argument("--one-to-one", action="store_true",
                    help="one-to-one correspondences: of the pairs that share a fixed point only the closest keeps its weight, "
                         "before trimming (not reference behaviour)")
    ap.add_argument("--median-factor", type=_median_factor, default=None, metavar="F",
                    help="median-distance rejection: in every iteration give the pairs farther apart than F times that iteration's "
                         "median pair distance weight 0, e.g. 2; behind --one-to-one, before --trim (not reference behaviour)")
    ap.add_argument("--adaptive-trim", type=_adaptive_trim, nargs="?", const=(0.05, 0.95, 4), default=None, metavar="MIN:MAX[:Q]",
                    help="adaptive trimming: every iteration chooses the kept fraction itself, between MIN and MAX, by minimising the "
                         "fractional RMSD with lambda = (Q - 1) / 2, Q in 2 .. 8 (default 0.05:0.95:4); in --trim's place, not together "
                         "with it (not reference behaviour)")
    ap.add_argument("--reciprocal", type=_point_weight, nargs="?", const=0.0, default=None, metavar="GAP",
                    help="reciprocal correspondences: a pair keeps its weight only if its fixed point, searching the moving frame, "
                         "finds the pair's moving point again, or one within GAP mm of it (default 0: exactly that point); before "
                         "--one-to-one and --trim (not reference behaviour)")
    ap.add_argument("--projective", type=_radius, nargs="?", const=1, default=None, metavar="RADIUS",
                    help="projective data association: pair every moving landmark with the closest fixed landmark of the "
                         "(2 RADIUS + 1)^2 window around the cell it projects to, instead of searching (RADIUS in [0, 8], default 1; "
                         "0 suits --point-to-plane; not reference behaviour)")
    ap.add_argument("--normal-angle", type=_angle, default=None, metavar="DEG",
                    help="give pairs whose two surface normals differ by more than DEG degrees weight 0, normals from both landmark "
                         "grids (not reference behaviour)")
    ap.add_argument("--reject-boundary", action="store_true",
                    help="give pairs whose fixed point lies on the rim of the fixed landmark grid or beside a depth hole weight 0 "
                         "(not reference behaviour)")
    ap.add_argument("--point-to-plane", type=_point_weight, default=None, metavar="MU",
                    help="point-to-plane ICP plus MU (>= 0) times the point-to-point error, normals from the fixed landmark grid "
                         "(not reference behaviour)")
    ap.add_argument("--colored", type=_point_weight, default=None, metavar="KAPPA",
                    help="colored ICP: point-to-plane plus KAPPA (>= 0) times the photometric term, normals and intensity gradients "
                         "from the fixed landmark grid; MU of --point-to-plane when given, else 0 (not reference behaviour)")
    ap.add_argument("--robust", type=_robust, default=None, metavar="KIND:SCALE",
                    help="robust loss: huber, cauchy or tukey with the scale SCALE (> 0, mm), e.g. tukey:50; every pair is "
                         "down-weighted by its own residual (not reference behaviour)")
    ap.add_argument("--plane-to-plane", type=_fraction, default=None, metavar="EPS",
                    help="Generalized ICP: point-to-plane with every pair weighed by both frames' grid normals, covariance parameter "
                         "EPS in (0, 1], e.g. 0.001; implies --point-to-plane 0 when no MU is given (not reference behaviour)")
    ap.add_argument("--symmetric", action="store_true",
                    help="symmetric ICP (Rusinkiewicz 2019): point-to-plane along the mean of both frames' grid normals, the rotation "
                         "split between the frames; implies --point-to-plane 0 when no MU is given (not reference behaviour)")
    ap.add_argument("--evaluate", type=_point_weight, default=None, metavar="MAXDIST",
                    help="after the run print the registration's fitness, inlier RMSE and inlier count at the final transform, for "
                         "pairs no farther apart than MAXDIST mm (0: no distance test)")
    ap.add_argument("--pairs", default=None, metavar="FILE",
                    help="after the run write the correspondence set at the final transform to FILE as .npy: one record (moving landmark "
                         "index, fixed landmark index, squared distance in mm^2, weight) per pair no farther apart than --evaluate's "
                         "MAXDIST (without --evaluate: no distance test), in ascending moving index; prints the count")
    ap.add_argument("--pyramid", type=_pyramid, default=None, metavar="LEVELS[:MAXDZ]",
                    help="coarse-to-fine: register on LEVELS landmark grids (128, 64, 32, .. wide; 256, 64, 64, .. representatives), "
                         "coarsest first, each level made of 2 x 2 means of the one below it (points within MAXDZ mm in z, doubling "
                         "per level; default 0: no band); the other options apply to every level (not reference behaviour)")
    args = ap.parse_args(argv)
    if args.adaptive_trim is not None and args.trim != 1.0:
        ap.error("--adaptive-trim and --trim exclude each other")
    fixed, moving = load_pc8d(args.fixed), load_pc8d(args.moving)
    # (every option's flag is stored under register_clouds' name for it)
    names = list(inspect.signature(register_clouds).parameters)[2:]
    o = _bind(fixed, moving, {name: getattr(args, name) for name in names if hasattr(args, name)})
    T, k, ms, out, quality, members = _run(args.pairs is not None, args.evaluate, o)
    q, t, s = T[:4], T[4:7], T[7]
    sinth_2 = float(np.linalg.norm(q[:3]))
    angle = 180.0 / math.pi * 2 * math.atan2(sinth_2, float(q[3]))
    axis = q[:3] / sinth_2 if sinth_2 else np.zeros(3)
    print("\n================\n")                                     # src/ocl_icp_reg.cpp:199-206
    print("    Iterations            :    %s" % (k if args.pyramid is None else " + ".join("%d" % v for v in k) + "  (per level, finest first)"))
    print("    Latency               :    %.3f ms" % ms)
    print("    Rotation angle        :    %g degrees" % angle)
    print("    Rotation axis         :    %s" % np.array2string(axis, precision=6))
    print("    Translation vector    :    %s" % np.array2string(t, precision=4))
    print("    Scale                 :    %g" % s)
    if quality is not None:
        print("    Fitness               :    %.6f" % quality.fitness)
        print("    Inlier RMSE           :    %.6f mm" % quality.inlier_rmse)
        print("    Inliers               :    %d of %d" % (quality.n_inliers, quality.n_moving))
    if members is not None:
        with open(args.pairs, "wb") as f:                # (a file object: np.save appends no extension to it)
            np.save(f, members)
        print("    Correspondences       :    %d" % len(members))
    if args.output:
        save_pc8d(args.output, out)


if __name__ == "__main__":
    main()
