"""Diagnostic (not a test): what coarse-to-fine registration costs and buys in wall-clock time.  In one process, on the synthetic
pair, from the identity: a blocking ICPPyramid.run() against a blocking single-level ICP.run() of level 0's shape, with the iteration
counts and the distance of both results from the ground truth, and the construction launch of the levels alone (HIP events around it).
    python tools/diag/pyramid_time.py [--rot-deg D] [--reps N] [--json FILE]
Shapes: |F| = 16384 as sides 128 / 64 / 32 (nr 256 / 64 / 64), and |F| = 2^20 as sides 1024 / 512 / 256 / 128 (nr 4096 / 1024 / 1024 /
256: the rule halves the side per level, so the 512 level stands between 1024 and 256)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np          # noqa: E402
import icp_amd              # noqa: E402

SHAPES = {"16384": (128, (256, 64, 64)), "2^20": (1024, (4096, 1024, 1024, 256))}


def error_to(T, T_true):
    q, p = np.asarray(T[:4], np.float64), np.asarray(T_true[:4], np.float64)
    d = abs(float(np.dot(q / np.linalg.norm(q), p / np.linalg.norm(p))))
    return float(np.degrees(2.0 * np.arccos(min(1.0, d)))), float(np.linalg.norm(np.asarray(T[4:7], np.float64) - np.asarray(T_true[4:7], np.float64)))


def timed(run, reset, sync, reps):
    """(median, min) wall-clock ms of `reps` blocking runs, each from the identity, and the result of the last one."""
    ms, out = [], None
    for _ in range(reps + 2):                    # (two untimed passes first)
        reset()
        sync()
        t0 = time.perf_counter()
        out = run()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[2:]
    return statistics.median(ms), min(ms), out


def measure(name, side, nr, rot_deg, reps, max_iterations=40):
    m = side * side
    F, M, T_true = icp_amd.synth_pair_scene(side, icp_amd.SCENE_CURVED, rot_deg=rot_deg)
    g = icp_amd.ICP(0)
    g.init(m, nr[0], 2e2, 1e-6, max_iterations)
    g.write(icp_amd.Memory.F, F)
    g.write(icp_amd.Memory.M, M)
    g.buildRBC()
    s_med, s_min, s_k = timed(g.run, g.reset_transform, g.sync, reps)
    s_err = error_to(g.read(icp_amd.Memory.T), T_true)
    s_conv = bool(g.state().converged)
    g.close()
    p = icp_amd.ICPPyramid(0)
    p.init(m, nr, 2e2, 1e-6, max_iterations)
    p.write(icp_amd.Memory.F, F)
    p.write(icp_amd.Memory.M, M)
    p.buildRBC()
    p_med, p_min, p_k = timed(p.run, p.reset_transform, p.sync, reps)
    p_err = error_to(p.level(0).read(icp_amd.Memory.T), T_true)
    p_conv = bool(p.level(0).state().converged)
    build_ms = p.time_build(icp_amd.Memory.F, 20)
    p.close()
    return dict(shape=name, sides=[side >> l for l in range(len(nr))], nr=list(nr), rot_deg=rot_deg,
                single=dict(ms_median=round(s_med, 4), ms_min=round(s_min, 4), k=s_k, converged=s_conv, deg=round(s_err[0], 4), mm=round(s_err[1], 3)),
                pyramid=dict(ms_median=round(p_med, 4), ms_min=round(p_min, 4), k=p_k, converged=p_conv, deg=round(p_err[0], 4), mm=round(p_err[1], 3)),
                build_launch_us=round(build_ms * 1e3, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rot-deg", type=float, nargs="*", default=[3.0, 10.0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for name, (side, nr) in SHAPES.items():
        for deg in args.rot_deg:
            r = measure(name, side, nr, deg, args.reps)
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
