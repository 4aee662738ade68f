"""Diagnostic (not a test): microseconds per iteration of the plane metrics, colored ICP (ICP_METRIC_COLORED), point-to-plane and
plane-to-plane (gicp: point-to-plane with icp_set_plane_to_plane 0.001, both frames' grid normals) and symmetric (sym: point-to-plane
with icp_set_symmetric, both frames' grid normals),
against the default point-to-point iteration at A (16384 / 256), B (65536 / 1024) and A x 64, through the fixed-length run graphs
bench.py times; and buildRBC back to back without normals, with grid normals (point-to-plane) and with grid normals and intensity
gradients (colored).

    python tools/diag/plane_time.py [--only {p2p,p2pl,colored,gicp,sym}] [--reps N] [--robust KIND:SCALE]

--robust (e.g. cauchy:20) times every configuration with that robust loss on (icp_set_robust_loss) as well as without it.

Prints one line per configuration and one JSON line at the end.  Under `rocprofv3 --kernel-trace --stats` (--only p2pl or colored)
the per-kernel table shows the search, k_plane_moments, k_p2pl_finalize, k_normals_grid and (colored) k_color_grad_grid; --only gicp shows
k_gicp_moments, --only sym k_sym_moments, in k_plane_moments' place."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import icp_amd  # noqa: E402

CONFIGS = {"A": (128, 256, 1), "B": (256, 1024, 1), "Ax64": (128, 256, 64)}
METRICS = {"p2p": icp_amd.ErrorMetric.POINT_TO_POINT, "p2pl": icp_amd.ErrorMetric.POINT_TO_PLANE, "colored": icp_amd.ErrorMetric.COLORED,
           "gicp": icp_amd.ErrorMetric.POINT_TO_PLANE, "sym": icp_amd.ErrorMetric.POINT_TO_PLANE}
GICP_EPS = 1e-3


def make(side, nr, batch, metric, robust=None, gicp=False, sym=False):
    g = icp_amd.ICP(0)
    g.init(side * side, nr, 2e2, 1e-6, batch=batch)
    g.setPowerMode(icp_amd.PowerMode.SQUARED)
    if metric != icp_amd.ErrorMetric.POINT_TO_POINT:
        g.set_normals(icp_amd.Normals.GRID, side)
        g.set_color_weight(1000.0)
        g.set_error_metric(metric, 0.05)
    if gicp:
        g.set_plane_to_plane(GICP_EPS)
    if sym:
        g.set_symmetric(True)
    if robust:
        g.set_robust_loss(*robust)
    for b in range(batch):
        F, M, _ = icp_amd.synth_pair_scene(side, icp_amd.SCENE_WALL, seed=0x1C9D5EED + b)
        g.write(icp_amd.Memory.F, F, batch_index=b)
        g.write(icp_amd.Memory.M, M, batch_index=b)
    g.buildRBC()
    return g


def per_iteration_us(g, iterations, reps):
    g.time_run_fixed(iterations, 2, True)                   # (warm-up: graph capture, clocks)
    best = min(g.time_run_fixed(iterations, reps, True) for _ in range(3))
    return best * 1e3 / (iterations * reps)


def build_us(g, n=200):
    g.buildRBC(); g.sync()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(n):
            g.buildRBC()
        g.sync()
        best = min(best, (time.perf_counter() - t0) / n * 1e6)
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--only", choices=sorted(METRICS), help="time this metric only")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--robust", default=None, metavar="KIND:SCALE", help="also time with this robust loss on (e.g. cauchy:20)")
    args = ap.parse_args()
    robust = None
    if args.robust:
        from icp_amd.register import _robust
        robust = _robust(args.robust)
    out = {}
    for name, (side, nr, batch) in CONFIGS.items():
        for mname, metric in METRICS.items():
            if args.only and mname != args.only:
                continue
            for tag, rb in (("", None), ("_robust", robust)) if robust else (("", None),):
                g = make(side, nr, batch, metric, rb, mname == "gicp", mname == "sym")
                us = per_iteration_us(g, 20, args.reps)
                bus = build_us(g)
                form, launches = g.run_form(), g.launches_per_iteration()
                g.close()
                out["%s_%s%s" % (name, mname, tag)] = round(us, 3)
                out["%s_%s%s_build" % (name, mname, tag)] = round(bus, 3)
                print("%-5s %-15s %8.3f us/iteration  (form %d, %d launches per iteration)   buildRBC %8.2f us"
                      % (name, mname + tag, us, form, launches, bus))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
