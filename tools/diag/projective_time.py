"""Diagnostic (not a test): what projective data association (icp_set_projective) costs per iteration, and where it ends.

    python tools/diag/projective_time.py [--runs N] [--sizes 16384,65536,2^20,64x16384]

Cost.  At |F| = 16384 (256 representatives), 65536 (1024), 2^20 (4096) and 64 batched registrations of 16384, for point-to-point and
point-to-plane (grid normals): us per iteration of the fixed 40-iteration graph, every pass a fresh registration, HIP events around
one pass behind a leading one (icp_time_run_fixed_tail) — the median of `runs` such passes — with the rule off and with the window
radius r = 0, 1 and 2 (the grid's own intrinsics), all on one handle in one run; and icp_time_masked's projection + apply pass alone.

Convergence.  synth_pair_scene (128) one and three degrees apart, point-to-point, icp_run: rotation and translation error against the
ground truth with the rule off (the RBC search) and with r = 0, 1, 2.

Prints one line per configuration and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import icp_amd  # noqa: E402
from icp_amd import workloads as W  # noqa: E402

CONFIGS = {"16384": (128, 256, 1), "65536": (256, 1024, 1), "2^20": (1024, 4096, 1), "64x16384": (128, 256, 64)}
ITERATIONS = 40
RADII = (0, 1, 2)


def handle(side, nr, batch, plane):
    g = icp_amd.ICP(0)
    g.init(side * side, nr, 2e2, 1e-6, batch=batch)
    g.setPowerMode(icp_amd.PowerMode.SQUARED)
    if plane:
        g.set_normals(icp_amd.Normals.GRID, side)
        g.set_error_metric(icp_amd.ErrorMetric.POINT_TO_PLANE, 0.05)
    F, M = icp_amd.synth_pair(side)
    for b in range(batch):
        g.write(icp_amd.Memory.F, F, batch_index=b)
        g.write(icp_amd.Memory.M, M, batch_index=b)
    g.buildRBC()
    g.sync()
    return g


def iteration_us(g, runs):
    g.time_run_fixed_tail(ITERATIONS, 2, True)                   # (captures the graph, warms up)
    us = []
    for _ in range(runs):
        ms, n = g.time_run_fixed_tail(ITERATIONS, 2, True)
        us.append(ms * 1e3 / (n * ITERATIONS))
    return round(statistics.median(us), 2)


def cost(name, runs):
    side, nr, batch = CONFIGS[name]
    intr = icp_amd.grid_intrinsics(side)
    out = {}
    for metric, plane in (("point_to_point", False), ("point_to_plane", True)):
        g = handle(side, nr, batch, plane)
        r = {"off_us": iteration_us(g, runs), "launches_off": g.launches_per_iteration()}
        for radius in RADII:
            g.set_projective(side, *intr, radius=radius)
            r["r%d_us" % radius] = iteration_us(g, runs)
            r["r%d_search_stage_us" % radius] = round(g.time_masked(1, ITERATIONS, 5), 2)
            r["r%d_words_last_iteration" % radius] = g.read(icp_amd.Memory.PROJECTIVE).tolist()
        r["launches_on"] = g.launches_per_iteration()
        g.close()
        out[metric] = r
        print("%-9s %-14s off %8.2f us   " % (name, metric, r["off_us"])
              + "   ".join("r = %d %8.2f us (projection%s %7.2f us)" % (k, r["r%d_us" % k], "" if plane else " + apply", r["r%d_search_stage_us" % k]) for k in RADII))
    return out


def convergence():
    out = {}
    for deg in (1.0, 3.0):
        F, M, T_true = icp_amd.synth_pair_scene(128, rot_deg=deg)
        for radius in (None,) + RADII:
            g = icp_amd.ICP(0)
            g.init(F.shape[0], 256, 2e2, 1e-6)
            g.setPowerMode(icp_amd.PowerMode.SQUARED)
            if radius is not None:
                g.set_projective(128, *icp_amd.grid_intrinsics(128), radius=radius)
            g.write(icp_amd.Memory.F, F)
            g.write(icp_amd.Memory.M, M)
            g.buildRBC()
            k = g.run()
            T = g.read(icp_amd.Memory.T).copy()
            g.close()
            name = "%g deg, %s" % (deg, "RBC search" if radius is None else "projective r = %d" % radius)
            out[name] = {"k": k, "rotation_error_deg": round(W.rotation_error_deg(T, T_true), 4),
                         "translation_error_mm": round(float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7].astype(np.float64))), 3)}
            print("synth_pair_scene (128)  %-26s k = %2d   %.4f deg   %.2f mm" % (name, k, out[name]["rotation_error_deg"], out[name]["translation_error_mm"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", default=",".join(CONFIGS))
    args = ap.parse_args()
    out = {"cost": {}}
    for name in args.sizes.split(","):
        out["cost"][name] = cost(name, args.runs)
        print(json.dumps({name: out["cost"][name]}), flush=True)
    out["convergence"] = convergence()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
