"""Diagnostic (not a test): what reciprocal correspondences (icp_set_reciprocal) cost per iteration, and what they buy.

    python tools/diag/reciprocal_time.py [--runs N] [--sizes 16384,65536,2^20,64x16384]

Cost.  At |F| = 16384 (256 representatives), 65536 (1024), 2^20 (4096) and 64 batched registrations of 16384, for point-to-point and
point-to-plane (grid normals): us per iteration of the fixed 40-iteration graph, every pass a fresh registration, HIP events around
one pass behind a leading one (icp_time_run_fixed_tail) — the median of `runs` such passes — with the rule off, on (max_gap 20), on
together with one-to-one, and with one-to-one alone (the yardstick of a rule in the separate form: stored outputs, two small passes,
on point-to-point the apply pass); icp_time_kernels' mean search stage with the rule off, in the same run; and the moving set's construction:
the wall clock of icp_build_rbc + icp_sync with the rule on minus the same with it off, medians of `runs`.
`excess`: the rule-on iteration minus (the rule-off iteration + the search stage) as a share of that sum.

Benefit.  icp_checks' partial-overlap scene (1 degree, (8, -4, 5) mm, a quarter of M moved 150 mm off): rotation and translation error
against the ground truth after icp_run with the rule off, one-to-one, reciprocal with max_gap 0 and reciprocal with max_gap 20.

Prints one line per configuration and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import icp_amd  # noqa: E402
from icp_amd import workloads as W  # noqa: E402

CONFIGS = {"16384": (128, 256, 1), "65536": (256, 1024, 1), "2^20": (1024, 4096, 1), "64x16384": (128, 256, 64)}
ITERATIONS = 40


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


def build_us(g, runs):
    us = []
    for _ in range(runs + 3):
        t0 = time.perf_counter()
        g.buildRBC()
        g.sync()
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us[3:])


def cost(name, runs):
    side, nr, batch = CONFIGS[name]
    out = {}
    for metric, plane in (("point_to_point", False), ("point_to_plane", True)):
        g = handle(side, nr, batch, plane)
        off = iteration_us(g, runs)
        search = round(g.time_kernels(20 if side <= 256 else 5)["search"] * 1e3, 2)
        build_off = build_us(g, runs)
        g.set_unique(True)
        alone = iteration_us(g, runs)
        g.set_unique(False)
        g.set_reciprocal(True, 20.0)
        build_on = build_us(g, runs)
        on = iteration_us(g, runs)
        words = g.read(icp_amd.Memory.RECIPROCAL).tolist()
        g.set_unique(True)
        both = iteration_us(g, runs)
        g.close()
        r = {"off_us": off, "on_us": on, "on_with_one_to_one_us": both, "one_to_one_alone_us": alone, "search_stage_us": search,
             "moving_set_build_us": round(build_on - build_off, 2), "build_rbc_off_us": round(build_off, 2), "build_rbc_on_us": round(build_on, 2),
             "excess": round((on - (off + search)) / (off + search), 3), "words_last_iteration": words}
        out[metric] = r
        print("%-9s %-14s off %8.2f us   on %8.2f us   on + one-to-one %8.2f us   one-to-one alone %8.2f us   search stage %8.2f us   excess %+6.1f %%   moving set %8.2f us"
              % (name, metric, off, on, both, alone, search, 100.0 * r["excess"], r["moving_set_build_us"]))
    return out


def partial_overlap():
    """icp_checks._partial_overlap, restated (the diagnostics do not import the tests)."""
    F, M, T_true = icp_amd.synth_pair_scene(128, rot_deg=1.0, t=(8.0, -4.0, 5.0))
    M = M.copy()
    M[np.arange(128 * 128) >= 96 * 128, 2] -= 150.0
    return F, M, T_true


def benefit():
    F, M, T_true = partial_overlap()
    out = {}
    for name, unique, gap in (("off", False, None), ("one-to-one", True, None), ("reciprocal, max_gap 0", False, 0.0), ("reciprocal, max_gap 20", False, 20.0)):
        g = icp_amd.ICP(0)
        g.init(F.shape[0], 256, 2e2, 1e-6)
        g.setPowerMode(icp_amd.PowerMode.SQUARED)
        g.set_unique(unique)
        if gap is not None:
            g.set_reciprocal(True, gap)
        g.write(icp_amd.Memory.F, F)
        g.write(icp_amd.Memory.M, M)
        g.buildRBC()
        k = g.run()
        T = g.read(icp_amd.Memory.T).copy()
        g.close()
        out[name] = {"k": k, "rotation_error_deg": round(W.rotation_error_deg(T, T_true), 4),
                     "translation_error_mm": round(float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7].astype(np.float64))), 3)}
        print("partial overlap  %-24s k = %2d   %.3f deg   %.2f mm" % (name, k, out[name]["rotation_error_deg"], out[name]["translation_error_mm"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", default=",".join(CONFIGS))
    args = ap.parse_args()
    out = {"cost": {}}
    for name in args.sizes.split(","):
        out["cost"][name] = cost(name, args.runs)
    out["partial_overlap"] = benefit()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
