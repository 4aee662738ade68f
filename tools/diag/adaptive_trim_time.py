"""Diagnostic (not a test): what adaptive trimming (icp_set_adaptive_trimming) costs per iteration, and where it ends.

    python tools/diag/adaptive_trim_time.py [--runs N] [--sizes 16384,65536,2^20,64x16384]

Cost.  At |F| = 16384 (256 representatives), 65536 (1024), 2^20 (4096) and 64 batched registrations of 16384, for point-to-point and
point-to-plane (grid normals): us per iteration of the fixed 40-iteration graph, every pass a fresh registration, HIP events around
one pass behind a leading one (icp_time_run_fixed_tail) — the median of `runs` such passes — with the rule off, with the rule on
(0.05 .. 0.95, q = 4), and with fixed trimming at 0.75, in the same run.  Fixed trimming is the yardstick: the same search, the same
apply pass and the same tail; the rule takes one selection launch at every size where trimming takes one up to 16384 pairs and three
beyond.

Where it ends.  icp_checks' partial-overlap scene (1 degree, (8, -4, 5) mm, a quarter of M moved 150 mm off): rotation and translation
error against the ground truth and the last kept fraction after icp_run with the rule off, with fixed trimming at 0.75 (the true
overlap, which the rule is not told) and with the rule at q = 3, 4 and 7.

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
RULE = (0.05, 0.95, 4)
KEEP = 0.75


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
    out = {}
    for metric, plane in (("point_to_point", False), ("point_to_plane", True)):
        g = handle(side, nr, batch, plane)
        off = iteration_us(g, runs)
        g.set_adaptive_trimming(*RULE)
        on = iteration_us(g, runs)
        words = g.read(icp_amd.Memory.TRIM).tolist() + g.read(icp_amd.Memory.TRIM_ADAPTIVE).tolist()
        launches = g.launches_per_iteration()
        g.set_adaptive_trimming(0.0, 0.0, 0)
        g.set_trimming(KEEP)
        trim = iteration_us(g, runs)
        trim_launches = g.launches_per_iteration()
        g.close()
        out[metric] = {"off_us": off, "on_us": on, "trim_0.75_us": trim, "launches_on": launches, "launches_trim": trim_launches,
                       "on_over_trim": round(on / trim, 3), "words_last_iteration": words}
        print("%-9s %-14s off %8.2f us   on %8.2f us (%d launches)   trimming 0.75 %8.2f us (%d launches)   on / trimming %.3f"
              % (name, metric, off, on, launches, trim, trim_launches, on / trim))
    return out


def partial_overlap():
    """icp_checks._partial_overlap, restated (the diagnostics do not import the tests)."""
    F, M, T_true = icp_amd.synth_pair_scene(128, rot_deg=1.0, t=(8.0, -4.0, 5.0))
    M = M.copy()
    M[np.arange(128 * 128) >= 96 * 128, 2] -= 150.0
    return F, M, T_true


def where_it_ends():
    F, M, T_true = partial_overlap()
    out = {}
    for name, keep, q in (("off", 1.0, 0), ("trimming 0.75", KEEP, 0), ("q = 3", 1.0, 3), ("q = 4", 1.0, 4), ("q = 7", 1.0, 7)):
        g = icp_amd.ICP(0)
        g.init(F.shape[0], 256, 2e2, 1e-6)
        g.setPowerMode(icp_amd.PowerMode.SQUARED)
        g.set_trimming(keep)
        g.set_adaptive_trimming(RULE[0], RULE[1], q)
        g.write(icp_amd.Memory.F, F)
        g.write(icp_amd.Memory.M, M)
        g.buildRBC()
        k = g.run()
        T = g.read(icp_amd.Memory.T).copy()
        words = g.read(icp_amd.Memory.TRIM)
        g.close()
        out[name] = {"k": k, "rotation_error_deg": round(W.rotation_error_deg(T, T_true), 4),
                     "translation_error_mm": round(float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7].astype(np.float64))), 3),
                     "kept_fraction": round(float(words[2]) / float(words[1]), 4) if words[1] else None}
        print("partial overlap  %-14s k = %2d   %.3f deg   %.2f mm   kept %s"
              % (name, k, out[name]["rotation_error_deg"], out[name]["translation_error_mm"], out[name]["kept_fraction"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", default=",".join(CONFIGS))
    args = ap.parse_args()
    out = {"cost": {}}
    for name in args.sizes.split(","):
        out["cost"][name] = cost(name, args.runs)
    out["partial_overlap"] = where_it_ends()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
