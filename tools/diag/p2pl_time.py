"""Diagnostic (not a test): microseconds per iteration of point-to-plane ICP (icp_set_error_metric) against the default point-to-point
iteration, at A (16384 / 256), B (65536 / 1024) and A x 64, through the fixed-length run graphs bench.py times.

    python tools/diag/p2pl_time.py [--only-p2pl] [--reps N]

Prints one line per configuration and one JSON line at the end.  Under `rocprofv3 --kernel-trace --stats` (--only-p2pl) the per-kernel
table shows the search, k_p2pl_moments and k_p2pl_finalize."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import icp_amd  # noqa: E402

CONFIGS = {"A": (128, 256, 1), "B": (256, 1024, 1), "Ax64": (128, 256, 64)}


def per_iteration_us(side, nr, batch, p2pl, iterations, reps):
    g = icp_amd.ICP(0)
    g.init(side * side, nr, 2e2, 1e-6, batch=batch)
    g.setPowerMode(icp_amd.PowerMode.SQUARED)
    if p2pl:
        g.set_normals(icp_amd.Normals.GRID, side)
        g.set_error_metric(icp_amd.ErrorMetric.POINT_TO_PLANE, 0.05)
    for b in range(batch):
        F, M = icp_amd.synth_pair(side, seed=0x1C9D5EED + b)
        g.write(icp_amd.Memory.F, F, batch_index=b)
        g.write(icp_amd.Memory.M, M, batch_index=b)
    g.buildRBC()
    g.time_run_fixed(iterations, 2, True)                   # (warm-up: graph capture, clocks)
    best = min(g.time_run_fixed(iterations, reps, True) for _ in range(3))
    form, launches = g.run_form(), g.launches_per_iteration()
    g.close()
    return best * 1e3 / (iterations * reps), form, launches


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--only-p2pl", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    out = {}
    for name, (side, nr, batch) in CONFIGS.items():
        for p2pl in ((True,) if args.only_p2pl else (False, True)):
            us, form, launches = per_iteration_us(side, nr, batch, p2pl, 20, args.reps)
            key = "%s_%s" % (name, "p2pl" if p2pl else "p2p")
            out[key] = round(us, 3)
            print("%-10s %-5s %8.3f us/iteration  (form %d, %d launches per iteration)" % (name, "p2pl" if p2pl else "p2p", us, form, launches))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
