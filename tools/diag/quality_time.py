"""Diagnostic (not a test): what a call of icp_evaluate costs, beside the search-stage time of the same run from icp_time_kernels.

    python tools/diag/quality_time.py [--calls N]

At A (16384 / 256), B (65536 / 1024) and A x 64: the handle registers its pair (icp_run), then `calls` blocking evaluations back to
back on the wall clock — a call is the search into the evaluation's own buffers, the pair pass, the one-block second level, the copy
of the result words and the wait for it — the median and the best of them, and icp_time_kernels' mean search stage (HIP events
around the stage as a launch of its own).  Prints one line per configuration and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import icp_amd  # noqa: E402

CONFIGS = {"A": (128, 256, 1), "B": (256, 1024, 1), "Ax64": (128, 256, 64)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=300)
    args = ap.parse_args()
    out = {}
    for name, (side, nr, batch) in CONFIGS.items():
        g = icp_amd.ICP(0)
        g.init(side * side, nr, 2e2, 1e-6, batch=batch)
        g.setPowerMode(icp_amd.PowerMode.SQUARED)
        for b in range(batch):
            F, M = icp_amd.synth_pair(side, seed=0x1C9D5EED + b)
            g.write(icp_amd.Memory.F, F, batch_index=b)
            g.write(icp_amd.Memory.M, M, batch_index=b)
        g.buildRBC()
        g.run()
        for _ in range(20):
            q = g.evaluate(10.0)[0]
        us = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            g.evaluate(10.0)
            us.append((time.perf_counter() - t0) * 1e6)
        search = g.time_kernels(40)["search"] * 1e3
        g.close()
        out[name] = {"evaluate_us_median": round(statistics.median(us), 2), "evaluate_us_best": round(min(us), 2), "search_stage_us": round(search, 2)}
        print("%-5s icp_evaluate %8.2f us per call (median; best %8.2f)   search stage %8.2f us   fitness %.4f rmse %.3f"
              % (name, statistics.median(us), min(us), search, q.fitness, q.inlier_rmse))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
