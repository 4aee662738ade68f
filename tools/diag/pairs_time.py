"""Diagnostic (not a test): what a call of icp_correspondences costs, beside icp_evaluate and the search stage of the same run.

    python tools/diag/pairs_time.py [--calls N]

At |F| = 16384 (128 x 128, 256 representatives) and |F| = 2^20 (1024 x 1024, 4096): the handle registers its pair (icp_run), then
`calls` blocking calls back to back on the wall clock of
  - icp_correspondences (ICP_PAIRS_EVALUATED, 10 mm): the search into the evaluation's own buffers, the count pass, the scatter pass, the
    copy of the count words and the wait for it;
  - icp_correspondences (ICP_PAIRS_LAST_ITERATION): the two passes over the stored outputs, the copy, the wait — no search;
  - icp_evaluate (10 mm): the yardstick — the same search, the same number of launches, the same host wait;
the median and the best of each, the set's length, and icp_time_kernels' mean search stage (HIP events around the stage as a launch
of its own).  Prints one line per configuration and one JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import icp_amd  # noqa: E402

CONFIGS = {"16384": (128, 256), "2^20": (1024, 4096)}


def timed(fn, calls):
    for _ in range(5):
        fn()
    us = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(us), 2), round(min(us), 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    L = icp_amd.lib()
    out = {}
    for name, (side, nr) in CONFIGS.items():
        g = icp_amd.ICP(0)
        g.init(side * side, nr, 2e2, 1e-6)
        g.setPowerMode(icp_amd.PowerMode.SQUARED)
        F, M = icp_amd.synth_pair(side)
        g.write(icp_amd.Memory.F, F)
        g.write(icp_amd.Memory.M, M)
        g.buildRBC()
        g.run()
        n = C.c_uint32()
        q = (icp_amd.Quality * 1)()
        # (the C calls themselves: no record is copied to the host)
        ev = timed(lambda: g._chk(L.icp_correspondences(g._h, icp_amd.Pairs.EVALUATED, 10.0, C.byref(n), 1)), args.calls)
        n_ev = n.value
        last = timed(lambda: g._chk(L.icp_correspondences(g._h, icp_amd.Pairs.LAST_ITERATION, 0.0, C.byref(n), 1)), args.calls)
        n_last = n.value
        qual = timed(lambda: g._chk(L.icp_evaluate(g._h, 10.0, q, 1)), args.calls)
        search = round(g.time_kernels(40 if side <= 256 else 10)["search"] * 1e3, 2)
        g.close()
        out[name] = {"evaluated_us_median": ev[0], "evaluated_us_best": ev[1], "evaluated_pairs": n_ev,
                     "last_iteration_us_median": last[0], "last_iteration_us_best": last[1], "last_iteration_pairs": n_last,
                     "evaluate_us_median": qual[0], "evaluate_us_best": qual[1], "n_inliers": q[0].n_inliers, "search_stage_us": search}
        print("%-6s EVALUATED %9.2f us (best %9.2f, %7d pairs)   LAST_ITERATION %9.2f us (best %9.2f, %7d pairs)   icp_evaluate %9.2f us (best %9.2f)"
              "   search stage %9.2f us" % (name, ev[0], ev[1], n_ev, last[0], last[1], n_last, qual[0], qual[1], search))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
