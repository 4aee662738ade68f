"""Diagnostic (not a test, no GPU): how many queries the rule of icp_amd/csrc/icp_bounds.h keeps per iteration, simulated in float64 over
the oracle's own transforms (fused reductions + squared power start, the benchmarked modes).

    python tools/diag/bounds_sim.py [--side 128] [--nr 256] [--seed N] [--iterations 40] [--qpw 4]

Per iteration: the median query drift, the share of the queries that must scan stage 1 / stage 2 again, and — with the scanning queries
of every 64-query block handed over first (the chained search's order), --qpw queries per wave — the waves that still work in the worst
block and on average.  The bounds are those of the kernel: the runner-up of a stage at its last scan, minus the drift since."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
KAPPA, TAU = 2.0 ** -16, 2.0 ** -50


def transform(T, P):
    q, w, t, s = T[:3].astype(np.float64), float(T[3]), T[4:7].astype(np.float64), float(T[7])
    u = np.cross(q, P) + w * P
    return s * (P + np.cross(2 * q, u)) + t


def blocks_of(side, m):
    """query indices of every 64-query block (8 x 8 tiles of the grid where its side is a multiple of 8)"""
    if side % 8 == 0:
        idx = np.arange(m).reshape(side // 8, 8, side // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
        return [b for b in idx]
    return [np.arange(s, min(s + 64, m)) for s in range(0, m, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--nr", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0x1C9D5EED)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--a", type=float, default=2e2)
    ap.add_argument("--qpw", type=int, default=4, help="queries per wave (chained / latency form: 4, dense forms: 8)")
    o_ = ap.parse_args()
    import icp_amd
    from oracle import oracle as O
    side, nr, m, a = o_.side, o_.nr, o_.side * o_.side, o_.a
    F, M = icp_amd.synth_pair(side, seed=o_.seed)
    o = O.OracleICP(m, nr, a, 1e-6, threads=8, power_fast=True, fused=True, max_iterations=o_.iterations)
    o.write_f(F); o.write_m(M); o.build_rbc()
    sa = np.sqrt(a)
    six = lambda X: np.concatenate([X[:, :3].astype(np.float64), sa * X[:, 4:7].astype(np.float64)], axis=1)
    R6, F6 = six(o.reps), six(F)
    perm, Ol, Nl = o.rbc_perm, o.rbc_O, o.rbc_N
    P, C = M[:, :3].astype(np.float64), sa * M[:, 4:7].astype(np.float64)
    blocks = blocks_of(side, m)
    lo1 = np.zeros(m); lo2 = np.zeros(m); rwin = np.zeros(m, np.int64); jwin = np.full(m, -1, np.int64); prev = None
    nw = 64 // o_.qpw
    print("it  drift (mm)  scan s1  scan s2   worst block waves s1 / s2 (of %d)   mean waves s1 / s2" % nw)
    tot = np.zeros(4)
    for it in range(o_.iterations):
        Q = np.concatenate([transform(o.T, P), C], axis=1)
        if prev is None:
            need1 = np.ones(m, bool); need2 = np.ones(m, bool); drift = np.zeros(m)
        else:
            drift = np.linalg.norm(Q[:, :3] - prev, axis=1)
            lo1 = lo1 - drift * (1 + KAPPA) - KAPPA * lo1 - TAU
            lo2 = lo2 - drift * (1 + KAPPA) - KAPPA * lo2 - TAU
            u1 = np.linalg.norm(Q - R6[rwin], axis=1)
            has = jwin >= 0
            u2 = np.where(has, np.linalg.norm(Q - F6[np.where(has, jwin, 0)], axis=1), 0.0)
            keep1 = u1 * (1 + KAPPA) + TAU < lo1
            need1 = ~keep1
            need2 = need1 | (has & ~(u2 * (1 + KAPPA) + TAU < lo2))
        prev = Q[:, :3].copy()
        for i in np.nonzero(need1)[0]:
            d = np.linalg.norm(R6 - Q[i], axis=1)
            order = np.argsort(d, kind="stable")
            rwin[i] = order[0]
            lo1[i] = d[order[1]] * (1 - KAPPA) - TAU if nr > 1 else np.inf
        for i in np.nonzero(need2)[0]:
            r = rwin[i]
            if Nl[r] == 0:
                jwin[i], lo2[i] = -1, np.inf
                continue
            members = perm[Ol[r]:Ol[r] + Nl[r]]
            d = np.linalg.norm(F6[members] - Q[i], axis=1)
            order = np.argsort(d, kind="stable")
            jwin[i] = members[order[0]]
            lo2[i] = d[order[1]] * (1 - KAPPA) - TAU if len(members) > 1 else np.inf
        w1 = np.array([-(-np.count_nonzero(need1[b]) // o_.qpw) for b in blocks])
        w2 = np.array([-(-np.count_nonzero(need2[b]) // o_.qpw) for b in blocks])
        row = (need1.mean(), need2.mean(), w1.mean() / nw, w2.mean() / nw)
        if it:
            tot += row
        print("%2d  %8.4f   %5.1f %%  %5.1f %%      %2d / %2d                              %4.1f / %4.1f" %
              (it + 1, np.median(drift) if it else 0.0, 100 * row[0], 100 * row[1], w1.max(), w2.max(), w1.mean(), w2.mean()))
        o.step()
    n = max(o_.iterations - 1, 1)
    print("mean over iterations 2 .. %d: scan stage 1 %.1f %%, stage 2 %.1f %%; waves that work %.1f %% / %.1f %%" %
          (o_.iterations, 100 * tot[0] / n, 100 * tot[1] / n, 100 * tot[2] / n, 100 * tot[3] / n))


if __name__ == "__main__":
    main()
