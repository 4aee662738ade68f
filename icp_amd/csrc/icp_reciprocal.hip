// icp_reciprocal.hip — reciprocal (forward–backward consistent) correspondences (icp_set_reciprocal, include/icp_amd.h): a candidate pair
// (m_i, f_j) keeps its weight only if the moving point f_j finds when it searches the moving frame is m_i itself (exact), or lies within
// max_gap of it (near); every other candidate gets the weight +0 in PF.w and is then exactly a rejected pair.
//
// An iteration with the rule on is: the REJ search (icp_search_rej.hip), which stores its per-query outputs; the pair filter when it is
// on; then the three additions of this file (icp_launch_reciprocal) —
//   k_reciprocal_state: per registration, the reverse state = the run's state with T replaced by the inverse T' of the transform the
//     forward search of this iteration used (p.st[b].T: only the tail of the iteration changes it);
//   the back search: the engine's own search (icp_launch_search) on a copy of the parameters with F and M swapped, the moving set
//     (an RBC over M: icp_launch_reciprocal_build) as its database, the reverse state, buffers of its own, reference order, REGULAR,
//     every opt-in rule off — it writes nothing but its per-query outputs (ICP_MEM_REVERSE_ID);
//   k_reciprocal: one thread per pair, the test, the counts —
// then one-to-one, trimming's selection and the apply pass as before (the order: icp_route_of, icp_kernels.hip), and the unchanged tail.
// None of the existing kernels carries any of this code.  Built with -ffp-contract=off like every other translation unit: each expression
// below is evaluated exactly in the order it is written; tests/reciprocal_ref.py restates the inverse and the rule.
//
// All three launches leave a converged registration of a checked run alone under the test the other passes use (p.check && st.done): the
// state kernel copies `done` with the rest, so the back search's own test agrees with the run's.  (It writes the reverse state of such a
// registration again — the same words: T has not changed since.)
//
// Counting follows one-to-one's passes: the state kernel's first lane resets the registration's result words (n, exact, near, accepted:
// ICP_MEM_RECIPROCAL), k_reciprocal's blocks add their integer counts to them (pair_counts_add, icp_pair_rule.h, which says why no
// ticket).  The two kernels are launched together and test the same flag, which only the tail behind them changes.
#include "icp_rbc_set.h"
#include "icp_pair_rule.h"
#include <cstdio>
#include <cstdlib>

namespace {

constexpr uint32_t RECIPROCAL_BLOCK = 256u;

// The reverse state's guard word (icp_reg_state::reserved1, which nothing else reads): 1 = T had no inverse (s not finite or not > 0, or a
// component of T' not finite) — T' is the identity and k_reciprocal rejects every candidate of the iteration.
#define RECIPROCAL_GUARD reserved1

// ------------------------------------------------------------------------------------------
// k_reciprocal_state — one wave per registration, grid = batch.  Lane t copies dword t of the state; lane 0 then writes T'.
// T = [x y z w | tx ty tz s]: R = R (q) as written below, T' = [-x -y -z w | -(R^T t) / s, 1 / s], in double.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (64) void k_reciprocal_state (icp_params p, icp_reg_state *rst, uint32_t *result)
{
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    const icp_reg_state *st = p.st + b;
    icp_reg_state *out = rst + b;
    constexpr uint32_t T0 = offsetof (icp_reg_state, T) / 4u, G0 = offsetof (icp_reg_state, RECIPROCAL_GUARD) / 4u;
    // (T and the guard word are lane 0's: one writer per dword)
    if (t < sizeof (icp_reg_state) / 4u && !(t >= T0 && t < T0 + 8u) && t != G0)
        reinterpret_cast<uint32_t *> (out)[t] = reinterpret_cast<const uint32_t *> (st)[t];
    if (t != 0u) return;
    if (!icp_pass_leaves (p, b)) { uint32_t *w = result + 4u * b; w[0] = 0u; w[1] = 0u; w[2] = 0u; w[3] = 0u; }     // (a converged registration: its last iteration's counts stay)
    const double x = (double) st->T[0], y = (double) st->T[1], z = (double) st->T[2], w = (double) st->T[3];
    const double tx = (double) st->T[4], ty = (double) st->T[5], tz = (double) st->T[6];
    const float s = st->T[7];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const double R00 = 1.0 - 2.0 * (yy + zz), R01 = 2.0 * (xy - wz), R02 = 2.0 * (xz + wy);
    const double R10 = 2.0 * (xy + wz), R11 = 1.0 - 2.0 * (xx + zz), R12 = 2.0 * (yz - wx);
    const double R20 = 2.0 * (xz - wy), R21 = 2.0 * (yz + wx), R22 = 1.0 - 2.0 * (xx + yy);
    const double si = 1.0 / (double) s;
    const double u0 = (R00 * tx + R10 * ty) + R20 * tz, u1 = (R01 * tx + R11 * ty) + R21 * tz, u2 = (R02 * tx + R12 * ty) + R22 * tz;
    float Ti[8] = { -st->T[0], -st->T[1], -st->T[2], st->T[3], (float) -(u0 * si), (float) -(u1 * si), (float) -(u2 * si), (float) si };
    bool ok = isfinite (s) && s > 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) ok = ok && isfinite (Ti[k]);
    if (!ok) { Ti[0] = Ti[1] = Ti[2] = 0.f; Ti[3] = 1.f; Ti[4] = Ti[5] = Ti[6] = 0.f; Ti[7] = 1.f; }
#pragma unroll
    for (int k = 0; k < 8; ++k) out->T[k] = Ti[k];
    out->RECIPROCAL_GUARD = ok ? 0u : 1u;
}

// ------------------------------------------------------------------------------------------
// k_reciprocal — one thread per pair, grid (ceil (m / 256), batch).  rev: the back search's (dist, id) per fixed point; result, gap:
// icp_words (p, ICP_AREA_RECIPROCAL) (icp_kernels.h)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (RECIPROCAL_BLOCK) void k_reciprocal (icp_params p, const icp_dist_id *rev, const icp_reg_state *rst, uint32_t *result,
                                                                   const uint32_t *gap)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * RECIPROCAL_BLOCK + threadIdx.x;
    if (icp_pass_leaves (p, b)) return;
    const float max_gap = __uint_as_float (gap[0]);
    const float gap2 = (float) ((double) max_gap * (double) max_gap);
    const bool guard = rst[b].RECIPROCAL_GUARD != 0u;
    bool cand = false, exact = false, near = false;
    if (i < p.m) {
        const size_t o = (size_t) b * p.m, e = o + i;
        const uint32_t j = p.nn_id[e].id;
        cand = icp_pair_candidate (p.PF[e].w, j, p.m);
        if (cand) {
            if (!guard) {
                const uint32_t i2 = rev[o + j].id;           // (j < m: inside the registration's rows)
                exact = i2 == i;
                if (!exact && max_gap > 0.f && i2 < p.m) {
                    const float4 a = p.PM[e], c = p.PM[o + i2];
                    const float g = icp_pair_geo (c, a);     // (of a - c)
                    near = isfinite (g) && g <= gap2;
                }
            }
            if (!exact && !near) icp_pair_reject (p.PF + e);
        }
    }
    const uint32_t wave[3] = { (uint32_t) __popcll (__ballot (cand)), (uint32_t) __popcll (__ballot (exact)), (uint32_t) __popcll (__ballot (near)) };
    uint32_t sum[3];
    if (pair_block_counts<3, RECIPROCAL_BLOCK> (wave, sum)) {
        const uint32_t words[4] = { sum[0], sum[1], sum[2], sum[1] + sum[2] };       // (n, exact, near, accepted)
        pair_counts_add (result + 4u * b, words);
    }
}

// the parameters of a search or a construction that has M as its database: F and M swapped, the moving set, no opt-in rule, no metric
icp_params reciprocal_params (const icp_params &p, const icp_reciprocal_set &rs)
{
    icp_params q = p;
    q.F = p.M; q.M = p.F;
    icp_rbc_into (q, rs.rbc);
    q.st = rs.st; q.nn_id = rs.nn_id; q.PF = rs.PF; q.PM = rs.PM; q.rid = rs.rid;
    q.fused = 0; q.weighted = 0; q.emit = 1; q.hmirror = nullptr; q.hstate = nullptr; q.dbg = nullptr;
    q.reject = 0u; q.reject_d2 = 0.f; q.reject_max_dist = 0.f; q.trim_keep = 0.f; q.metric = 0u; q.p2pl_mu = 0.f; q.gicp = 0u; q.nrm_grid = 0u;
    q.run_flag = nullptr; q.track_seq = nullptr;
    return q;
}

}  // namespace

// buildRBC over M into the moving set: the construction icp_build_rbc runs over F (same m, nr, alpha; the representatives picked from M by
// the getReps grid rule).  It leaves k / done alone (no_state_reset) and launches no normals (nrm_grid = 0 in the copy).
void icp_launch_reciprocal_build (const icp_params &p, hipStream_t s, const icp_reciprocal_set &rs)
{
    icp_params q = reciprocal_params (p, rs);
    q.check = 0; q.no_state_reset = 1u;
    icp_launch_build_rbc (q, s);
}

void icp_launch_reciprocal (const icp_params &p, hipStream_t s, const icp_reciprocal_set *rs)
{
    if (!rs || !rs->st) {                                    // (every caller inside the library hands the handle's record on: a route without it has no kernels to run)
        std::fprintf (stderr, "icp_amd: reciprocal correspondences are on and the launch has no moving set\n");
        std::abort ();
    }
    const icp_area_words w = icp_words (p, ICP_AREA_RECIPROCAL);
    hipLaunchKernelGGL (k_reciprocal_state, dim3 (p.batch), dim3 (64), 0, s, p, rs->st, w.result);
    // (the back search's first search of a registration — k == 0, copied — seeds its pruning from the query's own grid cell, like the forward
    // one; later ones from the rule's own rid buffer, any content of which is a valid seed: pruning is exact)
    icp_launch_search (reciprocal_params (p, *rs), s);
    const dim3 grid ((p.m + RECIPROCAL_BLOCK - 1u) / RECIPROCAL_BLOCK, p.batch);
    hipLaunchKernelGGL (k_reciprocal, grid, dim3 (RECIPROCAL_BLOCK), 0, s, p, (const icp_dist_id *) rs->nn_id, (const icp_reg_state *) rs->st,
                        w.result, (const uint32_t *) w.settings);
}
