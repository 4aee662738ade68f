// icp_pair_filter.hip — rejection at the fixed grid's boundary (icp_set_boundary_rejection) and by normal compatibility
// (icp_set_normal_rejection), include/icp_amd.h: one pass, k_pair_filter, right behind the REJ search (icp_route_of, icp_kernels.hip) and in
// front of one-to-one correspondences, trimming's selection and every apply pass.  A candidate pair (weight != 0, id < m) that a rule
// rejects gets the weight +0 in PF.w and is then exactly a rejected pair: the passes behind this one see no candidate in it, the apply
// pass (icp_trim_apply.h; point-to-point) writes the search blocks' partials again from the weights, and the plane metrics read w in
// their moments.  None of the existing kernels carries any of this code.  Built with -ffp-contract=off like every other translation
// unit: each expression below is evaluated exactly in the order it is written; tests/pair_filter_ref.py restates both rules.
//
// The boundary rule, grid width gw (rows = m / gw; the host refuses a width that does not divide m): the fixed point id = (x, y) =
// (id % gw, id / gw) is a boundary point when it lies on the grid's rim, or when it or one of its 8 grid neighbours in F — the
// registration's fixed set in its original order, p.F, which a tracked frame brings with it — is invalid (xyz not finite, or all zero).
// The mask is evaluated here from F, nine points per candidate that is not on the rim: nothing is kept per fixed frame.
//
// The normal rule, in double from the float inputs: N_Q = NORMALS_F[id], N_M = NORMALS_M[i] (a non-finite normal counts as zero), R =
// p.st[b].R (the cumulative rotation the search of this iteration used, as in the plane-to-plane moments), N_P = R N_M
// (plane_rot_normal), qq = (qx qx + qy qy) + qz qz, pp likewise, o = (qx px + qy py) + qz pz; the pair is compatible iff
// qq > 0 && pp > 0 && o >= (double) min_cos * sqrt (qq * pp).  min_cos is a device word: a new threshold touches no graph.
//
// Counting: the boundary test comes first, a pair is counted once, n = at_boundary + incompatible + accepted: the result words are
// (n, at_boundary, incompatible, accepted: ICP_MEM_PAIR_FILTER).  No launch stands in front of the pass that could reset them, so
// its blocks count by ticket (pair_counts_ticket, icp_pair_rule.h).  Nothing else reads the words: the apply pass behind the filter
// accepts every pair that still has a weight (icp_trim_apply.h).
#include "icp_plane_moments.h"          // (plane_finite_or_zero, plane_rot_normal; icp_pair_rule.h)

namespace {

constexpr uint32_t FILTER_BLOCK = 256u;

// fixed point id of a grid gw wide and `rows` high: on the rim, invalid, or beside an invalid point
__device__ __forceinline__ bool filter_at_boundary (const float *F, uint32_t id, uint32_t gw, uint32_t rows)
{
    const uint32_t x = id % gw, y = id / gw;
    if (x == 0u || x + 1u >= gw || y == 0u || y + 1u >= rows) return true;
    // (1 <= x <= gw - 2 and 1 <= y <= rows - 2: every index below lies in [0, rows gw) and rows gw <= m)
    bool ok = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            ok = ok && icp_point_valid (F + (size_t) ((y + dy) * gw + (x + dx)) * 8u);
    return !ok;
}

// ------------------------------------------------------------------------------------------
// k_pair_filter — one thread per pair, grid (ceil (m / 256), batch).  result, counts, settings: icp_words (p, ICP_AREA_FILTER)
// (icp_kernels.h)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (FILTER_BLOCK) void k_pair_filter (icp_params p, const float4 *nrm, const float4 *nrm_m, uint32_t *result, uint32_t *counts,
                                                                const uint32_t *settings)
{
    const uint32_t b = blockIdx.y, t = threadIdx.x, i = blockIdx.x * FILTER_BLOCK + t;
    if (icp_pass_leaves (p, b)) return;
    const float min_cos = __uint_as_float (settings[0]);
    const uint32_t gw = settings[1];
    const bool by_boundary = (p.reject & ICP_REJECT_BOUNDARY_ON) != 0u && gw != 0u, by_normal = (p.reject & ICP_REJECT_NORMAL_ON) != 0u;
    bool cand = false, bnd = false, inc = false;
    if (i < p.m) {
        const size_t o = (size_t) b * p.m, e = o + i;
        const float4 f = p.PF[e];
        const uint32_t id = p.nn_id[e].id;
        cand = icp_pair_candidate (f.w, id, p.m);
        if (cand) {
            if (by_boundary) bnd = filter_at_boundary (p.F + o * 8u, id, gw, p.m / gw);
            if (by_normal && !bnd) {
                float Rf[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) Rf[k] = p.st[b].R[k];
                const float4 nf = plane_finite_or_zero (nrm[o + id]), nm = plane_finite_or_zero (nrm_m[e]);
                double np[3];
                plane_rot_normal (Rf, nm, np);
                const double qx = (double) nf.x, qy = (double) nf.y, qz = (double) nf.z;
                const double qq = (qx * qx + qy * qy) + qz * qz, pp = (np[0] * np[0] + np[1] * np[1]) + np[2] * np[2];
                const double dot = (qx * np[0] + qy * np[1]) + qz * np[2];
                inc = !(qq > 0.0 && pp > 0.0 && dot >= (double) min_cos * sqrt (qq * pp));
            }
            if (bnd || inc) icp_pair_reject (p.PF + e);
        }
    }
    const uint32_t wave[3] = { (uint32_t) __popcll (__ballot (cand)), (uint32_t) __popcll (__ballot (bnd)), (uint32_t) __popcll (__ballot (inc)) };
    uint32_t sum[3];
    if (pair_block_counts<3, FILTER_BLOCK> (wave, sum)) pair_counts_ticket (counts + 8u * b, result + 4u * b, sum[0], sum[1], sum[2], gridDim.x);
}

}  // namespace

void icp_launch_pair_filter (const icp_params &p, hipStream_t s)
{
    const dim3 grid ((p.m + FILTER_BLOCK - 1u) / FILTER_BLOCK, p.batch);
    const icp_area_words w = icp_words (p, ICP_AREA_FILTER);
    hipLaunchKernelGGL (k_pair_filter, grid, dim3 (FILTER_BLOCK), 0, s, p, (const float4 *) icp_normals_f (p), (const float4 *) icp_normals_m (p),
                        w.result, w.running, (const uint32_t *) w.settings);
}
