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
// Counting: the boundary test comes first, a pair is counted once, n = at_boundary + incompatible + accepted.  The blocks of a
// registration add their integer counts to four running words and then take a ticket; the block that draws the last ticket — every
// other block's counts are in by then (release / acquire on the ticket, agent scope) — moves the sums into the result words
// (n, at_boundary, incompatible, accepted: ICP_MEM_PAIR_FILTER), and leaves the running words and the ticket counter zero for the
// next launch.  Integer sums: nothing depends on the order in which the device gets to the pairs.  Nothing else reads the words: the
// apply pass behind the filter accepts every pair that still has a weight (icp_trim_apply.h).
#include "icp_plane_moments.h"          // (plane_finite_or_zero, plane_rot_normal)

namespace {

constexpr uint32_t FILTER_BLOCK = 256u;

__device__ __forceinline__ bool filter_valid (const float *r)
{
    const float x = r[0], y = r[1], z = r[2];
    return isfinite (x) && isfinite (y) && isfinite (z) && !(x == 0.f && y == 0.f && z == 0.f);
}

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
            ok = ok && filter_valid (F + (size_t) ((y + dy) * gw + (x + dx)) * 8u);
    return !ok;
}

// ------------------------------------------------------------------------------------------
// k_pair_filter — one thread per pair, grid (ceil (m / 256), batch).  result, counts, settings: icp_pair_filter_area / _counts /
// _settings (icp_kernels.h)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (FILTER_BLOCK) void k_pair_filter (icp_params p, const float4 *nrm, const float4 *nrm_m, uint32_t *result, uint32_t *counts,
                                                                const uint32_t *settings)
{
    __shared__ uint32_t s_cnt[FILTER_BLOCK / 64u][4];
    const uint32_t b = blockIdx.y, t = threadIdx.x, i = blockIdx.x * FILTER_BLOCK + t;
    if (p.check && p.st[b].done) return;                     // (a converged registration: its last iteration's outputs and counts stay)
    const float min_cos = __uint_as_float (settings[0]);
    const uint32_t gw = settings[1];
    const bool by_boundary = (p.reject & ICP_REJECT_BOUNDARY_ON) != 0u && gw != 0u, by_normal = (p.reject & ICP_REJECT_NORMAL_ON) != 0u;
    bool cand = false, bnd = false, inc = false;
    if (i < p.m) {
        const size_t o = (size_t) b * p.m, e = o + i;
        const float4 f = p.PF[e];
        const uint32_t id = p.nn_id[e].id;
        cand = f.w != 0.f && id < p.m;
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
            if (bnd || inc) reinterpret_cast<float *> (p.PF + e)[3] = 0.f;
        }
    }
    const uint32_t wn = (uint32_t) __popcll (__ballot (cand)), wb = (uint32_t) __popcll (__ballot (bnd)), wi = (uint32_t) __popcll (__ballot (inc));
    if ((t & 63u) == 0u) { s_cnt[t >> 6][0] = wn; s_cnt[t >> 6][1] = wb; s_cnt[t >> 6][2] = wi; }
    __syncthreads ();
    if (t == 0u) {
        uint32_t sn = 0u, sb = 0u, si = 0u;
#pragma unroll
        for (uint32_t v = 0; v < FILTER_BLOCK / 64u; ++v) { sn += s_cnt[v][0]; sb += s_cnt[v][1]; si += s_cnt[v][2]; }
        uint32_t *run = counts + 8u * b;
        if (sn) __hip_atomic_fetch_add (run + 0, sn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sb) __hip_atomic_fetch_add (run + 1, sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (si) __hip_atomic_fetch_add (run + 2, si, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t ticket = __hip_atomic_fetch_add (run + 4, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket + 1u == gridDim.x) {                      // (the last block of the registration: every count is in)
            const uint32_t n = __hip_atomic_exchange (run + 0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t nb = __hip_atomic_exchange (run + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t ni = __hip_atomic_exchange (run + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store (run + 4, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t *out = result + 4u * b;
            out[0] = n; out[1] = nb; out[2] = ni; out[3] = n - nb - ni;
        }
    }
}

}  // namespace

void icp_launch_pair_filter (const icp_params &p, hipStream_t s)
{
    const dim3 grid ((p.m + FILTER_BLOCK - 1u) / FILTER_BLOCK, p.batch);
    hipLaunchKernelGGL (k_pair_filter, grid, dim3 (FILTER_BLOCK), 0, s, p, (const float4 *) icp_normals_f (p), (const float4 *) icp_normals_m (p),
                        icp_pair_filter_area (p), icp_pair_filter_counts (p), icp_pair_filter_settings (p));
}
