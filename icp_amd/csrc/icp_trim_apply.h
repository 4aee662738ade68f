// icp_trim_apply.h — the pass that rewrites the weights behind the search (include/icp_amd.h: trimming, the robust loss) and the key of
// a pair.  The pass is trim_apply<FUSED, ROBUST> below, one body behind two __global__ names: k_trim_apply<FUSED> in icp_trim.hip
// (ROBUST false: trimming, the pair filter, one-to-one correspondences) and k_trim_apply_robust<FUSED> in icp_robust.hip (true: a
// point-to-point robust loss), so that each translation unit keeps its own kernel list.
//
// One acceptance rule for both: a pair is accepted iff it is a candidate and, with trimming on, among the K closest (key <= t, K != 0).
// icp_trimming (p) is a uniform test of the kernel argument p.reject; trimming's words (area = ICP_AREA_TRIM's, always) are read under
// it only.  With trimming off the pass accepts every candidate the passes in front of it left: nobody forges words for it.
//
// The key of a pair is the bit pattern of its geo (icp_pair_geo, icp_pair_rule.h) in fp32: a non-negative float orders as its bits
// do as uint32.  A pair that is no candidate — weight 0, geo not finite, no query — gets the key ~0u, above every candidate's.
#pragma once
#include "icp_search.h"
#include "icp_pair_rule.h"

namespace {

constexpr uint32_t TRIM_NONE = 0xFFFFFFFFu;     // the key of a pair that is no candidate

__device__ __forceinline__ uint32_t trim_key (float4 f, float4 q)
{
    if (f.w == 0.f) return TRIM_NONE;
    const float geo = icp_pair_geo (f, q);
    return geo < __builtin_inff () ? __float_as_uint (geo) : TRIM_NONE;      // (NaN and +inf: no candidate)
}

// ------------------------------------------------------------------------------------------
// trim_apply<FUSED, ROBUST> — one wave per block of the search, grid (nb | 2 nwg, batch), launch bounds 64.  Pair e of the block is the
// search's query e (fused: fused_query_index of tile blockIdx.x; reference order: group blockIdx.x / 2, parity blockIdx.x & 1).  A
// trimmed pair's weight becomes +0 in PF.w (the W output).  ROBUST (a point-to-point robust loss, icp_set_robust_loss): an accepted
// pair's weight becomes W' = (float) ((double) w * omega (geo / k^2)), k = *icp_robust_scale (p), and a W' of 0 makes it a rejected
// pair.  Then the block's partials are written again from PF / PM as ks_epilogue
// computes them: the 18 double moments of its 64 pairs (an accepted pair's terms from the same floats, a trimmed pair's exact zeros)
// through the same halving tree into p.mom's slot of the tile, or the weight partial (row_tree4) into p.wpart.
// ------------------------------------------------------------------------------------------
template <bool FUSED, bool ROBUST>
__device__ __forceinline__ void trim_apply (icp_params p, const uint32_t *area, uint32_t tpr_magic)
{
    __shared__ double s_mom[FUSED ? ICP_NMOM : 1][64];
    __shared__ float s_w[64];
    const uint32_t b = blockIdx.y, lane = threadIdx.x, m = p.m;
    if (icp_pass_leaves (p, b)) return;
    const uint32_t i = FUSED ? fused_query_index (m, p.side, tpr_magic, blockIdx.x, lane) : (blockIdx.x >> 1) * 128u + 2u * lane + (blockIdx.x & 1u);
    const bool v = i < m;
    float4 f = make_float4 (0.f, 0.f, 0.f, 0.f), q = f;
    if (v) { f = p.PF[(size_t) b * m + i]; q = p.PM[(size_t) b * m + i]; }
    const uint32_t key = v ? trim_key (f, q) : TRIM_NONE;
    // acc = key != TRIM_NONE && (!icp_trimming (p) || (K != 0u && key <= t)), trimming's words read under the uniform test only
    bool acc = key != TRIM_NONE;
    if (icp_trimming (p)) { const uint32_t t = area[4u * b], K = area[4u * b + 2u]; acc = acc && K != 0u && key <= t; }
    if constexpr (ROBUST) {
        const double k = (double) *icp_robust_scale (p), k2 = k * k, u = (double) __uint_as_float (key) / k2;
        const float wr = acc ? (float) ((double) f.w * icp_robust_omega (icp_robust (p), u)) : 0.f;
        if (v && f.w != 0.f) reinterpret_cast<float *> (p.PF + (size_t) b * m + i)[3] = wr;
        acc = wr != 0.f;
        f.w = wr;
    } else {
        if (v && f.w != 0.f && !acc) icp_pair_reject (p.PF + (size_t) b * m + i);
    }
    if constexpr (FUSED) {
        // (ks_epilogue's products, term for term)
        double W = acc ? (double) f.w : 0.0;
        double g0 = acc ? (double) f.x : 0.0, g1 = acc ? (double) f.y : 0.0, g2 = acc ? (double) f.z : 0.0;
        double q0 = acc ? (double) q.x : 0.0, q1 = acc ? (double) q.y : 0.0, q2 = acc ? (double) q.z : 0.0;
        double wq0 = W * q0, wq1 = W * q1, wq2 = W * q2;
        s_mom[0][lane] = W;
        s_mom[1][lane] = W * g0; s_mom[2][lane] = W * g1; s_mom[3][lane] = W * g2;
        s_mom[4][lane] = wq0; s_mom[5][lane] = wq1; s_mom[6][lane] = wq2;
        s_mom[7][lane] = wq0 * g0; s_mom[8][lane] = wq0 * g1; s_mom[9][lane] = wq0 * g2;
        s_mom[10][lane] = wq1 * g0; s_mom[11][lane] = wq1 * g1; s_mom[12][lane] = wq1 * g2;
        s_mom[13][lane] = wq2 * g0; s_mom[14][lane] = wq2 * g1; s_mom[15][lane] = wq2 * g2;
        s_mom[16][lane] = W * ((g0 * g0 + g1 * g1) + g2 * g2);
        s_mom[17][lane] = W * ((q0 * q0 + q1 * q1) + q2 * q2);
        __syncthreads ();
        // the search's halving tree over the 64 pairs, one 16-lane row per moment (four moments per round)
        const uint32_t l = lane & 15u;
        double *mom = p.mom + (size_t) b * 2 * ICP_NMOM * p.nb;
#pragma unroll
        for (uint32_t r = 0; r < (ICP_NMOM + 3u) / 4u; ++r) {
            const uint32_t mrow = r * 4u + (lane >> 4), k = min (mrow, (uint32_t) ICP_NMOM - 1u);
            double c0 = s_mom[k][l] + s_mom[k][l + 32], c1 = s_mom[k][l + 16] + s_mom[k][l + 48];
            double s = row_tree_tail_d (c0 + c1);
            if (l == 0 && mrow < ICP_NMOM) mom[(size_t) mrow * p.nb + blockIdx.x] = s;
        }
    } else {
        s_w[lane] = acc ? f.w : 0.f;
        __syncthreads ();
        const uint32_t l = lane & 15u;
        float a[4] = { s_w[l], s_w[l + 16], s_w[l + 32], s_w[l + 48] };
        float s = row_tree4 (a);
        if (lane == 0) p.wpart[(size_t) b * 2 * p.nwp + blockIdx.x] = s;
    }
}


}  // namespace
