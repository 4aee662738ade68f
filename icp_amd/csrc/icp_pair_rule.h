// icp_pair_rule.h — which pairs of a search count, once, for the two kernels that ask: k_quality_pairs (icp_quality.hip: icp_evaluate's
// sums and counts) and k_pairs_count / k_pairs_scatter (icp_pairs.hip: icp_correspondences' set of ICP_PAIRS_EVALUATED).  The count of
// the one is the length of the other because both evaluate this expression.  Every translation unit is built with -ffp-contract=off:
// each expression is evaluated in the order it is written; tests/quality_ref.py (masks, geo_of) restates them.
//
// Pair i, with e = PM[i].xyz (the transformed moving point), f = PF[i].xyz (the returned fixed point), mv = M[i].xyz:
//   counted = i < m, mv finite and not (0, 0, 0)                              (icp_pair_counted)
//   geo = (gx gx + gy gy) + gz gz in fp32, g = e - f componentwise            (icp_pair_geo: the rejection rule's quantity)
//   inlier = counted, f not (0, 0, 0), geo finite, and geo <= d2 unless the distance test is off        (icp_pair_inlier)
#pragma once

static __device__ __forceinline__ bool icp_pair_counted (bool in_range, const float4 &mv)
{
    return in_range && isfinite (mv.x) && isfinite (mv.y) && isfinite (mv.z) && !(mv.x == 0.f && mv.y == 0.f && mv.z == 0.f);
}

static __device__ __forceinline__ float icp_pair_geo (const float4 &f, const float4 &e)
{
    const float gx = e.x - f.x, gy = e.y - f.y, gz = e.z - f.z;
    return (gx * gx + gy * gy) + gz * gz;
}

static __device__ __forceinline__ bool icp_pair_inlier (bool counted, const float4 &f, float geo, uint32_t dist_on, float d2)
{
    return counted && !(f.x == 0.f && f.y == 0.f && f.z == 0.f) && isfinite (geo) && (!dist_on || geo <= d2);
}
