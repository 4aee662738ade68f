// icp_trim_apply.h — the pass that rewrites the weights behind the search (include/icp_amd.h: trimming, the robust loss) and the key of
// a pair.  The pass itself is icp_trim_apply.inc: icp_trim.hip instantiates it for trimming alone (k_trim_apply<FUSED>), icp_robust.hip
// for a point-to-point robust loss (k_trim_apply_robust<FUSED>).
//
// The key of a pair is the bit pattern of its geo = (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2 in fp32, summed in that order (the
// translation units are built with -ffp-contract=off): a non-negative float orders as its bits do as uint32.  A pair that is no
// candidate — weight 0, geo not finite, no query — gets the key ~0u, above every candidate's.
#pragma once
#include "icp_search.h"

namespace {

constexpr uint32_t TRIM_NONE = 0xFFFFFFFFu;     // the key of a pair that is no candidate

__device__ __forceinline__ uint32_t trim_key (float4 f, float4 q)
{
    if (f.w == 0.f) return TRIM_NONE;
    const float gx = q.x - f.x, gy = q.y - f.y, gz = q.z - f.z;
    const float geo = (gx * gx + gy * gy) + gz * gz;
    return geo < __builtin_inff () ? __float_as_uint (geo) : TRIM_NONE;      // (NaN and +inf: no candidate)
}

}  // namespace
