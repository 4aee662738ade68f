// icp_plane_moments.h — what the plane system's moments kernel (icp_plane_moments.inc) needs beyond icp_kernels.h: the intensity of a
// landmark, which k_color_grad_grid (icp_p2pl.hip) uses too.
#pragma once
#include "icp_kernels.h"

namespace {

// the intensity of a landmark [x y z 1 r g b 1], fp32
__device__ __forceinline__ float intensity (float r, float g, float b) { return ((r + g) + b) / 3.f; }

}  // namespace
