// icp_normal_rule.h — the normal of a point of a row-major grid from its four one-pixel neighbours, stated once: ICP_NORMALS_GRID
// (k_normals_grid, icp_p2pl.hip: the landmark grid) and the RGB-D front end (icp_rgbd.hip: the full-resolution vertex map) evaluate it.
// fp32, no contraction (every translation unit is built with -ffp-contract=off); tests/p2pl_ref.py::grid_normals restates it.
//   c = dh x dv,  n = c / sqrtf ((c.x^2 + c.y^2) + c.z^2),  n = -n if (n.x C.x + n.y C.y) + n.z C.z > 0 (faces the sensor at the origin),
//   n = 0 when the centre is invalid, a difference is missing, or the length is not > 0 and finite.
#pragma once
#include "icp_pair_rule.h"

// (a grid point takes part in a difference or a gradient when it is valid — icp_point_valid: a Kinect pixel without depth is not)
static __device__ __forceinline__ float3 nrm_sub (float3 a, float3 b) { return make_float3 (a.x - b.x, a.y - b.y, a.z - b.z); }

// the difference along one grid axis: central if both neighbours are valid, else one-sided against the centre (the next neighbour first)
static __device__ __forceinline__ bool nrm_diff (float3 prev, bool has_prev, float3 c, float3 next, bool has_next, float3 &d)
{
    const bool vp = has_prev && icp_point_valid (prev.x, prev.y, prev.z), vn = has_next && icp_point_valid (next.x, next.y, next.z);
    if (vp && vn) d = nrm_sub (next, prev);
    else if (vn) d = nrm_sub (next, c);
    else if (vp) d = nrm_sub (c, prev);
    return vp || vn;
}

// c: the centre; l, r, u, d: its left, right, upper and lower neighbour where the grid has one (has*), anything else
static __device__ __forceinline__ float4 icp_grid_normal (float3 c, float3 l, bool hasl, float3 r, bool hasr, float3 u, bool hasu, float3 d, bool hasd)
{
    float4 n = make_float4 (0.f, 0.f, 0.f, 0.f);
    float3 dh = make_float3 (0.f, 0.f, 0.f), dv = dh;
    if (icp_point_valid (c.x, c.y, c.z) && nrm_diff (l, hasl, c, r, hasr, dh) && nrm_diff (u, hasu, c, d, hasd, dv)) {
        const float cx = dh.y * dv.z - dh.z * dv.y, cy = dh.z * dv.x - dh.x * dv.z, cz = dh.x * dv.y - dh.y * dv.x;
        const float len = sqrtf ((cx * cx + cy * cy) + cz * cz);
        if (len > 0.f && len < __builtin_inff ()) {
            float nx = cx / len, ny = cy / len, nz = cz / len;
            if ((nx * c.x + ny * c.y) + nz * c.z > 0.f) { nx = -nx; ny = -ny; nz = -nz; }
            n = make_float4 (nx, ny, nz, 0.f);
        }
    }
    return n;
}
