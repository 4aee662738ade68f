// icp_tsdf.h — what icp_tsdf.hip (the volume, its two kernels and its C entries) shares with icp_capi.hip, which owns the one entry
// that needs the inside of an icp_context (icp_tsdf_raycast_to), and with icp_tsdf_surface.hip (icp_tsdf_extract_surface,
// icp_tsdf_extract_mesh) and icp_tsdf_register.hip (icp_tsdf_register; icp_capi.hip owns icp_tsdf_register_from): the volume's handle, the
// arguments of a ray cast and its launcher, the sample of the volume on the device, the scratch of a call.
#pragma once
#include "../../include/icp_amd.h"
#include "icp_rgbd.h"

#include <string>

// The device's view of a volume.  Voxel (i, j, k) lives at dw[(k ny + j) nx + i] = {D, W} and, with colour, col[(k ny + j) nx + i] =
// {C_0, C_1, C_2, -}: a wave's 64 consecutive i are one coalesced 8- or 16-byte access, and the march of the ray cast never touches col.
struct icp_tsdf_dev {
    uint32_t nx, ny, nz;
    float voxel, ox, oy, oz, mu, w_max;
    float2 *dw; float4 *col;                     // col: null without colour
};

// a camera at a pose: R row-major, camera -> world
struct icp_tsdf_view { icp_rgbd_t c; float R[9], t[3]; };

struct icp_tsdf_cast_args {
    icp_tsdf_dev v; icp_tsdf_view cam;
    float z_near, delta; uint32_t N;             // the march: lambda_n = z_near + n delta, n = 0 .. N
    uint32_t side;                               // 0: every pixel of the image, else the side x side landmarks of the lattice
    float4 *out, *nrm;                           // [pixels or landmarks][2] float4, [pixels or landmarks] float4 (may be null)
};

// ---- the sample of the volume on the device: what k_tsdf_raycast (icp_tsdf.hip) and k_tsdf_reg_moments (icp_tsdf_register.hip) share ----

__device__ __forceinline__ float dot3 (float a0, float b0, float a1, float b1, float a2, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// The cell of the world point w: false unless 0 <= floor (g_a) <= n_a - 2 on every axis (NaN fails; no conversion before the check).
// at: the cell's corner (i, j, k); f: the fractions.
__device__ __forceinline__ bool tsdf_cell (const icp_tsdf_dev &v, float wx, float wy, float wz, size_t &at, float3 &f)
{
    const float gx = (wx - v.ox) / v.voxel, gy = (wy - v.oy) / v.voxel, gz = (wz - v.oz) / v.voxel;
    const float ix = floorf (gx), iy = floorf (gy), iz = floorf (gz);
    if (!(ix >= 0.f && ix <= (float) (v.nx - 2u) && iy >= 0.f && iy <= (float) (v.ny - 2u) && iz >= 0.f && iz <= (float) (v.nz - 2u))) return false;
    at = ((size_t) (uint32_t) iz * v.ny + (uint32_t) iy) * v.nx + (uint32_t) ix;
    f = make_float3 (gx - ix, gy - iy, gz - iz);
    return true;
}

__device__ __forceinline__ float lerp1 (float a, float b, float t) { return a + t * (b - a); }

// along x, then y, then z; c[dz][dy][dx]
__device__ __forceinline__ float tsdf_trilinear (float c000, float c001, float c010, float c011, float c100, float c101, float c110, float c111, const float3 &f)
{
    const float y00 = lerp1 (c000, c001, f.x), y01 = lerp1 (c010, c011, f.x), y10 = lerp1 (c100, c101, f.x), y11 = lerp1 (c110, c111, f.x);
    return lerp1 (lerp1 (y00, y01, f.y), lerp1 (y10, y11, f.y), f.z);
}

// The eight {D, W} of the cell of a world point — of cell (0, 0, 0) where the point has none, so that a fetch is unconditional and the
// loads of several samples can be in flight together — and what decides the sample from them.
struct tsdf_corners { float2 c[8]; float3 f; size_t at; bool cell; };

__device__ __forceinline__ void tsdf_fetch (const icp_tsdf_dev &v, float wx, float wy, float wz, tsdf_corners &q)
{
    q.at = 0;
    q.cell = tsdf_cell (v, wx, wy, wz, q.at, q.f);
    const size_t sy = v.nx, sz = (size_t) v.nx * v.ny;
    const float2 *p = v.dw + q.at;
    q.c[0] = p[0]; q.c[1] = p[1]; q.c[2] = p[sy]; q.c[3] = p[sy + 1]; q.c[4] = p[sz]; q.c[5] = p[sz + 1]; q.c[6] = p[sz + sy]; q.c[7] = p[sz + sy + 1];
}

// S (w): known, and its value
__device__ __forceinline__ bool tsdf_value (const tsdf_corners &q, float &S)
{
    const float2 *c = q.c;
    if (!(q.cell && c[0].y > 0.f && c[1].y > 0.f && c[2].y > 0.f && c[3].y > 0.f && c[4].y > 0.f && c[5].y > 0.f && c[6].y > 0.f && c[7].y > 0.f)) return false;
    S = tsdf_trilinear (c[0].x, c[1].x, c[2].x, c[3].x, c[4].x, c[5].x, c[6].x, c[7].x, q.f);
    return true;
}

__device__ __forceinline__ float3 tsdf_world (const icp_tsdf_view &cam, float x, float y, float z)
{
    const float *R = cam.R, *t = cam.t;
    return make_float3 (dot3 (R[0], x, R[1], y, R[2], z) + t[0], dot3 (R[3], x, R[4], y, R[5], z) + t[1], dot3 (R[6], x, R[7], y, R[8], z) + t[2]);
}

struct icp_tsdf_context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    icp_tsdf_t cfg {};                           // (origin: the window's current one)
    icp_tsdf_dev v {};
    // the moving window (icp_tsdf_shift.hip): the origin given at create, the cumulative shift in voxels, and the second buffer of the
    // volume's size a shift writes into before v.dw / v.col swap with it (allocated by the first shift, kept until destroy)
    float base[3] = { 0.f, 0.f, 0.f };
    int32_t win[3] = { 0, 0, 0 };
    float2 *dw2 = nullptr; float4 *col2 = nullptr;
    // device copies of the images of an integration and the results of a ray cast to the host (grown when a call needs more)
    void *dDepth = nullptr, *dRgb = nullptr, *dOut = nullptr, *dNrm = nullptr;
    size_t depth_cap = 0, rgb_cap = 0, out_cap = 0, nrm_cap = 0;
    // the words of a surface extraction (icp_tsdf_surface.hip: block counts, their offsets, tile sums, tile offsets, the count)
    // and the edges of its members in order
    void *dSurf = nullptr, *dEdge = nullptr;
    size_t surf_cap = 0, edge_cap = 0;
    // the words of a mesh extraction's cell sweep (case bytes, wave counts, block counts and their scan), its triangles, and the case
    // table (256 words, uploaded by the first mesh extraction)
    void *dMesh = nullptr, *dTri = nullptr, *dMeshTab = nullptr;
    size_t mesh_cap = 0, tri_cap = 0;
    // a registration against the volume (icp_tsdf_register.hip): the uploaded cloud of icp_tsdf_register, and the state and block partials
    void *dRegCloud = nullptr, *dRegWork = nullptr;
    size_t reg_cloud_cap = 0, reg_work_cap = 0;
    std::string err;
};

namespace icp_host __attribute__ ((visibility ("hidden"))) {
int tsdf_fail (icp_tsdf_context *t, int code, const std::string &msg);
// The checks of a ray cast that need no device — camera, pose, z range, lattice (side != 0) — and its arguments but for out / nrm.
// ICP_OK, or the status with the volume's error text set.
int tsdf_cast_prepare (icp_tsdf_context *t, const char *who, const icp_rgbd_t *cam, const float *pose12, float z_near, float z_far, uint32_t side, icp_tsdf_cast_args *a);
void tsdf_launch_raycast (const icp_tsdf_cast_args &a, hipStream_t s);
// *q holds at least `bytes` on the device (grown on demand; ICP_ENOMEM with the volume's error text set)
int tsdf_reserve (icp_tsdf_context *t, void **q, size_t *cap, size_t bytes);
// icp_tsdf_time, what = 2 .. 4: `reps` extractions' launches (normals on, min_weight 1) between the volume's two events, after an untimed
// extraction — part 0: all of them, 1: the two scan launches alone, 2: the scatter and the points alone
int tsdf_time_surface (icp_tsdf_context *t, int part, uint32_t reps, float *us_per_group);
// icp_tsdf_time, what = 5 .. 7: the same for a mesh extraction — part 0: all of its launches, 1: the cell sweep alone, 2: the triangle pass alone
int tsdf_time_mesh (icp_tsdf_context *t, int part, uint32_t reps, float *us_per_group);
// The checks of a registration that need no device — pointers, n, the pose, the options.  ICP_OK, or ICP_EINVAL with the volume's error text set.
int tsdf_register_check (icp_tsdf_context *t, const char *who, const icp_tsdf_register_t *opt, const void *cloud, uint32_t n, const float *pose12, const icp_tsdf_registration_t *out);
// max_iterations pairs of k_tsdf_reg_moments / k_tsdf_reg_finalize over n float8 records on the device, on the volume's stream, one
// synchronisation, the record read back.  The arguments have passed tsdf_register_check.
int tsdf_register_run (icp_tsdf_context *t, const icp_tsdf_register_t *opt, const void *dcloud, uint32_t n, const float *pose12, icp_tsdf_registration_t *out);
// icp_tsdf_time, what = 8, 9: `reps` iterations' launches over the host cloud of n records (part 0: both launches, 1: k_tsdf_reg_moments alone)
// with the state held at pose12
int tsdf_time_register (icp_tsdf_context *t, int part, const void *cloud, uint32_t n, const float *pose12, uint32_t reps, float *us_per_group);
// icp_tsdf_time, what = 10: `reps` launches of k_tsdf_shift by +s, -s, +s, .. from the live buffers into the second ones, which never swap in:
// the volume stays as it is
int tsdf_time_shift (icp_tsdf_context *t, const int32_t *s, uint32_t reps, float *us_per_launch);
// icp_tsdf_time, what = 11: `reps` groups of the launches of one icp_tsdf_extract_surface_region (normals on, min_weight 1) for the kept box of s, OUTSIDE
int tsdf_time_region (icp_tsdf_context *t, const int32_t *s, uint32_t reps, float *us_per_group);
}

#define TSDFCHK(t, expr)                                                                                       \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return icp_host::tsdf_fail ((t), ICP_EHIP, std::string (#expr) + ": " + hipGetErrorString (e_));   \
    } while (0)
