// icp_tsdf.h — what icp_tsdf.hip (the volume, its two kernels and its C entries) shares with icp_capi.hip, which owns the one entry
// that needs the inside of an icp_context (icp_tsdf_raycast_to), and with icp_tsdf_surface.hip (icp_tsdf_extract_surface,
// icp_tsdf_extract_mesh): the volume's handle, the arguments of a ray cast and its launcher, the scratch of a call.
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

struct icp_tsdf_context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    icp_tsdf_t cfg {};
    icp_tsdf_dev v {};
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
}

#define TSDFCHK(t, expr)                                                                                       \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return icp_host::tsdf_fail ((t), ICP_EHIP, std::string (#expr) + ": " + hipGetErrorString (e_));   \
    } while (0)
