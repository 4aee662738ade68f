// icp_tsdf.hip — frame-to-model: a truncated signed distance volume fused and ray-cast on the device (the rule: include/icp_amd.h,
// "Frame-to-model"; tests/tsdf_ref.py restates it).  The volume's surface as a point cloud: icp_tsdf_surface.hip.  The moving window: icp_tsdf_shift.hip.  The reference has no model: each of its frames is registered against the previous one.
//
//   k_tsdf_integrate  one lane per voxel, lanes along i: a block of 256 owns 64 i x 4 j of one k, so every access to the volume is a
//                     wave-wide coalesced 8-byte {D, W} (16-byte colour) vector access.  A voxel the frame does not change is not stored.
//                     A touched voxel moves 16 bytes (48 with colour) and the depth image stays in L2, but a frame touches a few percent
//                     of a room-sized volume: measured, the launch is bound by the projection of the voxels that leave untouched
//                     (DESIGN.md section 5).  One writer per voxel, no atomics, no LDS.
//   k_tsdf_raycast    one lane per ray, an 8 x 8 tile of pixels (or of landmarks: the lattice form launches side x side lanes, not
//                     width x height) per wave, so that neighbouring rays gather neighbouring cells.  The march reads {D, W} only — eight
//                     8-byte loads a sample, those of four samples in flight together —; the colour and the six gradient samples are
//                     fetched once, at the hit.  At most N + 1 <= 4096 samples; no LDS, no cross-block word, no spin.
//
// -ffp-contract=off keeps every operation on its own; `/` and sqrtf are the correctly rounded ones.  Both kernels run on the stream the
// volume owns, and every public call is blocking.
#include "icp_tsdf.h"
#include "icp_cguard.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr uint32_t INT_I = 64u, INT_J = 4u;                // a block of k_tsdf_integrate: 64 i x 4 j
constexpr uint32_t TILE = 8u, TILES_X = 4u;                // a wave of k_tsdf_raycast: 8 x 8 rays; a block: four such tiles side by side
constexpr uint32_t AHEAD = 4u;                             // steps of the march whose loads are in flight together

struct tsdf_integrate_args { icp_tsdf_dev v; icp_tsdf_view cam; const uint16_t *depth; const uint8_t *rgb; };

__global__ __launch_bounds__ (256) void k_tsdf_integrate (tsdf_integrate_args a)
{
    const icp_tsdf_dev &v = a.v;
    const icp_rgbd_t &c = a.cam.c;
    const float *R = a.cam.R, *t = a.cam.t;
    const uint32_t i = blockIdx.x * INT_I + threadIdx.x % INT_I, j = blockIdx.y * INT_J + threadIdx.x / INT_I, k = blockIdx.z;
    if (i >= v.nx || j >= v.ny) return;
    const float d0 = (v.ox + (float) i * v.voxel) - t[0], d1 = (v.oy + (float) j * v.voxel) - t[1], d2 = (v.oz + (float) k * v.voxel) - t[2];
    const float qx = dot3 (R[0], d0, R[3], d1, R[6], d2), qy = dot3 (R[1], d0, R[4], d1, R[7], d2), qz = dot3 (R[2], d0, R[5], d1, R[8], d2);
    if (!(qz > 0.f)) return;
    const float pu = (c.fx * (qx / qz) + c.cx) + 0.5f, pv = (c.fy * (qy / qz) + c.cy) + 0.5f;
    if (!(pu >= 0.f && pu < (float) c.width && pv >= 0.f && pv < (float) c.height)) return;
    const size_t px = (size_t) (uint32_t) floorf (pv) * c.width + (uint32_t) floorf (pu);
    const uint32_t raw = a.depth[px];
    if (!(raw != 0u && raw >= c.d_min && raw <= c.d_max)) return;
    const float s = (float) raw * c.depth_scale - qz;
    if (!(s >= -v.mu)) return;
    const float e = fminf (1.f, s / v.mu);
    const size_t at = ((size_t) k * v.ny + j) * v.nx + i;
    const float2 dw = v.dw[at];
    const float w1 = dw.y + 1.f;
    if (v.col && a.rgb) {
        const uint8_t *p = a.rgb + px * 3;
        float4 col = v.col[at];
        col.x = (col.x * dw.y + (float) p[0] / 255.f) / w1;
        col.y = (col.y * dw.y + (float) p[1] / 255.f) / w1;
        col.z = (col.z * dw.y + (float) p[2] / 255.f) / w1;
        v.col[at] = col;
    }
    v.dw[at] = make_float2 ((dw.x * dw.y + e) / w1, fminf (w1, v.w_max));
}

__device__ __forceinline__ bool tsdf_sample (const icp_tsdf_dev &v, float wx, float wy, float wz, float &S, size_t *cell = nullptr, float3 *frac = nullptr)
{
    tsdf_corners q;
    tsdf_fetch (v, wx, wy, wz, q);
    if (!tsdf_value (q, S)) return false;
    if (cell) { *cell = q.at; *frac = q.f; }
    return true;
}

__global__ __launch_bounds__ (256) void k_tsdf_raycast (icp_tsdf_cast_args a)
{
    const icp_tsdf_dev &v = a.v;
    const icp_rgbd_t &c = a.cam.c;
    const uint32_t gw = a.side ? a.side : c.width, gh = a.side ? a.side : c.height;
    const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
    const uint32_t gi = (blockIdx.x * TILES_X + wave) * TILE + lane % TILE, gj = blockIdx.y * TILE + lane / TILE;
    if (gi >= gw || gj >= gh) return;
    const uint32_t pu = a.side ? c.x0 + c.step_x * gi : gi, pv = a.side ? c.y0 + c.step_y * gj : gj;
    const float ax = ((float) pu - c.cx) / c.fx, ay = ((float) pv - c.cy) / c.fy;
    // the march: n* = the first n whose sample is known and <= 0
    bool cross = false, prev_known = false;
    float s0 = 0.f, s1 = 0.f, lam0 = 0.f, prev_s = 0.f;
    // (the samples of AHEAD steps are fetched before the first of them is looked at: a ray's steps depend on one another only through
    // the decision to stop, and a step costs a round trip to memory)
    for (uint32_t n0 = 0u; n0 <= a.N; n0 += AHEAD) {
        tsdf_corners q[AHEAD];
#pragma unroll
        for (uint32_t j = 0u; j < AHEAD; ++j) {
            const float lam = a.z_near + (float) (n0 + j) * a.delta;
            const float3 w = tsdf_world (a.cam, ax * lam, ay * lam, lam);
            tsdf_fetch (v, w.x, w.y, w.z, q[j]);
        }
        bool stop = false;
#pragma unroll
        for (uint32_t j = 0u; j < AHEAD; ++j) {
            const uint32_t n = n0 + j;
            float s = 0.f;
            const bool known = tsdf_value (q[j], s);
            if (!stop && n <= a.N) {
                if (known && s <= 0.f) {
                    cross = n >= 1u && prev_known && prev_s > 0.f;
                    s0 = prev_s; s1 = s; lam0 = a.z_near + (float) (n - 1u) * a.delta;
                    stop = true;
                } else { prev_known = known; prev_s = s; }
            }
        }
        if (stop) break;
    }
    float4 pt = make_float4 (0.f, 0.f, 0.f, 1.f), colour = make_float4 (0.f, 0.f, 0.f, 1.f), nrm = make_float4 (0.f, 0.f, 0.f, 0.f);
    if (cross) {
        const float lam = lam0 + a.delta * (s0 / (s0 - s1));
        const float X = ((float) pu - c.cx) * lam / c.fx, Y = ((float) pv - c.cy) * lam / c.fy, Z = lam;
        const float3 h = tsdf_world (a.cam, X, Y, Z);
        size_t at = 0; float3 f; float sh;
        if (tsdf_sample (v, h.x, h.y, h.z, sh, &at, &f)) {
            pt = make_float4 (X, Y, Z, 1.f);
            if (v.col) {
                const size_t sy = v.nx, sz = (size_t) v.nx * v.ny;
                const float4 c000 = v.col[at], c001 = v.col[at + 1], c010 = v.col[at + sy], c011 = v.col[at + sy + 1];
                const float4 c100 = v.col[at + sz], c101 = v.col[at + sz + 1], c110 = v.col[at + sz + sy], c111 = v.col[at + sz + sy + 1];
                colour.x = tsdf_trilinear (c000.x, c001.x, c010.x, c011.x, c100.x, c101.x, c110.x, c111.x, f);
                colour.y = tsdf_trilinear (c000.y, c001.y, c010.y, c011.y, c100.y, c101.y, c110.y, c111.y, f);
                colour.z = tsdf_trilinear (c000.z, c001.z, c010.z, c011.z, c100.z, c101.z, c110.z, c111.z, f);
            }
            if (a.nrm) {
                float xp, xm, yp, ym, zp, zm;
                if (tsdf_sample (v, h.x + v.voxel, h.y, h.z, xp) && tsdf_sample (v, h.x - v.voxel, h.y, h.z, xm) &&
                    tsdf_sample (v, h.x, h.y + v.voxel, h.z, yp) && tsdf_sample (v, h.x, h.y - v.voxel, h.z, ym) &&
                    tsdf_sample (v, h.x, h.y, h.z + v.voxel, zp) && tsdf_sample (v, h.x, h.y, h.z - v.voxel, zm)) {
                    const float G0 = xp - xm, G1 = yp - ym, G2 = zp - zm, len = sqrtf (dot3 (G0, G0, G1, G1, G2, G2));
                    if (len > 0.f) {
                        const float n0 = G0 / len, n1 = G1 / len, n2 = G2 / len;
                        const float *R = a.cam.R;
                        const float c0 = dot3 (R[0], n0, R[3], n1, R[6], n2), c1 = dot3 (R[1], n0, R[4], n1, R[7], n2), c2 = dot3 (R[2], n0, R[5], n1, R[8], n2);
                        const bool flip = dot3 (c0, X, c1, Y, c2, Z) > 0.f;
                        nrm = flip ? make_float4 (-c0, -c1, -c2, 0.f) : make_float4 (c0, c1, c2, 0.f);
                    }
                }
            }
        }
    }
    const size_t g = (size_t) gj * gw + gi;
    a.out[2 * g] = pt;
    a.out[2 * g + 1] = colour;
    if (a.nrm) a.nrm[g] = nrm;
}

thread_local std::string g_tsdf_create_error;

bool finite_all (const float *p, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite (p[i])) return false; return true; }

const char *tsdf_refusal (const icp_tsdf_t &c)
{
    for (uint32_t n : { c.nx, c.ny, c.nz }) if (n < 2u || n > 1024u) return "nx, ny and nz must be in [2, 1024]";
    if (!(std::isfinite (c.voxel) && c.voxel > 0.f)) return "voxel must be finite and > 0";
    if (!finite_all (c.origin, 3)) return "origin must be finite";
    if (!(std::isfinite (c.mu) && c.mu > 0.f)) return "mu must be finite and > 0";
    if (!(c.w_max >= 1.f && c.w_max <= 65536.f && c.w_max == std::floor (c.w_max))) return "w_max must be an integer in [1, 65536]";
    if (c.colour > 1u) return "colour must be 0 or 1";
    return nullptr;
}

icp_tsdf_view view_of (const icp_rgbd_t &cam, const float *pose12)
{
    icp_tsdf_view w {};
    w.c = cam;
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) w.R[3 * r + k] = pose12[4 * r + k]; w.t[r] = pose12[4 * r + 3]; }
    return w;
}

size_t voxels (const icp_tsdf_t &c) { return (size_t) c.nx * c.ny * c.nz; }

}  // namespace

namespace icp_host {

int tsdf_fail (icp_tsdf_context *t, int code, const std::string &msg)
{
    if (t) t->err = msg; else g_tsdf_create_error = msg;
    return code;
}

int tsdf_cast_prepare (icp_tsdf_context *t, const char *who, const icp_rgbd_t *cam, const float *pose12, float z_near, float z_far, uint32_t side, icp_tsdf_cast_args *a)
{
    const std::string w = std::string (who) + ": ";
    if (!cam || !pose12) return tsdf_fail (t, ICP_EINVAL, w + "null pointer");
    if (const char *why = icp_rgbd_refusal (*cam)) return tsdf_fail (t, ICP_EINVAL, w + why);
    if (!finite_all (pose12, 12)) return tsdf_fail (t, ICP_EINVAL, w + "the pose must be finite");
    if (!(std::isfinite (z_near) && std::isfinite (z_far) && z_near > 0.f && z_near < z_far)) return tsdf_fail (t, ICP_EINVAL, w + "0 < z_near < z_far, both finite, is required");
    const float delta = 0.5f * t->cfg.mu, N = std::floor ((z_far - z_near) / delta);
    if (!(N <= 4095.f)) return tsdf_fail (t, ICP_EINVAL, w + "the march has more than 4096 samples: (z_far - z_near) / (0.5 mu) must stay below 4096");
    if (side && !icp_rgbd_lattice_fits (*cam, side)) return tsdf_fail (t, ICP_EINVAL, w + "the lattice of side x side landmarks leaves the image");
    *a = icp_tsdf_cast_args {};
    a->v = t->v; a->cam = view_of (*cam, pose12);
    a->z_near = z_near; a->delta = delta; a->N = (uint32_t) N; a->side = side;
    return ICP_OK;
}

int tsdf_reserve (icp_tsdf_context *t, void **q, size_t *cap, size_t bytes)
{
    if (*cap >= bytes) return ICP_OK;
    if (*q) (void) hipFree (*q);                    // (every public call is blocking: nothing in flight reads it)
    *q = nullptr; *cap = 0;
    if (hipMalloc (q, bytes) != hipSuccess) { (void) hipGetLastError (); *q = nullptr; return tsdf_fail (t, ICP_ENOMEM, "hipMalloc: out of device memory"); }
    *cap = bytes;
    return ICP_OK;
}

void tsdf_launch_raycast (const icp_tsdf_cast_args &a, hipStream_t s)
{
    const uint32_t gw = a.side ? a.side : a.cam.c.width, gh = a.side ? a.side : a.cam.c.height, bw = TILE * TILES_X;
    hipLaunchKernelGGL (k_tsdf_raycast, dim3 ((gw + bw - 1u) / bw, (gh + TILE - 1u) / TILE), dim3 (256), 0, s, a);
}

}  // namespace icp_host

using namespace icp_host;

namespace {

void launch_integrate (const tsdf_integrate_args &a, hipStream_t s)
{
    hipLaunchKernelGGL (k_tsdf_integrate, dim3 ((a.v.nx + INT_I - 1u) / INT_I, (a.v.ny + INT_J - 1u) / INT_J, a.v.nz), dim3 (256), 0, s, a);
}

int zero_volume (icp_tsdf_context *t)
{
    const size_t n = voxels (t->cfg);
    TSDFCHK (t, hipMemsetAsync (t->v.dw, 0, n * sizeof (float2), t->stream));
    if (t->v.col) TSDFCHK (t, hipMemsetAsync (t->v.col, 0, n * sizeof (float4), t->stream));
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    return ICP_OK;
}

// the checks of an integration that need no device, and the images on the device
int integrate_prepare (icp_tsdf_context *t, const char *who, const icp_rgbd_t *cam, const float *pose12, const uint16_t *depth, const uint8_t *rgb, tsdf_integrate_args *a)
{
    const std::string w = std::string (who) + ": ";
    if (!cam || !pose12 || !depth) return tsdf_fail (t, ICP_EINVAL, w + "null pointer");
    if (const char *why = icp_rgbd_refusal (*cam)) return tsdf_fail (t, ICP_EINVAL, w + why);
    if (!finite_all (pose12, 12)) return tsdf_fail (t, ICP_EINVAL, w + "the pose must be finite");
    TSDFCHK (t, hipSetDevice (t->device));
    const size_t n = (size_t) cam->width * cam->height;
    int rc;
    if ((rc = tsdf_reserve (t, &t->dDepth, &t->depth_cap, n * 2u))) return rc;
    if (rgb && (rc = tsdf_reserve (t, &t->dRgb, &t->rgb_cap, n * 3u))) return rc;
    TSDFCHK (t, hipMemcpyAsync (t->dDepth, depth, n * 2u, hipMemcpyHostToDevice, t->stream));
    if (rgb) TSDFCHK (t, hipMemcpyAsync (t->dRgb, rgb, n * 3u, hipMemcpyHostToDevice, t->stream));
    a->v = t->v; a->cam = view_of (*cam, pose12);
    a->depth = static_cast<const uint16_t *> (t->dDepth); a->rgb = rgb ? static_cast<const uint8_t *> (t->dRgb) : nullptr;
    return ICP_OK;
}

}  // namespace

extern "C" {

const char *icp_tsdf_last_error (icp_tsdf_handle t) { return t ? t->err.c_str () : g_tsdf_create_error.c_str (); }

int icp_tsdf_destroy (icp_tsdf_handle t) try
{
    if (!t) return ICP_EINVAL;
    (void) hipSetDevice (t->device);
    if (t->stream) (void) hipStreamSynchronize (t->stream);
    for (void *q : { (void *) t->v.dw, (void *) t->v.col, (void *) t->dw2, (void *) t->col2, t->dDepth, t->dRgb, t->dOut, t->dNrm, t->dSurf, t->dEdge, t->dMesh, t->dTri, t->dMeshTab, t->dRegCloud, t->dRegWork }) if (q) (void) hipFree (q);
    if (t->ev0) (void) hipEventDestroy (t->ev0);
    if (t->ev1) (void) hipEventDestroy (t->ev1);
    if (t->stream) (void) hipStreamDestroy (t->stream);
    delete t;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_create (icp_tsdf_handle *out, int device, const icp_tsdf_t *cfg) try
{
    if (!out) return ICP_EINVAL;
    *out = nullptr;
    if (!cfg) return tsdf_fail (nullptr, ICP_EINVAL, "icp_tsdf_create: null configuration");
    if (const char *why = tsdf_refusal (*cfg)) return tsdf_fail (nullptr, ICP_EINVAL, std::string ("icp_tsdf_create: ") + why);
    int count = 0;
    if (hipGetDeviceCount (&count) != hipSuccess || count <= 0) { (void) hipGetLastError (); return tsdf_fail (nullptr, ICP_ENODEVICE, "icp_tsdf_create: no HIP device visible (the engine has no CPU fallback)"); }
    if (device < 0 || device >= count) return tsdf_fail (nullptr, ICP_EINVAL, "icp_tsdf_create: device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties (&prop, device) != hipSuccess) return tsdf_fail (nullptr, ICP_EHIP, "icp_tsdf_create: hipGetDeviceProperties");
    if (std::strncmp (prop.gcnArchName, "gfx950", 6) != 0)
        return tsdf_fail (nullptr, ICP_ENODEVICE, std::string ("icp_tsdf_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    icp_tsdf_context *t = new icp_tsdf_context ();
    t->device = device; t->cfg = *cfg;
    for (int a = 0; a < 3; ++a) t->base[a] = cfg->origin[a];
    auto give_up = [&] (int code, const std::string &msg) { (void) hipGetLastError (); icp_tsdf_destroy (t); return tsdf_fail (nullptr, code, msg); };
    if (hipSetDevice (device) != hipSuccess || hipStreamCreateWithFlags (&t->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate (&t->ev0) != hipSuccess || hipEventCreate (&t->ev1) != hipSuccess) return give_up (ICP_EHIP, "icp_tsdf_create: stream and events");
    const size_t n = voxels (*cfg);
    if (hipMalloc ((void **) &t->v.dw, n * sizeof (float2)) != hipSuccess) { t->v.dw = nullptr; return give_up (ICP_ENOMEM, "icp_tsdf_create: the device cannot hold the volume"); }
    if (cfg->colour && hipMalloc ((void **) &t->v.col, n * sizeof (float4)) != hipSuccess) { t->v.col = nullptr; return give_up (ICP_ENOMEM, "icp_tsdf_create: the device cannot hold the volume's colour"); }
    t->v.nx = cfg->nx; t->v.ny = cfg->ny; t->v.nz = cfg->nz;
    t->v.voxel = cfg->voxel; t->v.ox = cfg->origin[0]; t->v.oy = cfg->origin[1]; t->v.oz = cfg->origin[2]; t->v.mu = cfg->mu; t->v.w_max = cfg->w_max;
    if (zero_volume (t) != ICP_OK) return give_up (ICP_EHIP, "icp_tsdf_create: " + t->err);
    *out = t;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_reset (icp_tsdf_handle t) try
{
    if (!t) return ICP_EINVAL;
    TSDFCHK (t, hipSetDevice (t->device));
    return zero_volume (t);                         // (the live buffers; the window of icp_tsdf_shift stays where it is)
}
ICP_CATCH_ALL

int icp_tsdf_get_config (icp_tsdf_handle t, icp_tsdf_t *cfg) try
{
    if (!t || !cfg) return ICP_EINVAL;
    *cfg = t->cfg;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_integrate (icp_tsdf_handle t, const icp_rgbd_t *cam, const float *pose12, const uint16_t *depth, const uint8_t *rgb) try
{
    if (!t) return ICP_EINVAL;
    tsdf_integrate_args a {};
    int rc = integrate_prepare (t, "icp_tsdf_integrate", cam, pose12, depth, rgb, &a); if (rc) return rc;
    launch_integrate (a, t->stream);
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_raycast (icp_tsdf_handle t, const icp_rgbd_t *cam, const float *pose12, float z_near, float z_far, uint32_t side, void *cloud_out, float *normals_out) try
{
    if (!t) return ICP_EINVAL;
    if (!cloud_out) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_raycast: null pointer");
    icp_tsdf_cast_args a;
    int rc = tsdf_cast_prepare (t, "icp_tsdf_raycast", cam, pose12, z_near, z_far, side, &a); if (rc) return rc;
    TSDFCHK (t, hipSetDevice (t->device));
    const size_t n = side ? (size_t) side * side : (size_t) cam->width * cam->height;
    if ((rc = tsdf_reserve (t, &t->dOut, &t->out_cap, n * 32u))) return rc;
    if (normals_out && (rc = tsdf_reserve (t, &t->dNrm, &t->nrm_cap, n * 16u))) return rc;
    a.out = static_cast<float4 *> (t->dOut); a.nrm = normals_out ? static_cast<float4 *> (t->dNrm) : nullptr;
    tsdf_launch_raycast (a, t->stream);
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipMemcpyAsync (cloud_out, t->dOut, n * 32u, hipMemcpyDeviceToHost, t->stream));
    if (normals_out) TSDFCHK (t, hipMemcpyAsync (normals_out, t->dNrm, n * 16u, hipMemcpyDeviceToHost, t->stream));
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_read (icp_tsdf_handle t, float *dw, float *rgb) try
{
    if (!t) return ICP_EINVAL;
    if (!dw || (rgb != nullptr) != (t->cfg.colour != 0u)) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_read: dw is required, rgb for (and only for) a volume with colour");
    TSDFCHK (t, hipSetDevice (t->device));
    const size_t n = voxels (t->cfg);
    std::vector<float4> col (rgb ? n : 0);
    TSDFCHK (t, hipMemcpyAsync (dw, t->v.dw, n * sizeof (float2), hipMemcpyDeviceToHost, t->stream));
    if (rgb) TSDFCHK (t, hipMemcpyAsync (col.data (), t->v.col, n * sizeof (float4), hipMemcpyDeviceToHost, t->stream));
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    for (size_t i = 0; i < col.size (); ++i) { rgb[3 * i] = col[i].x; rgb[3 * i + 1] = col[i].y; rgb[3 * i + 2] = col[i].z; }
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_write (icp_tsdf_handle t, const float *dw, const float *rgb) try
{
    if (!t) return ICP_EINVAL;
    if (!dw || (rgb != nullptr) != (t->cfg.colour != 0u)) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_write: dw is required, rgb for (and only for) a volume with colour");
    TSDFCHK (t, hipSetDevice (t->device));
    const size_t n = voxels (t->cfg);
    std::vector<float4> col (rgb ? n : 0);
    for (size_t i = 0; i < col.size (); ++i) col[i] = make_float4 (rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.f);
    TSDFCHK (t, hipMemcpyAsync (t->v.dw, dw, n * sizeof (float2), hipMemcpyHostToDevice, t->stream));
    if (rgb) TSDFCHK (t, hipMemcpyAsync (t->v.col, col.data (), n * sizeof (float4), hipMemcpyHostToDevice, t->stream));
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_compose_pose (const float *pose12, const float *T8, float *out12, float *scale) try
{
    if (!pose12 || !T8 || !out12) return ICP_EINVAL;
    const double x0 = T8[0], y0 = T8[1], z0 = T8[2], w0 = T8[3], len = std::sqrt (x0 * x0 + y0 * y0 + z0 * z0 + w0 * w0);
    if (!(len > 0.0) || !std::isfinite (len)) return ICP_EINVAL;
    const double x = x0 / len, y = y0 / len, z = z0 / len, w = w0 / len;
    const double Rq[3][3] = { { 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w) },
                              { 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w) },
                              { 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y) } };
    float res[12];
    for (int r = 0; r < 3; ++r) {
        const double P0 = pose12[4 * r], P1 = pose12[4 * r + 1], P2 = pose12[4 * r + 2];
        for (int k = 0; k < 3; ++k) res[4 * r + k] = (float) (P0 * Rq[0][k] + P1 * Rq[1][k] + P2 * Rq[2][k]);
        res[4 * r + 3] = (float) (P0 * (double) T8[4] + P1 * (double) T8[5] + P2 * (double) T8[6] + (double) pose12[4 * r + 3]);
    }
    std::memcpy (out12, res, sizeof res);           // (out12 may be pose12)
    if (scale) *scale = T8[7];
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_time (icp_tsdf_handle t, int what, const icp_rgbd_t *cam, const float *pose12, const uint16_t *depth, const uint8_t *rgb, float z_near, float z_far,
                           uint32_t side, uint32_t reps, float *us_per_launch) try
{
    if (!t) return ICP_EINVAL;
    if (!us_per_launch || reps == 0u || what < 0 || what > 11) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_time: bad arguments");
    if (what == 11) return tsdf_time_region (t, reinterpret_cast<const int32_t *> (depth), reps, us_per_launch);
    if (what == 10) return tsdf_time_shift (t, reinterpret_cast<const int32_t *> (depth), reps, us_per_launch);
    if (what >= 8) return tsdf_time_register (t, what - 8, depth, side, pose12, reps, us_per_launch);
    if (what >= 5) return tsdf_time_mesh (t, what - 5, reps, us_per_launch);
    if (what >= 2) return tsdf_time_surface (t, what - 2, reps, us_per_launch);
    tsdf_integrate_args ia {};
    icp_tsdf_cast_args ca {};
    int rc;
    if (what == 0) { if ((rc = integrate_prepare (t, "icp_tsdf_time", cam, pose12, depth, rgb, &ia))) return rc; }
    else {
        if ((rc = tsdf_cast_prepare (t, "icp_tsdf_time", cam, pose12, z_near, z_far, side, &ca))) return rc;
        TSDFCHK (t, hipSetDevice (t->device));
        const size_t n = side ? (size_t) side * side : (size_t) cam->width * cam->height;
        if ((rc = tsdf_reserve (t, &t->dOut, &t->out_cap, n * 32u)) || (rc = tsdf_reserve (t, &t->dNrm, &t->nrm_cap, n * 16u))) return rc;
        ca.out = static_cast<float4 *> (t->dOut); ca.nrm = static_cast<float4 *> (t->dNrm);
    }
    auto launch = [&] () { if (what == 0) launch_integrate (ia, t->stream); else tsdf_launch_raycast (ca, t->stream); };
    launch ();                                      // (untimed: the code object is loaded)
    TSDFCHK (t, hipEventRecord (t->ev0, t->stream));
    for (uint32_t i = 0; i < reps; ++i) launch ();
    TSDFCHK (t, hipEventRecord (t->ev1, t->stream));
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipEventSynchronize (t->ev1));
    float ms = 0.f;
    TSDFCHK (t, hipEventElapsedTime (&ms, t->ev0, t->ev1));
    *us_per_launch = ms * 1e3f / (float) reps;
    return ICP_OK;
}
ICP_CATCH_ALL

}  // extern "C"
