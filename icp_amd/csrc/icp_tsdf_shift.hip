// icp_tsdf_shift.hip — the moving volume: the window of a TSDF volume shifted by whole voxels on the device (icp_tsdf_shift,
// icp_tsdf_get_window; the rule: include/icp_amd.h, "Moving volume"; tests/tsdf_shift_ref.py restates it), and the two host-only entries
// that go with it: the box a shift keeps (icp_tsdf_kept_box) and the rule that decides when to shift (icp_tsdf_follow).  The part of the
// surface a shift drops is extracted by icp_tsdf_extract_surface_region (icp_tsdf_surface.hip).
//
//   k_tsdf_shift   one lane per voxel of the new window, lanes along i: a block of 256 owns 64 i x 4 j of one k, as k_tsdf_integrate's
//                  does, so a wave's 64 lanes share one row (j, k) and every access is a wave-wide coalesced 8-byte {D, W} (16-byte
//                  colour) vector access.  In the device layout the old voxel (i + s_x, j + s_y, k + s_z) lies one flat offset
//                  (s_z ny + s_y) nx + s_x behind the new one, and it exists inside a box of the new indices: a wave whose source row
//                  lies outside the volume stores zeros and loads nothing, a lane whose source column does stores zeros.  The records
//                  move as integer words: a NaN's payload and a -0 survive.
// An in-place move would race between workgroups, so the launch reads the live buffers and writes a second pair of the volume's size,
// and the two pairs swap after it: nothing waits for another workgroup, there are no atomics, one writer per voxel, no LDS.  The launch
// moves every byte of the volume twice (one read, one write, less the slab that enters).
#include "icp_tsdf.h"
#include "icp_cguard.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr uint32_t SH_I = 64u, SH_J = 4u;                  // a block of k_tsdf_shift: 64 i x 4 j
constexpr int32_t WINDOW_MAX = 1 << 24;                    // |c_a| <= 2^24: (float) c_a is exact

struct tsdf_shift_args {
    uint32_t nx, ny, nz;
    int32_t sx, sy, sz;                                    // each in [-n_a, n_a]
    const uint2 *src_dw; uint2 *dst_dw;
    const uint4 *src_col; uint4 *dst_col;                  // null without colour
};

__global__ __launch_bounds__ (256) void k_tsdf_shift (tsdf_shift_args a)
{
    const uint32_t i = blockIdx.x * SH_I + threadIdx.x % SH_I, j = blockIdx.y * SH_J + threadIdx.x / SH_I, k = blockIdx.z;
    if (i >= a.nx || j >= a.ny) return;
    const int32_t si = (int32_t) i + a.sx, sj = (int32_t) j + a.sy, sk = (int32_t) k + a.sz;        // (|.| <= 2047)
    const size_t at = ((size_t) k * a.ny + j) * a.nx + i;
    uint2 dw = make_uint2 (0u, 0u);
    uint4 col = make_uint4 (0u, 0u, 0u, 0u);
    if (sj >= 0 && sj < (int32_t) a.ny && sk >= 0 && sk < (int32_t) a.nz) {                         // (wave-uniform: a wave has one j and one k)
        if (si >= 0 && si < (int32_t) a.nx) {
            const size_t from = ((size_t) (uint32_t) sk * a.ny + (uint32_t) sj) * a.nx + (uint32_t) si;      // (< nx ny nz)
            dw = a.src_dw[from];
            if (a.src_col) col = a.src_col[from];
        }
    }
    a.dst_dw[at] = dw;
    if (a.dst_col) a.dst_col[at] = col;
}

size_t voxels (const icp_tsdf_t &c) { return (size_t) c.nx * c.ny * c.nz; }

tsdf_shift_args shift_args (const icp_tsdf_context *t, const int32_t *s)
{
    tsdf_shift_args a {};
    a.nx = t->cfg.nx; a.ny = t->cfg.ny; a.nz = t->cfg.nz;
    // (a shift of n_a or more empties the volume whatever it is: clamped, the kernel's index sums stay small)
    a.sx = std::max (-(int32_t) a.nx, std::min ((int32_t) a.nx, s[0]));
    a.sy = std::max (-(int32_t) a.ny, std::min ((int32_t) a.ny, s[1]));
    a.sz = std::max (-(int32_t) a.nz, std::min ((int32_t) a.nz, s[2]));
    a.src_dw = reinterpret_cast<const uint2 *> (t->v.dw); a.dst_dw = reinterpret_cast<uint2 *> (t->dw2);
    a.src_col = reinterpret_cast<const uint4 *> (t->v.col); a.dst_col = reinterpret_cast<uint4 *> (t->col2);
    return a;
}

void launch_shift (const tsdf_shift_args &a, hipStream_t s)
{
    hipLaunchKernelGGL (k_tsdf_shift, dim3 ((a.nx + SH_I - 1u) / SH_I, (a.ny + SH_J - 1u) / SH_J, a.nz), dim3 (256), 0, s, a);
}

// the second pair of buffers, allocated once (ICP_ENOMEM with the volume as it was)
int reserve_second (icp_tsdf_context *t, const char *who)
{
    const size_t n = voxels (t->cfg);
    if (!t->dw2 && hipMalloc ((void **) &t->dw2, n * sizeof (float2)) != hipSuccess) {
        (void) hipGetLastError (); t->dw2 = nullptr;
        return icp_host::tsdf_fail (t, ICP_ENOMEM, std::string (who) + ": the device cannot hold the second buffer of the volume");
    }
    if (t->v.col && !t->col2 && hipMalloc ((void **) &t->col2, n * sizeof (float4)) != hipSuccess) {
        (void) hipGetLastError (); t->col2 = nullptr;
        return icp_host::tsdf_fail (t, ICP_ENOMEM, std::string (who) + ": the device cannot hold the second buffer of the volume's colour");
    }
    return ICP_OK;
}

}  // namespace

namespace icp_host {

int tsdf_time_shift (icp_tsdf_context *t, const int32_t *s, uint32_t reps, float *us_per_launch)
{
    if (!s) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_time: what = 10 takes the three int32 of the shift through `depth`");
    TSDFCHK (t, hipSetDevice (t->device));
    int rc = reserve_second (t, "icp_tsdf_time"); if (rc) return rc;
    const int32_t back[3] = { -s[0], -s[1], -s[2] };
    const tsdf_shift_args fwd = shift_args (t, s), bwd = shift_args (t, back);
    launch_shift (fwd, t->stream);                  // (untimed: the code object is loaded)
    TSDFCHK (t, hipEventRecord (t->ev0, t->stream));
    for (uint32_t i = 0; i < reps; ++i) launch_shift (i & 1u ? bwd : fwd, t->stream);
    TSDFCHK (t, hipEventRecord (t->ev1, t->stream));
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipEventSynchronize (t->ev1));
    float ms = 0.f;
    TSDFCHK (t, hipEventElapsedTime (&ms, t->ev0, t->ev1));
    *us_per_launch = ms * 1e3f / (float) reps;
    return ICP_OK;
}

}  // namespace icp_host

using namespace icp_host;

extern "C" {

int icp_tsdf_get_window (icp_tsdf_handle t, int32_t cumulative[3]) try
{
    if (!t) return ICP_EINVAL;
    if (!cumulative) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_get_window: null pointer");
    for (int a = 0; a < 3; ++a) cumulative[a] = t->win[a];
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_shift (icp_tsdf_handle t, const int32_t shift[3]) try
{
    if (!t) return ICP_EINVAL;
    if (!shift) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_shift: null pointer");
    int32_t c[3];
    float origin[3];
    for (int a = 0; a < 3; ++a) {
        const int64_t sum = (int64_t) t->win[a] + shift[a];
        if (sum > WINDOW_MAX || sum < -WINDOW_MAX) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_shift: the cumulative shift must stay within 2^24 voxels on every axis");
        c[a] = (int32_t) sum;
        const float step = (float) c[a] * t->cfg.voxel;    // (one multiplication, one addition, each rounded on its own)
        origin[a] = t->base[a] + step;
        if (!std::isfinite (origin[a])) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_shift: the new origin is not finite");
    }
    if (shift[0] == 0 && shift[1] == 0 && shift[2] == 0) return ICP_OK;
    TSDFCHK (t, hipSetDevice (t->device));
    int rc = reserve_second (t, "icp_tsdf_shift"); if (rc) return rc;
    launch_shift (shift_args (t, shift), t->stream);
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    std::swap (t->v.dw, t->dw2);
    std::swap (t->v.col, t->col2);
    for (int a = 0; a < 3; ++a) { t->win[a] = c[a]; t->cfg.origin[a] = origin[a]; }
    t->v.ox = origin[0]; t->v.oy = origin[1]; t->v.oz = origin[2];
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_kept_box (const icp_tsdf_t *cfg, const int32_t shift[3], icp_tsdf_region_t *out) try
{
    if (!cfg || !shift || !out) return ICP_EINVAL;
    const uint32_t n[3] = { cfg->nx, cfg->ny, cfg->nz };
    for (int a = 0; a < 3; ++a) {
        const int64_t m = n[a], s = shift[a], lo = std::min (m, std::max<int64_t> (0, s)), hi = std::max (lo, std::min (m, m + s));
        out->lo[a] = (uint32_t) lo; out->hi[a] = (uint32_t) hi;
    }
    out->mode = ICP_TSDF_REGION_OUTSIDE;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_follow (const icp_tsdf_t *cfg, const float point[3], uint32_t threshold, int32_t shift_out[3]) try
{
    if (!cfg || !point || !shift_out) return ICP_EINVAL;
    const uint32_t n[3] = { cfg->nx, cfg->ny, cfg->nz };
    const double voxel = cfg->voxel;
    double d[3], far = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double centre = (double) cfg->origin[a] + 0.5 * ((double) n[a] - 1.0) * voxel;
        d[a] = ((double) point[a] - centre) / voxel;
        if (!(std::fabs (d[a]) <= 2147483520.0)) return ICP_EINVAL;       // (NaN, or a shift that is no int32)
        far = std::max (far, std::fabs (d[a]));
    }
    const bool move = far > (double) threshold;
    for (int a = 0; a < 3; ++a) shift_out[a] = move ? (int32_t) std::lrint (d[a]) : 0;
    return ICP_OK;
}
ICP_CATCH_ALL

}  // extern "C"
