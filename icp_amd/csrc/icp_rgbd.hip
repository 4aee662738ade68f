// icp_rgbd.hip — the RGB-D front end: a 16-bit depth image and an 8-bit colour image become float8 points on the device (the rule:
// include/icp_amd.h, "RGB-D front end"; tests/rgbd_ref.py restates it).  The reference makes the cloud on the host
// (src/kinect_frame_grabber.cpp:246-262) and can smooth the images first (:179-243); here the depth is filtered, back-projected and, where
// asked for, given normals by one launch, in two forms of the same arithmetic:
//
//   k_rgbd_dense    every pixel of an image.  A block of 256 lanes owns a tile of 32 x 8 pixels: it stages the counts of the tile and a halo
//                   of radius (+ 1 with normals) in LDS once — an invalid or absent count as 0 —, filters the depth of the tile (+ one
//                   ring with normals) from there into LDS, and each lane then builds its pixel's point — and, with normals, the four
//                   neighbouring vertices — from those depths.
//   k_rgbd_lattice  only the side x side landmarks (x0 + step_x i, y0 + step_y j).  Sixteen lanes, one DPP row, serve a landmark: the taps of
//                   a window (up to 169, five windows with normals) are dealt out lane by lane, each lane keeps its part of the two
//                   sums, and four xor-shuffles inside the row add the parts.  The sums are integers, so the split changes no bit.
//                   It reads the lattice's bounding box grown by radius (+ 1) and nothing else: icp_write_rgbd holds those image rows
//                   on the device, tracking the packed box (icp_rgbd_args).  Why sixteen: DESIGN.md section 5.
//
// The filter's sums in integers: with e = c_q - c0 and w = w_s w_r (< 2^30),  D = sum w  (< 2^36),  E = sum w e  (|E| < 2^48),
// N = c0 D + E  (< 2^53, the header's bound) — "any exact integer evaluation is allowed".  One double division, one rounding to float,
// one float multiplication; -ffp-contract=off keeps every other operation on its own.  No scratch, no atomics.
#include "icp_rgbd.h"
#include "icp_normal_rule.h"

#include <cmath>

namespace {

constexpr uint32_t TILE_W = 32u, TILE_H = 8u, MAX_R = 6u, MAX_HALO = MAX_R + 1u;
constexpr uint32_t CNT_W = TILE_W + 2u * MAX_HALO + 2u, CNT_H = TILE_H + 2u * MAX_HALO;      // 48 x 22 counts
constexpr uint32_t ZT_W = TILE_W + 2u + 2u, ZT_H = TILE_H + 2u;                                // 36 x 10 depths
constexpr uint32_t LPL = 16u;                                                                     // lanes per landmark (k_rgbd_lattice)

// a count as the filter sees it: itself where it is valid, else 0 (which is never valid)
__device__ __forceinline__ uint32_t rgbd_count (const icp_rgbd_t &c, uint32_t raw) { return (raw != 0u && raw >= c.d_min && raw <= c.d_max) ? raw : 0u; }

// one neighbour q = p + (dx, dy) with count cq (0: does not count) of a centre with count c0
__device__ __forceinline__ void rgbd_tap (uint32_t r, uint32_t S, uint32_t c0, uint32_t cq, int dx, int dy, unsigned long long &D, long long &E)
{
    const int ws = (int) ((r + 1u) * (r + 1u)) - dx * dx - dy * dy, e = (int) cq - (int) c0, ae = e < 0 ? -e : e;
    if (cq == 0u || ws <= 0 || (uint32_t) ae >= S) return;
    const uint32_t w = (uint32_t) ws * (S * S - (uint32_t) (ae * ae));
    D += w;
    E += (long long) w * e;
}

__device__ __forceinline__ float rgbd_depth (uint32_t c0, unsigned long long D, long long E, float scale)
{
    const unsigned long long N = (unsigned long long) ((long long) (c0 * D) + E);
    return (float) ((double) N / (double) D) * scale;
}

__device__ __forceinline__ float3 rgbd_vertex (const icp_rgbd_t &c, uint32_t u, uint32_t v, float z)
{
    return make_float3 (((float) u - c.cx) * z / c.fx, ((float) v - c.cy) * z / c.fy, z);
}

__device__ __forceinline__ float4 rgbd_colour (const uint8_t *px)
{
    if (!px) return make_float4 (0.f, 0.f, 0.f, 1.f);
    return make_float4 ((float) px[0] / 255.f, (float) px[1] / 255.f, (float) px[2] / 255.f, 1.f);
}

__global__ __launch_bounds__ (256) void k_rgbd_dense (icp_rgbd_args a)
{
    __shared__ uint16_t cnt[CNT_H][CNT_W];
    __shared__ float zt[ZT_H][ZT_W];
    const icp_rgbd_t &c = a.c;
    const uint32_t r = c.radius, e = a.nrm ? 1u : 0u, h = r + e, tid = threadIdx.x;
    const int u0 = (int) (blockIdx.x * TILE_W), v0 = (int) (blockIdx.y * TILE_H);
    // the counts of the tile and its halo: cnt[ly][lx] = pixel (u0 - h + lx, v0 - h + ly)
    const uint32_t cw = TILE_W + 2u * h, ch = TILE_H + 2u * h;
    for (uint32_t k = tid; k < cw * ch; k += 256u) {
        const uint32_t lx = k % cw, ly = k / cw;
        const int u = u0 - (int) h + (int) lx, v = v0 - (int) h + (int) ly;
        uint32_t raw = 0u;
        if (u >= 0 && v >= 0 && u < (int) c.width && v < (int) c.height) raw = a.depth[(size_t) v * a.dpitch + (uint32_t) u];
        cnt[ly][lx] = (uint16_t) rgbd_count (c, raw);
    }
    __syncthreads ();
    // the depths of the tile and, with normals, one ring: zt[ly][lx] = pixel (u0 - e + lx, v0 - e + ly), whose count is cnt[ly + r][lx + r]
    const uint32_t zw = TILE_W + 2u * e, zh = TILE_H + 2u * e;
    for (uint32_t k = tid; k < zw * zh; k += 256u) {
        const uint32_t lx = k % zw, ly = k / zw, c0 = cnt[ly + r][lx + r];
        float z = 0.f;
        if (c0 != 0u) {
            if (r == 0u) z = (float) c0 * c.depth_scale;
            else {
                unsigned long long D = 0ull; long long E = 0ll;
                for (int dy = -(int) r; dy <= (int) r; ++dy)
                    for (int dx = -(int) r; dx <= (int) r; ++dx)
                        rgbd_tap (r, c.range, c0, cnt[(int) (ly + r) + dy][(int) (lx + r) + dx], dx, dy, D, E);
                z = rgbd_depth (c0, D, E, c.depth_scale);
            }
        }
        zt[ly][lx] = z;
    }
    __syncthreads ();
    const uint32_t tx = tid % TILE_W, ty = tid / TILE_W, u = (uint32_t) u0 + tx, v = (uint32_t) v0 + ty;
    if (u >= c.width || v >= c.height) return;
    const size_t i = (size_t) v * c.width + u;
    const float3 p = rgbd_vertex (c, u, v, zt[ty + e][tx + e]);
    a.out[2 * i] = make_float4 (p.x, p.y, p.z, 1.f);
    a.out[2 * i + 1] = rgbd_colour (a.rgb ? a.rgb + i * 3 : nullptr);
    if (a.nrm) {
        const bool hasl = u > 0u, hasr = u + 1u < c.width, hasu = v > 0u, hasd = v + 1u < c.height;
        a.nrm[i] = icp_grid_normal (p, rgbd_vertex (c, u - 1u, v, zt[ty + 1u][tx]), hasl, rgbd_vertex (c, u + 1u, v, zt[ty + 1u][tx + 2u]), hasr,
                                    rgbd_vertex (c, u, v - 1u, zt[ty][tx + 1u]), hasu, rgbd_vertex (c, u, v + 1u, zt[ty + 2u][tx + 1u]), hasd);
    }
}

// the count of image pixel (u, v) as the filter sees it; 0 outside the image
__device__ __forceinline__ uint32_t rgbd_count_at (const icp_rgbd_args &a, int u, int v)
{
    if (u < 0 || v < 0 || u >= (int) a.c.width || v >= (int) a.c.height) return 0u;
    return rgbd_count (a.c, a.depth[(size_t) ((uint32_t) v - a.dy0) * a.dpitch + ((uint32_t) u - a.dx0)]);
}

// the depth of pixel (u, v), the same value in all sixteen lanes of the row (every lane of the wave calls it: the shuffles are unconditional)
__device__ __forceinline__ float rgbd_depth_row (const icp_rgbd_args &a, uint32_t l, int u, int v)
{
    const icp_rgbd_t &c = a.c;
    const uint32_t r = c.radius, c0 = rgbd_count_at (a, u, v);
    if (r == 0u) return (float) c0 * c.depth_scale;                       // (wave-uniform; an invalid pixel: 0 * scale = 0)
    unsigned long long D = 0ull; long long E = 0ll;
    const uint32_t n = 2u * r + 1u;
    if (c0 != 0u)
        for (uint32_t t = l; t < n * n; t += LPL) {
            const int dx = (int) (t % n) - (int) r, dy = (int) (t / n) - (int) r;
            rgbd_tap (r, c.range, c0, rgbd_count_at (a, u + dx, v + dy), dx, dy, D, E);
        }
#pragma unroll
    for (int m = 1; m < (int) LPL; m <<= 1) { D += __shfl_xor (D, m, (int) LPL); E += __shfl_xor (E, m, (int) LPL); }
    return c0 != 0u ? rgbd_depth (c0, D, E, c.depth_scale) : 0.f;
}

__global__ __launch_bounds__ (256) void k_rgbd_lattice (icp_rgbd_args a)
{
    const icp_rgbd_t &c = a.c;
    const uint32_t l = threadIdx.x % LPL, g = blockIdx.x * (256u / LPL) + threadIdx.x / LPL, m = a.side * a.side;
    const uint32_t gi = g < m ? g : m - 1u;                                 // (the lanes past the last landmark keep the shuffles whole and store nothing)
    const uint32_t u = c.x0 + c.step_x * (gi % a.side), v = c.y0 + c.step_y * (gi / a.side);
    const float3 p = rgbd_vertex (c, u, v, rgbd_depth_row (a, l, (int) u, (int) v));
    float4 n = make_float4 (0.f, 0.f, 0.f, 0.f);
    if (a.nrm) {                                                            // (wave-uniform)
        const bool hasl = u > 0u, hasr = u + 1u < c.width, hasu = v > 0u, hasd = v + 1u < c.height;
        const float3 pl = rgbd_vertex (c, u - 1u, v, rgbd_depth_row (a, l, (int) u - 1, (int) v));
        const float3 pr = rgbd_vertex (c, u + 1u, v, rgbd_depth_row (a, l, (int) u + 1, (int) v));
        const float3 pu = rgbd_vertex (c, u, v - 1u, rgbd_depth_row (a, l, (int) u, (int) v - 1));
        const float3 pd = rgbd_vertex (c, u, v + 1u, rgbd_depth_row (a, l, (int) u, (int) v + 1));
        n = icp_grid_normal (p, pl, hasl, pr, hasr, pu, hasu, pd, hasd);
    }
    if (g >= m || l != 0u) return;
    a.out[2 * (size_t) g] = make_float4 (p.x, p.y, p.z, 1.f);
    a.out[2 * (size_t) g + 1] = rgbd_colour (a.rgb ? a.rgb + ((size_t) ((v - a.cy0) / a.cstep) * a.cpitch + (u - a.cx0)) * 3 : nullptr);
    if (a.nrm) a.nrm[g] = n;
}

}  // namespace

void icp_launch_rgbd_dense (const icp_rgbd_args &a, hipStream_t s)
{
    hipLaunchKernelGGL (k_rgbd_dense, dim3 ((a.c.width + TILE_W - 1u) / TILE_W, (a.c.height + TILE_H - 1u) / TILE_H), dim3 (256), 0, s, a);
}

void icp_launch_rgbd_lattice (const icp_rgbd_args &a, hipStream_t s)
{
    const uint32_t per_block = 256u / LPL;
    hipLaunchKernelGGL (k_rgbd_lattice, dim3 ((a.side * a.side + per_block - 1u) / per_block), dim3 (256), 0, s, a);
}

icp_rgbd_t icp_rgbd_default ()
{
    icp_rgbd_t c {};
    c.width = 640u; c.height = 480u; c.fx = c.fy = 595.f; c.cx = 319.5f; c.cy = 239.5f; c.depth_scale = 1.f; c.d_min = 1u; c.d_max = 65535u;
    c.x0 = ICP_BAND_COL0; c.y0 = ICP_BAND_ROW0; c.step_x = 4u; c.step_y = ICP_BAND_ROW_STEP; c.radius = 0u; c.range = 30u;
    return c;
}

const char *icp_rgbd_refusal (const icp_rgbd_t &c)
{
    if (c.width < 1u || c.width > 4096u || c.height < 1u || c.height > 4096u) return "width and height must be in [1, 4096]";
    if (!(std::isfinite (c.fx) && c.fx > 0.f && std::isfinite (c.fy) && c.fy > 0.f)) return "fx and fy must be finite and > 0";
    if (!(std::isfinite (c.cx) && std::isfinite (c.cy))) return "cx and cy must be finite";
    if (!(std::isfinite (c.depth_scale) && c.depth_scale > 0.f)) return "depth_scale must be finite and > 0";
    if (c.d_max > 65535u || c.d_min > c.d_max) return "d_min <= d_max <= 65535 is required";
    if (c.step_x < 1u || c.step_y < 1u) return "step_x and step_y must be >= 1";
    if (c.radius > MAX_R) return "radius must be in [0, 6]";
    if (c.range < 1u || c.range > 4095u) return "range must be in [1, 4095]";
    return nullptr;
}

bool icp_rgbd_lattice_fits (const icp_rgbd_t &c, uint32_t side)
{
    if (side == 0u) return false;
    return (uint64_t) c.x0 + (uint64_t) c.step_x * (side - 1u) < c.width && (uint64_t) c.y0 + (uint64_t) c.step_y * (side - 1u) < c.height;
}

icp_rgbd_region icp_rgbd_region_of (const icp_rgbd_t &c, uint32_t side, bool normals)
{
    const uint32_t h = c.radius + (normals ? 1u : 0u), lastx = c.x0 + c.step_x * (side - 1u), lasty = c.y0 + c.step_y * (side - 1u);
    icp_rgbd_region g;
    g.dx0 = c.x0 > h ? c.x0 - h : 0u; g.dx1 = lastx + h + 1u < c.width ? lastx + h + 1u : c.width;
    g.dy0 = c.y0 > h ? c.y0 - h : 0u; g.dy1 = lasty + h + 1u < c.height ? lasty + h + 1u : c.height;
    g.cx1 = lastx + 1u;
    return g;
}
