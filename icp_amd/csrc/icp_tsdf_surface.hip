// icp_tsdf_surface.hip — the surface of a TSDF volume as a point cloud, extracted on the device (icp_tsdf_extract_surface; the rule:
// include/icp_amd.h, "Surface extraction"; tests/tsdf_surface_ref.py restates it).  The points are the zero crossings of D on the edges
// between neighbouring usable voxels, in ascending 3 * (linear voxel index) + axis: an ordered stream compaction of a sweep over the
// volume, in the form of icp_pairs.hip carried to a volume's 2^20 blocks.
//
// A block owns RUN = 1024 consecutive linear voxel indices, as STEPS = 4 sub-runs of 256: lane l of wave w judges voxel
// RUN blk + 256 s + 64 w + l in step s, so a wave's {D, W} access is one coalesced 8-byte vector access whether or not a row ends inside
// it, and the order of the output is the order of (blk, s, w, lane, axis).
//
//   k_tsdf_surface_count    the sweep.  A voxel that is not usable is the low end of no member: its +x, +y, +z neighbours (plain loads at
//                           offsets 1, nx, nx ny; the z neighbour comes back one slice later) are fetched, and its indices divided out,
//                           only where the voxel itself is usable — a wave of free or unseen space makes one load.  Every lane has 0 to 3
//                           members: three ballots a step.  A wave stores its four steps' counts as four bytes (at most 192 a step) and,
//                           for a step with members, the three ballots themselves (24 bytes for 512 bytes of {D, W}); the block stores
//                           the sum of its counts.
//   k_tsdf_scan_tiles       exclusive scan of SCAN_TILE = 1024 words per block, four per lane: the offsets inside the tile and the tile's
//                           sum.  Launched twice: over the block counts (at most 2^20: 1024 tiles), then as one block over the tile sums,
//                           whose sum is the number of members.
//   k_tsdf_surface_scatter  one block per block of the sweep, which judges nothing again: a wave reads its block's sixteen counts, its
//                           offsets and its own ballots in one round trip, leaves if it has no member, and member (lane, axis) goes to
//                               (tile offset + offset inside the tile) + (members of the steps and waves in front: sums of those bytes) +
//                               (members below the lane: mbcnt of the three ballots) + (the lane's own members on lower axes)
//                           as the word 3 * (linear voxel index) + axis.  No LDS, no barrier.  Positions past the capacity are not written.
//   k_tsdf_surface_points   a lane per written member: D0, D1, the colour and the twelve gradient samples are fetched for members only,
//                           all in one round trip, and the record is three 16-byte stores.  (A wall across the x axis has one member in
//                           every row, so one in a wave of 64 i: gathered from the scatter's lanes, the members' loads were instructions
//                           with one lane in use, and that pass was measured at 165 us for 465 000 members, 78 us without the gradients;
//                           here 64 members share an instruction.)
// A region (icp_tsdf_extract_surface_region; the rule: include/icp_amd.h, "Moving volume") is the same four passes with the box test in the
// sweep's member predicate (k_tsdf_surface_count_region), launched over the blocks that can hold a member of the wanted kind alone; the
// counts of the other blocks are cleared, so the scan, the scatter and the points are the full extraction's launches as they are.
// Nothing waits for another workgroup inside a launch: the order between the passes is the stream's.  The counts are integer sums and a
// position is a function of the predicate alone: no atomics, and the result does not depend on the launch shape.
//
// The mesh (icp_tsdf_extract_mesh; the rule: include/icp_amd.h, "Mesh extraction"; tests/tsdf_mesh_ref.py restates it) has the members as its
// vertices and adds a second compaction of the same form, of up to five triangles per cell, queued after the member sweep and its scan:
//   k_tsdf_mesh_count       the sweep over cells, lane = voxel = the cell's corner 0.  It stores 16 bits a wave and step (up to 320
//                           triangles) and, for a step with triangles, the lanes' case bytes; the block stores its sum (at most 5120).
//   k_tsdf_scan_tiles       as above, over the triangle block counts.  One synchronisation then reads both counts.
//   k_tsdf_mesh_triangles   a lane per cell: a cell's local edge becomes its vertex index by the scatter's formula read from the member
//                           sweep's tables (no dense edge-to-index volume), and the triples are stored in order.
// The case table (256 words: a 4-bit count, fifteen 4-bit edge ids) is generated on the host by its rule and read from device memory.
//
// -ffp-contract=off keeps every operation on its own; `/` and sqrtf are the correctly rounded ones.
#include "icp_tsdf.h"
#include "icp_cguard.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr uint32_t BLOCK = 256u, WAVES = BLOCK / 64u;
constexpr uint32_t STEPS = 4u, RUN = BLOCK * STEPS;        // voxels of a block
constexpr uint32_t SCAN_TILE = BLOCK * 4u;                 // words of a block of k_tsdf_scan_tiles
constexpr uint32_t MASKS = STEPS * 3u;                     // ballots a wave of the sweep may store: [step][axis]

typedef unsigned long long mask64;

struct tsdf_surface_args {
    icp_tsdf_dev v;
    float min_weight;
    uint32_t n_vox;                                        // nx ny nz <= 2^30
    // what the sweep leaves: [nblk][WAVES] words, byte s of word w = the members of wave w in step s;  [nblk][WAVES][STEPS][3] ballots,
    // written for the steps whose byte is not 0;  [nblk] sums
    uint32_t *wave_cnt; mask64 *masks; uint32_t *blk_cnt;
    const uint32_t *blk_off, *tile_off;                    // the scan: a block's offset inside its tile, a tile's offset
    uint32_t limit;                                        // min (count, capacity): positions below it are written
    uint32_t *edge;                                        // [limit]: member p is edge 3 * (linear voxel index) + axis
    float4 *out, *nrm;                                     // [limit][2], [limit] or null
};

__device__ __forceinline__ bool usable (float2 dw, float min_weight) { return dw.y >= min_weight && fabsf (dw.x) < 1.f; }

__device__ __forceinline__ uint32_t below_lane (mask64 bal, uint32_t add)
{
    return __builtin_amdgcn_mbcnt_hi ((uint32_t) (bal >> 32), __builtin_amdgcn_mbcnt_lo ((uint32_t) bal, add));
}

__global__ __launch_bounds__ (BLOCK) void k_tsdf_surface_count (tsdf_surface_args a)
{
    __shared__ uint32_t s_wave[WAVES];
    const icp_tsdf_dev &v = a.v;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, g0 = blockIdx.x * RUN + tid;
    float2 own[STEPS];                                     // all steps in flight together (a lane past the volume reads the last voxel)
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) own[s] = v.dw[min (g0 + s * BLOCK, a.n_vox - 1u)];
    const uint32_t off[3] = { 1u, v.nx, v.nx * v.ny };
    uint32_t c = 0u, steps = 0u;
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) {
        const uint32_t g = g0 + s * BLOCK;
        bool m[3] = { false, false, false };
        if (g < a.n_vox && usable (own[s], a.min_weight)) {
            const uint32_t row = g / v.nx, i = g - row * v.nx, k = row / v.ny, j = row - k * v.ny;
            const bool inside[3] = { i + 1u < v.nx, j + 1u < v.ny, k + 1u < v.nz };
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (!inside[ax]) continue;                 // (g + off <= n_vox - 1 where the neighbour exists)
                const float2 e = v.dw[g + off[ax]];
                m[ax] = usable (e, a.min_weight) && ((own[s].x > 0.f) != (e.x > 0.f));
            }
        }
        const mask64 b0 = __ballot (m[0]), b1 = __ballot (m[1]), b2 = __ballot (m[2]);
        const uint32_t n = (uint32_t) (__popcll (b0) + __popcll (b1) + __popcll (b2));
        c += n; steps |= n << (8u * s);
        if (n && lane < 3u) a.masks[((size_t) (blockIdx.x * WAVES + wave) * STEPS + s) * 3u + lane] = lane == 0u ? b0 : lane == 1u ? b1 : b2;
    }
    if (lane == 0u) { s_wave[wave] = c; a.wave_cnt[blockIdx.x * WAVES + wave] = steps; }
    __syncthreads ();
    if (tid == 0u) a.blk_cnt[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// A region of icp_tsdf_extract_surface_region: the box lo_a <= idx_a < hi_a and the first block of the sweep's launch (the blocks in
// front of it can hold no member of the wanted kind).
struct tsdf_region_dev { uint32_t lo[3], hi[3], first_blk; };
struct tsdf_region_args { tsdf_surface_args a; tsdf_region_dev r; };

// The sweep of a region: k_tsdf_surface_count with the box test in the member predicate, the wanted kind as a template parameter.  Member
// (v, ax) is INSIDE iff v and v + e_ax both lie in the box, and is kept iff that is the kind wanted.  A voxel that can be the low end of no
// member of the wanted kind — for INSIDE one with no edge that ends in the box; for OUTSIDE one in the box whose every edge ends in the
// box — is not loaded: a wave of such voxels makes no load at all.  (A kernel of its own, not a switch in k_tsdf_surface_count's body: with
// the body shared, the compiler reassociates the full extraction's integer sums differently, and that kernel is to stay the code it is.)
template <bool OUTSIDE>
__global__ __launch_bounds__ (BLOCK) void k_tsdf_surface_count_region (tsdf_region_args q)
{
    __shared__ uint32_t s_wave[WAVES];
    const tsdf_surface_args &a = q.a;
    const tsdf_region_dev &r = q.r;
    const icp_tsdf_dev &v = a.v;
    const uint32_t blk = blockIdx.x + r.first_blk;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, g0 = blk * RUN + tid;
    float2 own[STEPS];                                     // all steps in flight together
    bool in[STEPS][3];                                     // edge (v, ax) would be INSIDE
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) {
        const uint32_t g = min (g0 + s * BLOCK, a.n_vox - 1u);
        const uint32_t row = g / v.nx, i = g - row * v.nx, k = row / v.ny, j = row - k * v.ny;
        const bool vin = i >= r.lo[0] && i < r.hi[0] && j >= r.lo[1] && j < r.hi[1] && k >= r.lo[2] && k < r.hi[2];
        in[s][0] = vin && i + 1u < r.hi[0]; in[s][1] = vin && j + 1u < r.hi[1]; in[s][2] = vin && k + 1u < r.hi[2];
        const bool can = OUTSIDE ? !(vin && (in[s][0] || i + 1u >= v.nx) && (in[s][1] || j + 1u >= v.ny) && (in[s][2] || k + 1u >= v.nz))
                                 : (in[s][0] || in[s][1] || in[s][2]);
        own[s] = make_float2 (0.f, 0.f);                   // (W = 0: not usable)
        if (can) own[s] = v.dw[g];
    }
    const uint32_t off[3] = { 1u, v.nx, v.nx * v.ny };
    uint32_t c = 0u, steps = 0u;
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) {
        const uint32_t g = g0 + s * BLOCK;
        bool m[3] = { false, false, false };
        if (g < a.n_vox && usable (own[s], a.min_weight)) {
            const uint32_t row = g / v.nx, i = g - row * v.nx, k = row / v.ny, j = row - k * v.ny;
            const bool inside[3] = { i + 1u < v.nx, j + 1u < v.ny, k + 1u < v.nz };
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (!inside[ax] || in[s][ax] == OUTSIDE) continue;      // (no such edge, or not of the wanted kind)
                const float2 e = v.dw[g + off[ax]];
                m[ax] = usable (e, a.min_weight) && ((own[s].x > 0.f) != (e.x > 0.f));
            }
        }
        const mask64 b0 = __ballot (m[0]), b1 = __ballot (m[1]), b2 = __ballot (m[2]);
        const uint32_t n = (uint32_t) (__popcll (b0) + __popcll (b1) + __popcll (b2));
        c += n; steps |= n << (8u * s);
        if (n && lane < 3u) a.masks[((size_t) (blk * WAVES + wave) * STEPS + s) * 3u + lane] = lane == 0u ? b0 : lane == 1u ? b1 : b2;
    }
    if (lane == 0u) { s_wave[wave] = c; a.wave_cnt[blk * WAVES + wave] = steps; }
    __syncthreads ();
    if (tid == 0u) a.blk_cnt[blk] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// out[i] = in[first word of the tile] + .. + in[i - 1] for the n words in tiles of SCAN_TILE, sums[tile] = the tile's sum
__global__ __launch_bounds__ (BLOCK) void k_tsdf_scan_tiles (const uint32_t *in, uint32_t n, uint32_t *out, uint32_t *sums)
{
    __shared__ uint32_t s_wave[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, at = blockIdx.x * SCAN_TILE + tid * 4u;
    uint32_t x[4];
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) x[e] = at + e < n ? in[at + e] : 0u;
    const uint32_t mine = (x[0] + x[1]) + (x[2] + x[3]);
    uint32_t incl = mine;                                  // inclusive scan over the wave's lanes
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up (incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads ();
    uint32_t front = incl - mine;
    for (uint32_t w = 0; w < wave; ++w) front += s_wave[w];
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        if (at + e < n) out[at + e] = front;
        front += x[e];
    }
    if (tid == BLOCK - 1u) sums[blockIdx.x] = front;
}

// the six neighbours of voxel u = (i, j, k) at linear index g, which has all of them inside the volume
struct six { float2 xp, xm, yp, ym, zp, zm; };

__device__ __forceinline__ six neighbours (const icp_tsdf_dev &v, uint32_t g)
{
    const uint32_t sy = v.nx, sz = v.nx * v.ny;
    return six { v.dw[g + 1u], v.dw[g - 1u], v.dw[g + sy], v.dw[g - sy], v.dw[g + sz], v.dw[g - sz] };
}

__device__ __forceinline__ bool known (const six &n) { return n.xp.y > 0.f && n.xm.y > 0.f && n.yp.y > 0.f && n.ym.y > 0.f && n.zp.y > 0.f && n.zm.y > 0.f; }

// the record of member (v, AX), v = (i, j, k) at linear index g, at position pos: every load first, then the arithmetic of the rule
template <int AX>
__device__ __forceinline__ void emit (const tsdf_surface_args &a, uint32_t g, uint32_t i, uint32_t j, uint32_t k, uint32_t pos)
{
    const icp_tsdf_dev &v = a.v;
    const uint32_t off = AX == 0 ? 1u : AX == 1 ? v.nx : v.nx * v.ny;
    const uint32_t hi = i + (AX == 0), hj = j + (AX == 1), hk = k + (AX == 2);                // v + e_a
    // G is known at neither end unless both have their six neighbours inside
    const bool inside = a.nrm && i >= 1u && hi + 1u < v.nx && j >= 1u && hj + 1u < v.ny && k >= 1u && hk + 1u < v.nz;
    const float d0 = v.dw[g].x, d1 = v.dw[g + off].x;
    float4 c0 = make_float4 (0.f, 0.f, 0.f, 0.f), c1 = c0;
    if (v.col) { c0 = v.col[g]; c1 = v.col[g + off]; }
    six n0 {}, n1 {};
    if (inside) { n0 = neighbours (v, g); n1 = neighbours (v, g + off); }
    const float t = d0 / (d0 - d1);
    const float fi = (float) i, fj = (float) j, fk = (float) k;
    const float px = v.ox + (AX == 0 ? fi + t : fi) * v.voxel, py = v.oy + (AX == 1 ? fj + t : fj) * v.voxel, pz = v.oz + (AX == 2 ? fk + t : fk) * v.voxel;
    a.out[2 * (size_t) pos] = make_float4 (px, py, pz, 1.f);
    a.out[2 * (size_t) pos + 1] = make_float4 (c0.x + t * (c1.x - c0.x), c0.y + t * (c1.y - c0.y), c0.z + t * (c1.z - c0.z), 1.f);
    if (!a.nrm) return;
    float4 n = make_float4 (0.f, 0.f, 0.f, 0.f);
    if (inside && known (n0) && known (n1)) {
        const float g0x = n0.xp.x - n0.xm.x, g0y = n0.yp.x - n0.ym.x, g0z = n0.zp.x - n0.zm.x;
        const float g1x = n1.xp.x - n1.xm.x, g1y = n1.yp.x - n1.ym.x, g1z = n1.zp.x - n1.zm.x;
        const float gx = g0x + t * (g1x - g0x), gy = g0y + t * (g1y - g0y), gz = g0z + t * (g1z - g0z);
        const float len = sqrtf ((gx * gx + gy * gy) + gz * gz);
        if (len > 0.f) n = make_float4 (gx / len, gy / len, gz / len, 0.f);
    }
    a.nrm[pos] = n;
}

__global__ __launch_bounds__ (BLOCK) void k_tsdf_surface_scatter (tsdf_surface_args a)
{
    const uint32_t blk = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // one round trip: the block's counts, its offsets, the wave's ballots (those of a step without members were never written, and are not used)
    const uint4 wc = reinterpret_cast<const uint4 *> (a.wave_cnt)[blk];
    uint32_t front = a.tile_off[blk / SCAN_TILE] + a.blk_off[blk];                          // the position of the first member of step s
    const mask64 *mk = a.masks + (size_t) (blk * WAVES + wave) * MASKS;
    mask64 bal[MASKS];
#pragma unroll
    for (uint32_t e = 0; e < MASKS; ++e) bal[e] = mk[e];
    const uint32_t mine = wave == 0u ? wc.x : wave == 1u ? wc.y : wave == 2u ? wc.z : wc.w;
    if (mine == 0u || front >= a.limit) return;            // (wave-uniform)
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) {
        const uint32_t c0 = (wc.x >> (8u * s)) & 255u, c1 = (wc.y >> (8u * s)) & 255u, c2 = (wc.z >> (8u * s)) & 255u, c3 = (wc.w >> (8u * s)) & 255u;
        const uint32_t first = front + (wave > 0u ? c0 : 0u) + (wave > 1u ? c1 : 0u) + (wave > 2u ? c2 : 0u);
        front += (c0 + c1) + (c2 + c3);
        if (((mine >> (8u * s)) & 255u) == 0u) continue;
        if (first >= a.limit) break;                       // (the wave's later steps lie further back; the block's other waves may not)
        const mask64 b0 = bal[3u * s], b1 = bal[3u * s + 1u], b2 = bal[3u * s + 2u];
        const bool m0 = (b0 >> lane) & 1ull, m1 = (b1 >> lane) & 1ull, m2 = (b2 >> lane) & 1ull;
        if (!(m0 || m1 || m2)) continue;
        uint32_t pos = first + below_lane (b2, below_lane (b1, below_lane (b0, 0u)));
        const uint32_t e = 3u * (blk * RUN + s * BLOCK + wave * 64u + lane);               // (< 3 * 2^30)
        if (m0) { if (pos < a.limit) a.edge[pos] = e; ++pos; }
        if (m1) { if (pos < a.limit) a.edge[pos] = e + 1u; ++pos; }
        if (m2) { if (pos < a.limit) a.edge[pos] = e + 2u; }
    }
}

// a lane per written member: the gathers of 64 members are one wave's instructions
__global__ __launch_bounds__ (BLOCK) void k_tsdf_surface_points (tsdf_surface_args a)
{
    const icp_tsdf_dev &v = a.v;
    const uint32_t pos = blockIdx.x * BLOCK + threadIdx.x;
    if (pos >= a.limit) return;
    const uint32_t e = a.edge[pos], g = e / 3u, ax = e - 3u * g;
    if (g + (ax == 0u ? 1u : ax == 1u ? v.nx : v.nx * v.ny) >= a.n_vox) return;            // (never: a member's high end is inside the volume)
    const uint32_t row = g / v.nx, i = g - row * v.nx, k = row / v.ny, j = row - k * v.ny;
    if (ax == 0u) emit<0> (a, g, i, j, k, pos);
    else if (ax == 1u) emit<1> (a, g, i, j, k, pos);
    else emit<2> (a, g, i, j, k, pos);
}

// ---- the mesh: a second ordered compaction, of triangles per cell ---------------------------------------------------------------------------

constexpr uint32_t CELL_OK = 0x100u;                       // beside a lane's four sign bits: its corners 0, 2, 4, 6 are all usable

struct tsdf_mesh_args {
    tsdf_surface_args m;                                   // the volume and what the member sweep and its scan left
    const mask64 *table;                                   // [256]: a 4-bit triangle count, then fifteen 4-bit local edge ids
    // what the cell sweep leaves: [nblk][WAVES] pairs of words, 16 bits a step = the triangles of wave w in step s (at most 320);
    // [nblk][WAVES][STEPS][64] case bytes (0 for an inactive cell), written for the steps whose count is not 0;  [nblk] sums
    uint2 *wave_cnt; uint8_t *cases; uint32_t *blk_cnt;
    const uint32_t *blk_off, *tile_off;                    // the scan of the sums
    uint32_t limit;                                        // min (count, capacity): triangles below it are written
    uint32_t *tri;                                         // [limit][3]
};

// The sweep over cells in the member sweep's layout: lane = the cell's corner 0.  A lane fetches corners 2, 4 and 6 (+y, +z, +y +z) only
// where its own voxel is usable, and takes corners 1, 3, 5, 7 from the next lane, which fetched them as its own 0, 2, 4, 6 (the next
// lane is in the same row wherever the cell exists); only the wave's last lane loads them.  A lane's triangle count has three bits: three
// ballots give the wave's sum.
__global__ __launch_bounds__ (BLOCK) void k_tsdf_mesh_count (tsdf_mesh_args a)
{
    __shared__ uint32_t s_wave[WAVES];
    const icp_tsdf_dev &v = a.m.v;
    const float min_weight = a.m.min_weight;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, g0 = blockIdx.x * RUN + tid, n_vox = a.m.n_vox;
    float2 own[STEPS];
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) own[s] = v.dw[min (g0 + s * BLOCK, n_vox - 1u)];
    const uint32_t sy = v.nx, sz = v.nx * v.ny;
    uint32_t c = 0u, lo = 0u, hi = 0u;
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) {
        const uint32_t g = g0 + s * BLOCK;
        uint32_t mine = 0u;                                // CELL_OK | the signs of corners 0, 2, 4, 6 at their bits
        bool has_x = false;
        if (g < n_vox && usable (own[s], min_weight)) {
            const uint32_t row = g / v.nx, i = g - row * v.nx, k = row / v.ny, j = row - k * v.ny;
            has_x = i + 1u < v.nx;
            if (j + 1u < v.ny && k + 1u < v.nz) {          // (g + sz + sy <= n_vox - 1)
                const float2 e2 = v.dw[g + sy], e4 = v.dw[g + sz], e6 = v.dw[g + sz + sy];
                if (usable (e2, min_weight) && usable (e4, min_weight) && usable (e6, min_weight))
                    mine = CELL_OK | (uint32_t) (own[s].x > 0.f) | (uint32_t) (e2.x > 0.f) << 2 | (uint32_t) (e4.x > 0.f) << 4 | (uint32_t) (e6.x > 0.f) << 6;
            }
        }
        uint32_t next = __shfl_down (mine, 1u, 64);
        if (lane == 63u) {
            next = 0u;
            if (mine && has_x) {                           // (g + 1 + sz + sy <= n_vox - 1: the cell exists)
                const float2 e1 = v.dw[g + 1u], e3 = v.dw[g + 1u + sy], e5 = v.dw[g + 1u + sz], e7 = v.dw[g + 1u + sz + sy];
                if (usable (e1, min_weight) && usable (e3, min_weight) && usable (e5, min_weight) && usable (e7, min_weight))
                    next = CELL_OK | (uint32_t) (e1.x > 0.f) | (uint32_t) (e3.x > 0.f) << 2 | (uint32_t) (e5.x > 0.f) << 4 | (uint32_t) (e7.x > 0.f) << 6;
            }
        }
        const bool active = mine && has_x && next;
        const uint32_t cs = active ? (mine & 0x55u) | (next & 0x55u) << 1 : 0u;
        const uint32_t n = active ? (uint32_t) (a.table[cs] & 15ull) : 0u;
        const mask64 b0 = __ballot (n & 1u), b1 = __ballot (n & 2u), b2 = __ballot (n & 4u);
        const uint32_t tot = (uint32_t) (__popcll (b0) + 2 * __popcll (b1) + 4 * __popcll (b2));
        c += tot;
        if (s < 2u) lo |= tot << (16u * s); else hi |= tot << (16u * (s - 2u));
        if (tot) a.cases[((size_t) (blockIdx.x * WAVES + wave) * STEPS + s) * 64u + lane] = (uint8_t) cs;
    }
    if (lane == 0u) { s_wave[wave] = c; a.wave_cnt[blockIdx.x * WAVES + wave] = make_uint2 (lo, hi); }
    __syncthreads ();
    if (tid == 0u) a.blk_cnt[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__device__ __forceinline__ uint32_t step16 (uint2 w, uint32_t s) { return ((s < 2u ? w.x : w.y) >> (16u * (s & 1u))) & 0xFFFFu; }

// the position of the first member of voxel gv in the member order, by the scatter's formula, and whether (gv, x) and (gv, y) are members
__device__ __forceinline__ uint32_t first_member (const tsdf_surface_args &m, uint32_t gv, bool *m0, bool *m1)
{
    const uint32_t blk = gv / RUN, s = (gv / BLOCK) & (STEPS - 1u), w = (gv >> 6) & (WAVES - 1u), l = gv & 63u;
    const uint4 wc = reinterpret_cast<const uint4 *> (m.wave_cnt)[blk];
    uint32_t pos = m.tile_off[blk / SCAN_TILE] + m.blk_off[blk];
    const mask64 *mk = m.masks + ((size_t) (blk * WAVES + w) * STEPS + s) * 3u;
    const mask64 b0 = mk[0], b1 = mk[1], b2 = mk[2];       // (written: the voxel has a member in this step)
#pragma unroll
    for (uint32_t q = 0; q < STEPS; ++q) {
        const uint32_t c0 = (wc.x >> (8u * q)) & 255u, c1 = (wc.y >> (8u * q)) & 255u, c2 = (wc.z >> (8u * q)) & 255u, c3 = (wc.w >> (8u * q)) & 255u;
        if (q < s) pos += (c0 + c1) + (c2 + c3);
        else if (q == s) pos += (w > 0u ? c0 : 0u) + (w > 1u ? c1 : 0u) + (w > 2u ? c2 : 0u);
    }
    const mask64 below = (1ull << l) - 1ull;
    pos += (uint32_t) (__popcll (b0 & below) + __popcll (b1 & below) + __popcll (b2 & below));
    *m0 = (b0 >> l) & 1ull; *m1 = (b1 >> l) & 1ull;
    return pos;
}

// One block per block of the cell sweep, which judges nothing again: lane = cell.  The triangles of a cell go to
//     (tile offset + offset inside the tile) + (triangles of the steps and waves in front) + (triangles below the lane: three mbcnt)
// in table order.  A local edge 4 a + m is the lattice edge (corner voxel, a): its vertex index is that member's position, taken from the
// member sweep's own tables.  A lane keeps its up to twelve indices in LDS words of its own (no barrier), so that a triangle's edge id can
// index them.
__global__ __launch_bounds__ (BLOCK) void k_tsdf_mesh_triangles (tsdf_mesh_args a)
{
    __shared__ uint32_t s_idx[12][BLOCK];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4 wa = reinterpret_cast<const uint4 *> (a.wave_cnt)[2u * blk], wb = reinterpret_cast<const uint4 *> (a.wave_cnt)[2u * blk + 1u];
    uint32_t front = a.tile_off[blk / SCAN_TILE] + a.blk_off[blk];
    const uint2 w0 = make_uint2 (wa.x, wa.y), w1 = make_uint2 (wa.z, wa.w), w2 = make_uint2 (wb.x, wb.y), w3 = make_uint2 (wb.z, wb.w);
    const uint2 mine = wave == 0u ? w0 : wave == 1u ? w1 : wave == 2u ? w2 : w3;
    if ((mine.x | mine.y) == 0u || front >= a.limit) return;                                // (wave-uniform)
    const uint32_t sy = a.m.v.nx, sz = a.m.v.nx * a.m.v.ny;
#pragma unroll
    for (uint32_t s = 0; s < STEPS; ++s) {
        const uint32_t c0 = step16 (w0, s), c1 = step16 (w1, s), c2 = step16 (w2, s), c3 = step16 (w3, s);
        const uint32_t first = front + (wave > 0u ? c0 : 0u) + (wave > 1u ? c1 : 0u) + (wave > 2u ? c2 : 0u);
        front += (c0 + c1) + (c2 + c3);
        if (step16 (mine, s) == 0u) continue;
        if (first >= a.limit) break;
        const uint32_t cs = a.cases[((size_t) (blk * WAVES + wave) * STEPS + s) * 64u + lane];
        const mask64 word = a.table[cs];
        const uint32_t n = (uint32_t) (word & 15ull);
        const mask64 b0 = __ballot (n & 1u), b1 = __ballot (n & 2u), b2 = __ballot (n & 4u);
        const uint32_t pos = first + below_lane (b0, 0u) + 2u * below_lane (b1, 0u) + 4u * below_lane (b2, 0u);
        if (n == 0u || pos >= a.limit) continue;
        const uint32_t g = blk * RUN + s * BLOCK + wave * 64u + lane;
#pragma unroll
        for (uint32_t c = 0; c < 7u; ++c) {                // the corners that are the low end of a cell edge
            const uint32_t ends = (cs >> c) & 1u;
            const bool x0 = !(c & 1u) && ((cs >> (c | 1u)) & 1u) != ends, x1 = !(c & 2u) && ((cs >> (c | 2u)) & 1u) != ends, x2 = !(c & 4u) && ((cs >> (c | 4u)) & 1u) != ends;
            if (!(x0 || x1 || x2)) continue;
            bool m0, m1;
            const uint32_t at = first_member (a.m, g + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz, &m0, &m1);
            // local edge 4 a + m, m = bit_b1 + 2 bit_b2 of the corner
            if (!(c & 1u)) s_idx[((c >> 1) & 1u) + 2u * (c >> 2)][tid] = at;
            if (!(c & 2u)) s_idx[4u + (c & 1u) + 2u * (c >> 2)][tid] = at + (m0 ? 1u : 0u);
            if (!(c & 4u)) s_idx[8u + (c & 1u) + 2u * ((c >> 1) & 1u)][tid] = at + (m0 ? 1u : 0u) + (m1 ? 1u : 0u);
        }
        for (uint32_t t = 0; t < n && pos + t < a.limit; ++t) {
            uint32_t *out = a.tri + 3u * (size_t) (pos + t);
#pragma unroll
            for (uint32_t q = 0; q < 3u; ++q) out[q] = s_idx[(uint32_t) (word >> (4u + 4u * (3u * t + q))) & 15u][tid];
        }
    }
}

// The words of an extraction in the volume's scratch: the sweep's ballots (384 bytes a block of 8 KiB of {D, W}), its wave counts, its block
// counts; the blocks' offsets inside their tiles, the tile sums, the tile offsets, the count.  (The members' edges, like their records, are
// scratch of their own, sized by the count.)
struct surface_plan {
    uint32_t n_vox, nblk, ntile;
    mask64 *masks;
    uint32_t *wave_cnt, *blk_cnt, *blk_off, *tile_sum, *tile_off, *count;
};

int plan_surface (icp_tsdf_context *t, surface_plan *p)
{
    p->n_vox = t->cfg.nx * t->cfg.ny * t->cfg.nz;           // (<= 2^30: every axis <= 1024)
    p->nblk = (p->n_vox + RUN - 1u) / RUN;
    p->ntile = (p->nblk + SCAN_TILE - 1u) / SCAN_TILE;      // (<= 1024: the second scan is one block)
    const size_t units = (size_t) p->nblk * WAVES, words = units + 2u * (size_t) p->nblk + 2u * p->ntile + 1u;
    int rc = icp_host::tsdf_reserve (t, &t->dSurf, &t->surf_cap, units * MASKS * sizeof (mask64) + words * sizeof (uint32_t)); if (rc) return rc;
    p->masks = static_cast<mask64 *> (t->dSurf);
    p->wave_cnt = reinterpret_cast<uint32_t *> (p->masks + units * MASKS);                  // (16-byte aligned: a unit's ballots are 96 bytes)
    p->blk_cnt = p->wave_cnt + units; p->blk_off = p->blk_cnt + p->nblk;
    p->tile_sum = p->blk_off + p->nblk; p->tile_off = p->tile_sum + p->ntile; p->count = p->tile_off + p->ntile;
    return ICP_OK;
}

tsdf_surface_args args_of (const icp_tsdf_context *t, const surface_plan &p, float min_weight)
{
    tsdf_surface_args a {};
    a.v = t->v; a.min_weight = min_weight; a.n_vox = p.n_vox;
    a.wave_cnt = p.wave_cnt; a.masks = p.masks; a.blk_cnt = p.blk_cnt; a.blk_off = p.blk_off; a.tile_off = p.tile_off;
    return a;
}

void launch_scan (const surface_plan &p, hipStream_t s)
{
    hipLaunchKernelGGL (k_tsdf_scan_tiles, dim3 (p.ntile), dim3 (BLOCK), 0, s, (const uint32_t *) p.blk_cnt, p.nblk, p.blk_off, p.tile_sum);
    hipLaunchKernelGGL (k_tsdf_scan_tiles, dim3 (1), dim3 (BLOCK), 0, s, (const uint32_t *) p.tile_sum, p.ntile, p.tile_off, p.count);
}

// the count and the position of every block's first member
void launch_count_and_scan (const tsdf_surface_args &a, const surface_plan &p, hipStream_t s)
{
    hipLaunchKernelGGL (k_tsdf_surface_count, dim3 (p.nblk), dim3 (BLOCK), 0, s, a);
    launch_scan (p, s);
}

// the first a.limit > 0 members: their edges in order, then their records
void launch_scatter (const tsdf_surface_args &a, const surface_plan &p, hipStream_t s)
{
    hipLaunchKernelGGL (k_tsdf_surface_scatter, dim3 (p.nblk), dim3 (BLOCK), 0, s, a);
    hipLaunchKernelGGL (k_tsdf_surface_points, dim3 ((a.limit + BLOCK - 1u) / BLOCK), dim3 (BLOCK), 0, s, a);
}

// the output scratch of the first a.limit members
int reserve_records (icp_tsdf_context *t, tsdf_surface_args &a, bool normals)
{
    if (a.limit == 0u) return ICP_OK;
    int rc;
    if ((rc = icp_host::tsdf_reserve (t, &t->dEdge, &t->edge_cap, (size_t) a.limit * 4u))) return rc;
    if ((rc = icp_host::tsdf_reserve (t, &t->dOut, &t->out_cap, (size_t) a.limit * 32u))) return rc;
    if (normals && (rc = icp_host::tsdf_reserve (t, &t->dNrm, &t->nrm_cap, (size_t) a.limit * 16u))) return rc;
    a.edge = static_cast<uint32_t *> (t->dEdge); a.out = static_cast<float4 *> (t->dOut); a.nrm = normals ? static_cast<float4 *> (t->dNrm) : nullptr;
    return ICP_OK;
}

// the count of the volume's members on the host, and the output scratch for the first min (count, capacity) of them
int count_and_reserve (icp_tsdf_context *t, tsdf_surface_args &a, const surface_plan &p, uint32_t capacity, bool normals, uint32_t *total)
{
    launch_count_and_scan (a, p, t->stream);
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipMemcpyAsync (total, p.count, sizeof (uint32_t), hipMemcpyDeviceToHost, t->stream));
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    a.limit = std::min (*total, capacity);
    return reserve_records (t, a, normals);
}

// ---- a region's host side ---------------------------------------------------------------------------------------------------------------------

// the box on the device and the blocks [first_blk, first_blk + nb) of the sweep that can hold a member of the wanted kind
struct region_plan { tsdf_region_dev r; bool outside; uint32_t nb; };

// INSIDE: a member's low end lies in the box, so between the box's first and last voxel in linear order.  OUTSIDE: where the box spans x
// and y, the slices lo_z <= k < hi_z - 1 (and k = nz - 1 with them if hi_z = nz) hold INSIDE members only; if what is left is one run of
// slices at either end of the volume — what the kept box of a shift along z leaves — the sweep covers that run alone.
region_plan plan_region (const icp_tsdf_t &c, const icp_tsdf_region_t &g, const surface_plan &p)
{
    region_plan q {};
    for (int a = 0; a < 3; ++a) { q.r.lo[a] = g.lo[a]; q.r.hi[a] = g.hi[a]; }
    q.outside = g.mode == ICP_TSDF_REGION_OUTSIDE;
    const bool empty = g.lo[0] == g.hi[0] || g.lo[1] == g.hi[1] || g.lo[2] == g.hi[2];
    const uint32_t slice = c.nx * c.ny;
    uint32_t b0 = 0u, b1 = p.nblk;
    if (!q.outside) {
        if (empty) b1 = 0u;
        else {
            b0 = ((g.lo[2] * c.ny + g.lo[1]) * c.nx + g.lo[0]) / RUN;
            b1 = (((g.hi[2] - 1u) * c.ny + (g.hi[1] - 1u)) * c.nx + (g.hi[0] - 1u)) / RUN + 1u;
        }
    } else if (!empty && g.lo[0] == 0u && g.hi[0] == c.nx && g.lo[1] == 0u && g.hi[1] == c.ny) {
        const uint32_t in_end = g.hi[2] == c.nz ? c.nz : g.hi[2] - 1u;                // slices lo_z <= k < in_end hold no OUTSIDE member
        if (g.lo[2] == 0u && in_end == c.nz) b1 = 0u;                                // (the full box)
        else if (g.lo[2] == 0u) b0 = in_end * slice / RUN;
        else if (in_end == c.nz) b1 = (g.lo[2] * slice - 1u) / RUN + 1u;
    }
    q.r.first_blk = b0; q.nb = b1 - b0;
    return q;
}

// the count of the region's members and the position of every block's first one: the blocks the sweep leaves out count 0
hipError_t launch_region_count_and_scan (const tsdf_surface_args &a, const region_plan &q, const surface_plan &p, hipStream_t s)
{
    if (q.nb != p.nblk) {                           // (the wave counts and the block counts lie side by side: plan_surface)
        const hipError_t e = hipMemsetAsync (p.wave_cnt, 0, ((size_t) p.nblk * WAVES + p.nblk) * sizeof (uint32_t), s);
        if (e != hipSuccess) return e;
    }
    if (q.nb && q.outside) hipLaunchKernelGGL (k_tsdf_surface_count_region<true>, dim3 (q.nb), dim3 (BLOCK), 0, s, tsdf_region_args { a, q.r });
    else if (q.nb) hipLaunchKernelGGL (k_tsdf_surface_count_region<false>, dim3 (q.nb), dim3 (BLOCK), 0, s, tsdf_region_args { a, q.r });
    launch_scan (p, s);
    return hipSuccess;
}

int count_region_and_reserve (icp_tsdf_context *t, tsdf_surface_args &a, const region_plan &q, const surface_plan &p, uint32_t capacity, bool normals, uint32_t *total)
{
    TSDFCHK (t, launch_region_count_and_scan (a, q, p, t->stream));
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipMemcpyAsync (total, p.count, sizeof (uint32_t), hipMemcpyDeviceToHost, t->stream));
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    a.limit = std::min (*total, capacity);
    return reserve_records (t, a, normals);
}

const char *region_refusal (const icp_tsdf_t &c, const icp_tsdf_region_t &g)
{
    const uint32_t n[3] = { c.nx, c.ny, c.nz };
    for (int a = 0; a < 3; ++a) {
        if (g.lo[a] > g.hi[a]) return "lo must not exceed hi";
        if (g.hi[a] > n[a]) return "hi must not exceed the volume's size";
    }
    if (g.mode > 1u) return "mode must be ICP_TSDF_REGION_INSIDE or ICP_TSDF_REGION_OUTSIDE";
    return nullptr;
}

// ---- the mesh's host side --------------------------------------------------------------------------------------------------------------------

// The case table by its rule (include/icp_amd.h, "Mesh extraction": the case table; tests/tsdf_mesh_ref.py generates it again).
struct mesh_table { mask64 word[256]; };

void edge_ends (int e, int *c0, int *c1)
{
    const int a = e >> 2, m = e & 3, b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
    *c0 = ((m & 1) << b1) | ((m >> 1) << b2); *c1 = *c0 | (1 << a);
}

// the two faces 2 f + side of an edge as a mask of six bits
int edge_faces (int e)
{
    const int a = e >> 2, m = e & 3, b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
    return 1 << (2 * b1 + (m & 1)) | 1 << (2 * b2 + (m >> 1));
}

mesh_table make_mesh_table ()
{
    mesh_table T {};
    for (int cs = 0; cs < 256; ++cs) {
        int nb[12][2], nnb[12] = {}, c0, c1;
        bool cross[12];
        for (int e = 0; e < 12; ++e) { edge_ends (e, &c0, &c1); cross[e] = ((cs >> c0) ^ (cs >> c1)) & 1; }
        auto join = [&] (int x, int y) { nb[x][nnb[x]++] = y; nb[y][nnb[y]++] = x; };
        for (int face = 0; face < 6; ++face) {            // rule 2: the segments of a face
            int on[4], n_on = 0;
            for (int e = 0; e < 12; ++e) if (cross[e] && (edge_faces (e) >> face & 1)) on[n_on++] = e;
            if (n_on == 2) join (on[0], on[1]);
            if (n_on != 4) continue;
            for (int c = 0; c < 8; ++c) {                  // a positive corner of the face is cut off singly
                if (((c >> (face >> 1)) & 1) != (face & 1) || !((cs >> c) & 1)) continue;
                int pair[2], n_pair = 0;
                for (int q = 0; q < 4; ++q) { edge_ends (on[q], &c0, &c1); if (c0 == c || c1 == c) pair[n_pair++] = on[q]; }
                join (pair[0], pair[1]);
            }
        }
        mask64 word = 0ull;
        uint32_t n_tri = 0u;
        bool used[12] = {};
        for (int e0 = 0; e0 < 12; ++e0) {                  // rule 3: loops in ascending order of their smallest edge
            if (!cross[e0] || used[e0]) continue;
            int r[12], n = 0, prev = -1, cur = e0;
            r[n++] = e0;
            for (;;) {
                const int nxt = prev >= 0 && nb[cur][0] == prev ? nb[cur][1] : nb[cur][0];
                if (nxt == e0) break;
                prev = cur; cur = nxt; r[n++] = nxt;
            }
            // rule 4, in doubled coordinates: sum of P_i x P_i+1 against the sum of the edges' directions toward the positive end
            int area[3] = {}, up[3] = {}, P[12][3];
            for (int i = 0; i < n; ++i) {
                used[r[i]] = true;
                edge_ends (r[i], &c0, &c1);
                for (int b = 0; b < 3; ++b) P[i][b] = 2 * ((c0 >> b) & 1);
                P[i][r[i] >> 2] = 1;
                up[r[i] >> 2] += (cs >> c0) & 1 ? -1 : 1;
            }
            for (int i = 0; i < n; ++i) {
                const int *p = P[i], *q = P[(i + 1) % n];
                area[0] += p[1] * q[2] - p[2] * q[1]; area[1] += p[2] * q[0] - p[0] * q[2]; area[2] += p[0] * q[1] - p[1] * q[0];
            }
            if (area[0] * up[0] + area[1] * up[1] + area[2] * up[2] < 0) std::reverse (r + 1, r + n);
            int s = 0;                                     // rule 5: the first apex none of whose fan diagonals lies in a face
            for (; s < n; ++s) {
                bool ok = true;
                for (int i = 2; i + 1 < n; ++i) ok = ok && !(edge_faces (r[s]) & edge_faces (r[(s + i) % n]));
                if (ok) break;
            }
            for (int i = 1; i + 1 < n; ++i) {
                const int tri[3] = { r[s % n], r[(s + i) % n], r[(s + i + 1) % n] };
                for (int q = 0; q < 3; ++q) word |= (mask64) tri[q] << (4u + 4u * (3u * n_tri + q));
                ++n_tri;
            }
        }
        T.word[cs] = word | n_tri;
    }
    return T;
}

const mesh_table &mesh_cases () { static const mesh_table T = make_mesh_table (); return T; }

// The words of a mesh extraction's cell sweep in scratch of their own: a case byte per voxel, the wave counts, the block counts; their
// offsets inside their tiles, the tile sums, the tile offsets, the count.
struct mesh_plan {
    uint8_t *cases; uint2 *wave_cnt;
    uint32_t *blk_cnt, *blk_off, *tile_sum, *tile_off, *count;
};

int plan_mesh (icp_tsdf_context *t, const surface_plan &p, mesh_plan *q)
{
    if (!t->dMeshTab) {
        void *tab = nullptr;
        if (hipMalloc (&tab, sizeof (mesh_table)) != hipSuccess) { (void) hipGetLastError (); return icp_host::tsdf_fail (t, ICP_ENOMEM, "icp_tsdf_extract_mesh: the device cannot hold the case table"); }
        const hipError_t e = hipMemcpy (tab, mesh_cases ().word, sizeof (mesh_table), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void) hipFree (tab); return icp_host::tsdf_fail (t, ICP_EHIP, std::string ("icp_tsdf_extract_mesh: the case table: ") + hipGetErrorString (e)); }
        t->dMeshTab = tab;
    }
    const size_t units = (size_t) p.nblk * WAVES, words = 2u * (size_t) p.nblk + 2u * p.ntile + 1u;
    int rc = icp_host::tsdf_reserve (t, &t->dMesh, &t->mesh_cap, units * STEPS * 64u + units * sizeof (uint2) + words * sizeof (uint32_t)); if (rc) return rc;
    q->cases = static_cast<uint8_t *> (t->dMesh);
    q->wave_cnt = reinterpret_cast<uint2 *> (q->cases + units * STEPS * 64u);                 // (16-byte aligned: a block's case bytes are 1024)
    q->blk_cnt = reinterpret_cast<uint32_t *> (q->wave_cnt + units); q->blk_off = q->blk_cnt + p.nblk;
    q->tile_sum = q->blk_off + p.nblk; q->tile_off = q->tile_sum + p.ntile; q->count = q->tile_off + p.ntile;
    return ICP_OK;
}

tsdf_mesh_args mesh_args_of (const icp_tsdf_context *t, const tsdf_surface_args &m, const mesh_plan &q)
{
    tsdf_mesh_args a {};
    a.m = m; a.table = static_cast<const mask64 *> (t->dMeshTab);
    a.wave_cnt = q.wave_cnt; a.cases = q.cases; a.blk_cnt = q.blk_cnt; a.blk_off = q.blk_off; a.tile_off = q.tile_off;
    return a;
}

// the triangle count and the position of every block's first triangle
void launch_cells (const tsdf_mesh_args &a, const surface_plan &p, hipStream_t s)
{
    hipLaunchKernelGGL (k_tsdf_mesh_count, dim3 (p.nblk), dim3 (BLOCK), 0, s, a);
}

void launch_mesh_scan (const surface_plan &p, const mesh_plan &q, hipStream_t s)
{
    hipLaunchKernelGGL (k_tsdf_scan_tiles, dim3 (p.ntile), dim3 (BLOCK), 0, s, (const uint32_t *) q.blk_cnt, p.nblk, q.blk_off, q.tile_sum);
    hipLaunchKernelGGL (k_tsdf_scan_tiles, dim3 (1), dim3 (BLOCK), 0, s, (const uint32_t *) q.tile_sum, p.ntile, q.tile_off, q.count);
}

void launch_triangles (const tsdf_mesh_args &a, const surface_plan &p, hipStream_t s)
{
    hipLaunchKernelGGL (k_tsdf_mesh_triangles, dim3 (p.nblk), dim3 (BLOCK), 0, s, a);
}

// Both sweeps and their scans, both counts on the host in one round trip, and the output scratch for the first min (count, capacity) of
// each kind.  a.m.limit and a.limit are set.
int count_mesh_and_reserve (icp_tsdf_context *t, tsdf_mesh_args &a, const surface_plan &p, const mesh_plan &q, uint32_t vertex_capacity, bool normals,
                            uint32_t triangle_capacity, uint32_t *vertices, uint32_t *triangles)
{
    launch_count_and_scan (a.m, p, t->stream);
    launch_cells (a, p, t->stream);
    launch_mesh_scan (p, q, t->stream);
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipMemcpyAsync (vertices, p.count, sizeof (uint32_t), hipMemcpyDeviceToHost, t->stream));
    TSDFCHK (t, hipMemcpyAsync (triangles, q.count, sizeof (uint32_t), hipMemcpyDeviceToHost, t->stream));
    TSDFCHK (t, hipStreamSynchronize (t->stream));
    a.m.limit = std::min (*vertices, vertex_capacity);
    a.limit = std::min (*triangles, triangle_capacity);
    int rc = reserve_records (t, a.m, normals); if (rc) return rc;
    if (a.limit == 0u) return ICP_OK;
    if ((rc = icp_host::tsdf_reserve (t, &t->dTri, &t->tri_cap, (size_t) a.limit * 12u))) return rc;
    a.tri = static_cast<uint32_t *> (t->dTri);
    return ICP_OK;
}

// `reps` groups of launches between the volume's two events, after an untimed group
template <class G>
int time_groups (icp_tsdf_context *t, uint32_t reps, G group, float *us_per_group)
{
    group ();
    TSDFCHK (t, hipEventRecord (t->ev0, t->stream));
    for (uint32_t i = 0; i < reps; ++i) group ();
    TSDFCHK (t, hipEventRecord (t->ev1, t->stream));
    TSDFCHK (t, hipGetLastError ());
    TSDFCHK (t, hipEventSynchronize (t->ev1));
    float ms = 0.f;
    TSDFCHK (t, hipEventElapsedTime (&ms, t->ev0, t->ev1));
    *us_per_group = ms * 1e3f / (float) reps;
    return ICP_OK;
}

}  // namespace

namespace icp_host {

int tsdf_time_surface (icp_tsdf_context *t, int part, uint32_t reps, float *us_per_group)
{
    TSDFCHK (t, hipSetDevice (t->device));
    surface_plan p;
    int rc = plan_surface (t, &p); if (rc) return rc;
    tsdf_surface_args a = args_of (t, p, 1.f);
    uint32_t total = 0u;
    if ((rc = count_and_reserve (t, a, p, UINT32_MAX, true, &total))) return rc;      // (untimed: the code objects are loaded, the scratch holds every member)
    return time_groups (t, reps, [&] () {
        if (part == 1) { launch_scan (p, t->stream); return; }
        if (part != 2) launch_count_and_scan (a, p, t->stream);
        if (a.limit) launch_scatter (a, p, t->stream);
    }, us_per_group);
}

int tsdf_time_region (icp_tsdf_context *t, const int32_t *s, uint32_t reps, float *us_per_group)
{
    if (!s) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_time: what = 11 takes the three int32 of the shift through `depth`");
    icp_tsdf_region_t box;
    if (icp_tsdf_kept_box (&t->cfg, s, &box) != ICP_OK) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_time: the kept box");
    TSDFCHK (t, hipSetDevice (t->device));
    surface_plan p;
    int rc = plan_surface (t, &p); if (rc) return rc;
    const region_plan q = plan_region (t->cfg, box, p);
    tsdf_surface_args a = args_of (t, p, 1.f);
    uint32_t total = 0u;
    if ((rc = count_region_and_reserve (t, a, q, p, UINT32_MAX, true, &total))) return rc;      // (untimed, as above)
    return time_groups (t, reps, [&] () {
        (void) launch_region_count_and_scan (a, q, p, t->stream);
        if (a.limit) launch_scatter (a, p, t->stream);
    }, us_per_group);
}

int tsdf_time_mesh (icp_tsdf_context *t, int part, uint32_t reps, float *us_per_group)
{
    TSDFCHK (t, hipSetDevice (t->device));
    surface_plan p;
    mesh_plan q;
    int rc;
    if ((rc = plan_surface (t, &p)) || (rc = plan_mesh (t, p, &q))) return rc;
    tsdf_mesh_args a = mesh_args_of (t, args_of (t, p, 1.f), q);
    uint32_t vertices = 0u, triangles = 0u;
    if ((rc = count_mesh_and_reserve (t, a, p, q, UINT32_MAX, true, UINT32_MAX, &vertices, &triangles))) return rc;      // (untimed, as above)
    return time_groups (t, reps, [&] () {
        if (part == 0) launch_count_and_scan (a.m, p, t->stream);
        if (part != 2) launch_cells (a, p, t->stream);
        if (part == 0) {
            launch_mesh_scan (p, q, t->stream);
            if (a.m.limit) launch_scatter (a.m, p, t->stream);
        }
        if (part != 1 && a.limit) launch_triangles (a, p, t->stream);
    }, us_per_group);
}

}  // namespace icp_host

using namespace icp_host;

extern "C" {

int icp_tsdf_extract_surface (icp_tsdf_handle t, const icp_tsdf_surface_t *opt, uint32_t capacity, void *cloud_out, float *normals_out, uint32_t *count) try
{
    if (!t) return ICP_EINVAL;
    if (!count) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface: count is required");
    const icp_tsdf_surface_t o = opt ? *opt : icp_tsdf_surface_t { 1.f, 0u };
    if (!(std::isfinite (o.min_weight) && o.min_weight >= 1.f)) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface: min_weight must be finite and >= 1");
    if (o.normals > 1u) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface: normals must be 0 or 1");
    if (capacity && (!cloud_out || (o.normals && !normals_out)))
        return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface: with a capacity, cloud_out is required, and normals_out if normals are wanted");
    TSDFCHK (t, hipSetDevice (t->device));
    surface_plan p;
    int rc = plan_surface (t, &p); if (rc) return rc;
    tsdf_surface_args a = args_of (t, p, o.min_weight);
    uint32_t total = 0u;
    if ((rc = count_and_reserve (t, a, p, capacity, o.normals != 0u, &total))) return rc;
    if (a.limit) {
        launch_scatter (a, p, t->stream);
        TSDFCHK (t, hipGetLastError ());
        TSDFCHK (t, hipMemcpyAsync (cloud_out, t->dOut, (size_t) a.limit * 32u, hipMemcpyDeviceToHost, t->stream));
        if (a.nrm) TSDFCHK (t, hipMemcpyAsync (normals_out, t->dNrm, (size_t) a.limit * 16u, hipMemcpyDeviceToHost, t->stream));
        TSDFCHK (t, hipStreamSynchronize (t->stream));
    }
    *count = total;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_extract_surface_region (icp_tsdf_handle t, const icp_tsdf_surface_t *opt, const icp_tsdf_region_t *region, uint32_t capacity, void *cloud_out,
                                     float *normals_out, uint32_t *count) try
{
    if (!t) return ICP_EINVAL;
    if (!count) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface_region: count is required");
    if (!region) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface_region: region is required");
    const icp_tsdf_surface_t o = opt ? *opt : icp_tsdf_surface_t { 1.f, 0u };
    if (!(std::isfinite (o.min_weight) && o.min_weight >= 1.f)) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface_region: min_weight must be finite and >= 1");
    if (o.normals > 1u) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface_region: normals must be 0 or 1");
    if (capacity && (!cloud_out || (o.normals && !normals_out)))
        return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_surface_region: with a capacity, cloud_out is required, and normals_out if normals are wanted");
    if (const char *why = region_refusal (t->cfg, *region)) return tsdf_fail (t, ICP_EINVAL, std::string ("icp_tsdf_extract_surface_region: ") + why);
    TSDFCHK (t, hipSetDevice (t->device));
    surface_plan p;
    int rc = plan_surface (t, &p); if (rc) return rc;
    const region_plan q = plan_region (t->cfg, *region, p);
    tsdf_surface_args a = args_of (t, p, o.min_weight);
    uint32_t total = 0u;
    if ((rc = count_region_and_reserve (t, a, q, p, capacity, o.normals != 0u, &total))) return rc;
    if (a.limit) {
        launch_scatter (a, p, t->stream);
        TSDFCHK (t, hipGetLastError ());
        TSDFCHK (t, hipMemcpyAsync (cloud_out, t->dOut, (size_t) a.limit * 32u, hipMemcpyDeviceToHost, t->stream));
        if (a.nrm) TSDFCHK (t, hipMemcpyAsync (normals_out, t->dNrm, (size_t) a.limit * 16u, hipMemcpyDeviceToHost, t->stream));
        TSDFCHK (t, hipStreamSynchronize (t->stream));
    }
    *count = total;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_extract_mesh (icp_tsdf_handle t, const icp_tsdf_surface_t *opt, uint32_t vertex_capacity, void *cloud_out, float *normals_out, uint32_t *vertex_count,
                           uint32_t triangle_capacity, uint32_t *triangles_out, uint32_t *triangle_count) try
{
    if (!t) return ICP_EINVAL;
    if (!vertex_count || !triangle_count) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_mesh: vertex_count and triangle_count are required");
    const icp_tsdf_surface_t o = opt ? *opt : icp_tsdf_surface_t { 1.f, 0u };
    if (!(std::isfinite (o.min_weight) && o.min_weight >= 1.f)) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_mesh: min_weight must be finite and >= 1");
    if (o.normals > 1u) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_mesh: normals must be 0 or 1");
    if (vertex_capacity && (!cloud_out || (o.normals && !normals_out)))
        return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_mesh: with a vertex capacity, cloud_out is required, and normals_out if normals are wanted");
    if (triangle_capacity && !triangles_out) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_mesh: with a triangle capacity, triangles_out is required");
    if (5ull * (t->cfg.nx - 1u) * (t->cfg.ny - 1u) * (t->cfg.nz - 1u) > 0xFFFFFFFFull)
        return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_extract_mesh: five triangles a cell of this volume do not count in 32 bits");
    TSDFCHK (t, hipSetDevice (t->device));
    surface_plan p;
    mesh_plan q;
    int rc;
    if ((rc = plan_surface (t, &p)) || (rc = plan_mesh (t, p, &q))) return rc;
    tsdf_mesh_args a = mesh_args_of (t, args_of (t, p, o.min_weight), q);
    uint32_t vertices = 0u, triangles = 0u;
    if ((rc = count_mesh_and_reserve (t, a, p, q, vertex_capacity, o.normals != 0u, triangle_capacity, &vertices, &triangles))) return rc;
    if (a.m.limit || a.limit) {
        if (a.m.limit) launch_scatter (a.m, p, t->stream);
        if (a.limit) launch_triangles (a, p, t->stream);
        TSDFCHK (t, hipGetLastError ());
        if (a.m.limit) {
            TSDFCHK (t, hipMemcpyAsync (cloud_out, t->dOut, (size_t) a.m.limit * 32u, hipMemcpyDeviceToHost, t->stream));
            if (a.m.nrm) TSDFCHK (t, hipMemcpyAsync (normals_out, t->dNrm, (size_t) a.m.limit * 16u, hipMemcpyDeviceToHost, t->stream));
        }
        if (a.limit) TSDFCHK (t, hipMemcpyAsync (triangles_out, t->dTri, (size_t) a.limit * 12u, hipMemcpyDeviceToHost, t->stream));
        TSDFCHK (t, hipStreamSynchronize (t->stream));
    }
    *vertex_count = vertices; *triangle_count = triangles;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_tsdf_mesh_case (uint32_t case_index, uint32_t *n_triangles, uint8_t edges[15]) try
{
    if (case_index > 255u || !n_triangles || !edges) return ICP_EINVAL;
    const mask64 word = mesh_cases ().word[case_index];
    *n_triangles = (uint32_t) (word & 15ull);
    for (uint32_t q = 0; q < 15u; ++q) edges[q] = (uint8_t) ((word >> (4u + 4u * q)) & 15ull);      // (0 past the case's triangles)
    return ICP_OK;
}
ICP_CATCH_ALL

}  // extern "C"
