// icp_projective.hip — projective data association (icp_set_projective, include/icp_amd.h): a second way to FIND the pairs.  The fixed set is
// read as a row-major grid gw wide; a moving point is transformed, projected through the fixed frame's pinhole model (fx, fy, cx, cy, in
// grid units) onto that grid, and paired with the closest valid fixed point of the (2 r + 1)^2 window around the cell it lands on.  O (1)
// per query, no search structure: k_projective stands where the RBC search stands in a route (icp_route::projective, icp_kernels.hip) and
// every pass behind the search and every tail stay what they are.
//
// The rule per query i, T = p.st[b].T (only the tail of an iteration changes it):
//   e = icp_transform_point (T, M[i].xyz); QT[i] = (e, d) for every i < m, d = +inf for a miss.
//   The query counts iff M[i].xyz is finite and not (0, 0, 0) (icp_pair_counted).
//   In double from the float inputs, every expression in the order written (the translation unit is built with -ffp-contract=off):
//       u = (double) fx * ((double) e.x / (double) e.z) + (double) cx,  v likewise with fy, e.y, cy;  pu = floor (u + 0.5), pv = floor (v + 0.5).
//   Inside iff it counts, e is finite, e.z > 0, 0 <= pu <= gw - 1 and 0 <= pv <= rows - 1, compared in double (a NaN fails).
//   Candidates: the window's cells j = y gw + x (columns max (0, pu - r) .. min (gw - 1, pu + r), rows likewise) whose F[j].xyz is finite
//   and not (0, 0, 0); d_j = icp_metric8 (e, M[i].rgb; F[j].xyz, F[j].rgb; alpha).  The winner is the candidate with the smallest
//   d_j < +inf, compared as floats (a negative alpha makes negative distances; a NaN or +inf never wins), a tie to the smallest j: what a
//   scan of the window in ascending j that starts from +inf and updates on a strict '<' keeps.
//   Hit: d = dist_scale d_j, NN_ID[i] = {d, j}, NN[i] = (F[j].xyz, w), w = weighted ? 100 / (100 + d) : 1 — and +0 where
//   icp_set_rejection's distance test rejects the pair, which keeps its record as behind the RBC search.
//   Miss (not counting, not inside, no winner): NN_ID[i] = {+inf, 0xFFFFFFFF}, NN[i] = (0, 0, 0, +0): exactly a rejected pair.
// The kernel writes the per-query outputs and the count words and nothing else: the block partials (moments, or the weight partials of the
// reference-order reductions) come from the apply pass behind it (icp_trim_apply.h), the plane metrics read the outputs in their moments.
// ICP_MEM_RID is left as it is: a later RBC search seeds its pruning from it, any content is a valid seed (pruning is exact).
//
// The obligations of a separate-form search (icp_search.h, the prologue of k_search): block 0 publishes the progress word of a host-driven
// checked run — not for a converged registration in fused mode, whose finalize has published DONE | FINAL itself —, a converged
// registration of a checked run is left alone, batched registrations are indexed by blockIdx.y.
//
// Layout: one thread per query, whatever the radius (it is a device word: a new radius touches no graph, so no launch decision may depend
// on it).  The thread walks its window in row-major order; at every step the lanes of a wave — neighbouring queries, which project to
// neighbouring cells — read neighbouring 32-byte records of F, so a wave's loads are as contiguous with the window walked by one lane as
// with the window spread over a lane group, and the gather lives in L2.  float4 loads of M and of the two halves of F[j].
//
// Counting (ICP_MEM_PROJECTIVE: n, hits, outside, empty; hits + outside + empty == n): this kernel has no launch in front of it that
// could reset the words, so its blocks count by ticket (pair_counts_ticket, icp_pair_rule.h, which has the measurements).  A block of
// 256 threads serves 1024 queries in four rounds at the sizes where the number of tickets matters, 256 where the grid would otherwise
// not fill the chip; a wave accumulates its counts over the rounds.
#include "icp_search.h"                 // (icp_mirror_store)
#include "icp_pair_rule.h"

namespace {

constexpr uint32_t PROJ_BLOCK = 256u;
constexpr uint32_t PROJ_NONE = 0xFFFFFFFFu;

// ------------------------------------------------------------------------------------------
// k_projective — one thread per query, 256 queries per round, `rounds` rounds per block; grid (ceil (m / (256 rounds)), batch).
// result, counts, settings: icp_words (p, ICP_AREA_PROJECTIVE) (icp_kernels.h); settings = (gw, fx, fy, cx, cy, r)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (PROJ_BLOCK) void k_projective (icp_params p, uint32_t rounds, uint32_t *result, uint32_t *counts, const uint32_t *settings)
{
    const uint32_t b = blockIdx.y, t = threadIdx.x, m = p.m;
    const icp_reg_state *st = p.st + b;
    const uint32_t done = st->done;
    if (p.hmirror && blockIdx.x == 0u && t == 0u && !(p.fused && done)) icp_mirror_store (p.hmirror + b, ICP_MIRROR_WORD (p.epoch, st->k, done));
    if (p.check && done) return;                             // (icp_pass_leaves, with the one load of `done` above)
    float T[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) T[k] = st->T[k];
    uint32_t gw = settings[0];
    const double fx = (double) __uint_as_float (settings[1]), fy = (double) __uint_as_float (settings[2]);
    const double cx = (double) __uint_as_float (settings[3]), cy = (double) __uint_as_float (settings[4]);
    const uint32_t r = min (settings[5], 8u);
    // (the host refuses a width that does not divide m; whatever the words hold, every index below stays inside the registration's m rows:
    // a width of 0 or beyond m makes every query a miss, and rows gw <= m)
    if (gw > m) gw = 0u;
    const uint32_t rows = gw ? m / gw : 0u;
    const size_t o = (size_t) b * m;
    const float4 *F4 = reinterpret_cast<const float4 *> (p.F) + o * 2u, *M4 = reinterpret_cast<const float4 *> (p.M) + o * 2u;
    uint32_t cn = 0u, ch = 0u, co = 0u;                      // this wave's counts over the rounds
    for (uint32_t rd = 0; rd < rounds; ++rd) {
        const uint32_t i = (blockIdx.x * rounds + rd) * PROJ_BLOCK + t;
        const bool v = i < m;
        float4 mg = make_float4 (0.f, 0.f, 0.f, 0.f), mc = mg;
        if (v) { mg = M4[2u * (size_t) i]; mc = M4[2u * (size_t) i + 1u]; }
        const bool counts_ = icp_pair_counted (v, mg);
        float ex, ey, ez;
        icp_transform_point (T, mg.x, mg.y, mg.z, ex, ey, ez);
        const double u = fx * ((double) ex / (double) ez) + cx, w_ = fy * ((double) ey / (double) ez) + cy;
        const double pu = floor (u + 0.5), pv = floor (w_ + 0.5);
        const bool inside = counts_ && gw != 0u && isfinite (ex) && isfinite (ey) && isfinite (ez) && (double) ez > 0.0
                            && pu >= 0.0 && pu <= (double) (gw - 1u) && pv >= 0.0 && pv <= (double) (rows - 1u);
        float best = __builtin_inff (); uint32_t bj = PROJ_NONE;
        if (inside) {
            // (0 <= pu <= gw - 1 and 0 <= pv <= rows - 1: the conversions are exact, and every cell (x, y) below has y gw + x < rows gw <= m)
            const uint32_t ux = (uint32_t) pu, uy = (uint32_t) pv;
            const uint32_t x0 = ux >= r ? ux - r : 0u, x1 = min (gw - 1u, ux + r), y0 = uy >= r ? uy - r : 0u, y1 = min (rows - 1u, uy + r);
            for (uint32_t y = y0; y <= y1; ++y)
                for (uint32_t x = x0; x <= x1; ++x) {
                    const uint32_t j = y * gw + x;
                    const float4 fg = F4[2u * (size_t) j], fc = F4[2u * (size_t) j + 1u];
                    const float d = icp_metric8 (ex, ey, ez, mc.x, mc.y, mc.z, fg.x, fg.y, fg.z, fc.x, fc.y, fc.z, p.a);
                    // (the thread's cells ascend: a strict '<' from +inf keeps the smallest j among equal distances, and a NaN or +inf never wins)
                    if (icp_point_valid (fg) && d < best) { best = d; bj = j; }
                }
        }
        const bool hit = inside && bj != PROJ_NONE;
        if (v) {
            icp_dist_id di; di.dist = __builtin_inff (); di.id = PROJ_NONE;
            float4 pf = make_float4 (0.f, 0.f, 0.f, 0.f);
            if (hit) {
                const uint32_t j = bj;
                const float4 fg = F4[2u * (size_t) j];       // (j < m: a cell of the window)
                const float d = p.dist_scale * best;
                float w = p.weighted ? 100.f / (100.f + d) : 1.f;
                if (p.reject & ICP_REJECT_DIST_ON) {         // (icp_set_rejection's distance test, as the REJ search's epilogue applies it:
                    // icp_pair_geo of e - fg, written out — through the helper the compiler branches where it selects here: profiles/pair_pass_isa_diff.txt)
                    const float gx = ex - fg.x, gy = ey - fg.y, gz = ez - fg.z;
                    if (!(((gx * gx + gy * gy) + gz * gz) <= p.reject_d2)) w = 0.f;
                }
                di.dist = d; di.id = j;
                pf = make_float4 (fg.x, fg.y, fg.z, w);
            }
            p.nn_id[o + i] = di;
            p.PF[o + i] = pf;
            p.PM[o + i] = make_float4 (ex, ey, ez, di.dist);
        }
        cn += (uint32_t) __popcll (__ballot (counts_));
        ch += (uint32_t) __popcll (__ballot (hit));
        co += (uint32_t) __popcll (__ballot (counts_ && !inside));
    }
    const uint32_t wave[3] = { cn, ch, co };
    uint32_t sum[3];
    if (pair_block_counts<3, PROJ_BLOCK> (wave, sum)) pair_counts_ticket (counts + 8u * b, result + 4u * b, sum[0], sum[1], sum[2], gridDim.x);
}

}  // namespace

void icp_launch_projective (const icp_params &p, hipStream_t s)
{
    // queries per block: 1024 where a registration's tickets would be many (see the header), else one round's worth
    const uint32_t rounds = (size_t) p.batch * p.m > 65536u ? 4u : 1u, per_block = rounds * PROJ_BLOCK;
    const dim3 grid ((p.m + per_block - 1u) / per_block, p.batch);
    const icp_area_words w = icp_words (p, ICP_AREA_PROJECTIVE);
    hipLaunchKernelGGL (k_projective, grid, dim3 (PROJ_BLOCK), 0, s, p, rounds, w.result, w.running, (const uint32_t *) w.settings);
}
