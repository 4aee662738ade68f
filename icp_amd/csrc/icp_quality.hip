// icp_quality.hip — registration quality on the device (icp_evaluate; include/icp_amd.h states the rule): fitness, inlier RMSE and the
// 6 x 6 information matrix of a registration at its current transform.
//
// icp_evaluate (icp_capi.hip) runs one search of M against the RBC at the registration's state, with the per-query outputs pointed at the
// evaluation's own buffers, then the two kernels here: k_quality_pairs, the 22 terms of every pair in double and their tree over blocks
// of ICP_P2PL_BLOCK pairs, plus the block's two counts; k_quality_finish, one workgroup per registration: the tree over the block
// partials and the sum of the counts.  Nothing an iteration reads or writes is touched, and no iteration kernel carries any of this
// code.  The translation unit is built with -ffp-contract=off like every other: each expression is evaluated in the order it is written;
// tests/quality_ref.py restates them.
//
// Pair i, with e = PM[i].xyz (the transformed moving point), f = PF[i].xyz (the returned fixed point), mv = M[i].xyz:
//   counted, geo, inlier: icp_pair_counted, icp_pair_geo, icp_pair_inlier (icp_pair_rule.h; icp_correspondences' set is made of the same inliers); n_moving counts the
//   counted pairs, n_inliers the inliers
//   terms 0 .. 20: G about the point Q = f in double (plane_point_share: [[qq I - Q Q^T, [Q]x], [-[Q]x, I]], upper triangle, row-major);
//   term 21: (double) geo.  A pair that is no inlier leaves exact zeros (selected: a NaN coordinate makes no NaN).
#include "icp_plane_moments.h"          // (plane_point_share, plane_block_tree)
#include "icp_pair_rule.h"

__global__ __launch_bounds__ (256) void k_quality_pairs (const float4 *PF, const float4 *PM, const float *M, uint32_t m, uint32_t dist_on, float d2,
                                                         double *part, uint32_t *cnt, uint32_t nblk)
{
    const uint32_t b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * ICP_P2PL_BLOCK + tid;
    const size_t o = (size_t) b * m;
    const uint32_t ic = min (i, m - 1u);
    const float4 f = PF[o + ic], e = PM[o + ic];
    const float4 mv = *reinterpret_cast<const float4 *> (M + (o + ic) * 8);
    __shared__ uint32_t s_cnt[2][ICP_P2PL_BLOCK / 64u];
    const bool counted = icp_pair_counted (i < m, mv);
    const float geo = icp_pair_geo (f, e);
    const bool inlier = icp_pair_inlier (counted, f, geo, dist_on, d2);
    double v[ICP_QUALITY_TERMS];
#pragma unroll
    for (int t = 0; t < (int) ICP_QUALITY_TERMS; ++t) v[t] = 0.0;
    if (inlier) {
        const plane_share S = plane_point_share ((double) f.x, (double) f.y, (double) f.z, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
#pragma unroll
        for (int t = 0; t < 21; ++t) v[t] = S.G[t];
        v[21] = (double) geo;
    }
    // the block's counts: a popcount per wave (integers: any order gives the same sum)
    const unsigned long long bm = __ballot (counted), bi = __ballot (inlier);
    if ((tid & 63u) == 0u) { s_cnt[0][tid >> 6] = (uint32_t) __popcll (bm); s_cnt[1][tid >> 6] = (uint32_t) __popcll (bi); }
    plane_block_tree (v, part, nblk, b);                 // (its barriers stand between the waves' counts and their sum below)
    if (tid < 2u) cnt[((size_t) b * 2 + tid) * nblk + blockIdx.x] = (s_cnt[tid][0] + s_cnt[tid][1]) + (s_cnt[tid][2] + s_cnt[tid][3]);
}

#define QUALITY_LDS 4096u        // doubles of the second level's tree buffer (nblk <= 4096: m <= 2^20)

// One workgroup per registration: the halving tree over the block partials zero-padded to P = 2^ceil(log2 nblk), as many terms at a
// time as the LDS buffer holds (k_p2pl_finalize's tree), and the sum of the blocks' counts.  res: ICP_QUALITY_RES doubles per
// registration — the 22 sums, then (n_moving, n_inliers) as two uint32.
__global__ __launch_bounds__ (256) void k_quality_finish (const double *part, const uint32_t *cnt, double *res, uint32_t nblk, uint32_t P)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    __shared__ double s[QUALITY_LDS];
    __shared__ uint32_t s_cnt[2];
    const uint32_t lgP = 31u - (uint32_t) __builtin_clz (P), tc = min (ICP_QUALITY_TERMS, QUALITY_LDS / P);
    const double *pb = part + (size_t) b * ICP_QUALITY_TERMS * nblk;
    double *rb = res + (size_t) b * ICP_QUALITY_RES;
    if (tid < 2u) s_cnt[tid] = 0u;
    for (uint32_t t0 = 0; t0 < ICP_QUALITY_TERMS; t0 += tc) {
        const uint32_t nt = min (tc, ICP_QUALITY_TERMS - t0), n = nt << lgP;          // (n <= QUALITY_LDS)
        for (uint32_t j = tid; j < n; j += 256u) {
            const uint32_t t = j >> lgP, i = j & (P - 1u);
            s[j] = i < nblk ? pb[(size_t) (t0 + t) * nblk + i] : 0.0;
        }
        __syncthreads ();
        for (uint32_t lh = lgP; lh-- > 0u;) {
            const uint32_t h = 1u << lh;
            for (uint32_t j = tid; j < (nt << lh); j += 256u) {
                const uint32_t t = j >> lh, i = j & (h - 1u);
                s[(t << lgP) + i] = s[(t << lgP) + i] + s[(t << lgP) + i + h];
            }
            __syncthreads ();
        }
        if (tid < nt) rb[t0 + tid] = s[tid << lgP];
        __syncthreads ();
    }
    uint32_t c0 = 0u, c1 = 0u;
    for (uint32_t i = tid; i < nblk; i += 256u) { c0 += cnt[((size_t) b * 2 + 0) * nblk + i]; c1 += cnt[((size_t) b * 2 + 1) * nblk + i]; }
    atomicAdd (&s_cnt[0], c0); atomicAdd (&s_cnt[1], c1);
    __syncthreads ();
    if (tid < 2u) reinterpret_cast<uint32_t *> (rb + ICP_QUALITY_TERMS)[tid] = s_cnt[tid];
}

void icp_launch_quality (const float4 *PF, const float4 *PM, const float *M, uint32_t m, uint32_t batch, bool dist_on, float d2, double *part, uint32_t *cnt,
                         double *res, hipStream_t s)
{
    const uint32_t nblk = icp_p2pl_nblk (m);
    uint32_t P = 1u; while (P < nblk) P <<= 1;
    hipLaunchKernelGGL (k_quality_pairs, dim3 (nblk, batch), dim3 (ICP_P2PL_BLOCK), 0, s, PF, PM, M, m, dist_on ? 1u : 0u, d2, part, cnt, nblk);
    hipLaunchKernelGGL (k_quality_finish, dim3 (batch), dim3 (256), 0, s, (const double *) part, (const uint32_t *) cnt, res, nblk, P);
}
