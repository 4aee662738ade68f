// icp_pairs.hip — the correspondence set of a registration on the device (icp_correspondences; include/icp_amd.h states the rule): the
// member pairs of a search as one compact list of 16-byte records in ascending query index, and their number.
//
// An ordered stream compaction in two launches over blocks of ICP_P2PL_BLOCK consecutive pairs, grid (nblk, batch):
//   k_pairs_count    every wave counts its members with a ballot and a popcount, the block stores the sum of its four waves.
//   k_pairs_scatter  every block sums the counts of the blocks of its registration in front of it (nblk <= 4096: at most 16 loads per
//                    thread), judges its pairs again, and member i goes to position
//                        (members in the blocks in front) + (members in the waves of the block in front) + (members below the lane),
//                    the last term the ballot's bits below the lane (mbcnt).  The last block stores the registration's count.
// Nothing waits for another workgroup inside a launch: the order between the two passes is the stream's.  The counts are integer sums
// and a position is a function of the predicate alone: no atomics on positions, and the result does not depend on the launch shape.
// A member is one 16-byte store; the positions of a block's members are consecutive, so the stores of a block are contiguous.
//
// The predicate, by source:
//   ICP_PAIRS_EVALUATED (0)       icp_pair_inlier (icp_pair_rule.h: the expression k_quality_pairs counts n_inliers with), from
//                                 the evaluation's PF / PM and M; fixed = the evaluation's id, weight = 1.0f.
//   ICP_PAIRS_LAST_ITERATION (1)  PF[i].w != 0.f, the weight the last iteration left (a float comparison: a NaN is a member, -0 is
//                                 none); fixed = ICP_MEM_NN_ID[i].id, weight = PF[i].w.  M is not read.
// geo is icp_pair_geo of both: (gx gx + gy gy) + gz gz in fp32, g = PM.xyz - PF.xyz; the translation unit is built with
// -ffp-contract=off like every other.  tests/pairs_ref.py restates both sets.
#include "icp_kernels.h"
#include "icp_pair_rule.h"

namespace {

struct pair_record { bool member; uint4 rec; };

// pair i of registration b as a record (loads at i clamped to the last pair: a lane past the end is no member)
template <int SOURCE>
__device__ __forceinline__ pair_record pair_of (const float4 *PF, const float4 *PM, const float *M, const icp_dist_id *nn_id, uint32_t m, uint32_t b, uint32_t i,
                                                uint32_t dist_on, float d2)
{
    const size_t o = (size_t) b * m + min (i, m - 1u);
    const float4 f = PF[o], e = PM[o];
    pair_record r;
    float geo, w;
    if (SOURCE == 0) {
        const float4 mv = *reinterpret_cast<const float4 *> (M + o * 8);
        geo = icp_pair_geo (f, e); w = 1.f;
        r.member = icp_pair_inlier (icp_pair_counted (i < m, mv), f, geo, dist_on, d2);
    } else {
        r.member = i < m && f.w != 0.f; geo = icp_pair_geo (f, e); w = f.w;
    }
    r.rec = make_uint4 (i, nn_id[o].id, __float_as_uint (geo), __float_as_uint (w));
    return r;
}

template <int SOURCE>
__global__ __launch_bounds__ (ICP_P2PL_BLOCK) void k_pairs_count (const float4 *PF, const float4 *PM, const float *M, const icp_dist_id *nn_id, uint32_t m,
                                                                  uint32_t dist_on, float d2, uint32_t *blk_cnt, uint32_t nblk)
{
    const uint32_t b = blockIdx.y, tid = threadIdx.x;
    __shared__ uint32_t s_wave[ICP_P2PL_BLOCK / 64u];
    const pair_record r = pair_of<SOURCE> (PF, PM, M, nn_id, m, b, blockIdx.x * ICP_P2PL_BLOCK + tid, dist_on, d2);
    const unsigned long long bal = __ballot (r.member);
    if ((tid & 63u) == 0u) s_wave[tid >> 6] = (uint32_t) __popcll (bal);
    __syncthreads ();
    if (tid == 0u) blk_cnt[(size_t) b * nblk + blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

template <int SOURCE>
__global__ __launch_bounds__ (ICP_P2PL_BLOCK) void k_pairs_scatter (const float4 *PF, const float4 *PM, const float *M, const icp_dist_id *nn_id, uint32_t m,
                                                                    uint32_t dist_on, float d2, const uint32_t *blk_cnt, uint32_t nblk, uint4 *pairs, uint32_t *count)
{
    const uint32_t b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    __shared__ uint32_t s_wave[ICP_P2PL_BLOCK / 64u], s_front;
    if (tid == 0u) s_front = 0u;
    const pair_record r = pair_of<SOURCE> (PF, PM, M, nn_id, m, b, blockIdx.x * ICP_P2PL_BLOCK + tid, dist_on, d2);
    const unsigned long long bal = __ballot (r.member);
    if ((tid & 63u) == 0u) s_wave[wave] = (uint32_t) __popcll (bal);
    uint32_t c = 0u;                                     // the members in the blocks in front (integers: any order gives the same sum)
    for (uint32_t j = tid; j < blockIdx.x; j += ICP_P2PL_BLOCK) c += blk_cnt[(size_t) b * nblk + j];
    __syncthreads ();
    if (c) atomicAdd (&s_front, c);
    __syncthreads ();
    uint32_t base = s_front;
    for (uint32_t w = 0; w < wave; ++w) base += s_wave[w];
    const uint32_t below = __builtin_amdgcn_mbcnt_hi ((uint32_t) (bal >> 32), __builtin_amdgcn_mbcnt_lo ((uint32_t) bal, 0u));
    if (r.member) pairs[(size_t) b * m + base + below] = r.rec;       // (base + below <= the pair's own index < m)
    if (blockIdx.x == nblk - 1u && tid == ICP_P2PL_BLOCK - 1u) count[b] = base + s_wave[wave];
}

template <int SOURCE>
void launch_pairs (const float4 *PF, const float4 *PM, const float *M, const icp_dist_id *nn_id, uint32_t m, uint32_t batch, uint32_t dist_on, float d2,
                   uint32_t *blk_cnt, uint4 *pairs, uint32_t *count, hipStream_t s)
{
    const uint32_t nblk = icp_p2pl_nblk (m);
    hipLaunchKernelGGL (k_pairs_count<SOURCE>, dim3 (nblk, batch), dim3 (ICP_P2PL_BLOCK), 0, s, PF, PM, M, nn_id, m, dist_on, d2, blk_cnt, nblk);
    hipLaunchKernelGGL (k_pairs_scatter<SOURCE>, dim3 (nblk, batch), dim3 (ICP_P2PL_BLOCK), 0, s, PF, PM, M, nn_id, m, dist_on, d2, (const uint32_t *) blk_cnt, nblk,
                        pairs, count);
}

}  // namespace

void icp_launch_pairs (int source, const float4 *PF, const float4 *PM, const float *M, const icp_dist_id *nn_id, uint32_t m, uint32_t batch, bool dist_on, float d2,
                       uint32_t *blk_cnt, uint4 *pairs, uint32_t *count, hipStream_t s)
{
    if (source == 0) launch_pairs<0> (PF, PM, M, nn_id, m, batch, dist_on ? 1u : 0u, d2, blk_cnt, pairs, count, s);
    else launch_pairs<1> (PF, PM, M, nn_id, m, batch, 0u, 0.f, blk_cnt, pairs, count, s);
}
