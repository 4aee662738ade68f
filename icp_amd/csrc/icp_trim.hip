// icp_trim.hip — trimmed ICP (icp_set_trimming, include/icp_amd.h): every iteration keeps the closest fraction ξ of the pairs that
// correspondence rejection leaves, and gives the rest the weight +0.
//
// An iteration with trimming on is (icp_route_of, icp_kernels.hip): the REJ search (icp_search_rej.hip), which stores its per-query
// outputs; the selection (icp_launch_trim_select: k_trim_select), which finds per registration n (the candidates), K = ceil (ξ n) and t,
// the K-th smallest key; the apply pass (icp_launch_trim_apply: k_trim_apply), which zeroes the weights of the pairs above t and rewrites
// the search blocks' partials in exactly the order the search wrote them; then the unchanged tail of the iteration
// (k_finalize_fused<ROT, true>, or k_means / k_sij / k_finalize).  A trimmed pair is then exactly a rejected pair, and the oracle's
// pieces with the trimmed rows zeroed give the same bits.  None of the existing kernels carries any of this code.
//
// The key of a pair and the apply pass are in icp_trim_apply.h (a point-to-point robust loss instantiates the pass in icp_robust.hip).
// The pass also runs with trimming off, behind the pair filter or one-to-one correspondences on point-to-point: it then accepts every
// candidate they left and reads none of trimming's words.
//
// The selection is the radix select of icp_select.h at the rank K = ceil (ξ n), in the words of ICP_AREA_TRIM: up to
// ICP_TRIM_ONE_BLOCK_MAX pairs per registration one workgroup with the keys in registers (k_trim_select, grid.y = registration), beyond
// it three launches of many workgroups (k_trim_select_pass<D>).  Both take the same t: the K-th smallest key is one number.
#include "icp_select.h"                 // (the digit helpers, trim_pick, block_sum, select_pass; TRIM_NONE, trim_key, trim_apply)

namespace {

// K = ceil (ξ n) (ξ n is exact in double: a float times an integer below 2^21)
__device__ __forceinline__ uint32_t trim_rank (float keep, uint32_t n)
{
    return min ((uint32_t) ceil ((double) keep * (double) n), n);
}

// the rule's words for the selection: out = (t bits, n, K, accepted)
struct trim_rule {
    float keep;
    __device__ __forceinline__ uint32_t rank (uint32_t n) const { return trim_rank (keep, n); }
    __device__ __forceinline__ void first (uint32_t *out, uint32_t n, uint32_t K) const { out[1] = n; out[2] = K; }
    __device__ __forceinline__ void last (uint32_t *out, uint32_t t, uint32_t below, uint32_t at) const { out[0] = t; out[3] = below + at; }
};

// ------------------------------------------------------------------------------------------
// k_trim_select — one workgroup per registration (m <= ICP_TRIM_ONE_BLOCK_MAX): 16 keys per thread in registers, three passes.
// The digit loop is select_digits' (icp_select.h), written out: calling it here costs 0.1 - 0.2 us per iteration (profiles/select_ab.txt).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (1024) void k_trim_select (icp_params p, uint32_t *area)
{
    constexpr int NT = 1024, KPT = (int) ICP_TRIM_ONE_BLOCK_MAX / NT;
    __shared__ uint32_t s_hist[ICP_TRIM_BINS], s_wsum[NT / 64], s_pick[3];
    const uint32_t b = blockIdx.y, t = threadIdx.x, m = p.m;
    if (icp_pass_leaves (p, b)) return;
    const trim_rule rule = { p.trim_keep };
    const float4 *PF = p.PF + (size_t) b * m, *PM = p.PM + (size_t) b * m;
    uint32_t key[KPT], cnt = 0u;
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const uint32_t i = t + (uint32_t) (NT * k);
        key[k] = i < m ? trim_key (PF[i], PM[i]) : TRIM_NONE;
        cnt += key[k] != TRIM_NONE ? 1u : 0u;
    }
    const uint32_t n = block_sum<NT> (cnt, s_wsum), K = rule.rank (n);
    uint32_t *out = area + 4u * b;
    if (n == 0u) {                                           // nothing to keep: k_trim_apply trims every pair
        if (t == 0u) { out[0] = 0u; out[1] = 0u; out[2] = 0u; out[3] = 0u; }
        return;
    }
    uint32_t prefix = 0u, kk = K, below = 0u, at = 0u;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        for (uint32_t j = t; j < ICP_TRIM_BINS; j += NT) s_hist[j] = 0u;
        __syncthreads ();
#pragma unroll
        for (int k = 0; k < KPT; ++k)
            if (trim_match (key[k], prefix, d)) atomicAdd (&s_hist[trim_digit (key[k], d)], 1u);
        __syncthreads ();
        trim_pick<NT> (s_hist, kk, s_wsum, s_pick);
        const uint32_t j = s_pick[0], lo = s_pick[1];
        at = s_pick[2];
        prefix |= j << trim_shift (d); kk -= lo; below += lo;
        __syncthreads ();                                    // (s_pick and s_hist are written again by the next pass)
    }
    if (t == 0u) { rule.first (out, n, K); rule.last (out, prefix, below, at); }
}

// ------------------------------------------------------------------------------------------
// k_trim_select_pass<D> — pass D of the selection of large sets (select_pass, icp_select.h), in the words of trimming's area
// ------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__ (256) void k_trim_select_pass (icp_params p, uint32_t *area)
{
    const uint32_t b = blockIdx.y, t = threadIdx.x;
    if (icp_pass_leaves (p, b)) return;
    select_pass<D> (p, b, t, icp_select_words_of (area, icp_area_desc_of (ICP_AREA_TRIM), p.batch, b, p.m), trim_rule { p.trim_keep });
}

// the apply pass with the loss off (icp_trim_apply.h)
template <bool FUSED>
__global__ __launch_bounds__ (64) void k_trim_apply (icp_params p, const uint32_t *area, uint32_t tpr_magic)
{
    trim_apply<FUSED, false> (p, area, tpr_magic);
}

}  // namespace

// the selection: one workgroup's up to ICP_TRIM_ONE_BLOCK_MAX pairs per registration, three multi-workgroup passes beyond (launches: icp_route::select)
void icp_launch_trim_select (const icp_params &p, hipStream_t s, uint32_t launches)
{
    uint32_t *area = icp_words (p, ICP_AREA_TRIM).result;
    if (launches == 1u) { hipLaunchKernelGGL (k_trim_select, dim3 (1, p.batch), dim3 (1024), 0, s, p, area); return; }
    const dim3 grid ((p.m + 2047u) / 2048u, p.batch);
    hipLaunchKernelGGL (k_trim_select_pass<0>, grid, dim3 (256), 0, s, p, area);
    hipLaunchKernelGGL (k_trim_select_pass<1>, grid, dim3 (256), 0, s, p, area);
    hipLaunchKernelGGL (k_trim_select_pass<2>, grid, dim3 (256), 0, s, p, area);
}

void icp_launch_trim_apply (const icp_params &p, hipStream_t s)
{
    const uint32_t *area = icp_words (p, ICP_AREA_TRIM).result;
    if (p.fused) hipLaunchKernelGGL (k_trim_apply<true>, dim3 (p.nb, p.batch), dim3 (64), 0, s, p, area, icp_tpr_magic (p.side));
    else hipLaunchKernelGGL (k_trim_apply<false>, dim3 (2 * p.nwg, p.batch), dim3 (64), 0, s, p, area, icp_tpr_magic (p.side));
}
