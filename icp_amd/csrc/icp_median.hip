// icp_median.hip — median-distance rejection (icp_set_median_rejection, include/icp_amd.h): every iteration rejects the candidate pairs
// that lie farther apart than factor times the median pair distance of that iteration — geo > thr, thr = factor^2 t_med, t_med the lower
// median of the candidates' geo — and gives them the weight +0.  A pair the rule rejects is then exactly a rejected pair.
//
// An iteration with the rule on is (icp_route_of, icp_kernels.hip): the REJ search (icp_search_rej.hip) or k_projective, which store the
// per-query outputs; the pair filter, the reciprocal rule and one-to-one, where they are on; this rule; trimming's selection, whose
// candidates are the pairs this rule accepts; the apply pass (point-to-point: it writes the search blocks' partials again from the
// weights; the plane metrics read the weights in their moments); the unchanged tail.  None of the existing kernels carries any of this code.
//
// The median is the radix select of icp_select.h at the rank K = (n + 1) / 2.  Up to ICP_TRIM_ONE_BLOCK_MAX pairs per registration one
// workgroup does everything in one launch with the keys in registers (k_median): the count, the three digit passes, the threshold, the
// rejection of its own pairs, the accepted count, the four words.  Beyond it: the three multi-workgroup passes (k_median_select_pass<D>),
// whose last workgroup leaves t_med and thr and zeroes the accepted word, and one pass over the stored keys that rejects and counts
// (k_median_reject: pair_counts_add, a launch stands in front that resets the word).
//
// Determinism: the median is one number — the K-th smallest of a set —, the threshold a function of it, and the counts are integer sums.
// Nothing depends on the order of arrival.
//
// The rule's words are no part of icp_params or of the moments' allocation: they are an allocation of their own on the handle
// (a selection's words with two settings, the factor and a word of padding: icp_median_desc, icp_kernels.h) and reach the kernels as an
// argument.  Result words of a registration: (t_med bits, n, thr bits, accepted), ICP_MEM_MEDIAN as it is read.
#include "icp_select.h"                 // (select_digits, select_pass; TRIM_NONE, trim_key; icp_pair_rule.h)

namespace {

constexpr uint32_t MEDIAN_BLOCK = 256u;

__device__ __forceinline__ uint32_t median_rank (uint32_t n) { return (n + 1u) / 2u; }      // the lower median, counting from 1

// thr = (float) ((factor factor) t_med) in double, in the order written, as bits: +inf (0x7F800000) lies above every candidate's key
__device__ __forceinline__ uint32_t median_threshold (uint32_t factor_bits, uint32_t t_med)
{
    const double f = (double) __uint_as_float (factor_bits);
    return __float_as_uint ((float) ((f * f) * (double) __uint_as_float (t_med)));
}

// the rule's words for the multi-workgroup selection: out = (t_med bits, n, thr bits, accepted)
struct median_rule {
    const uint32_t *factor;
    __device__ __forceinline__ uint32_t rank (uint32_t n) const { return median_rank (n); }
    __device__ __forceinline__ void first (uint32_t *out, uint32_t n, uint32_t) const { out[1] = n; }
    // (the accepted word: k_median_reject's blocks add into it)
    __device__ __forceinline__ void last (uint32_t *out, uint32_t t, uint32_t, uint32_t) const { out[0] = t; out[2] = median_threshold (*factor, t); out[3] = 0u; }
};

// ------------------------------------------------------------------------------------------
// k_median — one workgroup per registration (m <= ICP_TRIM_ONE_BLOCK_MAX): 16 keys per thread in registers, the whole rule in one launch
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (1024) void k_median (icp_params p, uint32_t *words)
{
    constexpr int NT = 1024, KPT = (int) ICP_TRIM_ONE_BLOCK_MAX / NT;
    __shared__ uint32_t s_hist[ICP_TRIM_BINS], s_wsum[NT / 64], s_pick[3];
    const uint32_t b = blockIdx.y, t = threadIdx.x, m = p.m;
    if (icp_pass_leaves (p, b)) return;
    float4 *PF = p.PF + (size_t) b * m;
    const float4 *PM = p.PM + (size_t) b * m;
    uint32_t key[KPT], cnt = 0u;
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const uint32_t i = t + (uint32_t) (NT * k);
        key[k] = i < m ? trim_key (PF[i], PM[i]) : TRIM_NONE;
        cnt += key[k] != TRIM_NONE ? 1u : 0u;
    }
    const uint32_t n = block_sum<NT> (cnt, s_wsum);
    uint32_t *out = words + 4u * b;
    if (n == 0u) {                                           // no candidate: nothing to reject
        if (t == 0u) { out[0] = 0u; out[1] = 0u; out[2] = 0u; out[3] = 0u; }
        return;
    }
    uint32_t t_med, below, at;
    select_digits<NT, KPT> (key, median_rank (n), t, s_hist, s_wsum, s_pick, t_med, below, at);
    const uint32_t thr = median_threshold (*icp_words (words, icp_median_desc (), p.batch).settings, t_med);
    uint32_t acc = 0u;
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        if (key[k] == TRIM_NONE) continue;                   // (no candidate, or no pair: i >= m)
        if (key[k] <= thr) ++acc;
        else icp_pair_reject (PF + t + (uint32_t) (NT * k));
    }
    const uint32_t accepted = block_sum<NT> (acc, s_wsum);
    if (t == 0u) { out[0] = t_med; out[1] = n; out[2] = thr; out[3] = accepted; }
}

// ------------------------------------------------------------------------------------------
// k_median_select_pass<D> — pass D of the selection of large sets (select_pass, icp_select.h), in the rule's words
// ------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__ (256) void k_median_select_pass (icp_params p, uint32_t *words)
{
    const uint32_t b = blockIdx.y, t = threadIdx.x;
    if (icp_pass_leaves (p, b)) return;
    select_pass<D> (p, b, t, icp_select_words_of (words, icp_median_desc (), p.batch, b, p.m), median_rule { icp_words (words, icp_median_desc (), p.batch).settings });
}

// ------------------------------------------------------------------------------------------
// k_median_reject — behind the selection of large sets: one thread per pair over the stored keys, grid (ceil (m / 256), batch)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (MEDIAN_BLOCK) void k_median_reject (icp_params p, uint32_t *words)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * MEDIAN_BLOCK + threadIdx.x, m = p.m;
    if (icp_pass_leaves (p, b)) return;
    const icp_select_words w = icp_select_words_of (words, icp_median_desc (), p.batch, b, m);
    uint32_t *out = w.out;
    if (out[1] == 0u) return;                                // (no candidate: pass 0 has written the four zeros)
    const uint32_t thr = out[2];
    bool acc = false;
    if (i < m) {
        const uint32_t key = w.keys[i];
        acc = key != TRIM_NONE && key <= thr;
        if (key != TRIM_NONE && !acc) icp_pair_reject (p.PF + (size_t) b * m + i);
    }
    const uint32_t wave[1] = { (uint32_t) __popcll (__ballot (acc)) };
    uint32_t sum[1];
    if (pair_block_counts<1, MEDIAN_BLOCK> (wave, sum)) pair_counts_add (out + 3, sum);
}

}  // namespace

// the rule: one workgroup's launch up to ICP_TRIM_ONE_BLOCK_MAX pairs per registration, three select passes and the reject pass beyond
// (launches: icp_route::median); words: the rule's allocation (icp_median_desc)
void icp_launch_median (const icp_params &p, hipStream_t s, uint32_t *words, uint32_t launches)
{
    if (launches == 1u) { hipLaunchKernelGGL (k_median, dim3 (1, p.batch), dim3 (1024), 0, s, p, words); return; }
    const dim3 grid ((p.m + 2047u) / 2048u, p.batch);
    hipLaunchKernelGGL (k_median_select_pass<0>, grid, dim3 (256), 0, s, p, words);
    hipLaunchKernelGGL (k_median_select_pass<1>, grid, dim3 (256), 0, s, p, words);
    hipLaunchKernelGGL (k_median_select_pass<2>, grid, dim3 (256), 0, s, p, words);
    hipLaunchKernelGGL (k_median_reject, dim3 ((p.m + MEDIAN_BLOCK - 1u) / MEDIAN_BLOCK, p.batch), dim3 (MEDIAN_BLOCK), 0, s, p, words);
}
