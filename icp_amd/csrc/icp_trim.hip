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
// The selection is a radix select on 11 / 11 / 10-bit digits: a histogram of the digit over the keys that match the digits picked so
// far, then the bin that holds the remaining rank.  Up to ICP_TRIM_ONE_BLOCK_MAX pairs per registration one workgroup does all three
// passes with the keys in registers and the histogram in LDS (grid.y = registration); beyond it every pass is a launch of many
// workgroups whose LDS histograms are merged by device atomics, and the workgroup that arrives last picks the bin (k_trim_select_pass).
// Both take the same t: the K-th smallest key is one number.
#include "icp_trim_apply.h"             // (TRIM_NONE, trim_key, trim_apply)

namespace {

// pass d of the select: the digit's shift and width, and the shift above which a key must match the prefix picked so far
__device__ __forceinline__ uint32_t trim_shift (int d) { return d == 0 ? 21u : d == 1 ? 10u : 0u; }
__device__ __forceinline__ bool trim_match (uint32_t key, uint32_t prefix, int d)
{
    return key != TRIM_NONE && (d == 0 || (key >> (trim_shift (d - 1))) == (prefix >> trim_shift (d - 1)));
}
__device__ __forceinline__ uint32_t trim_digit (uint32_t key, int d) { return (key >> trim_shift (d)) & (d == 2 ? 1023u : 2047u); }

// K = ceil (ξ n) (ξ n is exact in double: a float times an integer below 2^21)
__device__ __forceinline__ uint32_t trim_rank (float keep, uint32_t n)
{
    return min ((uint32_t) ceil ((double) keep * (double) n), n);
}

// Block-wide: the bin j of s_hist[0 .. 2048) where the cumulative count reaches kk (1 <= kk <= the total): s_pick = (j, count in the
// bins below j, count of bin j).  Every thread of the block calls it; it ends behind a barrier.
template <int NT>
__device__ void trim_pick (const uint32_t *s_hist, uint32_t kk, uint32_t *s_wsum, uint32_t *s_pick)
{
    constexpr int PER = (int) ICP_TRIM_BINS / NT;
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t c[PER], sum = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) { c[k] = s_hist[t * PER + k]; sum += c[k]; }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up (incl, d); if ((int) lane >= d) incl += u; }
    if (lane == 63u) s_wsum[wv] = incl;
    __syncthreads ();
    uint32_t before = incl - sum;
    for (uint32_t w = 0; w < wv; ++w) before += s_wsum[w];
    if (before < kk && kk <= before + sum) {                 // (exactly one thread)
        uint32_t run = before;
        bool found = false;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (!found && run + c[k] >= kk) { s_pick[0] = t * PER + k; s_pick[1] = run; s_pick[2] = c[k]; found = true; }
            run += c[k];
        }
    }
    __syncthreads ();
}

template <int NT>
__device__ __forceinline__ uint32_t block_sum (uint32_t v, uint32_t *s_wsum)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor (v, d);
    __syncthreads ();                                        // (s_wsum may still be read by a trim_pick before)
    if ((threadIdx.x & 63u) == 0u) s_wsum[threadIdx.x >> 6] = v;
    __syncthreads ();
    uint32_t s = 0u;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += s_wsum[w];
    __syncthreads ();
    return s;
}

// ------------------------------------------------------------------------------------------
// k_trim_select — one workgroup per registration (m <= ICP_TRIM_ONE_BLOCK_MAX): 16 keys per thread in registers, three passes
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (1024) void k_trim_select (icp_params p, uint32_t *area)
{
    constexpr int NT = 1024, KPT = (int) ICP_TRIM_ONE_BLOCK_MAX / NT;
    __shared__ uint32_t s_hist[ICP_TRIM_BINS], s_wsum[NT / 64], s_pick[3];
    const uint32_t b = blockIdx.y, t = threadIdx.x, m = p.m;
    if (icp_pass_leaves (p, b)) return;
    const float4 *PF = p.PF + (size_t) b * m, *PM = p.PM + (size_t) b * m;
    uint32_t key[KPT], cnt = 0u;
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const uint32_t i = t + (uint32_t) (NT * k);
        key[k] = i < m ? trim_key (PF[i], PM[i]) : TRIM_NONE;
        cnt += key[k] != TRIM_NONE ? 1u : 0u;
    }
    const uint32_t n = block_sum<NT> (cnt, s_wsum), K = trim_rank (p.trim_keep, n);
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
    if (t == 0u) { out[0] = prefix; out[1] = n; out[2] = K; out[3] = below + at; }
}

// ------------------------------------------------------------------------------------------
// k_trim_select_pass<D> — pass D of the selection of large sets: 2048 pairs per workgroup, grid (ceil (m / 2048), batch).  Pass 0
// computes the keys and leaves them for passes 1 and 2.  The workgroups merge their histograms into the registration's by device
// atomics; the one that arrives last picks the bin, leaves the state for the next pass and clears the histogram and the counter.
// ------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__ (256) void k_trim_select_pass (icp_params p, uint32_t *area)
{
    constexpr int NT = 256, KPT = 8;
    __shared__ uint32_t s_hist[ICP_TRIM_BINS], s_wsum[NT / 64], s_pick[3];
    __shared__ uint32_t s_last;
    const uint32_t b = blockIdx.y, t = threadIdx.x, m = p.m, B = p.batch;
    if (icp_pass_leaves (p, b)) return;
    uint32_t *out = area + 4u * b, *sel = area + 4u * B + 4u * b, *hist = area + 8u * B + (size_t) ICP_TRIM_BINS * b;
    uint32_t *keys = area + (8u + ICP_TRIM_BINS) * (size_t) B + (size_t) b * m;
    if (D > 0 && out[1] == 0u) return;                       // (no candidate: pass 0 has said so)
    const uint32_t prefix = D > 0 ? sel[0] : 0u;
    for (uint32_t j = t; j < ICP_TRIM_BINS; j += NT) s_hist[j] = 0u;
    __syncthreads ();
    const float4 *PF = p.PF + (size_t) b * m, *PM = p.PM + (size_t) b * m;
    const uint32_t i0 = blockIdx.x * (uint32_t) (NT * KPT) + t;
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const uint32_t i = i0 + (uint32_t) (NT * k);
        uint32_t key = TRIM_NONE;
        if (i < m) {
            if constexpr (D == 0) { key = trim_key (PF[i], PM[i]); keys[i] = key; }
            else key = keys[i];
        }
        if (trim_match (key, prefix, D)) atomicAdd (&s_hist[trim_digit (key, D)], 1u);
    }
    __syncthreads ();
    for (uint32_t j = t; j < ICP_TRIM_BINS; j += NT)
        if (s_hist[j]) __hip_atomic_fetch_add (hist + j, s_hist[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence ();                                        // this thread's counts, before its arrival counts
    __syncthreads ();                                        // (every wave's: the ticket below speaks for the whole workgroup)
    if (t == 0u) s_last = __hip_atomic_fetch_add (sel + 3, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads ();
    if (!s_last) return;
    __threadfence ();                                        // the others' counts
    for (uint32_t j = t; j < ICP_TRIM_BINS; j += NT) {
        s_hist[j] = __hip_atomic_load (hist + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store (hist + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (clear for the next pass)
    }
    if (t == 0u) __hip_atomic_store (sel + 3, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads ();
    uint32_t kk, below, n = 0u, K = 0u;
    if constexpr (D == 0) {
        uint32_t c = 0u;
        for (uint32_t j = t; j < ICP_TRIM_BINS; j += NT) c += s_hist[j];
        n = block_sum<NT> (c, s_wsum); K = trim_rank (p.trim_keep, n);
        if (n == 0u) {
            if (t == 0u) { out[0] = 0u; out[1] = 0u; out[2] = 0u; out[3] = 0u; }
            return;
        }
        kk = K; below = 0u;
    } else { kk = sel[1]; below = sel[2]; }
    trim_pick<NT> (s_hist, kk, s_wsum, s_pick);
    if (t == 0u) {
        const uint32_t j = s_pick[0], lo = s_pick[1];
        sel[0] = prefix | (j << trim_shift (D)); sel[1] = kk - lo; sel[2] = below + lo;
        if constexpr (D == 0) { out[1] = n; out[2] = K; }
        if constexpr (D == 2) { out[0] = prefix | j; out[3] = below + lo + s_pick[2]; }
    }
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
