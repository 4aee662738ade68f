// icp_select.h — the deterministic radix select over the keys of a registration's pairs (trim_key, icp_trim_apply.h): the K-th smallest
// key among the candidates, parametrised by the rank rule and the words it works in.  Two rules instantiate it: trimming (icp_trim.hip:
// K = ceil (ξ n), the words of ICP_AREA_TRIM) and median-distance rejection (icp_median.hip: K = (n + 1) / 2, the words of the rule's
// own allocation).  The words of both have one shape (icp_select_words_of, icp_kernels.h).
//
// The selection works on 11 / 11 / 10-bit digits: a histogram of the digit over the keys that match the digits picked so far, then the
// bin that holds the remaining rank.  One workgroup with its keys in registers runs the three digits in one launch (select_digits);
// beyond ICP_TRIM_ONE_BLOCK_MAX pairs every digit is a launch of many workgroups (select_pass<D>) whose LDS histograms are merged by
// device atomics, and the workgroup that arrives last picks the bin.  Both take the same t: the K-th smallest key is one number, and
// every count is an integer sum.
//
// One exception, measured: k_trim_select writes select_digits' loop out in its own body, from the helpers here.  Calling select_digits
// there changes the kernel's instructions, and trimming's iteration at 16384 pairs then takes 0.1 - 0.2 us longer than the parent's
// range (profiles/select_ab.txt).  tests/test_gpu_select.py holds the two rules against each other.
//
// What a rule brings to select_pass (RULE, a struct of three members; the kernel hands its words in as icp_select_words):
//   uint32_t rank (uint32_t n)                                the rank K in 1 .. n of n >= 1 candidates
//   void first (uint32_t *out, uint32_t n, uint32_t K)        pass 0's last workgroup, thread 0: n and K are known
//   void last (uint32_t *out, uint32_t t, uint32_t below, uint32_t at)    pass 2's last workgroup, thread 0: t, how many keys are < t and == t
// With no candidate pass 0 writes four zeros to `out` and the later passes leave at out[1] == 0: out[1] is n under every rule.
#pragma once
#include "icp_trim_apply.h"             // (TRIM_NONE, trim_key)

namespace {

// pass d of the select: the digit's shift and width, and the shift above which a key must match the prefix picked so far
__device__ __forceinline__ uint32_t trim_shift (int d) { return d == 0 ? 21u : d == 1 ? 10u : 0u; }
__device__ __forceinline__ bool trim_match (uint32_t key, uint32_t prefix, int d)
{
    return key != TRIM_NONE && (d == 0 || (key >> (trim_shift (d - 1))) == (prefix >> trim_shift (d - 1)));
}
__device__ __forceinline__ uint32_t trim_digit (uint32_t key, int d) { return (key >> trim_shift (d)) & (d == 2 ? 1023u : 2047u); }

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
// select_digits — one workgroup of NT threads, KPT keys per thread in registers: the three digit passes at rank K (1 <= K <= the number
// of candidates).  prefix: the K-th smallest key; below + at: how many keys are <= it.  Every thread of the block calls it.
// ------------------------------------------------------------------------------------------
template <int NT, int KPT>
__device__ __forceinline__ void select_digits (uint32_t (&key)[KPT], uint32_t K, uint32_t t, uint32_t *s_hist, uint32_t *s_wsum, uint32_t *s_pick,
                                               uint32_t &prefix, uint32_t &below, uint32_t &at)
{
    uint32_t kk = K;
    prefix = 0u; below = 0u; at = 0u;
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
}

// ------------------------------------------------------------------------------------------
// select_pass<D> — pass D of the selection of large sets: 2048 pairs per workgroup of 256 threads, grid (ceil (m / 2048), batch).  Pass 0
// computes the keys and leaves them for passes 1 and 2 (and for whoever reads them behind the selection).  The workgroups merge their
// histograms into the registration's by device atomics; the one that arrives last picks the bin, leaves the state for the next pass
// and clears the histogram and the counter.
// ------------------------------------------------------------------------------------------
template <int D, class RULE>
__device__ __forceinline__ void select_pass (const icp_params &p, uint32_t b, uint32_t t, const icp_select_words w, const RULE &rule)
{
    constexpr int NT = 256, KPT = 8;
    __shared__ uint32_t s_hist[ICP_TRIM_BINS], s_wsum[NT / 64], s_pick[3];
    __shared__ uint32_t s_last;
    const uint32_t m = p.m;
    uint32_t *out = w.out, *sel = w.sel, *hist = w.hist, *keys = w.keys;
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
        n = block_sum<NT> (c, s_wsum); K = rule.rank (n);
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
        if constexpr (D == 0) rule.first (out, n, K);
        if constexpr (D == 2) rule.last (out, prefix | j, below + lo, s_pick[2]);
    }
}

}  // namespace
