// icp_adaptive_trim.hip — adaptive trimming (icp_set_adaptive_trimming, include/icp_amd.h): every iteration chooses the kept fraction
// itself, by the fractional root mean squared distance of Fractional ICP (Phillips, Liu, Tomasi): among the thresholds of a fixed table
// it takes the one that minimises (sum of the geo at or below it) / (their number)^q, and gives the pairs above it the weight +0.
//
// An iteration with the rule on is trimming's (icp_route_of, icp_kernels.hip) with this selection in the place of the radix select: the
// REJ search or k_projective; the pair filter, the reciprocal rule, one-to-one and median-distance rejection, where they are on; this
// selection, which fills the four words of ICP_AREA_TRIM (t bits, n, K, accepted); the apply pass, which reads them as it reads
// trimming's (icp_trim_apply.h: key <= t) — the plane metrics read the weights it leaves in their moments; the unchanged tail.  None of
// the existing kernels carries any of this code.
//
// The table: bin j = key >> 19 of a pair's key (trim_key: the float bits of geo), 4096 bins of 8 exponent bits and the top 4 mantissa
// bits.  Per bin the candidates' number c_j and the sum of their geo B_j.  B_j is kept integral: the keys of a bin share the exponent and
// the top of the significand, so sum (key & 0x7FFFF) in 64 bits and c_j say everything, and
//   B_j = ldexp ((double) (c_j * base_j + low_j), max (e, 1) - 150),  e = j >> 4,  base_j = (e ? 2^23 : 0) + ((j & 15) << 19)
// is exact (an integer below 2^53) in whatever order the pairs arrive.  64-bit integer adds are native in LDS and at the device's L2;
// nothing here loops on a compare-and-swap.
//
// One launch at every size.  Beyond ICP_TRIM_ONE_BLOCK_MAX pairs per registration (k_adaptive_trim<256, false>): grid
// (ceil (m / 2048), batch), 8 pairs per thread.  Each workgroup histograms its pairs into an LDS table (4096 x (count, low sum), 48 KB),
// adds its non-empty bins into the registration's table by device atomics and draws a ticket as select_pass does (icp_select.h); the
// workgroup that arrives last loads and clears the table and finishes.  Up to that size (k_adaptive_trim<1024, true>): one workgroup
// per registration, 16 pairs per thread, and the LDS table is the registration's — no device atomics, no ticket, no fence (an arrival's
// release at agent scope writes the L2 back, fresh outputs of the search and all: 64 batched registrations of 16384 pairs took 203 us
// per point-to-point iteration with eight tickets each, against trimming's 157).  Both finish alike: r_j by a block scan, S_j in the
// rule's run order (64 runs of 64 bins, one lane each, then a 64-step base — plain additions in the order written, no contraction:
// the unit is built with -ffp-contract=off), the costs S_j / r_j^q and the minimum over (cost bits, j), which is one number whatever the
// order.  The words do not depend on the form: B_j is exact.  No keys are stored: the apply pass computes them again.
//
// The rule's words are an allocation of their own on the handle (icp_adaptive_desc, icp_kernels.h) and reach the kernel as an argument.
// Result words of a registration there: (j*, r_lo, r_hi, candidate bins), ICP_MEM_TRIM_ADAPTIVE as it is read.
#include "icp_trim_apply.h"             // (TRIM_NONE, trim_key; icp_pair_rule.h)

namespace {

constexpr uint32_t AT_BINS = ICP_ADAPTIVE_BINS;
constexpr uint32_t AT_PAD = AT_BINS + AT_BINS / 64u;        // a run of 64 sums per lane, 65 apart: the lanes' banks differ

// as icp_trim.hip's trim_rank: min (ceil (fraction n), n), the product exact in double
__device__ __forceinline__ uint32_t adaptive_rank (uint32_t fraction_bits, uint32_t n)
{
    return min ((uint32_t) ceil ((double) __uint_as_float (fraction_bits) * (double) n), n);
}

// B_j from the bin's count and the sum of its keys' low 19 bits
__device__ __forceinline__ double adaptive_bin_sum (uint32_t j, uint32_t c, unsigned long long low)
{
    const uint32_t e = j >> 4;
    const unsigned long long base = (e ? 1ull << 23 : 0ull) + ((unsigned long long) (j & 15u) << 19);
    return ldexp ((double) ((unsigned long long) c * base + low), (int) max (e, 1u) - 150);
}

// ------------------------------------------------------------------------------------------
// k_adaptive_trim<NT, ONE> — the whole selection.  ONE: one workgroup of NT threads per registration (m <= NT * 16), else workgroups of
// NT threads and NT * 8 pairs, merged in the registration's table.  trim: ICP_AREA_TRIM's result words; words: the rule's allocation
// ------------------------------------------------------------------------------------------
template <uint32_t NT, bool ONE>
__global__ __launch_bounds__ (NT) void k_adaptive_trim (icp_params p, uint32_t *trim, uint32_t *words)
{
    constexpr uint32_t KPT = ONE ? 16u : 8u, PER = AT_BINS / NT, NW = NT / 64u;
    __shared__ unsigned long long s_sum[AT_PAD];            // the low sums; the finisher: B_j, then s_{u,i}, at j + (j >> 6)
    __shared__ uint32_t s_cnt[AT_BINS];                      // c_j
    __shared__ double s_base[64];
    __shared__ unsigned long long s_best[NW], s_bestjr[NW];
    __shared__ uint32_t s_wsum[NW], s_nbin[NW];
    __shared__ uint32_t s_last;
    const uint32_t b = blockIdx.y, t = threadIdx.x, m = p.m, lane = t & 63u, wv = t >> 6;
    if (icp_pass_leaves (p, b)) return;
    const icp_adaptive_words w = icp_adaptive_words_of (words, p.batch, b);
    for (uint32_t j = t; j < AT_BINS; j += NT) { s_cnt[j] = 0u; s_sum[j] = 0ull; }
    __syncthreads ();
    const float4 *PF = p.PF + (size_t) b * m, *PM = p.PM + (size_t) b * m;
    const uint32_t i0 = blockIdx.x * (NT * KPT) + t;
#pragma unroll
    for (uint32_t k = 0; k < KPT; ++k) {
        const uint32_t i = i0 + NT * k;
        const uint32_t key = i < m ? trim_key (PF[i], PM[i]) : TRIM_NONE;
        if (key != TRIM_NONE) {
            atomicAdd (&s_cnt[key >> 19], 1u);
            atomicAdd (&s_sum[key >> 19], (unsigned long long) (key & 0x7FFFFu));
        }
    }
    __syncthreads ();
    uint32_t cj[PER];
    unsigned long long low[PER];
    if constexpr (ONE) {
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) { cj[k] = s_cnt[t + NT * k]; low[k] = s_sum[t + NT * k]; }
    } else {
        for (uint32_t j = t; j < AT_BINS; j += NT) {
            const uint32_t c = s_cnt[j];
            if (c) {
                __hip_atomic_fetch_add (w.cnt + j, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add (w.sum + j, s_sum[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __threadfence ();                                    // this thread's bins, before its arrival counts
        __syncthreads ();                                    // (every wave's: the ticket below speaks for the whole workgroup)
        if (t == 0u) s_last = __hip_atomic_fetch_add (w.arrivals, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
        __syncthreads ();
        if (!s_last) return;
        __threadfence ();                                    // the others' bins
        // the last arrival finishes: the registration's table, cleared for the next launch
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint32_t j = t + NT * k;
            cj[k] = __hip_atomic_load (w.cnt + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            low[k] = 0ull;
            if (cj[k]) {
                low[k] = __hip_atomic_load (w.sum + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store (w.cnt + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store (w.sum + j, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (t == 0u) __hip_atomic_store (w.arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads ();                                        // (the workgroup's own table has been read: B_j moves into its padded place)
    // ---- the finish: c_j, and B_j where run u starts at 65 u
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t j = t + NT * k;
        s_cnt[j] = cj[k];
        s_sum[j + (j >> 6)] = (unsigned long long) __double_as_longlong (cj[k] ? adaptive_bin_sum (j, cj[k], low[k]) : 0.0);
    }
    __syncthreads ();
    // r_j: thread t has bins PER t .. PER t + PER - 1, the block scans the threads' sums
    uint32_t c[PER], sum = 0u;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) { c[k] = s_cnt[t * PER + k]; sum += c[k]; }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up (incl, d); if ((int) lane >= d) incl += u; }
    if (lane == 63u) s_wsum[wv] = incl;
    // S_j in the rule's order, wave 0: lane u adds run u up where it lies, then the bases one after the other
    if (wv == 0u) {
        unsigned long long *run = s_sum + 65u * lane;
        double s = __longlong_as_double ((long long) run[0]);
#pragma unroll
        for (uint32_t i = 1; i < 64u; ++i) { s = s + __longlong_as_double ((long long) run[i]); run[i] = (unsigned long long) __double_as_longlong (s); }
        double base = 0.0, acc = 0.0;
#pragma unroll
        for (uint32_t u = 1; u < 64u; ++u) { acc = acc + __shfl (s, (int) (u - 1u)); if (lane == u) base = acc; }
        s_base[lane] = base;
    }
    __syncthreads ();
    uint32_t before = incl - sum, n = 0u;
#pragma unroll
    for (uint32_t v = 0; v < NW; ++v) { if (v < wv) before += s_wsum[v]; n += s_wsum[v]; }
    uint32_t *out = trim + 4u * b;
    if (n == 0u) {                                           // no candidate: the apply pass trims every pair
        if (t == 0u) { out[0] = 0u; out[1] = 0u; out[2] = 0u; out[3] = 0u; w.out[0] = 0u; w.out[1] = 0u; w.out[2] = 0u; w.out[3] = 0u; }
        return;
    }
    // the costs of this thread's candidate bins and the least (cost bits, j); r_j rides along in the low word beside j
    const uint32_t r_lo = adaptive_rank (w.settings[0], n), r_hi = adaptive_rank (w.settings[1], n), q = w.settings[2];
    unsigned long long best = ~0ull, best_jr = ~0ull;
    uint32_t nbin = 0u, r = before;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t j = t * PER + k, prev = r;
        r += c[k];
        if (c[k] == 0u || r < r_lo || prev >= r_hi) continue;        // (j_lo <= j: r_j >= r_lo; j <= j_hi: r_{j-1} < r_hi)
        ++nbin;
        const double S = s_base[j >> 6] + __longlong_as_double ((long long) s_sum[j + (j >> 6)]);
        double P = (double) r;
        for (uint32_t e = 1u; e < q; ++e) P = P * (double) r;
        const unsigned long long cost = (unsigned long long) __double_as_longlong (S / P), jr = ((unsigned long long) j << 32) | r;
        if (cost < best || (cost == best && jr < best_jr)) { best = cost; best_jr = jr; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long ob = __shfl_xor (best, d), oj = __shfl_xor (best_jr, d);
        nbin += __shfl_xor (nbin, d);
        if (ob < best || (ob == best && oj < best_jr)) { best = ob; best_jr = oj; }
    }
    if (lane == 0u) { s_best[wv] = best; s_bestjr[wv] = best_jr; s_nbin[wv] = nbin; }
    __syncthreads ();
    if (t == 0u) {
#pragma unroll
        for (uint32_t v = 1; v < NW; ++v) {
            const unsigned long long ob = s_best[v], oj = s_bestjr[v];
            nbin += s_nbin[v];
            if (ob < best || (ob == best && oj < best_jr)) { best = ob; best_jr = oj; }
        }
        const uint32_t js = (uint32_t) (best_jr >> 32), K = (uint32_t) best_jr;
        out[0] = ((js + 1u) << 19) - 1u; out[1] = n; out[2] = K; out[3] = K;
        w.out[0] = js; w.out[1] = r_lo; w.out[2] = r_hi; w.out[3] = nbin;
    }
}

}  // namespace

// one workgroup per registration up to ICP_TRIM_ONE_BLOCK_MAX pairs, workgroups of 2048 pairs beyond: one launch either way
void icp_launch_adaptive_trim (const icp_params &p, hipStream_t s, uint32_t *words)
{
    uint32_t *trim = icp_words (p, ICP_AREA_TRIM).result;
    if (p.m <= ICP_TRIM_ONE_BLOCK_MAX) hipLaunchKernelGGL ((k_adaptive_trim<1024u, true>), dim3 (1, p.batch), dim3 (1024), 0, s, p, trim, words);
    else hipLaunchKernelGGL ((k_adaptive_trim<256u, false>), dim3 ((p.m + 2047u) / 2048u, p.batch), dim3 (256), 0, s, p, trim, words);
}
