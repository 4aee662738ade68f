// icp_pair_rule.h — the vocabulary of a pass over the pairs of a search, stated once.  Every pass behind the search or in its place
// speaks it: the pair filter, one-to-one, reciprocal, projective (icp_pair_filter / _unique / _reciprocal / _projective.hip), trimming
// and the apply passes (icp_trim.hip, icp_robust.hip, icp_trim_apply.h), the plane moments (icp_plane_moments.h: icp_pass_leaves), the
// grid normals and the pyramid (icp_p2pl.hip, icp_pyramid.hip: icp_point_valid), and the kernels that evaluate a finished search:
// k_quality_pairs (icp_quality.hip) and k_pairs_count / k_pairs_scatter (icp_pairs.hip), whose count and length agree because both
// evaluate icp_pair_inlier.  Every translation unit is built with -ffp-contract=off: each expression is evaluated in the order it is
// written; tests/quality_ref.py (masks, geo_of) and the passes' own *_ref.py restate them.
//
// A point is valid iff x, y, z are finite and not all zero (icp_point_valid; the searches and buildRBC test "at the origin" alone: a
// different rule).  Pair i, with e = PM[i].xyz (the transformed moving point), f = PF[i].xyz (the returned fixed point), mv = M[i].xyz:
//   candidate = PF[i].w != 0 and NN_ID[i].id < m: the passes in front have left it, its id is a row of F          (icp_pair_candidate)
//   counted = i < m and mv valid                                                                                   (icp_pair_counted)
//   geo = (gx gx + gy gy) + gz gz in fp32, g = e - f componentwise: the rejection rule's quantity, trimming's key  (icp_pair_geo)
//   inlier = counted, f not (0, 0, 0), geo finite, and geo <= d2 unless the distance test is off                   (icp_pair_inlier)
// A pass rejects a pair by storing +0 into PF[i].w (icp_pair_reject): it is then exactly a rejected pair for every pass behind, and
// leaves a converged registration of a checked run alone (icp_pass_leaves): its last iteration's outputs and counts stay.
#pragma once
#include "icp_kernels.h"

// (once, in the three forms its callers hold a point in: a forward from one form to another changes the code of one form's kernels —
// what the spellings of this header are checked against: tools/diag/isa_diff.py, profiles/pair_pass_isa_diff.txt)
#define ICP_POINT_VALID(x, y, z) (isfinite (x) && isfinite (y) && isfinite (z) && !((x) == 0.f && (y) == 0.f && (z) == 0.f))
static __device__ __forceinline__ bool icp_point_valid (float x, float y, float z) { return ICP_POINT_VALID (x, y, z); }
static __device__ __forceinline__ bool icp_point_valid (const float4 &g) { return ICP_POINT_VALID (g.x, g.y, g.z); }
static __device__ __forceinline__ bool icp_point_valid (const float *r) { const float x = r[0], y = r[1], z = r[2]; return ICP_POINT_VALID (x, y, z); }
#undef ICP_POINT_VALID

static __device__ __forceinline__ bool icp_pair_candidate (float w, uint32_t id, uint32_t m) { return w != 0.f && id < m; }
static __device__ __forceinline__ bool icp_pair_counted (bool in_range, const float4 &mv) { return in_range && icp_point_valid (mv); }

static __device__ __forceinline__ float icp_pair_geo (const float4 &f, const float4 &e)
{
    const float gx = e.x - f.x, gy = e.y - f.y, gz = e.z - f.z;
    return (gx * gx + gy * gy) + gz * gz;
}

static __device__ __forceinline__ bool icp_pair_inlier (bool counted, const float4 &f, float geo, uint32_t dist_on, float d2)
{
    return counted && !(f.x == 0.f && f.y == 0.f && f.z == 0.f) && isfinite (geo) && (!dist_on || geo <= d2);
}

static __device__ __forceinline__ void icp_pair_reject (float4 *pf) { reinterpret_cast<float *> (pf)[3] = 0.f; }      // pf: the pair's PF record

// (an `if`, as in the passes' own bodies before: `return a && b` compiles to another branch in some of them)
static __device__ __forceinline__ bool icp_pass_leaves (const icp_params &p, uint32_t b) { if (p.check && p.st[b].done) return true; return false; }

// Counting: per registration, how many pairs a rule pass saw and what became of them.  Integer sums: no order of arrival matters.
// pair_block_counts<N, BLOCK>: every thread hands in its wave's N counts (popcounts of ballots, summed over the block's rounds where
// it has several); behind one barrier thread 0, for which alone the call returns true, has the block's sums.  Count by count, not in a
// loop over k: the compiler merges a row's stores and loads only where they stand side by side.  k_quality_pairs and k_pairs_count /
// k_pairs_scatter keep their own: their counts cross barriers that other work shares (plane_block_tree's, the sum into s_front).
template <uint32_t N, uint32_t BLOCK>
static __device__ __forceinline__ bool pair_block_counts (const uint32_t (&wave)[N], uint32_t (&sum)[N])
{
    static_assert (N >= 1u && N <= 4u && BLOCK % 64u == 0u, "one to four counts per wave, whole waves");
    __shared__ uint32_t s_cnt[BLOCK / 64u][N];
    const uint32_t t = threadIdx.x;
    if ((t & 63u) == 0u) {
        s_cnt[t >> 6][0] = wave[0];
        if constexpr (N > 1u) s_cnt[t >> 6][1] = wave[1];
        if constexpr (N > 2u) s_cnt[t >> 6][2] = wave[2];
        if constexpr (N > 3u) s_cnt[t >> 6][3] = wave[3];
    }
    __syncthreads ();
    if (t != 0u) return false;
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) sum[k] = 0u;
#pragma unroll
    for (uint32_t v = 0; v < BLOCK / 64u; ++v) {
        sum[0] += s_cnt[v][0];
        if constexpr (N > 1u) sum[1] += s_cnt[v][1];
        if constexpr (N > 2u) sum[2] += s_cnt[v][2];
        if constexpr (N > 3u) sum[3] += s_cnt[v][3];
    }
    return true;
}

// Two ways to hand a block's sums on to the registration's result words, decided by whether a launch stands in front of the pass that
// can reset them.
// pair_counts_add — one does (k_unique_claim's first thread, k_reciprocal_state's first lane, under the pass's own icp_pass_leaves
// test: no reset without its counts, and a converged registration's words stay).  The blocks add straight into the result words:
// relaxed, agent scope, zero sums skipped; no ticket, no fence.
// pair_counts_ticket — none does (the pair filter follows the search, k_projective replaces it).  The blocks add into the running
// words run[0 .. 2] (relaxed) and draw a ticket from run[4] (acquire-release, agent scope); the block that draws the last of the
// registration's `blocks` tickets — every other block's counts are in by then — exchanges the sums out, zeroes the ticket and writes
// result[0 .. 3] = (n, a, b, n - a - b).  Running words and ticket are zero between launches.
// The ticket's cost: a block's release at agent scope writes its XCD's L2 back, the pass's fresh weights and all.  With it k_reciprocal
// took 388 instead of 294 us per iteration (64 batched registrations of 16384 pairs): a pass with a launch in front takes none.  A pass
// that must keeps its tickets few: k_projective serves 1024 queries per block in four rounds of 256 threads (at 2^20 points, blocks of
// 1024 threads and one round — as many tickets — take 188 instead of 90 us per point-to-point iteration at r = 0).
template <uint32_t N>
static __device__ __forceinline__ void pair_counts_add (uint32_t *out, const uint32_t (&sum)[N])
{
#pragma unroll
    for (uint32_t k = 0; k < N; ++k)
        if (sum[k]) __hip_atomic_fetch_add (out + k, sum[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static __device__ __forceinline__ void pair_counts_ticket (uint32_t *run, uint32_t *result, uint32_t a, uint32_t b, uint32_t c, uint32_t blocks)
{
    if (a) __hip_atomic_fetch_add (run + 0, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b) __hip_atomic_fetch_add (run + 1, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c) __hip_atomic_fetch_add (run + 2, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t ticket = __hip_atomic_fetch_add (run + 4, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket + 1u == blocks) {                             // (the last block of the registration: every count is in)
        const uint32_t n = __hip_atomic_exchange (run + 0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t na = __hip_atomic_exchange (run + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t nb = __hip_atomic_exchange (run + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store (run + 4, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        result[0] = n; result[1] = na; result[2] = nb; result[3] = n - na - nb;
    }
}
