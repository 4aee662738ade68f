// icp_unique.hip — one-to-one correspondences (icp_set_unique, include/icp_amd.h): of the candidate pairs that share a fixed point only
// the closest keeps its weight; every other gets the weight +0 and is then exactly a rejected pair.
//
// An iteration with the rule on is: the REJ search (icp_search_rej.hip), which stores its per-query outputs; k_unique_claim, in which
// every candidate pair i takes an unsigned 64-bit minimum of its key (bits (geo_i) << 32 | i) into claim[b][id_i]; k_unique_resolve, in
// which pair i is the winner of its fixed point when claim[b][id_i] == key_i, a loser's weight becomes +0 in PF.w, and the
// registration's (candidates, winners) are counted; then trimming's selection (when trimming is on too: its candidates are the winners)
// and the apply pass (icp_trim_apply.h), which writes the search blocks' partials again from PF / PM — point-to-point only: the plane
// metrics read w in k_plane_moments —; then the unchanged tail of the iteration (the order: icp_route_of, icp_kernels.hip).  None of the
// existing kernels carries any of this code.
//
// Determinism: the winner is the minimum of integers that are all different (the query index is part of the key), and an integer minimum
// does not depend on the order of arrival.  Nothing else decides a value: the counts are integer sums.
//
// The claim table is ONE table of m words per registration that reads all-ones between iterations.  A slot that was claimed has exactly
// one winner, and the winner — having compared — stores all-ones back into its slot in the resolve pass; a loser of that slot that reads
// it afterwards sees all-ones in place of the winner's key, and neither equals its own key (a candidate's geo is finite: its key's high
// word is below 0x7F800000), so it is a loser either way.  The two passes are launched together (icp_launch_unique) and both leave a
// registration alone under the same test (p.check && st.done, which only a finalize behind them changes), so a claim pass without its
// resolve pass does not exist: a converged registration's table is not touched and stays clean, and the first iteration after
// icp_init (which fills the table with 0xFF), buildRBC, reset_transform or a new graph finds it as the last resolve pass left it.  No
// memset, no extra launch, no second table.
//
// The result words of a registration, [batch][2] uint32 (ICP_AREA_UNIQUE): (n, winners), ICP_MEM_UNIQUE as it is read.  k_unique_claim's
// first thread resets them, k_unique_resolve's blocks add their counts (pair_counts_add, icp_pair_rule.h).  Nothing else reads them:
// the apply pass behind the rule accepts every pair that still has a weight (icp_trim_apply.h).
#include "icp_trim_apply.h"             // (TRIM_NONE, trim_key; icp_pair_rule.h)

namespace {

constexpr uint32_t UNIQUE_BLOCK = 256u;
constexpr unsigned long long UNIQUE_FREE = ~0ull;       // a slot nobody has claimed

// the claim key of pair i, and the slot it claims (candidate: key != UNIQUE_FREE)
__device__ __forceinline__ unsigned long long unique_key (const icp_params &p, uint32_t b, uint32_t i, uint32_t *id)
{
    const size_t e = (size_t) b * p.m + i;
    const uint32_t k = trim_key (p.PF[e], p.PM[e]);
    *id = p.nn_id[e].id;
    // (icp_pair_candidate, with a finite geo: an id is an index into F; a word that is not would be no claim, never a store outside the table)
    return (k != TRIM_NONE && *id < p.m) ? ((unsigned long long) k << 32) | i : UNIQUE_FREE;
}

// ------------------------------------------------------------------------------------------
// k_unique_claim — one thread per pair, grid (ceil (m / 256), batch)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (UNIQUE_BLOCK) void k_unique_claim (icp_params p, unsigned long long *claims, uint32_t *area)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * UNIQUE_BLOCK + threadIdx.x;
    if (icp_pass_leaves (p, b)) return;
    if (i == 0u) { uint32_t *out = area + 2u * b; out[0] = 0u; out[1] = 0u; }
    if (i >= p.m) return;
    uint32_t id;
    const unsigned long long key = unique_key (p, b, i, &id);
    if (key != UNIQUE_FREE) __hip_atomic_fetch_min (claims + (size_t) b * p.m + id, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------
// k_unique_resolve — one thread per pair, same grid
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__ (UNIQUE_BLOCK) void k_unique_resolve (icp_params p, unsigned long long *claims, uint32_t *area)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * UNIQUE_BLOCK + threadIdx.x;
    if (icp_pass_leaves (p, b)) return;
    bool cand = false, win = false;
    if (i < p.m) {
        uint32_t id;
        const unsigned long long key = unique_key (p, b, i, &id);
        cand = key != UNIQUE_FREE;
        if (cand) {
            unsigned long long *slot = claims + (size_t) b * p.m + id;
            win = __hip_atomic_load (slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key;
            if (win) __hip_atomic_store (slot, UNIQUE_FREE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (clean for the next iteration)
            else icp_pair_reject (p.PF + (size_t) b * p.m + i);
        }
    }
    const uint32_t wave[2] = { (uint32_t) __popcll (__ballot (cand)), (uint32_t) __popcll (__ballot (win)) };
    uint32_t sum[2];
    if (pair_block_counts<2, UNIQUE_BLOCK> (wave, sum)) pair_counts_add (area + 2u * b, sum);
}

}  // namespace

void icp_launch_unique (const icp_params &p, hipStream_t s)
{
    const dim3 grid ((p.m + UNIQUE_BLOCK - 1u) / UNIQUE_BLOCK, p.batch);
    unsigned long long *claims = icp_unique_claims (p);
    uint32_t *area = icp_words (p, ICP_AREA_UNIQUE).result;
    hipLaunchKernelGGL (k_unique_claim, grid, dim3 (UNIQUE_BLOCK), 0, s, p, claims, area);
    hipLaunchKernelGGL (k_unique_resolve, grid, dim3 (UNIQUE_BLOCK), 0, s, p, claims, area);
}
