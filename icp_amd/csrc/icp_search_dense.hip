// icp_search_dense.hip — the DENSE variants of the search kernel (icp_search.h: k_search<.., MINW = 4, LPQ = 8, ..>): 512-thread blocks,
// several per CU, eight lanes per query, exact stage-1 pruning; LDS tiles of 256 representatives (SINGLE: |R| <= 256, batches; MASKED:
// 256 < |R| <= 4096, the tile set of a block decided in one pre-pass) or 1024 (beyond); stage 2 by a query's lanes or with lanes = candidates
// (S2W: lists of >= 128 candidates).  Which one runs: icp_dense / icp_dense_tile / icp_s2_wave_of (icp_kernels.hip), reported by
// icp_search_layout.  The latency variants, the chained form and every other kernel of the iteration live in icp_kernels.hip.
#include "icp_search.h"

// RBC construct, step 1: owner(x) = nearest representative — the search kernel's stage 1 over the fixed points
// (LDS tiles of 256 representatives up to |R| = 4096 — four blocks per CU —, of 1024 beyond, where a 4 x 4 tile group no longer fits a
// 256-tile: icp_dense_tile)
void icp_launch_owner_search_dense (const icp_params &p, hipStream_t s)
{
    const ks_dense_form f = ks_dense_select (p.nr, p.nrx, 0u);
    const ks_kernel k = f.masked ? ks_owner<KS_OWNER_DENSE_256_MASKED> : f.single ? ks_owner<KS_OWNER_DENSE_256_SINGLE> : ks_owner<KS_OWNER_DENSE_1024>;
    hipLaunchKernelGGL (k, dim3 (p.nb, p.batch), dim3 (KS_DENSE_THREADS), 0, s, KS_OWNER_ARGS);
}

void icp_launch_search_dense (const icp_params &p, hipStream_t s) { ks_launch_dense<false> (p, s); }
