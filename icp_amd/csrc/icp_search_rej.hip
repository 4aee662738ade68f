// icp_search_rej.hip — the search kernels with correspondence rejection on (icp_set_rejection: k_search<.., REJ = true>, every layout and
// the chained form).  A translation unit of their own: the default kernels (icp_kernels.hip, icp_search_dense.hip) carry none of the
// rejection code, and the launchers there hand a handle with rejection on over to these.
#include "icp_search.h"

void icp_launch_search_rej (const icp_params &p, hipStream_t s)
{
    if (icp_dense (p)) ks_launch_dense<true> (p, s);
    else ks_launch_latency<true> (p, s);
}

void icp_launch_chain_one_rej (const icp_params &p, hipStream_t s, uint32_t j, bool fresh, bool emit)
{
    ks_launch_chain_one<true> (p, s, j, fresh, emit);
}
