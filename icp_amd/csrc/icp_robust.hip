// icp_robust.hip — the robust loss (icp_set_robust_loss, include/icp_amd.h): every pair is down-weighted by the loss's IRLS weight
// omega (icp_robust_omega) of its own residual.  The kernels are the existing ones with the loss switched on by a template argument:
// point-to-point weighs its pairs in the apply pass behind the search (k_trim_apply_robust<FUSED>, icp_trim_apply.inc; with trimming
// on too, behind trimming's selection), the plane metrics in their moments (k_plane_moments_robust<COLORED>, icp_plane_moments.inc).
// They live in this translation unit so that the loss-off kernels of icp_trim.hip and icp_p2pl.hip stay exactly what they were.  The
// scale k is a device word (icp_robust_scale, found from icp_params), written in stream order by icp_set_robust_loss: a new k touches no
// captured graph.
#include "icp_trim_apply.h"
#include "icp_plane_moments.h"

namespace {

#define ICP_APPLY_NAME k_trim_apply_robust
#define ICP_APPLY_ROBUST true
#include "icp_trim_apply.inc"

}  // namespace

#define ICP_MOMENTS_NAME k_plane_moments_robust
#define ICP_MOMENTS_ROBUST true
#include "icp_plane_moments.inc"

void icp_launch_robust_apply (const icp_params &p, hipStream_t s)
{
    const uint32_t *area = icp_trim_area (p);
    if (p.fused) hipLaunchKernelGGL (k_trim_apply_robust<true>, dim3 (p.nb, p.batch), dim3 (64), 0, s, p, area, icp_tpr_magic (p.side));
    else hipLaunchKernelGGL (k_trim_apply_robust<false>, dim3 (2 * p.nwg, p.batch), dim3 (64), 0, s, p, area, icp_tpr_magic (p.side));
}

void icp_launch_plane_moments_robust (const icp_params &p, hipStream_t s, double *part, uint32_t nblk)
{
    const float4 *nrm = icp_normals_f (p), *grad = icp_color_grad_f (p);
    const float *kappa = icp_color_kappa (p);
    const dim3 grid (nblk, p.batch);
    if (icp_colored (p)) hipLaunchKernelGGL (k_plane_moments_robust<true>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, part, nblk, grad, kappa);
    else hipLaunchKernelGGL (k_plane_moments_robust<false>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, part, nblk, grad, kappa);
}
