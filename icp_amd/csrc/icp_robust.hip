// icp_robust.hip — the robust loss (icp_set_robust_loss, include/icp_amd.h): every pair is down-weighted by the loss's IRLS weight
// omega (icp_robust_omega) of its own residual.  The kernels are the existing bodies with the loss switched on by a template argument:
// point-to-point weighs its pairs in the apply pass behind the search (k_trim_apply_robust<FUSED>: trim_apply<FUSED, true>,
// icp_trim_apply.h; with trimming on too, behind trimming's selection), the plane metrics in their moments
// (k_plane_moments_robust<COLORED>: plane_moments<COLORED, true>, icp_plane_moments.h; plane-to-plane and the symmetric objective carry
// the loss in their own kernels).  They are kernels of this translation unit so that icp_trim.hip and icp_p2pl.hip hold their loss-off
// kernels only.  The scale k is a device word (icp_robust_scale, found from icp_params), written in stream order by
// icp_set_robust_loss: a new k touches no captured graph.
#include "icp_trim_apply.h"
#include "icp_plane_moments.h"

namespace {

template <bool FUSED>
__global__ __launch_bounds__ (64) void k_trim_apply_robust (icp_params p, const uint32_t *area, uint32_t tpr_magic)
{
    trim_apply<FUSED, true> (p, area, tpr_magic);
}

}  // namespace

template <bool COLORED>
__global__ __launch_bounds__ (256) void k_plane_moments_robust (icp_params p, const float4 *nrm, double *part, uint32_t nblk, const float4 *grad,
                                                                const float *kappa_word)
{
    plane_moments<COLORED, true> (p, nrm, part, nblk, grad, kappa_word);
}

void icp_launch_robust_apply (const icp_params &p, hipStream_t s)
{
    const uint32_t *area = icp_words (p, ICP_AREA_TRIM).result;
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
