// icp_symmetric.hip — symmetric ICP (icp_set_symmetric, include/icp_amd.h; Rusinkiewicz 2019: "A Symmetric Objective Function for
// ICP"): the per-pair terms of the plane system with the residual taken along the mean of the two frames' normals and the rotation split
// evenly between the frames, and their first tree level.  k_sym_moments<ROBUST> takes k_plane_moments' place in an iteration
// (icp_launch_p2pl_solve, icp_p2pl.hip) while the symmetric objective is in effect: the same launch shape, block tree and partial layout,
// so k_p2pl_finalize consumes its output as it stands (its increment rule is the symmetric one then).  The point-to-plane, colored,
// plane-to-plane and point-to-point kernels carry none of this code.  Built with -ffp-contract=off like every other translation unit:
// each expression below is evaluated exactly in the order it is written; tests/sym_ref.py restates them.
//
// What is this kernel's own, per pair in double (icp_plane_moments.h states the terms, G, g, the loss and the tree), N_Q =
// NORMALS_F[NN_ID.id], N_M = NORMALS_M[i], R = p.st[b].R (the cumulative rotation the search of this iteration used):
//   N_P = R N_M (plane_rot_normal);   o = (nqx npx + nqy npy) + nqz npz;   o < 0: N_P = -N_P (componentwise)
//   n = 0.5 (N_Q + N_P): (nqx + npx) * 0.5, ..      s = P + Q,  d = Q - P (componentwise)
//   c = s x n: (sy nz - sz ny, sz nx - sx nz, sx ny - sy nx)       J = (c, n)       r = (dx nx + dy ny) + dz nz
//   the products J_a J_b and J_a r;   G and g about A = s with B = d: point-to-plane's G with s in P's place, g = (s x d, d)
// ROBUST: sG2 = r r + mu ((dx dx + dy dy) + dz dz).
#include "icp_plane_moments.h"

template <bool ROBUST>
__global__ __launch_bounds__ (256) void k_sym_moments (icp_params p, const float4 *nrm, const float4 *nrm_m, double *part, uint32_t nblk)
{
    const uint32_t b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * ICP_P2PL_BLOCK + tid;
    const size_t o = (size_t) b * p.m;
    const uint32_t ic = min (i, p.m - 1u);
    const float4 f = p.PF[o + ic], q = p.PM[o + ic], nmf = nrm_m[o + ic];
    const uint32_t id = p.nn_id[o + ic].id;
    float Rf[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rf[k] = p.st[b].R[k];
    // (a converged registration: asked behind the pair's loads — in front of them the flag's round trip would come first)
    if (icp_pass_leaves (p, b)) return;                  // (block-uniform)
    double v[ICP_P2PL_TERMS];
#pragma unroll
    for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) v[t] = 0.0;
    if (i < p.m && f.w != 0.f) {
        const float4 nf = plane_finite_or_zero (id < p.m ? nrm[o + id] : make_float4 (0.f, 0.f, 0.f, 0.f)), nm = plane_finite_or_zero (nmf);
        const double w = (double) f.w, mu = (double) p.p2pl_mu;
        const double px = (double) q.x, py = (double) q.y, pz = (double) q.z;
        const double qx = (double) f.x, qy = (double) f.y, qz = (double) f.z;
        const double nqx = (double) nf.x, nqy = (double) nf.y, nqz = (double) nf.z;
        double np[3];
        plane_rot_normal (Rf, nm, np);
        const double od = (nqx * np[0] + nqy * np[1]) + nqz * np[2];
        if (od < 0.0) { np[0] = -np[0]; np[1] = -np[1]; np[2] = -np[2]; }
        const double nx = (nqx + np[0]) * 0.5, ny = (nqy + np[1]) * 0.5, nz = (nqz + np[2]) * 0.5;
        const double sx = px + qx, sy = py + qy, sz = pz + qz;
        const double dx = qx - px, dy = qy - py, dz = qz - pz;
        const double r = (dx * nx + dy * ny) + dz * nz;
        const double J[7] = { sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz, r };
        const plane_share S = plane_point_share (sx, sy, sz, dx, dy, dz, dx, dy, dz);
        const double wG = ROBUST ? plane_loss_of (p).omega (r * r + mu * ((dx * dx + dy * dy) + dz * dz)) : 1.0;
        plane_emit<ROBUST> (v, w, mu, wG, S, [&] (int a, int c) __attribute__ ((always_inline)) { return J[a] * J[c]; });
    }
    plane_block_tree (v, part, nblk, b);
}

void icp_launch_sym_moments (const icp_params &p, hipStream_t s, double *part, uint32_t nblk)
{
    const float4 *nrm = icp_normals_f (p), *nrm_m = icp_normals_m (p);
    const dim3 grid (nblk, p.batch);
    if (icp_robust (p)) hipLaunchKernelGGL (k_sym_moments<true>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, nrm_m, part, nblk);
    else hipLaunchKernelGGL (k_sym_moments<false>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, nrm_m, part, nblk);
}
