// icp_gicp.hip — Generalized ICP (icp_set_plane_to_plane, include/icp_amd.h; Segal, Haehnel, Thrun 2009: "plane-to-plane"): the per-pair
// terms of the plane system with the 3-vector residual weighed by (C_Q + C_P)^-1, and their first tree level.  k_gicp_moments<ROBUST>
// takes k_plane_moments' place in an iteration (icp_launch_p2pl_solve, icp_p2pl.hip) while plane-to-plane is in effect: the same launch
// shape, block tree and partial layout, so k_p2pl_finalize consumes its output as it stands.  The point-to-plane, colored and
// point-to-point kernels carry none of this code.  Built with -ffp-contract=off like every other translation unit: each expression
// below is evaluated exactly in the order it is written; tests/gicp_ref.py restates them.
//
// What is this kernel's own, per pair in double (icp_plane_moments.h states the terms, G, g, the loss and the tree), N_Q =
// NORMALS_F[NN_ID.id], N_M = NORMALS_M[i], R = p.st[b].R (the cumulative rotation the search of this iteration used), eps =
// *icp_gicp_eps (p):
//   N_P = R N_M (plane_rot_normal)
//   cov (n): nn = (nx nx + ny ny) + nz nz;  nn > 0 and finite: k = (1.0 - eps) / nn, C_ab = delta_ab - k (n_a n_b);  else C = I
//   S = C_Q + C_P (s00 s01 s02 s11 s12 s22);  cofactors c00 = s11 s22 - s12 s12, c01 = s02 s12 - s01 s22, c02 = s01 s12 - s02 s11,
//   c11 = s00 s22 - s02 s02, c12 = s01 s02 - s00 s12, c22 = s00 s11 - s01 s01;  det = (s00 c00 + s01 c01) + s02 c02;  M_ab = c_ab / det;
//   det not finite or not > 0: the pair contributes exact zeros
//   H = [-[P]x | I]: h0 = (0, -pz, py), h1 = (pz, 0, -px), h2 = (-py, px, 0), h3 .. h5 the unit vectors;  u_a = M h_a with the products
//   of h's structural zeros and ones dropped:
//     u_0r = M_r1 (-pz) + M_r2 py,  u_1r = M_r0 pz + M_r2 (-px),  u_2r = M_r0 (-py) + M_r1 px,  u_(3+c)r = M_rc
//     h_0 . u_b = (-pz) u_b1 + py u_b2,  h_1 . u_b = pz u_b0 + (-px) u_b2,  h_2 . u_b = (-py) u_b0 + px u_b1,  h_(3+c) . u_b = u_bc
//   the products: q_t = h_a . u_b (a <= b, row-major),  q_(21 + a) = (u_a0 dx + u_a1 dy) + u_a2 dz;   G and g about A = P with B = Q
// ROBUST: u_d = M d ((M_r0 dx + M_r1 dy) + M_r2 dz), sG2 = ((u_d0 dx + u_d1 dy) + u_d2 dz) + mu ((dx dx + dy dy) + dz dz).
#include "icp_plane_moments.h"

namespace {

// the covariance of a normal, upper triangle (c00 c01 c02 c11 c12 c22)
__device__ __forceinline__ void gicp_cov (double nx, double ny, double nz, double eps, double (&C)[6])
{
    const double nn = (nx * nx + ny * ny) + nz * nz;
    if (nn > 0.0 && isfinite (nn)) {
        const double k = (1.0 - eps) / nn;
        C[0] = 1.0 - k * (nx * nx); C[1] = 0.0 - k * (nx * ny); C[2] = 0.0 - k * (nx * nz);
        C[3] = 1.0 - k * (ny * ny); C[4] = 0.0 - k * (ny * nz);
        C[5] = 1.0 - k * (nz * nz);
    } else {
        C[0] = 1.0; C[1] = 0.0; C[2] = 0.0; C[3] = 1.0; C[4] = 0.0; C[5] = 1.0;
    }
}

}  // namespace

template <bool ROBUST>
__global__ __launch_bounds__ (256) void k_gicp_moments (icp_params p, const float4 *nrm, const float4 *nrm_m, double *part, uint32_t nblk,
                                                        const float *eps_word)
{
    const uint32_t b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * ICP_P2PL_BLOCK + tid;
    const size_t o = (size_t) b * p.m;
    const uint32_t ic = min (i, p.m - 1u);
    const float4 f = p.PF[o + ic], q = p.PM[o + ic], nmf = nrm_m[o + ic];
    const uint32_t id = p.nn_id[o + ic].id;
    const float epsf = *eps_word;
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
        const double w = (double) f.w, mu = (double) p.p2pl_mu, eps = (double) epsf;
        const double px = (double) q.x, py = (double) q.y, pz = (double) q.z;
        const double qx = (double) f.x, qy = (double) f.y, qz = (double) f.z;
        double np[3], CQ[6], CP[6];
        plane_rot_normal (Rf, nm, np);
        gicp_cov ((double) nf.x, (double) nf.y, (double) nf.z, eps, CQ);
        gicp_cov (np[0], np[1], np[2], eps, CP);
        const double s00 = CQ[0] + CP[0], s01 = CQ[1] + CP[1], s02 = CQ[2] + CP[2], s11 = CQ[3] + CP[3], s12 = CQ[4] + CP[4], s22 = CQ[5] + CP[5];
        const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
        const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
        const double det = (s00 * c00 + s01 * c01) + s02 * c02;
        if (det > 0.0 && isfinite (det)) {
            // M, symmetric, by rows
            const double M[3][3] = { { c00 / det, c01 / det, c02 / det }, { c01 / det, c11 / det, c12 / det }, { c02 / det, c12 / det, c22 / det } };
            const double npx = -px, npy = -py, npz = -pz;
            double u[6][3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                u[0][r] = M[r][1] * npz + M[r][2] * py;
                u[1][r] = M[r][0] * pz + M[r][2] * npx;
                u[2][r] = M[r][0] * npy + M[r][1] * px;
                u[3][r] = M[r][0]; u[4][r] = M[r][1]; u[5][r] = M[r][2];
            }
            const double dx = qx - px, dy = qy - py, dz = qz - pz;
            const plane_share S = plane_point_share (px, py, pz, qx, qy, qz, dx, dy, dz);
            double wG = 1.0;
            if constexpr (ROBUST) {
                const double ud0 = (M[0][0] * dx + M[0][1] * dy) + M[0][2] * dz;
                const double ud1 = (M[1][0] * dx + M[1][1] * dy) + M[1][2] * dz;
                const double ud2 = (M[2][0] * dx + M[2][1] * dy) + M[2][2] * dz;
                wG = plane_loss_of (p).omega (((ud0 * dx + ud1 * dy) + ud2 * dz) + mu * ((dx * dx + dy * dy) + dz * dz));
            }
            // h_a . u_c, and u_a . d for the residual's column
            plane_emit<ROBUST> (v, w, mu, wG, S, [&] (int a, int c) __attribute__ ((always_inline)) {
                return c == 6 ? (u[a][0] * dx + u[a][1] * dy) + u[a][2] * dz
                     : a == 0 ? npz * u[c][1] + py * u[c][2]
                     : a == 1 ? pz * u[c][0] + npx * u[c][2]
                     : a == 2 ? npy * u[c][0] + px * u[c][1]
                     : u[c][a - 3];
            });
        }
    }
    plane_block_tree (v, part, nblk, b);
}

void icp_launch_gicp_moments (const icp_params &p, hipStream_t s, double *part, uint32_t nblk)
{
    const float4 *nrm = icp_normals_f (p), *nrm_m = icp_normals_m (p);
    const float *eps = icp_gicp_eps (p);
    const dim3 grid (nblk, p.batch);
    if (icp_robust (p)) hipLaunchKernelGGL (k_gicp_moments<true>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, nrm_m, part, nblk, eps);
    else hipLaunchKernelGGL (k_gicp_moments<false>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, nrm_m, part, nblk, eps);
}
