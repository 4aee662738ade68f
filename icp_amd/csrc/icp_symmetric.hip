// icp_symmetric.hip — symmetric ICP (icp_set_symmetric, include/icp_amd.h; Rusinkiewicz 2019: "A Symmetric Objective Function for
// ICP"): the per-pair terms of the plane system with the residual taken along the mean of the two frames' normals and the rotation split
// evenly between the frames, and their first tree level.  k_sym_moments<ROBUST> takes k_plane_moments' place in an iteration
// (icp_launch_p2pl_solve, icp_p2pl.hip) while the symmetric objective is in effect: the same launch shape, block tree and partial layout,
// so k_p2pl_finalize consumes its output as it stands (its increment rule is the symmetric one then).  The point-to-plane, colored,
// plane-to-plane and point-to-point kernels carry none of this code.  Built with -ffp-contract=off like every other translation unit:
// each expression below is evaluated exactly in the order it is written; tests/sym_ref.py restates them.
//
// The 27 terms of pair i in double, w = PF.w, P = PM.xyz, Q = PF.xyz, N_Q = NORMALS_F[NN_ID.id], N_M = NORMALS_M[i] (a non-finite
// normal counts as zero), R = p.st[b].R (the cumulative rotation the search of this iteration used), all converted from float first:
//   N_P = R N_M: (R_a0 mx + R_a1 my) + R_a2 mz;   o = (nqx npx + nqy npy) + nqz npz;   o < 0: N_P = -N_P (componentwise)
//   n = 0.5 (N_Q + N_P): (nqx + npx) * 0.5, ..      s = P + Q,  d = Q - P (componentwise)
//   c = s x n: (sy nz - sz ny, sz nx - sx nz, sx ny - sy nx)       J = (c, n)
//   r = (dx nx + dy ny) + dz nz      ss = (sx sx + sy sy) + sz sz
//   G = point-to-plane's G with s in P's place: G00 = ss - sx sx, G01 = -(sx sy), .., G04 = -sz, G05 = sy, G13 = sz, G15 = -sx,
//       G23 = -sy, G24 = sx; the unit block and the zeros as there
//   g = (s x d, d): (sy dz - sz dy, sz dx - sx dz, sx dy - sy dx, dx, dy, dz)
//   term (a, b), a <= b, row-major:  w (J_a J_b + mu G_ab)         term 21 + a:  w (J_a r + mu g_a)
// w == 0 (no query, rejected, trimmed) selects exact zeros.  ROBUST: sG2 = r r + mu ((dx dx + dy dy) + dz dz), wG = omega (sG2 / k2); the
// terms are w (wG (..)), wG == 0 selecting an exact zero.  Then the halving tree over the block's ICP_P2PL_BLOCK pairs, exactly
// k_plane_moments'.
#include "icp_kernels.h"

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
    if (p.check && p.st[b].done) return;                 // (block-uniform)
    double v[ICP_P2PL_TERMS];
#pragma unroll
    for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) v[t] = 0.0;
    if (i < p.m) {
        if (f.w != 0.f) {
            float4 nf = id < p.m ? nrm[o + id] : make_float4 (0.f, 0.f, 0.f, 0.f), nm = nmf;
            if (!(isfinite (nf.x) && isfinite (nf.y) && isfinite (nf.z))) nf = make_float4 (0.f, 0.f, 0.f, 0.f);
            if (!(isfinite (nm.x) && isfinite (nm.y) && isfinite (nm.z))) nm = make_float4 (0.f, 0.f, 0.f, 0.f);
            const double w = (double) f.w, mu = (double) p.p2pl_mu;
            const double px = (double) q.x, py = (double) q.y, pz = (double) q.z;
            const double qx = (double) f.x, qy = (double) f.y, qz = (double) f.z;
            const double nqx = (double) nf.x, nqy = (double) nf.y, nqz = (double) nf.z;
            const double mx = (double) nm.x, my = (double) nm.y, mz = (double) nm.z;
            double npx = ((double) Rf[0] * mx + (double) Rf[1] * my) + (double) Rf[2] * mz;
            double npy = ((double) Rf[3] * mx + (double) Rf[4] * my) + (double) Rf[5] * mz;
            double npz = ((double) Rf[6] * mx + (double) Rf[7] * my) + (double) Rf[8] * mz;
            const double od = (nqx * npx + nqy * npy) + nqz * npz;
            if (od < 0.0) { npx = -npx; npy = -npy; npz = -npz; }
            const double nx = (nqx + npx) * 0.5, ny = (nqy + npy) * 0.5, nz = (nqz + npz) * 0.5;
            const double sx = px + qx, sy = py + qy, sz = pz + qz;
            const double dx = qx - px, dy = qy - py, dz = qz - pz;
            const double J[6] = { sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz };
            const double r = (dx * nx + dy * ny) + dz * nz;
            const double ss = (sx * sx + sy * sy) + sz * sz;
            const double G[21] = { ss - sx * sx, -(sx * sy), -(sx * sz), 0.0, -sz, sy,
                                   ss - sy * sy, -(sy * sz), sz, 0.0, -sx,
                                   ss - sz * sz, -sy, sx, 0.0,
                                   1.0, 0.0, 0.0,
                                   1.0, 0.0,
                                   1.0 };
            const double g[6] = { sy * dz - sz * dy, sz * dx - sx * dz, sx * dy - sy * dx, dx, dy, dz };
            [[maybe_unused]] double wG = 1.0;
            if constexpr (ROBUST) {
                const double k = (double) *icp_robust_scale (p), k2 = k * k;
                const double sG2 = r * r + mu * ((dx * dx + dy * dy) + dz * dz);
                wG = icp_robust_omega (icp_robust (p), sG2 / k2);
            }
            int t = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = a; c < 6; ++c, ++t) {
                    const double x = J[a] * J[c] + mu * G[t];
                    if constexpr (ROBUST) v[t] = w * (wG != 0.0 ? wG * x : 0.0);
                    else v[t] = w * x;
                }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double x = J[a] * r + mu * g[a];
                if constexpr (ROBUST) v[21 + a] = w * (wG != 0.0 ? wG * x : 0.0);
                else v[21 + a] = w * x;
            }
        }
    }
    __shared__ double s[ICP_P2PL_TERMS][128];
    if (tid >= 128u) {
#pragma unroll
        for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) s[t][tid - 128u] = v[t];
    }
    __syncthreads ();
    if (tid < 128u) {
#pragma unroll
        for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) v[t] = v[t] + s[t][tid];
    }
    __syncthreads ();
    if (tid >= 64u && tid < 128u) {
#pragma unroll
        for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) s[t][tid - 64u] = v[t];
    }
    __syncthreads ();
    if (tid >= 64u) return;
#pragma unroll
    for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) {
        double x = v[t] + s[t][tid];
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) x = x + __shfl_down (x, (unsigned) h, 64);
        v[t] = x;
    }
    if (tid == 0u) {
#pragma unroll
        for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) part[((size_t) b * ICP_P2PL_TERMS + t) * nblk + blockIdx.x] = v[t];
    }
}

void icp_launch_sym_moments (const icp_params &p, hipStream_t s, double *part, uint32_t nblk)
{
    const float4 *nrm = icp_normals_f (p), *nrm_m = icp_normals_m (p);
    const dim3 grid (nblk, p.batch);
    if (icp_robust (p)) hipLaunchKernelGGL (k_sym_moments<true>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, nrm_m, part, nblk);
    else hipLaunchKernelGGL (k_sym_moments<false>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, nrm_m, part, nblk);
}
