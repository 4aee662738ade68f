// icp_color.hip — colored ICP (ICP_METRIC_COLORED, icp_set_color_weight: include/icp_amd.h states the rule; Park, Zhou, Koltun 2017).
//
// The point-to-plane system (icp_p2pl.hip) plus kappa times a linearised photometric residual per pair, built from the intensity
// gradient of the fixed frame in the tangent plane of the matched fixed point.  An iteration is the point-to-plane one with
// k_color_moments in place of k_p2pl_moments: the same 27 terms per pair, the same block partials, then the unchanged k_p2pl_finalize
// (icp_launch_p2pl_solve picks the moments).  k_color_grad_grid computes COLOR_GRAD_F behind k_normals_grid in buildRBC
// (ICP_NORMALS_GRID with the colored metric).  Built with -ffp-contract=off like every other unit: each expression below is evaluated
// exactly in the order it is written.
#include "icp_kernels.h"

namespace {

// a grid point takes part when its xyz is finite and not the origin (the rule of k_normals_grid)
__device__ __forceinline__ bool cg_valid (float x, float y, float z)
{
    return isfinite (x) && isfinite (y) && isfinite (z) && !(x == 0.f && y == 0.f && z == 0.f);
}

// the intensity of a landmark [x y z 1 r g b 1], fp32
__device__ __forceinline__ float cg_intensity (float r, float g, float b) { return ((r + g) + b) / 3.f; }

}  // namespace

// COLOR_GRAD_F of the fixed set, F read as a row-major grid p.nrm_grid wide (m % width == 0: the host checks it), n = NORMALS_F just
// computed.  One thread per point, grid.y = registration.  For a valid centre p with n != 0, over the valid points p' of the 3 x 3
// window (row-major, the centre excluded), in double from the float inputs:
//   v = p' - p,  vn = (vx nx + vy ny) + vz nz,  u = v - vn n (componentwise: vx - vn nx, ..),  dC = C(p') - C(p),
//   A_ab = A_ab + u_a u_b  (A00, A01, A02, A11, A12, A22),   b_a = b_a + u_a dC,   K = K + 1      (window order, from zeros)
// then with k = K, kn = (k nx, k ny, k nz):  A_ab = A_ab + kn_a kn_b;  LDL^T as k_p2pl_finalize's (the same pivot test), x rounded
// to float once.  g = 0 when K < 3, the centre is invalid, n = 0 or a pivot fails; .w = C(p) always.
__global__ __launch_bounds__ (256) void k_color_grad_grid (icp_params p, const float4 *nrm, float4 *grad)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.m) return;
    const uint32_t W = p.nrm_grid, x = i % W, y = i / W, H = p.m / W;
    const float *F = p.F + (size_t) b * p.m * 8;
    const float *c = F + (size_t) i * 8;
    const float cx = c[0], cy = c[1], cz = c[2], Cc = cg_intensity (c[4], c[5], c[6]);
    const float4 n = nrm[(size_t) b * p.m + i];
    float4 out = make_float4 (0.f, 0.f, 0.f, Cc);
    if (cg_valid (cx, cy, cz) && !(n.x == 0.f && n.y == 0.f && n.z == 0.f)) {
        const double nx = (double) n.x, ny = (double) n.y, nz = (double) n.z;
        const double px = (double) cx, py = (double) cy, pz = (double) cz, pc = (double) Cc;
        double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        uint32_t K = 0u;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dx == 0 && dy == 0) continue;
                const int xx = (int) x + dx, yy = (int) y + dy;
                if (xx < 0 || xx >= (int) W || yy < 0 || yy >= (int) H) continue;
                const uint32_t j = (uint32_t) yy * W + (uint32_t) xx;
                if (j >= p.m) continue;                      // (no read beyond the set even if the width did not divide m)
                const float *q = F + (size_t) j * 8;
                const float qx = q[0], qy = q[1], qz = q[2];
                if (!cg_valid (qx, qy, qz)) continue;
                const double vx = (double) qx - px, vy = (double) qy - py, vz = (double) qz - pz;
                const double vn = (vx * nx + vy * ny) + vz * nz;
                const double ux = vx - vn * nx, uy = vy - vn * ny, uz = vz - vn * nz;
                const double dC = (double) cg_intensity (q[4], q[5], q[6]) - pc;
                A00 = A00 + ux * ux; A01 = A01 + ux * uy; A02 = A02 + ux * uz;
                A11 = A11 + uy * uy; A12 = A12 + uy * uz; A22 = A22 + uz * uz;
                b0 = b0 + ux * dC; b1 = b1 + uy * dC; b2 = b2 + uz * dC;
                ++K;
            }
        }
        if (K >= 3u) {
            const double k = (double) K, kx = k * nx, ky = k * ny, kz = k * nz;
            A00 = A00 + kx * kx; A01 = A01 + kx * ky; A02 = A02 + kx * kz;
            A11 = A11 + ky * ky; A12 = A12 + ky * kz; A22 = A22 + kz * kz;
            // LDL^T column by column (k_p2pl_finalize's order): e_jk = L_jk d_k, d_j = A_jj - e_j0 L_j0 - ..,
            // L_ij = (A_ij - L_i0 e_j0 - ..) / d_j; singular when a pivot is not finite or d_j <= 1e-12 A_jj
            const double A[3][3] = { { A00, A01, A02 }, { A01, A11, A12 }, { A02, A12, A22 } }, bb[3] = { b0, b1, b2 };
            double L[3][3], E[3][3], d[3];
            bool ok = true;
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
                double v = A[jj][jj];
#pragma unroll
                for (int kk = 0; kk < jj; ++kk) v = v - E[jj][kk] * L[jj][kk];
                d[jj] = v;
                if (!isfinite (v) || v <= 1e-12 * A[jj][jj]) ok = false;
#pragma unroll
                for (int ii = jj + 1; ii < 3; ++ii) {
                    double u = A[ii][jj];
#pragma unroll
                    for (int kk = 0; kk < jj; ++kk) u = u - L[ii][kk] * E[jj][kk];
                    L[ii][jj] = u / v;
                    E[ii][jj] = L[ii][jj] * v;
                }
            }
            double yv[3], xv[3];
#pragma unroll
            for (int ii = 0; ii < 3; ++ii) {
                double u = bb[ii];
#pragma unroll
                for (int kk = 0; kk < ii; ++kk) u = u - L[ii][kk] * yv[kk];
                yv[ii] = u;
            }
#pragma unroll
            for (int ii = 2; ii >= 0; --ii) {
                double u = yv[ii] / d[ii];
#pragma unroll
                for (int kk = ii + 1; kk < 3; ++kk) u = u - L[kk][ii] * xv[kk];
                xv[ii] = u;
            }
            if (ok) { out.x = (float) xv[0]; out.y = (float) xv[1]; out.z = (float) xv[2]; }
        }
    }
    grad[(size_t) b * p.m + i] = out;
}

// The 27 terms of pair i (k_p2pl_moments' quantities and order, include/icp_amd.h; tests/colored_ref.py restates them), plus the
// photometric ones.  (d, C_Q) = COLOR_GRAD_F[NN_ID.id] (a non-finite d counts as zero), C_P = the intensity of M[i] (fp32), kappa =
// the device word icp_color_kappa; in double from the float inputs:
//   dn = (dx nx + dy ny) + dz nz,  t = d - dn N (componentwise: dx - dn nx, ..)          (the gradient in Q's tangent plane)
//   J_C = (P x t, t): (py tz - pz ty, pz tx - px tz, px ty - py tx, tx, ty, tz)
//   e = P - Q (componentwise),  r_C = C_P - (C_Q + ((tx ex + ty ey) + tz ez))
//   term (a, b), a <= b:  w ((J_a J_b + mu G_ab) + kappa (J_Ca J_Cb))        term 21 + a:  w ((J_a r + mu g_a) + kappa (J_Ca r_C))
// w == 0 selects exact zeros.  Then k_p2pl_moments' halving tree over the block's ICP_P2PL_BLOCK pairs and the same partials layout.
__global__ __launch_bounds__ (256) void k_color_moments (icp_params p, const float4 *nrm, const float4 *grad, const float *kappa_word,
                                                         double *part, uint32_t nblk)
{
    const uint32_t b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * ICP_P2PL_BLOCK + tid;
    const size_t o = (size_t) b * p.m;
    const uint32_t ic = min (i, p.m - 1u);
    const float4 f = p.PF[o + ic], q = p.PM[o + ic];
    const uint32_t id = p.nn_id[o + ic].id;
    const float4 mc = *reinterpret_cast<const float4 *> (p.M + (o + ic) * 8 + 4);      // (r, g, b, 1) of the moving landmark
    const float kap = *kappa_word;
    if (p.check && p.st[b].done) return;                 // (block-uniform)
    double v[ICP_P2PL_TERMS];
#pragma unroll
    for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) v[t] = 0.0;
    if (i < p.m) {
        if (f.w != 0.f) {
            float4 nf = id < p.m ? nrm[o + id] : make_float4 (0.f, 0.f, 0.f, 0.f);
            if (!(isfinite (nf.x) && isfinite (nf.y) && isfinite (nf.z))) nf = make_float4 (0.f, 0.f, 0.f, 0.f);
            float4 gf = id < p.m ? grad[o + id] : make_float4 (0.f, 0.f, 0.f, 0.f);
            if (!(isfinite (gf.x) && isfinite (gf.y) && isfinite (gf.z))) { gf.x = 0.f; gf.y = 0.f; gf.z = 0.f; }
            const double w = (double) f.w, mu = (double) p.p2pl_mu, kappa = (double) kap;
            const double px = (double) q.x, py = (double) q.y, pz = (double) q.z;
            const double qx = (double) f.x, qy = (double) f.y, qz = (double) f.z;
            const double nx = (double) nf.x, ny = (double) nf.y, nz = (double) nf.z;
            const double J[6] = { py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz };
            const double dx = qx - px, dy = qy - py, dz = qz - pz;
            const double r = (dx * nx + dy * ny) + dz * nz;
            const double pp = (px * px + py * py) + pz * pz;
            const double G[21] = { pp - px * px, -(px * py), -(px * pz), 0.0, -pz, py,
                                   pp - py * py, -(py * pz), pz, 0.0, -px,
                                   pp - pz * pz, -py, px, 0.0,
                                   1.0, 0.0, 0.0,
                                   1.0, 0.0,
                                   1.0 };
            const double g[6] = { py * qz - pz * qy, pz * qx - px * qz, px * qy - py * qx, dx, dy, dz };
            const double gx = (double) gf.x, gy = (double) gf.y, gz = (double) gf.z, cq = (double) gf.w;
            const double cp = (double) cg_intensity (mc.x, mc.y, mc.z);
            const double dn = (gx * nx + gy * ny) + gz * nz;
            const double tx = gx - dn * nx, ty = gy - dn * ny, tz = gz - dn * nz;
            const double JC[6] = { py * tz - pz * ty, pz * tx - px * tz, px * ty - py * tx, tx, ty, tz };
            const double ex = px - qx, ey = py - qy, ez = pz - qz;
            const double rc = cp - (cq + ((tx * ex + ty * ey) + tz * ez));
            int t = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = a; c < 6; ++c, ++t) v[t] = w * ((J[a] * J[c] + mu * G[t]) + kappa * (JC[a] * JC[c]));
#pragma unroll
            for (int a = 0; a < 6; ++a) v[21 + a] = w * ((J[a] * r + mu * g[a]) + kappa * (JC[a] * rc));
        }
    }
    // (k_p2pl_moments' tree: LDS for h = 128, 64, then the wave's shuffles — the same additions in the same order)
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

void icp_launch_color_moments (const icp_params &p, hipStream_t s, double *part, uint32_t nblk)
{
    hipLaunchKernelGGL (k_color_moments, dim3 (nblk, p.batch), dim3 (ICP_P2PL_BLOCK), 0, s, p, (const float4 *) icp_normals_f (p),
                        (const float4 *) icp_color_grad_f (p), (const float *) icp_color_kappa (p), part, nblk);
}

void icp_launch_color_grad_grid (const icp_params &p, hipStream_t s)
{
    hipLaunchKernelGGL (k_color_grad_grid, dim3 ((p.m + 255u) / 256u, p.batch), dim3 (256), 0, s, p, (const float4 *) icp_normals_f (p),
                        icp_color_grad_f (p));
}
