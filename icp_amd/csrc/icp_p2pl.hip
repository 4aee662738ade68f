// icp_p2pl.hip — the plane system: point-to-plane ICP (icp_set_error_metric, icp_set_normals) and colored ICP (ICP_METRIC_COLORED,
// icp_set_color_weight; Park, Zhou, Koltun 2017).  include/icp_amd.h states both rules.
//
// An iteration with either metric on is: the search stage (icp_route_of, icp_kernels.hip), which stores PF (matched fixed xyz, weight) and PM
// (transformed moving xyz) every time — rejection and trimming have put their zeros into PF.w already —; k_plane_moments<COLORED> (icp_plane_moments.h), the
// 27 terms of the linearised 6 x 6 system per pair in double (colored: plus kappa times a photometric term; a robust loss: each part
// weighed by the loss's omega of its residual) and their tree over blocks
// of ICP_P2PL_BLOCK pairs; k_p2pl_finalize, one workgroup per registration: the tree over the block partials, LDL^T in one lane, the
// increment composed with icp_compose's arithmetic and checked with icp_check_converged.  k_normals_grid computes NORMALS_F from F
// behind buildRBC (ICP_NORMALS_GRID; with plane-to-plane or the symmetric objective on, whose moments are icp_gicp.hip's and
// icp_symmetric.hip's, also NORMALS_M from M), and with the colored metric k_color_grad_grid computes COLOR_GRAD_F behind it.  None of the
// point-to-point kernels carries any of this code; the translation unit is built with -ffp-contract=off like every other, so each
// expression below is evaluated exactly in the order it is written.
#include "icp_plane_moments.h"          // (plane_moments, intensity; icp_pair_rule.h)
#include "icp_normal_rule.h"            // (icp_grid_normal)
#include "icp_ldlt.h"                   // (ldlt_solve)

// NORMALS_F of the fixed set (src = F), read as a row-major grid p.nrm_grid wide (m % width == 0: icp_build_rbc checks it); with
// plane-to-plane or the symmetric objective on also NORMALS_M of the moving set (src = M).  One thread per point, grid.y = registration counted from src and nrm.
// The rule: icp_grid_normal (icp_normal_rule.h).
__global__ __launch_bounds__ (256) void k_normals_grid (icp_params p, const float *src, float4 *nrm)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.m) return;
    const uint32_t W = p.nrm_grid, x = i % W, y = i / W, H = p.m / W;
    const float *F = src + (size_t) b * p.m * 8;
    auto at = [&] (uint32_t j) { const float *r = F + (size_t) j * 8; return make_float3 (r[0], r[1], r[2]); };
    const float3 zero = make_float3 (0.f, 0.f, 0.f);
    // (i + 1 < m, y + 1 < H: no read beyond the set even if the width did not divide m — the host refuses that, ICP_ESTATE)
    const bool hasl = x > 0u, hasr = x + 1u < W && i + 1u < p.m, hasu = y > 0u, hasd = y + 1u < H;
    const float4 n = icp_grid_normal (at (i), hasl ? at (i - 1u) : zero, hasl, hasr ? at (i + 1u) : zero, hasr,
                                      hasu ? at (i - W) : zero, hasu, hasd ? at (i + W) : zero, hasd);
    nrm[(size_t) b * p.m + i] = n;
}

// COLOR_GRAD_F of the fixed set, F read as a row-major grid p.nrm_grid wide (m % width == 0: the host checks it), n = NORMALS_F just
// computed.  One thread per point, grid.y = registration.  For a valid centre p with n != 0, over the valid points p' of the 3 x 3
// window (row-major, the centre excluded), in double from the float inputs:
//   v = p' - p,  vn = (vx nx + vy ny) + vz nz,  u = v - vn n (componentwise: vx - vn nx, ..),  dC = C(p') - C(p),
//   A_ab = A_ab + u_a u_b  (A00, A01, A02, A11, A12, A22),   b_a = b_a + u_a dC,   K = K + 1      (window order, from zeros)
// then with k = K, kn = (k nx, k ny, k nz):  A_ab = A_ab + kn_a kn_b;  ldlt_solve<3>, x rounded to float once.  g = 0 when K < 3, the
// centre is invalid, n = 0 or a pivot fails; .w = C(p) always.
__global__ __launch_bounds__ (256) void k_color_grad_grid (icp_params p, const float4 *nrm, float4 *grad)
{
    const uint32_t b = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.m) return;
    const uint32_t W = p.nrm_grid, x = i % W, y = i / W, H = p.m / W;
    const float *F = p.F + (size_t) b * p.m * 8;
    const float *c = F + (size_t) i * 8;
    const float cx = c[0], cy = c[1], cz = c[2], Cc = intensity (c[4], c[5], c[6]);
    const float4 n = nrm[(size_t) b * p.m + i];
    float4 out = make_float4 (0.f, 0.f, 0.f, Cc);
    if (icp_point_valid (cx, cy, cz) && !(n.x == 0.f && n.y == 0.f && n.z == 0.f)) {
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
                if (!icp_point_valid (qx, qy, qz)) continue;
                const double vx = (double) qx - px, vy = (double) qy - py, vz = (double) qz - pz;
                const double vn = (vx * nx + vy * ny) + vz * nz;
                const double ux = vx - vn * nx, uy = vy - vn * ny, uz = vz - vn * nz;
                const double dC = (double) intensity (q[4], q[5], q[6]) - pc;
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
            const double A[3][3] = { { A00, A01, A02 }, { A01, A11, A12 }, { A02, A12, A22 } }, bb[3] = { b0, b1, b2 };
            double xv[3];
            bool ok;
            ldlt_solve (A, bb, xv, ok);
            if (ok) { out.x = (float) xv[0]; out.y = (float) xv[1]; out.z = (float) xv[2]; }
        }
    }
    grad[(size_t) b * p.m + i] = out;
}

// the 27 terms per pair and their block tree with the loss off (icp_plane_moments.h)
template <bool COLORED>
__global__ __launch_bounds__ (256) void k_plane_moments (icp_params p, const float4 *nrm, double *part, uint32_t nblk, const float4 *grad,
                                                         const float *kappa_word)
{
    plane_moments<COLORED, false> (p, nrm, part, nblk, grad, kappa_word);
}

#define P2PL_LDS 4096u           // doubles of the finalize's tree buffer (nblk <= 4096: m <= 2^20)

// One workgroup per registration: the halving tree over the block partials zero-padded to P = 2^ceil(log2 nblk), as many terms at a time
// as the LDS buffer holds; then lane 0: ldlt_solve<6>, the increment (point-to-plane's, or the symmetric objective's while icp_sym (p)),
// the composition and the check.
__global__ __launch_bounds__ (256) void k_p2pl_finalize (icp_params p, const double *part, double *sys, uint32_t nblk, uint32_t P)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    icp_reg_state *st = p.st + b;
    __shared__ double s[P2PL_LDS];
    __shared__ double s_sum[ICP_P2PL_TERMS];
    const uint32_t lgP = 31u - (uint32_t) __builtin_clz (P), tc = min (ICP_P2PL_TERMS, P2PL_LDS / P);
    const double *pb = part + (size_t) b * ICP_P2PL_TERMS * nblk;
    // the transform before the step, in lane 0's registers from the start (the composition then waits for no load)
    float Tprev[8], Rprev[9];
    if (tid == 0u) {
#pragma unroll
        for (int k = 0; k < 8; ++k) Tprev[k] = st->T[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rprev[k] = st->R[k];
    }
    for (uint32_t t0 = 0; t0 < ICP_P2PL_TERMS; t0 += tc) {
        const uint32_t nt = min (tc, ICP_P2PL_TERMS - t0), n = nt << lgP;
        // (every load of the pass in flight at once: at most P2PL_LDS / 256 per lane)
        double x[P2PL_LDS / 256u];
#pragma unroll
        for (uint32_t u = 0; u < P2PL_LDS / 256u; ++u) {
            const uint32_t j = tid + 256u * u, t = j >> lgP, i = j & (P - 1u);
            x[u] = (j < n && i < nblk) ? pb[(size_t) (t0 + t) * nblk + i] : 0.0;
        }
        // (a converged registration: asked behind the first loads)
        if (t0 == 0u && p.check && st->done) return;     // (block-uniform)
#pragma unroll
        for (uint32_t u = 0; u < P2PL_LDS / 256u; ++u) {
            const uint32_t j = tid + 256u * u;
            if (j < n) s[j] = x[u];
        }
        __syncthreads ();
        for (uint32_t lh = lgP; lh-- > 0u;) {
            const uint32_t h = 1u << lh;
            for (uint32_t j = tid; j < (nt << lh); j += 256u) {
                const uint32_t t = j >> lh, i = j & (h - 1u);
                s[(t << lgP) + i] = s[(t << lgP) + i] + s[(t << lgP) + i + h];
            }
            __syncthreads ();
        }
        if (tid < nt) s_sum[t0 + tid] = s[tid << lgP];
        __syncthreads ();
    }
    if (tid != 0u) return;

    // A (symmetric, from the upper triangle) and b
    double A[6][6], bb[6];
    {
        int t = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c, ++t) { A[a][c] = s_sum[t]; A[c][a] = s_sum[t]; }
#pragma unroll
        for (int a = 0; a < 6; ++a) bb[a] = s_sum[21 + a];
    }
    double x[6];
    bool ok;
    ldlt_solve (A, bb, x, ok);

    double *sb = sys + (size_t) b * ICP_P2PL_SYS;
#pragma unroll
    for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) sb[t] = s_sum[t];
    sb[ICP_P2PL_TERMS] = ok ? 1.0 : 0.0;

    if (p.st_prev) {
#pragma unroll
        for (int k = 0; k < 8; ++k) p.st_prev[b].T[k] = Tprev[k];
    }
    float Tk[8], Tn[8], Rn[9], Rk[9];
    if (ok) {
        if (icp_sym (p)) {
            // the symmetric objective (icp_set_symmetric): x = (a, t) with half the rotation applied to each frame, the step Rot o Trans o Rot.
            // qk = (a, 1) / |(a, 1)|: the rotation by 2 theta about a, tan theta = |a|;  tk = R_a (cos theta t), R_a the rotation by theta,
            // by Rodrigues' formula with c = cos theta: c2 t + c2 (a x t) + a ((a . t) c3 / (1 + c));  sk = 1
            const double ax = x[0], ay = x[1], az = x[2], tx = x[3], ty = x[4], tz = x[5];
            const double aa = (ax * ax + ay * ay) + az * az;
            const double c = 1.0 / sqrt (aa + 1.0);
            Tk[0] = (float) (ax * c); Tk[1] = (float) (ay * c); Tk[2] = (float) (az * c); Tk[3] = (float) c;
            const double ux = ay * tz - az * ty, uy = az * tx - ax * tz, uz = ax * ty - ay * tx;
            const double at = (ax * tx + ay * ty) + az * tz;
            const double c2 = c * c;
            const double k3 = (c2 * c) / (1.0 + c);
            Tk[4] = (float) ((c2 * tx + c2 * ux) + ax * (at * k3));
            Tk[5] = (float) ((c2 * ty + c2 * uy) + ay * (at * k3));
            Tk[6] = (float) ((c2 * tz + c2 * uz) + az * (at * k3));
            Tk[7] = 1.f;
        } else {
            // qk = (w/2, 1) / |(w/2, 1)| in double, rounded to float; tk = (float) tau; sk = 1
            const double hx = x[0] * 0.5, hy = x[1] * 0.5, hz = x[2] * 0.5;
            const double inv = 1.0 / sqrt (((hx * hx + hy * hy) + hz * hz) + 1.0);
            Tk[0] = (float) (hx * inv); Tk[1] = (float) (hy * inv); Tk[2] = (float) (hz * inv); Tk[3] = (float) inv;
            Tk[4] = (float) x[3]; Tk[5] = (float) x[4]; Tk[6] = (float) x[5]; Tk[7] = 1.f;
        }
        icp_compose_pure (Tprev, Rprev, Tk, nullptr, 0, Tn, Rn, Rk);            // (icp_compose's arithmetic, registers in and out)
    } else {
        float S[11], means[8];
        int iters = 0;
        icp_identity_step (Tprev, Rprev, S, means, Tk, Tn, Rn, Rk, iters);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { st->T[k] = Tn[k]; st->Tk[k] = Tk[k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) { st->R[k] = Rn[k]; st->Rk[k] = Rk[k]; }
    st->pm_iters = 0u;
    st->k = st->k + 1u;
    if (p.check && icp_check_converged (Tk, p.tan_half_thr, p.trans_thr)) st->done = 1u;
}

void icp_launch_p2pl_solve (const icp_params &p, hipStream_t s)
{
    const uint32_t nblk = icp_p2pl_nblk (p.m);
    uint32_t P = 1u; while (P < nblk) P <<= 1;
    double *sys = icp_p2pl_area (p), *part = icp_p2pl_part (p);
    const float4 *nrm = icp_normals_f (p), *grad = icp_color_grad_f (p);
    const float *kappa = icp_color_kappa (p);
    const dim3 grid (nblk, p.batch);
    if (icp_gicp (p)) icp_launch_gicp_moments (p, s, part, nblk);                  // (icp_gicp.hip: plane-to-plane, with or without a robust loss)
    else if (icp_sym (p)) icp_launch_sym_moments (p, s, part, nblk);               // (icp_symmetric.hip: the symmetric objective, likewise)
    else if (icp_robust (p)) icp_launch_plane_moments_robust (p, s, part, nblk);   // (icp_robust.hip)
    else if (icp_colored (p)) hipLaunchKernelGGL (k_plane_moments<true>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, part, nblk, grad, kappa);
    else hipLaunchKernelGGL (k_plane_moments<false>, grid, dim3 (ICP_P2PL_BLOCK), 0, s, p, nrm, part, nblk, grad, kappa);
    hipLaunchKernelGGL (k_p2pl_finalize, dim3 (p.batch), dim3 (256), 0, s, p, (const double *) part, sys, nblk, P);
}

void icp_launch_normals_grid (const icp_params &p, hipStream_t s)
{
    const dim3 grid ((p.m + 255u) / 256u, p.batch);
    hipLaunchKernelGGL (k_normals_grid, grid, dim3 (256), 0, s, p, p.F, icp_normals_f (p));
    // (the intensity gradients need the normals just computed)
    if (icp_colored (p)) hipLaunchKernelGGL (k_color_grad_grid, grid, dim3 (256), 0, s, p, (const float4 *) icp_normals_f (p), icp_color_grad_f (p));
    if (icp_moving_normals (p)) icp_launch_normals_m (p, s, 0u, p.batch);
}

// plane-to-plane, symmetric or normal rejection with ICP_NORMALS_GRID: NORMALS_M of registrations b0 .. b0 + nb - 1 from M, by the same kernel
void icp_launch_normals_m (const icp_params &p, hipStream_t s, uint32_t b0, uint32_t nb)
{
    const dim3 grid ((p.m + 255u) / 256u, nb);
    hipLaunchKernelGGL (k_normals_grid, grid, dim3 (256), 0, s, p, p.M + (size_t) b0 * p.m * 8, icp_normals_m (p) + (size_t) b0 * p.m);
}
