// icp_plane_moments.h — the per-pair algebra of the plane system and its first tree level, once, for the four moments kernels:
// k_plane_moments<COLORED> (icp_p2pl.hip) and k_plane_moments_robust<COLORED> (icp_robust.hip), which are plane_moments<COLORED, ROBUST>
// below behind a __global__ name each; k_gicp_moments<ROBUST> (icp_gicp.hip) and k_sym_moments<ROBUST> (icp_symmetric.hip), which keep
// what is their own and take the rest from here.  Also the intensity of a landmark, which k_color_grad_grid (icp_p2pl.hip) uses too.
// k_quality_pairs (icp_quality.hip: icp_evaluate) takes G from plane_point_share and the tree, over its 22 terms, from plane_block_tree.
// Every translation unit is built with -ffp-contract=off: each expression below is evaluated exactly in the order it is written;
// tests/p2pl_ref.py, colored_ref.py, robust_ref.py, gicp_ref.py and sym_ref.py restate them.
//
// The 27 terms of pair i in double (include/icp_amd.h), w = PF.w, P = PM.xyz, Q = PF.xyz, d = Q - P (componentwise), normals read as
// plane_finite_or_zero leaves them, everything converted from float first.  A metric gives its 27 products q and a point A:
//   term (a, b), a <= b, row-major (t = 0 .. 20):  w (q_t + mu G_ab)        term 21 + a:  w (q_(21 + a) + mu g_a)         (plane_emit)
//   G = [[aa I - A A^T, [A]x], [-[A]x, I]], aa = (ax ax + ay ay) + az az: G00 = aa - ax ax, G01 = -(ax ay), G02 = -(ax az),
//       G11 = aa - ay ay, G12 = -(ay az), G22 = aa - az az; G03 = 0, G04 = -az, G05 = ay, G13 = az, G14 = 0, G15 = -ax, G23 = -ay,
//       G24 = ax, G25 = 0; G33 = G44 = G55 = 1, G34 = G35 = G45 = 0
//   g = (A x B, d): A x B = (ay bz - az by, az bx - ax bz, ax by - ay bx)                                        (plane_point_share)
//   point-to-plane, colored, plane-to-plane: A = P, B = Q;   symmetric: A = s = P + Q, B = d
//   q of a Jacobian row J and a residual r:  q_t = J_a J_b,  q_(21 + a) = J_a r
// A robust loss (icp_set_robust_loss): with k = *icp_robust_scale (p), k2 = k k, wG = omega (sG2 / k2) (plane_loss; sG2 is the metric's),
//   term:  w (wG (q + mu G))       wG == 0 selects an exact zero for the bracket
// A photometric part (colored) with its own products qc and weight kc:  w ((q + mu G) + kc qc), with a loss w ((wG (..)) + kc qc),
// wC == 0 selecting an exact zero for kc qc.  w == 0 (no query, rejected, trimmed) and i >= m leave exact zeros.
// Then the halving tree over the block's ICP_P2PL_BLOCK pairs, x[i] += x[i + h] for h = 128 .. 1 (lanes: h = 32 .. 1 pair lane i with
// lane i + h, the same additions), and lane 0's store of the 27 block partials (plane_block_tree).
//
// plane_moments<COLORED, ROBUST> — point-to-plane: N = NORMALS_F[NN_ID.id],
//   c = P x N: (py nz - pz ny, pz nx - px nz, px ny - py nx)       J = (c, N)       r = (dx nx + dy ny) + dz nz
//   sG2 = r r + mu ((dx dx + dy dy) + dz dz)
// COLORED adds the photometric part: (dC, C_Q) = grad[NN_ID.id] (COLOR_GRAD_F), C_P = the intensity of M[i] (fp32), kappa =
// *kappa_word (icp_color_kappa):
//   dn = (dCx nx + dCy ny) + dCz nz,  t = dC - dn N (componentwise: dCx - dn nx, ..)          (the gradient in Q's tangent plane)
//   J_C = (P x t, t): (py tz - pz ty, pz tx - px tz, px ty - py tx, tx, ty, tz)
//   e = P - Q (componentwise),  r_C = C_P - (C_Q + ((tx ex + ty ey) + tz ez))
//   qc of J_C and r_C as q of J and r,  kc = kappa;   with a loss sC2 = kappa (r_C r_C),  wC = omega (sC2 / k2),  kc = kappa wC
#pragma once
#include <type_traits>
#include "icp_pair_rule.h"              // (icp_pass_leaves; icp_kernels.h)

namespace {

// the intensity of a landmark [x y z 1 r g b 1], fp32
__device__ __forceinline__ float intensity (float r, float g, float b) { return ((r + g) + b) / 3.f; }

// a normal or a colour gradient whose xyz is not all finite counts as zero (.w stays: the gradient's carries C_Q)
__device__ __forceinline__ float4 plane_finite_or_zero (float4 v)
{
    if (!(isfinite (v.x) && isfinite (v.y) && isfinite (v.z))) { v.x = 0.f; v.y = 0.f; v.z = 0.f; }
    return v;
}

// N_P = R N_M in double from nine floats: (R_a0 mx + R_a1 my) + R_a2 mz
__device__ __forceinline__ void plane_rot_normal (const float (&R)[9], float4 nm, double (&n)[3])
{
    const double mx = (double) nm.x, my = (double) nm.y, mz = (double) nm.z;
    n[0] = ((double) R[0] * mx + (double) R[1] * my) + (double) R[2] * mz;
    n[1] = ((double) R[3] * mx + (double) R[4] * my) + (double) R[5] * mz;
    n[2] = ((double) R[6] * mx + (double) R[7] * my) + (double) R[8] * mz;
}

// G about the point A and g = (A x B, d)
struct plane_share { double G[21], g[6]; };

__device__ __forceinline__ plane_share plane_point_share (double ax, double ay, double az, double bx, double by, double bz, double dx,
                                                          double dy, double dz)
{
    const double aa = (ax * ax + ay * ay) + az * az;
    return { { aa - ax * ax, -(ax * ay), -(ax * az), 0.0, -az, ay,
               aa - ay * ay, -(ay * az), az, 0.0, -ax,
               aa - az * az, -ay, ax, 0.0,
               1.0, 0.0, 0.0,
               1.0, 0.0,
               1.0 },
             { ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, dx, dy, dz } };
}

// the handle's robust loss: its kind and k2 = k k, k = *icp_robust_scale (p); omega (s2) is its weight of a squared residual s2
struct plane_loss {
    uint32_t kind;
    double k2;
    __device__ __forceinline__ double omega (double s2) const { return icp_robust_omega (kind, s2 / k2); }
};

__device__ __forceinline__ plane_loss plane_loss_of (const icp_params &p)
{
    const double k = (double) *icp_robust_scale (p);
    return { icp_robust (p), k * k };
}

// The 27 terms of a pair.  q (a, c) is the metric's product for term (a, c), c == 6 standing for the residual's column (term 21 + a);
// S is about the pair's point; pho (a, c), if given, is colored's photometric part kc qc of the same term.
template <bool ROBUST, class Q, class PHO = std::nullptr_t>
__device__ __forceinline__ void plane_emit (double (&v)[ICP_P2PL_TERMS], double w, double mu, [[maybe_unused]] double wG, const plane_share &S,
                                            Q q, [[maybe_unused]] PHO pho = nullptr)
{
    int t = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = a; c < 6; ++c, ++t) {
            double x = q (a, c) + mu * S.G[t];
            if constexpr (ROBUST) x = wG != 0.0 ? wG * x : 0.0;
            if constexpr (!std::is_same_v<PHO, std::nullptr_t>) x = x + pho (a, c);
            v[t] = w * x;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double x = q (a, 6) + mu * S.g[a];
        if constexpr (ROBUST) x = wG != 0.0 ? wG * x : 0.0;
        if constexpr (!std::is_same_v<PHO, std::nullptr_t>) x = x + pho (a, 6);
        v[21 + a] = w * x;
    }
}

// The halving tree over the block's 256 pairs and the store of its N partials of registration b (N = ICP_P2PL_TERMS for the plane
// system, ICP_QUALITY_TERMS for icp_quality.hip).  Every thread of the block calls it.
template <uint32_t N>
__device__ __forceinline__ void plane_block_tree (double (&v)[N], double *part, uint32_t nblk, uint32_t b)
{
    const uint32_t tid = threadIdx.x;
    __shared__ double s[N][128];
    if (tid >= 128u) {
#pragma unroll
        for (int t = 0; t < (int) N; ++t) s[t][tid - 128u] = v[t];
    }
    __syncthreads ();
    if (tid < 128u) {
#pragma unroll
        for (int t = 0; t < (int) N; ++t) v[t] = v[t] + s[t][tid];
    }
    __syncthreads ();
    if (tid >= 64u && tid < 128u) {
#pragma unroll
        for (int t = 0; t < (int) N; ++t) s[t][tid - 64u] = v[t];
    }
    __syncthreads ();
    if (tid >= 64u) return;
#pragma unroll
    for (int t = 0; t < (int) N; ++t) {
        double x = v[t] + s[t][tid];
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) x = x + __shfl_down (x, (unsigned) h, 64);
        v[t] = x;
    }
    if (tid == 0u) {
#pragma unroll
        for (int t = 0; t < (int) N; ++t) part[((size_t) b * N + t) * nblk + blockIdx.x] = v[t];
    }
}

// the body of k_plane_moments<COLORED> (ROBUST false) and k_plane_moments_robust<COLORED> (true)
template <bool COLORED, bool ROBUST>
__device__ __forceinline__ void plane_moments (icp_params p, const float4 *nrm, double *part, uint32_t nblk, const float4 *grad,
                                               const float *kappa_word)
{
    const uint32_t b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * ICP_P2PL_BLOCK + tid;
    const size_t o = (size_t) b * p.m;
    const uint32_t ic = min (i, p.m - 1u);
    const float4 f = p.PF[o + ic], q = p.PM[o + ic];
    const uint32_t id = p.nn_id[o + ic].id;
    // (colored: (r, g, b, 1) of the moving landmark, and kappa)
    const float4 mc = COLORED ? *reinterpret_cast<const float4 *> (p.M + (o + ic) * 8 + 4) : make_float4 (0.f, 0.f, 0.f, 0.f);
    const float kap = COLORED ? *kappa_word : 0.f;
    // (a converged registration: asked behind the pair's loads — in front of them the flag's round trip would come first)
    if (icp_pass_leaves (p, b)) return;                  // (block-uniform)
    double v[ICP_P2PL_TERMS];
#pragma unroll
    for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) v[t] = 0.0;
    if (i < p.m && f.w != 0.f) {
        const float4 nf = plane_finite_or_zero (id < p.m ? nrm[o + id] : make_float4 (0.f, 0.f, 0.f, 0.f));
        const double w = (double) f.w, mu = (double) p.p2pl_mu;
        const double px = (double) q.x, py = (double) q.y, pz = (double) q.z;
        const double qx = (double) f.x, qy = (double) f.y, qz = (double) f.z;
        const double nx = (double) nf.x, ny = (double) nf.y, nz = (double) nf.z;
        const double dx = qx - px, dy = qy - py, dz = qz - pz;
        const double r = (dx * nx + dy * ny) + dz * nz;
        const double J[7] = { py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz, r };
        const plane_share S = plane_point_share (px, py, pz, qx, qy, qz, dx, dy, dz);
        double kappa = 0.0, JC[7] = {};
        if constexpr (COLORED) {
            const float4 gf = plane_finite_or_zero (id < p.m ? grad[o + id] : make_float4 (0.f, 0.f, 0.f, 0.f));
            kappa = (double) kap;
            const double gx = (double) gf.x, gy = (double) gf.y, gz = (double) gf.z, cq = (double) gf.w;
            const double cp = (double) intensity (mc.x, mc.y, mc.z);
            const double dn = (gx * nx + gy * ny) + gz * nz;
            const double tx = gx - dn * nx, ty = gy - dn * ny, tz = gz - dn * nz;
            JC[0] = py * tz - pz * ty; JC[1] = pz * tx - px * tz; JC[2] = px * ty - py * tx; JC[3] = tx; JC[4] = ty; JC[5] = tz;
            const double ex = px - qx, ey = py - qy, ez = pz - qz;
            JC[6] = cp - (cq + ((tx * ex + ty * ey) + tz * ez));                     // r_C
        }
        double wG = 1.0, wC = 1.0;
        if constexpr (ROBUST) {
            const plane_loss L = plane_loss_of (p);
            wG = L.omega (r * r + mu * ((dx * dx + dy * dy) + dz * dz));
            if constexpr (COLORED) wC = L.omega (kappa * (JC[6] * JC[6]));
        }
        const double kc = ROBUST ? kappa * wC : kappa;
        const auto jj = [&] (int a, int c) __attribute__ ((always_inline)) { return J[a] * J[c]; };
        const auto pho = [&] (int a, int c) __attribute__ ((always_inline)) {
            const double y = kc * (JC[a] * JC[c]);
            return ROBUST ? (wC != 0.0 ? y : 0.0) : y;
        };
        if constexpr (COLORED) plane_emit<ROBUST> (v, w, mu, wG, S, jj, pho);
        else plane_emit<ROBUST> (v, w, mu, wG, S, jj);
    }
    plane_block_tree (v, part, nblk, b);
}

}  // namespace
