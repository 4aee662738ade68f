// icp_plane_moments.inc — the per-pair terms of the plane system and their first tree level as a kernel template (include/icp_amd.h:
// point-to-plane, colored, the robust loss), included behind icp_plane_moments.h with ICP_MOMENTS_NAME and ICP_MOMENTS_ROBUST defined:
// icp_p2pl.hip as k_plane_moments<COLORED> (false), icp_robust.hip as k_plane_moments_robust<COLORED> (true).  One body; the loss-off
// kernel is, instruction for instruction, the one the plane metrics had, and the robust kernels live in a translation unit of their own.
// The 27 terms of pair i in double (include/icp_amd.h; tests/p2pl_ref.py and tests/colored_ref.py restate them), w = PF.w, P = PM.xyz,
// Q = PF.xyz, N = NORMALS_F[NN_ID.id] (a non-finite normal counts as zero), all converted from float first:
//   c = P x N: (py nz - pz ny, pz nx - px nz, px ny - py nx)       J = (c, N)
//   d = Q - P (componentwise)     r = (dx nx + dy ny) + dz nz      pp = (px px + py py) + pz pz
//   G = [[pp I - P P^T, [P]x], [-[P]x, I]]: G00 = pp - px px, G01 = -(px py), G02 = -(px pz), G11 = pp - py py, G12 = -(py pz),
//       G22 = pp - pz pz; G03 = 0, G04 = -pz, G05 = py, G13 = pz, G14 = 0, G15 = -px, G23 = -py, G24 = px, G25 = 0;
//       G33 = G44 = G55 = 1, G34 = G35 = G45 = 0
//   g = (P x Q, d): P x Q = (py qz - pz qy, pz qx - px qz, px qy - py qx)
//   term (a, b), a <= b, row-major:  w (J_a J_b + mu G_ab)         term 21 + a:  w (J_a r + mu g_a)
// COLORED adds the photometric terms: (d, C_Q) = grad[NN_ID.id] (COLOR_GRAD_F; a non-finite d counts as zero), C_P = the intensity of
// M[i] (fp32), kappa = *kappa_word (icp_color_kappa):
//   dn = (dx nx + dy ny) + dz nz,  t = d - dn N (componentwise: dx - dn nx, ..)          (the gradient in Q's tangent plane)
//   J_C = (P x t, t): (py tz - pz ty, pz tx - px tz, px ty - py tx, tx, ty, tz)
//   e = P - Q (componentwise),  r_C = C_P - (C_Q + ((tx ex + ty ey) + tz ez))
//   term (a, b), a <= b:  w ((J_a J_b + mu G_ab) + kappa (J_Ca J_Cb))        term 21 + a:  w ((J_a r + mu g_a) + kappa (J_Ca r_C))
// w == 0 (no query, rejected, trimmed) selects exact zeros.  ROBUST (icp_set_robust_loss): with k = *icp_robust_scale (p), k2 = k k and omega of
// the handle's loss (icp_robust_omega),
//   sG2 = r r + mu ((dx dx + dy dy) + dz dz),  wG = omega (sG2 / k2);   colored: sC2 = kappa (r_C r_C),  wC = omega (sC2 / k2)
//   term (a, b):  w ((wG (J_a J_b + mu G_ab)) + (kappa wC) (J_Ca J_Cb))     term 21 + a:  w ((wG (J_a r + mu g_a)) + (kappa wC) (J_Ca r_C))
// where wG == 0 (wC == 0) selects an exact zero for the geometric (photometric) part.  Then the halving tree over the block's ICP_P2PL_BLOCK pairs,
// x[i] += x[i + h] for h = 128 .. 1 (lanes: h = 32 .. 1 pair lane i with lane i + h, the same additions).
template <bool COLORED>
__global__ __launch_bounds__ (256) void ICP_MOMENTS_NAME (icp_params p, const float4 *nrm, double *part, uint32_t nblk, const float4 *grad,
                                                          const float *kappa_word)
{
    constexpr bool ROBUST = ICP_MOMENTS_ROBUST;
    const uint32_t b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * ICP_P2PL_BLOCK + tid;
    const size_t o = (size_t) b * p.m;
    const uint32_t ic = min (i, p.m - 1u);
    const float4 f = p.PF[o + ic], q = p.PM[o + ic];
    const uint32_t id = p.nn_id[o + ic].id;
    // (colored: (r, g, b, 1) of the moving landmark, and kappa)
    const float4 mc = COLORED ? *reinterpret_cast<const float4 *> (p.M + (o + ic) * 8 + 4) : make_float4 (0.f, 0.f, 0.f, 0.f);
    const float kap = COLORED ? *kappa_word : 0.f;
    // (a converged registration: asked behind the pair's loads — in front of them the flag's round trip would come first)
    if (p.check && p.st[b].done) return;                 // (block-uniform)
    double v[ICP_P2PL_TERMS];
#pragma unroll
    for (int t = 0; t < (int) ICP_P2PL_TERMS; ++t) v[t] = 0.0;
    if (i < p.m) {
        if (f.w != 0.f) {
            float4 nf = id < p.m ? nrm[o + id] : make_float4 (0.f, 0.f, 0.f, 0.f);
            if (!(isfinite (nf.x) && isfinite (nf.y) && isfinite (nf.z))) nf = make_float4 (0.f, 0.f, 0.f, 0.f);
            const double w = (double) f.w, mu = (double) p.p2pl_mu;
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
            double kappa = 0.0, JC[6] = {}, rc = 0.0;
            if constexpr (COLORED) {
                float4 gf = id < p.m ? grad[o + id] : make_float4 (0.f, 0.f, 0.f, 0.f);
                if (!(isfinite (gf.x) && isfinite (gf.y) && isfinite (gf.z))) { gf.x = 0.f; gf.y = 0.f; gf.z = 0.f; }
                kappa = (double) kap;
                const double gx = (double) gf.x, gy = (double) gf.y, gz = (double) gf.z, cq = (double) gf.w;
                const double cp = (double) intensity (mc.x, mc.y, mc.z);
                const double dn = (gx * nx + gy * ny) + gz * nz;
                const double tx = gx - dn * nx, ty = gy - dn * ny, tz = gz - dn * nz;
                JC[0] = py * tz - pz * ty; JC[1] = pz * tx - px * tz; JC[2] = px * ty - py * tx; JC[3] = tx; JC[4] = ty; JC[5] = tz;
                const double ex = px - qx, ey = py - qy, ez = pz - qz;
                rc = cp - (cq + ((tx * ex + ty * ey) + tz * ez));
            }
            if constexpr (ROBUST) {
                const double k = (double) *icp_robust_scale (p), k2 = k * k;
                const uint32_t loss = icp_robust (p);
                const double wG = icp_robust_omega (loss, (r * r + mu * ((dx * dx + dy * dy) + dz * dz)) / k2);
                const double wC = COLORED ? icp_robust_omega (loss, (kappa * (rc * rc)) / k2) : 0.0, kwC = kappa * wC;
                int t = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int c = a; c < 6; ++c, ++t) {
                        double x = wG != 0.0 ? wG * (J[a] * J[c] + mu * G[t]) : 0.0;
                        if constexpr (COLORED) x = x + (wC != 0.0 ? kwC * (JC[a] * JC[c]) : 0.0);
                        v[t] = w * x;
                    }
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    double x = wG != 0.0 ? wG * (J[a] * r + mu * g[a]) : 0.0;
                    if constexpr (COLORED) x = x + (wC != 0.0 ? kwC * (JC[a] * rc) : 0.0);
                    v[21 + a] = w * x;
                }
            } else {
                int t = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int c = a; c < 6; ++c, ++t) {
                        double x = J[a] * J[c] + mu * G[t];
                        if constexpr (COLORED) x = x + kappa * (JC[a] * JC[c]);
                        v[t] = w * x;
                    }
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    double x = J[a] * r + mu * g[a];
                    if constexpr (COLORED) x = x + kappa * (JC[a] * rc);
                    v[21 + a] = w * x;
                }
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


#undef ICP_MOMENTS_NAME
#undef ICP_MOMENTS_ROBUST
