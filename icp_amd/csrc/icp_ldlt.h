// icp_ldlt.h — the one LDL^T solve of the engine: the plane system's 6 x 6 and the colour gradient's 3 x 3 (icp_p2pl.hip), and the 6 x 6 of a
// registration against the TSDF volume (icp_tsdf_register.hip).  tests/p2pl_ref.py restates it.
#pragma once
#include <hip/hip_runtime.h>

// A x = bb for a symmetric N x N A by LDL^T, column by column:  e_jk = L_jk d_k;  d_j = A_jj - e_j0 L_j0 - .. - e_j(j-1) L_j(j-1)
// (subtracted in order k = 0, 1, ..);  L_ij = (A_ij - L_i0 e_j0 - .. - L_i(j-1) e_j(j-1)) / d_j for i > j.  Then L y = bb (y_i = bb_i -
// L_i0 y_0 - .. in order), z = y / d, L^T x = z (x_i = z_i - L_(i+1)i x_(i+1) - .. - L_(N-1)i x_(N-1), ascending k).  ok = false
// (singular) when a pivot is not finite or d_j <= 1e-12 A_jj; x is computed either way.
template <int N>
__device__ __forceinline__ void ldlt_solve (const double (&A)[N][N], const double (&bb)[N], double (&x)[N], bool &ok)
{
    double L[N][N], E[N][N], d[N], y[N];
    ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double v = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) v = v - E[j][k] * L[j][k];
        d[j] = v;
        if (!isfinite (v) || v <= 1e-12 * A[j][j]) ok = false;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double u = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) u = u - L[i][k] * E[j][k];
            L[i][j] = u / v;
            E[i][j] = L[i][j] * v;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double u = bb[i];
#pragma unroll
        for (int k = 0; k < i; ++k) u = u - L[i][k] * y[k];
        y[i] = u;
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double u = y[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) u = u - L[k][i] * x[k];
        x[i] = u;
    }
}
