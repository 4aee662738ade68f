// icp_tsdf_register.hip — a cloud registered directly against the TSDF volume (the rule: include/icp_amd.h, "Registration against the volume
// itself"; tests/tsdf_register_ref.py restates it).  The residual of a moving point is the volume's value at the point, the Jacobian the
// volume's gradient there: no view, no search structure, no correspondence.
//
//   k_tsdf_reg_moments   one lane per point, 256 lanes a block.  The seven samples of a point (the ray cast's tsdf_fetch / tsdf_value, icp_tsdf.h)
//                        are 56 unconditional 8-byte loads, all issued before the first is used; the 29 terms in double; the plane system's
//                        block tree (plane_block_tree<29>: 29 x 128 doubles of LDS); lane 0 stores the block's 29 partials.  No atomics, no
//                        cross-block word, no spin.
//   k_tsdf_reg_finalize  one workgroup: k_p2pl_finalize's tree over the block partials, then lane 0: LDL^T (icp_ldlt.h), the step, the check,
//                        the state and the record.
// Both read the state's `done` word first and return if it is set: an iteration is the pair of launches, a call enqueues max_iterations
// pairs on the volume's stream and synchronises once.  -ffp-contract=off keeps every operation on its own.
#include "icp_tsdf.h"
#include "icp_cguard.h"
#include "icp_plane_moments.h"          // (plane_block_tree)
#include "icp_ldlt.h"                   // (ldlt_solve)

#include <cmath>

namespace {

constexpr uint32_t REG_BLOCK = 256u, REG_TERMS = 29u, REG_SYS = 27u;
constexpr uint32_t REG_MAX_N = 1u << 20, REG_MAX_BLK = REG_MAX_N / REG_BLOCK;
constexpr uint32_t REG_LDS = 4096u;              // doubles of the finalize's tree buffer (nblk <= 4096)

// the state of a registration on the device, and what the call reads back
struct tsdf_reg_state {
    float R[9], t[3];
    uint32_t k, done, converged, singular, members, pad_;
    double rmse, sys[REG_SYS];
};

struct tsdf_reg_args {
    icp_tsdf_dev v;
    const float4 *cloud; uint32_t n, nblk, P;    // n float8 records; nblk blocks of REG_BLOCK; P = 2^ceil (log2 nblk)
    tsdf_reg_state *st; double *part;            // part[term][block]
    double tan_half_thr, trans_thr;
    uint32_t hold;                               // icp_tsdf_time: the finalize leaves R, t, k and the flags as they are
};

__global__ __launch_bounds__ (256) void k_tsdf_reg_moments (tsdf_reg_args a)
{
    if (a.st->done) return;                      // (block-uniform)
    const icp_tsdf_dev &v = a.v;
    const uint32_t i = blockIdx.x * REG_BLOCK + threadIdx.x;
    icp_tsdf_view cam;
#pragma unroll
    for (int k = 0; k < 9; ++k) cam.R[k] = a.st->R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) cam.t[k] = a.st->t[k];
    const float4 p = i < a.n ? a.cloud[2u * (size_t) i] : make_float4 (0.f, 0.f, 0.f, 1.f);
    const bool valid = !(p.x == 0.f && p.y == 0.f && p.z == 0.f);
    const float3 w = tsdf_world (cam, p.x, p.y, p.z);
    // (a point without a cell fetches cell (0, 0, 0): every load is in bounds whatever the coordinates are)
    tsdf_corners q[7];
    tsdf_fetch (v, w.x, w.y, w.z, q[0]);
    tsdf_fetch (v, w.x + v.voxel, w.y, w.z, q[1]); tsdf_fetch (v, w.x - v.voxel, w.y, w.z, q[2]);
    tsdf_fetch (v, w.x, w.y + v.voxel, w.z, q[3]); tsdf_fetch (v, w.x, w.y - v.voxel, w.z, q[4]);
    tsdf_fetch (v, w.x, w.y, w.z + v.voxel, q[5]); tsdf_fetch (v, w.x, w.y, w.z - v.voxel, q[6]);
    float s[7];
    bool member = valid;
#pragma unroll
    for (int j = 0; j < 7; ++j) { s[j] = 0.f; const bool known = tsdf_value (q[j], s[j]); member = member && known; }
    member = member && fabsf (s[0]) < 1.f;
    double term[REG_TERMS];
    {
        const double r = -((double) v.mu * (double) s[0]);
        const double kg = (double) v.mu / ((double) v.voxel + (double) v.voxel);
        const double gx = (double) (s[1] - s[2]) * kg, gy = (double) (s[3] - s[4]) * kg, gz = (double) (s[5] - s[6]) * kg;
        const double wx = (double) w.x, wy = (double) w.y, wz = (double) w.z;
        const double J[6] = { wy * gz - wz * gy, wz * gx - wx * gz, wx * gy - wy * gx, gx, gy, gz };
        int t = 0;
#pragma unroll
        for (int b = 0; b < 6; ++b)
#pragma unroll
            for (int c = b; c < 6; ++c, ++t) term[t] = member ? J[b] * J[c] : 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) term[21 + b] = member ? J[b] * r : 0.0;
        term[27] = member ? 1.0 : 0.0;
        term[28] = member ? r * r : 0.0;
    }
    plane_block_tree<REG_TERMS> (term, a.part, a.nblk, 0u);
}

__global__ __launch_bounds__ (256) void k_tsdf_reg_finalize (tsdf_reg_args a)
{
    tsdf_reg_state *st = a.st;
    if (st->done) return;                        // (block-uniform)
    const uint32_t tid = threadIdx.x, nblk = a.nblk, P = a.P;
    __shared__ double s[REG_LDS];
    __shared__ double s_sum[REG_TERMS];
    const uint32_t lgP = 31u - (uint32_t) __builtin_clz (P), tc = min (REG_TERMS, REG_LDS / P);
    // the halving tree over the block partials zero-padded to P, as many terms at a time as the LDS buffer holds (k_p2pl_finalize's)
    for (uint32_t t0 = 0; t0 < REG_TERMS; t0 += tc) {
        const uint32_t nt = min (tc, REG_TERMS - t0), n = nt << lgP;
        double x[REG_LDS / 256u];
#pragma unroll
        for (uint32_t u = 0; u < REG_LDS / 256u; ++u) {
            const uint32_t j = tid + 256u * u, t = j >> lgP, i = j & (P - 1u);
            x[u] = (j < n && i < nblk) ? a.part[(size_t) (t0 + t) * nblk + i] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < REG_LDS / 256u; ++u) {
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

    double A[6][6], bb[6];
    {
        int t = 0;
#pragma unroll
        for (int b = 0; b < 6; ++b)
#pragma unroll
            for (int c = b; c < 6; ++c, ++t) { A[b][c] = s_sum[t]; A[c][b] = s_sum[t]; }
#pragma unroll
        for (int b = 0; b < 6; ++b) bb[b] = s_sum[21 + b];
    }
    double x[6];
    bool ok;
    ldlt_solve (A, bb, x, ok);
    const double members = s_sum[27], srr = s_sum[28];
    if (!(members > 0.0)) ok = false;

#pragma unroll
    for (int t = 0; t < (int) REG_SYS; ++t) st->sys[t] = s_sum[t];
    st->members = (uint32_t) members;
    st->rmse = members > 0.0 ? sqrt (srr / members) : 0.0;
    if (a.hold) return;
    if (!ok) { st->singular = 1u; st->done = 1u; return; }

    // q = (omega / 2, 1) / |(omega / 2, 1)| as the point-to-plane step forms it; dR by icp_tsdf_compose_pose's formula
    const double hx = x[0] * 0.5, hy = x[1] * 0.5, hz = x[2] * 0.5;
    const double inv = 1.0 / sqrt (((hx * hx + hy * hy) + hz * hz) + 1.0);
    const double qx = hx * inv, qy = hy * inv, qz = hz * inv, qw = inv;
    const double dR[3][3] = { { 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw) },
                              { 2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw) },
                              { 2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy) } };
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (double) st->R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (double) st->t[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) st->R[3 * r + c] = (float) ((dR[r][0] * R[c] + dR[r][1] * R[3 + c]) + dR[r][2] * R[6 + c]);
        st->t[r] = (float) (((dR[r][0] * t[0] + dR[r][1] * t[1]) + dR[r][2] * t[2]) + x[3 + r]);
    }
    st->k = st->k + 1u;
    const float Tk[8] = { (float) qx, (float) qy, (float) qz, (float) qw, (float) x[3], (float) x[4], (float) x[5], 1.f };
    if (icp_check_converged (Tk, a.tan_half_thr, a.trans_thr)) { st->converged = 1u; st->done = 1u; }
}

bool finite_all (const float *p, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite (p[i])) return false; return true; }

const icp_tsdf_register_t REG_DEFAULTS = { 20u, 0.001, 0.01 };

size_t work_bytes () { return sizeof (tsdf_reg_state) + (size_t) REG_TERMS * REG_MAX_BLK * sizeof (double); }

// the arguments of a call's launches, the work area reserved and the state at pose12 uploaded from *st0, which the caller keeps until it
// has synchronised
int reg_prepare (icp_tsdf_context *t, const icp_tsdf_register_t *opt, const void *dcloud, uint32_t n, const float *pose12, tsdf_reg_args *a, tsdf_reg_state *st0)
{
    const icp_tsdf_register_t &o = opt ? *opt : REG_DEFAULTS;
    int rc;
    if ((rc = icp_host::tsdf_reserve (t, &t->dRegWork, &t->reg_work_cap, work_bytes ()))) return rc;
    *a = tsdf_reg_args {};
    a->v = t->v;
    a->cloud = static_cast<const float4 *> (dcloud); a->n = n; a->nblk = (n + REG_BLOCK - 1u) / REG_BLOCK;
    a->P = 1u; while (a->P < a->nblk) a->P <<= 1;
    a->st = static_cast<tsdf_reg_state *> (t->dRegWork);
    a->part = reinterpret_cast<double *> (static_cast<char *> (t->dRegWork) + sizeof (tsdf_reg_state));
    a->tan_half_thr = std::tan (o.angle_threshold * M_PI / 360.0); a->trans_thr = o.translation_threshold;
    *st0 = tsdf_reg_state {};
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) st0->R[3 * r + k] = pose12[4 * r + k]; st0->t[r] = pose12[4 * r + 3]; }
    TSDFCHK (t, hipMemcpyAsync (t->dRegWork, st0, sizeof *st0, hipMemcpyHostToDevice, t->stream));
    return ICP_OK;
}

void launch_iteration (const tsdf_reg_args &a, hipStream_t s, bool finalize = true)
{
    hipLaunchKernelGGL (k_tsdf_reg_moments, dim3 (a.nblk), dim3 (REG_BLOCK), 0, s, a);
    if (finalize) hipLaunchKernelGGL (k_tsdf_reg_finalize, dim3 (1), dim3 (256), 0, s, a);
}

}  // namespace

static_assert (sizeof (tsdf_reg_state) % sizeof (double) == 0, "the block partials follow the state, aligned");

namespace icp_host {

int tsdf_register_check (icp_tsdf_context *t, const char *who, const icp_tsdf_register_t *opt, const void *cloud, uint32_t n, const float *pose12, const icp_tsdf_registration_t *out)
{
    const std::string w = std::string (who) + ": ";
    if (!cloud || !pose12 || !out) return tsdf_fail (t, ICP_EINVAL, w + "null pointer");
    if (n == 0u || n > REG_MAX_N) return tsdf_fail (t, ICP_EINVAL, w + "the number of points must be in [1, 2^20]");
    if (!finite_all (pose12, 12)) return tsdf_fail (t, ICP_EINVAL, w + "the pose must be finite");
    if (opt) {
        if (opt->max_iterations < 1u || opt->max_iterations > 256u) return tsdf_fail (t, ICP_EINVAL, w + "max_iterations must be in [1, 256]");
        if (!(std::isfinite (opt->angle_threshold) && opt->angle_threshold >= 0.0)) return tsdf_fail (t, ICP_EINVAL, w + "angle_threshold must be finite and >= 0");
        if (!(std::isfinite (opt->translation_threshold) && opt->translation_threshold >= 0.0)) return tsdf_fail (t, ICP_EINVAL, w + "translation_threshold must be finite and >= 0");
    }
    return ICP_OK;
}

int tsdf_register_run (icp_tsdf_context *t, const icp_tsdf_register_t *opt, const void *dcloud, uint32_t n, const float *pose12, icp_tsdf_registration_t *out)
{
    TSDFCHK (t, hipSetDevice (t->device));
    tsdf_reg_args a;
    tsdf_reg_state st0;
    tsdf_reg_state st;
    // (every path below synchronises before it returns: nothing in flight reads st0, st, the caller's cloud or the scratch afterwards)
    int rc = reg_prepare (t, opt, dcloud, n, pose12, &a, &st0);
    if (rc) { (void) hipStreamSynchronize (t->stream); return rc; }
    const uint32_t its = opt ? opt->max_iterations : REG_DEFAULTS.max_iterations;
    for (uint32_t i = 0; i < its; ++i) launch_iteration (a, t->stream);
    hipError_t e = hipGetLastError ();
    if (e == hipSuccess) e = hipMemcpyAsync (&st, a.st, sizeof st, hipMemcpyDeviceToHost, t->stream);
    const hipError_t es = hipStreamSynchronize (t->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return tsdf_fail (t, ICP_EHIP, std::string ("icp_tsdf_register: ") + hipGetErrorString (e));
    icp_tsdf_registration_t res {};
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) res.pose12[4 * r + k] = st.R[3 * r + k]; res.pose12[4 * r + 3] = st.t[r]; }
    res.iterations = st.k; res.converged = st.converged; res.singular = st.singular; res.members = st.members; res.rmse = st.rmse;
    for (uint32_t k = 0; k < REG_SYS; ++k) res.sys[k] = st.sys[k];
    *out = res;
    return ICP_OK;
}

int tsdf_time_register (icp_tsdf_context *t, int part, const void *cloud, uint32_t n, const float *pose12, uint32_t reps, float *us_per_group)
{
    icp_tsdf_registration_t unused;
    int rc = tsdf_register_check (t, "icp_tsdf_time", nullptr, cloud, n, pose12, &unused); if (rc) return rc;
    TSDFCHK (t, hipSetDevice (t->device));
    if ((rc = tsdf_reserve (t, &t->dRegCloud, &t->reg_cloud_cap, (size_t) n * 32u))) return rc;
    TSDFCHK (t, hipMemcpyAsync (t->dRegCloud, cloud, (size_t) n * 32u, hipMemcpyHostToDevice, t->stream));
    tsdf_reg_args a;
    tsdf_reg_state st0;
    // (every path below synchronises before it returns: nothing in flight reads st0, the caller's cloud or the scratch afterwards)
    if ((rc = reg_prepare (t, nullptr, t->dRegCloud, n, pose12, &a, &st0))) { (void) hipStreamSynchronize (t->stream); return rc; }
    a.hold = 1u;
    launch_iteration (a, t->stream);                 // (untimed: the code object is loaded)
    hipError_t e = hipEventRecord (t->ev0, t->stream);
    for (uint32_t i = 0; i < reps; ++i) launch_iteration (a, t->stream, part == 0);
    if (e == hipSuccess) e = hipEventRecord (t->ev1, t->stream);
    if (e == hipSuccess) e = hipGetLastError ();
    const hipError_t es = hipStreamSynchronize (t->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return tsdf_fail (t, ICP_EHIP, std::string ("icp_tsdf_time: ") + hipGetErrorString (e));
    float ms = 0.f;
    TSDFCHK (t, hipEventElapsedTime (&ms, t->ev0, t->ev1));
    *us_per_group = ms * 1e3f / (float) reps;
    return ICP_OK;
}

}  // namespace icp_host

using namespace icp_host;

extern "C" {

int icp_tsdf_register (icp_tsdf_handle t, const icp_tsdf_register_t *opt, const void *cloud_nx8, uint32_t n, const float *pose12, icp_tsdf_registration_t *out) try
{
    if (!t) return ICP_EINVAL;
    int rc = tsdf_register_check (t, "icp_tsdf_register", opt, cloud_nx8, n, pose12, out); if (rc) return rc;
    TSDFCHK (t, hipSetDevice (t->device));
    if ((rc = tsdf_reserve (t, &t->dRegCloud, &t->reg_cloud_cap, (size_t) n * 32u))) return rc;
    TSDFCHK (t, hipMemcpyAsync (t->dRegCloud, cloud_nx8, (size_t) n * 32u, hipMemcpyHostToDevice, t->stream));
    return tsdf_register_run (t, opt, t->dRegCloud, n, pose12, out);
}
ICP_CATCH_ALL

}  // extern "C"
