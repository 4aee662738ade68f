// icp_pyramid.hip — icp_pyramid_*: coarse-to-fine registration.  One ordinary engine handle per level on one device; the levels of F and
// M are built on the device from level 0 by one launch (k_pyramid_build), and T goes from a level to the next finer one on the device
// (k_set_T reading the coarser handle's state, the streams ordered by an event).  The rule is in include/icp_amd.h.
// No reference counterpart (one resolution: src/ICP/algorithms.cpp:4403-4582); Open3D: multi_scale_icp, KinectFusion's three-level pyramid.
#include "icp_host.h"
#include "icp_pair_rule.h"              // (icp_point_valid)

using namespace icp_host;

// ------------------------------------------------------------------------------------------
// The construction.  A 256-thread block takes a 16 x 16 tile of level 0 (tile origins are multiples of 16; side % 2^(levels-1) == 0
// keeps every 2 x 2 block of every level inside one tile, so a partial tile at the rim just has fewer points) and reduces it
// 16x16 -> 8x8 -> 4x4 -> 2x2 -> 1x1 through LDS, a barrier per level.  Global traffic is float4 throughout: consecutive lanes take
// consecutive 16-byte halves of a row of points, on the way in and — from LDS — on the way out.  The two LDS buffers alternate between
// source and destination; the barrier behind a level's reduction also stands between that level's reads and the next level's writes.
// (The 2 x 2 gather reads LDS rows 32 / 64 bytes apart per lane: a few-way bank conflict on 8 KB per block, beside 16 KB of HBM traffic.)
// ------------------------------------------------------------------------------------------
struct icp_pyramid_args {
    const float4 *in;            // level 0, side x side points of two float4
    float4 *out[ICP_PYRAMID_MAX_LEVELS - 1];     // levels 1 .. levels - 1: each handle's own F or M buffer
    uint32_t side, levels, kind;
    float max_dz;
};

// one point of a block joins the running sums (s = the first included value as it is — a lone -0 stays -0 —, then s = s + next)
static __device__ __forceinline__ void pyr_add (bool inc, const float4 &g, const float4 &c, uint32_t &n, float4 &sg, float4 &sc)
{
    if (inc) {
        const bool first = n == 0u;
        sg.x = first ? g.x : sg.x + g.x; sg.y = first ? g.y : sg.y + g.y; sg.z = first ? g.z : sg.z + g.z;
        sc.x = first ? c.x : sc.x + c.x; sc.y = first ? c.y : sc.y + c.y; sc.z = first ? c.z : sc.z + c.z;
        ++n;
    }
}

// one output point from its block (g: xyz1, c: rgb1, block order 0 .. 3); band < 0: no band test
static __device__ __forceinline__ void pyr_reduce (const float4 &g0, const float4 &c0, const float4 &g1, const float4 &c1, const float4 &g2, const float4 &c2,
                                                   const float4 &g3, const float4 &c3, uint32_t kind, float band, float4 &og, float4 &oc)
{
    og = g0; oc = c0;                                                // PICK, and a block without a valid point: element 0, bit for bit
    if (kind == ICP_PYRAMID_PICK) return;
    const bool v0 = icp_point_valid (g0), v1 = icp_point_valid (g1), v2 = icp_point_valid (g2), v3 = icp_point_valid (g3);
    if (!(v0 || v1 || v2 || v3)) return;
    const float zref = v0 ? g0.z : v1 ? g1.z : v2 ? g2.z : g3.z;
    float4 sg = make_float4 (0.f, 0.f, 0.f, 0.f), sc = sg;
    uint32_t n = 0u;
    pyr_add (v0 && (band < 0.f || fabsf (g0.z - zref) <= band), g0, c0, n, sg, sc);
    pyr_add (v1 && (band < 0.f || fabsf (g1.z - zref) <= band), g1, c1, n, sg, sc);
    pyr_add (v2 && (band < 0.f || fabsf (g2.z - zref) <= band), g2, c2, n, sg, sc);
    pyr_add (v3 && (band < 0.f || fabsf (g3.z - zref) <= band), g3, c3, n, sg, sc);
    const float fn = (float) n;
    og = make_float4 (sg.x / fn, sg.y / fn, sg.z / fn, 1.0f);
    oc = make_float4 (sc.x / fn, sc.y / fn, sc.z / fn, 1.0f);
}

// level L (1 ..) of the tile from level L - 1 in `src` (ws = 16 >> (L - 1) points wide) into `dst`, and from there into the level's buffer
template <int L>
static __device__ __forceinline__ void pyr_level (const icp_pyramid_args &a, const float4 *src, float4 *dst, uint32_t t, uint32_t ox, uint32_t oy)
{
    constexpr uint32_t ws = 16u >> (L - 1), wd = 16u >> L;
    const uint32_t side_l = a.side >> L, gx0 = ox >> L, gy0 = oy >> L;
    if (t < wd * wd) {
        const uint32_t X = t % wd, Y = t / wd;
        if (gx0 + X < side_l && gy0 + Y < side_l) {
            const uint32_t q = ((2u * Y) * ws + 2u * X) * 2u;                 // (2x, 2y); +2: (2x+1, 2y); + 2 ws: the row below
            const float4 g0 = src[q], c0 = src[q + 1u], g1 = src[q + 2u], c1 = src[q + 3u];
            const float4 g2 = src[q + 2u * ws], c2 = src[q + 2u * ws + 1u], g3 = src[q + 2u * ws + 2u], c3 = src[q + 2u * ws + 3u];
            // band_l = max_dz * 2^(l-1); max_dz 0 or +inf: no band test
            const float band = (a.max_dz == 0.f || isinf (a.max_dz)) ? -1.f : a.max_dz * (float) (1u << (L - 1));
            float4 og, oc;
            pyr_reduce (g0, c0, g1, c1, g2, c2, g3, c3, a.kind, band, og, oc);
            dst[2u * t] = og; dst[2u * t + 1u] = oc;
        }
    }
    __syncthreads ();
    if (t < 2u * wd * wd) {
        const uint32_t Y = t / (2u * wd), j = t % (2u * wd), X = j >> 1;
        if (gx0 + X < side_l && gy0 + Y < side_l)
            a.out[L - 1][((size_t) (gy0 + Y) * side_l + gx0 + X) * 2u + (j & 1u)] = dst[t];
    }
}

__global__ __launch_bounds__ (256) void k_pyramid_build (icp_pyramid_args a)
{
    __shared__ float4 bufA[512], bufB[128];
    const uint32_t t = threadIdx.x, ox = blockIdx.x * 16u, oy = blockIdx.y * 16u;
#pragma unroll
    for (uint32_t r = 0; r < 2u; ++r) {
        const uint32_t i = t + 256u * r, y = oy + (i >> 5), x = ox + ((i & 31u) >> 1);
        if (x < a.side && y < a.side) bufA[i] = a.in[((size_t) y * a.side + x) * 2u + (i & 1u)];
    }
    __syncthreads ();
    pyr_level<1> (a, bufA, bufB, t, ox, oy);
    if (a.levels > 2u) pyr_level<2> (a, bufB, bufA, t, ox, oy);
    if (a.levels > 3u) pyr_level<3> (a, bufA, bufB, t, ox, oy);
    if (a.levels > 4u) pyr_level<4> (a, bufB, bufA, t, ox, oy);
}

// ------------------------------------------------------------------------------------------
// The object
// ------------------------------------------------------------------------------------------
struct icp_pyramid_context {
    int device = 0, rot = ICP_ROT_POWER_METHOD, weighted = 1;
    icp_handle lv[ICP_PYRAMID_MAX_LEVELS] = { nullptr, nullptr, nullptr, nullptr, nullptr };     // created as init first needs them; kept (with their settings) from then on
    hipEvent_t ev[ICP_PYRAMID_MAX_LEVELS] = { nullptr, nullptr, nullptr, nullptr, nullptr };    // level l's stream has reached ..
    hipEvent_t evTaken[ICP_PYRAMID_MAX_LEVELS] = { nullptr, nullptr, nullptr, nullptr, nullptr };   // level l's T has been read by the hand-over to level l - 1
    hipEvent_t evBuilt = nullptr;                // the construction launch on level 0's stream is done
    hipEvent_t evRun = nullptr;                  // the end of the last icp_pyramid_run_fixed on level 0's stream (icp_pyramid_pending)
    hipEvent_t evT0 = nullptr, evT1 = nullptr;   // icp_pyramid_time_build
    uint32_t levels = 0, side = 0;
    bool inited = false, built = false;
    int kind = ICP_PYRAMID_MEAN;
    float max_dz = 0.f;
    std::string err;
};

namespace {

thread_local std::string g_pyramid_create_error;

int pfail (icp_pyramid_context *p, int code, const std::string &msg)
{
    if (p) p->err = msg; else g_pyramid_create_error = msg;
    return code;
}

#define PYRHIP(p, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return pfail ((p), ICP_EHIP, std::string (#expr) + ": " + hipGetErrorString (e_));   \
    } while (0)

// a call on a level's handle: its status and its message are the pyramid's, with the level named
#define PYRLEVEL(p, l, expr)                                                                     \
    do {                                                                                         \
        int rc_ = (expr);                                                                        \
        if (rc_ != ICP_OK)                                                                       \
            return pfail ((p), rc_, "level " + std::to_string (l) + ": " + icp_last_error ((p)->lv[l])); \
    } while (0)

int pyr_need (icp_pyramid_context *p, bool built, const char *who)
{
    if (!p) return ICP_EINVAL;
    if (!p->inited) return pfail (p, ICP_ESTATE, std::string (who) + ": icp_pyramid_init has not been called");
    if (built && !p->built) return pfail (p, ICP_ESTATE, std::string (who) + ": icp_pyramid_build_rbc has not been called");
    PYRHIP (p, hipSetDevice (p->device));
    return ICP_OK;
}

void destroy_all (icp_pyramid_context *p)
{
    (void) hipSetDevice (p->device);
    for (uint32_t l = 0; l < ICP_PYRAMID_MAX_LEVELS; ++l) {
        if (p->lv[l]) (void) icp_destroy (p->lv[l]);
        if (p->ev[l]) (void) hipEventDestroy (p->ev[l]);
        if (p->evTaken[l]) (void) hipEventDestroy (p->evTaken[l]);
    }
    if (p->evBuilt) (void) hipEventDestroy (p->evBuilt);
    if (p->evRun) (void) hipEventDestroy (p->evRun);
    if (p->evT0) (void) hipEventDestroy (p->evT0);
    if (p->evT1) (void) hipEventDestroy (p->evT1);
    delete p;
}

// Levels 1 .. of F or M from level 0, into the level handles' own buffers: level 0's stream first waits for whatever the other levels'
// streams still read from those buffers, then the one launch, then every level's stream waits for it and the handle takes note of the
// device-side write exactly as icp_write of the same object does (note_inputs_change; the moving normals follow a new M).
int build_levels (icp_pyramid_context *p, int mem, bool timed)
{
    icp_context *h0 = p->lv[0];
    if (p->levels > 1u) {
        icp_pyramid_args a {};
        a.in = reinterpret_cast<const float4 *> (mem == ICP_MEM_F ? h0->dF : h0->dM);
        a.side = p->side; a.levels = p->levels; a.kind = (uint32_t) p->kind; a.max_dz = p->max_dz;
        for (uint32_t l = 1; l < p->levels; ++l) {
            icp_context *h = p->lv[l];
            api_guard guard_ (h);
            { int rc = need (h, false); if (rc) return pfail (p, rc, "level " + std::to_string (l) + ": " + h->err); }
            a.out[l - 1] = reinterpret_cast<float4 *> (mem == ICP_MEM_F ? h->dF : h->dM);
            PYRHIP (p, hipEventRecord (p->ev[l], h->stream));
            PYRHIP (p, hipStreamWaitEvent (h0->stream, p->ev[l], 0));
        }
        const uint32_t tiles = (p->side + 15u) / 16u;
        if (timed) PYRHIP (p, hipEventRecord (p->evT0, h0->stream));
        hipLaunchKernelGGL (k_pyramid_build, dim3 (tiles, tiles), dim3 (256), 0, h0->stream, a);
        PYRHIP (p, hipGetLastError ());
        if (timed) PYRHIP (p, hipEventRecord (p->evT1, h0->stream));
        PYRHIP (p, hipEventRecord (p->evBuilt, h0->stream));
        for (uint32_t l = 1; l < p->levels; ++l) {
            icp_context *h = p->lv[l];
            api_guard guard_ (h);
            PYRHIP (p, hipStreamWaitEvent (h->stream, p->evBuilt, 0));
            note_inputs_change (h);
            if (mem == ICP_MEM_M) { normals_m_follow (h, 0u, 1u); PYRHIP (p, hipGetLastError ()); }
        }
    }
    return ICP_OK;
}

int sync_levels (icp_pyramid_context *p)
{
    for (uint32_t l = 0; l < p->levels; ++l) PYRLEVEL (p, l, icp_sync (p->lv[l]));
    return ICP_OK;
}

// The count of the coarsest level starts at 0, as after icp_build_rbc; its T stays.
int restart_count (icp_pyramid_context *p, uint32_t l)
{
    icp_context *h = p->lv[l];
    api_guard guard_ (h);
    { int rc = need (h, true); if (rc) return pfail (p, rc, "level " + std::to_string (l) + ": " + h->err); }
    note_enqueue (h);
    icp_launch_reset_state (h->p, h->stream, 0);
    PYRHIP (p, hipGetLastError ());
    h->k_base = 0;
    return ICP_OK;
}

// Level l - 1's T <- level l's T as it is on the device when level l's stream gets here; the count of level l - 1 restarts.  What
// icp_write (ICP_MEM_T) does behind its upload (k_set_T: T replaced, the rotation state re-derived), the source being the coarser
// handle's state itself: no host copy, no host wait.  The order holds both ways: the finer stream waits for the coarser level's run, and
// the coarser stream then waits for the read — whatever writes that level's state next (the next run's restart or hand-over,
// icp_pyramid_reset_transform, icp_pyramid_write (ICP_MEM_T), a setter through the borrowed handle) is enqueued behind it.
int hand_over (icp_pyramid_context *p, uint32_t l)
{
    icp_context *hc = p->lv[l], *hf = p->lv[l - 1];
    api_guard guard_ (hf);
    { int rc = need (hf, true); if (rc) return pfail (p, rc, "level " + std::to_string (l - 1) + ": " + hf->err); }
    PYRHIP (p, hipEventRecord (p->ev[l], hc->stream));
    PYRHIP (p, hipStreamWaitEvent (hf->stream, p->ev[l], 0));
    note_enqueue (hf);
    const float *T = reinterpret_cast<const float *> (reinterpret_cast<const char *> (hc->p.st) + offsetof (icp_reg_state, T));
    icp_launch_set_T (hf->p, 0, T, hf->stream, 1);
    PYRHIP (p, hipGetLastError ());
    PYRHIP (p, hipEventRecord (p->evTaken[l], hf->stream));
    PYRHIP (p, hipStreamWaitEvent (hc->stream, p->evTaken[l], 0));
    hf->k_base = 0;
    return ICP_OK;
}

}  // namespace

extern "C" {

const char *icp_pyramid_last_error (icp_pyramid_handle p) { return p ? p->err.c_str () : g_pyramid_create_error.c_str (); }

int icp_pyramid_create (icp_pyramid_handle *out, int device, int rot, int weighted) try
{
    if (!out) return ICP_EINVAL;
    *out = nullptr;
    icp_handle h0 = nullptr;
    int rc = icp_create (&h0, device, rot, weighted);
    if (rc != ICP_OK) return pfail (nullptr, rc, std::string ("icp_pyramid_create: ") + icp_last_error (nullptr));
    struct guard { icp_pyramid_context *p; ~guard () { if (p) destroy_all (p); } } g { nullptr };
    try { g.p = new icp_pyramid_context (); } catch (...) { (void) icp_destroy (h0); throw; }
    icp_pyramid_context *p = g.p;
    p->device = device; p->rot = rot; p->weighted = weighted; p->lv[0] = h0;
    if (hipSetDevice (device) != hipSuccess) return pfail (nullptr, ICP_EHIP, "icp_pyramid_create: hipSetDevice");
    hipEvent_t *evs[] = { &p->ev[0], &p->evBuilt, &p->evRun };
    for (hipEvent_t *e : evs)
        if (hipEventCreateWithFlags (e, hipEventDisableTiming) != hipSuccess) return pfail (nullptr, ICP_EHIP, "icp_pyramid_create: hipEventCreate");
    if (hipEventCreate (&p->evT0) != hipSuccess || hipEventCreate (&p->evT1) != hipSuccess) return pfail (nullptr, ICP_EHIP, "icp_pyramid_create: hipEventCreate");
    g.p = nullptr;
    *out = p;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_destroy (icp_pyramid_handle p) try
{
    if (!p) return ICP_EINVAL;
    destroy_all (p);
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_init (icp_pyramid_handle p, uint32_t levels, uint32_t m, const uint32_t *nr, float a, float c,
                      const uint32_t *max_iterations, double angle_threshold, double translation_threshold) try
{
    if (!p) return ICP_EINVAL;
    if (levels < 1u || levels > ICP_PYRAMID_MAX_LEVELS) return pfail (p, ICP_EINVAL, "icp_pyramid_init: levels must be in [1, 5]");
    if (!nr || !max_iterations) return pfail (p, ICP_EINVAL, "icp_pyramid_init: nr and max_iterations are arrays of `levels` entries");
    const uint32_t side = (uint32_t) std::lround (std::sqrt ((double) m));
    if (m == 0u || (uint64_t) side * side != m) return pfail (p, ICP_EINVAL, "icp_pyramid_init: m must be the point count of a square side x side grid");
    if (side % (1u << (levels - 1u))) return pfail (p, ICP_EINVAL, "icp_pyramid_init: side = " + std::to_string (side) + " is not a multiple of 2^(levels - 1) = " + std::to_string (1u << (levels - 1u)));
    PYRHIP (p, hipSetDevice (p->device));
    p->inited = false; p->built = false;
    for (uint32_t l = 0; l < levels; ++l) {
        if (!p->lv[l]) {
            int rc = icp_create (&p->lv[l], p->device, p->rot, p->weighted);
            if (rc != ICP_OK) return pfail (p, rc, "icp_pyramid_init: level " + std::to_string (l) + ": " + icp_last_error (nullptr));
        }
        if (!p->ev[l]) PYRHIP (p, hipEventCreateWithFlags (&p->ev[l], hipEventDisableTiming));
        if (!p->evTaken[l]) PYRHIP (p, hipEventCreateWithFlags (&p->evTaken[l], hipEventDisableTiming));
        const uint32_t side_l = side >> l;
        int rc = icp_init (p->lv[l], side_l * side_l, nr[l], a, c, max_iterations[l], angle_threshold, translation_threshold);
        if (rc != ICP_OK)
            return pfail (p, rc, "icp_pyramid_init: level " + std::to_string (l) + " (side " + std::to_string (side_l) + ", nr " + std::to_string (nr[l]) + "): " + icp_last_error (p->lv[l]));
    }
    p->levels = levels; p->side = side; p->inited = true;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_set_reduction (icp_pyramid_handle p, int kind, float max_dz) try
{
    if (!p) return ICP_EINVAL;
    if (kind != ICP_PYRAMID_MEAN && kind != ICP_PYRAMID_PICK) return pfail (p, ICP_EINVAL, "icp_pyramid_set_reduction: unknown kind");
    if (!(max_dz >= 0.f)) return pfail (p, ICP_EINVAL, "icp_pyramid_set_reduction: max_dz must be >= 0 (0 or +inf: no band test)");
    p->kind = kind; p->max_dz = max_dz;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_get_reduction (icp_pyramid_handle p, int *kind, float *max_dz) try
{
    if (!p) return ICP_EINVAL;
    if (!kind || !max_dz) return pfail (p, ICP_EINVAL, "icp_pyramid_get_reduction: null output");
    *kind = p->kind; *max_dz = p->max_dz;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_levels (icp_pyramid_handle p, uint32_t *levels) try
{
    if (!p) return ICP_EINVAL;
    if (!levels) return pfail (p, ICP_EINVAL, "icp_pyramid_levels: null output");
    *levels = p->inited ? p->levels : 0u;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_level (icp_pyramid_handle p, uint32_t l, icp_handle *h) try
{
    if (!p) return ICP_EINVAL;
    if (!h) return pfail (p, ICP_EINVAL, "icp_pyramid_level: null output");
    *h = nullptr;
    if (!p->inited) return pfail (p, ICP_ESTATE, "icp_pyramid_level: icp_pyramid_init has not been called");
    if (l >= p->levels) return pfail (p, ICP_EINVAL, "icp_pyramid_level: level out of range");
    *h = p->lv[l];
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_write (icp_pyramid_handle p, int mem, const void *host_ptr, int block) try
{
    { int rc = pyr_need (p, false, "icp_pyramid_write"); if (rc) return rc; }
    if (mem == ICP_MEM_T) {
        const uint32_t l = p->levels - 1u;
        PYRLEVEL (p, l, icp_write (p->lv[l], ICP_MEM_T, host_ptr, block));
        return ICP_OK;
    }
    if (mem != ICP_MEM_F && mem != ICP_MEM_M) return pfail (p, ICP_EINVAL, "icp_pyramid_write: mem must be ICP_MEM_F, ICP_MEM_M or ICP_MEM_T");
    PYRLEVEL (p, 0, icp_write (p->lv[0], mem, host_ptr, 0));
    { int rc = build_levels (p, mem, false); if (rc) return rc; }
    return block ? sync_levels (p) : (int) ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_write_cloud (icp_pyramid_handle p, int which, const void *host_cloud_640x480x8, int block) try
{
    { int rc = pyr_need (p, false, "icp_pyramid_write_cloud"); if (rc) return rc; }
    PYRLEVEL (p, 0, icp_write_cloud (p->lv[0], which, host_cloud_640x480x8, 0));
    { int rc = build_levels (p, which, false); if (rc) return rc; }
    return block ? sync_levels (p) : (int) ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_time_build (icp_pyramid_handle p, int mem, uint32_t reps, float *ms_per_launch) try
{
    { int rc = pyr_need (p, false, "icp_pyramid_time_build"); if (rc) return rc; }
    if ((mem != ICP_MEM_F && mem != ICP_MEM_M) || reps == 0u || !ms_per_launch) return pfail (p, ICP_EINVAL, "icp_pyramid_time_build: bad arguments");
    if (p->levels < 2u) return pfail (p, ICP_ESTATE, "icp_pyramid_time_build: a pyramid of one level has no construction launch");
    float sum = 0.f;
    for (uint32_t r = 0; r < reps; ++r) {
        { int rc = build_levels (p, mem, true); if (rc) return rc; }
        { int rc = sync_levels (p); if (rc) return rc; }
        float ms = 0.f;
        PYRHIP (p, hipEventElapsedTime (&ms, p->evT0, p->evT1));
        sum += ms;
    }
    *ms_per_launch = sum / (float) reps;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_reset_transform (icp_pyramid_handle p) try
{
    { int rc = pyr_need (p, false, "icp_pyramid_reset_transform"); if (rc) return rc; }
    const uint32_t l = p->levels - 1u;
    PYRLEVEL (p, l, icp_reset_transform (p->lv[l]));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_build_rbc (icp_pyramid_handle p) try
{
    { int rc = pyr_need (p, false, "icp_pyramid_build_rbc"); if (rc) return rc; }
    for (uint32_t l = 0; l < p->levels; ++l) PYRLEVEL (p, l, icp_build_rbc (p->lv[l]));
    p->built = true;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_run (icp_pyramid_handle p, uint32_t *k) try
{
    { int rc = pyr_need (p, true, "icp_pyramid_run"); if (rc) return rc; }
    for (uint32_t l = p->levels; l-- > 0u;) {
        { int rc = l + 1u == p->levels ? restart_count (p, l) : hand_over (p, l + 1u); if (rc) return rc; }
        uint32_t kl = 0u;
        PYRLEVEL (p, l, icp_run (p->lv[l], &kl));
        if (k) k[l] = kl;
    }
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_run_fixed (icp_pyramid_handle p, const uint32_t *iterations) try
{
    { int rc = pyr_need (p, true, "icp_pyramid_run_fixed"); if (rc) return rc; }
    if (!iterations) return pfail (p, ICP_EINVAL, "icp_pyramid_run_fixed: iterations is an array of `levels` entries");
    for (uint32_t l = p->levels; l-- > 0u;) {
        { int rc = l + 1u == p->levels ? restart_count (p, l) : hand_over (p, l + 1u); if (rc) return rc; }
        PYRLEVEL (p, l, icp_run_fixed (p->lv[l], iterations[l]));
    }
    PYRHIP (p, hipEventRecord (p->evRun, p->lv[0]->stream));
    return ICP_OK;
}
ICP_CATCH_ALL

// Diagnostic: is what the last icp_pyramid_run_fixed enqueued still in flight?  A query, not a wait.
int icp_pyramid_pending (icp_pyramid_handle p, int *pending) try
{
    { int rc = pyr_need (p, false, "icp_pyramid_pending"); if (rc) return rc; }
    if (!pending) return pfail (p, ICP_EINVAL, "icp_pyramid_pending: null output");
    const hipError_t e = hipEventQuery (p->evRun);
    if (e != hipSuccess && e != hipErrorNotReady) return pfail (p, ICP_EHIP, std::string ("hipEventQuery: ") + hipGetErrorString (e));
    *pending = e == hipErrorNotReady ? 1 : 0;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_pyramid_sync (icp_pyramid_handle p) try
{
    { int rc = pyr_need (p, false, "icp_pyramid_sync"); if (rc) return rc; }
    return sync_levels (p);
}
ICP_CATCH_ALL

}  // extern "C"
