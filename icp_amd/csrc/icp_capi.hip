// icp_capi.hip — C-ABI (include/icp_amd.h) over the HIP kernels: life cycle of a handle, its buffers, reads and writes, single steps and
// runs, setters, diagnostics.
//
// Host-side counterpart of ICPStep<CR,CW> / ICP<CR,CW> (include/ICP/algorithms.hpp:2234-2496,
// src/ICP/algorithms.cpp:4348-4903).  The reference wires ten kernel-wrapper objects by sharing
// cl::Buffer handles (:4499-4581) and syncs with the host every iteration (:4681-4697); here one
// handle owns its streams, all device buffers of a batch of registrations and the device-resident
// registration state; a fixed-length run is one hipGraph launch, a checked run is driven launch by launch
// from the host (icp_run.hip), frame-to-frame tracking lives in icp_track.hip.
//
// There is NO CPU fallback: without a gfx950 device icp_create fails with ICP_ENODEVICE.
#include "icp_host.h"
#include "icp_tsdf.h"

using namespace icp_host;

namespace {

void free_all (icp_context *h)
{
    drop_graphs (h);
    for (void *q : h->dev_allocs) (void) hipFree (q);
    h->dev_allocs.clear ();
    if (h->hF) (void) hipHostFree (h->hF);
    if (h->hM) (void) hipHostFree (h->hM);
    if (h->hT) (void) hipHostFree (h->hT);
    if (h->hState) (void) hipHostFree (h->hState);
    if (h->hMirror) (void) hipHostFree (h->hMirror);
    if (h->hTrackMirror) (void) hipHostFree (h->hTrackMirror);
    h->hState = nullptr; h->hMirror = h->hTrackMirror = nullptr; h->hstate_fresh = false;
    h->run = run_ctl {}; h->track_k_hist[0] = h->track_k_hist[1] = 0; h->track_hist_frame = 0;
    if (h->dCloud) (void) hipFree (h->dCloud);
    if (h->dCloudOut) (void) hipFree (h->dCloudOut);
    if (h->dRgbdDepth) (void) hipFree (h->dRgbdDepth);
    if (h->dRgbdColour) (void) hipFree (h->dRgbdColour);
    h->dRgbdDepth = nullptr; h->dRgbdColour = nullptr; h->rgbd_depth_cap = h->rgbd_colour_cap = 0;
    for (int k = 0; k < 2; ++k) {
        if (h->hRgbd[k]) (void) hipHostFree (h->hRgbd[k]);
        if (h->dRgbd[k]) (void) hipFree (h->dRgbd[k]);
        h->hRgbd[k] = h->dRgbd[k] = nullptr;
    }
    h->rgbd_track_cap = 0;
    h->hF = h->hM = h->hT = nullptr; h->dCloud = h->dCloudOut = nullptr; h->cloud_cap = 0;
    h->dF = h->dM = nullptr; h->ownF = h->ownM = true;
    h->quality = icp_context::quality_buffers {};                 // (they were among dev_allocs)
    h->pairs = icp_context::pairs_buffers {};
    h->recip = icp_reciprocal_set {};                              // (likewise; stale: the next handle's moving set is yet to be built)
    h->median = nullptr;                                           // (likewise: median-distance rejection's words)
    h->adaptive = nullptr;                                         // (likewise: adaptive trimming's words)
    for (int k = 0; k < 2; ++k) {
        if (h->hBand[k]) (void) hipHostFree (h->hBand[k]);
        if (h->hFrame[k]) (void) hipHostFree (h->hFrame[k]);
        if (h->dBand[k]) (void) hipFree (h->dBand[k]);
        h->hBand[k] = h->hFrame[k] = h->dBand[k] = nullptr;
    }
    for (const auto &r : h->sources) (void) hipHostUnregister (const_cast<char *> (r.base));
    h->sources.clear ();
    if (h->lm[2]) (void) hipFree (h->lm[2]);
    h->lm[0] = h->lm[1] = h->lm[2] = nullptr;
    if (h->hTrack) (void) hipHostFree (h->hTrack);
    h->hTrack = nullptr;
    // (whatever track_prepare got to: a failed stream probe leaves the buffers allocated and rbc2_ready false)
    (void) icp_rbc_for_each (h->rbc[1], h->p, [] (const char *, void **q, size_t) { if (*q) (void) hipFree (*q); return 0; });
    h->rbc[0] = h->rbc[1] = icp_rbc_set {}; h->rbc2_ready = false;
    if (h->dSeq) (void) hipFree (h->dSeq);
    if (h->dRunFlag) (void) hipFree (h->dRunFlag);
    if (h->hGateFlag) (void) hipHostFree (h->hGateFlag);
    h->dSeq = h->dRunFlag = h->hGateFlag = nullptr; h->run2 = run_ctl {}; h->stream2_dirty = false; h->track_last_gated = false;
    h->inited = h->built = false; h->parity = 0; h->track_submitted = h->track_collected = 0;
}

// A setter is about to change what a re-run search would produce (alpha, the metric's scale, the reduction mode): per-query outputs a
// checked run left to be reproduced on demand (lazy outputs: materialize_outputs) are reproduced NOW, with the parameters the run used —
// icp_read then returns the bits of the last executed iteration, as include/icp_amd.h promises, whatever was set in between.
int outputs_before_change (icp_context *h)
{
    if (!h->inited || !h->outputs_stale) return ICP_OK;
    int rc = set_device (h); if (rc) return rc;
    if ((rc = run_close_all (h))) return rc;
    return materialize_outputs (h, ICP_MEM_NN_ID);
}

// The fields of icp_params that follow from what the user set.  The ONLY place that packs the bits of `reject` or decides the word
// `gicp`: icp_create and icp_init_batched start from it, commit () brings p up to date behind every setter.
uint32_t moving_normals_word (const icp_options &o)    // plane-to-plane and symmetric share p.gicp; both on: 1, and need () refuses the run
{
    return o.gicp_eps > 0.f ? 1u : o.symmetric ? ICP_MOVING_NORMALS_SYM : 0u;
}
constexpr int reject_user_flags = ICP_REJECT_INVALID;    // the bits of `reject` that icp_set_rejection takes from the caller as they are
void derive_params (const icp_options &o, icp_params &p)
{
    constexpr uint64_t sum = (uint64_t) ICP_REJECT_INVALID + ICP_REJECT_DIST_ON + ICP_REJECT_TRIM_ON + ICP_REJECT_ROBUST_MASK + ICP_REJECT_UNIQUE_ON + ICP_REJECT_FILTER_MASK + ICP_REJECT_RECIPROCAL_ON + ICP_REJECT_PROJECTIVE_ON + ICP_REJECT_MEDIAN_ON + ICP_REJECT_TRIM_ADAPTIVE;
    static_assert (sum == (ICP_REJECT_INVALID | ICP_REJECT_DIST_ON | ICP_REJECT_TRIM_ON | ICP_REJECT_ROBUST_MASK | ICP_REJECT_UNIQUE_ON | ICP_REJECT_FILTER_MASK | ICP_REJECT_RECIPROCAL_ON | ICP_REJECT_PROJECTIVE_ON | ICP_REJECT_MEDIAN_ON | ICP_REJECT_TRIM_ADAPTIVE),
                   "every rule's bits in icp_params::reject are its own");
    static_assert (ICP_REJECT_INVALID == 1, "ks_epilogue tests bit 0");
    static_assert (ICP_ROBUST_TUKEY << ICP_REJECT_ROBUST_SHIFT == ICP_REJECT_ROBUST_MASK, "the loss's kind fills the mask's two bits");
    static_assert (ICP_REJECT_BOUNDARY_ON + ICP_REJECT_NORMAL_ON == ICP_REJECT_FILTER_MASK, "the pair filter's two rules, a bit each");
    const bool dist = o.reject_max_dist > 0.f && !std::isinf (o.reject_max_dist), trim = o.trim_keep < 1.f, adaptive = o.adaptive_power != 0u;
    p.rot = o.rot; p.weighted = o.weighted; p.power_mode = o.power_mode; p.fused = o.reduce_mode; p.chain = o.chain;
    p.dist_scale = o.metric_scale;
    p.reject = (uint32_t) o.reject_flags | (dist ? ICP_REJECT_DIST_ON : 0u) | (trim || adaptive ? ICP_REJECT_TRIM_ON : 0u)
             | ((uint32_t) o.robust << ICP_REJECT_ROBUST_SHIFT) | (o.unique ? ICP_REJECT_UNIQUE_ON : 0u)
             | (o.boundary_gw ? ICP_REJECT_BOUNDARY_ON : 0u) | (o.normal_on ? ICP_REJECT_NORMAL_ON : 0u)
             | (o.reciprocal ? ICP_REJECT_RECIPROCAL_ON : 0u) | (o.projective ? ICP_REJECT_PROJECTIVE_ON : 0u)
             | (o.median_factor > 0.f ? ICP_REJECT_MEDIAN_ON : 0u) | (adaptive ? ICP_REJECT_TRIM_ADAPTIVE : 0u);     // (the setters keep trim and adaptive apart)
    p.reject_max_dist = o.reject_max_dist;
    p.reject_d2 = dist ? (float) ((double) o.reject_max_dist * (double) o.reject_max_dist) : 0.f;     // (the product of two floats is exact in double)
    p.trim_keep = trim ? o.trim_keep : 0.f;
    p.metric = (uint32_t) o.metric; p.p2pl_mu = o.p2pl_mu;
    p.gicp = moving_normals_word (o);
    p.nrm_grid = o.nrm_grid;
}

// The settings the kernels read from device words instead of captured arguments (a new value touches no graph): which value of the
// record goes where.  write_words writes the chosen ones (OPT_WORDS: all) in stream order behind whatever the handle's stream holds.
enum : unsigned { OPT_W_KAPPA = 1u, OPT_W_ROBUST = 2u, OPT_W_EPS = 4u, OPT_W_MIN_COS = 8u, OPT_W_GRID = 16u, OPT_W_GAP = 32u, OPT_W_PROJ = 64u, OPT_W_MEDIAN = 128u, OPT_W_ADAPTIVE = 2048u, OPT_WORDS = 255u | OPT_W_ADAPTIVE };
int write_words (icp_context *h, unsigned which)
{
    const icp_options &o = h->opt;
    auto bits = [] (float f) { uint32_t u; std::memcpy (&u, &f, sizeof u); return u; };
    uint32_t *const filter = icp_words (h->p, ICP_AREA_FILTER).settings, *const proj = icp_words (h->p, ICP_AREA_PROJECTIVE).settings;
    const struct { unsigned flag; uint32_t value; void *word; } words[] = {
        { OPT_W_KAPPA, bits (o.color_kappa), icp_color_kappa (h->p) },
        { OPT_W_ROBUST, bits (o.robust_scale), icp_robust_scale (h->p) },
        { OPT_W_EPS, bits (o.gicp_eps), icp_gicp_eps (h->p) },
        { OPT_W_MIN_COS, bits (o.normal_min_cos), filter },
        { OPT_W_GRID, o.boundary_gw, filter + 1 },
        { OPT_W_GAP, bits (o.reciprocal_gap), icp_words (h->p, ICP_AREA_RECIPROCAL).settings },
        { OPT_W_PROJ, o.proj_gw, proj }, { OPT_W_PROJ, bits (o.proj_fx), proj + 1 }, { OPT_W_PROJ, bits (o.proj_fy), proj + 2 },
        { OPT_W_PROJ, bits (o.proj_cx), proj + 3 }, { OPT_W_PROJ, bits (o.proj_cy), proj + 4 }, { OPT_W_PROJ, o.proj_radius, proj + 5 },
    };
    // (median-distance rejection's factor lives in the rule's own allocation: nothing to write before median_ready has made it)
    if ((which & OPT_W_MEDIAN) && h->median)
        HIPCHK (h, hipMemsetD32Async (reinterpret_cast<hipDeviceptr_t> (icp_words (h->median, icp_median_desc (), h->p.batch).settings), (int) bits (o.median_factor), 1, h->stream));
    // (adaptive trimming's fractions and power: likewise, once adaptive_ready has made the rule's words)
    if ((which & OPT_W_ADAPTIVE) && h->adaptive) {
        uint32_t *set = icp_words (h->adaptive, icp_adaptive_desc (), h->p.batch).settings;
        const uint32_t v[3] = { bits (o.adaptive_min), bits (o.adaptive_max), o.adaptive_power };
        for (int k = 0; k < 3; ++k) HIPCHK (h, hipMemsetD32Async (reinterpret_cast<hipDeviceptr_t> (set + k), (int) v[k], 1, h->stream));
    }
    for (const auto &w : words)
        if (which & w.flag) HIPCHK (h, hipMemsetD32Async (reinterpret_cast<hipDeviceptr_t> (w.word), (int) w.value, 1, h->stream));
    return ICP_OK;
}

// The one route behind every setter, once it has updated the record.  `what` is what the setter alone knows: which device words it
// changed (OPT_W_*), and whether the change is a parameter update (OPT_PARAMS: cached graphs are updated in place when next used), a
// change of route (OPT_ROUTE: other kernels run, graphs are captured anew), or neither.  What follows from the parameters is found
// by comparing them, old against new: the result area of a feature that went off is cleared (area_features: its memory object reads
// zeros while it is off), the moving set of reciprocal correspondences
// is stale when the rule comes on (M may have been written while it was off), and with grid normals a handle that now needs something its
// last buildRBC did not compute — the moving normals, the intensity gradients — needs a new buildRBC, as after a new F.
// Device work in a fixed order: the open runs end, words, clears, then the stream is drained, so that work later enqueued on any of
// the handle's streams sees them.  OPT_QUIESCE: the open runs end although nothing is written.
enum : unsigned { OPT_PARAMS = 256u, OPT_ROUTE = 512u, OPT_QUIESCE = 1024u };
// The word areas (icp_area, icp_kernels.h) on the host, indexed by area: the memory object that reads an area's result words and the
// test that its feature is on.  commit and mem_of go by it.
const struct { int mem; bool (*on) (const icp_params &); } area_features[ICP_AREA_COUNT] = {
    { ICP_MEM_TRIM, icp_trimming }, { ICP_MEM_PLANE_SYSTEM, icp_p2pl }, { ICP_MEM_UNIQUE, icp_unique },
    { ICP_MEM_PAIR_FILTER, icp_pair_filter }, { ICP_MEM_RECIPROCAL, icp_reciprocal }, { ICP_MEM_PROJECTIVE, icp_projective },
};
int commit (icp_context *h, unsigned what)
{
    const icp_params was = h->p;
    icp_params &p = h->p;
    derive_params (h->opt, p);
    if (p.nrm_grid && ((icp_moving_normals (p) && !icp_moving_normals (was)) || (icp_colored (p) && !icp_colored (was)))) h->built = false;
    bool off[ICP_AREA_COUNT], clears = false;               // per word area: its feature went off
    for (int a = 0; a < ICP_AREA_COUNT; ++a) { off[a] = area_features[a].on (was) && !area_features[a].on (p); clears = clears || off[a]; }
    if (icp_reciprocal (p) && !icp_reciprocal (was)) h->recip.stale = true;
    const bool median_off = icp_median (was) && !icp_median (p) && h->median;    // (its result words are its own allocation's: ICP_MEM_MEDIAN reads zeros while it is off)
    const bool adaptive_off = icp_adaptive_trim (was) && !icp_adaptive_trim (p) && h->adaptive;    // (likewise: ICP_MEM_TRIM_ADAPTIVE; trimming's words go with ICP_AREA_TRIM)
    clears = clears || median_off || adaptive_off;
    if (h->inited && ((what & (OPT_WORDS | OPT_QUIESCE)) || clears)) {
        int rc = set_device (h); if (rc) return rc;
        if ((rc = run_close_all (h))) return rc;
        if ((rc = write_words (h, what & OPT_WORDS))) return rc;
        for (int a = 0; a < ICP_AREA_COUNT; ++a)
            if (off[a]) HIPCHK (h, hipMemsetAsync (icp_words (p, (icp_area) a).result, 0, sizeof (uint32_t) * icp_area_desc_of (a).result * p.batch, h->stream));
        if (median_off) HIPCHK (h, hipMemsetAsync (h->median, 0, sizeof (uint32_t) * icp_median_desc ().result * p.batch, h->stream));
        if (adaptive_off) HIPCHK (h, hipMemsetAsync (h->adaptive, 0, sizeof (uint32_t) * icp_adaptive_desc ().result * p.batch, h->stream));
        if ((what & OPT_WORDS) || clears) HIPCHK (h, hipStreamSynchronize (h->stream));
    }
    if (what & OPT_ROUTE) drop_graphs (h);
    else if (what & OPT_PARAMS) ++h->param_gen;
    return ICP_OK;
}

// landmark-grid / representative-grid validation — src/ICP/algorithms.cpp:842-854 generalised (oracle: orc_reps_grid)
bool reps_grid (uint32_t m, uint32_t nr, uint32_t *nrx, uint32_t *nry, uint32_t *side)
{
    if (m == 0 || nr == 0 || nr > m) return false;
    if (nr & (nr - 1)) return false;
    uint32_t g = (uint32_t) std::floor (std::sqrt ((double) m) + 0.5);
    if ((uint64_t) g * g != m) return false;
    uint32_t pw = 0; while ((1u << (pw + 1)) <= nr) ++pw;
    uint32_t x = 1u << (pw - pw / 2), y = 1u << (pw / 2);
    if (g % x || g % y) return false;
    *nrx = x; *nry = y; *side = g;
    return true;
}

// the device the caller names exists and is a gfx950; who: the caller's message prefix
int gfx950_device (int device, const std::string &who)
{
    int count = 0;
    if (hipGetDeviceCount (&count) != hipSuccess || count <= 0)
        return fail (nullptr, ICP_ENODEVICE, who + ": no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= count) return fail (nullptr, ICP_EINVAL, who + ": device ordinal out of range");
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties (&prop, device);
    if (e != hipSuccess) return fail (nullptr, ICP_EHIP, std::string ("hipGetDeviceProperties: ") + hipGetErrorString (e));
    if (std::strncmp (prop.gcnArchName, "gfx950", 6) != 0)
        return fail (nullptr, ICP_ENODEVICE, who + ": device is " + prop.gcnArchName + ", kernels are built for gfx950 only");
    return ICP_OK;
}

// the cloud scratch (dCloud, dCloudOut) holds n points of 32 bytes
int cloud_reserve (icp_context *h, uint32_t n)
{
    if (h->cloud_cap >= n) return ICP_OK;
    if (h->dCloud) (void) hipFree (h->dCloud);
    if (h->dCloudOut) (void) hipFree (h->dCloudOut);
    h->dCloud = h->dCloudOut = nullptr; h->cloud_cap = 0;
    for (float **q : { &h->dCloud, &h->dCloudOut }) HIPCHK (h, hipMalloc ((void **) q, (size_t) n * 32));
    h->cloud_cap = n;
    return ICP_OK;
}

}  // namespace

// plane-to-plane, symmetric or normal rejection with ICP_NORMALS_GRID: the moving normals of registrations b0 .. b0 + nb - 1 follow a new M, in stream order behind its copy
// (a width that does not divide m: nothing — icp_build_rbc refuses the handle anyway)
namespace icp_host {
void normals_m_follow (icp_context *h, uint32_t b0, uint32_t nb)
{
    if (icp_moving_normals (h->p) && h->p.nrm_grid && h->p.m % h->p.nrm_grid == 0u) icp_launch_normals_m (h->p, h->stream, b0, nb);
    h->recip.stale = true;                           // (reciprocal correspondences: the moving set describes the old M)
}

int reciprocal_ready (icp_context *h)
{
    icp_reciprocal_set &rs = h->recip;
    const icp_params &p = h->p;
    const size_t n = (size_t) p.batch * p.m;
    int rc = set_device (h); if (rc) return rc;
    // (first need; each buffer on its own, zeroed: a call that ran out of memory half way leaves what it got to the next one)
    if ((rc = icp_rbc_for_each (rs.rbc, p, [&] (const char *, void **q, size_t bytes) { return *q ? ICP_OK : dalloc (h, reinterpret_cast<char **> (q), bytes); }))) return rc;
    if (!rs.st && (rc = dalloc (h, &rs.st, (size_t) p.batch))) return rc;
    if (!rs.nn_id && (rc = dalloc (h, &rs.nn_id, n))) return rc;
    if (!rs.PF && (rc = dalloc (h, &rs.PF, n))) return rc;
    if (!rs.PM && (rc = dalloc (h, &rs.PM, n))) return rc;
    if (!rs.rid && (rc = dalloc (h, &rs.rid, n))) return rc;
    if (!rs.stale) return ICP_OK;
    icp_launch_reciprocal_build (p, h->stream, rs);
    HIPCHK (h, hipGetLastError ());
    rs.stale = false;
    return ICP_OK;
}

int median_ready (icp_context *h)
{
    if (h->median) return ICP_OK;
    int rc = set_device (h); if (rc) return rc;
    if ((rc = dalloc (h, &h->median, icp_area_size (icp_median_desc (), h->p.batch, icp_select_keys (h->p.batch, h->p.m))))) return rc;                  // (zeroed: the histograms and the arrival counters start clean)
    float f = h->opt.median_factor; uint32_t u; std::memcpy (&u, &f, sizeof u);
    HIPCHK (h, hipMemsetD32Async (reinterpret_cast<hipDeviceptr_t> (icp_words (h->median, icp_median_desc (), h->p.batch).settings), (int) u, 1, h->stream));
    return ICP_OK;
}

int adaptive_ready (icp_context *h)
{
    if (h->adaptive) return ICP_OK;
    int rc = set_device (h); if (rc) return rc;
    if ((rc = dalloc (h, &h->adaptive, icp_area_size (icp_adaptive_desc (), h->p.batch, 0u)))) return rc;      // (zeroed: the tables and the arrival words start clean)
    return write_words (h, OPT_W_ADAPTIVE);
}
}  // namespace icp_host

extern "C" {

const char *icp_version (void) { return "icp_amd 0.1 (gfx950)"; }

const char *icp_last_error (icp_handle h) { return h ? h->err.c_str () : g_create_error.c_str (); }

// PCI bus id of a device ("0000:c1:00.0"): icp_batch_create looks the device's NUMA node up with it.
int icp_device_pci_bus_id (int device, char *out, size_t cap) try
{
    if (!out || cap < 16) return ICP_EINVAL;
    int n = 0;
    if (hipGetDeviceCount (&n) != hipSuccess || device < 0 || device >= n) { (void) hipGetLastError (); return ICP_ENODEVICE; }
    if (hipDeviceGetPCIBusId (out, (int) cap, device) != hipSuccess) { (void) hipGetLastError (); out[0] = 0; return ICP_EHIP; }
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_device_count (int *n) try
{
    if (!n) return fail (nullptr, ICP_EINVAL, "icp_device_count: null output");
    int c = 0;
    hipError_t e = hipGetDeviceCount (&c);
    if (e != hipSuccess) { *n = 0; return fail (nullptr, ICP_ENODEVICE, std::string ("hipGetDeviceCount: ") + hipGetErrorString (e)); }
    *n = c;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_create (icp_handle *out, int device, int rot, int weighted) try
{
    if (!out) return ICP_EINVAL;
    *out = nullptr;
    if ((rot != ICP_ROT_EIGEN && rot != ICP_ROT_POWER_METHOD) || (weighted != 0 && weighted != 1))
        return fail (nullptr, ICP_EINVAL, "icp_create: rot must be 0|1 and weighted 0|1");
    { int rc = gfx950_device (device, "icp_create"); if (rc) return rc; }
    icp_context *h = new icp_context ();
    h->device = device;
    // Default modes = the benchmarked path: single-pass double moments + squared power start.
    // ICP_AMD_MODE=reference (read here) starts the handle in the reference-order / literal modes instead, whose
    // intermediates restate the reference's arithmetic order; icp_set_reduce_mode / icp_set_power_mode switch later.
    icp_options &o = h->opt;
    o.rot = rot; o.weighted = weighted;
    { const char *e = std::getenv ("ICP_AMD_MODE"); if (e && (e[0] == 'r' || e[0] == 'R')) { o.power_mode = ICP_POWER_LITERAL; o.reduce_mode = ICP_REDUCE_REFERENCE_ORDER; } }
    { const char *e = std::getenv ("ICP_AMD_CHAIN"); o.chain = !e ? 1 : (e[0] == '1') ? 2 : (e[0] == '0') ? 0 : 1; }   // see icp_route_of
    derive_params (o, h->p);
    { const char *e = std::getenv ("ICP_AMD_RUN_ADAPTIVE"); if (e && e[0] == '0') h->run_adaptive = 0; }                  // see run_ctl
    { const char *e = std::getenv ("ICP_AMD_TRACK_GATE"); if (e && e[0] == '0') h->track_gate = 0; }
    { const char *e = std::getenv ("ICP_AMD_OUTPUTS"); if (e && (e[0] == 'e' || e[0] == 'E')) h->outputs_lazy = 0; }
    { const char *e = std::getenv ("ICP_AMD_RUN_DEPTH"); if (e) { const int d = std::atoi (e); if (d >= 1 && d <= 64) h->run_depth = (uint32_t) d; } }
    hipError_t e = hipSetDevice (device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags (&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags (&h->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate (&h->ev0);
    if (e == hipSuccess) e = hipEventCreate (&h->ev1);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreateWithFlags (&h->evUp[k], hipEventDisableTiming);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreateWithFlags (&h->evFrame[k], hipEventDisableTiming);
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreateWithFlags (&h->evDone[k], hipEventDisableTiming);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreateWithFlags (&h->evStage[k], hipEventDisableTiming);
    if (e != hipSuccess) { std::string m = hipGetErrorString (e); h->inited = false; icp_destroy (h); return fail (nullptr, ICP_EHIP, "icp_create: " + m); }
    *out = h;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_destroy (icp_handle h) try
{
    if (!h) return ICP_EINVAL;
    keeper_stop (h);                                 // (the tracking keeper, if this handle ever started one: joined before anything is freed)
    (void) hipSetDevice (h->device);
    if (h->run.active || h->run2.active) (void) run_close_all (h);
    if (h->stream2) (void) hipStreamSynchronize (h->stream2);
    if (h->copy_stream) (void) hipStreamSynchronize (h->copy_stream);
    if (h->stream) (void) hipStreamSynchronize (h->stream);
    free_all (h);
    if (h->dTin) (void) hipFree (h->dTin);
    if (h->ev0) (void) hipEventDestroy (h->ev0);
    if (h->ev1) (void) hipEventDestroy (h->ev1);
    for (int k = 0; k < 2; ++k) if (h->evUp[k]) (void) hipEventDestroy (h->evUp[k]);
    for (int k = 0; k < 2; ++k) if (h->evFrame[k]) (void) hipEventDestroy (h->evFrame[k]);
    for (int k = 0; k < 4; ++k) if (h->evDone[k]) (void) hipEventDestroy (h->evDone[k]);
    for (int k = 0; k < 3; ++k) if (h->evStage[k]) (void) hipEventDestroy (h->evStage[k]);
    if (h->copy_stream) (void) hipStreamDestroy (h->copy_stream);
    if (h->stream2) (void) hipStreamDestroy (h->stream2);
    if (h->stream) (void) hipStreamDestroy (h->stream);
    delete h;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_init_batched (icp_handle h, uint32_t batch, uint32_t m, uint32_t nr, float a, float c,
                      uint32_t max_iterations, double angle_threshold, double translation_threshold) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    // argument checks of the reference: src/ICP/algorithms.cpp:4413-4420, :1573, :842-854
    if (m == 0) return fail (h, ICP_EINVAL, "The sets of landmarks cannot have zero points");
    if (nr == 0) return fail (h, ICP_EINVAL, "The sets of representatives cannot have zero points");
    if (a == 0.f) return fail (h, ICP_EINVAL, "The alpha parameter cannot be equal to zero");
    if (!std::isfinite (a)) return fail (h, ICP_EINVAL, "The alpha parameter cannot be NaN or infinite");
    if (m % 2) return fail (h, ICP_EINVAL, "The number of points in the array must be a multiple of 2");
    if (batch == 0 || batch > 65535u) return fail (h, ICP_EINVAL, "batch must be in [1, 65535]");
    if (max_iterations == 0) return fail (h, ICP_EINVAL, "max_iterations must be positive");
    uint32_t nrx, nry, side;
    if (!reps_grid (m, nr, &nrx, &nry, &side))
        return fail (h, ICP_EINVAL, "nr must be a power of two whose grid tiles the sqrt(m) x sqrt(m) landmark grid");
    if (nr > 32768u) return fail (h, ICP_EINVAL, "nr must be <= 32768");
    if (m > (1u << 20)) return fail (h, ICP_EINVAL, "m must be <= 2^20");
    int rc = set_device (h); if (rc) return rc;
    if ((rc = run_close_all (h))) return rc;
    if (h->copy_stream) HIPCHK (h, hipStreamSynchronize (h->copy_stream));
    if (h->stream2) HIPCHK (h, hipStreamSynchronize (h->stream2));
    if (h->stream) HIPCHK (h, hipStreamSynchronize (h->stream));
    free_all (h);
    icp_params &p = h->p;
    p = icp_params {};
    derive_params (h->opt, p);
    p.check = 0; p.emit = 1;
    p.m = m; p.nr = nr; p.batch = batch; p.side = side; p.nrx = nrx; p.nry = nry;
    p.a = a; p.c = c;
    {   // division-free cell lookups in the kernels (reps_grid guarantees a square grid that the representative grid tiles)
        auto magic = [] (uint32_t d) { return d > 1u ? (uint32_t) ((1ull << 32) / d + 1ull) : 0u; };
        p.side_magic = magic (side); p.cellw_magic = magic (side / nrx); p.cellh_magic = magic (side / nry);
    }
    h->max_iterations = max_iterations; h->angle_threshold = angle_threshold; h->translation_threshold = translation_threshold;
    p.tan_half_thr = std::tan (angle_threshold * M_PI / 360.0);
    p.trans_thr = translation_threshold;
    p.nwg = (m + 127u) / 128u;                                       // src/ICP/algorithms.cpp:1038
    p.nwp = p.nwg; if (p.nwp != 1 && (p.nwp % 4)) p.nwp += 4 - p.nwp % 4;          // :1040
    uint32_t n4 = m; if (n4 % 4) n4 += 4 - n4 % 4;
    p.G = n4 / 4;                                                    // :2344-2346
    p.nsp = (p.G + 511u) / 512u; if (p.nsp != 1 && (p.nsp % 4)) p.nsp += 4 - p.nsp % 4;   // :140-142
    p.nchunk = (m + ICP_CHUNK - 1) / ICP_CHUNK;
    p.nb = (m + 63u) / 64u;
    { const uint32_t ng = (p.nb + 127u) / 128u; p.ng_magic = ng > 1u ? (uint32_t) ((1ull << 32) / ng + 1ull) : 0u; }    // (tasks: 18 ng < 2^16)

    const size_t B = batch;
    float *F = nullptr, *M = nullptr;
    if ((rc = dalloc (h, &F, B * m * 8))) return rc;
    if ((rc = dalloc (h, &M, B * m * 8))) return rc;
    h->dF = F; h->dM = M; p.F = F; p.M = M; h->lm[0] = F; h->lm[1] = M;
    p.n16 = (nr + 15u) / 16u;
    p.tbox = icp_tbox_of (p); p.n1k = (nr + p.tbox - 1u) / p.tbox;
    p.s2wave = icp_s2_wave_of (p);
    { const char *e = std::getenv ("ICP_AMD_XCDMAP"); p.xcdmap = e ? (e[0] == '1') : (B == 1u); }
    { const char *e = std::getenv ("ICP_AMD_WARM_SEED"); p.warm_seed = (e && e[0] == '1') ? 1u : 0u; }
    p.gtile = 0u;                                                    // 4 x 4 tile groups where the representative grid allows
    if (nrx % 4u == 0u && nry % 4u == 0u && !std::getenv ("ICP_AMD_STRIP_GROUPS")) { uint32_t lg = 0; while ((4u << lg) < nrx) ++lg; p.gtile = lg + 1u; }
    p.nlb = m / 16u + 2u;
    {   // the RBC set (icp_rbc_set.h), zeroed: XP's tail reads 0 until something has written it
        icp_rbc_set s;
        if ((rc = icp_rbc_for_each (s, p, [&] (const char *, void **q, size_t bytes) { return dalloc (h, reinterpret_cast<char **> (q), bytes); }))) return rc;
        icp_rbc_into (p, s);
    }
    if ((rc = dalloc (h, &p.rid, B * m))) return rc;
    if ((rc = dalloc (h, &p.nn_id, B * m))) return rc;
    if ((rc = dalloc (h, &p.PF, B * m))) return rc;
    if ((rc = dalloc (h, &p.PM, B * m))) return rc;
    if ((rc = dalloc (h, &p.wpart, B * 2 * p.nwp))) return rc;      // two half-trees per group; padding stays 0.f
    if ((rc = dalloc (h, &p.mpart, B * 2 * p.nwg))) return rc;
    if ((rc = dalloc (h, &p.mscr, B * 2 * ((p.nwg + 127u) / 128u)))) return rc;
    if ((rc = dalloc (h, &p.spart, B * 11 * p.nsp * 8))) return rc;    // 8 sub-trees per work-group; padding stays 0.f
    // (behind the moments, icp_mom_layout: trimming's words, the plane system and its block partials, the device words of the
    // settings (written below); zeroed: ICP_MEM_TRIM and ICP_MEM_PLANE_SYSTEM read 0 until an iteration has written them, and the histograms and counters start clear)
    if ((rc = dalloc (h, &p.mom, icp_mom_layout_of (batch, m, p.nb).total))) return rc;
    if ((rc = write_words (h, OPT_WORDS))) return rc;
    // (one-to-one correspondences: the claim table reads all-ones between iterations — icp_unique.hip)
    HIPCHK (h, hipMemsetAsync (icp_unique_claims (p), 0xFF, sizeof (unsigned long long) * B * m, h->stream));
    if ((rc = dalloc (h, &p.ml1, B * 18 * ((p.nb + 127u) / 128u)))) return rc;
    if ((rc = dalloc (h, &p.cst, B * 2))) return rc;
    if ((rc = dalloc (h, &p.st, B))) return rc;
    if ((rc = dalloc (h, &p.st_prev, B))) return rc;
    if (!h->dTin) HIPCHK (h, hipMalloc ((void **) &h->dTin, 8 * sizeof (float)));
    HIPCHK (h, hipHostMalloc ((void **) &h->hF, B * m * 8 * sizeof (float), hipHostMallocDefault));
    HIPCHK (h, hipHostMalloc ((void **) &h->hM, B * m * 8 * sizeof (float), hipHostMallocDefault));
    HIPCHK (h, hipHostMalloc ((void **) &h->hT, 64 * sizeof (float), hipHostMallocDefault));
    // (fine-grained: the device stores into these while the host polls them — run_ctl)
    HIPCHK (h, hipHostMalloc ((void **) &h->hState, B * sizeof (icp_reg_state), hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK (h, hipHostMalloc ((void **) &h->hMirror, B * sizeof (unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset (h->hMirror, 0, B * sizeof (unsigned long long));
    icp_launch_reset_state (p, h->stream, 1);
    HIPCHK (h, hipGetLastError ());
    HIPCHK (h, hipStreamSynchronize (h->stream));
    h->inited = true; h->built = false;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_init (icp_handle h, uint32_t m, uint32_t nr, float a, float c, uint32_t max_iterations,
              double angle_threshold, double translation_threshold) try
{
    api_guard guard_ (h);
    return icp_init_batched (h, 1, m, nr, a, c, max_iterations, angle_threshold, translation_threshold);
}
ICP_CATCH_ALL

// A memory object of registration b: where it lives on the device, its full size (0: no such object) and, where icp_write takes it as a
// plain copy of m x 16 bytes from the caller's memory, its name (else nullptr).  icp_mem_size, icp_read, icp_device_ptr and icp_write go by it.
struct mem_desc { const void *ptr; size_t bytes; const char *plain_write; };
static mem_desc mem_of (const icp_context *h, uint32_t b, int mem)
{
    const icp_params &p = h->p;
    const size_t m = p.m, nr = p.nr;
    const char *st = reinterpret_cast<const char *> (p.st + b);
    switch (mem) {
        case ICP_MEM_F: return { h->dF + b * m * 8, m * 32, nullptr };
        case ICP_MEM_M: return { h->dM + b * m * 8, m * 32, nullptr };
        case ICP_MEM_RBC_XP: return { p.XP + b * m * 8, m * 32, nullptr };
        case ICP_MEM_T: return { st + offsetof (icp_reg_state, T), 32, nullptr };
        case ICP_MEM_TK: return { st + offsetof (icp_reg_state, Tk), 32, nullptr };
        case ICP_MEM_MEANS: return { st + offsetof (icp_reg_state, means), 32, nullptr };
        case ICP_MEM_S: return { st + offsetof (icp_reg_state, S), 44, nullptr };
        case ICP_MEM_SUM_W: return { st + offsetof (icp_reg_state, sum_w), 8, nullptr };
        case ICP_MEM_R: return { st + offsetof (icp_reg_state, R), 36, nullptr };
        case ICP_MEM_RK: return { st + offsetof (icp_reg_state, Rk), 36, nullptr };
        case ICP_MEM_NN_ID: return { p.nn_id + b * m, m * 8, nullptr };
        case ICP_MEM_RBC_PERM: return { p.perm + b * m, m * 4, nullptr };
        case ICP_MEM_RBC_OWNER: return { p.owner + b * m, m * 4, nullptr };
        case ICP_MEM_RID: return { p.rid + b * m, m * 4, nullptr };
        case ICP_MEM_REPS: return { p.R + b * nr * 8, nr * 32, nullptr };
        case ICP_MEM_RBC_N: return { ICP_N_FULL (p, b), nr * 4, nullptr };
        case ICP_MEM_RBC_O: return { p.O + b * nr, nr * 4, nullptr };
        case ICP_MEM_NN: return { p.PF + b * m, m * 16, nullptr };
        case ICP_MEM_QT: return { p.PM + b * m, m * 16, nullptr };
        case ICP_MEM_W: return { reinterpret_cast<const float *> (p.PF + b * m) + 3, m * 4, nullptr };    // (the .w lane of the matched points: a strided read)
        case ICP_MEM_REVERSE_ID: return { h->recip.nn_id ? h->recip.nn_id + b * m : nullptr, m * 8, nullptr };   // (allocated with the rule's first use)
        case ICP_MEM_MEDIAN: return { h->median ? h->median + icp_median_desc ().result * b : nullptr, icp_median_desc ().result * sizeof (uint32_t), nullptr };                  // (likewise; before that it reads zeros)
        case ICP_MEM_TRIM_ADAPTIVE: return { h->adaptive ? h->adaptive + icp_adaptive_desc ().result * b : nullptr, icp_adaptive_desc ().result * sizeof (uint32_t), nullptr };    // (likewise)
        case ICP_MEM_NORMALS_F: return { icp_normals_f (p) + b * m, m * 16, "ICP_MEM_NORMALS_F" };
        case ICP_MEM_COLOR_GRAD_F: return { icp_color_grad_f (p) + b * m, m * 16, "ICP_MEM_COLOR_GRAD_F" };
        case ICP_MEM_NORMALS_M: return { icp_normals_m (p) + b * m, m * 16, "ICP_MEM_NORMALS_M" };
        default: break;
    }
    // (registration b's result words of a word area)
    for (int a = 0; a < ICP_AREA_COUNT; ++a)
        if (area_features[a].mem == mem) return { icp_words (p, (icp_area) a).result + (size_t) icp_area_desc_of (a).result * b, icp_area_desc_of (a).result * sizeof (uint32_t), nullptr };
    return { nullptr, 0, nullptr };
}

int icp_write_b (icp_handle h, uint32_t b, int mem, const void *host_ptr, int block) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (b >= h->p.batch) return fail (h, ICP_EINVAL, "batch index out of range");
    if ((rc = set_device (h))) return rc;
    const size_t fm = (size_t) h->p.m * 8 * sizeof (float);
    switch (mem) {
        case ICP_MEM_F:
        case ICP_MEM_M: {
            float *stage = (mem == ICP_MEM_F ? h->hF : h->hM) + (size_t) b * h->p.m * 8;
            float *dst = (mem == ICP_MEM_F ? h->dF : h->dM) + (size_t) b * h->p.m * 8;
            // the staging buffer may still feed an earlier asynchronous copy of the same kind: wait for THAT copy (an event of a
            // never-recorded event returns at once), not for whatever else the stream holds (a run in flight keeps going)
            hipEvent_t ev = h->evStage[mem == ICP_MEM_F ? 0 : 1];
            note_inputs_change (h);
            HIPCHK (h, hipEventSynchronize (ev));
            if (host_ptr) std::memcpy (stage, host_ptr, fm);           // algorithms.cpp:4604-4606
            HIPCHK (h, hipMemcpyAsync (dst, stage, fm, hipMemcpyHostToDevice, h->stream));
            HIPCHK (h, hipEventRecord (ev, h->stream));
            if (mem == ICP_MEM_M) { normals_m_follow (h, b, 1u); HIPCHK (h, hipGetLastError ()); }
            break;
        }
        case ICP_MEM_T: {
            HIPCHK (h, hipEventSynchronize (h->evStage[2]));
            if (host_ptr) std::memcpy (h->hT, host_ptr, 8 * sizeof (float));   // :4613-4617
            HIPCHK (h, hipMemcpyAsync (h->dTin, h->hT, 8 * sizeof (float), hipMemcpyHostToDevice, h->stream));
            HIPCHK (h, hipEventRecord (h->evStage[2], h->stream));
            { const long long kb = h->k_base; note_enqueue (h); h->k_base = kb; }       // (T changes, the iteration count does not)
            icp_launch_set_T (h->p, b, h->dTin, h->stream);
            HIPCHK (h, hipGetLastError ());
            break;
        }
        default: {
            // (the fixed normals, colored ICP's intensity gradients, the moving normals, ICP_NORMALS_GIVEN: small and rare — a blocking copy
            // from the caller's memory; the stream is ordered in front of it, so the iterations queued before this read what they were queued with)
            const mem_desc d = mem_of (h, b, mem);
            if (!d.plain_write)
                return fail (h, ICP_EINVAL, "icp_write: mem must be ICP_MEM_F, ICP_MEM_M, ICP_MEM_T, ICP_MEM_NORMALS_F, ICP_MEM_COLOR_GRAD_F or ICP_MEM_NORMALS_M");
            if (!host_ptr) return fail (h, ICP_EINVAL, std::string ("icp_write: ") + d.plain_write + " needs a source");
            note_inputs_change (h);
            HIPCHK (h, hipStreamSynchronize (h->stream));
            HIPCHK (h, hipMemcpy (const_cast<void *> (d.ptr), host_ptr, d.bytes, hipMemcpyHostToDevice));
        }
    }
    if (block) HIPCHK (h, hipStreamSynchronize (h->stream));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_write (icp_handle h, int mem, const void *host_ptr, int block) try { api_guard guard_ (h); return icp_write_b (h, 0, mem, host_ptr, block); } ICP_CATCH_ALL

size_t icp_mem_size (icp_handle h, int mem) { return h && h->inited ? mem_of (h, 0, mem).bytes : 0; }

int icp_read_b (icp_handle h, uint32_t b, int mem, void *host_dst, size_t bytes) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (!host_dst) return fail (h, ICP_EINVAL, "icp_read: null destination");
    if (b >= h->p.batch) return fail (h, ICP_EINVAL, "batch index out of range");
    const mem_desc d = mem_of (h, b, mem);
    if (!d.bytes) return fail (h, ICP_EINVAL, "unknown icp_mem value");
    if (bytes > d.bytes) return fail (h, ICP_EINVAL, "icp_read: more bytes requested than the object holds");
    if (!d.ptr && (mem == ICP_MEM_MEDIAN || mem == ICP_MEM_TRIM_ADAPTIVE)) { std::memset (host_dst, 0, bytes); return ICP_OK; }     // (the rule has not run since icp_init: its words are yet to be allocated)
    if (!d.ptr) return fail (h, ICP_ESTATE, "icp_read: ICP_MEM_REVERSE_ID: no back search has run since icp_init (icp_set_reciprocal)");
    if ((rc = set_device (h))) return rc;
    const void *src = d.ptr;
    if ((rc = materialize_outputs (h, mem))) return rc;
    if (mem == ICP_MEM_W) {                        // weights live in the .w lane of the matched points
        size_t rows = bytes / 4;
        HIPCHK (h, hipMemcpy2DAsync (host_dst, 4, src, 16, 4, rows, hipMemcpyDeviceToHost, h->stream));
    } else
        HIPCHK (h, hipMemcpyAsync (host_dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK (h, hipStreamSynchronize (h->stream));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_read (icp_handle h, int mem, void *host_dst, size_t bytes) try { api_guard guard_ (h); return icp_read_b (h, 0, mem, host_dst, bytes); } ICP_CATCH_ALL

int icp_device_ptr (icp_handle h, int mem, void **dptr) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (!dptr) return fail (h, ICP_EINVAL, "null pointer");
    const mem_desc d = mem_of (h, 0, mem);
    if (!d.bytes) return fail (h, ICP_EINVAL, "unknown icp_mem value");
    if (!d.ptr && mem == ICP_MEM_MEDIAN) return fail (h, ICP_ESTATE, "icp_device_ptr: ICP_MEM_MEDIAN: the rule has not run since icp_init (icp_set_median_rejection)");
    if (!d.ptr && mem == ICP_MEM_TRIM_ADAPTIVE) return fail (h, ICP_ESTATE, "icp_device_ptr: ICP_MEM_TRIM_ADAPTIVE: the rule has not run since icp_init (icp_set_adaptive_trimming)");
    if (!d.ptr) return fail (h, ICP_ESTATE, "icp_device_ptr: ICP_MEM_REVERSE_ID: no back search has run since icp_init (icp_set_reciprocal)");
    if ((rc = set_device (h))) return rc;
    if ((rc = materialize_outputs (h, mem))) return rc;
    *dptr = const_cast<void *> (d.ptr);
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_adopt_device_buffer (icp_handle h, int mem, void *dptr) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (!dptr) return fail (h, ICP_EINVAL, "null pointer");
    if (mem == ICP_MEM_F) { h->dF = static_cast<float *> (dptr); h->p.F = h->dF; h->ownF = false; h->built = false; }
    else if (mem == ICP_MEM_M) { h->dM = static_cast<float *> (dptr); h->p.M = h->dM; h->ownM = false; h->recip.stale = true; }
    else return fail (h, ICP_EINVAL, "only ICP_MEM_F and ICP_MEM_M can be adopted");
    note_inputs_change (h);
    drop_graphs (h);
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_build_rbc (icp_handle h) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if ((rc = set_device (h))) return rc;
    if (h->p.nrm_grid && h->p.m % h->p.nrm_grid)
        return fail (h, ICP_ESTATE, "icp_build_rbc: ICP_NORMALS_GRID: m is not a multiple of the grid width");
    if (h->opt.boundary_gw && h->p.m % h->opt.boundary_gw)
        return fail (h, ICP_ESTATE, "icp_build_rbc: icp_set_boundary_rejection: m is not a multiple of the grid width");
    if (h->opt.projective && h->p.m % h->opt.proj_gw)
        return fail (h, ICP_ESTATE, "icp_build_rbc: icp_set_projective: m is not a multiple of the grid width");
    note_inputs_change (h);
    note_enqueue (h);
    icp_launch_build_rbc (h->p, h->stream);          // (plain launches: docs/HISTORY.md has the comparison with a cached graph)
    HIPCHK (h, hipGetLastError ());
    h->built = true; h->k_base = 0;                                 // (ICP::buildRBC resets k, :4796)
    // (reciprocal correspondences: the moving set behind the fixed one, whatever the handle believes about M — the caller may have
    // changed an adopted buffer)
    if (icp_reciprocal (h->p)) { h->recip.stale = true; if ((rc = reciprocal_ready (h))) return rc; }
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_step (icp_handle h, int config) try
{
    api_guard guard_ (h);
    (void) config;   // the reference sizes the list-scan launch from a host read when config is set; nothing to configure here
    int rc = need (h, true); if (rc) return rc;
    if ((rc = set_device (h))) return rc;
    icp_params p = h->p; p.check = 0; p.hmirror = nullptr; p.hstate = nullptr;
    { const long long kb = h->k_base; note_enqueue (h); if (kb >= 0) h->k_base = kb + 1; }
    note_outputs_stored (h);
    icp_launch_iteration (p, h->stream, &h->recip, h->median, h->adaptive);
    HIPCHK (h, hipGetLastError ());
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_run_fixed (icp_handle h, uint32_t iterations) try
{
    api_guard guard_ (h);
    int rc = need (h, true); if (rc) return rc;
    if (iterations == 0) return ICP_OK;
    if ((rc = set_device (h))) return rc;
    return launch_run (h, iterations, 0);
}
ICP_CATCH_ALL

int icp_run_fixed_fresh (icp_handle h, uint32_t iterations) try
{
    api_guard guard_ (h);
    int rc = need (h, true); if (rc) return rc;
    if (iterations == 0) return icp_reset_transform (h);
    if ((rc = set_device (h))) return rc;
    return launch_run (h, iterations, 0, true);
}
ICP_CATCH_ALL

int icp_run (icp_handle h, uint32_t *k) try
{
    api_guard guard_ (h);
    int rc = need (h, true); if (rc) return rc;
    if ((rc = set_device (h))) return rc;
    if (!h->run_adaptive) {                                              // rounds 1 - 3: one graph of max_iterations launches
        if ((rc = launch_run (h, h->max_iterations, 1))) return rc;
        if ((rc = settle (h))) return rc;                                // queue.finish () — :4813
        h->stat_launches = h->max_iterations; h->stat_k = h->hState[0].k; h->stat_dead = 0;
    } else {
        // the host loop of the reference (:4806-4814: run one step, check (), stop), with the check on the device and the host `run_depth`
        // launches ahead of it: the calling thread polls the registration's progress word and tops the queue up
        if ((rc = run_begin (h, h->run, h->stream, h->p, false, false, h->run_depth + 1u, h->hMirror, h->hState, -1))) return rc;
        if ((rc = run_finish (h))) return rc;
        if ((rc = run_wait_final (h, h->hMirror, h->p.batch, h->run.p.epoch))) return rc;      // (the end kernel is the last thing on the stream: queue.finish ())
        h->stat_t[5] = now_s ();
        h->hstate_fresh = true; h->hstate_here = true;
        if (h->p.batch == 1u) h->k_base = h->hState[0].k;
        {   // the statistics of the run, now that its outcome is known (a run whose launches all went out at once was "decided" before it ran)
            uint32_t kmax = 0u, all_done = 1u;
            for (uint32_t b = 0; b < h->p.batch; ++b) { kmax = std::max (kmax, h->hState[b].k); all_done &= h->hState[b].done ? 1u : 0u; }
            h->stat_k = kmax;
            const uint32_t ran = kmax > h->run.k0 ? kmax - h->run.k0 : 0u;
            h->stat_dead = all_done ? h->run.enq - std::min (h->run.enq, ran + 1u) : 0u;
        }
    }
    if (k) {
        if (h->hstate_fresh) *k = h->hState[0].k;                        // (the run left the states in the pinned mirror)
        else {
            icp_reg_state st;
            HIPCHK (h, hipMemcpy (&st, h->p.st, sizeof st, hipMemcpyDeviceToHost));
            *k = st.k;
        }
    }
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_run_stats (icp_handle h, uint32_t *launches, uint32_t *k, uint32_t *dead) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (launches) *launches = h->stat_launches;
    if (k) *k = h->stat_k;
    if (dead) *dead = h->stat_dead;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_launch_stats (icp_handle h, double *max_us, uint64_t *slower_than_10us, uint64_t *total, int reset) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (max_us) *max_us = h->stat_launch_max_us;
    if (slower_than_10us) *slower_than_10us = h->stat_launch_slow;
    if (total) *total = h->stat_launch_total;
    if (reset) { h->stat_launch_max_us = 0.0; h->stat_launch_slow = h->stat_launch_total = 0; }
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_set_output_mode (icp_handle h, int mode) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (mode != ICP_OUTPUTS_LAZY && mode != ICP_OUTPUTS_EVERY_ITERATION) return fail (h, ICP_EINVAL, "unknown output mode");
    h->outputs_lazy = mode == ICP_OUTPUTS_LAZY;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_run_timeline (icp_handle h, double *us6) try
{
    api_guard guard_ (h);
    if (!h || !us6) return ICP_EINVAL;
    for (int i = 0; i < 6; ++i) us6[i] = (h->stat_t[i] - h->stat_t[0]) * 1e6;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_set_run_depth (icp_handle h, uint32_t depth, int adaptive) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (depth == 0 || depth > 64u) return fail (h, ICP_EINVAL, "icp_set_run_depth: depth must be in [1, 64]");
    { int rc = set_device (h); if (rc) return rc; if ((rc = run_close_all (h))) return rc; }
    h->run_depth = depth; h->run_adaptive = adaptive ? 1 : 0;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_sync (icp_handle h) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    int rc = set_device (h); if (rc) return rc;
    return settle (h);
}
ICP_CATCH_ALL

int icp_get_alpha (icp_handle h, float *a) try { api_guard guard_ (h); if (!h || !a) return ICP_EINVAL; *a = h->p.a; return ICP_OK; } ICP_CATCH_ALL
// The setters change a number in the handle's parameters and nothing else: checked runs are plain launches that read the parameters as they
// are, and a cached fixed-length graph of an older parameter generation is updated in place when it is next used (get_graph).
int icp_set_alpha (icp_handle h, float a) try
{   // setAlpha updates construct and search (src/ICP/algorithms.cpp:4712-4717); lists must be rebuilt by the caller
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (a == 0.f) return fail (h, ICP_EINVAL, "The alpha parameter cannot be equal to zero");
    if (!std::isfinite (a)) return fail (h, ICP_EINVAL, "The alpha parameter cannot be NaN or infinite");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    h->p.a = a; ++h->param_gen; return ICP_OK;
}
ICP_CATCH_ALL
int icp_set_metric_scale (icp_handle h, float f_g) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (!(f_g > 0.f) || !std::isfinite (f_g)) return fail (h, ICP_EINVAL, "the metric scale must be positive and finite");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    h->opt.metric_scale = f_g;
    return commit (h, OPT_PARAMS);
}
ICP_CATCH_ALL
int icp_get_metric_scale (icp_handle h, float *f_g) try { api_guard guard_ (h); if (!h || !f_g) return ICP_EINVAL; *f_g = h->opt.metric_scale; return ICP_OK; } ICP_CATCH_ALL
// The opt-in settings (include/icp_amd.h).  Each setter validates its arguments, reproduces lazy outputs where the change would alter
// them (outputs_before_change), updates the record (icp_options) and commits.
// correspondence rejection: the weights of the pairs change, the search does not — a parameter update, as the metric's scale
int icp_set_rejection (icp_handle h, int flags, float max_dist) try
{
    api_guard guard_ (h);
    if (flags & ~reject_user_flags) return fail (h, ICP_EINVAL, "icp_set_rejection: unknown flag bits");
    if (!(max_dist >= 0.f)) return fail (h, ICP_EINVAL, "icp_set_rejection: max_dist must be >= 0 (0 or +inf: no distance test)");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_rejection: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    h->opt.reject_flags = flags; h->opt.reject_max_dist = max_dist;
    return commit (h, OPT_PARAMS);
}
ICP_CATCH_ALL
int icp_get_rejection (icp_handle h, int *flags, float *max_dist) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (flags) *flags = h->opt.reject_flags;
    if (max_dist) *max_dist = h->opt.reject_max_dist;
    return ICP_OK;
}
ICP_CATCH_ALL
// trimmed ICP (icp_trim.hip).  On <-> off changes which kernels run — the REJ search, select and apply, no chained form —: a change of
// route.  A new fraction while trimming stays on is a parameter update.
int icp_set_trimming (icp_handle h, float keep_fraction) try
{
    api_guard guard_ (h);
    if (!(keep_fraction > 0.f && keep_fraction <= 1.f)) return fail (h, ICP_EINVAL, "icp_set_trimming: keep_fraction must be in (0, 1] (1: off)");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_trimming: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    if (keep_fraction < 1.f && h->opt.adaptive_power != 0u)
        return fail (h, ICP_ESTATE, "icp_set_trimming: adaptive trimming is on (icp_set_adaptive_trimming): switch it off first");
    const bool was = h->opt.trim_keep < 1.f, on = keep_fraction < 1.f;
    h->opt.trim_keep = keep_fraction;
    return commit (h, on != was ? OPT_ROUTE : on ? OPT_PARAMS : 0u);
}
ICP_CATCH_ALL
int icp_get_trimming (icp_handle h, float *keep_fraction) try
{
    api_guard guard_ (h);
    if (!h || !keep_fraction) return ICP_EINVAL;
    *keep_fraction = h->opt.trim_keep;
    return ICP_OK;
}
ICP_CATCH_ALL
// adaptive trimming (icp_adaptive_trim.hip).  On <-> off changes which kernels run — the REJ search, the rule's selection and the apply
// pass, no chained form —: a change of route.  New fractions or a new power while the rule stays on go to its device words alone: no
// graph is touched.  The rule's words are allocated by the next call that enqueues an iteration (need: adaptive_ready).
int icp_set_adaptive_trimming (icp_handle h, float min_fraction, float max_fraction, uint32_t power) try
{
    api_guard guard_ (h);
    if (power != 0u && !(power >= 2u && power <= 8u && min_fraction > 0.f && min_fraction <= max_fraction && max_fraction <= 1.f))
        return fail (h, ICP_EINVAL, "icp_set_adaptive_trimming: power must be 0 (off) or in 2 .. 8 with 0 < min_fraction <= max_fraction <= 1");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_adaptive_trimming: null handle");
    if (power != 0u && h->opt.trim_keep < 1.f)
        return fail (h, ICP_ESTATE, "icp_set_adaptive_trimming: trimming is on (icp_set_trimming): switch it off first (keep_fraction 1)");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const bool was = h->opt.adaptive_power != 0u, on = power != 0u;
    h->opt.adaptive_min = on ? min_fraction : 0.f; h->opt.adaptive_max = on ? max_fraction : 0.f; h->opt.adaptive_power = power;
    return commit (h, on != was ? OPT_ROUTE | OPT_W_ADAPTIVE : on ? OPT_W_ADAPTIVE : 0u);
}
ICP_CATCH_ALL
int icp_get_adaptive_trimming (icp_handle h, float *min_fraction, float *max_fraction, uint32_t *power) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (min_fraction) *min_fraction = h->opt.adaptive_min;
    if (max_fraction) *max_fraction = h->opt.adaptive_max;
    if (power) *power = h->opt.adaptive_power;
    return ICP_OK;
}
ICP_CATCH_ALL
// one-to-one correspondences (icp_unique.hip).  On <-> off changes which kernels run — the REJ search, claim and resolve, on
// point-to-point the apply pass, no chained form —: a change of route.
int icp_set_unique (icp_handle h, int on) try
{
    api_guard guard_ (h);
    if (on != 0 && on != 1) return fail (h, ICP_EINVAL, "icp_set_unique: on must be 0 or 1");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_unique: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const bool was = h->opt.unique;
    h->opt.unique = on != 0;
    return commit (h, h->opt.unique != was ? OPT_ROUTE : 0u);
}
ICP_CATCH_ALL
int icp_get_unique (icp_handle h, int *on) try
{
    api_guard guard_ (h);
    if (!h || !on) return ICP_EINVAL;
    *on = h->opt.unique ? 1 : 0;
    return ICP_OK;
}
ICP_CATCH_ALL
// median-distance rejection (icp_median.hip).  On <-> off changes which kernels run — the REJ search, the rule's launches, on point-to-point
// the apply pass, no chained form —: a change of route.  A new factor while the rule stays on goes to its device word alone: no graph
// is touched.  The rule's words are allocated by the next call that enqueues an iteration (need: median_ready).
int icp_set_median_rejection (icp_handle h, float factor) try
{
    api_guard guard_ (h);
    if (!(factor >= 0.f && std::isfinite (factor))) return fail (h, ICP_EINVAL, "icp_set_median_rejection: factor must be finite and >= 0");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_median_rejection: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const bool was = h->opt.median_factor > 0.f, on = factor > 0.f;
    h->opt.median_factor = factor;
    return commit (h, on != was ? OPT_ROUTE | OPT_W_MEDIAN : on ? OPT_W_MEDIAN : 0u);
}
ICP_CATCH_ALL
int icp_get_median_rejection (icp_handle h, float *factor) try
{
    api_guard guard_ (h);
    if (!h || !factor) return ICP_EINVAL;
    *factor = h->opt.median_factor;
    return ICP_OK;
}
ICP_CATCH_ALL
// reciprocal correspondences (icp_reciprocal.hip).  On <-> off changes which kernels run — the REJ search, the inverse transform, the back
// search and the test, on point-to-point the apply pass, no chained form —: a change of route.  A new max_gap while the rule stays on goes
// to its device word alone: no graph is touched.  The moving set is built by the next call that enqueues an iteration (need).
int icp_set_reciprocal (icp_handle h, int on, float max_gap) try
{
    api_guard guard_ (h);
    if (on != 0 && on != 1) return fail (h, ICP_EINVAL, "icp_set_reciprocal: on must be 0 or 1");
    if (!(max_gap >= 0.f && std::isfinite (max_gap))) return fail (h, ICP_EINVAL, "icp_set_reciprocal: max_gap must be finite and >= 0");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_reciprocal: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const bool was = h->opt.reciprocal;
    h->opt.reciprocal = on != 0; h->opt.reciprocal_gap = on ? max_gap : 0.f;
    return commit (h, h->opt.reciprocal != was ? OPT_ROUTE | OPT_W_GAP : on ? OPT_W_GAP : 0u);
}
ICP_CATCH_ALL
int icp_get_reciprocal (icp_handle h, int *on, float *max_gap) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (on) *on = h->opt.reciprocal ? 1 : 0;
    if (max_gap) *max_gap = h->opt.reciprocal_gap;
    return ICP_OK;
}
ICP_CATCH_ALL
// projective data association (icp_projective.hip).  On <-> off changes which kernels run — k_projective in place of the search, on
// point-to-point the apply pass, no chained form —: a change of route.  New intrinsics, a new width or a new radius while the rule stays
// on go to their device words alone: no graph is touched.
int icp_set_projective (icp_handle h, int on, uint32_t grid_width, float fx, float fy, float cx, float cy, uint32_t radius) try
{
    api_guard guard_ (h);
    if (on != 0 && on != 1) return fail (h, ICP_EINVAL, "icp_set_projective: on must be 0 or 1");
    if (on && grid_width == 0u) return fail (h, ICP_EINVAL, "icp_set_projective: grid_width must be > 0");
    if (!(fx > 0.f && std::isfinite (fx) && fy > 0.f && std::isfinite (fy))) return fail (h, ICP_EINVAL, "icp_set_projective: fx and fy must be finite and > 0");
    if (!(std::isfinite (cx) && std::isfinite (cy))) return fail (h, ICP_EINVAL, "icp_set_projective: cx and cy must be finite");
    if (radius > 8u) return fail (h, ICP_EINVAL, "icp_set_projective: radius must be in [0, 8]");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_projective: null handle");
    if (on && h->inited && h->p.m % grid_width) return fail (h, ICP_ESTATE, "icp_set_projective: m is not a multiple of the grid width");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    icp_options &o = h->opt;
    const bool was = o.projective;
    o.projective = on != 0;
    o.proj_gw = on ? grid_width : 0u; o.proj_radius = on ? radius : 0u;
    o.proj_fx = on ? fx : 0.f; o.proj_fy = on ? fy : 0.f; o.proj_cx = on ? cx : 0.f; o.proj_cy = on ? cy : 0.f;
    return commit (h, o.projective != was ? OPT_ROUTE | OPT_W_PROJ : on ? OPT_W_PROJ : 0u);
}
ICP_CATCH_ALL
int icp_get_projective (icp_handle h, int *on, uint32_t *grid_width, float *fx, float *fy, float *cx, float *cy, uint32_t *radius) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    const icp_options &o = h->opt;
    if (on) *on = o.projective ? 1 : 0;
    if (grid_width) *grid_width = o.proj_gw;
    if (fx) *fx = o.proj_fx;
    if (fy) *fy = o.proj_fy;
    if (cx) *cx = o.proj_cx;
    if (cy) *cy = o.proj_cy;
    if (radius) *radius = o.proj_radius;
    return ICP_OK;
}
ICP_CATCH_ALL
// boundary and normal rejection (icp_pair_filter.hip).  A rule on <-> off changes which kernels run — the REJ search, k_pair_filter, on
// point-to-point the apply pass, no chained form —: a change of route (a new width too).  A new min_cos while the normal rule stays on
// goes to its device word alone: no graph is touched.
int icp_set_normal_rejection (icp_handle h, int on, float min_cos) try
{
    api_guard guard_ (h);
    if (on != 0 && on != 1) return fail (h, ICP_EINVAL, "icp_set_normal_rejection: on must be 0 or 1");
    if (!(min_cos >= -1.f && min_cos <= 1.f)) return fail (h, ICP_EINVAL, "icp_set_normal_rejection: min_cos must be in [-1, 1]");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_normal_rejection: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const bool was = h->opt.normal_on;
    h->opt.normal_on = on != 0; h->opt.normal_min_cos = on ? min_cos : 0.f;
    return commit (h, h->opt.normal_on != was ? OPT_ROUTE | OPT_W_MIN_COS : on ? OPT_W_MIN_COS : 0u);
}
ICP_CATCH_ALL
int icp_get_normal_rejection (icp_handle h, int *on, float *min_cos) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (on) *on = h->opt.normal_on ? 1 : 0;
    if (min_cos) *min_cos = h->opt.normal_min_cos;
    return ICP_OK;
}
ICP_CATCH_ALL
int icp_set_boundary_rejection (icp_handle h, uint32_t grid_width) try
{
    api_guard guard_ (h);
    if (!h) return fail (h, ICP_EINVAL, "icp_set_boundary_rejection: null handle");
    if (grid_width && h->inited && h->p.m % grid_width) return fail (h, ICP_ESTATE, "icp_set_boundary_rejection: m is not a multiple of the grid width");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    if (grid_width == h->opt.boundary_gw) return ICP_OK;
    h->opt.boundary_gw = grid_width;
    return commit (h, OPT_ROUTE | OPT_W_GRID);
}
ICP_CATCH_ALL
int icp_get_boundary_rejection (icp_handle h, uint32_t *grid_width) try
{
    api_guard guard_ (h);
    if (!h || !grid_width) return ICP_EINVAL;
    *grid_width = h->opt.boundary_gw;
    return ICP_OK;
}
ICP_CATCH_ALL
// robust loss (icp_trim.hip, icp_p2pl.hip).  On <-> off and a new kind change which kernels run — point-to-point: the REJ search and
// the apply pass, no chained form; the plane metrics: other moments —: a change of route.  A new scale while the loss stays on goes to
// its device word alone: no graph is touched.
int icp_set_robust_loss (icp_handle h, int loss, float scale) try
{
    api_guard guard_ (h);
    if (loss != ICP_ROBUST_NONE && loss != ICP_ROBUST_HUBER && loss != ICP_ROBUST_CAUCHY && loss != ICP_ROBUST_TUKEY)
        return fail (h, ICP_EINVAL, "icp_set_robust_loss: unknown loss");
    if (loss != ICP_ROBUST_NONE && !(scale > 0.f && std::isfinite (scale)))
        return fail (h, ICP_EINVAL, "icp_set_robust_loss: scale must be finite and > 0");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_robust_loss: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const int was = h->opt.robust;
    h->opt.robust = loss; h->opt.robust_scale = loss != ICP_ROBUST_NONE ? scale : 0.f;
    return commit (h, OPT_W_ROBUST | (loss != was ? OPT_ROUTE : 0u));
}
ICP_CATCH_ALL
int icp_get_robust_loss (icp_handle h, int *loss, float *scale) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (loss) *loss = h->opt.robust;
    if (scale) *scale = h->opt.robust_scale;
    return ICP_OK;
}
ICP_CATCH_ALL
// The two settings that need the moving frame's normals, plane-to-plane (icp_gicp.hip) and symmetric (icp_symmetric.hip), share one
// word of icp_params (moving_normals_word); the record keeps them apart, so that need () can name both when they are on together.  A
// changed word changes which moments kernel a point-to-plane iteration runs and what buildRBC launches: a change of route.  A new
// epsilon while plane-to-plane stays on goes to its device word alone: no graph is touched.
int icp_set_plane_to_plane (icp_handle h, float epsilon) try
{
    api_guard guard_ (h);
    if (!(epsilon >= 0.f && epsilon <= 1.f)) return fail (h, ICP_EINVAL, "icp_set_plane_to_plane: epsilon must be in [0, 1] (0: off)");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_plane_to_plane: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const uint32_t was = moving_normals_word (h->opt);
    h->opt.gicp_eps = epsilon;
    return commit (h, OPT_W_EPS | (moving_normals_word (h->opt) != was ? OPT_ROUTE : 0u));
}
ICP_CATCH_ALL
int icp_get_plane_to_plane (icp_handle h, float *epsilon) try
{
    api_guard guard_ (h);
    if (!h || !epsilon) return ICP_EINVAL;
    *epsilon = h->opt.gicp_eps;
    return ICP_OK;
}
ICP_CATCH_ALL
int icp_set_symmetric (icp_handle h, int on) try
{
    api_guard guard_ (h);
    if (on != 0 && on != 1) return fail (h, ICP_EINVAL, "icp_set_symmetric: on must be 0 or 1");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_symmetric: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const uint32_t was = moving_normals_word (h->opt);
    h->opt.symmetric = on != 0;
    return commit (h, OPT_QUIESCE | (moving_normals_word (h->opt) != was ? OPT_ROUTE : 0u));
}
ICP_CATCH_ALL
int icp_get_symmetric (icp_handle h, int *on) try
{
    api_guard guard_ (h);
    if (!h || !on) return ICP_EINVAL;
    *on = h->opt.symmetric ? 1 : 0;
    return ICP_OK;
}
ICP_CATCH_ALL
// point-to-plane (icp_p2pl.hip).  On <-> off changes which kernels run — the moments and the 6 x 6 finalize, no chained form —: a
// change of route.  A new mu while the metric stays on is a parameter update.  Colored ICP is point-to-plane with other moments:
// POINT_TO_PLANE <-> COLORED changes the kernels too.
int icp_set_error_metric (icp_handle h, int metric, float point_weight) try
{
    api_guard guard_ (h);
    if (metric != ICP_METRIC_POINT_TO_POINT && metric != ICP_METRIC_POINT_TO_PLANE && metric != ICP_METRIC_COLORED)
        return fail (h, ICP_EINVAL, "icp_set_error_metric: unknown metric");
    if (!(point_weight >= 0.f && std::isfinite (point_weight))) return fail (h, ICP_EINVAL, "icp_set_error_metric: point_weight must be finite and >= 0");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_error_metric: null handle");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    const int was = h->opt.metric;
    h->opt.metric = metric; h->opt.p2pl_mu = metric != ICP_METRIC_POINT_TO_POINT ? point_weight : 0.f;
    return commit (h, metric != was ? OPT_ROUTE : metric != ICP_METRIC_POINT_TO_POINT ? OPT_PARAMS : 0u);
}
ICP_CATCH_ALL
int icp_get_error_metric (icp_handle h, int *metric, float *point_weight) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (metric) *metric = h->opt.metric;
    if (point_weight) *point_weight = h->opt.p2pl_mu;
    return ICP_OK;
}
ICP_CATCH_ALL
// kappa lives in a device word the moments read (icp_color_kappa), not in the captured arguments: a new kappa touches no graph, and no
// search would give other outputs for it (no outputs_before_change).
int icp_set_color_weight (icp_handle h, float kappa) try
{
    api_guard guard_ (h);
    if (!(kappa >= 0.f && std::isfinite (kappa))) return fail (h, ICP_EINVAL, "icp_set_color_weight: kappa must be finite and >= 0");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_color_weight: null handle");
    h->opt.color_kappa = kappa;
    return commit (h, OPT_W_KAPPA);
}
ICP_CATCH_ALL
int icp_get_color_weight (icp_handle h, float *kappa) try
{
    api_guard guard_ (h);
    if (!h || !kappa) return ICP_EINVAL;
    *kappa = h->opt.color_kappa;
    return ICP_OK;
}
ICP_CATCH_ALL
// The source of the normals changes what buildRBC launches (k_normals_grid behind it): the build graph goes with the others.
int icp_set_normals (icp_handle h, int source, uint32_t grid_width) try
{
    api_guard guard_ (h);
    if (source != ICP_NORMALS_GIVEN && source != ICP_NORMALS_GRID) return fail (h, ICP_EINVAL, "icp_set_normals: unknown source");
    if (source == ICP_NORMALS_GRID && grid_width == 0u) return fail (h, ICP_EINVAL, "icp_set_normals: ICP_NORMALS_GRID needs a grid width");
    if (!h) return fail (h, ICP_EINVAL, "icp_set_normals: null handle");
    const uint32_t w = source == ICP_NORMALS_GRID ? grid_width : 0u;
    if (w && h->inited && h->p.m % w) return fail (h, ICP_ESTATE, "icp_set_normals: m is not a multiple of the grid width");
    if (w == h->opt.nrm_grid) return ICP_OK;
    h->opt.nrm_grid = w;
    return commit (h, OPT_ROUTE);
}
ICP_CATCH_ALL
int icp_get_normals (icp_handle h, int *source, uint32_t *grid_width) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (source) *source = h->opt.nrm_grid ? ICP_NORMALS_GRID : ICP_NORMALS_GIVEN;
    if (grid_width) *grid_width = h->opt.nrm_grid;
    return ICP_OK;
}
ICP_CATCH_ALL
int icp_get_scaling (icp_handle h, float *c) try { api_guard guard_ (h); if (!h || !c) return ICP_EINVAL; *c = h->p.c; return ICP_OK; } ICP_CATCH_ALL
int icp_set_scaling (icp_handle h, float c) try { api_guard guard_ (h); if (!h) return ICP_EINVAL; h->p.c = c; ++h->param_gen; return ICP_OK; } ICP_CATCH_ALL
int icp_get_max_iterations (icp_handle h, uint32_t *n) try { api_guard guard_ (h); if (!h || !n) return ICP_EINVAL; *n = h->max_iterations; return ICP_OK; } ICP_CATCH_ALL
int icp_set_max_iterations (icp_handle h, uint32_t n) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (n == 0) return fail (h, ICP_EINVAL, "max_iterations must be positive");
    h->max_iterations = n; return ICP_OK;
}
ICP_CATCH_ALL
int icp_get_angle_threshold (icp_handle h, double *d) try { api_guard guard_ (h); if (!h || !d) return ICP_EINVAL; *d = h->angle_threshold; return ICP_OK; } ICP_CATCH_ALL
int icp_set_angle_threshold (icp_handle h, double d) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    h->angle_threshold = d; h->p.tan_half_thr = std::tan (d * M_PI / 360.0); ++h->param_gen; return ICP_OK;
}
ICP_CATCH_ALL
int icp_get_translation_threshold (icp_handle h, double *d) try { api_guard guard_ (h); if (!h || !d) return ICP_EINVAL; *d = h->translation_threshold; return ICP_OK; } ICP_CATCH_ALL
int icp_set_translation_threshold (icp_handle h, double d) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    h->translation_threshold = d; h->p.trans_thr = d; ++h->param_gen; return ICP_OK;
}
ICP_CATCH_ALL
int icp_set_power_mode (icp_handle h, int mode) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (mode != ICP_POWER_LITERAL && mode != ICP_POWER_SQUARED) return fail (h, ICP_EINVAL, "unknown power mode");
    h->opt.power_mode = mode;
    return commit (h, OPT_PARAMS);
}
ICP_CATCH_ALL

int icp_set_reduce_mode (icp_handle h, int mode) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (mode != ICP_REDUCE_REFERENCE_ORDER && mode != ICP_REDUCE_FUSED) return fail (h, ICP_EINVAL, "unknown reduce mode");
    { int rc = outputs_before_change (h); if (rc) return rc; }
    h->opt.reduce_mode = mode;
    return commit (h, OPT_ROUTE);
}
ICP_CATCH_ALL

int icp_state_b (icp_handle h, uint32_t b, icp_state_t *out) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (!out) return fail (h, ICP_EINVAL, "null pointer");
    if (b >= h->p.batch) return fail (h, ICP_EINVAL, "batch index out of range");
    if ((rc = set_device (h))) return rc;
    icp_reg_state st;
    if (h->hstate_fresh) {                       // a checked run was the last thing that changed the states: its end left them in the mirror
        if (!h->hstate_here) HIPCHK (h, hipStreamSynchronize (h->stream));
        st = h->hState[b];
    } else {
        HIPCHK (h, hipMemcpyAsync (&st, h->p.st + b, sizeof st, hipMemcpyDeviceToHost, h->stream));
        HIPCHK (h, hipStreamSynchronize (h->stream));
    }
    std::memcpy (out->R, st.R, sizeof st.R); std::memcpy (out->Rk, st.Rk, sizeof st.Rk);
    std::memcpy (out->q, st.T, 16); std::memcpy (out->t, st.T + 4, 12); out->s = st.T[7];
    std::memcpy (out->qk, st.Tk, 16); std::memcpy (out->tk, st.Tk + 4, 12); out->sk = st.Tk[7];
    out->k = st.k; out->converged = st.done; out->power_iterations = st.pm_iters; out->reserved = 0;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_state (icp_handle h, icp_state_t *out) try { api_guard guard_ (h); return icp_state_b (h, 0, out); } ICP_CATCH_ALL

// What icp_evaluate and icp_correspondences ask of the handle before they touch the device (`who`: the call's name for the messages).
// need () brings an open checked run to its end, as icp_read does.
static int evaluation_ready (icp_context *h, const char *who, uint32_t count)
{
    const std::string w (who);
    if (count == 0) return fail (h, ICP_EINVAL, w + ": count must be at least 1");
    int rc = need (h, false); if (rc) return rc;
    if (count > h->p.batch) return fail (h, ICP_EINVAL, w + ": count is above the handle's batch");
    if (h->track_submitted) return fail (h, ICP_ESTATE, w + ": the handle has tracked frames (the quality of tracked frames is not provided): icp_init or icp_track_reset first");
    if (!h->built) return fail (h, ICP_ESTATE, "icp_build_rbc has not been called");
    return set_device (h);
}

// The search into the evaluation's own buffers, shared by icp_evaluate and icp_correspondences (ICP_PAIRS_EVALUATED): the plain search of
// the handle's layout in its reference-order form with every opt-in rule off and REGULAR weights — the same correspondences and points
// bit for bit as an iteration's search at this state, and a form that writes nothing but its per-query outputs: no moment partials (the
// fused form's), no weight partials (the WEIGHTED ones).  The state, the flags of the lazy outputs, the graphs and the pinned mirror are
// not touched.
static int evaluation_search (icp_context *h)
{
    const icp_params &p = h->p;
    const size_t n = (size_t) p.batch * p.m;
    icp_context::quality_buffers &Q = h->quality;
    int rc;
    // (first use; each buffer on its own: a call that ran out of memory half way leaves what it got to the next one)
    if (!Q.nn_id && (rc = dalloc (h, &Q.nn_id, n))) return rc;
    if (!Q.PF && (rc = dalloc (h, &Q.PF, n))) return rc;
    if (!Q.PM && (rc = dalloc (h, &Q.PM, n))) return rc;
    if (!Q.rid && (rc = dalloc (h, &Q.rid, n))) return rc;
    icp_params q = p;
    q.check = 0; q.emit = 1; q.fused = 0; q.weighted = 0; q.hmirror = nullptr; q.hstate = nullptr; q.dbg = nullptr;
    q.reject = 0u; q.reject_d2 = 0.f; q.reject_max_dist = 0.f; q.trim_keep = 0.f; q.metric = ICP_METRIC_POINT_TO_POINT; q.p2pl_mu = 0.f; q.gicp = 0u;
    q.nn_id = Q.nn_id; q.PF = Q.PF; q.PM = Q.PM; q.rid = Q.rid;
    // (the dense search seeds its pruning with the nearest representatives of the search before it and leaves its own: the seeds are the
    // iterations', the answers stay here)
    if (icp_dense (q)) HIPCHK (h, hipMemcpyAsync (Q.rid, p.rid, n * sizeof (uint32_t), hipMemcpyDeviceToDevice, h->stream));
    icp_launch_search (q, h->stream);
    return ICP_OK;
}

// Registration quality (include/icp_amd.h; icp_quality.hip): one search at the registrations' current state into the evaluation's own
// buffers (evaluation_search), the pair kernel, the second level, one copy of the result words.
int icp_evaluate (icp_handle h, float max_dist, icp_quality_t *out, uint32_t count) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (!out) return fail (h, ICP_EINVAL, "icp_evaluate: null output");
    if (!(max_dist >= 0.f)) return fail (h, ICP_EINVAL, "icp_evaluate: max_dist must be >= 0 (0 or +inf: no distance test)");
    int rc = evaluation_ready (h, "icp_evaluate", count); if (rc) return rc;
    const icp_params &p = h->p;
    const size_t B = p.batch, nblk = icp_p2pl_nblk (p.m);
    icp_context::quality_buffers &Q = h->quality;
    if ((rc = evaluation_search (h))) return rc;
    if (!Q.part && (rc = dalloc (h, &Q.part, B * ICP_QUALITY_TERMS * nblk))) return rc;
    if (!Q.cnt && (rc = dalloc (h, &Q.cnt, B * 2 * nblk))) return rc;
    if (!Q.res && (rc = dalloc (h, &Q.res, B * ICP_QUALITY_RES))) return rc;
    const bool dist_on = max_dist > 0.f && !std::isinf (max_dist);
    icp_launch_quality (Q.PF, Q.PM, p.M, p.m, p.batch, dist_on, dist_on ? (float) ((double) max_dist * (double) max_dist) : 0.f, Q.part, Q.cnt, Q.res, h->stream);
    HIPCHK (h, hipGetLastError ());
    std::vector<double> res (B * ICP_QUALITY_RES);
    HIPCHK (h, hipMemcpyAsync (res.data (), Q.res, res.size () * sizeof (double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK (h, hipStreamSynchronize (h->stream));
    for (uint32_t b = 0; b < count; ++b) {
        const double *r = res.data () + (size_t) b * ICP_QUALITY_RES;
        icp_quality_t &o = out[b];
        uint32_t c[2];
        std::memcpy (c, r + ICP_QUALITY_TERMS, sizeof c);
        o.n = p.m; o.n_moving = c[0]; o.n_inliers = c[1]; o.reserved = 0u;
        o.sum_geo = r[21];
        o.fitness = c[0] ? (double) c[1] / (double) c[0] : 0.0;
        o.inlier_rmse = c[1] ? std::sqrt (r[21] / (double) c[1]) : 0.0;
        int t = 0;
        for (int a = 0; a < 6; ++a)
            for (int cc = a; cc < 6; ++cc, ++t) { o.information[a * 6 + cc] = r[t]; o.information[cc * 6 + a] = r[t]; }
    }
    return ICP_OK;
}
ICP_CATCH_ALL

// The correspondence set (include/icp_amd.h; icp_pairs.hip).  ICP_PAIRS_EVALUATED: evaluation_search, then the two passes over the
// evaluation's buffers — icp_evaluate's launch count.  ICP_PAIRS_LAST_ITERATION: the two passes over the per-query outputs as icp_read
// would deliver them (lazy outputs are reproduced first: materialize_outputs).  One copy of the count words, the wait.
int icp_correspondences (icp_handle h, int source, float max_dist, uint32_t *counts, uint32_t count) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (source != ICP_PAIRS_EVALUATED && source != ICP_PAIRS_LAST_ITERATION) return fail (h, ICP_EINVAL, "icp_correspondences: unknown source");
    if (!counts) return fail (h, ICP_EINVAL, "icp_correspondences: null counts");
    if (!(max_dist >= 0.f)) return fail (h, ICP_EINVAL, "icp_correspondences: max_dist must be >= 0 (0 or +inf: no distance test)");
    if (source == ICP_PAIRS_LAST_ITERATION && max_dist != 0.f)
        return fail (h, ICP_EINVAL, "icp_correspondences: ICP_PAIRS_LAST_ITERATION takes the pairs the iteration used: max_dist must be 0");
    int rc = evaluation_ready (h, "icp_correspondences", count); if (rc) return rc;
    const icp_params &p = h->p;
    const size_t B = p.batch;
    icp_context::pairs_buffers &P = h->pairs;
    static_assert (sizeof (icp_pair_t) == sizeof (uint4) && sizeof (icp_pair_t) == 16, "a record is one 16-byte store");
    if (source == ICP_PAIRS_LAST_ITERATION && (rc = materialize_outputs (h, ICP_MEM_W))) return rc;
    // (first use; each buffer on its own, as the evaluation's)
    if (!P.blk && (rc = dalloc (h, &P.blk, B * icp_p2pl_nblk (p.m)))) return rc;
    if (!P.rec && (rc = dalloc (h, &P.rec, B * p.m))) return rc;
    if (!P.count && (rc = dalloc (h, &P.count, B))) return rc;
    P.valid = false;
    if (source == ICP_PAIRS_EVALUATED) {
        if ((rc = evaluation_search (h))) return rc;
        const icp_context::quality_buffers &Q = h->quality;
        const bool dist_on = max_dist > 0.f && !std::isinf (max_dist);
        icp_launch_pairs (source, Q.PF, Q.PM, p.M, Q.nn_id, p.m, p.batch, dist_on, dist_on ? (float) ((double) max_dist * (double) max_dist) : 0.f, P.blk, P.rec, P.count, h->stream);
    } else
        icp_launch_pairs (source, p.PF, p.PM, nullptr, p.nn_id, p.m, p.batch, false, 0.f, P.blk, P.rec, P.count, h->stream);
    HIPCHK (h, hipGetLastError ());
    P.n.assign (B, 0u);
    HIPCHK (h, hipMemcpyAsync (P.n.data (), P.count, B * sizeof (uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK (h, hipStreamSynchronize (h->stream));
    for (uint32_t b = 0; b < count; ++b) counts[b] = P.n[b];
    P.valid = true;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_correspondences_read (icp_handle h, uint32_t b, icp_pair_t *host_dst, uint32_t capacity, uint32_t *n) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (b >= h->p.batch) return fail (h, ICP_EINVAL, "batch index out of range");
    const icp_context::pairs_buffers &P = h->pairs;
    if (!P.valid) return fail (h, ICP_ESTATE, "icp_correspondences_read: no set has been computed since icp_init: icp_correspondences first");
    const uint32_t c = P.n[b];
    if (n) *n = c;
    if (capacity < c) return fail (h, ICP_EINVAL, "icp_correspondences_read: the set holds more records than `capacity`");
    if (c == 0u) return ICP_OK;
    if (!host_dst) return fail (h, ICP_EINVAL, "icp_correspondences_read: null destination");
    if ((rc = set_device (h))) return rc;
    HIPCHK (h, hipMemcpyAsync (host_dst, P.rec + (size_t) b * h->p.m, (size_t) c * sizeof (icp_pair_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK (h, hipStreamSynchronize (h->stream));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_correspondences_device_ptr (icp_handle h, uint32_t b, void **pairs, void **count_word) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (b >= h->p.batch) return fail (h, ICP_EINVAL, "batch index out of range");
    const icp_context::pairs_buffers &P = h->pairs;
    if (!P.rec || !P.count) return fail (h, ICP_ESTATE, "icp_correspondences_device_ptr: the buffers are allocated by the first icp_correspondences");
    if (pairs) *pairs = P.rec + (size_t) b * h->p.m;
    if (count_word) *count_word = P.count + b;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_write_cloud (icp_handle h, int which, const void *cloud, int block) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (h->p.m != 16384u) return fail (h, ICP_EINVAL, "getLMs produces 128 x 128 landmarks: m must be 16384");
    if (which != ICP_MEM_F && which != ICP_MEM_M) return fail (h, ICP_EINVAL, "which must be ICP_MEM_F or ICP_MEM_M");
    if (!cloud) return fail (h, ICP_EINVAL, "null pointer");
    if ((rc = set_device (h))) return rc;
    const uint32_t n = 640u * 480u;
    if ((rc = cloud_reserve (h, n))) return rc;
    note_inputs_change (h);
    HIPCHK (h, hipMemcpyAsync (h->dCloud, cloud, (size_t) n * 32, hipMemcpyHostToDevice, h->stream));
    icp_launch_get_lms (h->dCloud, which == ICP_MEM_F ? h->dF : h->dM, h->stream);
    if (which == ICP_MEM_M) normals_m_follow (h, 0u, 1u);
    HIPCHK (h, hipGetLastError ());
    HIPCHK (h, hipStreamSynchronize (h->stream));   // the source is pageable host memory
    (void) block;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_set_rgbd (icp_handle h, const icp_rgbd_t *cfg) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    const icp_rgbd_t c = cfg ? *cfg : icp_rgbd_default ();
    if (const char *why = icp_rgbd_refusal (c)) return fail (h, ICP_EINVAL, std::string ("icp_set_rgbd: ") + why);
    if (h->inited && !icp_rgbd_lattice_fits (c, h->p.side)) return fail (h, ICP_EINVAL, "icp_set_rgbd: the lattice of sqrt (m) x sqrt (m) landmarks leaves the image");
    if (h->track_submitted != h->track_collected) return fail (h, ICP_ESTATE, "icp_set_rgbd: tracked frames are in flight: collect them first (icp_track_collect)");
    h->rgbd = c;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_get_rgbd (icp_handle h, icp_rgbd_t *cfg) try
{
    api_guard guard_ (h);
    if (!h || !cfg) return ICP_EINVAL;
    *cfg = h->rgbd;
    return ICP_OK;
}
ICP_CATCH_ALL

// the device copy of `bytes` of image rows: *q holds at least that much
static int rgbd_reserve (icp_context *h, void **q, size_t *cap, size_t bytes)
{
    if (*cap >= bytes) return ICP_OK;
    if (*q) { HIPCHK (h, hipStreamSynchronize (h->stream)); (void) hipFree (*q); }
    *q = nullptr; *cap = 0;
    HIPCHK (h, hipMalloc (q, bytes));
    *cap = bytes;
    return ICP_OK;
}

int icp_write_rgbd (icp_handle h, int which, const uint16_t *depth, const uint8_t *rgb, int normals, int block) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (which != ICP_MEM_F && which != ICP_MEM_M) return fail (h, ICP_EINVAL, "which must be ICP_MEM_F or ICP_MEM_M");
    if (!depth) return fail (h, ICP_EINVAL, "null pointer");
    const icp_rgbd_t &c = h->rgbd;
    const uint32_t side = h->p.side;
    if ((uint64_t) side * side != h->p.m || !icp_rgbd_lattice_fits (c, side))
        return fail (h, ICP_EINVAL, "icp_write_rgbd: the lattice of sqrt (m) x sqrt (m) landmarks does not fit the image (icp_set_rgbd)");
    if ((rc = set_device (h))) return rc;
    // (whole image rows: contiguous in the caller's images, so each goes up by one copy)
    const icp_rgbd_region g = icp_rgbd_region_of (c, side, normals != 0);
    const uint32_t d0 = g.dy0, c0 = c.y0, c1 = c.y0 + c.step_y * (side - 1u) + 1u;
    const size_t dbytes = g.depth_bytes (false, c.width), cbytes = (size_t) (c1 - c0) * c.width * 3u;
    if ((rc = rgbd_reserve (h, (void **) &h->dRgbdDepth, &h->rgbd_depth_cap, dbytes))) return rc;
    if (rgb && (rc = rgbd_reserve (h, (void **) &h->dRgbdColour, &h->rgbd_colour_cap, cbytes))) return rc;
    note_inputs_change (h);
    HIPCHK (h, hipMemcpyAsync (h->dRgbdDepth, depth + (size_t) d0 * c.width, dbytes, hipMemcpyHostToDevice, h->stream));
    if (rgb) HIPCHK (h, hipMemcpyAsync (h->dRgbdColour, rgb + (size_t) c0 * c.width * 3u, cbytes, hipMemcpyHostToDevice, h->stream));
    icp_rgbd_args a {};
    a.c = c; a.depth = h->dRgbdDepth; a.rgb = rgb ? h->dRgbdColour : nullptr;
    a.dx0 = 0u; a.dy0 = d0; a.dpitch = c.width; a.cx0 = 0u; a.cy0 = c0; a.cpitch = c.width; a.cstep = 1u; a.side = side;
    a.out = reinterpret_cast<float4 *> (which == ICP_MEM_F ? h->dF : h->dM);
    // (the normals as icp_write of the object places them: registration 0's, behind whatever the stream holds)
    a.nrm = normals ? const_cast<float4 *> (static_cast<const float4 *> (mem_of (h, 0u, which == ICP_MEM_F ? ICP_MEM_NORMALS_F : ICP_MEM_NORMALS_M).ptr)) : nullptr;
    icp_launch_rgbd_lattice (a, h->stream);
    if (which == ICP_MEM_M) normals_m_follow (h, 0u, 1u);
    HIPCHK (h, hipGetLastError ());
    HIPCHK (h, hipStreamSynchronize (h->stream));   // the sources are pageable host memory
    (void) block;
    return ICP_OK;
}
ICP_CATCH_ALL

// Diagnostic: one form of the front end alone — whole images uploaded once, `reps` launches between two events on the handle's stream, into
// the cloud scratch (F, M and the normals stay as they are).
int icp_time_rgbd (icp_handle h, int dense, int normals, const uint16_t *depth, const uint8_t *rgb, uint32_t reps, float *us_per_launch) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (!depth || !us_per_launch || reps == 0u) return fail (h, ICP_EINVAL, "icp_time_rgbd: bad arguments");
    const icp_rgbd_t &c = h->rgbd;
    const uint32_t side = h->p.side, n = c.width * c.height;
    if (!dense && !icp_rgbd_lattice_fits (c, side)) return fail (h, ICP_EINVAL, "icp_time_rgbd: the lattice does not fit the image (icp_set_rgbd)");
    if ((rc = set_device (h))) return rc;
    if ((rc = rgbd_reserve (h, (void **) &h->dRgbdDepth, &h->rgbd_depth_cap, (size_t) n * 2u))) return rc;
    if (rgb && (rc = rgbd_reserve (h, (void **) &h->dRgbdColour, &h->rgbd_colour_cap, (size_t) n * 3u))) return rc;
    if ((rc = cloud_reserve (h, n))) return rc;                          // (n >= side^2: the lattice lies inside the image)
    HIPCHK (h, hipMemcpyAsync (h->dRgbdDepth, depth, (size_t) n * 2u, hipMemcpyHostToDevice, h->stream));
    if (rgb) HIPCHK (h, hipMemcpyAsync (h->dRgbdColour, rgb, (size_t) n * 3u, hipMemcpyHostToDevice, h->stream));
    icp_rgbd_args a {};
    a.c = c; a.depth = h->dRgbdDepth; a.rgb = rgb ? h->dRgbdColour : nullptr;
    a.dpitch = a.cpitch = c.width; a.cstep = 1u; a.side = side;
    a.out = reinterpret_cast<float4 *> (h->dCloud); a.nrm = normals ? reinterpret_cast<float4 *> (h->dCloudOut) : nullptr;
    auto launch = [&] () { if (dense) icp_launch_rgbd_dense (a, h->stream); else icp_launch_rgbd_lattice (a, h->stream); };
    launch ();                                                           // (untimed: the code object is loaded)
    HIPCHK (h, hipEventRecord (h->ev0, h->stream));
    for (uint32_t i = 0; i < reps; ++i) launch ();
    HIPCHK (h, hipEventRecord (h->ev1, h->stream));
    HIPCHK (h, hipGetLastError ());
    HIPCHK (h, hipEventSynchronize (h->ev1));
    float ms = 0.f;
    HIPCHK (h, hipEventElapsedTime (&ms, h->ev0, h->ev1));
    *us_per_launch = ms * 1e3f / (float) reps;
    return ICP_OK;
}
ICP_CATCH_ALL

// The view of a TSDF volume (icp_tsdf.hip) as the landmarks of F or M: the volume's ray cast writes the handle's buffers itself, on the
// volume's stream, between two synchronisations — the handle's stream has drained before and the cast has finished after.
int icp_tsdf_raycast_to (icp_tsdf_handle t, icp_handle h, int which, const icp_rgbd_t *cam, const float *pose12, float z_near, float z_far, int normals) try
{
    if (!t) return ICP_EINVAL;
    if (!h) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_raycast_to: null handle");
    api_guard guard_ (h);
    if (!h->inited) return tsdf_fail (t, ICP_ESTATE, "icp_tsdf_raycast_to: icp_init has not been called on the handle");
    if (h->device != t->device) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_raycast_to: the handle lives on another device than the volume");
    if (which != ICP_MEM_F && which != ICP_MEM_M) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_raycast_to: which must be ICP_MEM_F or ICP_MEM_M");
    if (h->track_submitted != h->track_collected) return tsdf_fail (t, ICP_ESTATE, "icp_tsdf_raycast_to: tracked frames are in flight: collect them first (icp_track_collect)");
    const uint32_t side = h->p.side;
    if ((uint64_t) side * side != h->p.m) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_raycast_to: m is not a square number");
    icp_tsdf_cast_args a;
    int rc = tsdf_cast_prepare (t, "icp_tsdf_raycast_to", cam ? cam : &h->rgbd, pose12, z_near, z_far, side, &a); if (rc) return rc;
    if ((rc = need (h, false)) || (rc = set_device (h))) return tsdf_fail (t, rc, "icp_tsdf_raycast_to: " + h->err);
    a.out = reinterpret_cast<float4 *> (which == ICP_MEM_F ? h->dF : h->dM);
    a.nrm = normals ? const_cast<float4 *> (static_cast<const float4 *> (mem_of (h, 0u, which == ICP_MEM_F ? ICP_MEM_NORMALS_F : ICP_MEM_NORMALS_M).ptr)) : nullptr;
    auto chk = [&] (hipError_t e, const char *what) { return e == hipSuccess ? ICP_OK : tsdf_fail (t, ICP_EHIP, std::string (what) + ": " + hipGetErrorString (e)); };
    note_inputs_change (h);
    if ((rc = chk (hipStreamSynchronize (h->stream), "hipStreamSynchronize"))) return rc;
    tsdf_launch_raycast (a, t->stream);
    if ((rc = chk (hipGetLastError (), "icp_tsdf_raycast_to"))) return rc;
    if ((rc = chk (hipStreamSynchronize (t->stream), "hipStreamSynchronize"))) return rc;
    if (which == ICP_MEM_M) {
        normals_m_follow (h, 0u, 1u);
        if ((rc = chk (hipGetLastError (), "icp_tsdf_raycast_to"))) return rc;
        if ((rc = chk (hipStreamSynchronize (h->stream), "hipStreamSynchronize"))) return rc;
    }
    return ICP_OK;
}
ICP_CATCH_ALL

// F or M of registration 0 registered against a TSDF volume (icp_tsdf_register.hip), device to device: the volume's kernels read the
// handle's buffer on the volume's stream, behind everything the handle's stream holds.  Nothing in the handle changes.
int icp_tsdf_register_from (icp_tsdf_handle t, const icp_tsdf_register_t *opt, icp_handle h, int which, const float *pose12, icp_tsdf_registration_t *out) try
{
    if (!t) return ICP_EINVAL;
    if (!h) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_register_from: null handle");
    api_guard guard_ (h);
    if (!h->inited) return tsdf_fail (t, ICP_ESTATE, "icp_tsdf_register_from: icp_init has not been called on the handle");
    if (h->device != t->device) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_register_from: the handle lives on another device than the volume");
    if (which != ICP_MEM_F && which != ICP_MEM_M) return tsdf_fail (t, ICP_EINVAL, "icp_tsdf_register_from: which must be ICP_MEM_F or ICP_MEM_M");
    if (h->track_submitted != h->track_collected) return tsdf_fail (t, ICP_ESTATE, "icp_tsdf_register_from: tracked frames are in flight: collect them first (icp_track_collect)");
    const void *cloud = which == ICP_MEM_F ? h->dF : h->dM;
    int rc = tsdf_register_check (t, "icp_tsdf_register_from", opt, cloud, h->p.m, pose12, out); if (rc) return rc;
    if ((rc = need (h, false)) || (rc = set_device (h))) return tsdf_fail (t, rc, "icp_tsdf_register_from: " + h->err);
    if (hipError_t e = hipStreamSynchronize (h->stream); e != hipSuccess) return tsdf_fail (t, ICP_EHIP, std::string ("hipStreamSynchronize: ") + hipGetErrorString (e));
    return tsdf_register_run (t, opt, cloud, h->p.m, pose12, out);
}
ICP_CATCH_ALL

int icp_transform_cloud (icp_handle h, const void *host_in, void *host_out, uint32_t n) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (!host_in || !host_out || n == 0) return fail (h, ICP_EINVAL, "bad arguments");
    if ((rc = set_device (h))) return rc;
    if ((rc = cloud_reserve (h, n))) return rc;
    HIPCHK (h, hipMemcpyAsync (h->dCloud, host_in, (size_t) n * 32, hipMemcpyHostToDevice, h->stream));
    icp_launch_transform_cloud (h->dCloud, h->dCloudOut, h->p.st, n, h->stream);
    HIPCHK (h, hipGetLastError ());
    HIPCHK (h, hipMemcpyAsync (host_out, h->dCloudOut, (size_t) n * 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK (h, hipStreamSynchronize (h->stream));
    return ICP_OK;
}
ICP_CATCH_ALL


int icp_transform_cloud_ex (icp_handle h, int kind, const float *T, const void *host_in, void *host_out, uint32_t n) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (kind != ICP_TRANSFORM_QUATERNION && kind != ICP_TRANSFORM_QUATERNION_2 && kind != ICP_TRANSFORM_MATRIX)
        return fail (h, ICP_EINVAL, "icp_transform_cloud_ex: unknown transformation kind");
    if (!T || !host_in || !host_out || n == 0) return fail (h, ICP_EINVAL, "bad arguments");
    int rc = set_device (h); if (rc) return rc;
    if ((rc = cloud_reserve (h, n))) return rc;
    HIPCHK (h, hipMemcpyAsync (h->dCloud, host_in, (size_t) n * 32, hipMemcpyHostToDevice, h->stream));
    icp_launch_transform_cloud_ex (kind, h->dCloud, h->dCloudOut, T, n, h->stream);
    HIPCHK (h, hipGetLastError ());
    HIPCHK (h, hipMemcpyAsync (host_out, h->dCloudOut, (size_t) n * 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK (h, hipStreamSynchronize (h->stream));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_power_method (int device, int rot, int power_mode, const float *S11, const float *means8, float *Tk8, float *Rk9, uint32_t *iters) try
{
    if (!S11 || !means8 || !Tk8) return fail (nullptr, ICP_EINVAL, "icp_power_method: null pointer");
    if ((rot != ICP_ROT_EIGEN && rot != ICP_ROT_POWER_METHOD) || (power_mode != ICP_POWER_LITERAL && power_mode != ICP_POWER_SQUARED))
        return fail (nullptr, ICP_EINVAL, "icp_power_method: rot must be 0|1 and power_mode 0|1");
    { int rc = gfx950_device (device, "icp_power_method"); if (rc) return rc; }
    HIPCHK (nullptr, hipSetDevice (device));
    float *d = nullptr;
    HIPCHK (nullptr, hipMalloc ((void **) &d, (19 + 18) * sizeof (float)));
    float in[19], out[18];
    std::memcpy (in, S11, 11 * sizeof (float)); std::memcpy (in + 11, means8, 8 * sizeof (float));
    hipError_t e = hipMemcpy (d, in, sizeof in, hipMemcpyHostToDevice);
    if (e == hipSuccess) { icp_launch_rotation_solver (rot, power_mode, d, d + 19, nullptr); e = hipGetLastError (); }
    if (e == hipSuccess) e = hipMemcpy (out, d + 19, sizeof out, hipMemcpyDeviceToHost);      // (blocking: waits for the kernel on the null stream)
    (void) hipFree (d);
    if (e != hipSuccess) return fail (nullptr, ICP_EHIP, std::string ("icp_power_method: ") + hipGetErrorString (e));
    std::memcpy (Tk8, out, 8 * sizeof (float));
    if (Rk9) std::memcpy (Rk9, out + 8, 9 * sizeof (float));
    if (iters) std::memcpy (iters, out + 17, sizeof (uint32_t));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_reset_transform (icp_handle h) try
{   // T <- identity, k <- 0 (what ICPStep::init uploads, src/ICP/algorithms.cpp:4486-4493); enqueue only
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if ((rc = set_device (h))) return rc;
    note_enqueue (h);
    icp_launch_reset_state (h->p, h->stream, 1);
    HIPCHK (h, hipGetLastError ());
    h->k_base = 0;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_time_run_fixed (icp_handle h, uint32_t iterations, uint32_t reps, int from_identity, float *ms_total) try
{
    api_guard guard_ (h);
    int rc = need (h, true); if (rc) return rc;
    if (!ms_total || iterations == 0 || reps == 0) return fail (h, ICP_EINVAL, "bad arguments");
    if ((rc = set_device (h))) return rc;
    hipGraphExec_t exec;
    if ((rc = get_graph (h, iterations, 0, &exec, from_identity != 0))) return rc;     // from_identity: every pass is a fresh registration
    HIPCHK (h, hipEventRecord (h->ev0, h->stream));
    for (uint32_t r = 0; r < reps; ++r) HIPCHK (h, hipGraphLaunch (exec, h->stream));
    h->hstate_fresh = false; h->k_base = -1; note_outputs_stored (h);
    HIPCHK (h, hipEventRecord (h->ev1, h->stream));
    HIPCHK (h, hipStreamSynchronize (h->stream));                       // (not hipEventSynchronize: its wake-up now and then takes 0.5 ms, tools/diag/overhead.py)
    HIPCHK (h, hipEventElapsedTime (ms_total, h->ev0, h->ev1));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_time_run_fixed_tail (icp_handle h, uint32_t iterations, uint32_t reps, int from_identity, float *ms_timed, uint32_t *reps_timed) try
{
    api_guard guard_ (h);
    int rc = need (h, true); if (rc) return rc;
    if (!ms_timed || !reps_timed || iterations == 0 || reps == 0) return fail (h, ICP_EINVAL, "bad arguments");
    if ((rc = set_device (h))) return rc;
    hipGraphExec_t exec;
    if ((rc = get_graph (h, iterations, 0, &exec, from_identity != 0))) return rc;
    // the first event goes in BEHIND the first pass: a marker recorded on an idle stream delays the graph launched right after it by
    // 0.1 - 0.25 ms (7.22 - 7.39 ms for 20 passes of 0.357 ms against 7.17 ms wall-clock for the same launches without events;
    // with the GPU busy when the marker arrives: 7.14 ms, tools/diag/overhead.py); the events then bracket the passes 2 .. reps
    const uint32_t lead = reps >= 2u ? 1u : 0u;
    if (lead) HIPCHK (h, hipGraphLaunch (exec, h->stream));
    HIPCHK (h, hipEventRecord (h->ev0, h->stream));
    for (uint32_t r = lead; r < reps; ++r) HIPCHK (h, hipGraphLaunch (exec, h->stream));
    h->hstate_fresh = false; h->k_base = -1; note_outputs_stored (h);
    HIPCHK (h, hipEventRecord (h->ev1, h->stream));
    HIPCHK (h, hipStreamSynchronize (h->stream));                       // (not hipEventSynchronize: its wake-up now and then takes 0.5 ms, tools/diag/overhead.py)
    HIPCHK (h, hipEventElapsedTime (ms_timed, h->ev0, h->ev1));
    *reps_timed = reps - lead;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_run_form (icp_handle h, int *form) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (!form) return fail (h, ICP_EINVAL, "null output");
    *form = icp_route_of (h->p).chained ? ICP_FORM_CHAINED : ICP_FORM_SEPARATE;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_search_layout (icp_handle h, int *dense, int *tile, int *stage2) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    icp_search_layout_of (h->p, dense, tile, stage2);
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_launches_per_iteration (icp_handle h, uint32_t *n) try
{
    api_guard guard_ (h);
    int rc = need (h, false); if (rc) return rc;
    if (!n) return fail (h, ICP_EINVAL, "null output");
    *n = icp_route_of (h->p).launches;
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_time_masked (icp_handle h, uint32_t mask, uint32_t iterations, uint32_t reps, float *ms_total) try
{
    api_guard guard_ (h);
    int rc = need (h, true); if (rc) return rc;
    if (!ms_total || iterations == 0 || reps == 0 || mask == 0) return fail (h, ICP_EINVAL, "bad arguments");
    if ((rc = set_device (h))) return rc;
    icp_params p = h->p; p.check = 0; p.hmirror = nullptr; p.hstate = nullptr;
    note_enqueue (h); note_outputs_stored (h);                          // (the masked graphs change the device state: the pinned mirror is stale)
    graph_entry ge;
    // (the per-query outputs follow the policy of the fixed-length graphs: stored by the last iteration only in fused mode)
    if ((rc = capture_graph (h, [&] {
             for (uint32_t k = 0; k < iterations; ++k) { p.emit = (k + 1 == iterations) ? 1 : 0; icp_launch_masked (p, h->stream, mask, &h->recip, h->median, h->adaptive); }
         }, &ge))) return rc;
    hipError_t e = hipGraphLaunch (ge.exec, h->stream);                 // warm-up
    if (e == hipSuccess) e = hipEventRecord (h->ev0, h->stream);
    for (uint32_t r = 0; r < reps && e == hipSuccess; ++r) e = hipGraphLaunch (ge.exec, h->stream);
    if (e == hipSuccess) e = hipEventRecord (h->ev1, h->stream);
    if (e == hipSuccess) e = hipEventSynchronize (h->ev1);
    if (e == hipSuccess) e = hipEventElapsedTime (ms_total, h->ev0, h->ev1);
    (void) hipGraphExecDestroy (ge.exec); (void) hipGraphDestroy (ge.graph);
    if (e != hipSuccess) return fail (h, ICP_EHIP, std::string ("icp_time_masked: ") + hipGetErrorString (e));
    return ICP_OK;
}
ICP_CATCH_ALL

#ifdef ICP_DBG_STAMPS
__attribute__ ((visibility ("default")))          // (diagnostic builds only: not part of the ABI)
#endif
int icp_debug_stamps (icp_handle h, unsigned long long *out, uint32_t nblocks) try
{   // diagnostic builds (ICP_DBG_STAMPS): one k_search launch, per-block s_memtime stamps
    api_guard guard_ (h);
    int rc = need (h, true); if (rc) return rc;
    if (!out || nblocks == 0) return fail (h, ICP_EINVAL, "bad arguments");
    if ((rc = set_device (h))) return rc;
    unsigned long long *d = nullptr;
    HIPCHK (h, hipMalloc ((void **) &d, (size_t) nblocks * 16 * 8));
    hipError_t e = hipMemset (d, 0, (size_t) nblocks * 16 * 8);
    icp_params p = h->p; p.check = 0; p.dbg = d; p.hmirror = nullptr; p.hstate = nullptr;
    note_enqueue (h); note_outputs_stored (h);
    if (e == hipSuccess) {
        if (icp_route_of (p).chained) icp_launch_chain (p, h->stream, 2);
        else icp_launch_masked (p, h->stream, p.fused ? 1u | 8u : 1u, &h->recip, h->median, h->adaptive);
        e = hipGetLastError ();
    }
    if (e == hipSuccess) e = hipStreamSynchronize (h->stream);
    if (e == hipSuccess) e = hipMemcpy (out, d, (size_t) nblocks * 16 * 8, hipMemcpyDeviceToHost);
    (void) hipFree (d);
    if (e != hipSuccess) return fail (h, ICP_EHIP, std::string ("icp_debug_stamps: ") + hipGetErrorString (e));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_profile_run (icp_handle h, uint32_t iterations, float *out_ms, float *total_ms) try
{
    api_guard guard_ (h);
    int rc = need (h, true); if (rc) return rc;
    if (!out_ms || iterations == 0) return fail (h, ICP_EINVAL, "bad arguments");
    if ((rc = set_device (h))) return rc;
    icp_params p = h->p; p.check = 0; p.emit = 1; p.hmirror = nullptr; p.hstate = nullptr;
    note_enqueue (h); note_outputs_stored (h);
    std::vector<hipEvent_t> ev ((size_t) iterations * 5, nullptr);
    hipError_t e = hipSuccess;
    for (auto &x : ev) if (e == hipSuccess) e = hipEventCreate (&x);
    // the stages as separate launches (the chained form has no stage boundaries to time), events around each
    for (uint32_t r = 0; r < iterations && e == hipSuccess; ++r) {
        hipEvent_t *x = &ev[(size_t) r * 5];
        e = hipEventRecord (x[0], h->stream);                                             // (trimming, adaptive trimming, one-to-one, the pair filter, reciprocal correspondences on: their passes time with the search)
        for (int k = 0; k < 4; ++k) {
            icp_launch_masked (p, h->stream, 1u << k, &h->recip, h->median, h->adaptive);
            if (e == hipSuccess) e = hipEventRecord (x[k + 1], h->stream);
        }
    }
    if (e == hipSuccess) e = hipGetLastError ();
    if (e == hipSuccess) e = hipStreamSynchronize (h->stream);
    for (uint32_t r = 0; r < iterations && e == hipSuccess; ++r)
        for (int k = 0; k < 4 && e == hipSuccess; ++k)
            e = hipEventElapsedTime (&out_ms[(size_t) r * 4 + k], ev[(size_t) r * 5 + k], ev[(size_t) r * 5 + k + 1]);
    if (e == hipSuccess && total_ms) e = hipEventElapsedTime (total_ms, ev[0], ev[(size_t) iterations * 5 - 1]);
    for (auto &x : ev) if (x) (void) hipEventDestroy (x);
    if (e != hipSuccess) return fail (h, ICP_EHIP, std::string ("icp_profile_run: ") + hipGetErrorString (e));
    return ICP_OK;
}
ICP_CATCH_ALL

int icp_time_kernels (icp_handle h, uint32_t reps, float *out_ms4) try
{
    api_guard guard_ (h);
    if (!h) return ICP_EINVAL;
    if (!out_ms4 || reps == 0) return fail (h, ICP_EINVAL, "bad arguments");
    std::vector<float> t ((size_t) reps * 4);
    int rc = icp_profile_run (h, reps, t.data (), nullptr);
    if (rc) return rc;
    for (int k = 0; k < 4; ++k) {
        double acc = 0.0;
        for (uint32_t r = 0; r < reps; ++r) acc += t[(size_t) r * 4 + k];
        out_ms4[k] = (float) (acc / reps);
    }
    return ICP_OK;
}
ICP_CATCH_ALL

}  // extern "C"
