// icp_kernels.h — launch parameters shared by the HIP kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "icp_device.h"
#include "icp_search_select.h"

// fused finalize: beyond this many 128-block groups (|F| > 16384) the first level of the moment tree gets a kernel of its own
// (k_moment_level1: the block moments come from all over the chip; one CU fetching 147 KB of them at |F| = 65536 costs more than
// a launch that spreads the fetch — finalize 6.29 -> 5.71 us for the two launches, iteration 19.4 -> 18.55 us; same tree, same bits)
#ifndef ICP_L1_MIN_GROUPS
#define ICP_L1_MIN_GROUPS 2u
#endif
// The band of a 640 x 480 frame getLMs reads (kernels/icp_kernels.cl:63-76: landmark (i, j) = pixel (col 65 + 4 i, row 49 + 3 j)):
// rows 49, 52, .., 430 and, of each, the pixels 65 .. 573.
#define ICP_BAND_ROW0 49u
#define ICP_BAND_ROW_STEP 3u
#define ICP_BAND_ROWS 128u
#define ICP_BAND_COL0 65u
#define ICP_BAND_COLS 509u
#define ICP_BAND_ROW_BYTES (ICP_BAND_COLS * 32u)
#define ICP_BAND_BYTES ((size_t) ICP_BAND_ROWS * ICP_BAND_ROW_BYTES)
#define ICP_TBOX 1024u            // representatives per LDS tile box of the 1024-tile dense search (k_reps_and_boxes, k_search)
#ifndef ICP_OL_BOXED_MIN
#define ICP_OL_BOXED_MIN 128u        // the list of the representatives at the origin: beyond this length ordered by colour, its chunks of 8 tested by their boxes before they are scanned
#endif
#define ICP_OL_MASKS(nr) ((nr) + 1u + 2u * (((nr) + 7u) / 8u))                            // float4 offset of the ballots inside a registration's OL
#define ICP_OL_STRIDE(nr) (ICP_OL_MASKS (nr) + ((nr) + 127u) / 128u)                          // float4 per registration of icp_params::OL
#define ICP_CHUNK 1024u          // fixed points per block in the stable RBC placement

struct icp_params {
    // problem
    uint32_t m, nr, batch;
    uint32_t side, nrx, nry;     // landmark grid side and representative grid (getReps)
    uint32_t ng_magic;                               // floor (2^32 / ng) + 1 for ng = groups of 128 block moments: task / ng = umulhi (task, magic)
    uint32_t side_magic, cellw_magic, cellh_magic;   // floor (2^32 / d) + 1 for d = side, side / nrx, side / nry (0: the set is no square grid): n / d = umulhi (n, magic)
    float a, c;
    float dist_scale;            // f_g of the metric text: reported distance (NN_ID.dist, the weights' input) = dist_scale * (geo + a pho); default 1
    int weighted, rot, power_mode, check;
    int chain;                   // fused mode, one launch per iteration (finalize in the next search's prologue): 0 never, 1 automatic, 2 always
    int fused;                   // 0: reference-order reductions (3 global trees), 1: single-pass double moments
    int emit;                    // fused mode: this search also stores the per-query outputs (nn_id, PF, PM; rid unless pruning needs it anyway); graphs of a
                                 // fixed length switch it off for all but their last iteration (nothing in between can read them)
    double tan_half_thr, trans_thr;
    // derived sizes
    uint32_t nwg;                // 128-element groups = ceil(m/128)         (weights / means partials)
    uint32_t nwp;                // weight partials padded (multiple of 4 unless 1)
    uint32_t G;                  // S columns = ceil4(m)/4                    (icpSijProducts work-items)
    uint32_t nsp;                // reduce_sum_f work-groups per S row, padded (multiple of 4 unless 1)
    uint32_t nchunk;             // ceil(m / ICP_CHUNK)
    uint32_t nb;                 // fused mode: blocks of 64 pairs = ceil(m/64)
    // inputs / RBC
    const float *F, *M;          // [batch][m][8]
    float *R;                    // [batch][nr][8]
    float4 *GB;                  // [batch][2*(n16+n32)] geometry bounding boxes (lo, hi) of the groups of 16 representatives, then of the tiles of 1024
    uint32_t n16, n1k;           // ceil(nr/16), ceil(nr/tbox)
    uint32_t tbox;               // representatives per tile box (k_tile_boxes): the LDS tile of the dense k_search for multi-tile sets, 256 or 1024
    uint32_t gtile;              // stage-1 pruning groups of 16: 0 = 16 consecutive representatives, 1 + log2 (nrx / 4) = 4 x 4 tiles of the representative grid
    uint32_t xcdmap;             // dense search: XCD-aware block -> tile bands (a single large registration: halves the fabric-side traffic)
    uint32_t warm_seed;          // diagnostics (ICP_AMD_WARM_SEED=1): a registration's first search is seeded with p.rid as it stands (the previous
                                 // registration's answer) instead of the query's own grid cell
    uint32_t s2wave;             // stage 2 of the dense search with lanes = candidates (lists of >= ICP_S2_WAVE_MIN candidates on average: see k_search)
    uint32_t nrm_grid;           // point-to-plane normals (icp_set_normals): the grid width of ICP_NORMALS_GRID (buildRBC computes them), 0: ICP_NORMALS_GIVEN
                                 // (this and the next two p2pl fields fill alignment holes: no other field moves — see the static_assert below)
    float *XP;                   // [batch][m][8]  permuted database (RBCConstruct D_OUT_X_P)
    float *XQ;                   // [batch][m][8]  same, lane 3 = original index bits (search copy)
    float4 *OL;                  // [batch][ICP_OL_STRIDE (nr)]  the representatives at the origin (invalid points), ascending: [0].x = their number (bits),
                                 // [1 .. nr]: (r, g, b, index bits) each — kept out of the pruning boxes, scanned by the queries near the origin (dense
                                 // search) —, behind them the colour boxes (lo rgb, hi rgb) of the chunks of 8 consecutive entries, then one 64-bit ballot per 64
                                 // representatives ([0].y: the arrival counter of k_reps_and_boxes' blocks, zero between constructions; a search looks the seed of a query
                                 // whose own seed is of the wrong kind up in the ballots: icp_other_kind_near)
    float4 *LB;                  // [batch][3 * nlb]  6-D bounding boxes of the list chunks (16 consecutive positions of one list, chunk c >= 1 of list r at
                                 // index (O[r] >> 4) + c: k_list_boxes) as [lo.x lo.y lo.z lo.r | lo.g lo.b hi.x hi.y | hi.z hi.r hi.g hi.b]
    uint32_t nlb;                // m / 16 + 2 boxes per registration
    uint32_t metric;             // ICP_METRIC_POINT_TO_POINT (0, the default), ICP_METRIC_POINT_TO_PLANE or ICP_METRIC_COLORED (icp_p2pl.hip)
    uint32_t *rep_src, *owner, *N, *O, *perm, *chunk_hist;   // [batch][...]; N: [2][batch][nr] — [0] the length of a list AS THE SEARCH SCANS IT (k_search reads
                                 // p.N: a long list without the tail members that repeat an earlier member bit for bit, k_list_boxes), [1] = ICP_N_FULL: the list's
                                 // length N of the construction (RBCConstruct's output, ICP_MEM_RBC_N); the two differ for long lists with duplicates only
    uint2 *blist; uint32_t *bn; uint8_t *brank;   // buildRBC of the latency-bound sizes (k_place_lists): per block of 64 fixed points its (owner, count) list
                                                  // [batch][nb][64] and the list's length [batch][nb]; rank of a point inside its block [batch][m]
    // per-iteration
    uint32_t *rid;               // [batch][m]
    icp_dist_id *nn_id;          // [batch][m]
    float4 *PF, *PM;             // [batch][m]  (nn.xyz, w) / (q'.xyz, dist)
    float *wpart;                // [batch][2*nwp]   even / odd half-trees of every 128-query group
    float4 *mpart;               // [batch][2][nwg]
    float4 *mscr;                // [batch][2][ceil(nwg/128)]  scratch of the multi-level icpGMean
    float *spart;                // [batch][11][nsp*8] 8 residue sub-trees per work-group
    double *mom;                 // [batch][2][18][nb]  fused mode: per-block moment partials (double-buffered for the chain)
    double *ml1;                 // [batch][18][ceil(nb/128)]  fused mode, large sets: first tree level of the moments (k_moment_level1)
    icp_reg_state *cst;          // [batch][2]  chained fused mode: state slots, launch j reads slot j&1 and writes the other
    uint32_t slot;               // chained fused mode: slot this launch reads
    float p2pl_mu;               // point-to-plane: the share mu of the point-to-point term
    icp_reg_state *st;           // [batch]
    icp_reg_state *st_prev;      // [batch]  .T = the transform the last executed search used (stored by every finalize; everything else stays zero):
                                 // icp_launch_search on it reproduces that iteration's per-query outputs (checked runs do not store them on the way)
    unsigned long long *dbg;     // diagnostic builds only (ICP_DBG_STAMPS): [blocks][16] s_memtime stamps
    // checked runs driven from the host (icp_run, icp_track_*: see run_ctl in icp_capi.hip): progress words and the final states in
    // host memory the device writes straight into (fine-grained pinned allocations; nullptr: nobody is watching)
    unsigned long long *hmirror; // [batch]  ICP_MIRROR_WORD (epoch, done, k) stored by the lane that publishes a registration's state
    icp_reg_state *hstate;       // [batch]  the final state of a run, stored by its end kernel in front of the word's FINAL bit
    uint32_t epoch;              // tag of the run the words belong to (a word of another epoch is stale)
    uint32_t gicp;               // a metric that needs the moving frame's normals, whatever the metric word: 1 plane-to-plane (icp_set_plane_to_plane,
                                 // epsilon > 0; icp_gicp: in effect), 2 symmetric (icp_set_symmetric; icp_sym: in effect), 0 neither.  With both
                                 // switched on it is 1 and every run is refused (icp_run.hip: need).  It fills the alignment hole behind `epoch`:
                                 // no other field moves.  epsilon itself is a device word (icp_gicp_eps)
    // tracking with frames gated on the device (icp_capi.hip: track_submit): consecutive frames alternate between two streams, so the
    // launches of a frame that has converged and the next frame's run concurrently
    uint32_t *run_flag;          // [batch]  epoch of the run that has converged: its remaining launches leave at once and WRITE NOTHING (one flag per
                                 // stream: it has to outlive the run's last queued launch, and the next frame on the other stream may converge before that)
    uint32_t *track_seq;         // number of the last registration of a tracked sequence that has finished (k_gate waits on it)
    uint32_t seq_value;          // this registration's number
    uint32_t no_state_reset;     // buildRBC leaves k / done alone (it runs ahead of the previous frame's end; the run's first launch resets them)
    // correspondence rejection (icp_set_rejection; all zero = off, the reference's behaviour): a rejected pair keeps its correspondence
    // and gets the weight +0 — its moment, mean and S terms are written as zeros —, REGULAR mode then divides by sum W like WEIGHTED
    uint32_t reject;             // ICP_REJECT_* flags (bit 0: a pair with an invalid endpoint, a point at the origin) | ICP_REJECT_DIST_ON; 0: off
    float reject_d2;             // ICP_REJECT_DIST_ON: max_dist^2 rounded to float (a pair is rejected when !(geo <= reject_d2))
    float reject_max_dist;       // max_dist as it was set (icp_get_rejection)
    // trimmed ICP (icp_set_trimming): with ICP_REJECT_TRIM_ON in `reject`, each iteration keeps the closest fraction trim_keep of the
    // pairs rejection leaves (icp_trim.hip).  The field sits in the struct's tail padding: sizeof (icp_params) must not grow — every
    // kernel takes the struct by value, and the hidden arguments (the grid's size) lie behind it in the argument segment.
    float trim_keep;             // keep_fraction in (0, 1] while trimming is on; 0 while it is off
};
#define ICP_REJECT_DIST_ON 0x80000000u   // icp_params::reject: the distance test is on (one scalar test of one word says whether anything is)
#define ICP_REJECT_TRIM_ON 0x40000000u   // icp_params::reject: trimming is on (the REJ kernels, plus the selection and the apply pass: icp_route_of)
#define ICP_REJECT_ROBUST_SHIFT 28u
#define ICP_REJECT_ROBUST_MASK 0x30000000u   // icp_params::reject: the robust loss (icp_set_robust_loss): ICP_ROBUST_* << 28, 0: off
#define ICP_REJECT_UNIQUE_ON 0x08000000u   // icp_params::reject: one-to-one correspondences are on (icp_set_unique: the REJ kernels, plus claim and resolve: icp_launch_unique)
#define ICP_REJECT_BOUNDARY_ON 0x04000000u   // icp_params::reject: boundary rejection is on (icp_set_boundary_rejection: the REJ kernels, plus k_pair_filter: icp_launch_pair_filter)
#define ICP_REJECT_NORMAL_ON 0x02000000u   // icp_params::reject: rejection by normal compatibility is on (icp_set_normal_rejection: likewise; the moving frame's normals are needed)
#define ICP_REJECT_FILTER_MASK (ICP_REJECT_BOUNDARY_ON | ICP_REJECT_NORMAL_ON)
#define ICP_REJECT_RECIPROCAL_ON 0x01000000u   // icp_params::reject: reciprocal correspondences are on (icp_set_reciprocal: the REJ kernels, plus the back search and k_reciprocal: icp_launch_reciprocal)
#define ICP_REJECT_PROJECTIVE_ON 0x00800000u   // icp_params::reject: projective data association is on (icp_set_projective: k_projective in place of the search: icp_launch_projective)
#define ICP_REJECT_MEDIAN_ON 0x00400000u   // icp_params::reject: median-distance rejection is on (icp_set_median_rejection: the REJ kernels, plus the rule's launches: icp_launch_median)
#define ICP_REJECT_TRIM_ADAPTIVE 0x00200000u   // icp_params::reject, beside ICP_REJECT_TRIM_ON: adaptive trimming's selection fills trimming's words (icp_set_adaptive_trimming: icp_launch_adaptive_trim in icp_launch_trim_select's place)
static_assert (sizeof (icp_params) == 480, "icp_params grew: the hidden kernel arguments of every kernel would move");

// rejection on: the sum-W formulas in every mode, and a step of nothing accepted (sum W == 0) is the identity
static __host__ __device__ __forceinline__ bool icp_rejecting (const icp_params &p) { return p.reject != 0u; }
static __host__ __device__ __forceinline__ bool icp_trimming (const icp_params &p) { return (p.reject & ICP_REJECT_TRIM_ON) != 0u; }
// one-to-one correspondences (icp_unique.hip): of the candidates that share a fixed point only the closest keeps its weight
static __host__ __device__ __forceinline__ bool icp_unique (const icp_params &p) { return (p.reject & ICP_REJECT_UNIQUE_ON) != 0u; }
// the pair filter (icp_pair_filter.hip): rejection at the fixed grid's boundary and / or by normal compatibility, one pass behind the search
static __host__ __device__ __forceinline__ bool icp_pair_filter (const icp_params &p) { return (p.reject & ICP_REJECT_FILTER_MASK) != 0u; }
// reciprocal correspondences (icp_reciprocal.hip): a candidate keeps its weight only if its fixed point's back search into M finds it again
static __host__ __device__ __forceinline__ bool icp_reciprocal (const icp_params &p) { return (p.reject & ICP_REJECT_RECIPROCAL_ON) != 0u; }
// projective data association (icp_projective.hip): the pairs come from a projection onto the fixed grid instead of the RBC search
static __host__ __device__ __forceinline__ bool icp_projective (const icp_params &p) { return (p.reject & ICP_REJECT_PROJECTIVE_ON) != 0u; }
// median-distance rejection (icp_median.hip): a candidate farther than factor times the iteration's median pair distance loses its weight
static __host__ __device__ __forceinline__ bool icp_median (const icp_params &p) { return (p.reject & ICP_REJECT_MEDIAN_ON) != 0u; }
// adaptive trimming (icp_adaptive_trim.hip): trimming (icp_trimming holds too) whose kept fraction the selection chooses per iteration
static __host__ __device__ __forceinline__ bool icp_adaptive_trim (const icp_params &p) { return (p.reject & ICP_REJECT_TRIM_ADAPTIVE) != 0u; }
// the moving frame's normals are needed: by a metric (p.gicp: plane-to-plane, symmetric) or by normal rejection, whatever the metric
static __host__ __device__ __forceinline__ bool icp_moving_normals (const icp_params &p) { return p.gicp != 0u || (p.reject & ICP_REJECT_NORMAL_ON) != 0u; }
// the robust loss's kind (ICP_ROBUST_HUBER 1, CAUCHY 2, TUKEY 3; 0: off).  Its scale k is a device word (icp_robust_scale).
static __host__ __device__ __forceinline__ uint32_t icp_robust (const icp_params &p) { return (p.reject & ICP_REJECT_ROBUST_MASK) >> ICP_REJECT_ROBUST_SHIFT; }
// The robust loss's IRLS weight omega (u) of u = s^2 / k^2 (include/icp_amd.h), in double, each expression in the order written; NaN: 0
static __host__ __device__ __forceinline__ double icp_robust_omega (uint32_t loss, double u)
{
    if (u != u) return 0.0;
    if (loss == 1u) return u <= 1.0 ? 1.0 : 1.0 / sqrt (u);            // Huber
    if (loss == 2u) return 1.0 / (1.0 + u);                             // Cauchy
    return u < 1.0 ? (1.0 - u) * (1.0 - u) : 0.0;                        // Tukey
}
// Trimming (icp_trim.hip; its words: ICP_AREA_TRIM below)
#define ICP_TRIM_ONE_BLOCK_MAX 16384u    // up to this many pairs per registration: the selection is one workgroup's (k_trim_select)
#define ICP_TRIM_BINS 2048u

// The plane system (icp_set_error_metric, icp_p2pl.hip): point-to-plane ICP and colored ICP (ICP_METRIC_COLORED), the point-to-plane
// system with a photometric term.  [batch][28] ICP_MEM_PLANE_SYSTEM (A's upper triangle, b, status), [batch][27][icp_p2pl_nblk] the
// block partials of k_plane_moments.
#define ICP_P2PL_BLOCK 256u      // pairs per block of the first tree level
#define ICP_P2PL_TERMS 27u       // 21 upper-triangle terms of A, then the 6 of b
#define ICP_P2PL_SYS 28u         // doubles of ICP_MEM_PLANE_SYSTEM per registration
#define ICP_METRIC_COLORED_ 2u
static __host__ __device__ __forceinline__ bool icp_p2pl (const icp_params &p) { return p.metric != 0u; }
static __host__ __device__ __forceinline__ bool icp_colored (const icp_params &p) { return p.metric == ICP_METRIC_COLORED_; }
// plane-to-plane in effect: switched on, and the metric is point-to-plane (icp_gicp.hip has the moments then)
static __host__ __device__ __forceinline__ bool icp_gicp (const icp_params &p) { return p.gicp == 1u && p.metric == 1u; }
// the symmetric objective in effect: switched on, and the metric is point-to-plane (icp_symmetric.hip has the moments then, and
// k_p2pl_finalize takes the symmetric increment)
#define ICP_MOVING_NORMALS_SYM 2u
static __host__ __device__ __forceinline__ bool icp_sym (const icp_params &p) { return p.gicp == ICP_MOVING_NORMALS_SYM && p.metric == 1u; }
static __host__ __device__ __forceinline__ uint32_t icp_p2pl_nblk (uint32_t m) { return (m + ICP_P2PL_BLOCK - 1u) / ICP_P2PL_BLOCK; }

// Registration quality (icp_evaluate, icp_quality.hip): the 21 upper-triangle terms of the information matrix, then the sum of geo, by the
// plane system's two trees over blocks of ICP_P2PL_BLOCK pairs.  Per registration the result is ICP_QUALITY_RES doubles: the 22 sums,
// then one double's room for the two counts (n_moving, n_inliers: uint32) and one of padding.
#define ICP_QUALITY_TERMS 22u
#define ICP_QUALITY_RES 24u

// The moments' allocation p.mom, offsets in doubles.  icp_params has no room for more pointers, so everything the opt-in paths keep per
// iteration lies behind the fused mode's moment partials: the passes' and the plane system's word areas, the plane system's block
// partials, and the device words kappa, k (the robust scale) and epsilon, which the setters write in stream order and the run graphs
// read instead of capturing them.
// A word area, in uint32 words: [batch][result] what the feature's ICP_MEM_* object reads (zeros while the feature is off),
// [batch][running] what an iteration's blocks keep between themselves (zero between launches), `settings` words the kernels read
// instead of capturing them, then what a feature keeps per pair.  An area starts on a double.  As they lie — result, running, settings:
//   trimming      4 (t bits, n, K, accepted), 4 + ICP_TRIM_BINS, 0: a selection's words (icp_select_words_of below, which says what
//                 the running words and the words per pair are)
//   plane system  2 ICP_P2PL_SYS (the doubles of A's upper triangle, b, status), 0, 0; behind it [batch][ICP_P2PL_TERMS][icp_p2pl_nblk]
//                 doubles, k_plane_moments' block partials, and the words kappa, k, epsilon, a double's room each
//   one-to-one    2 (n, winners), 0, 0; [batch][m] uint64 the claim table (2 batch words in front: it starts on a double)
//   pair filter   4 (n, at_boundary, incompatible, accepted), 8 (running counts, ticket), 2 (min_cos: float; grid width)
//   reciprocal    4 (n, exact, near, accepted), 0, 1 (max_gap: float; the kernel squares it in double)
//   projective    4 (n, hits, outside, empty), 8 (running counts, ticket), 6 (grid width; fx, fy, cx, cy: float bits; radius)
enum icp_area { ICP_AREA_TRIM = 0, ICP_AREA_PLANE, ICP_AREA_UNIQUE, ICP_AREA_FILTER, ICP_AREA_RECIPROCAL, ICP_AREA_PROJECTIVE, ICP_AREA_COUNT };
struct icp_area_desc { uint32_t result, running, settings; };
static __host__ __device__ inline icp_area_desc icp_area_desc_of (int a)
{
    constexpr icp_area_desc d[ICP_AREA_COUNT] = { { 4u, 4u + ICP_TRIM_BINS, 0u }, { 2u * ICP_P2PL_SYS, 0u, 0u }, { 2u, 0u, 0u },     // trimming, plane system, one-to-one
                                                  { 4u, 8u, 2u }, { 4u, 0u, 1u }, { 4u, 8u, 6u } };                                    // pair filter, reciprocal, projective
    return d[a];
}
// a selection keeps its keys where it is not one workgroup's
static __host__ __device__ inline size_t icp_select_keys (size_t B, uint32_t m) { return m > ICP_TRIM_ONE_BLOCK_MAX ? B * m : 0u; }
static __host__ __device__ inline size_t icp_area_size (icp_area_desc d, size_t B, size_t per_pair) { return B * (d.result + d.running) + d.settings + per_pair; }
static __host__ __device__ inline size_t icp_area_size (int a, size_t B, uint32_t m)    // words, with trimming's keys and the claim table
{
    return icp_area_size (icp_area_desc_of (a), B, a == ICP_AREA_TRIM ? icp_select_keys (B, m) : a == ICP_AREA_UNIQUE ? 2u * B * m : 0u);
}
struct icp_mom_layout { size_t area[ICP_AREA_COUNT], part, kappa, robust, gicp, total; };    // part: icp_p2pl_part; the three words: icp_color_kappa, icp_robust_scale, icp_gicp_eps
// (the robust kernels compute `robust` on the device: the steps up to it stand in the order the compiler has always seen them)
static __host__ __device__ inline icp_mom_layout icp_mom_layout_of (uint32_t batch, uint32_t m, uint32_t nb)
{
    const size_t B = batch, trim_words = icp_area_size (ICP_AREA_TRIM, B, m);
    icp_mom_layout l;
    l.area[ICP_AREA_TRIM] = B * 2 * 18 * nb;             // behind [batch][2][18][nb], the fused mode's moment partials
    l.area[ICP_AREA_PLANE] = l.area[ICP_AREA_TRIM] + (trim_words + 1u) / 2u;
    l.part = l.area[ICP_AREA_PLANE] + icp_area_size (ICP_AREA_PLANE, B, m) / 2u;
    l.kappa = l.part + B * ICP_P2PL_TERMS * icp_p2pl_nblk (m);
    l.robust = l.kappa + 1u;
    l.gicp = l.robust + 1u;
    size_t at = l.gicp + 1u;
    for (int a = ICP_AREA_UNIQUE; a < ICP_AREA_COUNT; ++a) { l.area[a] = at; at += (icp_area_size (a, B, m) + 1u) / 2u; }
    l.total = at;
    return l;
}
static __host__ __device__ inline icp_mom_layout icp_mom_layout_of (const icp_params &p) { return icp_mom_layout_of (p.batch, p.m, p.nb); }
// an area's three runs of words (.result + result-words * b is registration b's; behind .settings lies what the area keeps per pair)
struct icp_area_words { uint32_t *result, *running, *settings; };
static __host__ __device__ inline icp_area_words icp_words (uint32_t *w, icp_area_desc d, size_t B)
{
    return { w, w + d.result * B, w + (d.result + d.running) * B };
}
static inline icp_area_words icp_words (const icp_params &p, icp_area a)
{
    return icp_words (reinterpret_cast<uint32_t *> (p.mom + icp_mom_layout_of (p).area[a]), icp_area_desc_of (a), p.batch);
}
// A selection's words (icp_select.h), the shape of trimming's area and of median-distance rejection's words: registration b's result
// words out [4]; the running words, [batch][4] the state between the multi-workgroup passes (sel: prefix, rank left, count below,
// arrivals), then [batch][ICP_TRIM_BINS] their histograms (hist); behind the settings [batch][m] the keys, where the selection is not
// one workgroup's (icp_select_keys).  base: the area's first word.
struct icp_select_words { uint32_t *out, *sel, *hist, *keys; };
static __host__ __device__ inline icp_select_words icp_select_words_of (uint32_t *base, icp_area_desc d, uint32_t B, uint32_t b, uint32_t m)
{
    // (icp_words' three runs; the first two steps in 32 bits, as the pass kernels have always taken them: mom_layout_test.cpp pins the places)
    return { base + d.result * b, base + d.result * B + 4u * b, base + (d.result + 4u) * B + (size_t) ICP_TRIM_BINS * b,
             base + (d.result + d.running) * (size_t) B + d.settings + (size_t) b * m };
}
// Median-distance rejection (icp_median.hip): its words are an allocation of their own on the handle (icp_context::median, made at the
// first need, freed by icp_init) and reach the kernels as an argument.  They are a selection's words with the result words (t_med bits,
// n, thr bits, accepted: ICP_MEM_MEDIAN) and two settings: the factor (float bits: a new factor touches no graph) and a word of
// padding.  Their size: icp_area_size (icp_median_desc (), batch, icp_select_keys (batch, m)).
static __host__ __device__ inline icp_area_desc icp_median_desc () { return { 4u, 4u + ICP_TRIM_BINS, 2u }; }
// Adaptive trimming (icp_adaptive_trim.hip): its words are an allocation of their own on the handle likewise (icp_context::adaptive).
// Result words (j*, r_lo, r_hi, candidate bins: ICP_MEM_TRIM_ADAPTIVE); running words per registration: the arrival word and three of
// padding, then the table — [ICP_ADAPTIVE_BINS] uint64 the sums of the keys' low 19 bits, [ICP_ADAPTIVE_BINS] uint32 the counts —, zero
// between launches; four settings: min_fraction, max_fraction (float bits), the power q, a word of padding (new values touch no graph).
// Every run starts on a double.  Its size: icp_area_size (icp_adaptive_desc (), batch, 0).
#define ICP_ADAPTIVE_BINS 4096u
static __host__ __device__ inline icp_area_desc icp_adaptive_desc () { return { 4u, 4u + 3u * ICP_ADAPTIVE_BINS, 4u }; }
struct icp_adaptive_words { uint32_t *out, *arrivals; unsigned long long *sum; uint32_t *cnt; const uint32_t *settings; };
static __host__ __device__ inline icp_adaptive_words icp_adaptive_words_of (uint32_t *base, uint32_t B, uint32_t b)
{
    const icp_area_desc d = icp_adaptive_desc ();
    uint32_t *run = base + (size_t) d.result * B + (size_t) d.running * b;
    return { base + d.result * b, run, reinterpret_cast<unsigned long long *> (run + 4), run + 4u + 2u * ICP_ADAPTIVE_BINS, base + (size_t) (d.result + d.running) * B };
}
static inline double *icp_p2pl_area (const icp_params &p) { return reinterpret_cast<double *> (icp_words (p, ICP_AREA_PLANE).result); }
static inline double *icp_p2pl_part (const icp_params &p) { return p.mom + icp_mom_layout_of (p).part; }
static inline float *icp_color_kappa (const icp_params &p) { return reinterpret_cast<float *> (p.mom + icp_mom_layout_of (p).kappa); }
// (also on the device: the robust kernels find the word from their icp_params, the loss-off kernels take no argument for it)
static __host__ __device__ inline float *icp_robust_scale (const icp_params &p) { return reinterpret_cast<float *> (p.mom + icp_mom_layout_of (p).robust); }
static __host__ __device__ inline float *icp_gicp_eps (const icp_params &p) { return reinterpret_cast<float *> (p.mom + icp_mom_layout_of (p).gicp); }
// (one-to-one's claim table)
static inline unsigned long long *icp_unique_claims (const icp_params &p) { return reinterpret_cast<unsigned long long *> (icp_words (p, ICP_AREA_UNIQUE).settings); }

// The XP allocation of one RBC set, offsets in floats: [batch][m][8] the permuted database, then [batch][m] float4 NORMALS_F and
// [batch][m] float4 COLOR_GRAD_F ([gx gy gz C] per fixed point).  The normals and gradients belong to the fixed frame as the RBC does,
// so a tracked handle's second RBC set (icp_track.hip) carries its own with it.  Behind them [batch][m] float4 NORMALS_M, the moving
// frame's normals of plane-to-plane and the symmetric objective (icp_params has no room for a pointer of their own; tracking does not combine with them).
struct icp_xp_layout {
    size_t normals, color_grad, normals_m, total;
};
static __host__ __device__ __forceinline__ icp_xp_layout icp_xp_layout_of (uint32_t batch, uint32_t m)
{
    const size_t n = (size_t) batch * m;
    return { n * 8, n * 12, n * 16, n * 20 };
}
static __host__ __device__ __forceinline__ float4 *icp_normals_f (const icp_params &p)
{
    return reinterpret_cast<float4 *> (p.XP + icp_xp_layout_of (p.batch, p.m).normals);
}
static __host__ __device__ __forceinline__ float4 *icp_color_grad_f (const icp_params &p)
{
    return reinterpret_cast<float4 *> (p.XP + icp_xp_layout_of (p.batch, p.m).color_grad);
}
static __host__ __device__ __forceinline__ float4 *icp_normals_m (const icp_params &p)
{
    return reinterpret_cast<float4 *> (p.XP + icp_xp_layout_of (p.batch, p.m).normals_m);
}

#define ICP_N_FULL(p, b) ((p).N + ((size_t) (p).batch + (b)) * (p).nr)

// progress word of a checked run: bits 0..23 k (iterations whose transform has been published), bit 30 FINAL (the end kernel has
// left the state in p.hstate), bit 31 done (ICP::check said stop), bits 32..63 the run's epoch
#define ICP_MIRROR_FINAL (1ull << 30)
#define ICP_MIRROR_DONE (1ull << 31)
#define ICP_MIRROR_WORD(epoch, k, done) (((unsigned long long) (epoch) << 32) | ((done) ? ICP_MIRROR_DONE : 0ull) | (unsigned long long) ((k) & 0xFFFFFFu))

// Index of the fixed point representative r is sampled from (generalised getReps: kernels/icp_kernels.cl:107-113 with the
// grid side of the set instead of 128).
static __device__ __forceinline__ uint32_t rep_src_index (const icp_params &p, uint32_t r)
{
    uint32_t gX = r % p.nrx, gY = r / p.nrx;
    uint32_t stepX = p.side / p.nrx, stepY = p.side / p.nry;
    uint32_t xi = (stepX == 1) ? gX : gX * stepX + (stepX >> 1) - 1;
    uint32_t yi = (stepY == 1) ? gY : gY * stepY + (stepY >> 1) - 1;
    return yi * p.side + xi;
}

// The same mapping for a thread that walks many representatives (the boxes of k_reps_and_boxes): the two step divisions once, and shifts
// for r / nrx, r % nrx — the grid's width is a power of two (icp_init accepts no other: icp_capi.hip, "nr must be a power of two").
struct rep_src_map {
    uint32_t nrx, side, stepX, stepY, offX, offY, lgx;
    __device__ __forceinline__ explicit rep_src_map (const icp_params &p)
        : nrx (p.nrx), side (p.side), stepX (p.side / p.nrx), stepY (p.side / p.nry), lgx (31u - (uint32_t) __builtin_clz (p.nrx | 1u))
    {
        offX = (stepX == 1u) ? 0u : (stepX >> 1) - 1u; offY = (stepY == 1u) ? 0u : (stepY >> 1) - 1u;
    }
    __device__ __forceinline__ uint32_t operator() (uint32_t r) const
    {
        return ((r >> lgx) * stepY + offY) * side + (r & (nrx - 1u)) * stepX + offX;
    }
};


// The representative nearest by index to r that is of the OTHER kind — not at the origin when r is, at the origin when r is not —, looked up in
// the ballots k_reps_and_boxes leaves (bit l of word w: representative 64 w + l is an invalid point of its frame: at the origin); `fallback`
// where r's word and four words to either side hold none.  (ks_seed_against_invalid: a handful of lanes, a registration's first search.)
static __device__ __forceinline__ uint32_t icp_other_kind_near (const unsigned long long *MK, uint32_t nr, uint32_t r, bool r_at_origin, uint32_t fallback)
{
    const uint32_t nw = (nr + 63u) / 64u, w = r >> 6, l = r & 63u;
    auto other = [&] (uint32_t ww) -> unsigned long long {
        const uint32_t left = nr - 64u * ww;
        const unsigned long long m = MK[ww];
        return (r_at_origin ? ~m : m) & (left < 64u ? (1ull << left) - 1ull : ~0ull);
    };
    const unsigned long long o = other (w), below = o & ((1ull << l) - 1ull), above = l < 63u ? o & ~((2ull << l) - 1ull) : 0ull;
    uint32_t best_d = 0xFFFFFFFFu, best = fallback;
    if (below) { const uint32_t q = 63u - (uint32_t) __builtin_clzll (below); best_d = l - q; best = 64u * w + q; }
    if (above) { const uint32_t q = (uint32_t) __builtin_ctzll (above); if (q - l < best_d) { best_d = q - l; best = 64u * w + q; } }
    if (best_d != 0xFFFFFFFFu) return best;
    for (uint32_t d = 1; d <= 4u; ++d) {
        if (w >= d) { const unsigned long long ol = other (w - d); if (ol) return 64u * (w - d) + 63u - (uint32_t) __builtin_clzll (ol); }
        if (w + d < nw) { const unsigned long long orr = other (w + d); if (orr) return 64u * (w + d) + (uint32_t) __builtin_ctzll (orr); }
    }
    return fallback;
}

// The route of an iteration: what icp_launch_iteration enqueues for these parameters, and how the run graphs and the host-driven runs
// execute it.  icp_route_of (icp_kernels.hip) is the one place that decides it; the launchers, the run code (icp_run.hip, icp_host.h),
// icp_run_form and icp_launches_per_iteration read the record.
enum icp_apply_kind { ICP_APPLY_NONE = 0, ICP_APPLY_PLAIN, ICP_APPLY_ROBUST };    // k_trim_apply<fused?> / k_trim_apply_robust<fused?>
enum icp_tail_kind { ICP_TAIL_FUSED = 0, ICP_TAIL_FUSED_L1, ICP_TAIL_REFERENCE, ICP_TAIL_PLANE };
struct icp_route {
    bool chained;                // runs take one launch per iteration (icp_launch_chain): no pass below is on, and the tail is what the
                                 // diagnostics that time an iteration stage by stage enqueue (icp_launch_masked)
    bool stored;                 // the search stores its per-query outputs every iteration: a pass or the plane moments read them
    bool ref_search;             // the search in its reference-order form whatever p.fused (the plane metrics)
    bool projective;             // k_projective in place of the search (icp_launch_projective): the pairs by projection onto the fixed grid
    bool filter;                 // k_pair_filter
    bool reciprocal;             // k_reciprocal_state + the back search + k_reciprocal (icp_launch_reciprocal)
    bool unique;                 // k_unique_claim + k_unique_resolve
    uint32_t median;             // median-distance rejection: 0, 1 (k_median) or 4 launches (k_median_select_pass<0 .. 2>, k_median_reject)
    uint32_t select;             // trimming's selection: 0, 1 (k_trim_select, or k_adaptive_trim at any size) or 3 launches (k_trim_select_pass<0 .. 2>)
    bool adaptive;               // the selection is adaptive trimming's (icp_launch_adaptive_trim)
    icp_apply_kind apply;        // the pass that writes the search's partials again from the weights
    icp_tail_kind tail;          // k_finalize_fused / k_moment_level1 + k_finalize_fused / k_means, k_sij, k_finalize / k_plane_moments, k_p2pl_finalize
    uint32_t launches;           // what icp_launches_per_iteration reports
};
icp_route icp_route_of (const icp_params &p);

// launchers (icp_kernels.hip, icp_build.hip)
void icp_launch_build_rbc (const icp_params &p, hipStream_t s);
void icp_launch_search (const icp_params &p, hipStream_t s);
// rs: what reciprocal correspondences keep outside icp_params (icp_reciprocal_set, icp_rbc_set.h: the moving set, the reverse state, the
// back search's outputs); a route with the rule on needs it, every other ignores it
// median: the words of median-distance rejection (icp_median_desc), which live outside icp_params likewise
// adaptive: the words of adaptive trimming (icp_adaptive_desc), likewise
struct icp_reciprocal_set;
void icp_launch_iteration (const icp_params &p, hipStream_t s, const icp_reciprocal_set *rs = nullptr, uint32_t *median = nullptr, uint32_t *adaptive = nullptr);
// any subset of an iteration's stages (bit 0 the search with the passes behind it, 1 means, 2 sij, 3 finalize; 4: an empty kernel)
void icp_launch_masked (const icp_params &p, hipStream_t s, unsigned mask, const icp_reciprocal_set *rs = nullptr, uint32_t *median = nullptr, uint32_t *adaptive = nullptr);
void icp_launch_chain (const icp_params &p, hipStream_t s, uint32_t iterations, bool fresh = false);
void icp_launch_chain_one (const icp_params &p, hipStream_t s, uint32_t j, bool fresh, bool emit);   // launch j of a chain (j = 0: reads the user-visible state)
void icp_launch_chain_end (const icp_params &p, hipStream_t s, uint32_t launches);                  // after `launches` chained launches: the last moments -> p.st (and p.hstate)
void icp_launch_publish_state (const icp_params &p, hipStream_t s);                                  // separate launches: p.st -> p.hstate + the FINAL bit
bool icp_build_lists (const icp_params &p);      // buildRBC = owner search + k_place_lists (2 launches)
bool icp_dense (const icp_params &p);            // the dense search variant (several blocks per CU, stage-1 pruning)
uint32_t icp_dense_tile (const icp_params &p);   // its LDS tile: 256 or 1024 representatives
void icp_launch_owner_search (const icp_params &p, hipStream_t s);   // RBC construct, step 1 (k_search<.., OWNER>)
void icp_launch_search_dense (const icp_params &p, hipStream_t s);          // icp_search_dense.hip: the dense variants (icp_dense (p))
void icp_launch_search_rej (const icp_params &p, hipStream_t s);            // icp_search_rej.hip: every search with correspondence rejection on
void icp_launch_chain_one_rej (const icp_params &p, hipStream_t s, uint32_t j, bool fresh, bool emit);
void icp_launch_trim_select (const icp_params &p, hipStream_t s, uint32_t launches);   // icp_trim.hip: k_trim_select (1) or k_trim_select_pass<0 .. 2> (3: icp_route::select)
void icp_launch_trim_apply (const icp_params &p, hipStream_t s);             // icp_trim.hip: k_trim_apply<fused?>
void icp_launch_unique (const icp_params &p, hipStream_t s);                 // icp_unique.hip: k_unique_claim + k_unique_resolve
void icp_launch_median (const icp_params &p, hipStream_t s, uint32_t *words, uint32_t launches);   // icp_median.hip: k_median (1) or k_median_select_pass<0 .. 2> + k_median_reject (4: icp_route::median)
void icp_launch_adaptive_trim (const icp_params &p, hipStream_t s, uint32_t *words);   // icp_adaptive_trim.hip: k_adaptive_trim, in the selection's place (icp_route::adaptive)
void icp_launch_reciprocal (const icp_params &p, hipStream_t s, const icp_reciprocal_set *rs);   // icp_reciprocal.hip: k_reciprocal_state + the back search + k_reciprocal
void icp_launch_reciprocal_build (const icp_params &p, hipStream_t s, const icp_reciprocal_set &rs);   // icp_reciprocal.hip: buildRBC over M into the moving set
void icp_launch_projective (const icp_params &p, hipStream_t s);             // icp_projective.hip: k_projective, in place of the search (icp_set_projective)
void icp_launch_pair_filter (const icp_params &p, hipStream_t s);            // icp_pair_filter.hip: k_pair_filter (boundary and / or normal rejection), behind the search
void icp_launch_robust_apply (const icp_params &p, hipStream_t s);            // icp_robust.hip: k_trim_apply_robust<fused?> (a point-to-point robust loss)
void icp_launch_plane_moments_robust (const icp_params &p, hipStream_t s, double *part, uint32_t nblk);   // icp_robust.hip: k_plane_moments_robust<colored?>
void icp_launch_p2pl_solve (const icp_params &p, hipStream_t s);             // icp_p2pl.hip: k_plane_moments<colored?> + k_p2pl_finalize
void icp_launch_normals_grid (const icp_params &p, hipStream_t s);           // icp_p2pl.hip: k_normals_grid (+ colored: k_color_grad_grid; plane-to-plane, symmetric, normal rejection: + NORMALS_M), behind buildRBC
void icp_launch_normals_m (const icp_params &p, hipStream_t s, uint32_t b0, uint32_t nb);   // icp_p2pl.hip: k_normals_grid pointed at M, registrations b0 .. b0 + nb - 1
void icp_launch_gicp_moments (const icp_params &p, hipStream_t s, double *part, uint32_t nblk);          // icp_gicp.hip: k_gicp_moments<robust?>
void icp_launch_sym_moments (const icp_params &p, hipStream_t s, double *part, uint32_t nblk);           // icp_symmetric.hip: k_sym_moments<robust?>
void icp_launch_owner_search_dense (const icp_params &p, hipStream_t s);
// icp_quality.hip: k_quality_pairs + k_quality_finish over the pairs a search has left in PF / PM (its own buffers: icp_evaluate), M the
// moving sets [batch][m][8]; part [batch][ICP_QUALITY_TERMS][icp_p2pl_nblk (m)], cnt [batch][2][icp_p2pl_nblk (m)], res [batch][ICP_QUALITY_RES]
void icp_launch_quality (const float4 *PF, const float4 *PM, const float *M, uint32_t m, uint32_t batch, bool dist_on, float d2, double *part, uint32_t *cnt,
                         double *res, hipStream_t s);
// icp_pairs.hip: k_pairs_count<source> + k_pairs_scatter<source>, the correspondence set (icp_correspondences) of the pairs in PF / PM /
// nn_id — the evaluation's buffers with M (ICP_PAIRS_EVALUATED), or the last iteration's per-query outputs (ICP_PAIRS_LAST_ITERATION: the
// weight is PF.w; M, dist_on and d2 are not read).  blk_cnt [batch][icp_p2pl_nblk (m)], pairs [batch][m] records of 16 bytes, count [batch]
void icp_launch_pairs (int source, const float4 *PF, const float4 *PM, const float *M, const icp_dist_id *nn_id, uint32_t m, uint32_t batch, bool dist_on, float d2,
                       uint32_t *blk_cnt, uint4 *pairs, uint32_t *count, hipStream_t s);
uint32_t icp_tbox_of (const icp_params &p);
uint32_t icp_s2_wave_of (const icp_params &p);
void icp_search_layout_of (const icp_params &p, int *dense, int *tile, int *stage2);   // what icp_launch_search selects          // 1: the dense search scans the lists with lanes = candidates (long lists)
void icp_launch_reset_state (const icp_params &p, hipStream_t s, int reset_T);
void icp_launch_set_T (const icp_params &p, uint32_t b, const float *dT8, hipStream_t s, int reset_k = 0);
// holds the stream until *seq >= want; bounded: max_spins rounds of ~0.25 us, then *host_timeout_flag = 1 and the stream goes on
// (on a timeout also *run_flag = epoch: the launches of the run behind the gate leave without a store)
void icp_launch_gate (const uint32_t *seq, uint32_t want, uint32_t *host_timeout_flag, hipStream_t s, uint32_t max_spins = 1u << 21, icp_reg_state *warm = nullptr,
                      uint32_t *run_flag = nullptr, uint32_t epoch = 0u);
void icp_launch_seq_set (uint32_t *seq, uint32_t v, hipStream_t s);
void icp_launch_rotation_solver (int rot, int power_mode, const float *din19, float *dout18, hipStream_t s);   // [S 11 | means 8] -> [Tk 8 | Rk 9 | trips]
void icp_launch_get_lms (const float *cloud, float *lms, hipStream_t s);
void icp_launch_get_lms_band (const float *band, float *lms, hipStream_t s);
void icp_launch_transform_cloud (const float *in, float *out, const icp_reg_state *st, uint32_t n, hipStream_t s);
// kind 0 / 1: T = [q | t, s] (8 floats), 2: T = row-major 4x4 (16 floats); host pointer, passed by value
void icp_launch_transform_cloud_ex (int kind, const float *in, float *out, const float *T, uint32_t n, hipStream_t s);
