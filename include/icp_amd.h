/* icp_amd.h — C-ABI of the MI355X-native photogeometric ICP iteration engine.
 *
 * Drop-in boundary for the hot path of nlamprian/ICP: every entry point below names the
 * reference interface it replaces (paths relative to the reference checkout).  Plain C: opaque
 * handle, plain pointers and sizes, int status codes; no OpenCL, Eigen, CLUtils or torch types.
 * The C++ facade include/ICP/algorithms.hpp re-creates the reference's class templates
 * (cl_algo::ICP::ICPStep<CR,CW>, ICP<CR,CW>) on top of this file.
 *
 * Data layouts (unchanged from the reference):
 *   landmark   float[8]  = [x y z 1 r g b 1], xyz in mm, rgb in [0,1]   (src/kinect_frame_grabber.cpp:252-261)
 *   transform  float[8]  = [qx qy qz qw | tx ty tz s]                   (include/ICP/algorithms.hpp:2245-2254)
 *   dist/id    {float dist; uint32 id}                                  (kernels/icp_kernels.cl:34-38)
 *
 * Threading: a handle owns one device, one HIP stream and all its buffers; it is not
 * thread-safe, distinct handles are independent (one per GPU / host thread for batched work).
 * Errors: no exit(), no exceptions: every call returns an icp_status; icp_last_error() gives
 * the text (reference: exit(EXIT_FAILURE) from library code, src/ICP/algorithms.cpp:4411-4427).
 */
#ifndef ICP_AMD_H
#define ICP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with hidden visibility; what this header declares is what it exports. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct icp_context *icp_handle;

typedef enum {
    ICP_OK = 0,
    ICP_EINVAL = 1,        /* bad argument (reference: throw const char* -> exit)            */
    ICP_EHIP = 2,          /* HIP runtime failure (reference: cl::Error exception)           */
    ICP_ENOMEM = 3,
    ICP_ESTATE = 4,        /* call order violated (e.g. run before init / buildRBC)          */
    ICP_ENODEVICE = 5      /* no usable gfx950 device: the engine has NO CPU fallback        */
} icp_status;

/* ICPStepConfigT / ICPStepConfigW — include/ICP/algorithms.hpp:1544-1564 */
typedef enum { ICP_ROT_EIGEN = 0, ICP_ROT_POWER_METHOD = 1 } icp_rot;
typedef enum { ICP_W_REGULAR = 0, ICP_W_WEIGHTED = 1 } icp_weighting;

/* How the power method starts.  LITERAL = the reference loop from x=(1,1,1,1)
 * (kernels/icp_kernels.cl:1003-1022); SQUARED = same loop started from normalize(N^1024 * 1).
 * Default of icp_create: SQUARED (the benchmarked path). */
typedef enum { ICP_POWER_LITERAL = 0, ICP_POWER_SQUARED = 1 } icp_power_mode;

/* How the three reductions of an iteration are evaluated.  Default of icp_create: FUSED (the
 * benchmarked path: 1 launch per iteration at latency-bound sizes, 2 otherwise); REFERENCE_ORDER (4 launches per
 * iteration) is the opt-in for intermediates that restate the reference's arithmetic order.  The environment variable
 * ICP_AMD_MODE=reference, read by icp_create, starts handles in REFERENCE_ORDER + LITERAL without a code change.
 * Contract between the two: final [q | t, s] within 1e-5 relative (|q| = 1, scene scale for t, s itself).
 * REFERENCE_ORDER: sum of weights -> means -> S as three global trees in the reference's order
 * (kernels/icp_kernels.cl:213-329, 455-566, 588-743); every intermediate matches the literal oracle.
 * FUSED: one pass accumulating 18 moments in double, means and S derived from them; one global tree;
 * correspondences identical for identical T, means / S / T within 1 ulp of the coordinates. */
typedef enum { ICP_REDUCE_REFERENCE_ORDER = 0, ICP_REDUCE_FUSED = 1 } icp_reduce_mode;

/* Memory objects.  F/M/T are the reference's ICPStep::Memory D_IN_F / D_IN_M / D_IO_T
 * (include/ICP/algorithms.hpp:2241-2267); the rest are the intermediates the reference exposes
 * through the get() of its sub-objects (src/ICP/algorithms.cpp:4499-4581). */
typedef enum {
    ICP_MEM_F = 0,         /* in   m x float8   fixed landmarks                         */
    ICP_MEM_M = 1,         /* in   m x float8   moving landmarks                        */
    ICP_MEM_T = 2,         /* io   float8       cumulative [q | t, s]   (D_IO_T)        */
    ICP_MEM_TK = 3,        /* out  float8       incremental [qk | tk, sk]               */
    ICP_MEM_MEANS = 4,     /* out  2 x float4   [mean_fixed | mean_moving]              */
    ICP_MEM_S = 5,         /* out  float[11]    S (row-major, a=moving,b=fixed), Sf2, Sm2 */
    ICP_MEM_NN_ID = 6,     /* out  m x {dist,id}  query order, id = index into F        */
    ICP_MEM_W = 7,         /* out  m x float    weights 100/(100+dist)                  */
    ICP_MEM_SUM_W = 8,     /* out  double       sum of weights                          */
    ICP_MEM_REPS = 9,      /* out  nr x float8  representatives                         */
    ICP_MEM_RBC_N = 10,    /* out  nr x uint32  list sizes        (RBCConstruct D_OUT_N)   */
    ICP_MEM_RBC_O = 11,    /* out  nr x uint32  list offsets      (RBCConstruct D_OUT_O)   */
    ICP_MEM_RBC_PERM = 12, /* out  m x uint32   list position -> index into F           */
    ICP_MEM_RBC_OWNER = 13,/* out  m x uint32   owner representative of each fixed point */
    ICP_MEM_RBC_XP = 14,   /* out  m x float8   permuted database (RBCConstruct D_OUT_X_P) */
    ICP_MEM_RID = 15,      /* out  m x uint32   nearest representative of each query    */
    ICP_MEM_R = 16,        /* out  float[9]     cumulative rotation, row-major          */
    ICP_MEM_RK = 17,       /* out  float[9]     incremental rotation, row-major         */
    ICP_MEM_NN = 18,       /* out  m x float4   matched fixed xyz (+ weight in .w)      */
    ICP_MEM_QT = 19,       /* out  m x float4   transformed moving xyz (+ dist in .w)   */
    ICP_MEM_TRIM = 20,     /* out  uint32[4]    trimming, last iteration: t (float bits), n, K, accepted (0 when off) */
    ICP_MEM_NORMALS_F = 21,/* io   m x float4   normals of the fixed landmarks [nx ny nz 0] (point-to-plane) */
    ICP_MEM_PLANE_SYSTEM = 22, /* out double[28] point-to-plane: A's upper triangle (21), b (6), status (0 while off) */
    ICP_MEM_COLOR_GRAD_F = 23, /* io m x float4  colored ICP: intensity gradients of the fixed landmarks [gx gy gz C] */
    ICP_MEM_NORMALS_M = 24,    /* io m x float4  normals of the moving landmarks [nx ny nz 0], indexed like M (plane-to-plane, symmetric) */
    ICP_MEM_UNIQUE = 25,       /* out uint32[2]   one-to-one correspondences, last iteration: candidates n, winners (0 when off) */
    ICP_MEM_PAIR_FILTER = 26,  /* out uint32[4]   boundary / normal rejection, last iteration: n, at_boundary, incompatible, accepted (0 when off) */
    ICP_MEM_RECIPROCAL = 27,   /* out uint32[4]   reciprocal correspondences, last iteration: n, exact, near, accepted (0 when off) */
    ICP_MEM_REVERSE_ID = 28,   /* out m x {dist,id}  reciprocal correspondences: the back search, fixed-point order, id = index into M */
    ICP_MEM_PROJECTIVE = 29,   /* out uint32[4]   projective data association, last iteration: n, hits, outside, empty (0 when off) */
    ICP_MEM_MEDIAN = 30,       /* out uint32[4]   median-distance rejection, last iteration: t_med (float bits), n, thr (float bits), accepted (0 when off) */
    ICP_MEM_TRIM_ADAPTIVE = 31, /* out uint32[4]  adaptive trimming, last iteration: the winning bin j*, r_lo, r_hi, candidate bins (0 when off) */
    ICP_MEM_COUNT_
} icp_mem;

/* Host-visible state of one registration: the public members Rk qk tk sk R q t s k of
 * ICPStep / ICP (include/ICP/algorithms.hpp:2302-2320, 2462). */
typedef struct {
    float R[9], q[4], t[3], s;         /* cumulative, up to iteration k   */
    float Rk[9], qk[4], tk[3], sk;     /* incremental, iteration k        */
    uint32_t k;                        /* iterations executed             */
    uint32_t converged;                /* ICP::check() said stop before max_iterations */
    uint32_t power_iterations;         /* power-method loop trips of the last step */
    uint32_t reserved;
} icp_state_t;

/* ---- life cycle ------------------------------------------------------------------------- */

/* ICPStep<CR,CW>::ICPStep (env, infoRBC, infoICP) — include/ICP/algorithms.hpp:2269,
 * src/ICP/algorithms.cpp:4348-4358.  `device` replaces the CLEnv/CLEnvInfo pair.  The handle starts in the modes
 * ICP_REDUCE_FUSED + ICP_POWER_SQUARED (see above). */
int icp_create (icp_handle *h, int device, int rot, int weighted);
int icp_destroy (icp_handle h);

/* ICP<CR,CW>::init (m, nr, a, c, max_iterations, angle_threshold, translation_threshold, staging)
 * — include/ICP/algorithms.hpp:2437-2440, src/ICP/algorithms.cpp:4777-4786 and ICPStep::init
 * :4403-4582.  Rejects m == 0, nr == 0, a == 0 (reference :4413-4420), a NaN or infinite a, odd m (:1573),
 * nr not a power of two or not tiling the sqrt(m) landmark grid (:842-854).
 * `batch` >= 1 independent registrations share the launch set (SURVEY §8e "replicas only"). */
int icp_init (icp_handle h, uint32_t m, uint32_t nr, float a, float c,
              uint32_t max_iterations, double angle_threshold, double translation_threshold);
int icp_init_batched (icp_handle h, uint32_t batch, uint32_t m, uint32_t nr, float a, float c,
                      uint32_t max_iterations, double angle_threshold,
                      double translation_threshold);

/* ---- data movement ------------------------------------------------------------------------ */

/* ICPStep::write (mem, ptr, block, events, event) — include/ICP/algorithms.hpp:2273,
 * src/ICP/algorithms.cpp:4596-4622.  mem in {ICP_MEM_F, ICP_MEM_M, ICP_MEM_T}, or ICP_MEM_NORMALS_F / ICP_MEM_COLOR_GRAD_F /
 * ICP_MEM_NORMALS_M (m x float4, the point-to-plane normals, colored ICP's gradients and plane-to-plane's moving normals of ICP_NORMALS_GIVEN).  Host -> pinned staging -> device on the handle's stream; block != 0 waits for
 * completion. */
int icp_write (icp_handle h, int mem, const void *host_ptr, int block);
int icp_write_b (icp_handle h, uint32_t batch_index, int mem, const void *host_ptr, int block);

/* ICPStep::read (mem, block, events, event) — include/ICP/algorithms.hpp:2275,
 * src/ICP/algorithms.cpp:4634-4649; also the read() of the sub-objects (ICPMean :1757, ICPS :2496,
 * ICPPowerMethod :3123, ICPWeights :1198).  Copies `bytes` (<= object size) to host_dst; always blocking. */
int icp_read (icp_handle h, int mem, void *host_dst, size_t bytes);
int icp_read_b (icp_handle h, uint32_t batch_index, int mem, void *host_dst, size_t bytes);
size_t icp_mem_size (icp_handle h, int mem);

/* cl::Memory& ICPStep::get (Memory) — include/ICP/algorithms.hpp:2270,
 * src/ICP/algorithms.cpp:4366-4383: the device buffer itself, for zero-copy chaining.
 * The pointers icp_device_ptr returns are valid until the next icp_init* / icp_destroy on the handle (init frees and
 * re-creates every buffer the handle owns).
 * adopt: the caller's device buffer replaces the handle's (F/M only; call after init, again after every re-init; the
 * buffer stays the caller's — never freed by the handle — and must outlive its use by the handle). */
int icp_device_ptr (icp_handle h, int mem, void **dptr);
int icp_adopt_device_buffer (icp_handle h, int mem, void *dptr);

/* ---- the hot path ------------------------------------------------------------------------- */

/* ICPStep::buildRBC (events, event) — include/ICP/algorithms.hpp:2277,
 * src/ICP/algorithms.cpp:4655-4660 (getReps + RBCConstruct); ICP::buildRBC also resets k (:4796). */
int icp_build_rbc (icp_handle h);

/* ICPStep::run (events, event, config) — include/ICP/algorithms.hpp:2278,
 * src/ICP/algorithms.cpp:4670-4698: one iteration; on return T, Tk, R.. are updated on the
 * device (the reference blocks on a 32-byte read here; this call only enqueues). */
int icp_step (icp_handle h, int config);

/* ICP::run () — include/ICP/algorithms.hpp:2446, src/ICP/algorithms.cpp:4806-4834: iterate until
 * check() stops; blocking.  *k receives the iteration count (ICP::k) of registration 0 (a batch: icp_state_b gives every
 * registration's own k and converged flag; a registration that has converged is skipped by the launches the others still need).
 * The loop is the reference's host loop (:4806-4814) with the check on the device: every new transform's (k, converged) reaches
 * the host as one 8-byte store into pinned memory, the calling thread keeps `depth` launches queued behind the one in flight and
 * stops enqueueing when the flag shows — a run costs k launches plus at most `depth` that leave at their first load, not
 * max_iterations; the final state arrives in pinned memory with the end kernel (no stream synchronisation, no copy). */
int icp_run (icp_handle h, uint32_t *k);

/* The last finished checked run (icp_run, a tracked frame): iteration launches enqueued, its final k, and how many of the launches
 * ran past the registration's last live iteration.  Any pointer may be NULL. */
int icp_run_stats (icp_handle h, uint32_t *launches, uint32_t *k, uint32_t *dead_launches);

/* Diagnostic: the host's own kernel-launch calls inside checked runs since icp_init (or the last reset): the longest one, how many took
 * more than 10 us, how many there were.  A host-driven run is as good as the host is punctual. */
int icp_launch_stats (icp_handle h, double *max_us, uint64_t *slower_than_10us, uint64_t *total, int reset);

/* Per-query outputs of checked runs (icp_run, tracked frames: ICP_MEM_NN_ID, _W, _NN, _QT, _RID — the reference's D_OUT_NN_ID etc. of
 * the last executed iteration).  The fused kernels read none of them, and a checked run cannot know which iteration is its last:
 *   ICP_OUTPUTS_LAZY (default)     the run stores none; the first icp_read / icp_device_ptr of one re-runs the search of the last executed
 *                                  iteration with the transform it used (kept on the device): same bits, one extra launch, only when asked.
 *                                  If F, M or the RBC have changed since the run (icp_write, icp_build_rbc, the next tracked frame), the
 *                                  read fails with ICP_ESTATE instead;
 *   ICP_OUTPUTS_EVERY_ITERATION    every iteration stores them (0.4 us of every 9 at |F| = 16384); ICP_AMD_OUTPUTS=eager at icp_create.
 * Single steps, fixed-length runs and the reference-order mode always store them. */
typedef enum { ICP_OUTPUTS_LAZY = 0, ICP_OUTPUTS_EVERY_ITERATION = 1 } icp_output_mode;
int icp_set_output_mode (icp_handle h, int mode);

/* Diagnostic: host timeline of the last icp_run, microseconds after its begin — [0] 0, [1] the first launches enqueued, [2] the first
 * progress word seen, [3] decided (converged flag seen or max_iterations enqueued), [4] end kernel enqueued, [5] FINAL bit seen. */
int icp_run_timeline (icp_handle h, double *us6);

/* depth: launches kept queued behind the one in flight by checked runs (default 3; ICP_AMD_RUN_DEPTH at icp_create).
 * adaptive = 0 brings back rounds 1 - 3's form — one cached graph of max_iterations launches per checked run, converged iterations
 * leaving early — for comparisons (ICP_AMD_RUN_ADAPTIVE=0 at icp_create). */
int icp_set_run_depth (icp_handle h, uint32_t depth, int adaptive);

/* ICP::run (timer) — include/ICP/algorithms.hpp:2482-2494: exactly `iterations` steps, no
 * convergence test (the reference's profiling run; 40 there).  Enqueue only. */
int icp_run_fixed (icp_handle h, uint32_t iterations);

/* T <- identity, k <- 0: the state ICPStep::init uploads (src/ICP/algorithms.cpp:4486-4493). Enqueue only. */
int icp_reset_transform (icp_handle h);

/* icp_reset_transform + icp_run_fixed as ONE graph: a fresh registration of exactly `iterations` steps (the reference's
 * profiling run right after init, include/ICP/algorithms.hpp:2482-2494).  In the chained form the reset costs no launch
 * (the first search of the chain starts from the identity itself).  Enqueue only. */
int icp_run_fixed_fresh (icp_handle h, uint32_t iterations);

/* Blocks until everything enqueued on the handle's stream is done (queue.finish ()). */
int icp_sync (icp_handle h);

/* ---- parameters ---------------------------------------------------------------------------- */
/* getAlpha/setAlpha/getScaling/setScaling — include/ICP/algorithms.hpp:2279-2295;
 * get/setMaxIterations, AngleThreshold, TranslationThreshold — :2447-2460.
 * Alpha: every finite float but 0 is accepted (0, NaN and +-inf: ICP_EINVAL) — negative, denormal and huge ones included; the search gives
 * the serial scan's answer (strict '<' from +inf, a tie to the lowest index) for all of them, in every layout.  Its exact pruning rests on
 * d >= geo and is on for a > 0 only: with a < 0 every representative and every list member is scanned. */
int icp_get_alpha (icp_handle h, float *a);
int icp_set_alpha (icp_handle h, float a);
int icp_get_scaling (icp_handle h, float *c);
/* Absolute scale of the photogeometric metric.  The reference only states d = f_g(a) |x_g - x'_g|^2 + f_p(a) |x_p - x'_p|^2
 * (src/ICP/algorithms.cpp:4393-4398); euclideanSquaredMetric8 itself lives in the un-vendored RandomBallCover.  The engine
 * searches on geo + a pho (i.e. f_p / f_g = a: the correspondences depend only on that ratio) and reports
 * dist = f_g (geo + a pho), f_g = 1 by default.  f_g matters in WEIGHTED mode only, through w = 100 / (100 + dist)
 * (kernels/icp_kernels.cl:232): a normalised metric, e.g. f_g = 1 / (1 + a), f_p = a / (1 + a), is selected with
 * icp_set_alpha (h, a) + icp_set_metric_scale (h, 1 / (1 + a)).  Positive and finite. */
int icp_set_metric_scale (icp_handle h, float f_g);
int icp_get_metric_scale (icp_handle h, float *f_g);

/* Correspondence rejection (not reference behaviour: the reference weights every pair, w = 100 / (100 + dist) or 1).  Opt-in;
 * icp_set_rejection (h, 0, 0) — the default — changes nothing.  The search is not affected: a rejected pair keeps its
 * correspondence (NN_ID, RID, PF / PM as before) and gets the weight +0 (the W output holds 0), and its moment, mean and S terms are
 * exact zeros, written as such (a non-finite coordinate makes no NaN).  At the same T the correspondences are bit-identical to a
 * run without rejection.
 *   flags & ICP_REJECT_INVALID: reject a pair with an invalid endpoint — the moving point's untransformed x = y = z = 0 in M, or
 *     the returned fixed point's x = y = z = 0 (a Kinect pixel without depth; in the empty-list fallback the representative).
 *   max_dist > 0: reject a pair when !(geo <= max_dist^2), geo = (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2 in fp32, summed in this
 *     order without contraction (e = the transformed moving point, f = its fixed point; max_dist^2 rounded to float).  A geometric
 *     distance in the cloud's units (mm for Kinect data), not the photogeometric search metric; NaN / inf distances are rejected.
 *     0 or +inf: no distance test.
 * With rejection on, REGULAR mode uses the weighted formulas with w in {0, 1} (sum w x / sum w, not / n).  An iteration that
 * accepts no pair (sum W == 0) is the identity step: Tk = [0,0,0,1 | 0,0,0,1], T unchanged, means and S 0 — ICP::run's
 * convergence test then stops.  (Rejection off: sum W == 0 behaves as before.)
 * Applies to every registration of the handle: single, batched (icp_init_batched) and tracked (icp_track_*); it survives icp_init.
 * ICP_EINVAL: unknown flag bits, max_dist negative or NaN. */
#define ICP_REJECT_INVALID 1
int icp_set_rejection (icp_handle h, int flags, float max_dist);
int icp_get_rejection (icp_handle h, int *flags, float *max_dist);

/* Trimmed ICP (TrICP, Chetverikov et al.; not reference behaviour): in every iteration keep the closest fraction of the pairs and give
 * the rest weight 0.  The rule:
 *   - keep_fraction xi is in (0, 1].  xi = 1 is the default and means off: the same kernels, launches, graphs and bits as without it.
 *   - Candidates are the pairs that survive icp_set_rejection's rules and have a weight != 0, and whose geo is finite.  geo is the
 *     quantity the rejection rule defines: (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2 in fp32, summed in that order, with no contraction.
 *     Let n be the number of candidates.
 *   - K = (uint32_t) ceil ((double) xi * (double) n).
 *   - t is the K-th smallest geo among the candidates, counting from 1.  geo is never negative, so its float bits order the same
 *     way as uint32.
 *   - Accepted pairs are the candidates with geo <= t.  All ties at t are kept, so the accepted count can be above K.  Every other
 *     pair is trimmed.  A trimmed pair behaves exactly like a rejected one: its correspondence is kept, its weight is +0 (written to
 *     the W and NN outputs), and its moment, mean and S terms are exact zeros.  As with rejection, REGULAR mode uses the sum-W
 *     formulas with w in {0, 1}.
 *   - If n == 0, nothing is accepted: the sum W == 0 identity step (T unchanged, ICP::run stops).
 *   - Each registration of a batched handle (icp_init_batched) computes its own n, K and t.
 * Trimming is applied after icp_set_rejection's rules.  Kinect data needs ICP_REJECT_INVALID alongside it: invalid <-> invalid pairs
 * (pixels without depth in both frames) sit at geo = 0 and would be the first pairs kept.
 * ICP_MEM_TRIM holds (t bits, n, K, accepted) of the last iteration per registration; zeros while trimming is off.  With trimming on
 * the per-query outputs are stored by every iteration, and an iteration is the separate form (icp_run_form: the search, the
 * selection, the pass that applies it, the usual tail — icp_launches_per_iteration counts them).  The setting applies to single,
 * batched and tracked registrations and survives icp_init.  ICP_EINVAL: keep_fraction NaN, <= 0 or > 1. */
int icp_set_trimming (icp_handle h, float keep_fraction);
int icp_get_trimming (icp_handle h, float *keep_fraction);

/* One-to-one correspondences (PCL: CorrespondenceRejectorOneToOne; not reference behaviour): the search gives every moving point a
 * fixed point, and nothing stops many moving points from sharing one.  With the rule on, of the pairs that share a fixed point only
 * the closest keeps its weight.  The rule:
 *   - on is 0 or 1.  0 is the default and means off: the same kernels, launches, graphs and bits as without it.
 *   - Candidates are the pairs that survive icp_set_rejection's rules and have a weight != 0, and whose geo is finite.  geo is the
 *     quantity the rejection rule defines: (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2 in fp32, summed in that order, with no contraction.
 *   - For a fixed index j, take the candidates i with ICP_MEM_NN_ID[i].id == j.  The winner is the one with the smallest 64-bit key
 *     ((uint64_t) bits (geo_i) << 32) | i: the closest pair wins, a tie goes to the lowest query index.  geo is never negative, so its
 *     float bits order as the values do.
 *   - Every other candidate of j behaves exactly like a rejected pair: its correspondence is kept (NN_ID, RID and the NN / QT xyz stay
 *     as they are), its weight is +0 (written to the W and NN outputs), and its moment, mean and S terms — for a plane metric its
 *     plane-system terms — are exact zeros.  A pair that is no candidate neither claims a fixed point nor changes.  As with rejection,
 *     REGULAR mode uses the sum-W formulas with w in {0, 1}.
 *   - No winner at all: the sum W == 0 identity step (T unchanged, ICP::run stops).
 *   - Each registration of a batched handle (icp_init_batched) resolves its own claims.
 * The rule acts after icp_set_rejection's rules and before trimming and the robust loss: trimming's candidates, and its n, are the
 * pairs this rule leaves (with both on, ICP_MEM_TRIM's n equals the winner count).  The search is untouched: at the same T the ids,
 * distances and RID are bit-identical to a run with the rule off.  The winner is an integer minimum, so the result does not depend on
 * the order in which the device gets to the pairs.
 * ICP_MEM_UNIQUE holds (n, winners) of the last iteration per registration; zeros while the rule is off.  With the rule on the
 * per-query outputs are stored by every iteration, and an iteration is the separate form (icp_run_form is ICP_FORM_SEPARATE, there is
 * no chained launch).  icp_launches_per_iteration counts what the rule adds behind the search:
 *   - point-to-point: 3 launches — the claim pass, the resolve pass, and the pass that writes the search's partials again from the
 *     weights (the apply pass of trimming and of a point-to-point robust loss; with either of them on it runs anyway, and the rule
 *     adds 2);
 *   - the plane metrics (point-to-plane, colored, plane-to-plane, symmetric): 2 launches — the claim pass and the resolve pass; their
 *     moments read the weights themselves.
 * Turning the rule on or off captures the graphs anew (as icp_set_trimming does).  The setting applies to single, batched and tracked
 * registrations, to every error metric, both reduce modes and both rotation solvers, and survives icp_init.  icp_profile_run counts
 * its passes into the search stage.  ICP_EINVAL: on outside {0, 1}. */
int icp_set_unique (icp_handle h, int on);
int icp_get_unique (icp_handle h, int *on);

/* Median-distance rejection (PCL: CorrespondenceRejectorMedianDistance; libpointmatcher: MedianDistOutlierFilter; not reference
 * behaviour): a pair is rejected when it is farther apart than `factor` times the median pair distance of the same iteration.  The
 * threshold shrinks as the registration converges and scales with the level of a pyramid; its one parameter has no unit.  The rule:
 *   - factor == 0 is the default and means off: the same kernels, launches, graphs and bits as without it, for every metric.
 *     factor > 0 and finite turns the rule on; values below 1 are allowed.
 *   - Candidates are the pairs that the passes in front have left — icp_set_rejection's rules, boundary and normal rejection,
 *     reciprocal correspondences, one-to-one —, with a weight != 0 and a finite geo.  geo is the quantity the rejection rule defines:
 *     (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2 in fp32, summed in that order, with no contraction.  Let n be their number.
 *   - K = (n + 1) / 2 in integer division, and t_med is the K-th smallest geo among the candidates, counting from 1: the lower median,
 *     an element of the set — what trimming selects at keep_fraction 0.5.
 *   - thr = (float) (((double) factor * (double) factor) * (double) t_med), in the order written.  A thr that rounds to +inf accepts
 *     every candidate; t_med == 0 gives thr == 0.
 *   - Accepted are the candidates with geo <= thr, an fp32 compare (geo is never negative: the same as a compare of the bit patterns).
 *   - Every other candidate behaves exactly like a rejected pair: its correspondence is kept, its weight is +0 (written to the W and
 *     NN outputs), and its moment, mean and S terms — for a plane metric its plane-system terms — are exact zeros.  As with
 *     rejection, REGULAR mode uses the sum-W formulas with w in {0, 1}.
 *   - n == 0, or nothing accepted: the sum W == 0 identity step (T unchanged, ICP::run stops).
 *   - Each registration of a batched handle (icp_init_batched) computes its own n, t_med and thr.  A converged registration of a
 *     checked run is left alone: its words stay.
 * The rule runs behind one-to-one and in front of trimming and the robust loss: trimming's candidates, and its n, are the pairs this
 * rule accepts.  The search is untouched: at the same T the ids, distances and RID are bit-identical to a run with the rule off.  The
 * median is one number and the counts are integer sums: nothing depends on the order in which the device gets to the pairs.
 * ICP_MEM_MEDIAN holds (t_med bits, n, thr bits, accepted) of the last iteration per registration; zeros while the rule is off.  With
 * the rule on the per-query outputs are stored by every iteration, and an iteration is the separate form (icp_run_form is
 * ICP_FORM_SEPARATE, there is no chained launch).  icp_launches_per_iteration counts what the rule adds behind the search: 1 launch
 * up to 16384 pairs per registration (one workgroup selects the median, rejects and counts), 4 beyond (three selection passes and
 * the pass that rejects and counts); on point-to-point also the pass that writes the search's partials again from the weights, unless
 * another rule runs it anyway.  The plane metrics add nothing more: their moments read the weights.  icp_profile_run counts the
 * rule's passes into the search stage.
 * Turning the rule on or off captures the graphs anew; a new factor while it stays on is a parameter update that takes effect in
 * already captured graphs.  The setting survives icp_init.  It applies to single, batched and icp_batch_* registrations and the level
 * handles of a pyramid (icp_pyramid_level), to every error metric, both reduce modes, both rotation solvers, the search and
 * projective association.  Tracking is not provided: icp_track_submit / icp_track_next return ICP_ESTATE while the rule is on, as
 * with plane-to-plane.
 * ICP_EINVAL: a null handle, or a negative, NaN or infinite factor. */
int icp_set_median_rejection (icp_handle h, float factor);
int icp_get_median_rejection (icp_handle h, float *factor);

/* Adaptive trimming (Fractional ICP: Phillips, Liu & Tomasi; the automatic overlap search of Trimmed ICP: Chetverikov et al.; PCL:
 * CorrespondenceRejectorVarTrimmed; libpointmatcher: VarTrimmedDistOutlierFilter; not reference behaviour): trimming whose kept
 * fraction every iteration chooses itself, so that the overlap need not be known beforehand.  The choice minimises the fractional
 * root mean squared distance FRMSD (f) = RMSD of the closest fraction f, divided by f^lambda, over a fixed table of thresholds; the
 * power q below is 2 lambda + 1 (FRMSD^2 = mean of the closest geo / f^(2 lambda) = their sum / f^q, up to a constant).  The rule:
 *   - power == 0 is the default and means off: the fractions are ignored and read back as 0, and the same kernels, launches, graphs
 *     and bits run as without the rule.  On requires power q in 2 .. 8 and 0 < min_fraction <= max_fraction <= 1.
 *   - Fixed and adaptive trimming exclude each other: turning the rule on while icp_set_trimming's keep_fraction is < 1, and
 *     icp_set_trimming (keep_fraction < 1) while the rule is on, return ICP_ESTATE.  icp_set_trimming (1) always passes.
 *   - Candidates are exactly trimming's: the pairs that the passes in front have left — icp_set_rejection's rules, boundary and
 *     normal rejection, reciprocal correspondences, one-to-one, median-distance rejection —, with a weight != 0 and a finite geo.
 *     The key of a candidate is the bit pattern of its geo in fp32; n is the number of candidates.
 *   - Bin j of a key is key >> 19, j in 0 .. 4095: the 8 exponent bits and the top 4 mantissa bits — sixteen thresholds per octave
 *     of squared distance, at most 3.1 % apart in distance.  c_j is the number of candidates in bin j, B_j the sum of their geo in
 *     double.  B_j is exact in any order: a bin's members share an exponent, so the sum of their 24-bit significands is an integer
 *     below 2^44.
 *   - r_j = c_0 + .. + c_j.  S_j is the cumulative sum of B in double, in this fixed order: the 4096 bins are 64 runs of 64
 *     consecutive bins; within run u, s_{u,0} = B_{64u} and s_{u,i} = s_{u,i-1} + B_{64u+i}; Base_0 = 0 and Base_u = Base_{u-1} +
 *     s_{u-1,63}; S_{64u+i} = Base_u + s_{u,i}.  No contraction, no other order.
 *   - r_lo = min (ceil ((double) min_fraction * n), n), r_hi the same with max_fraction.  j_lo is the first bin with r_j >= r_lo,
 *     j_hi the first with r_j >= r_hi; both exist and are non-empty.  Candidate bins are the non-empty bins in [j_lo, j_hi].
 *   - cost_j = S_j / P_j, P_j = r_j^q in double by q - 1 successive multiplications ((r r) r ..).  The winner j* is the candidate
 *     bin with the smallest cost; among equal costs the lowest j.  Costs are non-negative doubles: the minimum over the pair (cost
 *     bits, j) as integers is one number, whatever the order in which the device gets to the bins.
 *   - t = ((j* + 1) << 19) - 1, the largest key of bin j*.  Accepted are the candidates with key <= t, exactly r_{j*} of them; ties
 *     at t are all kept.  Every other candidate behaves exactly like a trimmed pair: its correspondence is kept, its weight is +0
 *     (written to the W and NN outputs), and its moment, mean and S terms — for a plane metric its plane-system terms — are exact
 *     zeros.  REGULAR mode uses the sum-W formulas with w in {0, 1}.
 *   - n == 0: eight zero words and the sum W == 0 identity step (T unchanged, ICP::run stops).
 *   - Each registration of a batched handle (icp_init_batched) computes its own words.  A converged registration of a checked run is
 *     left alone: its words stay.
 * ICP_MEM_TRIM holds (t, n, K = r_{j*}, accepted = r_{j*}) of the last iteration per registration — the kept fraction is K / n —,
 * ICP_MEM_TRIM_ADAPTIVE (j*, r_lo, r_hi, the number of candidate bins); both read zeros while the rule is off or before an iteration.
 * The rule stands where trimming stands: behind median-distance rejection, in front of the robust loss.  The search is untouched.
 * With the rule on the per-query outputs are stored by every iteration, and an iteration is the separate form (icp_run_form is
 * ICP_FORM_SEPARATE).  icp_launches_per_iteration counts what the rule adds behind the search: one selection launch at every size,
 * and the pass that applies the weights, as for trimming.  icp_profile_run counts both into the search stage.
 * Turning the rule on or off captures the graphs anew; new fractions or a new power while it stays on are parameter updates that
 * take effect in already captured graphs.  The setting survives icp_init.  It applies to single, batched and icp_batch_*
 * registrations and the level handles of a pyramid (icp_pyramid_level), to every error metric, both reduce modes, both rotation
 * solvers, the search and projective association.  Tracking is not provided: icp_track_submit / icp_track_next return ICP_ESTATE
 * while the rule is on, as with median-distance rejection.
 * ICP_EINVAL: a null handle; a power of 1 or above 8; with a power in 2 .. 8, fractions that are NaN or not 0 < min <= max <= 1. */
int icp_set_adaptive_trimming (icp_handle h, float min_fraction, float max_fraction, uint32_t power);
int icp_get_adaptive_trimming (icp_handle h, float *min_fraction, float *max_fraction, uint32_t *power);

/* Reciprocal (forward-backward consistent) correspondences (PCL: setUseReciprocalCorrespondences,
 * CorrespondenceEstimation::determineReciprocalCorrespondences; libpointmatcher; Rusinkiewicz & Levoy's matching taxonomy; not reference
 * behaviour): a pair (m_i, f_j) is kept only if the moving point that f_j finds when it searches the moving frame is m_i itself, or
 * lies next to it.  It is the usual answer to partial overlap: icp_set_unique keeps the closest of the pairs that share a fixed point,
 * but cannot tell that f_j has a much better partner that no query happened to pick.  The rule:
 *   - on is 0 or 1.  0 is the default and means off: the same kernels, launches, graphs and bits as without the rule; the getter then
 *     gives (0, 0.f).  max_gap is finite and >= 0, in the cloud's units.
 *   - The moving set is an RBC over M, per registration, built by exactly the construction icp_build_rbc runs over F: same m, nr and
 *     alpha, the representatives picked from M by the getReps grid rule.  icp_build_rbc builds it behind the fixed set when the rule is
 *     on.  It goes stale when M is written by any route (icp_write, icp_write_b, icp_write_cloud, icp_batch_write, icp_pyramid_write,
 *     icp_adopt_device_buffer (ICP_MEM_M)), when the rule is switched on after icp_build_rbc, and by icp_init.  A stale set is rebuilt
 *     on the handle's stream by the next call that enqueues an iteration, in front of it: no ICP_ESTATE, no extra call.  A caller who
 *     changes an adopted M buffer behind the handle's back calls icp_build_rbc, as for F; after icp_set_alpha the caller rebuilds, as
 *     for F.
 *   - The inverse transform T' is computed per registration from the eight floats T = [x y z w | tx ty tz s] that this iteration's
 *     forward search used, in double, every expression in the order written, with no contraction:
 *         xx = x x, and likewise yy zz xy xz yz wx wy wz;
 *         R00 = 1 - 2 (yy + zz), R01 = 2 (xy - wz), R02 = 2 (xz + wy);
 *         R10 = 2 (xy + wz), R11 = 1 - 2 (xx + zz), R12 = 2 (yz - wx);
 *         R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = 1 - 2 (xx + yy);
 *         si = 1.0 / (double) s;  u_a = (R0a tx + R1a ty) + R2a tz;
 *         T' = [-x, -y, -z, w | (float) -(u_0 si), (float) -(u_1 si), (float) -(u_2 si), (float) si]  (the three sign flips are exact).
 *     If s is not finite or not > 0, or a component of T' is not finite, T' is the identity and every candidate of that iteration is
 *     rejected.
 *   - The back search is the engine's own search: the queries are F of the registration, transformed by T' (the arithmetic of the
 *     forward search's transform), the database is the moving set, alpha and the metric scale are the handle's.  It runs in the form
 *     icp_evaluate's search uses: reference order, REGULAR, every opt-in rule off, nothing written but per-query outputs.  Its result,
 *     in fixed-point order, is ICP_MEM_REVERSE_ID: m x {dist, id}, id an index into M.  With s != 1 the back search weighs geometry
 *     against colour differently from the forward one, by s^2: it measures geometry in the moving frame.  Reciprocity is with respect
 *     to the engine's one-shot RBC search, not an exact nearest neighbour.
 *   - Candidates are the pairs that survive icp_set_rejection's rules and the boundary and normal rules and have a weight != 0 and an
 *     ICP_MEM_NN_ID id < m.  For candidate i let j = NN_ID[i].id and i' = REVERSE_ID[j].id.
 *         exact: i' == i.
 *         near:  not exact, max_gap > 0, i' < m, and gap = (gx gx + gy gy) + gz gz in fp32 is finite and
 *                <= (float) ((double) max_gap * max_gap), with g = QT[i].xyz - QT[i'].xyz componentwise, the transformed moving points
 *                of this iteration.
 *     Every other candidate behaves exactly like a rejected pair: its correspondence is kept, its weight is +0 (written to the W and NN
 *     outputs), and its moment, mean and S terms — for a plane metric its plane-system terms — are exact zeros.  REGULAR mode uses the
 *     sum-W formulas.  Nothing accepted: the sum W == 0 identity step.
 *   - The forward search is untouched: at the same T its ids, distances and RID are bit-identical to a run with the rule off.
 * The rule acts after the boundary and normal rules and before one-to-one correspondences, trimming and the robust loss: with
 * icp_set_unique on, ICP_MEM_UNIQUE's n equals this rule's accepted count.  ICP_MEM_RECIPROCAL holds (n, exact, near, accepted) of the
 * last iteration per registration, accepted = exact + near; zeros while the rule is off.  The counts are integer sums: they do not
 * depend on the order in which the device gets to the pairs.  A converged registration of a checked run is left alone by every launch
 * the rule adds.  With the rule on the per-query outputs are stored by every iteration, and an iteration is the separate form
 * (icp_run_form is ICP_FORM_SEPARATE).  icp_launches_per_iteration counts what the rule adds behind the search:
 *   - point-to-point: 4 launches — the inverse transform, the back search, the test, and the pass that writes the search's partials
 *     again from the weights (the apply pass of trimming, one-to-one, the boundary and normal rules and a point-to-point robust loss;
 *     with any of them on it runs anyway, and the rule adds 3);
 *   - the plane metrics: 3 launches; their moments read the weights themselves.
 * Switching the rule on or off captures the run graphs anew; a new max_gap while the rule stays on is a parameter update held in a
 * device word, which captured run graphs see.  The setting applies to single, batched and icp_batch_* registrations and the level
 * handles of a pyramid, to every error metric, both reduce modes and both rotation solvers, and survives icp_init.  Tracking is not
 * provided: icp_track_submit / icp_track_next return ICP_ESTATE while the rule is on.  icp_evaluate and ICP_PAIRS_EVALUATED ignore the
 * rule; ICP_PAIRS_LAST_ITERATION shows it through W.  icp_profile_run counts its launches into the search stage.  ICP_EINVAL: on
 * outside {0, 1}, max_gap negative, NaN or infinite. */
int icp_set_reciprocal (icp_handle h, int on, float max_gap);
int icp_get_reciprocal (icp_handle h, int *on, float *max_gap);

/* Projective data association (KinectFusion; Open3D's RGB-D odometry; "projection" in Rusinkiewicz & Levoy's matching taxonomy; not
 * reference behaviour): a second way to FIND the pairs.  The fixed set is an organised grid sampled from a pinhole image; a moving point
 * is transformed, projected through the fixed camera onto that grid, and paired with what it lands on, or with the closest point of a
 * small window around it.  O (1) per query, no search structure.  Every rule behind the search (rejection, the boundary and normal
 * rules, one-to-one, trimming, the robust loss) and every tail (point-to-point, the plane metrics) stay what they are.  The rule:
 *   - on is 0 or 1.  0 is the default and means off: the same kernels, launches, graphs and bits as without the rule; the getter then
 *     gives zeros.
 *   - F is read as a row-major grid gw = grid_width wide, rows = m / gw.  m % gw == 0 is required and checked as
 *     icp_set_boundary_rejection checks its width: ICP_ESTATE from this call on an initialised handle, and from icp_build_rbc.
 *   - fx, fy, cx, cy are the pinhole model in grid units: grid column u and row v of a point (x, y, z) are fx x / z + cx and
 *     fy y / z + cy.  For icp_synth_pair* with side G they are 595 G / 640, 595 G / 480, 319.5 G / 640 and 239.5 G / 480; for the
 *     landmarks icp_write_cloud samples from a 640 x 480 frame (column 65 + 4 i, row 49 + 3 j) they are 595 / 4, 595 / 3,
 *     (319.5 - 65) / 4 and (239.5 - 49) / 3.  radius r is in [0, 8]: the window is (2 r + 1)^2 cells, clipped at the grid's edges.
 *     r = 0 is the KinectFusion pairing, meant for the plane metrics; a point-to-point registration needs r >= 1 to move along the
 *     surface.
 *   - Per query i of a registration, with T the transform this iteration's search uses:
 *       mv = M[i].xyz.  The query counts iff mv is finite and not (0, 0, 0).
 *       e = T (mv), the transformed point, with the arithmetic of the search's transform.  ICP_MEM_QT[i] = (e, d) is written for every
 *       i < m; for a miss d = +inf.
 *       In double from the float inputs, every expression in the order written, with no contraction:
 *           u = (double) fx * ((double) e.x / (double) e.z) + (double) cx,  v = (double) fy * ((double) e.y / (double) e.z) + (double) cy,
 *           pu = floor (u + 0.5), pv = floor (v + 0.5).
 *       The query is inside iff it counts, e is finite, e.z > 0, 0 <= pu <= gw - 1 and 0 <= pv <= rows - 1, compared in double (a
 *       NaN fails).
 *       The window is columns max (0, pu - r) .. min (gw - 1, pu + r), and rows likewise.  A candidate is a window cell j = y gw + x
 *       whose F[j].xyz is finite and not (0, 0, 0); d_j is the engine's metric between (e, M[i].rgb) and (F[j].xyz, F[j].rgb) with
 *       the handle's alpha (any alpha icp_set_alpha accepts: a negative one makes negative distances).
 *       The winner is the smallest d_j with d_j < +inf, compared as floats — a NaN or +inf never wins —, a tie going to the smallest
 *       j.  The result does not depend on the order in which the window is walked.
 *       Hit: d = dist_scale d_j, NN_ID[i] = {d, j}, NN[i] = (F[j].xyz, w) with w = weighted ? 100 / (100 + d) : 1, W[i] = w.
 *       icp_set_rejection's distance test applies to a hit as it does behind the search: the pair keeps its record, its weight is +0.
 *       Miss — the query does not count, is not inside, or has no winner —: NN_ID[i] = {+inf, 0xFFFFFFFF}, NN[i] = (0, 0, 0, +0),
 *       W[i] = +0.  A miss is exactly a rejected pair: every pass and every tail guards id < m and w != 0.
 *   - ICP_MEM_RID is left as it is by a projective iteration.  A later RBC search on the handle seeds its pruning from whatever it
 *     holds; pruning is exact, so that search's results do not depend on it.
 *   - ICP_MEM_PROJECTIVE holds (n, hits, outside, empty) of the last iteration per registration: n the counting queries, outside those
 *     that count and are not inside, empty those inside without a winner; hits + outside + empty == n.  Integer sums, independent of
 *     the order of arrival; zeros while the rule is off; a converged registration of a checked run keeps its last words.
 *   - As with rejection, REGULAR mode uses the sum-W formulas, and an iteration without a hit is the sum W == 0 identity step (T
 *     unchanged, ICP::run stops).
 * With the rule on the per-query outputs are stored by every iteration, and an iteration is the separate form (icp_run_form is
 * ICP_FORM_SEPARATE, there is no chained launch).  The projection kernel takes the search's place in icp_launches_per_iteration;
 * point-to-point adds 1 launch — the pass that writes the block partials from the weights (the apply pass of trimming, one-to-one, the
 * boundary and normal rules and a point-to-point robust loss; with any of them on it runs anyway, and the rule adds 0) —, the plane
 * metrics add none.  Switching the rule on or off captures the run graphs anew; a new width, new intrinsics or a new radius while the
 * rule stays on are parameter updates held in device words, which captured run graphs see.  The setting applies to single, batched and
 * icp_batch_* registrations and the level handles of a pyramid (icp_pyramid_level), to every error metric, both reduce modes and both
 * rotation solvers, and survives icp_init.  Intrinsics are per handle: level l of a pyramid takes f / 2^l, and c / 2^l for ICP_PYRAMID_PICK
 * (a level's cell is finest cell 2^l i), (c - (2^l - 1) / 2) / 2^l for ICP_PYRAMID_MEAN (centred on finest column 2^l i + (2^l - 1) / 2).  icp_build_rbc stays required and still builds the RBC: icp_evaluate, ICP_PAIRS_EVALUATED and the reciprocal rule's back
 * search use it and ignore this rule; ICP_PAIRS_LAST_ITERATION shows the rule through W.  The rule does not combine with
 * icp_set_reciprocal (runs return ICP_ESTATE while both are on).  Tracking is not provided: icp_track_submit / icp_track_next return
 * ICP_ESTATE while the rule is on.  icp_profile_run counts the kernel as the search stage.  ICP_EINVAL: on outside {0, 1}, grid_width 0
 * with on, fx or fy not finite or not > 0, cx or cy not finite, radius > 8. */
int icp_set_projective (icp_handle h, int on, uint32_t grid_width, float fx, float fy, float cx, float cy, uint32_t radius);
int icp_get_projective (icp_handle h, int *on, uint32_t *grid_width, float *fx, float *fy, float *cx, float *cy, uint32_t *radius);

/* Rejection by normal compatibility (PCL: CorrespondenceRejectorSurfaceNormal) and at the fixed grid's boundary (PCL:
 * CorrespondenceRejectorBoundaryPoints; Turk & Levoy; both in Rusinkiewicz & Levoy, "Efficient Variants of ICP"; not reference
 * behaviour).  Two independent settings, both off by default; with both off: the same kernels, launches, graphs and bits as without
 * them.  The common rule:
 *   - Candidates are the pairs that survive icp_set_rejection's rules and have a weight != 0 and an ICP_MEM_NN_ID id < m.
 *   - A candidate that a rule rejects behaves exactly like a rejected pair: its correspondence is kept (NN_ID, RID and the NN / QT xyz
 *     stay as they are), its weight is +0 (written to the W and NN outputs), and its moment, mean and S terms — for a plane metric its
 *     plane-system terms — are exact zeros.  As with rejection, REGULAR mode uses the sum-W formulas.  No pair accepted: the
 *     sum W == 0 identity step (T unchanged, ICP::run stops).
 *   - The rules act after icp_set_rejection's rules and before one-to-one correspondences, trimming and the robust loss: a rejected
 *     pair claims no fixed point (with icp_set_unique on, ICP_MEM_UNIQUE's n equals `accepted` below), and is none of trimming's n.
 *   - The boundary test comes first and a pair is counted once: ICP_MEM_PAIR_FILTER holds (n, at_boundary, incompatible, accepted) of
 *     the last iteration per registration, n = at_boundary + incompatible + accepted; zeros while both rules are off.
 *   - The search is untouched: at the same T the ids, distances and RID are bit-identical to a run with the rules off.  The counts are
 *     integer sums and nothing else is accumulated: the result does not depend on the order in which the device gets to the pairs.
 * The boundary rule, icp_set_boundary_rejection (h, grid_width) with grid_width gw > 0 (0: off):
 *   - F is read as a row-major grid gw wide, rows = m / gw.  m % gw == 0 is required and checked as icp_set_normals checks its width:
 *     ICP_ESTATE from this call on an initialised handle, and from icp_build_rbc and the icp_track_* calls that build the RBC.
 *   - A point of F is valid as in the icp_set_normals rule: xyz finite and not (0, 0, 0).
 *   - With x = id % gw, y = id / gw the fixed point id is a boundary point when x == 0, x == gw - 1, y == 0 or y == rows - 1, when the
 *     point itself is invalid, or when any of its 8 grid neighbours in F is invalid.  F is the registration's fixed set in its original
 *     order, the one id indexes.  A depth jump between valid neighbours is no boundary.
 *   - A candidate whose fixed point is a boundary point is rejected.  The mask is evaluated from F in every iteration; nothing is kept
 *     per fixed frame, so a tracked frame needs nothing more than its landmarks.
 * The normal rule, icp_set_normal_rejection (h, 1, min_cos); min_cos is the cosine of the largest accepted angle, finite, in [-1, 1]:
 *   - Per pair in double from the float inputs, every expression in the order written, with no contraction: N_Q =
 *     ICP_MEM_NORMALS_F[id], N_M = ICP_MEM_NORMALS_M[i] in query order (a non-finite normal counts as zero); R the cumulative
 *     rotation this iteration's search used, as in the plane-to-plane rule; N_P = R N_M, each component (R_a0 mx + R_a1 my) + R_a2 mz;
 *     qq = (qx qx + qy qy) + qz qz, pp likewise from N_P, o = (qx px + qy py) + qz pz.
 *   - The pair is compatible iff qq > 0 && pp > 0 && o >= (double) min_cos * sqrt (qq * pp); every other candidate is rejected.  A
 *     pair with an absent normal cannot be shown compatible; a NaN or an infinity makes the comparison false.
 *   - The setting makes the handle need the moving frame's normals under every metric, point-to-point included, and
 *     ICP_MEM_NORMALS_M follows plane-to-plane's rules: ICP_NORMALS_GIVEN: used as written; ICP_NORMALS_GRID: computed by
 *     icp_build_rbc behind the fixed normals and again by every later write of M — switching the rule on with ICP_NORMALS_GRID
 *     makes runs return ICP_ESTATE until icp_build_rbc has run again.
 *   - It combines with every metric.  Tracking is not provided (as for plane-to-plane): icp_track_submit / icp_track_next return
 *     ICP_ESTATE.
 * With a rule on the per-query outputs are stored by every iteration, and an iteration is the separate form (icp_run_form is
 * ICP_FORM_SEPARATE, there is no chained launch).  icp_launches_per_iteration counts what the rules add behind the search:
 *   - point-to-point: 2 launches — the pass, and the pass that writes the search's partials again from the weights (the apply pass of
 *     trimming, one-to-one correspondences and a point-to-point robust loss; with any of them on it runs anyway, and the rules add 1);
 *   - the plane metrics: 1 launch; their moments read the weights themselves.
 * Switching a rule on or off, or a new width, captures the graphs anew (as icp_set_trimming does); a new min_cos while the normal rule
 * stays on is a parameter update that captured run graphs see.  The settings apply to single and batched registrations, the boundary
 * rule to tracked ones too, to both reduce modes and both rotation solvers, and survive icp_init.  icp_profile_run counts the pass
 * into the search stage.  ICP_EINVAL: on outside {0, 1}, min_cos NaN or outside [-1, 1].  icp_get_normal_rejection gives (0, 0.f)
 * while the rule is off. */
int icp_set_normal_rejection (icp_handle h, int on, float min_cos);
int icp_get_normal_rejection (icp_handle h, int *on, float *min_cos);
int icp_set_boundary_rejection (icp_handle h, uint32_t grid_width);
int icp_get_boundary_rejection (icp_handle h, uint32_t *grid_width);

/* Point-to-plane ICP with a share of point-to-point (not reference behaviour; off by default).  The rule:
 *   - metric is ICP_METRIC_POINT_TO_POINT (the default: the same kernels, launches, graphs and bits as without it) or
 *     ICP_METRIC_POINT_TO_PLANE.  point_weight mu is finite and >= 0.
 *   - With point-to-plane on, each iteration minimises, linearised about the current transform (x = (omega, tau)),
 *         E = sum_i w_i [ ((P_i + omega x P_i + tau - Q_i) . N_i)^2 + mu |P_i + omega x P_i + tau - Q_i|^2 ]
 *     P = the transformed moving point the search used (ICP_MEM_QT xyz), Q = its matched fixed point (ICP_MEM_NN xyz), N = the normal
 *     of that fixed point (ICP_MEM_NORMALS_F[id], id = ICP_MEM_NN_ID.id; a non-finite normal counts as zero), w = the weight the
 *     search stores (ICP_MEM_W: 100 / (100 + dist) in WEIGHTED mode, 1 in REGULAR mode, 0 for a pair rejection or trimming removed).
 *   - Per pair, in double from the float inputs, with J = (P x N, N), r = (Q - P) . N and [P]x the cross-product matrix:
 *         A_i = J J^T + mu [[ |P|^2 I - P P^T, [P]x ], [ -[P]x, I ]]      b_i = J r + mu (P x Q, Q - P)
 *     21 upper-triangle terms (row-major) and 6, each w (J_a J_b + mu G_ab) and w (J_a r + mu g_a); every expression is evaluated in
 *     the order icp_p2pl.hip writes it down, with no contraction.  A pair with w == 0 contributes exact zeros (selected,
 *     not multiplied: a NaN coordinate makes no NaN).
 *   - The 27 sums: a halving tree x[i] += x[i + h] inside blocks of 256 consecutive pairs, then a halving tree over the block partials
 *     zero-padded to a power of two.  No atomics; the result does not depend on the launch shape.
 *   - A x = b is solved by LDL^T in double.  If a pivot d_j is not finite or d_j <= 1e-12 A_jj, the iteration is the identity step:
 *     Tk = [0,0,0,1 | 0,0,0,1], Rk = I, T unchanged, and ICP::run's convergence test stops the run.  Otherwise
 *     qk = (omega / 2, 1) normalised in double by 1 / sqrt of its squared length and rounded to float, tk = (float) tau, sk = 1,
 *     composed as every other step (R = Rk R, Rk from qk) and checked with the same convergence test.
 *   - rot, the power mode and the reduce mode do not affect a point-to-plane iteration; power_iterations is 0; ICP_MEM_MEANS, S and
 *     SUM_W are not written.  The per-query outputs are stored by every iteration, and the form is the separate one (icp_run_form).
 *   - ICP_MEM_PLANE_SYSTEM holds, per registration, A's upper triangle row-major (21), b (6) and the status (1 solved, 0 identity
 *     step) of the last point-to-plane iteration; it reads zeros while the metric is off.
 * Rejection and trimming apply as in point-to-point: their zeros are the weights.  A new mu while the metric stays on is a parameter
 * update; switching the metric captures the run graphs anew.  The setting survives icp_init and applies to single, batched and
 * tracked registrations (tracking needs ICP_NORMALS_GRID: icp_track_submit returns ICP_ESTATE with ICP_NORMALS_GIVEN).
 * ICP_EINVAL: an unknown metric, mu negative, NaN or infinite.  ICP_METRIC_COLORED (below) is point-to-plane with a photometric term. */
#define ICP_METRIC_POINT_TO_POINT 0
#define ICP_METRIC_POINT_TO_PLANE 1
#define ICP_METRIC_COLORED 2
int icp_set_error_metric (icp_handle h, int metric, float point_weight);
int icp_get_error_metric (icp_handle h, int *metric, float *point_weight);

/* Colored ICP (Park, Zhou, Koltun 2017; not reference behaviour; off by default): ICP_METRIC_COLORED is point-to-plane (the rule
 * above, every part of it: mu, weights, trees, LDL^T, identity step, composition, PLANE_SYSTEM, the separate form) plus kappa times a
 * linearised photometric residual per pair.  The rule:
 *   - kappa (icp_set_color_weight) is finite and >= 0, default 0, in mm^2 per intensity^2; it survives icp_init.  A new kappa is a
 *     parameter update (no graph is captured anew); POINT_TO_PLANE <-> COLORED changes the kernels (graphs captured anew).
 *   - Intensity: C = ((r + g) + b) / 3 in fp32, from a landmark's rgb (floats 4..6).
 *   - ICP_MEM_COLOR_GRAD_F, m x float4 [gx gy gz C] per registration, indexed like F: the intensity gradient at each fixed point in its
 *     tangent plane, and its intensity.  ICP_NORMALS_GIVEN: the user writes it (icp_write, as ICP_MEM_NORMALS_F); it starts as zeros.
 *     ICP_NORMALS_GRID with the colored metric: icp_build_rbc computes it behind the normals, for a valid centre p (finite, not the
 *     origin) with normal n != 0, from the valid points p' of its 3 x 3 grid window in row-major order (the centre excluded), in double
 *     from the float inputs:
 *         v = p' - p, vn = (vx nx + vy ny) + vz nz, u = v - vn n (componentwise: vx - vn nx, ..), dC = C(p') - C(p);
 *         from zeros, in window order: A_ab = A_ab + u_a u_b (A00 A01 A02 A11 A12 A22), b_a = b_a + u_a dC;  K = their number;
 *         then with kn = (K nx, K ny, K nz): A_ab = A_ab + kn_a kn_b  (min sum (u . g - dC)^2 + (K n . g)^2);
 *     solved by LDL^T with the 6 x 6 solve's order and pivot test, rounded to float once.  g = 0 when K < 3, the centre is invalid,
 *     n = 0 or a pivot fails; C = C(p) always.  The gradients belong to the RBC set as the normals do (tracked frames get their own).
 *     Switching a handle with ICP_NORMALS_GRID to the colored metric leaves it without gradients: icp_run and the other runs return
 *     ICP_ESTATE until icp_build_rbc has run again.
 *   - Per pair, with point-to-plane's P, Q, N, w, J, r, G, g and in double from the float inputs: (d, C_Q) = COLOR_GRAD_F[id] (a
 *     non-finite d counts as zero), C_P = the intensity of the moving landmark M[i] (query order), and
 *         dn = (dx nx + dy ny) + dz nz,  t = d - dn N (componentwise: dx - dn nx, ..)         (d in Q's tangent plane)
 *         J_C = (P x t, t) = (py tz - pz ty, pz tx - px tz, px ty - py tx, tx, ty, tz)
 *         e = P - Q,  r_C = C_P - (C_Q + ((tx ex + ty ey) + tz ez))
 *         term (a, b), a <= b:  w ((J_a J_b + mu G_ab) + kappa (J_Ca J_Cb))     term 21 + a:  w ((J_a r + mu g_a) + kappa (J_Ca r_C))
 *     so that J_C . x = r_C is the photometric match after the step, as J . x = r is the geometric one.  w == 0 selects exact zeros.
 *     kappa = 0 gives point-to-plane's values (a -0 may become +0).
 *   - Tracking needs ICP_NORMALS_GRID, as point-to-plane does; each frame's gradients come from its own buildRBC.
 * ICP_EINVAL: kappa negative, NaN or infinite. */
int icp_set_color_weight (icp_handle h, float kappa);
int icp_get_color_weight (icp_handle h, float *kappa);

/* Robust loss (an M-estimator as iteratively reweighted least squares; not reference behaviour; off by default): every pair is
 * down-weighted by the size of its own residual, for every error metric.  The rule:
 *   - loss = ICP_ROBUST_NONE (the default) is off: the same kernels, launches, graphs and bits as without it; the scale is ignored and
 *     icp_get_robust_loss returns (0, 0.f).  For any other loss the scale k is finite and > 0, in the cloud's units (mm for Kinect data).
 *   - The weight of a residual of squared size s2 is omega (u), in double: k2 = (double) k * (double) k, u = s2 / k2, and
 *         HUBER   u <= 1.0 ? 1.0 : 1.0 / sqrt (u)             (rho (s) = s^2 / 2 for s <= k, k s - k^2 / 2 beyond)
 *         CAUCHY  1.0 / (1.0 + u)                             (rho (s) = (k^2 / 2) log (1 + s^2 / k^2))
 *         TUKEY   u < 1.0 ? (1.0 - u) * (1.0 - u) : 0.0       (rho (s) = (k^2 / 6) (1 - (1 - s^2 / k^2)^3) for s <= k, k^2 / 6 beyond)
 *     omega = rho'(s) / s; omega = 0 when u is NaN (u = +inf gives 0 by each formula).  Every expression in the order written, with no
 *     contraction.
 *   - Point-to-point: s2 = (double) geo, the rejection rule's fp32 quantity.  The loss acts after rejection and trimming: every pair
 *     they leave with w != 0 gets W' = (float) ((double) w * omega (u)), and ICP_MEM_W holds W'.  A pair whose W' is 0 is exactly a
 *     rejected pair (its correspondence kept, its moment, mean and S terms exact zeros).  As with rejection, REGULAR mode uses the
 *     sum-W formulas, and an iteration with sum W == 0 is the identity step (ICP::run stops).  The per-query outputs are stored by
 *     every iteration, and an iteration is the separate form: the search, trimming's selection (when trimming is on too), the pass
 *     that applies the weights, the usual tail (icp_run_form, icp_launches_per_iteration).
 *   - Point-to-plane and colored, with the point-to-plane rule's r, d, mu and the colored rule's kappa and r_C:
 *         sG2 = r * r + mu * ((dx * dx + dy * dy) + dz * dz),  wG = omega (sG2 / k2)        (point-to-plane with its point-to-point share)
 *         sC2 = kappa * (r_C * r_C),                         wC = omega (sC2 / k2)        (colored: sqrt (kappa) r_C is in the cloud's units)
 *         term (a, b):  w * ((wG * (J_a J_b + mu G_ab)) + (kappa * wC) * (J_Ca J_Cb))
 *         term 21 + a:  w * ((wG * (J_a r + mu g_a)) + (kappa * wC) * (J_Ca r_C))
 *     point-to-plane without the photometric part: w * (wG * (J_a J_b + mu G_ab)) and w * (wG * (J_a r + mu g_a)).  wG == 0 selects an
 *     exact zero for the geometric part and wC == 0 for the photometric part (selections, not products: a non-finite residual makes
 *     no NaN); w == 0 still selects zeros for the whole pair.  ICP_MEM_W keeps the search's weight (with rejection's and trimming's
 *     zeros); the factors show only in ICP_MEM_PLANE_SYSTEM.  omega = 1 gives the loss-off system (up to the sign of a zero).
 *   - Turning the loss on or off, or changing its kind, captures the graphs anew (as icp_set_trimming does).  A new scale while the loss
 *     stays on is a parameter update: it takes effect in already captured run graphs, as kappa does.
 *   - The setting applies to single, batched (icp_init_batched), icp_batch_* and tracked (icp_track_*) registrations and survives
 *     icp_init.
 * ICP_EINVAL: an unknown loss, or a scale that is not finite and > 0 with a loss on. */
#define ICP_ROBUST_NONE 0
#define ICP_ROBUST_HUBER 1
#define ICP_ROBUST_CAUCHY 2
#define ICP_ROBUST_TUKEY 3
int icp_set_robust_loss (icp_handle h, int loss, float scale);
int icp_get_robust_loss (icp_handle h, int *loss, float *scale);

/* Generalized ICP (Segal, Haehnel, Thrun 2009: "plane-to-plane"; not reference behaviour; off by default): point-to-plane with the
 * 3-vector residual of every pair weighed by (C_Q + C_P)^-1, the sum of the two frames' local covariances.  The rule:
 *   - epsilon == 0 (the default) is off: the same kernels, launches, graphs and bits as without it, for every metric.  0 < epsilon <= 1
 *     turns it on; it takes effect while the metric is ICP_METRIC_POINT_TO_PLANE.  ICP_METRIC_POINT_TO_POINT ignores it, as it ignores
 *     mu.  With ICP_METRIC_COLORED every run, step and batched run returns ICP_ESTATE (the combination is not provided).
 *   - ICP_MEM_NORMALS_M, m x float4 [nx ny nz 0] per registration, indexed like M: the moving frame's normals, in the moving frame.  It
 *     starts as zeros.  ICP_NORMALS_GIVEN: the user writes it (icp_write, as ICP_MEM_NORMALS_F); it is used as given.
 *     ICP_NORMALS_GRID with plane-to-plane on: computed from M by exactly the grid rule of ICP_MEM_NORMALS_F (icp_set_normals), by
 *     icp_build_rbc behind the fixed normals, and again by every later icp_write / icp_write_b / icp_write_cloud / icp_batch_write of
 *     ICP_MEM_M.  Switching plane-to-plane on with ICP_NORMALS_GRID leaves the handle without moving normals: icp_run and the other runs
 *     return ICP_ESTATE until icp_build_rbc has run again (as with colored ICP's gradients).  With plane-to-plane off, nothing computes
 *     or reads the buffer.
 *   - Per pair, with point-to-plane's P, Q, w, d = Q - P, G and g, in double from the float inputs, every expression in the order
 *     written, with no contraction:
 *         N_Q = NORMALS_F[id],  N_M = NORMALS_M[i] (query order); a non-finite normal counts as zero.
 *         R = the registration's cumulative rotation before the step (ICP_MEM_R, the floats this iteration's search used);
 *         N_P = R N_M, each component (R_a0 nx + R_a1 ny) + R_a2 nz.
 *         Covariance of a normal n:  nn = (nx nx + ny ny) + nz nz.  If nn > 0 and finite: k = (1.0 - (double) epsilon) / nn and
 *         C_ab = delta_ab - k (n_a n_b) (C01 = 0.0 - k (nx ny), ..); otherwise C = I.  (R diag (epsilon, 1, 1) R^T for a unit normal; an
 *         absent normal makes that side isotropic.)
 *         S = C_Q + C_P, componentwise, upper triangle (s00 s01 s02 s11 s12 s22).
 *         c00 = s11 s22 - s12 s12, c01 = s02 s12 - s01 s22, c02 = s01 s12 - s02 s11, c11 = s00 s22 - s02 s02, c12 = s01 s02 - s00 s12,
 *         c22 = s00 s11 - s01 s01;  det = (s00 c00 + s01 c01) + s02 c02;  M_ab = c_ab / det (symmetric).  A pair whose det is not
 *         finite or not > 0 contributes exact zeros.
 *         H = [-[P]x | I], columns h0 = (0, -pz, py), h1 = (pz, 0, -px), h2 = (-py, px, 0), h3 .. h5 the unit vectors;  u_a = M h_a.
 *         term (a, b), a <= b, row-major:  w (h_a . u_b + mu G_ab)        term 21 + a:  w (u_a . d + mu g_a)
 *     The products with the structural zeros and ones of h_a are dropped, everywhere alike:
 *         u_0r = M_r1 (-pz) + M_r2 py,   u_1r = M_r0 pz + M_r2 (-px),   u_2r = M_r0 (-py) + M_r1 px,   u_(3+c)r = M_rc      (r = 0, 1, 2)
 *         h_0 . u_b = (-pz) u_b1 + py u_b2,   h_1 . u_b = pz u_b0 + (-px) u_b2,   h_2 . u_b = (-py) u_b0 + px u_b1,   h_(3+c) . u_b = u_bc
 *         u_a . d = (u_a0 dx + u_a1 dy) + u_a2 dz
 *     So each iteration minimises sum_i w_i [ e^T (C_Q + C_P)^-1 e + mu |e|^2 ], e = Q - (P + omega x P + tau).  w == 0 selects exact
 *     zeros for the pair.  epsilon = 1 makes M = I / 2 for every pair.
 *   - Robust loss: u_d = M d, each component (M_r0 dx + M_r1 dy) + M_r2 dz;  sG2 = ((u_d0 dx + u_d1 dy) + u_d2 dz) + mu ((dx dx +
 *     dy dy) + dz dz),  wG = omega (sG2 / k2);  the terms are w (wG (h_a . u_b + mu G_ab)) and w (wG (u_a . d + mu g_a)), wG == 0
 *     selecting an exact zero, as in the point-to-plane rule.
 *   - Everything behind the 27 terms is point-to-plane's: the two trees, LDL^T with its pivot test, the identity step, qk, tk, sk = 1,
 *     the composition, the convergence test, ICP_MEM_PLANE_SYSTEM, the separate form, the per-query outputs stored by every iteration.
 *     Rejection and trimming act through w.
 *   - Turning it on or off captures the run graphs anew.  A new epsilon while it stays on is a parameter update: it takes effect in
 *     already captured run graphs, as kappa does.  The setting survives icp_init and applies to single, batched (icp_init_batched) and
 *     icp_batch_* registrations.  Tracking is not provided: icp_track_submit and icp_track_next return ICP_ESTATE while it is on.
 * ICP_EINVAL: epsilon negative, NaN, infinite or above 1. */
int icp_set_plane_to_plane (icp_handle h, float epsilon);
int icp_get_plane_to_plane (icp_handle h, float *epsilon);

/* Symmetric ICP (Rusinkiewicz 2019, "A Symmetric Objective Function for ICP"; not reference behaviour; off by default): point-to-plane
 * with the residual of every pair taken along the mean of the two frames' normals and the rotation split evenly between the frames,
 *     sum_i w_i [ (P_i - Q_i) . (n_P,i + n_Q,i) ]^2,
 * which is zero whenever a pair lies on a common circular arc or quadratic patch, not only on a common plane.  The rule:
 *   - on == 0 (the default) is off: the same kernels, launches, graphs and bits as without it, for every metric.  on == 1 turns it on;
 *     it takes effect while the metric is ICP_METRIC_POINT_TO_PLANE.  ICP_METRIC_POINT_TO_POINT ignores it, as it ignores mu.  With
 *     ICP_METRIC_COLORED, or with plane-to-plane (icp_set_plane_to_plane) on at the same time under a plane metric, every step, run,
 *     fixed run and batched run returns ICP_ESTATE with a message that names both settings (the combinations are not provided).
 *   - ICP_MEM_NORMALS_M follows exactly plane-to-plane's rules.  ICP_NORMALS_GIVEN: the user writes it; it is used as written.
 *     ICP_NORMALS_GRID with the setting on: computed from M by the grid rule of ICP_MEM_NORMALS_F, by icp_build_rbc behind the fixed
 *     normals, and again by every later icp_write / icp_write_b / icp_write_cloud / icp_batch_write of ICP_MEM_M.  Switching the setting
 *     on with ICP_NORMALS_GRID (plane-to-plane off) leaves the handle without moving normals: icp_run and the other runs return
 *     ICP_ESTATE until icp_build_rbc has run again.  While both this setting and plane-to-plane are off, nothing computes or reads the
 *     buffer.
 *   - Per pair, in double from the float inputs, every expression in the order written, with no contraction; w = PF.w, P = PM.xyz,
 *     Q = PF.xyz as in the point-to-plane rule:
 *         N_Q = NORMALS_F[id],  N_M = NORMALS_M[i] (query order); a non-finite normal counts as zero.
 *         R = the registration's cumulative rotation before the step (ICP_MEM_R, the floats this iteration's search used);
 *         N_P = R N_M, each component (R_a0 mx + R_a1 my) + R_a2 mz.
 *         o = (nqx npx + nqy npy) + nqz npz.  If o < 0, N_P is negated componentwise: the two normals point the same way.
 *         n = 0.5 (N_Q + N_P), componentwise (nqx + npx) * 0.5: the mean normal, so that mu and a robust scale k keep the meaning they
 *         have under point-to-plane.  A pair with one absent normal counts a quarter; a pair with none contributes its mu share only.
 *         s = P + Q,  d = Q - P, componentwise.
 *         c = s x n = (sy nz - sz ny, sz nx - sx nz, sx ny - sy nx);  J = (c, n).
 *         r = (dx nx + dy ny) + dz nz;  ss = (sx sx + sy sy) + sz sz.
 *         G = point-to-plane's G with s in P's place: G00 = ss - sx sx, G01 = -(sx sy), G02 = -(sx sz), G11 = ss - sy sy,
 *         G12 = -(sy sz), G22 = ss - sz sz, G04 = -sz, G05 = sy, G13 = sz, G15 = -sx, G23 = -sy, G24 = sx; the unit block and the zeros
 *         as there.
 *         g = (s x d, d) = (sy dz - sz dy, sz dx - sx dz, sx dy - sy dx, dx, dy, dz).
 *         term (a, b), a <= b, row-major:  w (J_a J_b + mu G_ab)        term 21 + a:  w (J_a r + mu g_a)
 *     w == 0 selects exact zeros for the pair.
 *   - Robust loss: sG2 = r r + mu ((dx dx + dy dy) + dz dz),  wG = omega (sG2 / k2);  the terms are w (wG (J_a J_b + mu G_ab)) and
 *     w (wG (J_a r + mu g_a)), wG == 0 selecting an exact zero, as in the point-to-plane rule.
 *   - The block tree, the partial layout, the second tree, LDL^T with its pivot test, the identity step on a singular system and
 *     ICP_MEM_PLANE_SYSTEM are point-to-plane's, unchanged.  Rejection and trimming act through w.
 *   - The increment differs.  The solution x = (a, t) is Rusinkiewicz's: half the rotation is applied to each frame, the step is
 *     Rot o Trans o Rot.  In double:
 *         aa = (ax ax + ay ay) + az az;   c = 1.0 / sqrt (aa + 1.0);   qk = ((float) (ax c), (float) (ay c), (float) (az c), (float) c)
 *         u = a x t = (ay tz - az ty, az tx - ax tz, ax ty - ay tx);   at = (ax tx + ay ty) + az tz
 *         c2 = c c;   k3 = (c2 c) / (1.0 + c)
 *         tk_x = (float) ((c2 tx + c2 ux) + ax (at k3)), likewise y and z;   sk = 1
 *     So qk is the rotation by 2 theta about a with tan theta = |a|, and tk = R_a (cos theta t) with R_a the rotation by theta.  The
 *     composition and the convergence test follow as they are.
 *   - Turning it on or off captures the run graphs anew.  The setting survives icp_init and applies to single, batched
 *     (icp_init_batched) and icp_batch_* registrations.  Tracking is not provided: icp_track_submit and icp_track_next return ICP_ESTATE
 *     while it is on.
 * ICP_EINVAL: a null handle, or `on` other than 0 / 1. */
int icp_set_symmetric (icp_handle h, int on);
int icp_get_symmetric (icp_handle h, int *on);

/* Where the fixed frame's normals come from (point-to-plane):
 *   ICP_NORMALS_GIVEN (the default): the user writes ICP_MEM_NORMALS_F (m x float4 [nx ny nz 0] per registration, indexed like F);
 *     it is used as given and starts as zeros.  grid_width is ignored (pass 0).
 *   ICP_NORMALS_GRID: icp_build_rbc computes ICP_MEM_NORMALS_F from F, read as a row-major grid grid_width wide, in fp32 with no
 *     contraction.  A point is valid when its xyz is finite and not (0,0,0).  The horizontal difference is P(x+1) - P(x-1) if both
 *     neighbours are valid, else P(x+1) - P(x) if the right one is, else P(x) - P(x-1) if the left one is, else there is none; the
 *     vertical difference follows the same rule with y.  c = dh x dv, n = c / sqrtf ((c.x^2 + c.y^2) + c.z^2), flipped to -n if
 *     (n.x C.x + n.y C.y) + n.z C.z > 0 (it faces the sensor at the origin).  n = 0 when the centre C is invalid, a difference is
 *     missing, or the length is not > 0 and finite.  The normals belong to the fixed frame as the RBC does: batched and tracked
 *     runs need no extra call.
 * m % grid_width must be 0: checked here on an initialised handle, and by icp_build_rbc and icp_track_submit / icp_track_next, which
 * build the RBC (ICP_ESTATE).  The setting survives icp_init.
 * ICP_EINVAL: an unknown source, or grid_width 0 with ICP_NORMALS_GRID. */
#define ICP_NORMALS_GIVEN 0
#define ICP_NORMALS_GRID 1
int icp_set_normals (icp_handle h, int source, uint32_t grid_width);
int icp_get_normals (icp_handle h, int *source, uint32_t *grid_width);
int icp_set_scaling (icp_handle h, float c);
int icp_get_max_iterations (icp_handle h, uint32_t *n);
int icp_set_max_iterations (icp_handle h, uint32_t n);
int icp_get_angle_threshold (icp_handle h, double *deg);
int icp_set_angle_threshold (icp_handle h, double deg);
int icp_get_translation_threshold (icp_handle h, double *mm);
int icp_set_translation_threshold (icp_handle h, double mm);
int icp_set_power_mode (icp_handle h, int mode);      /* icp_power_mode */
int icp_set_reduce_mode (icp_handle h, int mode);     /* icp_reduce_mode */

/* Public state members of ICPStep/ICP (Rk qk tk sk R q t s k) — blocking. */
int icp_state (icp_handle h, icp_state_t *out);
int icp_state_b (icp_handle h, uint32_t batch_index, icp_state_t *out);

/* Registration quality (Open3D: evaluate_registration and GetInformationMatrixFromPointClouds; PCL: getFitnessScore; not reference
 * behaviour): what tells a caller whether the clouds overlap at the transform a run ended with — `converged` only says that the last
 * increment was small.  Nothing runs unless the call is made: without it every kernel, launch, graph and bit is as before.  The rule:
 *   - icp_evaluate measures registration b of a handle at its current cumulative transform: the state after the last executed
 *     iteration, the one icp_state_b reports (after icp_write (ICP_MEM_T): that transform).  Its inputs are the handle's F, M, RBC and
 *     alpha, and max_dist.
 *   - One search of M against the RBC with that state: the same kernel family, layout and bits as an iteration's search would produce
 *     at this T.  For every query i it gives e, the transformed moving point (what ICP_MEM_QT would hold), f, the returned fixed point
 *     (what ICP_MEM_NN would hold), and the id.
 *   - The handle's rejection, boundary and normal rules, one-to-one, trimming, robust loss, error metric and weighting have no
 *     influence: quality is a property of (F, M, alpha, T, max_dist).
 *   - geo_i = (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2 in fp32, summed in this order, with no contraction: the rejection rule's quantity.
 *   - A moving point counts when M[i]'s own xyz is finite and not (0, 0, 0); n_moving is the number of such points.
 *   - A pair is an inlier when its moving point counts, f is not (0, 0, 0), geo is finite and geo <= (float) ((double) max_dist *
 *     max_dist); with max_dist 0 or +inf the last test is dropped.  n_inliers is their number.  Both counts are integer sums on the
 *     device: independent of order.
 *   - 22 sums in double on the device: sum_geo = sum (double) geo_i over the inliers, and the 21 upper-triangle terms, row-major, of
 *     sum G (Q_i) over the inliers, Q = f converted to double, G the matrix of the point-to-plane rule about the point Q:
 *     [[qq I - Q Q^T, [Q]x], [-[Q]x, I]], qq = (qx qx + qy qy) + qz qz — Open3D's G^T G with the rows (0, z, -y, 1, 0, 0),
 *     (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1); rotation first, then translation, as in ICP_MEM_PLANE_SYSTEM.  A pair that is no inlier
 *     contributes exact zeros (selected, not multiplied: a NaN coordinate makes no NaN).
 *   - Both trees are the plane system's: a halving tree x[i] += x[i + h] inside blocks of 256 consecutive pairs, then a halving tree
 *     over the block partials zero-padded to a power of two.  No atomics on the doubles; the result does not depend on the launch shape.
 *   - On the host, in double: fitness = n_inliers / n_moving (0 when n_moving == 0), inlier_rmse = sqrt (sum_geo / n_inliers) (0 when
 *     there is none), information[36] the symmetric 6 x 6, row-major.  n is m.
 * The call blocks.  It first brings an open checked run to its end, as icp_read does.  One launch set — the search, the pair pass, a
 * one-block pass per registration — serves all registrations of a batched handle; out receives the records of registrations
 * 0 .. count - 1.  It disturbs nothing: the search writes into buffers of the evaluation's own (allocated at the first call), so the
 * five per-query outputs of the last iteration, lazy outputs still to be reproduced, the registration state, the partials a later
 * launch consumes and the cached graphs are as they were, and icp_step / icp_run behind it give the bits they would have given.
 * Cost: the device work is one search plus one small pass; a blocking call — three launches, the copy of the result words, the wait —
 * measured 40 us at |F| = 16384 beside a search stage of 9.0 us in the same run (icp_time_kernels).
 * ICP_EINVAL: out NULL, count 0 or above the batch, max_dist negative or NaN.  ICP_ESTATE: before icp_build_rbc, and on a handle
 * that has tracked a frame since icp_init / icp_track_reset — the quality of tracked frames is not provided.
 * icp_batch_evaluate: the record of registration i of an icp_batch_* object (one icp_evaluate on its slot). */
typedef struct {
    double fitness, inlier_rmse, sum_geo, information[36];
    uint32_t n, n_moving, n_inliers, reserved;
} icp_quality_t;
int icp_evaluate (icp_handle h, float max_dist, icp_quality_t *out, uint32_t count);

/* Correspondence set (Open3D: RegistrationResult::correspondence_set; PCL: pcl::Correspondences; not reference behaviour): WHICH pairs a
 * registration holds, as one compact list on the device.  Nothing runs unless the call is made: without it every kernel, launch, graph
 * and bit is as before.  The rule:
 *   - Set membership.  The set of registration b holds one 16-byte record per member pair: moving = the query index i into M, fixed =
 *     the id into F, geo = (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2 in fp32, summed in this order, with no contraction (the rejection
 *     rule's quantity; e = the transformed moving point, f = its fixed point), and weight, defined per source below.
 *   - Order and layout.  Records are in ascending i.  A member's position is the number of members with a lower index: integer counts
 *     per wave and per block of 256 consecutive pairs, then their prefix sums.  No atomics on positions; the result does not depend on
 *     the launch shape.  Records at positions >= count are unspecified.  Each registration of a batched handle has its own set and
 *     count; one launch set serves all of them; counts receives the counts of registrations 0 .. count - 1.
 *   - ICP_PAIRS_EVALUATED: the member pairs are exactly the inliers of icp_evaluate's rule at the same max_dist (0 or +inf: no distance
 *     test), from the same search at the current cumulative transform into the evaluation's own buffers: the handle's opt-in rules have
 *     no influence, and the count equals icp_evaluate's n_inliers for the same arguments.  fixed is that search's id, weight = 1.0f.
 *     It disturbs nothing, exactly as icp_evaluate promises: the per-query outputs, lazy outputs still to be reproduced, the state,
 *     the partials and the cached graphs are as they were.
 *   - ICP_PAIRS_LAST_ITERATION: the member pairs are the pairs the solver used in the last executed iteration: ICP_MEM_W[i] != 0.f (a
 *     float comparison: a NaN weight is a member, -0 is none).  fixed = ICP_MEM_NN_ID[i].id, geo from the ICP_MEM_NN / ICP_MEM_QT xyz,
 *     weight = ICP_MEM_W[i] (under a plane metric with a robust loss: the search's weight, as stated there).  max_dist must be 0.  The
 *     four arrays are what icp_read would deliver at the moment of the call: lazy outputs are reproduced first, and the call returns
 *     ICP_ESTATE exactly where icp_read (ICP_MEM_W) would — after a lazy run whose inputs have changed.  Rejection, the boundary and
 *     normal rules, one-to-one, trimming and a point-to-point robust loss all show through W: the count equals ICP_MEM_TRIM's
 *     accepted, ICP_MEM_UNIQUE's winners or ICP_MEM_PAIR_FILTER's accepted whenever that rule is the last one acting.
 *   - icp_correspondences blocks: it first brings an open checked run to its end, as icp_read does, and returns after the counts have
 *     reached the host.  The set stays readable until the next icp_correspondences, icp_init* or icp_destroy on the handle.
 *   - icp_correspondences_read copies the `count` records of registration batch_index and writes count to *n (n may be NULL); with
 *     capacity < count it copies nothing, writes count to *n and returns ICP_EINVAL; ICP_ESTATE when no set has been computed since
 *     icp_init.  host_dst may be NULL when count is 0.
 *   - icp_correspondences_device_ptr gives the device buffer of the registration's records (room for m of them) and its device count
 *     word, for zero-copy use (either pointer may be NULL).  The pointers are valid from the first icp_correspondences until
 *     icp_init* / icp_destroy; the buffers are allocated at that first call, each on its own, as icp_evaluate's are.  ICP_ESTATE before it.
 * Cost: the device work behind the search (EVALUATED) or behind nothing (LAST_ITERATION) is two small passes over the pairs; a blocking
 * call has icp_evaluate's shape — the same number of launches, a copy of the counts, the wait (INTEGRATION.md §5 has the figures).
 * ICP_EINVAL: an unknown source, counts NULL, count 0 or above the batch, max_dist negative or NaN (LAST_ITERATION: not 0), batch_index
 * out of range.  ICP_ESTATE: before icp_build_rbc, and on a handle that has tracked a frame since icp_init / icp_track_reset, as for
 * icp_evaluate.  icp_batch_correspondences: one icp_correspondences on registration i's slot, then the records of registration i. */
typedef struct { uint32_t moving, fixed; float geo, weight; } icp_pair_t;      /* 16 bytes */
#define ICP_PAIRS_EVALUATED      0
#define ICP_PAIRS_LAST_ITERATION 1
int icp_correspondences (icp_handle h, int source, float max_dist, uint32_t *counts, uint32_t count);
int icp_correspondences_read (icp_handle h, uint32_t batch_index, icp_pair_t *host_dst, uint32_t capacity, uint32_t *n);
int icp_correspondences_device_ptr (icp_handle h, uint32_t batch_index, void **pairs, void **count_word);

/* ---- adjacent steps -------------------------------------------------------------- */

/* ICPLMs: getLMs — kernels/icp_kernels.cl:63-76, src/ICP/algorithms.cpp:621-785.
 * cloud: 640x480 float8 on the host; which = ICP_MEM_F or ICP_MEM_M (m must be 16384). */
int icp_write_cloud (icp_handle h, int which, const void *host_cloud_640x480x8, int block);

/* ICPTransform<QUATERNION> on an arbitrary cloud with the handle's current T —
 * src/ocl_icp_reg.cpp:175 (full-cloud transform after run()).  Host in, host out; n points. */
int icp_transform_cloud (icp_handle h, const void *host_in, void *host_out, uint32_t n);

/* Frame-to-frame tracking — README.md:4 ("real-time frame-to-frame registration"); per pair the demo's flow
 * src/ocl_icp_reg.cpp:128-172 (init: getLMs of both clouds; registerPC: buildRBC + run).  Frames of a sequence are fed one by
 * one (640x480 float8 each); frame f is registered against frame f - 1, whose landmarks are already resident: they become the
 * fixed set by a rotation of three landmark buffers (no copy, no host trip).  Only the band of a frame that getLMs reads
 * (128 rows x 509 pixels = 2.08 MB of the 9.83 MB) is uploaded; the landmarks are extracted on the device (kernels/icp_kernels.cl:63-76).
 *
 * icp_track_submit   upload + getLMs on a copy stream, then buildRBC + ICP::run; up to four frames may be in flight, so frame f + 1 is
 *                    uploaded while frame f registers.  The registration is a host-driven checked run (icp_run) that gets as many
 *                    iterations up front as the last two registrations suggest it needs (the smaller k, + 1); later icp_track_* calls
 *                    top it up.  No launch is spent on iterations past the convergence of a frame beyond that prediction / the run depth.
 *                    Consecutive registrations alternate between two streams (icp_track_form: gated): this frame's RBC construction
 *                    (into its own set of RBC buffers) and its launches are enqueued at once, behind a one-wave gate kernel that holds
 *                    its stream until the previous registration has released the sequence word — the device goes from one frame to
 *                    the next without the host.  (Host-ordered form: the call first brings the previous frame's run to its end.)
 *                    No deadline for the caller, and (round 6) no waiting for the device either: in the gated form the call returns
 *                    once this frame's own launches are out, and a thread of the engine (the keeper, one per tracking handle,
 *                    started with the first gated frame) looks after the open runs while the application is outside the library:
 *                    it polls their progress words, keeps their queues topped up, enqueues their end kernels.  Every entry point
 *                    pauses the keeper on its way in and hands the runs back on its way out — the two never touch the handle at the
 *                    same time.  So what a frame's gate waits for never depends on a later call, and neither does the frame submitted
 *                    last: a caller that stays away for a second or an hour finds its results waiting.  An error the keeper runs into
 *                    (below) is reported by the next icp_track_* call.  ICP_AMD_TRACK_KEEPER=0: no thread — the call itself brings
 *                    the previous frame's registration to its decision before it returns (round 5's rule), later calls top up the rest.
 *                    (The gate's own bound — ~0.5 s, more for large max_iterations — is a guard against a device that has stopped:
 *                    the frames behind it are then skipped without a store, the next call returns ICP_EHIP, icp_track_reset recovers.)
 *                    warm_start != 0: the registration starts from the previous hop's transform (written back as by
 *                    icp_write (ICP_MEM_T): the rotation state is re-derived from it) instead of the identity; the first
 *                    registration of a sequence (after icp_init / icp_track_reset) has no previous hop and starts from the
 *                    identity.
 *                    `cloud` may be pageable host memory (the band is copied into pinned staging by the calling thread) or one
 *                    of the engine's two pinned frame buffers (icp_track_staging: the band goes by DMA straight from there —
 *                    the reference's mapped staging buffers hPtrInF / hPtrInM, src/ICP/algorithms.cpp:4438-4475;
 *                    icp_track_staging returns a buffer only after the band of the frame it last held has left it — whichever
 *                    of the two buffers a frame came from, in any order, mixed with pageable frames).
 * icp_track_collect  blocks until the oldest frame in flight is done: *registered = 0 for the first frame after icp_init /
 *                    icp_track_reset (nothing to register against; *k = 0, T8 = identity), else 1, *k = iterations executed and
 *                    T8 = [q | t, s] mapping that frame onto the previous one.  Any output pointer may be NULL.
 * icp_track_next     submit + collect (blocking): afterwards T (icp_read, icp_state) maps the new frame onto the previous one.
 * m must be 16384 (getLMs), batch 1, and the handle's own F / M buffers (not adopted ones). */
int icp_track_next (icp_handle h, const void *host_cloud_640x480x8, int warm_start, uint32_t *k, int *registered);
int icp_track_submit (icp_handle h, const void *host_cloud_640x480x8, int warm_start);
int icp_track_collect (icp_handle h, uint32_t *k, float *T8, int *registered);
int icp_track_staging (icp_handle h, uint32_t slot /* 0 | 1 */, void **pinned_host_frame);
/* The caller's own frame buffers as DMA sources: page-locks `bytes` (>= one frame) at `frames` (hipHostRegister, once: a capture loop
 * reuses its buffers); a frame submitted from inside a registered range is uploaded like one from the engine's pinned frame buffers —
 * the band by one 2-D DMA, no copy by the calling thread (60 us of a frame's host time).  A frame must stay as it is until it has been
 * collected (icp_track_collect) — the engine cannot tell when the caller refills its own memory.  icp_track_unregister_source (the
 * range's start) before the memory is freed; icp_init / icp_destroy unregister what is left. */
int icp_track_register_source (icp_handle h, void *frames, size_t bytes);
int icp_track_unregister_source (icp_handle h, void *frames);
int icp_track_reset (icp_handle h);
/* How tracked frames follow each other on the device: *gated = 1 — consecutive registrations alternate between two streams, each held by a
 * device-side gate (a one-wave kernel, bounded wait) until its predecessor has released the sequence word: a frame's RBC construction and
 * its predicted launches are enqueued while the previous frame is still running, and the host is not on the path between two frames;
 * 0 — one stream, a frame's work enqueued when the host has seen the previous one decided (ICP_AMD_TRACK_GATE=0, checked runs as graphs, or
 * a runtime that serves the two streams from one hardware queue: probed once per handle).  Same results either way. */
int icp_track_form (icp_handle h, int *gated);

/* ---- RGB-D front end: depth and colour images to landmarks on the device --------------------------------------------------------
 * A sensor delivers a 16-bit depth image and an 8-bit colour image, not a float8 cloud; the reference makes the cloud in its grabber
 * (src/kinect_frame_grabber.cpp:246-262) and can first pass the images through an edge-preserving filter (:179-243).  Here the
 * device filters the depth (optionally), back-projects it with the caller's intrinsics, picks the landmarks on a configurable lattice
 * and can compute normals from the full-resolution filtered vertex map.  With no RGB-D call made, none of this code runs.
 *
 * A fresh handle, and cfg == NULL, hold: width, height = 640, 480; fx, fy = 595, 595; cx, cy = 319.5, 239.5; depth_scale = 1;
 * d_min, d_max = 1, 65535; x0, y0 = 65, 49; step_x, step_y = 4, 3; radius = 0, range = 30 — the reference's unfiltered writer followed
 * by getLMs (icp_write_cloud).
 *
 * Depth at pixel p = (u, v) with count c0.  If c0 is invalid, z = 0: holes are not filled.  Otherwise the neighbours q = p + (dx, dy)
 * count when |dx|, |dy| <= r, q lies inside the image and its count c_q is valid:
 *   w_s = max (0, (r + 1)^2 - dx^2 - dy^2),   w_r = max (0, S^2 - (c_q - c0)^2),
 *   N = sum w_s w_r c_q  and  D = sum w_s w_r,  both as exact integers,
 *   z = (float) ((double) N / (double) D) * depth_scale:  one correctly rounded double division, one rounding to float, one float
 *   multiplication.
 * Both kernels are Epanechnikov kernels in place of KinectFusion's two Gaussians; a pixel across a depth step of S or more counts has
 * weight 0; the result contains no transcendental function and does not depend on summation order.  D > 0 always (the centre weighs
 * (r + 1)^2 S^2); N < 2^53 at r <= 6 and S <= 4095 (sum w_s = 3765 at r = 6, and 3765 * 4095^2 * 65535 = 4.14e15), so the conversion
 * to double is exact; any exact integer evaluation is allowed.  With r = 0, z = (float) c0 * depth_scale.
 *
 * Point:  X = ((float) u - cx) * z / fx,  Y = ((float) v - cy) * z / fy,  Z = z,  lane 3 = 1;  the colour lanes are (float) channel /
 * 255.f, or 0 if no colour image is given;  lane 7 = 1.  Each operation is rounded on its own.  An invalid pixel gets the same formulas
 * from z = 0: xyz = +-0 is the engine's invalid point with its colour kept, exactly as the reference's writer produces it.
 *
 * Normals (optional): ICP_NORMALS_GRID's rule (icp_set_normals) applied to the whole width x height vertex map as a `width`-wide grid —
 * one-pixel neighbours, central differences where both neighbours are valid, one-sided ones otherwise, oriented toward the camera, zero
 * where the rule has no answer.
 *
 * Landmarks: side = sqrt (m); landmark j * side + i is pixel (x0 + step_x i, y0 + step_y j), its normal that pixel's normal.  The
 * lattice must lie inside the image. */
typedef struct {
    uint32_t width, height;                 /* image size, 1 .. 4096 each; both images row-major, colour interleaved R G B */
    float    fx, fy, cx, cy;                /* pinhole model: fx, fy finite and > 0, cx, cy finite */
    float    depth_scale;                   /* engine units per depth count, finite and > 0 (1: the reference's millimetres) */
    uint32_t d_min, d_max;                  /* a count c is valid iff c != 0 and d_min <= c <= d_max <= 65535 */
    uint32_t x0, y0, step_x, step_y;        /* landmark (i, j) = pixel (x0 + step_x i, y0 + step_y j); steps >= 1 */
    uint32_t radius;                        /* filter radius r, 0 .. 6; 0: no filter */
    uint32_t range;                         /* range cut-off S in counts, 1 .. 4095 (unused when r = 0) */
} icp_rgbd_t;
/* The handle's configuration (it survives icp_init as the other settings do).  ICP_EINVAL for every value outside the ranges above, and,
 * on an initialised handle, for a lattice that does not fit sqrt (m) landmarks into the image; ICP_ESTATE while tracked frames are in
 * flight.  A refused call leaves the configuration as it was. */
int icp_set_rgbd (icp_handle h, const icp_rgbd_t *cfg);
int icp_get_rgbd (icp_handle h, icp_rgbd_t *cfg);
/* The landmarks of an image pair into F or M (which = ICP_MEM_F or ICP_MEM_M), as icp_write of the same values would: the lattice form
 * of the front end reads only the rows of the lattice's bounding box grown by r (+ 1 with normals).  The input-change bookkeeping, the
 * lazy outputs and the restriction to registration 0 are icp_write_cloud's.  normals != 0: also ICP_MEM_NORMALS_F / ICP_MEM_NORMALS_M, as
 * icp_write of that object would (for a registration with ICP_NORMALS_GIVEN; with ICP_NORMALS_GRID buildRBC replaces them).  rgb may be
 * NULL.  ICP_EINVAL if m is not a square number or the lattice does not fit sqrt (m) landmarks into the image.  Blocking (the images may
 * be pageable host memory). */
int icp_write_rgbd (icp_handle h, int which, const uint16_t *depth, const uint8_t *rgb, int normals, int block);
/* Tracking from images: icp_track_submit / icp_track_next with an image pair in place of the float8 frame; icp_track_collect collects both
 * kinds, which may alternate within one sequence.  The calling thread copies the depth rows of the lattice's bounding box (grown by r) and
 * the colour rows of the lattice into pinned staging — at the defaults 0.58 MB of the images' 1.54 MB, beside the 2.08 MB of a float8
 * frame's band —, one upload on the copy stream follows, and the lattice form runs there in getLMs' place.  m must be 16384: any image
 * size and lattice that give 128 x 128 landmarks are accepted (ICP_EINVAL otherwise).  Tracked frames get no front-end normals:
 * point-to-plane tracking keeps ICP_NORMALS_GRID.  icp_track_register_source stays what it is: zero-copy submission of RGB-D frames is
 * out of scope.  rgb may be NULL. */
int icp_track_submit_rgbd (icp_handle h, const uint16_t *depth, const uint8_t *rgb, int warm_start);
int icp_track_next_rgbd (icp_handle h, const uint16_t *depth, const uint8_t *rgb, int warm_start, uint32_t *k, int *registered);
/* The dense form as a one-call operation beside the other icp_kernel_* entries (host in, host out, blocking, no icp_init; errors through
 * icp_kernel_last_error): every pixel of the image, the lattice fields of cfg ignored.  cfg == NULL: the defaults.  cloud_out: width x
 * height x 8 floats; normals_out: width x height x 4 floats, or NULL; rgb may be NULL. */
int icp_kernel_rgbd (int device, const icp_rgbd_t *cfg, const uint16_t *depth, const uint8_t *rgb, void *cloud_out, float *normals_out);
/* Diagnostic (tools/diag/rgbd_time.py): one form of the front end alone with the handle's configuration — dense != 0: every pixel, else the
 * sqrt (m) x sqrt (m) landmarks —, whole images uploaded once, `reps` launches between two events on the handle's stream, the results into
 * scratch (F, M and the normals stay as they are).  Microseconds per launch. */
int icp_time_rgbd (icp_handle h, int dense, int normals, const uint16_t *depth, const uint8_t *rgb, uint32_t reps, float *us_per_launch);

/* ---- Frame-to-model: a TSDF volume fused and ray-cast on the device -----------------------------------------------------------------
 * Registered frames are fused into a truncated signed distance volume (KinectFusion, Newcombe et al. 2011; Curless & Levoy 1996); the
 * next frame is registered against a view of that volume ray-cast from the last pose: an organised grid sampled from a pinhole image, with
 * normals, as projective association and the plane metrics want their fixed set.  A volume is a handle of its own with a stream of its
 * own; it touches nothing an iteration reads or writes, and with no icp_tsdf_* call made, none of this code runs.  The reference has no
 * model.  Arithmetic: fp32, each operation rounded on its own, IEEE divide and sqrt, dots as (a0 b0 + a1 b1) + a2 b2;
 * tests/tsdf_ref.py restates every value bit for bit.
 *
 * Volume.  Voxel (i, j, k), i < nx, j < ny, k < nz, has the centre origin + voxel * (i, j, k) and the state (D, W) and, with `colour`,
 * C[3]; all 0 after create and reset.  icp_tsdf_read / icp_tsdf_write exchange the logical layout, x fastest:
 * dw[((k ny + j) nx + i) 2 + {0, 1}] = D, W and rgb[((k ny + j) nx + i) 3 + ch].
 *
 * Pose.  pose12: 12 floats, row-major [R | t], camera -> world: x_w = R x_c + t, R_ab = pose12[4 a + b], t_a = pose12[4 a + 3]; checked
 * for finiteness only.  Camera.  An icp_rgbd_t gives the image size, the intrinsics, depth_scale, d_min / d_max and the lattice; radius
 * and range are ignored: the raw counts are fused, as KinectFusion does.
 *
 * Integrate, per voxel:
 *    p_a = origin_a + (float) idx_a * voxel;   d = p - t;   q_a = (R_0a d_0 + R_1a d_1) + R_2a d_2;       unchanged unless q_z > 0
 *    u = (fx * (q_x / q_z) + cx) + 0.5f, v likewise;   unchanged unless 0 <= u < width and 0 <= v < height (float comparisons, made before
 *    any conversion: NaN fails); the pixel is (floor u, floor v);   unchanged unless its count c is valid by the front end's rule
 *    z = (float) c * depth_scale;   s = z - q_z;   unchanged unless s >= -mu;   e = min (1.f, s / mu)
 *    D' = (D * W + e) / (W + 1.f);   with `colour` and a colour image C'_ch = (C_ch * W + (float) ch / 255.f) / (W + 1.f), else C stays;
 *    W' = min (W + 1.f, w_max)
 *
 * Ray cast, per output pixel (u, v):  a_x = ((float) u - cx) / fx, a_y likewise;  delta = 0.5f * mu;  N = floorf ((z_far - z_near) / delta);
 * lambda_n = z_near + (float) n * delta for n = 0 .. N (no running sum); the sample point is x_c = (a_x lambda, a_y lambda, lambda),
 * w_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a.
 *    The sample S (w):  g_a = (w_a - origin_a) / voxel, i_a = floorf (g_a);  it is KNOWN iff 0 <= i_a <= n_a - 2 on every axis (float
 *    comparisons) and all eight corners of the cell have W > 0;  f_a = g_a - i_a;  lerp (a, b, t) = a + t * (b - a) along x, then y, then z.
 *    n* = the first n whose sample is known and <= 0.  The pixel is a HIT iff n* exists, n* >= 1, sample n* - 1 is known and S_{n*-1} > 0;
 *    then lambda* = lambda_{n*-1} + delta * (S_{n*-1} / (S_{n*-1} - S_{n*})), and the vertex is the front end's back-projection of the depth
 *    lambda*:  X = ((float) u - cx) * lambda* / fx, Y likewise, Z = lambda*.  Its world point h comes from the formula above, and the hit
 *    stands only if S (h) is known (the hit's own cell).  The colour is the same trilinear form of C in that cell (0 without `colour`).
 *    Normal:  G_a = S (h + voxel e_a) - S (h - voxel e_a); all six samples known and len = sqrt ((G_0^2 + G_1^2) + G_2^2) > 0, otherwise the
 *    normal is 0;  n_w = G / len;  n_c,a = (R_0a n_0 + R_1a n_1) + R_2a n_2, negated if (n_c . vertex) > 0: toward the camera, as
 *    ICP_NORMALS_GRID orients its normals.
 *    A hit gives the point [X Y Z 1 r g b 1] and the normal [n_c 0]; every other pixel the engine's invalid point [0 0 0 1 0 0 0 1] and a
 *    zero normal.
 * Any shortcut that leaves every bit as the rule gives it is allowed. */
typedef struct icp_tsdf_context *icp_tsdf_handle;
typedef struct {
    uint32_t nx, ny, nz;                    /* voxels per axis, 2 .. 1024 each */
    float    voxel;                         /* edge of a voxel in engine units, finite and > 0 */
    float    origin[3];                     /* centre of voxel (0, 0, 0), finite */
    float    mu;                            /* truncation distance, finite and > 0 */
    float    w_max;                         /* weight cap, integer-valued, 1 .. 65536 */
    uint32_t colour;                        /* 0 or 1: the volume keeps C */
} icp_tsdf_t;
/* Life cycle.  ICP_EINVAL for every field outside its range, ICP_ENOMEM if the device cannot hold the volume (8 bytes a voxel, 24 with
 * colour; the first icp_tsdf_shift allocates a second buffer of the same size and keeps it until destroy: 16 bytes a voxel from then on,
 * 48 with colour).  icp_tsdf_reset clears the voxels and keeps the window where icp_tsdf_shift has moved it: the origin and the cumulative
 * shift stay (for a volume that was never shifted, the state after create).  icp_tsdf_get_config returns the window's current origin.
 * icp_tsdf_last_error (NULL): why the last icp_tsdf_create of this thread failed.  A refused call of any entry below leaves the
 * volume (and the handle of icp_tsdf_raycast_to) as it was.  All calls are blocking. */
int icp_tsdf_create (icp_tsdf_handle *out, int device, const icp_tsdf_t *cfg);
int icp_tsdf_destroy (icp_tsdf_handle t);
int icp_tsdf_reset (icp_tsdf_handle t);
int icp_tsdf_get_config (icp_tsdf_handle t, icp_tsdf_t *cfg);
const char *icp_tsdf_last_error (icp_tsdf_handle t);
/* One frame into the volume: depth is cam->width x cam->height counts, rgb the interleaved colour image or NULL (host pointers). */
int icp_tsdf_integrate (icp_tsdf_handle t, const icp_rgbd_t *cam, const float *pose12, const uint16_t *depth, const uint8_t *rgb);
/* The view from pose12, host pointers out.  side == 0: every pixel, cloud_out width x height x 8 floats, normals_out width x height x 4
 * floats or NULL; otherwise the side x side landmarks of cam's lattice, landmark j side + i = pixel (x0 + step_x i, y0 + step_y j)
 * (ICP_EINVAL if the lattice leaves the image).  ICP_EINVAL unless 0 < z_near < z_far are finite and N <= 4095. */
int icp_tsdf_raycast (icp_tsdf_handle t, const icp_rgbd_t *cam, const float *pose12, float z_near, float z_far, uint32_t side, void *cloud_out, float *normals_out);
/* The sqrt (m) x sqrt (m) landmarks of the view, device to device, into F or M of handle h (which = ICP_MEM_F or ICP_MEM_M) and, with
 * normals != 0, into ICP_MEM_NORMALS_F / ICP_MEM_NORMALS_M: as icp_write of the same values would leave them, with icp_write_rgbd's
 * bookkeeping.  cam == NULL: the handle's configuration (icp_set_rgbd).  Registration 0 only.  ICP_EINVAL for a handle on another device,
 * a non-square m or a lattice that does not fit; ICP_ESTATE while tracked frames are in flight.  An error is left in the volume's
 * icp_tsdf_last_error. */
int icp_tsdf_raycast_to (icp_tsdf_handle t, icp_handle h, int which, const icp_rgbd_t *cam, const float *pose12, float z_near, float z_far, int normals);
/* The whole volume in the logical layout, host pointers: dw nx ny nz x 2 floats; rgb nx ny nz x 3 floats, NULL for (and only for) a volume
 * without colour. */
int icp_tsdf_read (icp_tsdf_handle t, float *dw, float *rgb);
int icp_tsdf_write (icp_tsdf_handle t, const float *dw, const float *rgb);
/* Host only, computed in double and rounded once: out12 = pose12 o (R (q / |q|), t) of the engine's T8 = [q | t, s], the pose of the moving
 * frame of a registration whose fixed frame was ray-cast from pose12.  T's scale s is returned through `scale` (may be NULL), not applied. */
int icp_tsdf_compose_pose (const float *pose12, const float *T8, float *out12, float *scale);
/* Surface extraction: the model itself as a point cloud — the zero crossings of D on the edges of the voxel lattice (what Open3D's
 * extract_point_cloud and KinFu's fetchCloudHost / fetchNormals give), compacted in order on the device.  The arithmetic is the volume's:
 * fp32, each operation rounded on its own, IEEE divide and sqrt, dots as (a0 b0 + a1 b1) + a2 b2; tests/tsdf_surface_ref.py restates
 * every value bit for bit.  The volume is never modified.
 *    Usable.  Voxel v is USABLE iff W (v) >= min_weight and fabsf (D (v)) < 1.f (float comparisons: a NaN in either fails).  The second
 *    test drops the crossings between a truncated free-space value and the back of another surface (Open3D's 0.98).  A fused D reaches
 *    +-1 where the distance along the ray reaches mu, so both ends of a member lie within mu of the surface: choose mu well above the
 *    voxel edge.  Where neighbouring voxels differ by 2 mu or more along the rays — a surface seen along an axis of a volume whose mu
 *    is at most half its voxel edge — no edge has two usable ends and the volume yields nothing.
 *    Edges.  Edge (v, a), a in {x, y, z} = {0, 1, 2}, joins voxel v = (i, j, k) to v + e_a; it exists only where v + e_a is inside the
 *    volume.  With D0 = D (v), D1 = D (v + e_a) the edge is a MEMBER iff both ends are usable and (D0 > 0.f) != (D1 > 0.f): -0 and +0 both
 *    count as "not positive".
 *    Order.  Members are output in ascending 3 * ((k ny + j) nx + i) + a: a function of the volume alone.
 *    Point.  t = D0 / (D0 - D1), in [0, 1] (-0 or +0 where D0 is a zero);  p_a = origin_a + ((float) idx_a + t) * voxel and
 *    p_b = origin_b + (float) idx_b * voxel on the two other axes;  the record is [p_x p_y p_z 1 r g b 1] with the colour
 *    C_ch (v) + t * (C_ch (v + e_a) - C_ch (v)), 0 without `colour`.
 *    Normal (if wanted).  For a voxel u, G_b (u) = D (u + e_b) - D (u - e_b); it is KNOWN iff all six neighbours are inside the volume and
 *    have W > 0 (nothing else is asked of a neighbour: truncated ones count).  G = G (v) + t * (G (v + e_a) - G (v)) per component,
 *    len = sqrtf ((G_0^2 + G_1^2) + G_2^2).  The normal is [G / len, 0] iff both ends' gradients are known and len > 0 (NaN fails),
 *    otherwise [0 0 0 0].  It points from inside to free space, where the ray cast's normals point.
 *    A voxel with D exactly 0 and positive neighbours on both sides of an axis is the end of two members, whose points coincide
 *    (t = 1 on one edge, t = -0 on the next): that is the rule, not a defect.
 * opt == NULL: min_weight 1, no normals.  The call stores the number of members in *count (at most 3 * 2^30) and writes the first
 * min (count, capacity) of them: cloud_out holds capacity x 8 floats, normals_out capacity x 4 floats (host pointers; normals_out is
 * required iff opt->normals).  capacity 0 with NULL outputs is the counting call.  ICP_EINVAL for a NULL count, a min_weight that is not
 * finite and >= 1, normals outside {0, 1}, a NULL output with capacity > 0; ICP_ENOMEM if the device cannot hold the scratch. */
typedef struct {
    float    min_weight;                    /* finite, >= 1 */
    uint32_t normals;                       /* 0 or 1 */
} icp_tsdf_surface_t;
int icp_tsdf_extract_surface (icp_tsdf_handle t, const icp_tsdf_surface_t *opt, uint32_t capacity, void *cloud_out, float *normals_out, uint32_t *count);
/* Mesh extraction: the model as a triangle mesh (what Open3D's extract_triangle_mesh and KinFu's marching cubes give), compacted in order
 * on the device; tests/tsdf_mesh_ref.py restates it.  The volume is never modified.
 *    Vertices.  The vertices are the members of icp_tsdf_extract_surface for the same min_weight and normals: the same records in the
 *    same order, bit for bit.  A vertex index is a member's position.
 *    Cells.  Cell v = (i, j, k) exists where i + 1 < nx, j + 1 < ny and k + 1 < nz.  Its corner c = bx + 2 by + 4 bz is voxel
 *    v + (bx, by, bz).  It is ACTIVE iff all eight corners are usable (W >= min_weight && fabsf (D) < 1.f); its case is the sum of
 *    (D (corner c) > 0.f) << c.  An inactive cell yields nothing: the mesh ends where the usable volume ends.
 *    Cell edges.  Local edge e = 4 a + m: a is its axis, b1 < b2 are the two other axes, m = bit_b1 + 2 bit_b2 of its low corner.  It is
 *    the lattice edge (v + bits, a).  In an active cell it is a member iff its ends differ in sign, and its vertex index is that member's
 *    position.
 *    The case table: 256 entries of at most five triangles, each a triple of local edge ids, generated by this rule (icp_tsdf_mesh_case
 *    returns an entry):
 *      1. The crossing edges are those whose ends differ in sign.
 *      2. Each of the six faces has 0, 2 or 4 crossing edges.  Two give one segment.  Four give two segments, each joining the two face
 *         edges that meet at a POSITIVE corner: positive corners are cut off singly, the two non-positive corners stay joined.  The
 *         choice depends on the face's four signs alone, so the two cells that share a face draw the same segments.
 *      3. Every crossing edge lies on two faces, so the segments close into loops; loops are taken in ascending order of their smallest
 *         edge id.
 *      4. With the vertices at the edge midpoints P_i, a loop is traversed in the direction for which sum P_i x P_i+1 has a positive dot
 *         product with the sum over the loop's edges of the unit vector from the non-positive end to the positive end (never 0).  Triangle
 *         normals (v1 - v0) x (v2 - v0) then point into free space, where the ray cast's and the surface's normals point.
 *      5. Let r be the loop in that direction from its smallest edge id.  The fan (r_s, r_s+i, r_s+i+1), i = 1 .. n - 2, takes as apex
 *         the first r_s in that order none of whose fan diagonals joins two edges of one cube face (a diagonal in a face could be drawn
 *         by the neighbouring cell too, and the edge would carry four triangles).  18 loops move the apex off their smallest edge.
 *      The table has 820 triangles; no case has more than five.
 *    Triangles.  Output in ascending cell index (k ny + j) nx + i and, inside a cell, in table order; a record is three uint32_t vertex
 *    indices, which always refer to the full member order, whatever the vertex capacity is.  A voxel with D exactly 0 gives coincident
 *    vertices and so zero-area triangles: that is the rule, as it is for the points, and keeps the index topology closed.
 * opt, cloud_out, normals_out and vertex_capacity are icp_tsdf_extract_surface's, with its refusals.  Both counts are required;
 * triangles_out (triangle_capacity x 3 words, a host pointer) is required iff triangle_capacity > 0.  The first min (count, capacity)
 * records of each kind are written and nothing past them is touched; both capacities 0 is the counting call, which makes one host round
 * trip for both counts.  ICP_EINVAL, before any launch, also if 5 (nx - 1) (ny - 1) (nz - 1) > 2^32 - 1 (1024 x 1024 x 821 passes,
 * 1024 x 1024 x 822 is refused): the triangle count stays in 32 bits; lifting this limit is later work. */
int icp_tsdf_extract_mesh (icp_tsdf_handle t, const icp_tsdf_surface_t *opt, uint32_t vertex_capacity, void *cloud_out, float *normals_out, uint32_t *vertex_count,
                           uint32_t triangle_capacity, uint32_t *triangles_out, uint32_t *triangle_count);
/* Host only, no device needed: entry case_index of the case table — the number of triangles (0 .. 5) and their local edge ids, three a
 * triangle, 0 past them.  ICP_EINVAL for case_index > 255 or a NULL output. */
int icp_tsdf_mesh_case (uint32_t case_index, uint32_t *n_triangles, uint8_t edges[15]);
/* Registration against the volume itself (the SDF tracker of Bylow, Sturm, Kerl, Kahl and Cremers, RSS 2013; Canelhas et al. 2013): the
 * residual of a moving point is the volume's own value at that point, the Jacobian the volume's own gradient there.  No view, no search
 * structure, no correspondence, no normals.  tests/tsdf_register_ref.py restates it bit for bit.  The volume is never modified.
 *    Inputs.  n moving points, float8 records [x y z 1 r g b 1] in the camera's frame, and pose12 (camera -> world, checked for finiteness
 *    only).  State: R[9], t[3] in fp32 (from pose12), the iteration count k = 0, the flags done = singular = converged = 0.
 *    Per point i, at the state's R, t:
 *      1. It is VALID iff not (x == 0 && y == 0 && z == 0): the engine's invalid point.
 *      2. w_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a in fp32: the ray cast's world point.
 *      3. S = S (w) and G_a = S (w + voxel e_a) - S (w - voxel e_a) are the ray cast's sample and gradient: each of the seven samples has
 *         its own cell and fractions, its own KNOWN test and its fp32 lerps along x, then y, then z; w_a + voxel and w_a - voxel in fp32.
 *      4. It is a MEMBER iff it is valid, all seven samples are known and fabsf (S) < 1.f (NaN fails; a truncated value carries no distance).
 *      5. In double, each operation on its own, converted from float first:  r = -((double) mu * S);
 *         kg = (double) mu / ((double) voxel + (double) voxel);  g_a = G_a * kg;
 *         c = w x g = (wy gz - wz gy, wz gx - wx gz, wx gy - wy gx);  J = (c, g).
 *      6. Its 29 terms: J_a J_b for a <= b, row-major (21); J_a r (6); 1.0; r r.  A non-member contributes 29 exact zeros, selected and never
 *         multiplied: a NaN coordinate makes no NaN.
 *    Sums.  The plane system's two trees: the halving tree over blocks of 256 points, x[i] += x[i + h] for h = 128 .. 1 (points past n are
 *    non-members), then the halving tree over the block partials zero-padded to the next power of two.  n <= 2^20.
 *    Solve and step.  A from the first 21 sums (its upper triangle), b from the next six; x = (omega, tau) by the plane system's LDL^T under
 *    its singularity rule (a pivot not finite or d_j <= 1e-12 A_jj), members == 0 being singular too.  Singular: the pose stays bit for
 *    bit, singular = 1, done = 1.  Otherwise x is a world-frame increment, w' = w + omega x w + tau:
 *      h = omega / 2 (omega_a * 0.5);  inv = 1.0 / sqrt (((hx hx + hy hy) + hz hz) + 1.0);  q = (x, y, z, w) = (hx inv, hy inv, hz inv, inv), as
 *      the point-to-plane step forms it;  dR = the rotation matrix of q by icp_tsdf_compose_pose's formula (1 - 2 (y y + z z), 2 (x y - z w),
 *      ..), q not normalised again;  R'_ab = (float) ((dR_a0 R_0b + dR_a1 R_1b) + dR_a2 R_2b);  t'_a = (float) (((dR_a0 t_0 + dR_a1 t_1) +
 *      dR_a2 t_2) + tau_a), all in double and rounded once;  k = k + 1.
 *      converged = done = 1 when the engine's two convergence tests hold for Tk = [(float) q | (float) tau, 1]:  |q_xyz| < q_w tan
 *      (angle_threshold pi / 360) with q_w > 0, and |tau| < translation_threshold, norms in fp32 as (a a + b b) + c c and sqrtf.
 *    A done state is left as it is by every later iteration.
 * The record: pose12 from R, t; iterations = k; converged; singular; and of the last iteration evaluated, at the pose before its step:
 * members, rmse = sqrt (sum r r / members) (0 without members), and sys = the 27 sums — the first 21 are the information matrix of the
 * pose (J^T J, rotation first, then translation), in the order icp_quality_t uses, the last six J^T r.
 * opt == NULL: max_iterations 20, angle_threshold 0.001 degrees, translation_threshold 0.01 — the defaults of the facades' icp_init.
 * icp_tsdf_register takes the cloud from the host; icp_tsdf_register_from reads F or M (which = ICP_MEM_F / ICP_MEM_M) of registration 0
 * of an initialised handle on the volume's device, device to device, after the handle's stream has drained, and changes nothing in the
 * handle.  A call enqueues max_iterations pairs of launches (k_tsdf_reg_moments, k_tsdf_reg_finalize) on the volume's stream, synchronises
 * once and reads the record: no host round trip between iterations.  Both are blocking; a refused call leaves the volume and the handle
 * as they were, the reason in icp_tsdf_last_error.  ICP_EINVAL for a null pointer, n == 0 or n > 2^20 (for _from: the handle's m), a
 * non-finite pose, options out of range, `which` other than F / M, a handle on another device; ICP_ESTATE for an uninitialised handle or
 * tracked frames in flight. */
typedef struct {
    uint32_t max_iterations;                /* 1 .. 256 */
    double   angle_threshold;               /* degrees, finite, >= 0 */
    double   translation_threshold;         /* engine units, finite, >= 0 */
} icp_tsdf_register_t;
typedef struct {
    float    pose12[12];
    uint32_t iterations, converged, singular, members;
    double   rmse;
    double   sys[27];
} icp_tsdf_registration_t;
int icp_tsdf_register (icp_tsdf_handle t, const icp_tsdf_register_t *opt, const void *cloud_nx8, uint32_t n, const float *pose12, icp_tsdf_registration_t *out);
int icp_tsdf_register_from (icp_tsdf_handle t, const icp_tsdf_register_t *opt, icp_handle h, int which, const float *pose12, icp_tsdf_registration_t *out);
/* Moving volume: the window of the volume follows the camera by whole voxels, on the device (KinFu large-scale, Kintinuous, Open3D's
 * scalable volume), and the part of the surface that a shift drops can be extracted first.  tests/tsdf_shift_ref.py restates it.
 *    State.  The handle keeps base, the origin given at create, and c, the cumulative shift per axis in voxels, 0 at create.
 *    Shift by s.  c'_a = c_a + s_a;  origin_a = base_a + (float) c'_a * voxel in fp32, one multiplication and one addition, each rounded
 *    on its own: recomputed from c', never accumulated, so a thousand shifts round once.  The new voxel (i, j, k) holds the old voxel
 *    (i + s_x, j + s_y, k + s_z) where that lies inside the volume — D, W and C as bit patterns: a NaN, its payload and a -0 survive —;
 *    every other voxel becomes all-zero bits, the state after create.  |s_a| >= n_a on any axis empties the volume and still moves the
 *    window.  s = 0: no launch, nothing changes, ICP_OK.  World points keep their values: old voxel v + s and new voxel v have the same
 *    centre up to the rounding of the origin.
 *    Refusals, the volume untouched: ICP_EINVAL for a NULL pointer, a new |c_a| > 2^24 (so that (float) c_a stays exact), a new origin
 *    that is not finite;  ICP_ENOMEM if the device cannot hold the second buffer.
 *    Every other entry — integrate, both ray casts, read and write, both extractions, both registrations — sees the new origin and the
 *    new contents after a shift, with no other change.
 * icp_tsdf_get_window returns c. */
int icp_tsdf_shift (icp_tsdf_handle t, const int32_t shift[3]);
int icp_tsdf_get_window (icp_tsdf_handle t, int32_t cumulative[3]);
/* The part of the surface inside or outside a box of voxels.  A member (v, a) of icp_tsdf_extract_surface is INSIDE iff both its ends, v and
 * v + e_a, lie in the box lo_b <= idx_b < hi_b; it is OUTSIDE otherwise.  The call returns exactly the full extraction's records for the
 * members of the chosen kind: the same bits and the same normals (gradients look at neighbours wherever they lie), in the same relative
 * order.  For any box INSIDE and OUTSIDE partition the full extraction; an empty box (lo == hi on some axis) makes every member OUTSIDE,
 * the full box every member INSIDE.  The counting call, the capacity prefix and the refusals are icp_tsdf_extract_surface's; in addition
 * ICP_EINVAL for a NULL region, lo > hi, hi > n, a mode other than 0 or 1.  The volume is never modified.  The mesh of a region is not
 * offered: stitching vertex indices across slabs is later work.
 * icp_tsdf_kept_box (host only) gives the box a shift by s keeps: lo_a = max (0, s_a) (at most n_a), hi_a = max (lo_a, min (n_a, n_a + s_a)),
 * mode OUTSIDE.  Extracting with that region and then shifting by s loses no member, whatever the signs of s: a member whose low end stays
 * but whose high end leaves is OUTSIDE (a rule that looked at v alone would drop it from both sets).  ICP_EINVAL for a NULL pointer. */
typedef struct { uint32_t lo[3], hi[3]; uint32_t mode; } icp_tsdf_region_t;   /* voxels lo_a <= idx_a < hi_a, hi_a <= n_a, lo_a <= hi_a */
enum { ICP_TSDF_REGION_INSIDE = 0, ICP_TSDF_REGION_OUTSIDE = 1 };
int icp_tsdf_extract_surface_region (icp_tsdf_handle t, const icp_tsdf_surface_t *opt, const icp_tsdf_region_t *region,
                                     uint32_t capacity, void *cloud_out, float *normals_out, uint32_t *count);
int icp_tsdf_kept_box (const icp_tsdf_t *cfg, const int32_t shift[3], icp_tsdf_region_t *out);
/* When to shift (host only; KinFu large-scale's rule), in double:  centre_a = origin_a + 0.5 (n_a - 1) voxel,  d_a = (point_a - centre_a) /
 * voxel.  The shift is 0 on every axis if max |d_a| <= threshold, otherwise shift_a = lrint (d_a) on every axis (ties to even): the window
 * is centred on the point again.  ICP_EINVAL for a NULL pointer, a NaN d_a or one past the range of int32_t. */
int icp_tsdf_follow (const icp_tsdf_t *cfg, const float point[3], uint32_t threshold, int32_t shift_out[3]);
/* Diagnostic (tools/diag/tsdf_time.py): `reps` launches of one kernel between two events on the volume's stream, after one untimed launch.
 * what = 0: k_tsdf_integrate of (depth, rgb) at pose12 — the volume is left as reps + 1 integrations leave it;  what = 1: k_tsdf_raycast as
 * icp_tsdf_raycast (cam, pose12, z_near, z_far, side) runs it, into scratch (depth, rgb unused);  what = 2: the launches of one
 * icp_tsdf_extract_surface with normals and min_weight 1 as a group, every member into scratch;  what = 3: the two scan launches of
 * that group alone;  what = 4: its last two launches (the members' edges, their records) alone (for 2 .. 7 every argument but reps is unused, cam and
 * pose12 may be NULL);  what = 5: the launches of one icp_tsdf_extract_mesh with normals and min_weight 1 as a group, every vertex and
 * triangle into scratch;  what = 6: its cell sweep alone;  what = 7: its triangle pass alone;  what = 8: the two launches of one iteration of
 * icp_tsdf_register as a group, over the host cloud `depth` points to (side records of 8 floats, 1 .. 2^20) from pose12, the state held at
 * that pose with `done` clear (every group does the same work; the record goes to scratch);  what = 9: k_tsdf_reg_moments of that group alone;
 * what = 10: k_tsdf_shift alone for the shift of three int32_t that `depth` points to, by +s and -s in turn, from the live buffers into the
 * second ones, which are not swapped in: the volume stays as it is;  what = 11: the launches of one icp_tsdf_extract_surface_region with
 * normals and min_weight 1 as a group, for icp_tsdf_kept_box of that shift (for 10 and 11 nothing else but reps is used).
 * Microseconds per launch (per group). */
int icp_tsdf_time (icp_tsdf_handle t, int what, const icp_rgbd_t *cam, const float *pose12, const uint16_t *depth, const uint8_t *rgb, float z_near, float z_far,
                   uint32_t side, uint32_t reps, float *us_per_launch);

/* ICPTransform<QUATERNION> / ICPTransform<MATRIX> with an explicit transformation — include/ICP/algorithms.hpp:1189-1211,
 * 1240, 1348; src/ICP/algorithms.cpp:2554-2753 (quaternion), :2760-2960 (matrix); kernels/icp_kernels.cl:772-802
 * (icpTransform_Quaternion), :842-879 (icpTransform_Quaternion_2: the same mapping through two 4x4 products),
 * :904-933 (icpTransform_Matrix).  T: 8 floats [q | t, s] for the quaternion kinds, 16 floats (row-major 4x4, the
 * scaling already in the rotation block) for MATRIX.  Host in, host out; n points of 8 floats; needs no icp_init. */
typedef enum { ICP_TRANSFORM_QUATERNION = 0, ICP_TRANSFORM_QUATERNION_2 = 1, ICP_TRANSFORM_MATRIX = 2 } icp_transform_kind;
int icp_transform_cloud_ex (icp_handle h, int kind, const float *T, const void *host_in, void *host_out, uint32_t n);

/* ICPPowerMethod — include/ICP/algorithms.hpp:1451-1537 (init / write (D_IN_S, D_IN_MEAN) / run / read (H_OUT_T_K)),
 * src/ICP/algorithms.cpp:2966-3150, kernel icpPowerMethod kernels/icp_kernels.cl:977-1054 — and, with rot = ICP_ROT_EIGEN, the
 * host JacobiSVD of ICPStep<EIGEN, *>::run (src/ICP/algorithms.cpp:3877-3902) as the engine evaluates it on the device.
 * S: the 11 floats of ICPS (S row-major, then the numerator and denominator of the scale); means: [mean_fixed, 0 | mean_moving, 0];
 * Tk: [qk | tk, sk].  power_mode: icp_power_mode (ignored for ICP_ROT_EIGEN).  Rk9 (row-major rotation) and iters (power-method
 * loop trips) may be NULL.  One wave of the same device code the iteration's finalize runs (no other math); host pointers in and
 * out, blocking, needs no icp_init.  The reference's known-answer test (tests/testsICP.cpp:988-1052) drives exactly this entry. */
int icp_power_method (int device, int rot, int power_mode, const float *S11, const float *means8, float *Tk8, float *Rk9, uint32_t *iters);

/* ---- the reference's per-kernel wrapper classes as stand-alone operations (host in, host out, blocking, no icp_init) ---------------
 * A user of the reference can call its kernel classes one by one (and its tests do, tests/testsICP.cpp:66-790); the iteration here
 * fuses these steps (icp_step), so the classes are served by small kernels of their own with the canonical reduction trees —
 * bit-identical to what the fused path computes for the same inputs in reference-order mode.
 *   icp_kernel_lms      ICPLMs      include/ICP/algorithms.hpp:312-383   getLMs: 640 x 480 float8 -> 128 x 128 float8
 *   icp_kernel_reps     ICPReps     :397-468                             getReps (grid side sqrt (m)): m float8 -> nr float8
 *   icp_kernel_weights  ICPWeights  :485-568                             {dist, id}[n] -> W[n], sum of weights (double)
 *   icp_kernel_mean     ICPMean<REGULAR | WEIGHTED>  :625-843            F[n] float8, M[n] float8 (, W[n], sum_w) -> [mean_F, 0 | mean_M, 0]
 *   icp_kernel_devs     ICPDevs     :867-940                             F, M, means -> DF[n] float4, DM[n] float4
 *   icp_kernel_s        ICPS<REGULAR | WEIGHTED>     :976-1183           DM, DF (, W), c -> S[11] (S row-major, sum w |f|^2, sum w |m|^2) */
int icp_kernel_lms (int device, const void *cloud_640x480x8, void *lms_16384x8);
int icp_kernel_reps (int device, const void *F, uint32_t m, uint32_t nr, void *R);
int icp_kernel_weights (int device, const void *nn_id, uint32_t n, float *W, double *sum_w);
int icp_kernel_mean (int device, int weighted, const void *F, const void *M, const float *W, double sum_w, uint32_t n, float *mean8);
int icp_kernel_devs (int device, const void *F, const void *M, const float *mean8, uint32_t n, float *DF, float *DM);
int icp_kernel_s (int device, int weighted, const float *DM, const float *DF, const float *W, uint32_t m, float c, float *S11);
const char *icp_kernel_last_error (void);

/* The same classes as RESIDENT objects — the reference's L2 classes own cl::Buffers, hand them out through get (Memory) and are wired
 * by sharing them (include/ICP/algorithms.hpp:312-1537; wiring src/ICP/algorithms.cpp:4499-4581): device buffers live with the object,
 * icp_ko_device_ptr = get (Memory), icp_ko_adopt = a buffer assigned through get () before init (:2214-2220: the object then does not
 * own it), icp_ko_run = kernels only on the device's null stream (one in-order queue for all kernel objects), icp_ko_write / _read = the
 * staged upload / blocking download of one Memory object.  A slot's buffer is created at its first use, so adoption costs no allocation.
 * Slots (Memory objects) per kind, inputs first:
 *   ICP_KO_LMS      0 cloud 640 x 480 float8          | 1 landmarks 16384 float8
 *   ICP_KO_REPS     0 F n float8 (aux = nr)           | 1 R nr float8
 *   ICP_KO_WEIGHTS  0 {dist, id}[n]                   | 1 W[n], 2 sum of weights (double)
 *   ICP_KO_MEAN(_WEIGHTED)  0 F, 1 M, 2 W[n], 3 sum of weights (double)  | 4 [mean_F, 0 | mean_M, 0]
 *   ICP_KO_DEVS     0 F, 1 M, 2 means (8 floats)      | 3 DF n float4, 4 DM n float4
 *   ICP_KO_S(_WEIGHTED)     0 DM, 1 DF, 2 W[n]        | 3 S[11]     (c: the scaling, icp_ko_set_scaling) */
typedef struct icp_ko *icp_ko_handle;
typedef enum { ICP_KO_LMS = 0, ICP_KO_REPS = 1, ICP_KO_WEIGHTS = 2, ICP_KO_MEAN = 3, ICP_KO_MEAN_WEIGHTED = 4, ICP_KO_DEVS = 5, ICP_KO_S = 6,
               ICP_KO_S_WEIGHTED = 7 } icp_ko_kind;
int icp_ko_create (icp_ko_handle *out, int device, int kind, uint32_t n, uint32_t aux, float c);
int icp_ko_destroy (icp_ko_handle k);
int icp_ko_adopt (icp_ko_handle k, int slot, void *device_ptr);
int icp_ko_device_ptr (icp_ko_handle k, int slot, void **device_ptr);
size_t icp_ko_slot_bytes (icp_ko_handle k, int slot);
int icp_ko_write (icp_ko_handle k, int slot, const void *host);
int icp_ko_read (icp_ko_handle k, int slot, void *host);
int icp_ko_run (icp_ko_handle k);
int icp_ko_set_scaling (icp_ko_handle k, float c);

/* ---- standalone Reduce / Scan classes of the reference ------------------------------ */

/* Reduce<MIN,float> / Reduce<MAX,uint> / Reduce<SUM,float> — include/ICP/algorithms.hpp:52-166,
 * kernels/reduce_kernels.cl:68, 149, 230, src/ICP/algorithms.cpp:131-322.  Row-wise over rows x cols (cols % 4 == 0);
 * host buffers in and out (rows results).  SUM reproduces reduce_sum_f's tree bit for bit. */
typedef enum { ICP_REDUCE_MIN_F = 0, ICP_REDUCE_MAX_UI = 1, ICP_REDUCE_SUM_F = 2 } icp_reduce_op;
int icp_reduce (int device, int op, const void *host_in, uint32_t cols, uint32_t rows, void *host_out);

/* Scan<INCLUSIVE|EXCLUSIVE,int> — include/ICP/algorithms.hpp:169-290, kernels/scan_kernels.cl:67, 188, 296,
 * src/ICP/algorithms.cpp:403-600.  Row-wise over rows x cols ints (cols % 4 == 0). */
int icp_scan (int device, int inclusive, const int32_t *host_in, uint32_t cols, uint32_t rows, int32_t *host_out);
const char *icp_reduce_scan_last_error (void);

/* The same as resident objects, the shape of the reference's classes (ctor / init / write / run / read / get,
 * include/ICP/algorithms.hpp:83-166, 200-290): the device buffers live as long as the object, run enqueues kernels only
 * (no allocation, no copy), device_ptr is `get (Memory::D_IN / D_OUT)` for zero-copy chaining, time brackets `reps` runs
 * with HIP events on the object's stream (the reference's run (timer): 44 us for a 1024 x 1024 sum, 151 us for a scan on its
 * R9 270X, tests/testsReduce.cpp:252, tests/testsScan.cpp:175). */
typedef enum { ICP_RS_MIN_F = 0, ICP_RS_MAX_UI = 1, ICP_RS_SUM_F = 2, ICP_RS_SCAN_INCLUSIVE = 3, ICP_RS_SCAN_EXCLUSIVE = 4 } icp_rs_kind;
typedef struct icp_rs_context *icp_rs_handle;
int icp_rs_create (icp_rs_handle *r, int device, int kind, uint32_t cols, uint32_t rows);
int icp_rs_write (icp_rs_handle r, const void *host_in);            /* cols x rows elements (4 bytes each) */
int icp_rs_run (icp_rs_handle r);                                   /* enqueue only */
int icp_rs_read (icp_rs_handle r, void *host_out);                  /* rows results (reduce) / cols x rows (scan); blocking */
int icp_rs_device_ptr (icp_rs_handle r, int output, void **dptr);   /* 0: input buffer, 1: output buffer (every run's result); both fixed from create to destroy */
int icp_rs_time (icp_rs_handle r, uint32_t reps, float *us_per_run);
int icp_rs_destroy (icp_rs_handle r);

/* ---- batches across devices (SURVEY.md §8b "icp_batch_*", §8e "replicas only") ---------------------------------------------
 * B independent registrations over a device list, inside the library: registration i lives on slot i mod n (slot s =
 * devices[s]; an ordinal may appear more than once) as batch entry i / n of that slot's engine handle, so every slot
 * serves its registrations with one launch set (icp_init_batched).  One host thread + one HIP stream per slot, pinned
 * staging per handle, no collective / peer access / RCCL.  The reference has no counterpart: one context, one in-order
 * queue (src/ICP/algorithms.cpp:4351-4352); per registration the calls mean what ICP<CR,CW>::init / write / buildRBC / run
 * mean (include/ICP/algorithms.hpp:2437-2462).  All calls block until every slot is done. */
typedef struct icp_batch_context *icp_batch_handle;
int icp_batch_create (icp_batch_handle *b, const int *devices, int n_devices, int rot, int weighted);
int icp_batch_destroy (icp_batch_handle b);
int icp_batch_init (icp_batch_handle b, uint32_t registrations, uint32_t m, uint32_t nr, float a, float c,
                    uint32_t max_iterations, double angle_threshold, double translation_threshold);
int icp_batch_set_modes (icp_batch_handle b, int reduce_mode, int power_mode);
int icp_batch_set_rejection (icp_batch_handle b, int flags, float max_dist);                /* icp_set_rejection on every slot */
int icp_batch_set_trimming (icp_batch_handle b, float keep_fraction);                        /* icp_set_trimming on every slot */
int icp_batch_set_unique (icp_batch_handle b, int on);                                       /* icp_set_unique on every slot */
int icp_batch_set_median_rejection (icp_batch_handle b, float factor);                        /* icp_set_median_rejection on every slot */
int icp_batch_set_adaptive_trimming (icp_batch_handle b, float min_fraction, float max_fraction, uint32_t power);   /* icp_set_adaptive_trimming on every slot */
int icp_batch_set_reciprocal (icp_batch_handle b, int on, float max_gap);                    /* icp_set_reciprocal on every slot */
int icp_batch_set_projective (icp_batch_handle b, int on, uint32_t grid_width, float fx, float fy, float cx, float cy, uint32_t radius);   /* icp_set_projective on every slot */
int icp_batch_set_normal_rejection (icp_batch_handle b, int on, float min_cos);              /* icp_set_normal_rejection on every slot */
int icp_batch_set_boundary_rejection (icp_batch_handle b, uint32_t grid_width);              /* icp_set_boundary_rejection on every slot */
int icp_batch_set_robust_loss (icp_batch_handle b, int loss, float scale);                   /* icp_set_robust_loss on every slot */
int icp_batch_set_error_metric (icp_batch_handle b, int metric, float point_weight);         /* icp_set_error_metric on every slot */
int icp_batch_set_normals (icp_batch_handle b, int source, uint32_t grid_width);             /* icp_set_normals on every slot */
int icp_batch_set_color_weight (icp_batch_handle b, float kappa);                            /* icp_set_color_weight on every slot */
int icp_batch_set_plane_to_plane (icp_batch_handle b, float epsilon);                        /* icp_set_plane_to_plane on every slot */
int icp_batch_set_symmetric (icp_batch_handle b, int on);                                    /* icp_set_symmetric on every slot */
int icp_batch_write (icp_batch_handle b, uint32_t i, int mem, const void *host_ptr);       /* mem: F, M, T, NORMALS_F, COLOR_GRAD_F or NORMALS_M of registration i */
int icp_batch_build_rbc (icp_batch_handle b);
int icp_batch_run (icp_batch_handle b);                                                      /* ICP::run of every registration */
int icp_batch_run_fixed (icp_batch_handle b, uint32_t iterations, int from_identity);
int icp_batch_state (icp_batch_handle b, uint32_t i, icp_state_t *out);
int icp_batch_read (icp_batch_handle b, uint32_t i, int mem, void *host_dst, size_t bytes);
int icp_batch_evaluate (icp_batch_handle b, uint32_t i, float max_dist, icp_quality_t *out);   /* icp_evaluate: the record of registration i */
/* icp_correspondences on registration i's slot, then icp_correspondences_read of registration i (capacity, *n and the codes as there) */
int icp_batch_correspondences (icp_batch_handle b, uint32_t i, int source, float max_dist,
                               icp_pair_t *host_dst, uint32_t capacity, uint32_t *n);
int icp_batch_size (icp_batch_handle b, uint32_t *registrations, uint32_t *n_slots);
/* wall-clock seconds of `reps` fixed-length passes (from the identity) on all slots at once = max over devices */
int icp_batch_time_run_fixed (icp_batch_handle b, uint32_t iterations, uint32_t reps, double *seconds);
/* the same with `warmup` untimed passes per slot first, a gate in front of the timed region (every slot has drained its stream
 * before the clock starts), and the HIP-event time of every slot's own passes in slot_ms[n_slots] (may be NULL; 0 for a slot
 * without registrations): what bench.py --gpus N prints per GPU */
int icp_batch_time_run_fixed_slots (icp_batch_handle b, uint32_t iterations, uint32_t reps, uint32_t warmup, double *seconds, float *slot_ms);
/* the partition rule as a pure function (no device needed): slot, index inside the slot, registrations of that slot */
int icp_batch_partition (uint32_t registrations, uint32_t n_slots, uint32_t i, uint32_t *slot, uint32_t *index, uint32_t *slot_count);
/* The CPUs the host thread of `slot` was pinned to, comma-separated ("" = not pinned).             */
int icp_batch_slot_cpus (icp_batch_handle b, uint32_t slot, char *out, size_t cap);
const char *icp_batch_last_error (icp_batch_handle b);   /* b may be NULL: error of the last failed create */

/* ---- coarse-to-fine registration (Open3D: multi_scale_icp; KinectFusion's three-level pyramid; not reference behaviour) ------------
 * An icp_pyramid_* object owns one ordinary engine handle per level, all on one device, and keeps them consistent: the levels of F and
 * M are built on the device from level 0, the coarsest level runs first, and every finer level starts from the transform the level
 * above it ended with.  Nothing else changes: every level runs the kernels, launches and graphs a plain handle of its shape runs.
 * The rule:
 *   Levels
 *   - Level 0 is the finest: m points, a row-major side x side grid, as icp_init requires.  Level l has side_l = side >> l and
 *     m_l = side_l^2.  levels is in [1, ICP_PYRAMID_MAX_LEVELS]; side % (1 << (levels - 1)) == 0 is required.
 *   - Every (m_l, nr[l]) must pass icp_init's own checks — in particular side_l must be even —, else icp_pyramid_init returns
 *     ICP_EINVAL with a message that names the level.
 *   - a, c and the two thresholds are common to all levels; nr[] and max_iterations[] are per level, finest first.
 *   - One registration per level (batch 1).  Batched pyramids and tracked frames are not provided.
 *   Reduction from level l - 1 to level l, applied to F and to M alike
 *   - Per output point (x, y) the block is the four points (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1) of level l - 1, in that
 *     (row-major) order.  A point is valid as in the icp_set_normals rule: xyz finite and not (0, 0, 0).
 *   - ICP_PYRAMID_PICK: the output is the eight floats of block element 0, copied bit for bit.
 *   - ICP_PYRAMID_MEAN (the default): the reference point is the first valid point of the block in block order.  Included are the valid
 *     points with fabsf (z - z_ref) <= band_l in fp32, band_l = max_dz * (float) (1u << (l - 1)): the grid spacing doubles per level,
 *     and so does the band.  max_dz == 0 (the default) or +inf: no band test.  With n included points, for each of x, y, z, r, g, b:
 *     s = the first included point's value, then s = s + next in block order; the output is s / (float) n — fp32, no contraction, an
 *     IEEE divide.  Floats 3 and 7 are written as 1.0f.  A block without a valid point gives the eight floats of element 0, bit for
 *     bit: an invalid pixel stays invalid and keeps its colour.
 *   - Levels are derived recursively: level l from level l - 1, never from level 0 directly.  No atomics; the result does not depend
 *     on the launch shape.
 *   Hand-over of T
 *   - Before level l - 1 runs, its T becomes level l's final T, with the effect of icp_write (ICP_MEM_T) of those eight floats: the
 *     rotation state is re-derived.  The source is the coarser handle's device state: no host copy, no host wait; the two levels'
 *     streams are ordered by events, both ways: the finer level waits for the coarser level's run, and whatever writes the coarser
 *     level's state next (a further run, icp_pyramid_reset_transform, icp_pyramid_write (ICP_MEM_T)) waits for the read.  No
 *     icp_pyramid_sync is needed between icp_pyramid_run_fixed and the next call.
 *   Iteration counts
 *   - In every pyramid run each level's count starts at 0, as after icp_build_rbc; afterwards icp_state (level l).k is what that level
 *     executed in this run.
 * The result is level 0's: icp_read (h0, ICP_MEM_T), icp_state (h0), icp_evaluate (h0, ..) with h0 from icp_pyramid_level (p, 0, &h0).
 * The coarsest level starts from its own current T: the identity after icp_pyramid_init and icp_pyramid_reset_transform, what
 * icp_pyramid_write (ICP_MEM_T) gave it, or — in a second run without either — where its last run ended.
 *
 * icp_pyramid_level hands out the BORROWED handle of a level.  Allowed on it: every setter and getter (modes, metric, normals,
 * rejection, trimming, robust loss, reciprocal correspondences — each level then keeps a moving set of its own —, ..; they survive icp_pyramid_init as they survive icp_init), icp_read, icp_state, icp_evaluate,
 * icp_correspondences, icp_correspondences_read, icp_correspondences_device_ptr, icp_device_ptr, icp_transform_cloud, icp_sync and the diagnostics.  The grid widths of icp_set_normals and icp_set_boundary_rejection are per level
 * (side_l): the caller sets them level by level.  NOT allowed, because they would take the levels apart: icp_init*, icp_destroy,
 * icp_write / icp_write_cloud of F or M, icp_adopt_device_buffer and icp_track_*.
 *
 * icp_pyramid_write       ICP_MEM_F / ICP_MEM_M: the staged upload into level 0 (icp_write), then ONE launch that writes all coarser
 *                         levels into the level handles' own device buffers; every level handle sees that write as it sees an icp_write
 *                         of the same object (lazy outputs are gone; with ICP_NORMALS_GRID the moving normals follow a new M).
 *                         Non-blocking unless `block`: the levels' streams wait on an event, not the host.  ICP_MEM_T: the coarsest
 *                         level's start.
 * icp_pyramid_write_cloud icp_write_cloud into level 0 (m must be 16384), then the same launch.
 * icp_pyramid_set_reduction  survives icp_pyramid_init and takes effect at the next write.  ICP_EINVAL: an unknown kind, max_dz negative or NaN.
 * icp_pyramid_run         a checked icp_run per level, coarsest to finest, the hand-over in front of each finer level; blocking.
 *                         k (may be NULL) receives `levels` counts, finest first.
 * icp_pyramid_run_fixed   exactly iterations[l] steps per level.  Enqueue only: fixed runs, event, hand-over, next level.
 * icp_pyramid_pending     diagnostic: 1 while what the last icp_pyramid_run_fixed enqueued is still in flight (a query, not a wait).
 * icp_pyramid_time_build  measurement: the construction launch of `mem` alone, `reps` times, HIP events around each; mean ms.
 * ICP_ESTATE: a run before icp_pyramid_build_rbc; before icp_pyramid_init every call but create, destroy, the reduction's setter and
 * getter and icp_pyramid_levels (which gives 0). */
#define ICP_PYRAMID_MAX_LEVELS 5
#define ICP_PYRAMID_MEAN 0
#define ICP_PYRAMID_PICK 1
typedef struct icp_pyramid_context *icp_pyramid_handle;
int icp_pyramid_create (icp_pyramid_handle *p, int device, int rot, int weighted);
int icp_pyramid_destroy (icp_pyramid_handle p);
int icp_pyramid_init (icp_pyramid_handle p, uint32_t levels, uint32_t m, const uint32_t *nr, float a, float c,
                      const uint32_t *max_iterations, double angle_threshold, double translation_threshold);
int icp_pyramid_set_reduction (icp_pyramid_handle p, int kind, float max_dz);
int icp_pyramid_get_reduction (icp_pyramid_handle p, int *kind, float *max_dz);
int icp_pyramid_levels (icp_pyramid_handle p, uint32_t *levels);
int icp_pyramid_level (icp_pyramid_handle p, uint32_t l, icp_handle *h);
int icp_pyramid_write (icp_pyramid_handle p, int mem, const void *host_ptr, int block);
int icp_pyramid_write_cloud (icp_pyramid_handle p, int which, const void *host_cloud_640x480x8, int block);
int icp_pyramid_reset_transform (icp_pyramid_handle p);                    /* coarsest T <- identity */
int icp_pyramid_build_rbc (icp_pyramid_handle p);                          /* icp_build_rbc of every level */
int icp_pyramid_run (icp_pyramid_handle p, uint32_t *k);
int icp_pyramid_run_fixed (icp_pyramid_handle p, const uint32_t *iterations);
int icp_pyramid_sync (icp_pyramid_handle p);
/* diagnostics and measurement (as icp_time_*: not part of a registration) */
int icp_pyramid_pending (icp_pyramid_handle p, int *pending);
int icp_pyramid_time_build (icp_pyramid_handle p, int mem, uint32_t reps, float *ms_per_launch);
const char *icp_pyramid_last_error (icp_pyramid_handle p);   /* p may be NULL: error of the last failed create */

/* ---- measurement (bench.py, HIP events on the handle's stream) --------------------------------- */

/* Times `reps` back-to-back icp_run_fixed(iterations) passes with hipEvents recorded on the
 * handle's own stream; *ms_total = elapsed ms over all reps.  from_identity != 0: every pass starts from
 * the identity transform (a fresh registration, like the reference's 40-step profiling run). */
int icp_time_run_fixed (icp_handle h, uint32_t iterations, uint32_t reps, int from_identity, float *ms_total);
/* The same `reps` passes, the events around all but the first: *ms_timed = elapsed ms over *reps_timed = reps - 1 passes (1 of 1).  A marker
 * recorded on an idle stream holds back the graph launched behind it by 0.1 - 0.25 ms; behind a pass in flight it costs nothing.
 * What bench.py brackets its K wall-clock-timed steps with (the wall clock covers all K, the events K - 1 of them). */
int icp_time_run_fixed_tail (icp_handle h, uint32_t iterations, uint32_t reps, int from_identity, float *ms_timed, uint32_t *reps_timed);
/* ICP::run (timer) — include/ICP/algorithms.hpp:2482-2494: the reference's profiling run, exactly `iterations` steps
 * (40 there) from the current state, no convergence test, with a per-step, per-stage table (the reference fills a
 * ProfilingInfo<40> per kernel class through the run (timer) overloads, e.g. :2359-2399).  The stages run as separate
 * launches with HIP events around each: out_ms[it * 4 + s], s = icp_stage; fused reductions have no means / Sij
 * stage (those entries read ~0: two events back to back); with trimming on (icp_set_trimming) the search stage includes the
 * selection and the pass that applies it.  *total_ms (may be NULL) = first event to last.  Blocking.
 * (The graphs behind icp_run / icp_run_fixed fuse stages further — icp_launches_per_iteration — and are timed whole by
 * icp_time_run_fixed.) */
typedef enum { ICP_STAGE_SEARCH = 0, ICP_STAGE_MEANS = 1, ICP_STAGE_SIJ = 2, ICP_STAGE_FINALIZE = 3, ICP_STAGE_COUNT_ = 4 } icp_stage;
int icp_profile_run (icp_handle h, uint32_t iterations, float *out_ms, float *total_ms);
/* Means of the same over `reps` iterations: out_ms[0..3] = mean ms of {search, means, sij, finalize}. */
int icp_time_kernels (icp_handle h, uint32_t reps, float *out_ms4);

/* Kernel launches per iteration of the graphs behind icp_run / icp_run_fixed with the current modes and sizes:
 * 4 (reference-order reductions), 2 (fused: search + finalize; 3 beyond |F| = 16384, where the first level of the
 * moment tree is a launch of its own) or 1 (fused, latency-bound sizes: chained, see icp_run_form).  The small second-level
 * launches of the reference-order reductions (the sum of the weights beyond 65536 pairs, the global means beyond 16384) are not
 * counted: the "4" holds at every size. */
int icp_launches_per_iteration (icp_handle h, uint32_t *n);

/* How icp_run / icp_run_fixed execute with the current modes and sizes:
 *   SEPARATE    one launch per stage (2 fused, 4 reference order);
 *   CHAINED     fused, one launch per iteration: the finalize of iteration k runs in the prologue of the search of
 *               iteration k+1 (latency-bound sizes; ICP_AMD_CHAIN=0 / 1 at icp_create forces it off / on);
 *   (a third form — one persistent launch per run, the per-iteration moment exchange between the blocks in-launch — was built and
 *   measured in round 2: 10.7 against 9.8 us per iteration at |F| = 16384, the all-to-all seam costs more than the launch boundary
 *   it replaces; retired in round 3)
 * Same bits in both forms. */
typedef enum { ICP_FORM_SEPARATE = 0, ICP_FORM_CHAINED = 1 } icp_run_form_t;
int icp_run_form (icp_handle h, int *form);
/* Diagnostic: how the search kernel behind the current modes and sizes is laid out.
 *   *dense   0: the latency variant (one 1024-thread block per CU, 16 lanes per query: a single small registration);
 *            1: the dense variant (512-thread blocks, several per CU, 8 lanes per query, exact stage-1 pruning);
 *   *tile    representatives per LDS tile (256 or 1024);
 *   *stage2  0: the lanes of a query scan its representative's list; 1: lanes = candidates — a wave loads a list once for
 *            all of its queries that share it (dense variant, lists of >= 128 candidates on average; ICP_AMD_S2WAVE=0 / 1 at
 *            icp_init forces it off / on).
 * Same bits in every layout.  Any output pointer may be NULL. */
int icp_search_layout (icp_handle h, int *dense, int *tile, int *stage2);

/* Diagnostic: a graph of `iterations` x (the kernels selected by mask: bit 0 search, 1 means, 2 sij,
 * 3 finalize, 4 an empty 256-block kernel), launched `reps` times; *ms_total = elapsed ms. */
int icp_time_masked (icp_handle h, uint32_t mask, uint32_t iterations, uint32_t reps, float *ms_total);

/* ---- utilities ---------------------------------------------------------------------------------- */

const char *icp_last_error (icp_handle h);      /* h may be NULL: error of the last failed create */
const char *icp_version (void);
int icp_device_count (int *n);
/* PCI bus id of device `device` ("0000:c1:00.0"; cap >= 16).                                        */
int icp_device_pci_bus_id (int device, char *out, size_t cap);
/* The cpulist ("0-47,96-143") of the NUMA node a PCI device hangs on, from a sysfs tree (sysfs_root NULL = "/sys"):
 * <root>/bus/pci/devices/<id>/local_cpulist, else node<numa_node>/cpulist; out = "" when the tree has no answer.
 * icp_batch_create pins the host thread of every device slot there unless ICP_AMD_SLOT_CPUS says otherwise
 * (ICP_AMD_SLOT_NUMA=0: no default placement).  No reference counterpart: one device, one queue
 * (src/ICP/algorithms.cpp:4351-4352).                                                                */
int icp_numa_cpulist (const char *sysfs_root, const char *pci_bus_id, char *out, size_t cap);

/* Synthetic RGB-D landmark pair: side x side grid, fixed and moving frame.
 * Host only; deterministic in (seed, side). */
int icp_synth_pair (uint64_t seed, uint32_t side, float rot_deg, const float *axis3,
                    const float *t3, float noise_mm, float noise_rgb, float zero_fraction,
                    float *F, float *M);
/* The same with a choice of scene.  scene 0: the curved scene of icp_synth_pair.  scene 1: a WALL — the reference's second example pair,
 * data/kg_pc8d_wall ("non-salient surface geometry ... highlights the benefit of utilizing the photometric information",
 * data/README.md:11-16): a tilted plane with a millimetre of surface roughness and the procedural texture, moved IN its own plane (a
 * rotation by rot_deg about the plane's normal through its centre — axis3 is ignored — and the in-plane part of t3): geometry alone
 * cannot see that motion.  T_true8 (may be NULL): the ground truth [q | t, 1] mapping the moving frame onto the fixed one. */
int icp_synth_pair_scene (uint64_t seed, uint32_t side, int scene, float rot_deg, const float *axis3, const float *t3,
                          float noise_mm, float noise_rgb, float *F, float *M, float *T_true8);
/* Synthetic 640x480 float8 cloud for the getLMs path; `moved` = frame number of a sequence (0: the scene, f: moved
 * rigidly by f steps of 3 degrees / (25, -10, 15) mm, with noise). */
int icp_synth_cloud_vga (uint64_t seed, int moved, float *cloud);
/* Invalid pixels as a Kinect frame holds them — depth 0: x = y = z = 0, the colour written regardless (reference
 * src/kinect_frame_grabber.cpp:246-262; getLMs picks such points on purpose, kernels/icp_kernels.cl:49-50) — punched in place into a
 * width x height grid of float8 points (a landmark set: side x side; a cloud: 640 x 480).  pattern 0: scattered, every point with
 * probability `fraction`; 1: contiguous — a band along the left edge and random ellipses until `fraction` of the points is covered.
 * keep_rgb 0 zeroes the colour too: all invalid points identical, one representative's list holds them all (the degenerate case). */
int icp_synth_punch_holes (uint64_t seed, uint32_t width, uint32_t height, int pattern, float fraction, int keep_rgb, float *cloud);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* ICP_AMD_H */
