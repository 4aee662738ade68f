// icp_rbc_set.h — the one description of an RBC set: the 15 device buffers buildRBC writes and the searches read.  Host side only:
// icp_params keeps its flat fields (the pointers sit between scalars there, and no byte of it may move), this table says which of
// them make up a set, what each holds and how large it is.  icp_init_batched allocates the handle's set from it, tracking its second
// one (icp_track.hip: frame f + 1's RBC is built on the other stream while frame f is still searching its own), free_all frees that.
#pragma once
#include "icp_kernels.h"

// X (element type, name, elements) in allocation order; the count is an expression of p's size fields (batch, m, nr, n16, n1k, nlb,
// nchunk, nb) and of B = (size_t) p.batch.
#define ICP_RBC_BUFFERS(X)                                                                                                           \
    X (float,    R,          B * p.nr * 8)                                                                                           \
    X (float4,   GB,         B * 2 * (p.n16 + p.n1k))                                                                                \
    X (float,    XP,         icp_xp_layout_of (p.batch, p.m).total)      /* behind the database: NORMALS_F, COLOR_GRAD_F, NORMALS_M */ \
    X (float,    XQ,         B * p.m * 8)                                                                                            \
    X (float4,   OL,         B * ICP_OL_STRIDE (p.nr))                                                                               \
    X (float4,   LB,         B * 3 * p.nlb)                                                                                          \
    X (uint32_t, rep_src,    B * p.nr)                                                                                               \
    X (uint32_t, owner,      B * p.m)                                                                                                \
    X (uint32_t, N,          2 * B * p.nr)                               /* the search's view of the lengths, then ICP_N_FULL */      \
    X (uint32_t, O,          B * p.nr)                                                                                               \
    X (uint32_t, perm,       B * p.m)                                                                                                \
    X (uint32_t, chunk_hist, B * p.nchunk * p.nr)                                                                                    \
    X (uint2,    blist,      B * p.nb * 64)                                                                                          \
    X (uint32_t, bn,         B * p.nb)                                                                                               \
    X (uint8_t,  brank,      B * p.m)

struct icp_rbc_set {
#define X(type, name, count) type *name = nullptr;
    ICP_RBC_BUFFERS (X)
#undef X
};

#define X(type, name, count) +1
constexpr int ICP_RBC_NBUF = 0 ICP_RBC_BUFFERS (X);
#undef X

// f (name, the set's pointer as void **, bytes) for every buffer, in allocation order; stops at the first nonzero return and hands it on
template <typename F>
int icp_rbc_for_each (icp_rbc_set &s, const icp_params &p, F &&f)
{
    const size_t B = p.batch;
    int rc = 0;
#define X(type, name, count) if ((rc = f (#name, reinterpret_cast<void **> (&s.name), (size_t) (count) * sizeof (type)))) return rc;
    ICP_RBC_BUFFERS (X)
#undef X
    return rc;
}

inline void icp_rbc_into (icp_params &p, const icp_rbc_set &s)
{
#define X(type, name, count) p.name = s.name;
    ICP_RBC_BUFFERS (X)
#undef X
}

inline icp_rbc_set icp_rbc_of (const icp_params &p)
{
    icp_rbc_set s;
#define X(type, name, count) s.name = p.name;
    ICP_RBC_BUFFERS (X)
#undef X
    return s;
}

// What reciprocal correspondences (icp_set_reciprocal, icp_reciprocal.hip) keep per handle: the moving set — an RBC over M, built by
// buildRBC's own launches —, the reverse state ([batch] icp_reg_state: T = the inverse transform, the rest the run's), and the back
// search's per-query outputs ([batch][m] each; nn_id is ICP_MEM_REVERSE_ID).  icp_params has no room for the pointers: the route's
// launchers take this record beside it.  Allocated when the rule is first needed on an initialised handle, each buffer on its own.
// stale: the moving set does not describe M (M was written, the rule was switched on after icp_build_rbc, icp_init): the next call
// that enqueues an iteration rebuilds it first.
struct icp_reciprocal_set {
    icp_rbc_set rbc;
    icp_reg_state *st = nullptr;
    icp_dist_id *nn_id = nullptr; float4 *PF = nullptr, *PM = nullptr; uint32_t *rid = nullptr;
    bool stale = true;
};
