// rbc_set_test.cpp — the table of an RBC set (icp_amd/csrc/icp_rbc_set.h) against the sizes written out by hand: host only, no HIP call.
// `make rbc_set_test` builds and runs it; tests/test_rbc_set_cpu.py does too.  Every allocation of the handle's set (icp_init_batched)
// and of tracking's second one (track_prepare) takes its size from the table, so these are the bytes both of them get.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../icp_amd/csrc/icp_rbc_set.h"

// tbox: icp_tbox_of's rule (icp_kernels.hip), read off for each shape — 256 for a dense multi-tile set whose tile is 256, else 1024
struct shape { uint32_t m, nr, batch, tbox; };
static const shape SHAPES[] = {
    { 16384u, 256u, 1u, 1024u }, { 65536u, 1024u, 1u, 1024u }, { 1u << 20, 4096u, 1u, 256u }, { 900u, 4u, 40u, 1024u }, { 36864u, 2048u, 1u, 256u }, { 4u, 1u, 1u, 1024u },
};

struct want { const char *name; size_t bytes; };

static size_t ceil_div (size_t a, size_t b) { return (a + b - 1) / b; }

int main ()
{
    int bad = 0, n = 0;
    if (ICP_RBC_NBUF != 15) { std::printf ("the table has %d entries, not 15\n", ICP_RBC_NBUF); ++bad; }
    for (const shape &s : SHAPES) {
        icp_params p {};
        p.batch = s.batch; p.m = s.m; p.nr = s.nr;
        p.n16 = (s.nr + 15u) / 16u; p.tbox = s.tbox; p.n1k = (s.nr + s.tbox - 1u) / s.tbox;
        p.nlb = s.m / 16u + 2u; p.nchunk = (s.m + 1023u) / 1024u; p.nb = (s.m + 63u) / 64u;
        const size_t B = s.batch, m = s.m, nr = s.nr;
        const size_t ol_stride = nr + 1 + 2 * ceil_div (nr, 8) + ceil_div (nr, 128);       // float4 per registration: count, entries, chunk boxes, ballots
        const want WANT[] = {
            { "R", B * nr * 32 },
            { "GB", B * 2 * (ceil_div (nr, 16) + ceil_div (nr, s.tbox)) * 16 },
            { "XP", B * m * 80 },
            { "XQ", B * m * 32 },
            { "OL", B * ol_stride * 16 },
            { "LB", B * 3 * (m / 16 + 2) * 16 },
            { "rep_src", B * nr * 4 },
            { "owner", B * m * 4 },
            { "N", 2 * B * nr * 4 },
            { "O", B * nr * 4 },
            { "perm", B * m * 4 },
            { "chunk_hist", B * ceil_div (m, 1024) * nr * 4 },
            { "blist", B * ceil_div (m, 64) * 512 },
            { "bn", B * ceil_div (m, 64) * 4 },
            { "brank", B * m },
        };
        if (ol_stride != ICP_OL_STRIDE (s.nr)) { std::printf ("nr %u: ICP_OL_STRIDE %u, by hand %zu\n", s.nr, ICP_OL_STRIDE (s.nr), ol_stride); ++bad; }
        icp_rbc_set set;
        std::vector<want> got;
        std::vector<void **> slots;
        icp_rbc_for_each (set, p, [&] (const char *name, void **q, size_t bytes) { got.push_back ({ name, bytes }); slots.push_back (q); return 0; });
        if (got.size () != 15u) { std::printf ("m %u nr %u batch %u: %zu buffers visited\n", s.m, s.nr, s.batch, got.size ()); ++bad; continue; }
        for (size_t k = 0; k < 15u; ++k, ++n)
            if (std::strcmp (got[k].name, WANT[k].name) || got[k].bytes != WANT[k].bytes) {
                std::printf ("m %u nr %u batch %u: buffer %zu is %s with %zu bytes, expected %s with %zu\n", s.m, s.nr, s.batch, k, got[k].name, got[k].bytes, WANT[k].name, WANT[k].bytes);
                ++bad;
            }
        // the visitor hands out the set's own 15 pointers, each once
        for (size_t k = 0; k < 15u; ++k) *slots[k] = reinterpret_cast<void *> ((uintptr_t) (0x1000u * (k + 1u)));
        const void *seen[15] = { set.R, set.GB, set.XP, set.XQ, set.OL, set.LB, set.rep_src, set.owner, set.N, set.O, set.perm, set.chunk_hist, set.blist, set.bn, set.brank };
        for (size_t k = 0; k < 15u; ++k)
            if (seen[k] != reinterpret_cast<void *> ((uintptr_t) (0x1000u * (k + 1u)))) { std::printf ("slot %zu is not the set's %s\n", k, WANT[k].name); ++bad; }
    }
    {   // icp_params -> set -> icp_params gives back every one of the 15 pointers, and touches nothing else
        icp_params a {};
        uintptr_t v = 0x10000u;
        auto next = [&] () { v += 0x100u; return v; };
        a.R = reinterpret_cast<float *> (next ()); a.GB = reinterpret_cast<float4 *> (next ()); a.OL = reinterpret_cast<float4 *> (next ());
        a.LB = reinterpret_cast<float4 *> (next ()); a.XP = reinterpret_cast<float *> (next ()); a.XQ = reinterpret_cast<float *> (next ());
        a.rep_src = reinterpret_cast<uint32_t *> (next ()); a.owner = reinterpret_cast<uint32_t *> (next ()); a.N = reinterpret_cast<uint32_t *> (next ());
        a.O = reinterpret_cast<uint32_t *> (next ()); a.perm = reinterpret_cast<uint32_t *> (next ()); a.chunk_hist = reinterpret_cast<uint32_t *> (next ());
        a.blist = reinterpret_cast<uint2 *> (next ()); a.bn = reinterpret_cast<uint32_t *> (next ()); a.brank = reinterpret_cast<uint8_t *> (next ());
        const icp_rbc_set s = icp_rbc_of (a);
        icp_params b {};
        icp_rbc_into (b, s);
        const bool back = b.R == a.R && b.GB == a.GB && b.OL == a.OL && b.LB == a.LB && b.XP == a.XP && b.XQ == a.XQ && b.rep_src == a.rep_src && b.owner == a.owner &&
                          b.N == a.N && b.O == a.O && b.perm == a.perm && b.chunk_hist == a.chunk_hist && b.blist == a.blist && b.bn == a.bn && b.brank == a.brank;
        if (!back) { std::printf ("icp_params -> set -> icp_params lost a pointer\n"); ++bad; }
        if (std::memcmp (&a, &b, sizeof (icp_params))) { std::printf ("icp_rbc_into wrote a field that is no part of the set\n"); ++bad; }
        ++n;
    }
    static_assert (sizeof (icp_params) == 480, "icp_params must not change");
    static_assert (sizeof (icp_rbc_set) == 15 * sizeof (void *), "an RBC set is its 15 pointers");
    if (bad) { std::printf ("rbc_set_test: %d of %d checks wrong\n", bad, n); return 1; }
    std::printf ("rbc_set_test: %d checks ok\n", n);
    return 0;
}
