// mom_layout_test.cpp — the word areas behind the moments (icp_amd/csrc/icp_kernels.h: icp_mom_layout_of, icp_words and the accessors)
// and the words of a selection under both its rules (icp_median_desc, icp_select_words_of) against offsets written out by hand: host
// only, no HIP call.  `make mom_layout_test` builds and runs it; tests/test_mom_layout_cpu.py
// does too.  The offsets are an ABI between the kernels, the C-ABI's icp_read and the graphs that have captured them: they must not move.
#include <cstdint>
#include <cstdio>
#include "../../icp_amd/csrc/icp_kernels.h"

struct shape { uint32_t batch, m, nb; };
static const shape SHAPES[] = {
    { 1u, 16u, 1u }, { 1u, 900u, 15u }, { 3u, 16384u, 256u }, { 1u, 65536u, 1024u }, { 64u, 16384u, 256u }, { 1u, 1048576u, 16384u },
};

static int bad = 0, n = 0;
static void check (const shape &s, const char *what, size_t got, size_t want)
{
    ++n;
    if (got != want) { std::printf ("batch %u m %u nb %u: %s is %zu, expected %zu\n", s.batch, s.m, s.nb, what, got, want); ++bad; }
}

int main ()
{
    for (const shape &s : SHAPES) {
        const size_t B = s.batch, m = s.m, nb = s.nb;
        // by hand, in doubles: the moment partials, then area by area
        const size_t keys = m > 16384 ? B * m : 0;                       // trimming keeps its keys beyond one workgroup's selection
        const size_t trim_words = B * 4 + B * 4 + B * 2048 + keys;       // result, selection state, histograms, keys
        const size_t nblk = (m + 255) / 256;
        const size_t trim = B * 2 * 18 * nb;
        const size_t sys = trim + (trim_words + 1) / 2;
        const size_t part = sys + B * 28;
        const size_t kappa = part + B * 27 * nblk, robust = kappa + 1, gicp = kappa + 2;
        const size_t uniq = kappa + 3;
        const size_t claims = uniq + B;                                  // behind [batch][2] uint32
        const size_t filt = claims + B * m;
        const size_t recip = filt + (B * 4 + B * 8 + 2 + 1) / 2;         // = 6 B + 1
        const size_t proj = recip + (B * 4 + 1 + 1) / 2;                 // = 2 B + 1
        const size_t total = proj + (B * 4 + B * 8 + 6 + 1) / 2;         // = 6 B + 3

        const icp_mom_layout l = icp_mom_layout_of (s.batch, s.m, s.nb);
        check (s, "trim", l.area[ICP_AREA_TRIM], trim);
        check (s, "sys", l.area[ICP_AREA_PLANE], sys);
        check (s, "part", l.part, part);
        check (s, "kappa", l.kappa, kappa);
        check (s, "robust", l.robust, robust);
        check (s, "gicp", l.gicp, gicp);
        check (s, "uniq", l.area[ICP_AREA_UNIQUE], uniq);
        check (s, "filt", l.area[ICP_AREA_FILTER], filt);
        check (s, "recip", l.area[ICP_AREA_RECIPROCAL], recip);
        check (s, "proj", l.area[ICP_AREA_PROJECTIVE], proj);
        check (s, "total", l.total, total);

        // the accessors, as byte offsets from p.mom (a made-up address that nothing dereferences)
        icp_params p {};
        p.batch = s.batch; p.m = s.m; p.nb = s.nb;
        const uintptr_t base = 0x40000000u;
        p.mom = reinterpret_cast<double *> (base);
        auto at = [&] (const void *q) { return (size_t) (reinterpret_cast<uintptr_t> (q) - base); };
        const icp_area_words t = icp_words (p, ICP_AREA_TRIM), u = icp_words (p, ICP_AREA_UNIQUE), f = icp_words (p, ICP_AREA_FILTER);
        const icp_area_words r = icp_words (p, ICP_AREA_RECIPROCAL), j = icp_words (p, ICP_AREA_PROJECTIVE), y = icp_words (p, ICP_AREA_PLANE);
        check (s, "trimming's result words", at (t.result), 8 * trim);
        check (s, "trimming's selection state", at (t.running), 8 * trim + 4 * (4 * B));
        check (s, "trimming's keys", at (t.settings), 8 * trim + 4 * ((8 + 2048) * B));
        check (s, "the plane system", at (icp_p2pl_area (p)), 8 * sys);
        check (s, "the plane system's words", at (y.result), 8 * sys);
        check (s, "the plane system's partials", at (icp_p2pl_part (p)), 8 * part);
        check (s, "kappa's word", at (icp_color_kappa (p)), 8 * kappa);
        check (s, "the robust scale's word", at (icp_robust_scale (p)), 8 * robust);
        check (s, "epsilon's word", at (icp_gicp_eps (p)), 8 * gicp);
        check (s, "one-to-one's result words", at (u.result), 8 * uniq);
        check (s, "the claim table", at (icp_unique_claims (p)), 8 * claims);
        check (s, "the claim table's alignment", at (icp_unique_claims (p)) % 8, 0);
        check (s, "the pair filter's result words", at (f.result), 8 * filt);
        check (s, "the pair filter's running words", at (f.running), 8 * filt + 4 * (4 * B));
        check (s, "the pair filter's settings", at (f.settings), 8 * filt + 4 * (12 * B));
        check (s, "reciprocal's result words", at (r.result), 8 * recip);
        check (s, "reciprocal's gap", at (r.settings), 8 * recip + 4 * (4 * B));
        check (s, "projective's result words", at (j.result), 8 * proj);
        check (s, "projective's running words", at (j.running), 8 * proj + 4 * (4 * B));
        check (s, "projective's settings", at (j.settings), 8 * proj + 4 * (12 * B));

        // median-distance rejection's words, an allocation of their own, as uint32 offsets from its first word: result 0, the
        // selection's state 4 B, its histograms 8 B, the factor (8 + 2048) B, the keys two words behind it
        uint32_t *const mbase = reinterpret_cast<uint32_t *> (base);
        auto word = [&] (const uint32_t *q) { return (size_t) (q - mbase); };
        const size_t fixed = (8 + 2048) * B;
        const icp_area_words mw = icp_words (mbase, icp_median_desc (), B);
        check (s, "median's result words", word (mw.result), 0);
        check (s, "median's selection state", word (mw.running), 4 * B);
        check (s, "median's factor", word (mw.settings), fixed);
        check (s, "median's total", icp_area_size (icp_median_desc (), B, icp_select_keys (B, s.m)), fixed + 2 + keys);
        // a registration's words in the multi-workgroup selection, under both rules: trimming's area has no settings in front of the keys
        const struct { const char *rule; uint32_t *first; icp_area_desc d; size_t settings; } RULES[] = {
            { "median", mbase, icp_median_desc (), 2 }, { "trimming", t.result, icp_area_desc_of (ICP_AREA_TRIM), 0 },
        };
        for (const auto &r : RULES)
            for (const size_t b : { (size_t) 0, B - 1 }) {
                const icp_select_words w = icp_select_words_of (r.first, r.d, s.batch, (uint32_t) b, s.m);
                const size_t first = word (r.first);
                check (s, r.rule, word (w.out), first + 4 * b);
                check (s, r.rule, word (w.sel), first + 4 * B + 4 * b);
                check (s, r.rule, word (w.hist), first + 8 * B + 2048 * b);
                check (s, r.rule, word (w.keys), first + fixed + r.settings + b * m);
            }

        // consecutive areas do not overlap: each one's bytes, by hand, end where the next begins or before
        const struct { const char *name; size_t begin, bytes; } AREAS[] = {
            { "moment partials", 0, 8 * B * 2 * 18 * nb }, { "trimming", at (t.result), 4 * trim_words }, { "plane system", at (y.result), 8 * 28 * B },
            { "plane partials", at (icp_p2pl_part (p)), 8 * B * 27 * nblk }, { "kappa", at (icp_color_kappa (p)), 4 }, { "robust scale", at (icp_robust_scale (p)), 4 },
            { "epsilon", at (icp_gicp_eps (p)), 4 }, { "one-to-one", at (u.result), 4 * 2 * B }, { "claim table", at (icp_unique_claims (p)), 8 * B * m },
            { "pair filter", at (f.result), 4 * (12 * B + 2) }, { "reciprocal", at (r.result), 4 * (4 * B + 1) }, { "projective", at (j.result), 4 * (12 * B + 6) },
            { "the end", 8 * l.total, 0 },
        };
        for (size_t k = 0; k + 1 < sizeof AREAS / sizeof AREAS[0]; ++k) {
            ++n;
            if (AREAS[k].begin + AREAS[k].bytes > AREAS[k + 1].begin) {
                std::printf ("batch %u m %u nb %u: %s (%zu + %zu bytes) runs into %s (%zu)\n", s.batch, s.m, s.nb, AREAS[k].name, AREAS[k].begin, AREAS[k].bytes,
                             AREAS[k + 1].name, AREAS[k + 1].begin);
                ++bad;
            }
        }
    }
    // an area's result words per registration: what commit clears and what icp_read hands out (16, 224, 8, 16, 16, 16 bytes)
    const struct { int area; const char *name; uint32_t words; } RESULT[] = {
        { ICP_AREA_TRIM, "ICP_MEM_TRIM", 4 }, { ICP_AREA_PLANE, "ICP_MEM_PLANE_SYSTEM (28 doubles)", 56 }, { ICP_AREA_UNIQUE, "ICP_MEM_UNIQUE", 2 },
        { ICP_AREA_FILTER, "ICP_MEM_PAIR_FILTER", 4 }, { ICP_AREA_RECIPROCAL, "ICP_MEM_RECIPROCAL", 4 }, { ICP_AREA_PROJECTIVE, "ICP_MEM_PROJECTIVE", 4 },
    };
    for (const auto &r : RESULT) check (SHAPES[0], r.name, icp_area_desc_of (r.area).result, r.words);
    static_assert (sizeof (icp_params) == 480, "icp_params must not change");
    if (bad) { std::printf ("mom_layout_test: %d of %d checks wrong\n", bad, n); return 1; }
    std::printf ("mom_layout_test: %d checks ok\n", n);
    return 0;
}
