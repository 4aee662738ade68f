// search_select_test.cpp — the selection of the dense search kernel (icp_amd/csrc/icp_search_select.h: ks_dense_select) against the rule
// written out as a table: host only, no HIP call.  `make search_select_test` builds and runs it; tests/test_search_select_cpu.py does too.
//   tile 256 iff nr <= 256 or the representative grid is at most 64 wide; SINGLE iff tile 256 and nr <= 256; MASKED iff tile 256 and
//   nr > 256; neither at tile 1024; S2W iff s2wave; grid x = nb (fused) or 2 * nwg (reference order); 512 threads.
#include <cstdint>
#include <cstdio>
#include "../../icp_amd/csrc/icp_search_select.h"

struct row { uint32_t nr, nrx, tile; bool single, masked; };
static const row TABLE[] = {
    {    1,  16,  256, true,  false }, {    1,  64,  256, true,  false }, {    1,  65,  256, true,  false }, {    1, 128,  256, true,  false },
    {   64,  16,  256, true,  false }, {   64,  64,  256, true,  false }, {   64,  65,  256, true,  false }, {   64, 128,  256, true,  false },
    {  256,  16,  256, true,  false }, {  256,  64,  256, true,  false }, {  256,  65,  256, true,  false }, {  256, 128,  256, true,  false },
    {  257,  16,  256, false, true  }, {  257,  64,  256, false, true  }, {  257,  65, 1024, false, false }, {  257, 128, 1024, false, false },
    {  512,  16,  256, false, true  }, {  512,  64,  256, false, true  }, {  512,  65, 1024, false, false }, {  512, 128, 1024, false, false },
    { 4096,  16,  256, false, true  }, { 4096,  64,  256, false, true  }, { 4096,  65, 1024, false, false }, { 4096, 128, 1024, false, false },
    { 4097,  16,  256, false, true  }, { 4097,  64,  256, false, true  }, { 4097,  65, 1024, false, false }, { 4097, 128, 1024, false, false },
    { 8192,  16,  256, false, true  }, { 8192,  64,  256, false, true  }, { 8192,  65, 1024, false, false }, { 8192, 128, 1024, false, false },
};

int main ()
{
    static_assert (sizeof (TABLE) / sizeof (TABLE[0]) == 8 * 4, "eight sizes x four grid widths");
    const uint32_t nb = 37u, nwg = 5u;               // (any two numbers with nb != 2 * nwg)
    int bad = 0, n = 0;
    for (const row &r : TABLE)
        for (uint32_t s2wave = 0; s2wave < 2; ++s2wave)
            for (uint32_t fused = 0; fused < 2; ++fused, ++n) {
                const ks_dense_form f = ks_dense_select (r.nr, r.nrx, s2wave);
                const uint32_t gx = ks_dense_grid_x (fused != 0u, nb, nwg);
                const bool ok = f.tile == r.tile && icp_dense_tile_rule (r.nr, r.nrx) == r.tile && f.single == r.single && f.masked == r.masked &&
                                f.s2w == (s2wave == 1u) && KS_DENSE_THREADS == 512u && gx == (fused ? 37u : 10u);
                if (!ok) {
                    ++bad;
                    std::printf ("nr %u nrx %u s2wave %u fused %u: tile %u single %d masked %d s2w %d grid x %u\n", r.nr, r.nrx, s2wave, fused, f.tile, (int) f.single,
                                 (int) f.masked, (int) f.s2w, gx);
                }
            }
    if (bad) { std::printf ("search_select_test: %d of %d cases wrong\n", bad, n); return 1; }
    std::printf ("search_select_test: %d cases ok\n", n);
    return 0;
}
