// icp_search_select.h — which dense search kernel runs: the tile of the dense variants and the form of their launch, as pure host
// functions of a registration's sizes.  No HIP, no kernels: icp_kernels.h includes it for the launchers (icp_search.h: ks_launch_dense;
// icp_kernels.hip: icp_dense_tile), tests/cpp/search_select_test.cpp checks it against the rule written out as a table.
#pragma once
#include <stdint.h>

// LDS tile of the dense search variant: 256 representatives (21 KB of LDS, 8 waves per SIMD) where a tile holds whole rows of
// 4 x 4 pruning groups (representative grid at most 64 wide: |R| <= 4096), else 1024.
// (Several 256-tiles with a block vote per tile measured slower than the 1024-tile — B 16.6 -> 17.5 us, C 417 -> 520 us —: the
// MASKED form of k_search decides a block's tile set in one pre-pass instead.)
static inline uint32_t icp_dense_tile_rule (uint32_t nr, uint32_t nrx) { return (nr <= 256u || nrx <= 64u) ? 256u : 1024u; }

// The dense search of a registration with nr representatives on a grid nrx wide:
//   tile    = icp_dense_tile_rule (nr, nrx);
//   single  iff tile == 256 and nr <= 256  (k_search's SINGLE: one tile, the tile loop folds away);
//   masked  iff tile == 256 and nr > 256   (the SINGLE = false instantiation at tile 256: k_search's MASKED form);
//           at tile 1024 neither (SINGLE is always false there: the tile loop);
//   s2w     iff s2wave (stage 2 with lanes = candidates, icp_s2_wave_of);
//   grid    fused: (nb, batch); reference order: (2 * nwg, batch) — ks_dense_grid_x; KS_DENSE_THREADS = 512 threads per block.
struct ks_dense_form {
    uint32_t tile;
    bool single, masked, s2w;
};
static inline ks_dense_form ks_dense_select (uint32_t nr, uint32_t nrx, uint32_t s2wave)
{
    ks_dense_form f;
    f.tile = icp_dense_tile_rule (nr, nrx);
    f.single = f.tile == 256u && nr <= 256u;
    f.masked = f.tile == 256u && nr > 256u;
    f.s2w = s2wave != 0u;
    return f;
}
#define KS_DENSE_THREADS 512u
static inline uint32_t ks_dense_grid_x (bool fused, uint32_t nb, uint32_t nwg) { return fused ? nb : 2u * nwg; }
