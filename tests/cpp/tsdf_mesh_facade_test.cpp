// tsdf_mesh_facade_test.cpp — the mesh of a TSDF volume through the C++ facade (include/ICP/algorithms.hpp: TSDFVolume::extractMesh)
// against the C-ABI it wraps (icp_tsdf_extract_mesh, icp_tsdf_mesh_case) and the rule of include/icp_amd.h written out as a host loop over
// cells, on a written 16 x 14 x 12 volume: a tilted plane with a few unseen voxels.  The vertices are extractSurface's.  Prints
// "tsdf mesh facade ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <ICP/algorithms.hpp>

using namespace cl_algo::ICP;

#define REQUIRE(c) do { if (!(c)) { std::fprintf (stderr, "tsdf_mesh_facade_test: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {

const uint32_t NX = 16, NY = 14, NZ = 12;

struct Host {
    std::vector<float> dw;
    size_t at (uint32_t i, uint32_t j, uint32_t k) const { return ((size_t) k * NY + j) * NX + i; }
    bool usable (size_t g, float min_weight) const { return dw[2 * g + 1] >= min_weight && std::fabs (dw[2 * g]) < 1.f; }
    bool positive (size_t g) const { return dw[2 * g] > 0.f; }
    // the rule: the position of every member in its order, then the cells in theirs
    void mesh (float min_weight, uint32_t *n_members, std::vector<uint32_t> &tri) const
    {
        std::vector<int64_t> pos (3 * (size_t) NX * NY * NZ, -1);
        uint32_t n = 0;
        for (uint32_t k = 0; k < NZ; ++k) for (uint32_t j = 0; j < NY; ++j) for (uint32_t i = 0; i < NX; ++i) for (int a = 0; a < 3; ++a) {
            const uint32_t idx[3] = { i, j, k }, dim[3] = { NX, NY, NZ };
            if (idx[a] + 1 >= dim[a]) continue;
            const size_t g0 = at (i, j, k), g1 = at (i + (a == 0), j + (a == 1), k + (a == 2));
            if (usable (g0, min_weight) && usable (g1, min_weight) && positive (g0) != positive (g1)) pos[3 * g0 + a] = n++;
        }
        *n_members = n;
        tri.clear ();
        for (uint32_t k = 0; k + 1 < NZ; ++k) for (uint32_t j = 0; j + 1 < NY; ++j) for (uint32_t i = 0; i + 1 < NX; ++i) {
            bool active = true;
            uint32_t cs = 0;
            for (uint32_t c = 0; c < 8; ++c) {
                const size_t g = at (i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));
                active = active && usable (g, min_weight);
                cs |= (uint32_t) positive (g) << c;
            }
            if (!active) continue;
            uint32_t n_tri = 0;
            uint8_t edges[15];
            if (icp_tsdf_mesh_case (cs, &n_tri, edges) != ICP_OK) { tri.assign (1, 0xFFFFFFFFu); return; }
            for (uint32_t e = 0; e < 3 * n_tri; ++e) {
                const int a = edges[e] >> 2, m = edges[e] & 3, b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
                uint32_t v[3] = { i, j, k };
                v[b1] += m & 1; v[b2] += m >> 1;
                tri.push_back ((uint32_t) pos[3 * at (v[0], v[1], v[2]) + a]);          // (-1, were the edge no member, shows as 0xFFFFFFFF)
            }
        }
    }
};

}  // namespace

int main ()
{
    try
    {
        icp_tsdf_t cfg {};
        cfg.nx = NX; cfg.ny = NY; cfg.nz = NZ; cfg.voxel = 2.f; cfg.origin[0] = -3.f; cfg.origin[1] = 5.f; cfg.origin[2] = 1.5f; cfg.mu = 8.f; cfg.w_max = 8.f; cfg.colour = 0;
        TSDFVolume vol (icp::Env (0), cfg);
        const size_t n = vol.voxels ();
        Host h;
        h.dw.resize (n * 2);
        for (uint32_t k = 0; k < NZ; ++k) for (uint32_t j = 0; j < NY; ++j) for (uint32_t i = 0; i < NX; ++i) {
            const size_t g = h.at (i, j, k);
            h.dw[2 * g] = std::fmax (-1.f, std::fmin (1.f, (6.3f + 0.11f * (float) i - 0.07f * (float) j - (float) k) / 4.f));
            h.dw[2 * g + 1] = (float) (1 + (i / 4 + j / 4 + k / 4) % 3);                // weights 1, 2, 3 in blocks of 4^3: cells survive min_weight 2
            if ((i * 7 + j * 5 + k * 3) % 31 == 0) h.dw[2 * g + 1] = 0.f;             // a few unseen voxels
        }
        vol.write (h.dw.data ());
        size_t count[2] = { 0, 0 };
        for (int w = 0; w < 2; ++w) {
            const float min_weight = w ? 2.f : 1.f;
            std::vector<uint32_t> want, tri, tri2;
            std::vector<float> cloud, nrm, points, points_n, only;
            uint32_t members = 0;
            h.mesh (min_weight, &members, want);
            REQUIRE (want.size () / 3 > 50 && members > 80);
            for (uint32_t x : want) REQUIRE (x < members);
            // the facade, against the host loop and against extractSurface
            const uint32_t got = vol.extractMesh (cloud, tri, &nrm, min_weight);
            REQUIRE (got == want.size () / 3 && tri == want);
            REQUIRE (vol.extractSurface (points, &points_n, min_weight) == members && cloud.size () == points.size () && nrm.size () == points_n.size ());
            REQUIRE (std::memcmp (cloud.data (), points.data (), cloud.size () * 4) == 0 && std::memcmp (nrm.data (), points_n.data (), nrm.size () * 4) == 0);
            REQUIRE (vol.extractMesh (only, tri2, nullptr, min_weight) == got && tri2 == want && only.size () == cloud.size ());
            // the C-ABI: the counting call, then capacities below the counts
            const icp_tsdf_surface_t o = { min_weight, 0u };
            uint32_t nv = 0, nt = 0;
            REQUIRE (icp_tsdf_extract_mesh (vol.handle (), &o, 0, nullptr, nullptr, &nv, 0, nullptr, &nt) == ICP_OK && nv == members && nt == got);
            const uint32_t cap = 20;
            std::vector<uint32_t> part (cap * 3 + 3, 0xA5A5A5A5u);
            REQUIRE (icp_tsdf_extract_mesh (vol.handle (), &o, 0, nullptr, nullptr, &nv, cap, part.data (), &nt) == ICP_OK && nv == members && nt == got);
            REQUIRE (std::memcmp (part.data (), want.data (), cap * 12) == 0);
            for (uint32_t e = 0; e < 3; ++e) REQUIRE (part[cap * 3 + e] == 0xA5A5A5A5u);
            count[w] = got;
        }
        REQUIRE (count[1] < count[0]);
        // the table's refusal, and a refusal of the facade, which throws and leaves the volume
        uint32_t n_tri = 0;
        uint8_t edges[15];
        REQUIRE (icp_tsdf_mesh_case (256, &n_tri, edges) == ICP_EINVAL && icp_tsdf_mesh_case (255, &n_tri, edges) == ICP_OK && n_tri == 0);
        bool thrown = false;
        std::vector<float> cloud;
        std::vector<uint32_t> tri;
        try { vol.extractMesh (cloud, tri, nullptr, 0.5f); } catch (const std::runtime_error &) { thrown = true; }
        REQUIRE (thrown);
        std::vector<float> dw2 (n * 2);
        vol.read (dw2.data ());
        REQUIRE (std::memcmp (dw2.data (), h.dw.data (), n * 8) == 0);
        std::printf ("tsdf mesh facade ok: %zu triangles, %zu at min_weight 2\n", count[0], count[1]);
    }
    catch (const std::exception &e) { std::fprintf (stderr, "tsdf_mesh_facade_test: %s\n", e.what ()); return 1; }
    return 0;
}
