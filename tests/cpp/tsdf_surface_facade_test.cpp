// tsdf_surface_facade_test.cpp — the surface of a TSDF volume through the C++ facade (include/ICP/algorithms.hpp:
// TSDFVolume::extractSurface) against the C-ABI it wraps (icp_tsdf_extract_surface) and the rule of include/icp_amd.h written out as a
// host loop, bit for bit, on a written 16 x 14 x 12 volume: a tilted plane with colour and a few unseen voxels.  Prints
// "tsdf surface facade ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <ICP/algorithms.hpp>

using namespace cl_algo::ICP;

#define REQUIRE(c) do { if (!(c)) { std::fprintf (stderr, "tsdf_surface_facade_test: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {

const uint32_t NX = 16, NY = 14, NZ = 12;
const float VOXEL = 2.f, ORIGIN[3] = { -3.f, 5.f, 1.5f };

struct Host {
    std::vector<float> dw, rgb;
    size_t at (uint32_t i, uint32_t j, uint32_t k) const { return ((size_t) k * NY + j) * NX + i; }
    float D (size_t g) const { return dw[2 * g]; }
    float W (size_t g) const { return dw[2 * g + 1]; }
    bool usable (size_t g, float min_weight) const { return W (g) >= min_weight && std::fabs (D (g)) < 1.f; }
    bool gradient (uint32_t i, uint32_t j, uint32_t k, float *G) const
    {
        if (!(i >= 1 && i + 1 < NX && j >= 1 && j + 1 < NY && k >= 1 && k + 1 < NZ)) return false;
        const size_t n[6] = { at (i + 1, j, k), at (i - 1, j, k), at (i, j + 1, k), at (i, j - 1, k), at (i, j, k + 1), at (i, j, k - 1) };
        for (int b = 0; b < 3; ++b) G[b] = D (n[2 * b]) - D (n[2 * b + 1]);
        for (size_t g : n) if (!(W (g) > 0.f)) return false;
        return true;
    }
    // the rule, in its order
    void extract (float min_weight, std::vector<float> &cloud, std::vector<float> &nrm) const
    {
        cloud.clear (); nrm.clear ();
        for (uint32_t k = 0; k < NZ; ++k) for (uint32_t j = 0; j < NY; ++j) for (uint32_t i = 0; i < NX; ++i) for (int a = 0; a < 3; ++a) {
            const uint32_t idx[3] = { i, j, k }, n[3] = { NX, NY, NZ };
            if (idx[a] + 1 >= n[a]) continue;
            const uint32_t hi[3] = { i + (a == 0), j + (a == 1), k + (a == 2) };
            const size_t g0 = at (i, j, k), g1 = at (hi[0], hi[1], hi[2]);
            const float D0 = D (g0), D1 = D (g1);
            if (!(usable (g0, min_weight) && usable (g1, min_weight) && (D0 > 0.f) != (D1 > 0.f))) continue;
            const float t = D0 / (D0 - D1);
            for (int b = 0; b < 3; ++b) cloud.push_back (b == a ? ORIGIN[b] + ((float) idx[b] + t) * VOXEL : ORIGIN[b] + (float) idx[b] * VOXEL);
            cloud.push_back (1.f);
            for (int ch = 0; ch < 3; ++ch) cloud.push_back (rgb[3 * g0 + ch] + t * (rgb[3 * g1 + ch] - rgb[3 * g0 + ch]));
            cloud.push_back (1.f);
            float G0[3], G1[3], out[4] = { 0.f, 0.f, 0.f, 0.f };
            const bool k0 = gradient (i, j, k, G0), k1 = gradient (hi[0], hi[1], hi[2], G1);
            if (k0 && k1) {
                float G[3];
                for (int b = 0; b < 3; ++b) G[b] = G0[b] + t * (G1[b] - G0[b]);
                const float len = std::sqrt ((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
                if (len > 0.f) for (int b = 0; b < 3; ++b) out[b] = G[b] / len;
            }
            nrm.insert (nrm.end (), out, out + 4);
        }
    }
};

bool same (const std::vector<float> &a, const std::vector<float> &b) { return a.size () == b.size () && (a.empty () || std::memcmp (a.data (), b.data (), a.size () * 4) == 0); }

}  // namespace

int main ()
{
    try
    {
        icp_tsdf_t cfg {};
        cfg.nx = NX; cfg.ny = NY; cfg.nz = NZ; cfg.voxel = VOXEL; std::memcpy (cfg.origin, ORIGIN, sizeof ORIGIN); cfg.mu = 8.f; cfg.w_max = 8.f; cfg.colour = 1;
        TSDFVolume vol (icp::Env (0), cfg);
        const size_t n = vol.voxels ();
        Host h;
        h.dw.resize (n * 2); h.rgb.resize (n * 3);
        for (uint32_t k = 0; k < NZ; ++k) for (uint32_t j = 0; j < NY; ++j) for (uint32_t i = 0; i < NX; ++i) {
            const size_t g = h.at (i, j, k);
            h.dw[2 * g] = std::fmax (-1.f, std::fmin (1.f, (6.3f + 0.11f * (float) i - 0.07f * (float) j - (float) k) / 4.f));
            h.dw[2 * g + 1] = (float) (1 + (i + 2 * j + 3 * k) % 3);                   // weights 1, 2, 3
            if ((i * 7 + j * 5 + k * 3) % 31 == 0) h.dw[2 * g + 1] = 0.f;             // a few unseen voxels
            h.rgb[3 * g] = (float) i / NX; h.rgb[3 * g + 1] = (float) j / NY; h.rgb[3 * g + 2] = (float) k / NZ;
        }
        vol.write (h.dw.data (), h.rgb.data ());
        size_t points[2] = { 0, 0 };
        for (int w = 0; w < 2; ++w) {
            const float min_weight = w ? 2.f : 1.f;
            std::vector<float> want, want_n, cloud, nrm, only;
            h.extract (min_weight, want, want_n);
            // the case is what it is meant to be: points on every axis' edges, normals present and absent
            size_t with_n = 0;
            for (size_t p = 0; p < want_n.size (); p += 4) with_n += want_n[p] != 0.f || want_n[p + 1] != 0.f || want_n[p + 2] != 0.f;
            REQUIRE (want.size () / 8 > 100 && with_n > 30 && with_n < want.size () / 8);
            // the facade
            const uint32_t got = vol.extractSurface (cloud, &nrm, min_weight);
            REQUIRE (got == want.size () / 8 && same (cloud, want) && same (nrm, want_n));
            REQUIRE (vol.extractSurface (only, nullptr, min_weight) == got && same (only, want));
            // the C-ABI: the counting call, then a capacity below the count
            const icp_tsdf_surface_t o = { min_weight, 1u };
            uint32_t cnt = 0;
            REQUIRE (icp_tsdf_extract_surface (vol.handle (), &o, 0, nullptr, nullptr, &cnt) == ICP_OK && cnt == got);
            const uint32_t cap = 50;
            REQUIRE (got > cap);
            std::vector<float> part (cap * 8 + 8, -7.f), part_n (cap * 4 + 4, -7.f);
            REQUIRE (icp_tsdf_extract_surface (vol.handle (), &o, cap, part.data (), part_n.data (), &cnt) == ICP_OK && cnt == got);
            REQUIRE (std::memcmp (part.data (), want.data (), cap * 32) == 0 && std::memcmp (part_n.data (), want_n.data (), cap * 16) == 0);
            for (uint32_t e = 0; e < 8; ++e) REQUIRE (part[cap * 8 + e] == -7.f);
            for (uint32_t e = 0; e < 4; ++e) REQUIRE (part_n[cap * 4 + e] == -7.f);
            points[w] = got;
        }
        REQUIRE (points[1] < points[0]);
        // the defaults of the C-ABI: min_weight 1, no normals
        {
            std::vector<float> want, want_n, cloud (points[0] * 8);
            h.extract (1.f, want, want_n);
            uint32_t cnt = 0;
            REQUIRE (icp_tsdf_extract_surface (vol.handle (), nullptr, (uint32_t) points[0], cloud.data (), nullptr, &cnt) == ICP_OK && cnt == points[0] && same (cloud, want));
        }
        // a refusal throws and the volume stays
        bool thrown = false;
        std::vector<float> cloud;
        try { vol.extractSurface (cloud, nullptr, 0.5f); } catch (const std::runtime_error &) { thrown = true; }
        REQUIRE (thrown);
        std::vector<float> dw2 (n * 2), rgb2 (n * 3);
        vol.read (dw2.data (), rgb2.data ());
        REQUIRE (same (dw2, h.dw) && same (rgb2, h.rgb));
        std::printf ("tsdf surface facade ok: %zu points, %zu at min_weight 2\n", points[0], points[1]);
    }
    catch (const std::exception &e) { std::fprintf (stderr, "tsdf_surface_facade_test: %s\n", e.what ()); return 1; }
    return 0;
}
