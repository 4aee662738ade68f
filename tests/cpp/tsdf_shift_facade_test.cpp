// tsdf_shift_facade_test.cpp — the moving volume through the C++ facade (include/ICP/algorithms.hpp: TSDFVolume::shift, window,
// extractSurfaceRegion, keptBox, shiftAndExtract) against the C-ABI it wraps (icp_tsdf_shift, icp_tsdf_get_window,
// icp_tsdf_extract_surface_region, icp_tsdf_kept_box) and the rule of include/icp_amd.h written out as host loops, bit for bit, on a
// written 16 x 14 x 12 volume: a tilted plane with colour and a few unseen voxels.  Prints "tsdf shift facade ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <ICP/algorithms.hpp>

using namespace cl_algo::ICP;

#define REQUIRE(c) do { if (!(c)) { std::fprintf (stderr, "tsdf_shift_facade_test: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {

const int N[3] = { 16, 14, 12 };
const float VOXEL = 2.f, BASE[3] = { -3.f, 5.f, 1.5f };

struct Host {
    std::vector<float> dw, rgb;
    float origin[3];
    static size_t at (int i, int j, int k) { return ((size_t) k * N[1] + j) * N[0] + i; }
    float D (size_t g) const { return dw[2 * g]; }
    float W (size_t g) const { return dw[2 * g + 1]; }
    bool usable (size_t g) const { return W (g) >= 1.f && std::fabs (D (g)) < 1.f; }
    // the shift's rule: contents as bit patterns, the origin from the cumulative shift
    Host shifted (const int32_t s[3], const int32_t c[3]) const
    {
        Host h;
        h.dw.assign (dw.size (), 0.f); h.rgb.assign (rgb.size (), 0.f);
        for (int a = 0; a < 3; ++a) { const float step = (float) c[a] * VOXEL; h.origin[a] = BASE[a] + step; }
        for (int k = 0; k < N[2]; ++k) for (int j = 0; j < N[1]; ++j) for (int i = 0; i < N[0]; ++i) {
            const int si = i + s[0], sj = j + s[1], sk = k + s[2];
            if (si < 0 || si >= N[0] || sj < 0 || sj >= N[1] || sk < 0 || sk >= N[2]) continue;
            std::memcpy (&h.dw[2 * at (i, j, k)], &dw[2 * at (si, sj, sk)], 8);
            std::memcpy (&h.rgb[3 * at (i, j, k)], &rgb[3 * at (si, sj, sk)], 12);
        }
        return h;
    }
    // the surface's rule without normals, with the box test: kind 0 INSIDE, 1 OUTSIDE, 2 every member
    void extract (const icp_tsdf_region_t *box, int kind, std::vector<float> &cloud) const
    {
        cloud.clear ();
        for (int k = 0; k < N[2]; ++k) for (int j = 0; j < N[1]; ++j) for (int i = 0; i < N[0]; ++i) for (int a = 0; a < 3; ++a) {
            const int idx[3] = { i, j, k };
            if (idx[a] + 1 >= N[a]) continue;
            const int hi[3] = { i + (a == 0), j + (a == 1), k + (a == 2) };
            const size_t g0 = at (i, j, k), g1 = at (hi[0], hi[1], hi[2]);
            const float D0 = D (g0), D1 = D (g1);
            if (!(usable (g0) && usable (g1) && (D0 > 0.f) != (D1 > 0.f))) continue;
            if (kind != 2) {
                bool in = true;
                for (int b = 0; b < 3; ++b) in = in && (uint32_t) idx[b] >= box->lo[b] && (uint32_t) idx[b] < box->hi[b] && (uint32_t) hi[b] < box->hi[b];
                if (in != (kind == 0)) continue;
            }
            const float t = D0 / (D0 - D1);
            for (int b = 0; b < 3; ++b) cloud.push_back (b == a ? origin[b] + ((float) idx[b] + t) * VOXEL : origin[b] + (float) idx[b] * VOXEL);
            cloud.push_back (1.f);
            for (int ch = 0; ch < 3; ++ch) cloud.push_back (rgb[3 * g0 + ch] + t * (rgb[3 * g1 + ch] - rgb[3 * g0 + ch]));
            cloud.push_back (1.f);
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
        cfg.nx = N[0]; cfg.ny = N[1]; cfg.nz = N[2]; cfg.voxel = VOXEL; std::memcpy (cfg.origin, BASE, sizeof BASE); cfg.mu = 8.f; cfg.w_max = 8.f; cfg.colour = 1;
        TSDFVolume vol (icp::Env (0), cfg);
        const size_t n = vol.voxels ();
        Host h;
        std::memcpy (h.origin, BASE, sizeof BASE);
        h.dw.resize (n * 2); h.rgb.resize (n * 3);
        for (int k = 0; k < N[2]; ++k) for (int j = 0; j < N[1]; ++j) for (int i = 0; i < N[0]; ++i) {
            const size_t g = Host::at (i, j, k);
            h.dw[2 * g] = std::fmax (-1.f, std::fmin (1.f, (6.3f + 0.11f * (float) i - 0.07f * (float) j - (float) k) / 4.f));
            h.dw[2 * g + 1] = 1.f;
            if ((i * 7 + j * 5 + k * 3) % 31 == 0) h.dw[2 * g + 1] = 0.f;             // a few unseen voxels
            h.rgb[3 * g] = (float) i / N[0]; h.rgb[3 * g + 1] = (float) j / N[1]; h.rgb[3 * g + 2] = (float) k / N[2];
        }
        vol.write (h.dw.data (), h.rgb.data ());
        std::vector<float> all;
        h.extract (nullptr, 2, all);
        REQUIRE (all.size () / 8 > 100);
        REQUIRE (vol.window () == (std::array<int32_t, 3> { 0, 0, 0 }));

        // keptBox against the C-ABI and the rule by hand; extractSurfaceRegion of both kinds against the host loop and the C-ABI
        const int32_t s1[3] = { 3, -2, 1 };
        const icp_tsdf_region_t box = TSDFVolume::keptBox (cfg, s1);
        icp_tsdf_region_t box_c;
        REQUIRE (icp_tsdf_kept_box (&cfg, s1, &box_c) == ICP_OK && std::memcmp (&box, &box_c, sizeof box) == 0);
        REQUIRE (box.lo[0] == 3 && box.hi[0] == 16 && box.lo[1] == 0 && box.hi[1] == 12 && box.lo[2] == 1 && box.hi[2] == 12 && box.mode == ICP_TSDF_REGION_OUTSIDE);
        std::vector<float> want_out, want_in, got, got_n, via_c;
        h.extract (&box, 1, want_out); h.extract (&box, 0, want_in);
        REQUIRE (want_out.size () / 8 > 20 && want_in.size () / 8 > 20 && want_out.size () + want_in.size () == all.size ());
        REQUIRE (vol.extractSurfaceRegion (box, got, &got_n) == want_out.size () / 8 && same (got, want_out) && got_n.size () == got.size () / 2);
        icp_tsdf_region_t inside = box;
        inside.mode = ICP_TSDF_REGION_INSIDE;
        REQUIRE (vol.extractSurfaceRegion (inside, got) == want_in.size () / 8 && same (got, want_in));
        uint32_t cnt = 0;
        const icp_tsdf_surface_t o = { 1.f, 0u };
        via_c.assign (want_out.size (), -7.f);
        REQUIRE (icp_tsdf_extract_surface_region (vol.handle (), &o, &box, (uint32_t) (want_out.size () / 8), via_c.data (), nullptr, &cnt) == ICP_OK);
        REQUIRE (cnt == want_out.size () / 8 && same (via_c, want_out));

        // shiftAndExtract: the leaving cloud, then the shifted volume, its window and origin, against the host loops and the C-ABI
        std::vector<float> leaving;
        REQUIRE (vol.shiftAndExtract (s1, leaving) == want_out.size () / 8 && same (leaving, want_out));
        int32_t c[3] = { 3, -2, 1 };
        Host h1 = h.shifted (s1, c);
        std::vector<float> dw2 (n * 2), rgb2 (n * 3), after, want_after;
        vol.read (dw2.data (), rgb2.data ());
        REQUIRE (same (dw2, h1.dw) && same (rgb2, h1.rgb));
        REQUIRE (vol.window () == (std::array<int32_t, 3> { 3, -2, 1 }));
        int32_t win[3];
        REQUIRE (icp_tsdf_get_window (vol.handle (), win) == ICP_OK && win[0] == 3 && win[1] == -2 && win[2] == 1);
        REQUIRE (std::memcmp (vol.config ().origin, h1.origin, 12) == 0 && h1.origin[0] == 3.f && h1.origin[1] == 1.f && h1.origin[2] == 3.5f);
        h1.extract (nullptr, 2, want_after);
        vol.extractSurface (after);
        REQUIRE (same (after, want_after) && after.size () == want_in.size ());       // nothing lost: what stayed is what was INSIDE

        // shift: a second one through the facade, a third through the C-ABI
        const int32_t s2[3] = { -5, 0, 0 }, s3[3] = { 0, 4, -3 };
        vol.shift (s2);
        c[0] += s2[0];
        Host h2 = h1.shifted (s2, c);
        REQUIRE (icp_tsdf_shift (vol.handle (), s3) == ICP_OK);
        for (int a = 0; a < 3; ++a) c[a] += s3[a];
        Host h3 = h2.shifted (s3, c);
        vol.read (dw2.data (), rgb2.data ());
        REQUIRE (same (dw2, h3.dw) && same (rgb2, h3.rgb) && std::memcmp (vol.config ().origin, h3.origin, 12) == 0);
        REQUIRE (vol.window () == (std::array<int32_t, 3> { -2, 2, -2 }));
        h3.extract (nullptr, 2, want_after);
        vol.extractSurface (after);
        REQUIRE (same (after, want_after) && !after.empty ());

        // a refusal throws and leaves the volume and its window
        bool thrown = false;
        const int32_t far[3] = { 1 << 24, 0, 0 };
        try { vol.shift (far); vol.shift (far); } catch (const std::runtime_error &) { thrown = true; }
        REQUIRE (thrown && vol.window () == (std::array<int32_t, 3> { (1 << 24) - 2, 2, -2 }));
        thrown = false;
        icp_tsdf_region_t bad = box;
        bad.hi[1] = 15;
        try { vol.extractSurfaceRegion (bad, got); } catch (const std::runtime_error &) { thrown = true; }
        REQUIRE (thrown);
        std::printf ("tsdf shift facade ok: %zu points, %zu left with the first shift, %zu after three\n", all.size () / 8, want_out.size () / 8, after.size () / 8);
    }
    catch (const std::exception &e) { std::fprintf (stderr, "tsdf_shift_facade_test: %s\n", e.what ()); return 1; }
    return 0;
}
