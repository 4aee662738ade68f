// tsdf_register_facade_test.cpp — a cloud registered against a TSDF volume through the C++ facade (include/ICP/algorithms.hpp:
// TSDFVolume::registerCloud, registerFrom) against the C-ABI it wraps (icp_tsdf_register, icp_tsdf_register_from), on a written 16^3 volume of
// three planes (a corner), where a shifted cloud must move back, and of one plane, which is singular.  Prints "tsdf register facade ok".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <ICP/algorithms.hpp>

using namespace cl_algo::ICP;

#define REQUIRE(c) do { if (!(c)) { std::fprintf (stderr, "tsdf_register_facade_test: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main () try
{
    const uint32_t N = 16;
    const float mu = 4.f;
    const icp_tsdf_t cfg = { N, N, N, 1.f, { 0.f, 0.f, 0.f }, mu, 64.f, 0u };
    TSDFVolume vol (icp::Env (0), cfg);
    // D = the distance to the nearest of the planes x = 4, y = 4, z = 4 (positive toward larger coordinates), over mu, clamped
    std::vector<float> corner (2 * (size_t) N * N * N), plane (corner.size ());
    for (uint32_t k = 0; k < N; ++k) for (uint32_t j = 0; j < N; ++j) for (uint32_t i = 0; i < N; ++i) {
        const size_t g = ((size_t) k * N + j) * N + i;
        const float d = std::min (std::min ((float) i - 4.f, (float) j - 4.f), (float) k - 4.f);
        corner[2 * g] = std::max (-1.f, std::min (1.f, d / mu)); corner[2 * g + 1] = 1.f;
        plane[2 * g] = std::max (-1.f, std::min (1.f, ((float) k - 4.f) / mu)); plane[2 * g + 1] = 1.f;
    }
    // points on the three planes, in a camera frame that is the world shifted by (0.4, -0.3, 0.5)
    std::vector<float> cloud;
    const float shift[3] = { 0.4f, -0.3f, 0.5f };
    for (int a = 0; a < 3; ++a) for (int u = 0; u < 8; ++u) for (int v = 0; v < 8; ++v) {
        float p[3];
        p[a] = 4.f; p[(a + 1) % 3] = 5.3f + (float) u; p[(a + 2) % 3] = 5.6f + (float) v;
        const float rec[8] = { p[0] - shift[0], p[1] - shift[1], p[2] - shift[2], 1.f, 0.f, 0.f, 0.f, 1.f };
        cloud.insert (cloud.end (), rec, rec + 8);
    }
    // (and 64 invalid points: 256 = 16 x 16 landmarks for the handle below)
    for (int i = 0; i < 64; ++i) { const float rec[8] = { 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f }; cloud.insert (cloud.end (), rec, rec + 8); }
    const uint32_t n = (uint32_t) (cloud.size () / 8);
    const float identity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    vol.write (corner.data ());
    const icp_tsdf_register_t opt = { 10u, 0.0, 0.0 };
    const icp_tsdf_registration_t got = vol.registerCloud (cloud.data (), n, identity, &opt);
    icp_tsdf_registration_t want;
    REQUIRE (icp_tsdf_register (vol.handle (), &opt, cloud.data (), n, identity, &want) == ICP_OK);
    REQUIRE (std::memcmp (&got, &want, sizeof got) == 0);
    REQUIRE (got.iterations == 10u && got.singular == 0u && got.converged == 0u && got.members > n / 2 && got.members <= 192u);
    for (int a = 0; a < 3; ++a) REQUIRE (std::fabs (got.pose12[4 * a + 3] - shift[a]) < 0.05f);
    // the defaults
    const icp_tsdf_registration_t dflt = vol.registerCloud (cloud.data (), n, identity);
    REQUIRE (dflt.iterations >= 1u && dflt.iterations <= 20u && dflt.singular == 0u);
    // from a handle: M holds the cloud
    ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> g { icp::Env (0) };
    g.init (n, 4, 2e2f, 1e-6f);
    std::vector<float> M (cloud);
    REQUIRE (icp_write (g.handle (), ICP_MEM_M, M.data (), 1) == ICP_OK);
    const icp_tsdf_registration_t from = vol.registerFrom (g.handle (), ICP_MEM_M, identity, &opt);
    REQUIRE (std::memcmp (&from, &want, sizeof from) == 0);
    bool threw = false;
    try { vol.registerFrom (g.handle (), ICP_MEM_T, identity, &opt); } catch (const std::runtime_error &) { threw = true; }
    REQUIRE (threw);
    // one plane: singular, the pose as it was
    vol.write (plane.data ());
    const icp_tsdf_registration_t one = vol.registerCloud (cloud.data (), n, identity, &opt);
    REQUIRE (one.singular == 1u && one.iterations == 0u && one.members > 0u && std::memcmp (one.pose12, identity, sizeof identity) == 0);
    std::printf ("tsdf register facade ok\n");
    return 0;
}
catch (const std::exception &e) { std::fprintf (stderr, "tsdf_register_facade_test: %s\n", e.what ()); return 1; }
