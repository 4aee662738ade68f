// pyramid_facade_test.cpp — cl_algo::ICP::ICPPyramid<CR, CW> (include/ICP/algorithms.hpp) against the C-ABI it wraps: the 10 degree
// synthetic pair registered through the facade and through icp_pyramid_* directly must give the same counts and the same bits, level 0
// must converge near the ground truth, and runFixed must leave every level's count.  Prints "pyramid facade ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <ICP/algorithms.hpp>

using namespace cl_algo::ICP;

#define REQUIRE(c) do { if (!(c)) { std::fprintf (stderr, "pyramid_facade_test: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main ()
{
    const uint32_t side = 128, m = side * side;
    std::vector<float> F (m * 8), M (m * 8);
    float T_true[8];
    const float axis[3] = { 0.3f, 0.9f, 0.1f }, t3[3] = { 25.f, -10.f, 15.f };
    REQUIRE (icp_synth_pair_scene (0x1C9D5EEDull, side, 0, 10.f, axis, t3, 1.0f, 0.01f, F.data (), M.data (), T_true) == ICP_OK);
    const std::vector<uint32_t> nr = { 256, 64, 64 };
    try
    {
        ICPPyramid<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> pyr { icp::Env (0) };
        pyr.init (m, nr, 2e2f, 1e-6f);
        REQUIRE (pyr.levels () == 3);
        int kind = -1; float dz = -1.f;
        pyr.getReduction (kind, dz);
        REQUIRE (kind == ICP_PYRAMID_MEAN && dz == 0.f);
        pyr.write (ICP_MEM_F, F.data ());
        pyr.write (ICP_MEM_M, M.data ());
        pyr.buildRBC ();
        pyr.run ();

        icp_pyramid_handle p = nullptr;
        const uint32_t its[3] = { 40, 40, 40 };
        uint32_t k[3] = { 0, 0, 0 };
        REQUIRE (icp_pyramid_create (&p, 0, ICP_ROT_POWER_METHOD, ICP_W_WEIGHTED) == ICP_OK);
        REQUIRE (icp_pyramid_init (p, 3, m, nr.data (), 2e2f, 1e-6f, its, 0.001, 0.01) == ICP_OK);
        REQUIRE (icp_pyramid_write (p, ICP_MEM_F, F.data (), 0) == ICP_OK && icp_pyramid_write (p, ICP_MEM_M, M.data (), 0) == ICP_OK);
        REQUIRE (icp_pyramid_build_rbc (p) == ICP_OK && icp_pyramid_run (p, k) == ICP_OK);
        icp_handle h0 = nullptr;
        REQUIRE (icp_pyramid_level (p, 0, &h0) == ICP_OK);
        icp_state_t st;
        REQUIRE (icp_state (h0, &st) == ICP_OK);
        for (int l = 0; l < 3; ++l) REQUIRE (pyr.k[l] == k[l]);
        REQUIRE (std::memcmp (pyr.q.c, st.q, 16) == 0 && std::memcmp (pyr.t.v, st.t, 12) == 0 && pyr.s == st.s && std::memcmp (pyr.R.m, st.R, 36) == 0);
        REQUIRE (icp_pyramid_destroy (p) == ICP_OK);

        const double dot = std::fabs ((double) pyr.q.c[0] * T_true[0] + (double) pyr.q.c[1] * T_true[1] + (double) pyr.q.c[2] * T_true[2] + (double) pyr.q.c[3] * T_true[3]);
        const double deg = 2.0 * std::acos (std::fmin (1.0, dot)) * 180.0 / M_PI;
        REQUIRE (st.converged && deg < 0.5);
        const icp_quality_t q = pyr.evaluate (20.f);
        REQUIRE (q.n == m && q.fitness > 0.5);

        pyr.resetTransform ();
        pyr.runFixed ({ 2, 3, 4 });
        pyr.sync ();
        pyr.pull ();
        REQUIRE (pyr.k[0] == 2 && pyr.k[1] == 3 && pyr.k[2] == 4);
        std::printf ("pyramid facade ok: k = %u %u %u, %.3f degrees from the ground truth, fitness %.4f\n", k[0], k[1], k[2], deg, q.fitness);
    }
    catch (const std::exception &e) { std::fprintf (stderr, "pyramid_facade_test: %s\n", e.what ()); return 1; }
    return 0;
}
