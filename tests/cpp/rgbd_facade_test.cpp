// rgbd_facade_test.cpp — the RGB-D front end through the C++ facade (include/ICP/algorithms.hpp): RGBDTo8D against the rule written out
// on the host, ICPStep::setRGBD / getRGBD / writeRGBD against icp_write_cloud of that host-made cloud, ICPTrack::nextRGBD / submitRGBD
// against next () of the host-made clouds.  Everything bit for bit.  Prints "rgbd facade ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <ICP/algorithms.hpp>

using namespace cl_algo::ICP;

#define REQUIRE(c) do { if (!(c)) { std::fprintf (stderr, "rgbd_facade_test: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

namespace {
constexpr uint32_t W = 640, H = 480, N = W * H;

struct Frame { std::vector<uint16_t> depth; std::vector<uint8_t> rgb; std::vector<float> cloud; };

// a synthetic frame as a sensor delivers it, and the cloud a host makes of it with the reference's writer (the rule at its defaults)
bool make_frame (int moved, Frame &f)
{
    std::vector<float> c ((size_t) N * 8);
    if (icp_synth_cloud_vga (0x1C9D5EEDull, moved, c.data ()) != ICP_OK) return false;
    f.depth.resize (N); f.rgb.resize ((size_t) N * 3); f.cloud.resize ((size_t) N * 8);
    for (uint32_t i = 0; i < N; ++i) {
        f.depth[i] = (uint16_t) std::lrintf (c[(size_t) i * 8 + 2]);
        for (int k = 0; k < 3; ++k) f.rgb[(size_t) i * 3 + k] = (uint8_t) std::lrintf (c[(size_t) i * 8 + 4 + k] * 255.f);
        const uint32_t u = i % W, v = i / W;
        const float z = (float) f.depth[i] * 1.f;
        float *p = &f.cloud[(size_t) i * 8];
        const float xn = ((float) u - 319.5f) * z, yn = ((float) v - 239.5f) * z;
        p[0] = xn / 595.f; p[1] = yn / 595.f; p[2] = z; p[3] = 1.f;
        for (int k = 0; k < 3; ++k) p[4 + k] = (float) f.rgb[(size_t) i * 3 + k] / 255.f;
        p[7] = 1.f;
    }
    return true;
}
}  // namespace

int main ()
{
    Frame fr[3];
    for (int i = 0; i < 3; ++i) REQUIRE (make_frame (i, fr[i]));
    try
    {
        // the dense form
        RGBDTo8D to8d { icp::Env (0) };
        std::vector<float> cloud ((size_t) N * 8), nrm ((size_t) N * 4);
        to8d.run (fr[0].depth.data (), fr[0].rgb.data (), cloud.data ());
        REQUIRE (std::memcmp (cloud.data (), fr[0].cloud.data (), cloud.size () * 4) == 0);
        to8d.cfg.radius = 3;
        to8d.run (fr[0].depth.data (), nullptr, cloud.data (), nrm.data ());
        size_t with_normal = 0;
        for (uint32_t i = 0; i < N; ++i) {
            REQUIRE (cloud[(size_t) i * 8 + 4] == 0.f && cloud[(size_t) i * 8 + 7] == 1.f);
            const float *n = &nrm[(size_t) i * 4];
            const float len = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
            REQUIRE (len == 0.f || std::fabs (len - 1.f) < 1e-5f);
            with_normal += len != 0.f;
        }
        REQUIRE (with_normal > N / 2);
        to8d.cfg.radius = 7;
        bool thrown = false;
        try { to8d.run (fr[0].depth.data (), nullptr, cloud.data ()); } catch (const std::runtime_error &) { thrown = true; }
        REQUIRE (thrown);

        // the lattice form through ICPStep: the default configuration is icp_write_cloud of the host-made cloud
        ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> a { icp::Env (0) }, b { icp::Env (0) };
        a.init (16384, 256, 2e2f, 1e-6f); b.init (16384, 256, 2e2f, 1e-6f);
        icp_rgbd_t cfg = a.getRGBD ();
        REQUIRE (cfg.width == 640 && cfg.height == 480 && cfg.x0 == 65 && cfg.y0 == 49 && cfg.step_x == 4 && cfg.step_y == 3 && cfg.radius == 0 && cfg.range == 30);
        std::vector<float> la (16384 * 8), lb (16384 * 8);
        for (int which : { ICP_MEM_F, ICP_MEM_M }) {
            a.writeRGBD (which, fr[1].depth.data (), fr[1].rgb.data ());
            REQUIRE (icp_write_cloud (b.handle (), which, fr[1].cloud.data (), 1) == ICP_OK);
            REQUIRE (icp_read (a.handle (), which, la.data (), la.size () * 4) == ICP_OK && icp_read (b.handle (), which, lb.data (), lb.size () * 4) == ICP_OK);
            REQUIRE (std::memcmp (la.data (), lb.data (), la.size () * 4) == 0);
        }
        cfg.radius = 2; cfg.range = 40;
        a.setRGBD (cfg);
        REQUIRE (a.getRGBD ().radius == 2 && a.getRGBD ().range == 40);
        cfg.range = 0;
        thrown = false;
        try { a.setRGBD (cfg); } catch (const std::runtime_error &) { thrown = true; }
        REQUIRE (thrown && a.getRGBD ().range == 40);

        // tracking: frames as images against frames as host-made clouds, blocking and with two in flight
        ICPTrack<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> ti { icp::Env (0) }, tc { icp::Env (0) };
        ti.init (); tc.init ();
        unsigned int ks[3] = { 0, 0, 0 };
        for (int i = 0; i < 3; ++i) {
            const bool ri = ti.nextRGBD (fr[i].depth.data (), fr[i].rgb.data ()), rc = tc.next (fr[i].cloud.data ());
            REQUIRE (ri == rc && ri == (i > 0));
            if (ri) { REQUIRE (ti.k == tc.k && std::memcmp (ti.q.c, tc.q.c, 16) == 0 && std::memcmp (ti.t.v, tc.t.v, 12) == 0 && ti.s == tc.s); ks[i] = ti.k; }
        }
        ti.reset (); tc.reset ();
        ti.submitRGBD (fr[0].depth.data (), fr[0].rgb.data ()); ti.submitRGBD (fr[1].depth.data (), fr[1].rgb.data ());
        tc.submit (fr[0].cloud.data ()); tc.submit (fr[1].cloud.data ());
        REQUIRE (!ti.collect () && !tc.collect ());
        ti.submit (fr[2].cloud.data ()); tc.submit (fr[2].cloud.data ());          // (the two kinds of frame alternate)
        for (int i = 1; i < 3; ++i) {
            REQUIRE (ti.collect () && tc.collect ());
            REQUIRE (ti.k == tc.k && ti.k == ks[i] && std::memcmp (ti.q.c, tc.q.c, 16) == 0 && std::memcmp (ti.t.v, tc.t.v, 12) == 0);
        }
        std::printf ("rgbd facade ok: k = %u %u\n", ks[1], ks[2]);
    }
    catch (const std::exception &e) { std::fprintf (stderr, "rgbd_facade_test: %s\n", e.what ()); return 1; }
    return 0;
}
