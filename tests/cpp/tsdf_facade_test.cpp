// tsdf_facade_test.cpp — the TSDF volume through the C++ facade (include/ICP/algorithms.hpp: TSDFVolume): write / read, a ray cast of a
// written plane against the plane itself, integrate against the rule written out on the host for the voxels on the optical axis,
// raycastTo against the lattice form read back through the handle, composePose, and a refusal.  Prints "tsdf facade ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <ICP/algorithms.hpp>

using namespace cl_algo::ICP;

#define REQUIRE(c) do { if (!(c)) { std::fprintf (stderr, "tsdf_facade_test: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main ()
{
    try
    {
        icp_tsdf_t cfg {};
        cfg.nx = 24; cfg.ny = 22; cfg.nz = 12; cfg.voxel = 1.f; cfg.origin[0] = cfg.origin[1] = cfg.origin[2] = 0.f; cfg.mu = 4.f; cfg.w_max = 8.f; cfg.colour = 1;
        TSDFVolume vol (icp::Env (0), cfg);
        REQUIRE (vol.config ().ny == 22 && vol.voxels () == 24u * 22u * 12u);
        const size_t n = vol.voxels ();
        // the plane z = 6.5 as a written volume, colour (0.25, 0.5, 0.75)
        std::vector<float> dw (n * 2), rgb (n * 3), dw2 (n * 2), rgb2 (n * 3);
        for (size_t i = 0; i < n; ++i) {
            const float k = (float) (i / (24u * 22u));
            dw[2 * i] = std::fmax (-1.f, std::fmin (1.f, (6.5f - k) / 4.f)); dw[2 * i + 1] = 1.f;
            rgb[3 * i] = 0.25f; rgb[3 * i + 1] = 0.5f; rgb[3 * i + 2] = 0.75f;
        }
        vol.write (dw.data (), rgb.data ());
        vol.read (dw2.data (), rgb2.data ());
        REQUIRE (std::memcmp (dw.data (), dw2.data (), n * 8) == 0 && std::memcmp (rgb.data (), rgb2.data (), n * 12) == 0);
        // a camera below the volume looking along +z: every ray that stays inside meets the plane at Z = 6.5 + 3
        icp_rgbd_t cam {};
        cam.width = 20; cam.height = 18; cam.fx = cam.fy = 40.f; cam.cx = 9.5f; cam.cy = 8.5f; cam.depth_scale = 1.f; cam.d_min = 1; cam.d_max = 65535;
        cam.x0 = 2; cam.y0 = 1; cam.step_x = 1; cam.step_y = 1; cam.radius = 0; cam.range = 30;
        const float pose[12] = { 1, 0, 0, 11.5f,  0, 1, 0, 10.5f,  0, 0, 1, -3.f };
        std::vector<float> cloud (20 * 18 * 8), nrm (20 * 18 * 4);
        vol.raycast (cam, pose, 1.f, 14.f, cloud.data (), nrm.data ());
        size_t hits = 0;
        for (int p = 0; p < 20 * 18; ++p) {
            const float *c = &cloud[(size_t) p * 8], *q = &nrm[(size_t) p * 4];
            REQUIRE (c[3] == 1.f && c[7] == 1.f && q[3] == 0.f);
            if (c[2] == 0.f) continue;
            ++hits;
            REQUIRE (std::fabs (c[2] - 9.5f) < 1e-4f && std::fabs (c[4] - 0.25f) < 1e-6f && std::fabs (c[5] - 0.5f) < 1e-6f && std::fabs (c[6] - 0.75f) < 1e-6f);
            REQUIRE (std::fabs (q[0]) < 1e-5f && std::fabs (q[1]) < 1e-5f && std::fabs (q[2] + 1.f) < 1e-5f);      // toward the camera
        }
        REQUIRE (hits == 20 * 18);
        // the same view as landmarks of a handle: raycastTo leaves what raycast (side) returns
        ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> a { icp::Env (0) };
        a.init (256, 4, 2e2f, 1e-6f);
        a.setRGBD (cam);
        std::vector<float> lm (256 * 8), ln (256 * 4), got (256 * 8), gotn (256 * 4);
        vol.raycast (cam, pose, 1.f, 14.f, lm.data (), ln.data (), 16);
        vol.raycastTo (a.handle (), ICP_MEM_F, pose, 1.f, 14.f, true);
        REQUIRE (icp_read (a.handle (), ICP_MEM_F, got.data (), got.size () * 4) == ICP_OK && icp_read (a.handle (), ICP_MEM_NORMALS_F, gotn.data (), gotn.size () * 4) == ICP_OK);
        REQUIRE (std::memcmp (lm.data (), got.data (), got.size () * 4) == 0 && std::memcmp (ln.data (), gotn.data (), gotn.size () * 4) == 0);
        for (int j = 0; j < 16; ++j) for (int i = 0; i < 16; ++i)
            REQUIRE (std::memcmp (&lm[(size_t) (j * 16 + i) * 8], &cloud[(size_t) ((1 + j) * 20 + 2 + i) * 8], 32) == 0);
        // a refusal: more than 4096 samples; the volume stays
        bool thrown = false;
        try { vol.raycast (cam, pose, 1.f, 1.f + 2.f * 4096.f, cloud.data ()); } catch (const std::runtime_error &) { thrown = true; }
        REQUIRE (thrown);
        vol.read (dw2.data (), rgb2.data ());
        REQUIRE (std::memcmp (dw.data (), dw2.data (), n * 8) == 0);
        // integrate: a constant depth image of 10 counts from the same pose; the voxels on the optical axis by hand
        vol.reset ();
        vol.read (dw2.data (), rgb2.data ());
        for (size_t i = 0; i < 2 * n; ++i) REQUIRE (dw2[i] == 0.f);
        const float pose_axis[12] = { 1, 0, 0, 11.f,  0, 1, 0, 10.f,  0, 0, 1, -3.f };
        std::vector<uint16_t> depth (20 * 18, 10);
        std::vector<uint8_t> colour (20 * 18 * 3, 51);
        vol.integrate (cam, pose_axis, depth.data (), colour.data ());
        vol.integrate (cam, pose_axis, depth.data ());
        vol.read (dw2.data (), rgb2.data ());
        for (uint32_t k = 0; k < 12; ++k) {
            const size_t at = ((size_t) k * 22 + 10) * 24 + 11;
            const float s = 10.f - ((float) k + 3.f), e = std::fmin (1.f, s / 4.f);
            if (s >= -4.f) { REQUIRE (dw2[2 * at] == (e * 1.f + e) / 2.f && dw2[2 * at + 1] == 2.f && rgb2[3 * at] == 51.f / 255.f); }
            else REQUIRE (dw2[2 * at] == 0.f && dw2[2 * at + 1] == 0.f && rgb2[3 * at] == 0.f);
        }
        // composePose
        const float T8[8] = { 0, 0, 0, 2.f, 1.f, 2.f, 3.f, 1.25f };
        float out[12];
        REQUIRE (TSDFVolume::composePose (pose, T8, out) == 1.25f);
        REQUIRE (out[0] == 1.f && out[5] == 1.f && out[10] == 1.f && out[3] == 12.5f && out[7] == 12.5f && out[11] == 0.f && out[1] == 0.f);
        std::printf ("tsdf facade ok: %zu hits\n", hits);
    }
    catch (const std::exception &e) { std::fprintf (stderr, "tsdf_facade_test: %s\n", e.what ()); return 1; }
    return 0;
}
