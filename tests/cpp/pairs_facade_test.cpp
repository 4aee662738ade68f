// pairs_facade_test.cpp — cl_algo::ICP::ICP<CR, CW>::correspondences () (include/ICP/algorithms.hpp) on a registration run through the
// facade: prints the transform the run ended with, and the count and a checksum of both sets, so that tests/test_gpu_pairs.py can
// compare them with its own call on the same data.
//     pairs_facade_test [side [nr [max_dist]]]
// The checksum is FNV-1a (64 bit) over the records' bytes in order.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <ICP/algorithms.hpp>

using namespace cl_algo::ICP;

static unsigned long long fnv1a (const std::vector<icp_pair_t> &v)
{
    unsigned long long h = 14695981039346656037ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *> (v.data ());
    for (size_t i = 0; i < v.size () * sizeof (icp_pair_t); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

int main (int argc, char **argv)
{
    const unsigned int side = argc > 1 ? (unsigned) atoi (argv[1]) : 64, r = argc > 2 ? (unsigned) atoi (argv[2]) : 64;
    const float max_dist = argc > 3 ? (float) atof (argv[3]) : 3.f;
    const unsigned int m = side * side;
    static_assert (sizeof (icp_pair_t) == 16, "icp_pair_t is 16 bytes");
    try
    {
        std::vector<float> F ((size_t) m * 8), M ((size_t) m * 8);
        const float axis[3] = { 0.3f, 0.9f, 0.1f }, t[3] = { 25.f, -10.f, 15.f };
        icp_synth_pair (0x1C9D5EEDull, side, 3.f, axis, t, 1.f, 0.01f, 0.f, F.data (), M.data ());
        ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> reg { icp::Env (0) };
        reg.init (m, r, 2e2f, 1e-6f, 40, 0.001, 0.01, Staging::IO);
        reg.write (decltype (reg)::Memory::D_IN_F, F.data ());
        reg.write (decltype (reg)::Memory::D_IN_M, M.data ());
        reg.buildRBC ();
        reg.run ();
        const std::vector<icp_pair_t> ev = reg.correspondences (ICP_PAIRS_EVALUATED, max_dist);
        const std::vector<icp_pair_t> last = reg.correspondences (ICP_PAIRS_LAST_ITERATION);
        const icp_quality_t q = reg.evaluate (max_dist);
        std::printf ("k %u\n", reg.k);
        std::printf ("EVALUATED %zu %016llx inliers %u\n", ev.size (), fnv1a (ev), q.n_inliers);
        std::printf ("LAST %zu %016llx\n", last.size (), fnv1a (last));
    }
    catch (const std::exception &e) { std::fprintf (stderr, "pairs_facade_test: %s\n", e.what ()); return 1; }
    return 0;
}
