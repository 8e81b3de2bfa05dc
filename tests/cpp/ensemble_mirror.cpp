// Exercises the Ensemble of include/grayscott_hip.hpp: a sweep of members with their own feed and kill rates, advanced
// together, plus one lone Species per member for comparison.
// Usage: ensemble_mirror MEMBERS ROWS COLS STEPS OUT.bin   (writes V of every member, then V of every lone Species)
// Built and run by tests/test_cpp_ensemble_mirror.py; plain g++, links libgs_hip.so.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s members rows cols steps out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t members = std::strtoull(argv[1], nullptr, 10);
    const std::size_t rows = std::strtoull(argv[2], nullptr, 10), cols = std::strtoull(argv[3], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[4], nullptr, 10);
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        std::vector<gs::Parameters> params(members);
        for (std::size_t i = 0; i < members; ++i) {
            params[i].feed_rate = 0.010f + 0.004f * (float)i;
            params[i].kill_rate = 0.050f + 0.002f * (float)(members - 1 - i);
        }
        gs::Ensemble ens = sim.make_ensemble({rows, cols}, params);
        const std::size_t half = steps / 2;
        ens.perform_steps(half);
        ens.prepare_steps(steps - half); // asynchronous; the download waits
        const std::vector<float> v = ens.download(0, members);
        bool threw = false;
        try {
            ens.download(members, 1); // outside the ensemble: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 3;
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 4;
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        for (std::size_t i = 0; i < members; ++i) {
            gs::Simulation solo = gs::Simulation::new_(params[i]);
            gs::Species species = solo.make_species({rows, cols});
            solo.perform_steps(species, steps);
            std::vector<float> sv(rows * cols);
            species.write_result_view(sv.data(), {rows, cols});
            std::fwrite(sv.data(), sizeof(float), sv.size(), f);
        }
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
