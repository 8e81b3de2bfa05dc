// Exercises the bundle statistics of include/grayscott_hip.hpp over the C ABI: Ensemble::bundle_stats.
// Usage: bundle_stats_mirror MEMBERS ROWS COLS SPAN STEPS OUT.bin
// MEMBERS seeded members with the default parameters and noise of their own (sigmas 0.02 / 0.01, seed 100 + i) run STEPS
// steps; every run of SPAN members is a bundle.  Writes the U and the V planes of all members (f32), then for each of mean,
// variance, min, max and occupancy (U below 0.5, V above 0.25) the U and the V planes of all bundles.
// Built and run by tests/test_cpp_bundle_stats_mirror.py (without a GPU: fails loudly).
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s members rows cols span steps out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t members = std::strtoull(argv[1], nullptr, 10);
    const std::size_t rows = std::strtoull(argv[2], nullptr, 10), cols = std::strtoull(argv[3], nullptr, 10);
    const std::size_t span = std::strtoull(argv[4], nullptr, 10), steps = std::strtoull(argv[5], nullptr, 10);
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        std::vector<gs_noise> noise(members);
        for (std::size_t i = 0; i < members; ++i) noise[i] = gs_noise{0.02f, 0.01f, 100 + i, 0};
        many.set_noise(noise);
        many.perform_steps(steps);
        bool threw = false;
        try {
            many.bundle_stats(span, {GS_TSTAT_ARRIVAL}); // no meaning across members: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        const std::vector<int32_t> which = {GS_TSTAT_MEAN, GS_TSTAT_VARIANCE, GS_TSTAT_MIN, GS_TSTAT_MAX, GS_TSTAT_OCCUPANCY};
        std::vector<gs::Ensemble> out = many.bundle_stats(span, which, {0.5f, 0.25f}, {0, 1});
        if (out.size() != which.size()) return 3;
        std::FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 5;
        for (int32_t species = 0; species < 2; ++species) {
            const std::vector<float> x = many.download(0, members, species);
            std::fwrite(x.data(), sizeof(float), x.size(), f);
        }
        for (const gs::Ensemble &e : out) {
            if (e.members() != members / span) return 6;
            for (int32_t species = 0; species < 2; ++species) {
                const std::vector<float> x = e.download(0, e.members(), species);
                std::fwrite(x.data(), sizeof(float), x.size(), f);
            }
        }
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
