// Exercises the regional two-point correlations of include/grayscott_hip.hpp: Species::region_correlation() over the C ABI.
// Usage: region_correlation_mirror ROWS COLS RH RW STEPS MAX_LAG OUT.bin
// Writes, for a lone Species after STEPS steps: RR, RC and MAX_LAG (u64); the pair counts ([4][MAX_LAG + 1] u64) of U's
// regions set below 0.5, then below 0.8, then of V's set above 0.25, then above 0.1, each with the region's rows and cols
// (u64) behind its counts; then the U and V planes (f32).
// Built and run by tests/test_region_correlation_cpu.py (without a GPU: fails loudly) and
// tests/test_gpu_region_correlation_mirror.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s rows cols rh rw steps max_lag out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const int32_t rh = (int32_t)std::strtol(argv[3], nullptr, 10), rw = (int32_t)std::strtol(argv[4], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[5], nullptr, 10);
    const int32_t max_lag = (int32_t)std::strtol(argv[6], nullptr, 10);
    const std::vector<float> tv = {0.25f, 0.1f}, tu = {0.5f, 0.8f};
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const auto pairs = species.region_correlation(rh, rw, tv, tu, max_lag);
        if (pairs.first.size() != 2 || pairs.second.size() != 2 || pairs.second[0].results.size() != pairs.second[0].rr * pairs.second[0].rc)
            return 3;
        if (!pairs.second[0].at(0, 0).above || pairs.first[0].at(0, 0).above || pairs.second[1].at(0, 0).max_lag() != max_lag) return 3;
        bool threw = false;
        try {
            species.region_correlation(rh, 18, tv, tu, max_lag); // no multiple of 4: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.region_correlation(rh, rw, tv, tu, 65); // too large a lag: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[7], "wb");
        if (!f) return 5;
        const uint64_t head[3] = {pairs.second[0].rr, pairs.second[0].rc, (uint64_t)max_lag};
        std::fwrite(head, sizeof(uint64_t), 3, f);
        for (const auto *list : {&pairs.first, &pairs.second})
            for (const gs::RegionCorrelation &c : *list)
                for (const gs::Correlation &x : c.results) {
                    for (std::size_t k = 0; k < 4; ++k) std::fwrite(x.pairs[k].data(), sizeof(uint64_t), x.pairs[k].size(), f);
                    const uint64_t shape[2] = {x.rows, x.cols};
                    std::fwrite(shape, sizeof(uint64_t), 2, f);
                }
        const std::vector<float> u = species.u().in().make_scalar_view(species.context());
        std::fwrite(u.data(), sizeof(float), u.size(), f);
        const std::vector<float> v = species.make_result_view();
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
