// Exercises TimeStats of include/grayscott_hip.hpp: Species::new's pattern, BEFORE steps, then SAMPLES samples EVERY steps
// apart, stamped with the step count, with every group selected and V thresholded at 0.25 from above, U at 0.5 from below;
// then the same over an ensemble of three members with their own feed rates.
// Usage: time_stats_mirror ROWS COLS BEFORE EVERY SAMPLES OUT.bin
//   writes, for the Species: V's six result planes (mean, variance, min, max, occupancy, arrival; f32), U's mean, V's raw sum
//   (f64) and first_stamp (u32), the sample count (u64); for the ensemble: V's mean, variance, max and arrival and U's
//   occupancy, each [3, rows, cols] f32.
// Built and run by tests/test_cpp_time_stats_mirror.py; plain g++, links libgs_hip.so.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

template <typename T>
static void put(std::FILE *f, const std::vector<T> &v)
{
    std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s rows cols before every samples out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const std::size_t before = std::strtoull(argv[3], nullptr, 10), every = std::strtoull(argv[4], nullptr, 10);
    const std::size_t samples = std::strtoull(argv[5], nullptr, 10);
    const uint32_t all = GS_TSTAT_SUM | GS_TSTAT_SQUARES | GS_TSTAT_EXTREMES | GS_TSTAT_CROSSINGS;
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        std::FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 4;
        {
            gs::Species species = sim.make_species({rows, cols});
            gs::TimeStats stats(species, all, {0.5f, 0.25f}, {0, 1});
            sim.perform_steps(species, before);
            for (std::size_t k = 0; k < samples; ++k) {
                if (k) sim.perform_steps(species, every);
                stats.accumulate((uint32_t)(before + k * every));
            }
            gs::Context ctx = species.context();
            for (int which = GS_TSTAT_MEAN; which <= GS_TSTAT_ARRIVAL; ++which) put(f, stats.result(1, which).make_scalar_view(ctx));
            put(f, stats.mean(0).make_scalar_view(ctx));
            put(f, stats.raw<double>(1, GS_TSTAT_RAW_SUM));
            put(f, stats.raw<uint32_t>(1, GS_TSTAT_RAW_FIRST_STAMP));
            const uint64_t n = stats.samples();
            std::fwrite(&n, sizeof n, 1, f);
        }
        {
            std::vector<gs::Parameters> params(3);
            for (std::size_t i = 0; i < params.size(); ++i) params[i].feed_rate = 0.014f + 0.004f * (float)i;
            gs::Ensemble ens = sim.make_ensemble({rows, cols}, params);
            gs::TimeStats stats(ens, all, {0.5f, 0.25f}, {0, 1});
            ens.perform_steps(before);
            for (std::size_t k = 0; k < samples; ++k) {
                if (k) ens.perform_steps(every);
                stats.accumulate((uint32_t)(before + k * every));
            }
            for (int which : {GS_TSTAT_MEAN, GS_TSTAT_VARIANCE, GS_TSTAT_MAX, GS_TSTAT_ARRIVAL}) put(f, stats.members_result(1, which));
            put(f, stats.members_result(0, GS_TSTAT_OCCUPANCY));
        }
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
