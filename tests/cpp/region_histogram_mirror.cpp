// Exercises the regional histograms of include/grayscott_hip.hpp: Species::region_histogram() over the C ABI.
// Usage: region_histogram_mirror ROWS COLS RH RW STEPS BINS OUT.bin
// Writes, for a lone Species after STEPS steps: RR, RC and BINS (u64); the counters of U's regions over [0, 1], then of V's
// over [-0.125, 0.5] -- counts[BINS], below, above, nan and the region's cells (u64) per region; then the U and V planes (f32).
// Built and run by tests/test_region_histogram_cpu.py (without a GPU: fails loudly) and
// tests/test_gpu_region_histogram_mirror.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s rows cols rh rw steps bins out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const int32_t rh = (int32_t)std::strtol(argv[3], nullptr, 10), rw = (int32_t)std::strtol(argv[4], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[5], nullptr, 10);
    const int32_t bins = (int32_t)std::strtol(argv[6], nullptr, 10);
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const auto uv = species.region_histogram(rh, rw, bins, {0.0f, 1.0f}, {-0.125f, 0.5f});
        if (uv.first.results.size() != uv.first.rr * uv.first.rc || uv.second.results.size() != uv.first.results.size()) return 3;
        if (uv.second.at(0, 0).counts.size() != (std::size_t)bins || uv.second.at(0, 0).lo != -0.125f || uv.first.at(0, 0).hi != 1.0f)
            return 3;
        bool threw = false;
        try {
            species.region_histogram(rh, 18, bins); // no multiple of 4: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.region_histogram(rh, rw, 4097); // too many bins: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[7], "wb");
        if (!f) return 5;
        const uint64_t head[3] = {uv.first.rr, uv.first.rc, (uint64_t)bins};
        std::fwrite(head, sizeof(uint64_t), 3, f);
        for (const gs::RegionHistogram *h : {&uv.first, &uv.second})
            for (const gs::Histogram &x : h->results) {
                std::fwrite(x.counts.data(), sizeof(uint64_t), x.counts.size(), f);
                const uint64_t tail[4] = {x.below, x.above, x.nan, x.size};
                std::fwrite(tail, sizeof(uint64_t), 4, f);
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
