// Exercises the regional observables of include/grayscott_hip.hpp: Species::region_summaries() and
// Species::region_morphology() over the C ABI.
// Usage: regions_mirror ROWS COLS RH RW STEPS OUT.bin
// Writes, for a lone Species after STEPS steps: RR and RC (u64); the summaries of U's regions, then of V's, as gs_summary
// records (32 bytes) with every region's cell count behind each plane's records (u64); the bit-quad counts (six u64: Q0, Q1,
// Q2, Q3, Q4, QD) of U's regions set below 0.5, then below 0.8, then of V's set above 0.25, then above 0.1; then the U and V
// planes (f32).
// Built and run by tests/test_regions_cpu.py (without a GPU: fails loudly) and tests/test_gpu_regions_mirror.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s rows cols rh rw steps out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const int32_t rh = (int32_t)std::strtol(argv[3], nullptr, 10), rw = (int32_t)std::strtol(argv[4], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[5], nullptr, 10);
    const std::vector<float> tv = {0.25f, 0.1f}, tu = {0.5f, 0.8f};
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const auto sums = species.region_summaries(rh, rw);
        const auto quads = species.region_morphology(rh, rw, tv, tu);
        if (quads.first.size() != 2 || quads.second.size() != 2 || sums.first.results.size() != sums.first.rr * sums.first.rc) return 3;
        if (quads.second[1].rr != sums.second.rr || quads.second[1].rc != sums.second.rc || !quads.second[0].at(0, 0).above || quads.first[0].at(0, 0).above)
            return 3;
        bool threw = false;
        try {
            species.region_summaries(rh, 18); // no multiple of 4: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.region_morphology(0, rw, tv, tu); // no rows: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 5;
        const uint64_t grid[2] = {sums.first.rr, sums.first.rc};
        std::fwrite(grid, sizeof(uint64_t), 2, f);
        for (const gs::RegionSummaries *s : {&sums.first, &sums.second}) {
            for (const gs::Summary &x : s->results) {
                const gs_summary c{x.sum, x.sum_sq, x.min, x.max, x.nonfinite};
                std::fwrite(&c, sizeof c, 1, f);
            }
            for (const gs::Summary &x : s->results) std::fwrite(&x.size, sizeof(uint64_t), 1, f);
        }
        for (const auto *list : {&quads.first, &quads.second})
            for (const gs::RegionMorphology &m : *list)
                for (const gs::Morphology &x : m.results) std::fwrite(x.quads.data(), sizeof(uint64_t), 6, f);
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
