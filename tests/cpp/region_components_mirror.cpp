// Exercises the regional connected components of include/grayscott_hip.hpp: Species::region_components() over the C ABI.
// Usage: region_components_mirror ROWS COLS RH RW STEPS CONNECTIVITY OUT.bin
// Writes, for a lone Species after STEPS steps: RR, RC and the number of thresholds (u64); per species (U below 0.5 and 0.9,
// then V above 0.25 and 0.1), threshold and region the 35 counters (u64) -- components, set_cells, largest, by_size[32]; then
// the U and V planes (f32).
// Built and run by tests/test_region_components_cpu.py (without a GPU: fails loudly) and
// tests/test_gpu_region_components_mirror.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s rows cols rh rw steps connectivity out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const int32_t rh = (int32_t)std::strtol(argv[3], nullptr, 10), rw = (int32_t)std::strtol(argv[4], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[5], nullptr, 10);
    const int32_t connectivity = (int32_t)std::strtol(argv[6], nullptr, 10);
    const std::vector<float> tv = {0.25f, 0.1f}, tu = {0.5f, 0.9f};
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const auto uv = species.region_components(rh, rw, tv, tu, true, false, connectivity);
        if (uv.first.size() != 2 || uv.second.size() != 2) return 3;
        for (const auto *list : {&uv.first, &uv.second})
            for (const gs::RegionComponents &c : *list)
                if (c.results.size() != c.rr * c.rc || c.rr != uv.second[0].rr || c.rc != uv.second[0].rc) return 3;
        if (uv.second[1].at(0, 0).threshold != 0.1f || !uv.second[1].at(0, 0).above || uv.first[0].at(0, 0).above ||
            uv.first[0].at(0, 0).connectivity != connectivity)
            return 3;
        bool threw = false;
        try {
            species.region_components(rh, 18, tv, tu); // no multiple of 4: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.region_components(rh, rw, tv, tu, true, false, 6); // neither 4 nor 8: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[7], "wb");
        if (!f) return 5;
        const uint64_t head[3] = {uv.second[0].rr, uv.second[0].rc, (uint64_t)tv.size()};
        std::fwrite(head, sizeof(uint64_t), 3, f);
        for (const auto *list : {&uv.first, &uv.second})
            for (const gs::RegionComponents &c : *list)
                for (const gs::Components &x : c.results) {
                    const uint64_t front[3] = {x.count, x.set_cells, x.largest};
                    std::fwrite(front, sizeof(uint64_t), 3, f);
                    std::fwrite(x.by_size.data(), sizeof(uint64_t), x.by_size.size(), f);
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
