// Exercises the morphology of include/grayscott_hip.hpp: Species::morphology() and Ensemble::morphologies() over the C ABI.
// Usage: morphology_mirror MEMBERS ROWS COLS STEPS OUT.bin
// Writes, as six u64 counters each (Q0, Q1, Q2, Q3, Q4, QD): U (set below 0.5 and 0.8) and V (set above 0.25 and 0.1) of a
// lone Species after STEPS steps -- U's two thresholds, then V's --, then the same four of every ensemble member (all with
// the default parameters) after the same steps; then the lone Species' U and V planes (f32).
// Built and run by tests/test_morphology_cpu.py (without a GPU: fails loudly) and tests/test_gpu_morphology.py.
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
    const std::vector<float> tv = {0.25f, 0.1f}, tu = {0.5f, 0.8f};
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const auto uv = species.morphology(tv, tu);
        if (uv.first.size() != 2 || uv.second.size() != 2 || uv.second[0].cells != rows * cols) return 3;
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        const std::vector<gs::Morphology> m = many.morphologies(0, members, tv, tu);
        if (m.size() != 4 * members) return 3;
        bool threw = false;
        try {
            many.morphologies(members, 1, tv, tu); // outside the ensemble: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.morphology({0.1f, 0.2f, 0.3f, 0.4f, 0.5f}, {0.1f, 0.2f, 0.3f, 0.4f, 0.5f}); // five thresholds: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 5;
        for (const gs::Morphology &x : uv.first) std::fwrite(x.quads.data(), sizeof(uint64_t), 6, f);
        for (const gs::Morphology &x : uv.second) std::fwrite(x.quads.data(), sizeof(uint64_t), 6, f);
        for (const gs::Morphology &x : m) std::fwrite(x.quads.data(), sizeof(uint64_t), 6, f);
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
