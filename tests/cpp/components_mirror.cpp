// Exercises the connected components of include/grayscott_hip.hpp: Species::components() and Ensemble::components() over the
// C ABI.
// Usage: components_mirror MEMBERS ROWS COLS STEPS OUT.bin
// Writes, as 35 u64 counters each (components, set_cells, largest, by_size[32]): U (set below 0.5 and 0.8) and V (set above
// 0.25 and 0.1) of a lone Species after STEPS steps under connectivity 8 -- U's two thresholds, then V's --, the same four
// under connectivity 4, then the four of every ensemble member (all with the default parameters, connectivity 8) after the
// same steps; then the lone Species' U and V planes (f32).
// Built and run by tests/test_components_cpu.py (without a GPU: fails loudly) and tests/test_gpu_components.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
void put(std::FILE *f, const gs::Components &c)
{
    const uint64_t head[3] = {c.count, c.set_cells, c.largest};
    std::fwrite(head, sizeof(uint64_t), 3, f);
    std::fwrite(c.by_size.data(), sizeof(uint64_t), 32, f);
}
} // namespace

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
        const auto eight = species.components(tv, tu), four = species.components(tv, tu, 4);
        if (eight.first.size() != 2 || eight.second.size() != 2 || four.second[1].connectivity != 4 || !eight.second[0].above ||
            eight.first[0].above)
            return 3;
        const auto morph = species.morphology(tv, tu);
        for (std::size_t k = 0; k < 2; ++k)
            if (eight.second[k].set_cells != morph.second[k].area() || eight.second[k].holes(morph.second[k]) < 0 ||
                four.first[k].holes(morph.first[k]) < 0)
                return 7;
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        const std::vector<gs::Components> m = many.components(0, members, tv, tu);
        if (m.size() != 4 * members) return 3;
        bool threw = false;
        try {
            many.components(members, 1, tv, tu); // outside the ensemble: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.components(tv, tu, 6); // neither 4 nor 8: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        threw = false;
        try {
            eight.second[0].holes(morph.second[1]); // a Morphology of another threshold: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 8;
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 5;
        for (const auto *uv : {&eight, &four}) {
            for (const gs::Components &x : uv->first) put(f, x);
            for (const gs::Components &x : uv->second) put(f, x);
        }
        for (const gs::Components &x : m) put(f, x);
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
