// Exercises the summaries of include/grayscott_hip.hpp: Species::summary() and Ensemble::summaries() over the C ABI.
// Usage: summary_mirror MEMBERS ROWS COLS STEPS OUT.bin
// Writes, as raw gs_summary-sized records: U and V of a lone Species after STEPS steps, then U and V of every ensemble
// member (all with the default parameters) after the same steps; then the lone Species' V plane (f32).
// Built and run by tests/test_summary_cpu.py (without a GPU: fails loudly) and tests/test_gpu_summary.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
void put(std::FILE *f, const gs::Summary &s)
{
    gs_summary c{s.sum, s.sum_sq, s.min, s.max, s.nonfinite};
    std::fwrite(&c, sizeof c, 1, f);
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
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const std::pair<gs::Summary, gs::Summary> uv = species.summary();
        if (uv.first.size != rows * cols || uv.first.cells() + uv.first.nonfinite != rows * cols) return 3;
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        const std::vector<gs::Summary> m = many.summaries(0, members);
        bool threw = false;
        try {
            many.summaries(members, 1); // outside the ensemble: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 5;
        put(f, uv.first);
        put(f, uv.second);
        for (const gs::Summary &s : m) put(f, s);
        const std::vector<float> v = species.make_result_view();
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
