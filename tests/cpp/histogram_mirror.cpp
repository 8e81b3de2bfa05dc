// Exercises the histograms of include/grayscott_hip.hpp: Species::histogram() and Ensemble::histograms() over the C ABI.
// Usage: histogram_mirror MEMBERS ROWS COLS STEPS BINS OUT.bin
// Writes, as BINS + 3 u64 counters each (counts, below, above, nan): U and V of a lone Species after STEPS steps (U over
// [0, 1], V over [0, 0.5]), then U and V of every ensemble member (all with the default parameters) after the same steps;
// then the lone Species' U and V planes (f32).
// Built and run by tests/test_histogram_cpu.py (without a GPU: fails loudly) and tests/test_gpu_histogram.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
void put(std::FILE *f, const gs::Histogram &h)
{
    std::fwrite(h.counts.data(), sizeof(uint64_t), h.counts.size(), f);
    const uint64_t tail[3] = {h.below, h.above, h.nan};
    std::fwrite(tail, sizeof(uint64_t), 3, f);
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s members rows cols steps bins out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t members = std::strtoull(argv[1], nullptr, 10);
    const std::size_t rows = std::strtoull(argv[2], nullptr, 10), cols = std::strtoull(argv[3], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[4], nullptr, 10);
    const int32_t bins = (int32_t)std::strtol(argv[5], nullptr, 10);
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const std::pair<gs::Histogram, gs::Histogram> uv = species.histogram(bins);
        if (uv.first.size != rows * cols || uv.first.in_range() + uv.first.below + uv.first.above + uv.first.nan != rows * cols)
            return 3;
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        const std::vector<gs::Histogram> m = many.histograms(0, members, bins);
        bool threw = false;
        try {
            many.histograms(members, 1, bins); // outside the ensemble: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.histogram(bins, {1.0f, 1.0f}); // an empty range: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 5;
        put(f, uv.first);
        put(f, uv.second);
        for (const gs::Histogram &h : m) put(f, h);
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
