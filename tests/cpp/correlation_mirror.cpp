// Exercises the correlations of include/grayscott_hip.hpp: Species::correlation() and Ensemble::correlations() over the C ABI.
// Usage: correlation_mirror MEMBERS ROWS COLS STEPS LAG OUT.bin
// Writes, as [4][LAG + 1] u64 counters each: U (set below 0.5 and 0.8) and V (set above 0.25 and 0.1) of a lone Species after
// STEPS steps -- U's two thresholds, then V's --, then the same four of every ensemble member (all with the default
// parameters) after the same steps; then the lone Species' U and V planes (f32).
// Built and run by tests/test_correlation_cpu.py (without a GPU: fails loudly) and tests/test_gpu_correlation.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s members rows cols steps lag out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t members = std::strtoull(argv[1], nullptr, 10);
    const std::size_t rows = std::strtoull(argv[2], nullptr, 10), cols = std::strtoull(argv[3], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[4], nullptr, 10);
    const int32_t lag = (int32_t)std::strtol(argv[5], nullptr, 10);
    const std::vector<float> tv = {0.25f, 0.1f}, tu = {0.5f, 0.8f};
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const auto uv = species.correlation(tv, tu, lag);
        if (uv.first.size() != 2 || uv.second.size() != 2 || uv.second[0].rows != rows || uv.second[0].max_lag() != lag) return 3;
        if (uv.second[0].pairs_total(2, 1) != (rows - 1) * (cols - 1) || uv.second[0].pairs_total(1, 1) != (rows - 1) * cols) return 3;
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        const std::vector<gs::Correlation> m = many.correlations(0, members, tv, tu, lag);
        if (m.size() != 4 * members) return 3;
        bool threw = false;
        try {
            many.correlations(members, 1, tv, tu, lag); // outside the ensemble: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.correlation(tv, tu, 65); // a lag beyond 64: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 5;
        auto put = [&](const gs::Correlation &x) {
            for (const auto &row : x.pairs) std::fwrite(row.data(), sizeof(uint64_t), row.size(), f);
        };
        for (const gs::Correlation &x : uv.first) put(x);
        for (const gs::Correlation &x : uv.second) put(x);
        for (const gs::Correlation &x : m) put(x);
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
