// Exercises the noise term of include/grayscott_hip.hpp: Simulation::set_noise(), noise() and clear_noise() over the C ABI.
// Usage: noise_mirror ROWS COLS STEPS SIGMA_U SIGMA_V SEED STEP OUT.bin
// A lone Species (Species::new's pattern) under the noise term for STEPS steps -- a gs_run of STEPS - 1, then a gs_step --;
// writes the step counter afterwards (u64), then the U and V planes (f32).
// Built and run by tests/test_gpu_noise_mirror.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>

int main(int argc, char **argv)
{
    if (argc != 9) {
        std::fprintf(stderr, "usage: %s rows cols steps sigma_u sigma_v seed step out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[3], nullptr, 10);
    const float su = std::strtof(argv[4], nullptr), sv = std::strtof(argv[5], nullptr);
    const uint64_t seed = std::strtoull(argv[6], nullptr, 10), step = std::strtoull(argv[7], nullptr, 10);
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        gs_noise n{};
        if (sim.noise(&n)) return 3; // nothing attached yet
        bool threw = false;
        try {
            sim.set_noise(std::numeric_limits<float>::quiet_NaN()); // must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw || sim.noise(&n)) return 4;
        sim.set_noise(su, sv, seed, step);
        if (!sim.noise(&n) || n.sigma_u != su || n.sigma_v != sv || n.seed != seed || n.step != step) return 5;
        if (steps > 1) sim.perform_steps(species, steps - 1);
        if (steps > 0) sim.perform_step(species);
        if (!sim.noise(&n) || n.step != step + steps) return 6;
        const uint64_t after = n.step;
        sim.clear_noise();
        if (sim.noise(&n)) return 7;
        std::FILE *f = std::fopen(argv[8], "wb");
        if (!f) return 8;
        std::fwrite(&after, sizeof after, 1, f);
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
