// Exercises the ensemble noise of include/grayscott_hip.hpp over the C ABI: Ensemble::set_noise / noise / clear_noise.
// Usage: ensemble_noise_mirror MEMBERS ROWS COLS STEPS OUT.bin
// MEMBERS seeded members with the default parameters: member i gets sigmas (0.01 (i + 1), 0.005 i), seed 100 + i and
// starting step 7 i; member 0 is then overwritten through the one-struct form.  All run STEPS steps.  Writes the structs
// read back (gs_noise, 24 bytes each), then the U and the V planes of all members (f32).
// Built and run by tests/test_cpp_ensemble_noise_mirror.py (without a GPU: fails loudly).
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
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        if (!many.noise().empty()) return 3; // nothing attached yet
        std::vector<gs_noise> noise(members);
        for (std::size_t i = 0; i < members; ++i) noise[i] = gs_noise{0.01f * (float)(i + 1), 0.005f * (float)i, 100 + i, 7 * i};
        many.set_noise(noise);
        many.set_noise(gs_noise{0.02f, 0.0f, 5, 1}, 0, 1);
        bool threw = false;
        try {
            many.set_noise(gs_noise{-1.0f, 0.0f, 0, 0}, 0, members); // a negative sigma: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        many.perform_steps(steps);
        const std::vector<gs_noise> got = many.noise();
        const std::vector<float> u = many.download(0, members, 0), v = many.download(0, members, 1);
        many.clear_noise();
        if (!many.noise().empty()) return 6;
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 5;
        std::fwrite(got.data(), sizeof(gs_noise), got.size(), f);
        std::fwrite(u.data(), sizeof(float), u.size(), f);
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
