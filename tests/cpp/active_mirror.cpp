// Exercises the active sets of include/grayscott_hip.hpp over the C ABI: Ensemble::set_active / active / steps_taken.
// Usage: active_mirror MEMBERS ROWS COLS STEPS OUT.bin
// MEMBERS (>= 2) seeded members with the default parameters run STEPS steps, the odd ones are retired, all run STEPS + 1
// steps twice.  Writes the V planes of all members (f32), then their step counts (u64) and their flags (u8).
// Built and run by tests/test_active_cpu.py (without a GPU: fails loudly) and tests/test_gpu_active.py.
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
        many.perform_steps(steps);
        std::vector<uint8_t> mask(members, 1);
        for (std::size_t i = 1; i < members; i += 2) mask[i] = 0;
        many.set_active(mask);
        many.perform_steps(steps + 1);
        many.perform_steps(steps + 1);
        bool threw = false;
        try {
            many.set_active(mask, 1); // reaches past the last member: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        const std::vector<float> v = many.download(0, members);
        const std::vector<uint64_t> taken = many.steps_taken();
        const std::vector<uint8_t> flags = many.active();
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 5;
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        std::fwrite(taken.data(), sizeof(uint64_t), taken.size(), f);
        std::fwrite(flags.data(), 1, flags.size(), f);
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
