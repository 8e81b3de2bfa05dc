// Exercises the component matches of include/grayscott_hip.hpp: Species::match_since() and Ensemble::matches_since() over the
// C ABI.
// Usage: match_mirror MEMBERS ROWS COLS STEPS OUT.bin
// A lone Species takes STEPS steps, is snapshot, takes STEPS more and is matched with the snapshot: V above 0.25 under
// connectivity 8 with min_size 1, then V above 0.1 under connectivity 4 with min_size 3.  Writes matches, each as three u64
// counts followed by that many gs_component_record (48 bytes each) of `before`, of `after`, and gs_component_overlap (16 bytes
// each): the two of the lone Species, then V above 0.25 (connectivity 8, min_size 1) of every ensemble member (all with the
// default parameters) treated the same way; then the lone Species' V plane at the snapshot and at the end (f32).
// Built and run by tests/test_match_cpu.py (without a GPU: fails loudly) and tests/test_gpu_match.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
void put(std::FILE *f, const gs::ComponentMatch &m)
{
    const uint64_t n[3] = {m.before.size(), m.after.size(), m.overlaps.size()};
    std::fwrite(n, sizeof n[0], 3, f);
    std::fwrite(m.before.data(), sizeof(gs_component_record), m.before.size(), f);
    std::fwrite(m.after.data(), sizeof(gs_component_record), m.after.size(), f);
    std::fwrite(m.overlaps.data(), sizeof(gs_component_overlap), m.overlaps.size(), f);
}

template <typename Call>
bool refused(Call call)
{
    try {
        call();
    } catch (const gs::HipError &e) {
        return e.code == GS_ERR_INVALID;
    }
    return false;
}
} // namespace

int main(int argc, char **argv)
{
    static_assert(sizeof(gs_component_overlap) == 16, "gs_component_overlap layout");
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
        const std::vector<float> v0 = species.make_result_view();
        gs::Snapshot snap = species.snapshot();
        sim.perform_steps(species, steps);
        const gs::ComponentMatch m8 = species.match_since(snap), m4 = species.match_since(snap, 0.1f, 1, true, 4, 3);
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        gs::Ensemble ref = many.snapshot();
        many.perform_steps(steps);
        const auto m = many.matches_since(ref, 0, members);
        if (m.size() != members) return 3;
        if (many.matches_since(ref, 1, members - 1).size() != members - 1) return 3;
        if (!refused([&] { many.matches_since(ref, members, 1); })) return 4;          // outside the ensemble
        if (!refused([&] { species.match_since(snap, 0.25f, 1, true, 6); })) return 6;    // neither 4 nor 8
        if (!refused([&] { species.match_since(snap, 0.25f, 1, true, 8, 0); })) return 7; // min_size 0
        if (!refused([&] { species.match_since(snap, 0.25f, 2); })) return 8;             // no such species
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 5;
        put(f, m8);
        put(f, m4);
        for (const auto &one : m) put(f, one);
        std::fwrite(v0.data(), sizeof(float), v0.size(), f);
        const std::vector<float> v = species.make_result_view();
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
