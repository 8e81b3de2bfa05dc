// Exercises the component lists of include/grayscott_hip.hpp: Species::component_list() and Ensemble::component_lists() over
// the C ABI.
// Usage: component_list_mirror MEMBERS ROWS COLS STEPS OUT.bin
// Writes lists, each as a u64 count followed by that many gs_component_record (48 bytes each): of a lone Species after STEPS
// steps V above 0.25 under connectivity 8 with min_size 1, V above 0.1 under connectivity 4 with min_size 3 and U below 0.5
// under connectivity 8 with min_size 1; then V above 0.25 (connectivity 8, min_size 1) of every ensemble member (all with the
// default parameters) after the same steps; then the lone Species' U and V planes (f32).
// Built and run by tests/test_component_list_cpu.py (without a GPU: fails loudly) and tests/test_gpu_component_list.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
void put(std::FILE *f, const std::vector<gs_component_record> &list)
{
    const uint64_t n = list.size();
    std::fwrite(&n, sizeof n, 1, f);
    std::fwrite(list.data(), sizeof(gs_component_record), list.size(), f);
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
    static_assert(sizeof(gs_component_record) == 48, "gs_component_record layout");
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
        const auto v8 = species.component_list(), v4 = species.component_list(0.1f, 1, true, 4, 3);
        const auto u8 = species.component_list(0.5f, 0, false);
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        const auto m = many.component_lists(0, members);
        if (m.size() != members) return 3;
        if (many.component_lists(1, members - 1).size() != members - 1) return 3;
        if (!refused([&] { many.component_lists(members, 1); })) return 4;        // outside the ensemble
        if (!refused([&] { species.component_list(0.25f, 1, true, 6); })) return 6; // neither 4 nor 8
        if (!refused([&] { species.component_list(0.25f, 1, true, 8, 0); })) return 7; // min_size 0
        if (!refused([&] { species.component_list(0.25f, 2); })) return 8;        // no such species
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 5;
        put(f, v8);
        put(f, v4);
        put(f, u8);
        for (const auto &list : m) put(f, list);
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
