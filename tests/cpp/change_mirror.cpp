// Exercises the comparisons and snapshots of include/grayscott_hip.hpp over the C ABI: Species::snapshot / change_since /
// restore and Ensemble::snapshot / changes_since.
// Usage: change_mirror MEMBERS ROWS COLS STEPS OUT.bin
// A lone Species runs STEPS steps, is snapshotted, runs STEPS more and is compared with the snapshot; ensemble members (all
// with the default parameters) do the same.  Writes, as raw gs_change-sized records: U and V of the lone Species, then U and
// V of every member; then the Species' V plane at the snapshot and after (f32 each); then, after a restore and STEPS steps
// again, the V plane once more (it must equal the second).
// Built and run by tests/test_change_cpu.py (without a GPU: fails loudly) and tests/test_gpu_change.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
void put(std::FILE *f, const gs::Change &c)
{
    gs_change x{c.sum_abs, c.sum_sq, c.max_abs, c.differing, c.nonfinite};
    std::fwrite(&x, sizeof x, 1, f);
}
void put(std::FILE *f, const std::vector<float> &v) { std::fwrite(v.data(), sizeof(float), v.size(), f); }
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
        gs::Snapshot snap = species.snapshot();
        const std::pair<gs::Change, gs::Change> same = species.change_since(snap);
        if (!same.first.equal() || !same.second.equal() || same.first.cells != rows * cols) return 3;
        const std::vector<float> v0 = species.make_result_view();
        sim.perform_steps(species, steps);
        const std::pair<gs::Change, gs::Change> uv = species.change_since(snap);
        const std::vector<float> v1 = species.make_result_view();
        species.restore(snap);
        if (!species.change_since(snap).second.equal()) return 6;
        sim.perform_steps(species, steps);
        const std::vector<float> v2 = species.make_result_view();

        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        gs::Ensemble kept = many.snapshot();
        many.perform_steps(steps);
        const std::vector<gs::Change> m = many.changes_since(kept, 0, members);
        bool threw = false;
        try {
            many.changes_since(kept, members, 1); // outside the ensemble: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        std::FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 5;
        put(f, uv.first);
        put(f, uv.second);
        for (const gs::Change &c : m) put(f, c);
        put(f, v0);
        put(f, v1);
        put(f, v2);
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
