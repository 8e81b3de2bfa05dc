// Exercises the regional state comparison of include/grayscott_hip.hpp: Species::region_changes_since() over the C ABI.
// Usage: region_change_mirror ROWS COLS RH RW STEPS OUT.bin
// Takes a snapshot of a lone Species after STEPS steps, runs 8 steps more and writes: RR, RC (u64); per species (U, then V)
// and region sum_abs, sum_sq, max_abs (f64), differing, nonfinite, cells (u64); then the snapshot's U and V planes and the
// current U and V planes (f32).
// Built and run by tests/test_region_change_cpu.py (without a GPU: fails loudly) and tests/test_gpu_region_change_mirror.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s rows cols rh rw steps out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const int32_t rh = (int32_t)std::strtol(argv[3], nullptr, 10), rw = (int32_t)std::strtol(argv[4], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[5], nullptr, 10);
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        gs::Snapshot snap = species.snapshot();
        const auto same = species.region_changes_since(snap, rh, rw);
        for (const gs::Change &c : same.second.results)
            if (!c.equal() || c.sum_abs != 0.0 || c.max_abs != 0.0) return 3; // nothing has moved yet
        sim.perform_steps(species, 8);
        const auto uv = species.region_changes_since(snap, rh, rw);
        for (const gs::RegionChange *c : {&uv.first, &uv.second})
            if (c->results.size() != c->rr * c->rc || c->rr != uv.second.rr || c->rc != uv.second.rc || c->rh != rh || c->rw != rw)
                return 3;
        if (uv.second.steady(1e30).size() != uv.second.results.size() || !uv.second.steady(1e30).at(0)) return 3;
        bool threw = false;
        try {
            species.region_changes_since(snap, rh, 18); // no multiple of 4: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        std::FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 5;
        const uint64_t head[2] = {uv.second.rr, uv.second.rc};
        std::fwrite(head, sizeof(uint64_t), 2, f);
        for (const gs::RegionChange *c : {&uv.first, &uv.second})
            for (const gs::Change &x : c->results) {
                const double sums[3] = {x.sum_abs, x.sum_sq, x.max_abs};
                const uint64_t counts[3] = {x.differing, x.nonfinite, x.cells};
                std::fwrite(sums, sizeof(double), 3, f);
                std::fwrite(counts, sizeof(uint64_t), 3, f);
            }
        for (gs::HipConcentration *p : {&snap.u(), &snap.v()}) {
            const std::vector<float> x = p->make_scalar_view(species.context());
            std::fwrite(x.data(), sizeof(float), x.size(), f);
        }
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
