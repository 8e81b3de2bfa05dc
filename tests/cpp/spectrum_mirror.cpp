// Exercises the power spectra of include/grayscott_hip.hpp: Species::spectrum() and Ensemble::spectra() over the C ABI.
// Usage: spectrum_mirror MEMBERS ROWS COLS STEPS TILE OUT.bin
// Writes, as [TILE][TILE / 2 + 1] f64 sums followed by the two u64 tile counts each: U and V of a lone Species after STEPS
// steps (periodic Hann window), then U and V of every ensemble member (all with the default parameters) after the same
// steps; then V's wavelength (f64) as the mirror computes it; then the lone Species' U and V planes (f32).
// Built and run by tests/test_gpu_spectrum_mirror.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s members rows cols steps tile out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t members = std::strtoull(argv[1], nullptr, 10);
    const std::size_t rows = std::strtoull(argv[2], nullptr, 10), cols = std::strtoull(argv[3], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[4], nullptr, 10);
    const int32_t tile = (int32_t)std::strtol(argv[5], nullptr, 10);
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, steps);
        const auto uv = species.spectrum(tile);
        if (uv.first.tile != tile || uv.second.window != 1 || uv.second.raw.size() != uv.second.bins()) return 3;
        if (uv.second.tiles_used != (rows / (std::size_t)tile) * (cols / (std::size_t)tile) || uv.second.tiles_skipped != 0) return 3;
        if (uv.second.radial().size() != (std::size_t)tile / 2 + 1) return 3;
        gs::Ensemble many = sim.make_ensemble({rows, cols}, std::vector<gs::Parameters>(members));
        many.perform_steps(steps);
        const std::vector<gs::Spectrum> m = many.spectra(0, members, tile);
        if (m.size() != 2 * members) return 3;
        bool threw = false;
        try {
            many.spectra(members, 1, tile); // outside the ensemble: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.spectrum(48); // no tile size: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 5;
        auto put = [&](const gs::Spectrum &x) {
            std::fwrite(x.raw.data(), sizeof(double), x.raw.size(), f);
            const uint64_t tiles[2] = {x.tiles_used, x.tiles_skipped};
            std::fwrite(tiles, sizeof(uint64_t), 2, f);
        };
        put(uv.first);
        put(uv.second);
        for (const gs::Spectrum &x : m) put(x);
        const double wavelength = uv.second.wavelength();
        std::fwrite(&wavelength, sizeof(double), 1, f);
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
