// Exercises the regional power spectra of include/grayscott_hip.hpp: Species::region_spectrum() over the C ABI.
// Usage: region_spectrum_mirror ROWS COLS RH RW TILE HANN OUT.bin
// Writes, for a lone Species after 31 steps: RR, RC and TILE (u64); per region of U, then of V: the raw sums
// (f64 [TILE][TILE/2 + 1]) and the tiles used and skipped (u64); then the U and V planes (f32).
// Built and run by tests/test_region_spectrum_cpu.py (without a GPU: fails loudly) and
// tests/test_gpu_region_spectrum_mirror.py.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s rows cols rh rw tile hann out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const int32_t rh = (int32_t)std::strtol(argv[3], nullptr, 10), rw = (int32_t)std::strtol(argv[4], nullptr, 10);
    const int32_t tile = (int32_t)std::strtol(argv[5], nullptr, 10);
    const bool hann = std::strtol(argv[6], nullptr, 10) != 0;
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        gs::Species species = sim.make_species({rows, cols});
        sim.perform_steps(species, 31);
        const auto uv = species.region_spectrum(rh, rw, tile, hann);
        if (uv.first.results.size() != uv.first.rr * uv.first.rc || uv.second.results.size() != uv.first.results.size()) return 3;
        if (uv.second.at(0, 0).raw.size() != (std::size_t)tile * (std::size_t)(tile / 2 + 1) || uv.first.at(0, 0).tile != tile) return 3;
        bool threw = false;
        try {
            species.region_spectrum(rh, 18, tile, hann); // no multiple of 4: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 4;
        threw = false;
        try {
            species.region_spectrum(rh, rw, 48, hann); // no tile size: must be rejected
        } catch (const gs::HipError &e) {
            threw = e.code == GS_ERR_INVALID;
        }
        if (!threw) return 6;
        std::FILE *f = std::fopen(argv[7], "wb");
        if (!f) return 5;
        const uint64_t head[3] = {uv.first.rr, uv.first.rc, (uint64_t)tile};
        std::fwrite(head, sizeof(uint64_t), 3, f);
        for (const gs::RegionSpectrum *s : {&uv.first, &uv.second})
            for (const gs::Spectrum &x : s->results) {
                std::fwrite(x.raw.data(), sizeof(double), x.raw.size(), f);
                const uint64_t tail[2] = {x.tiles_used, x.tiles_skipped};
                std::fwrite(tail, sizeof(uint64_t), 2, f);
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
