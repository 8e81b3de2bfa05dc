// Exercises Simulation::set_param_map of include/grayscott_hip.hpp: Species::new's pattern under a map whose feed rate
// rises along the rows and whose kill rate rises along the columns, `steps` steps through gs_run, then the map detached
// and `steps` more.
// Usage: param_map_mirror ROWS COLS STEPS OUT.bin   (writes V after the mapped steps, then V after the unmapped ones)
// Built and run by tests/test_cpp_param_map_mirror.py; plain g++, links libgs_hip.so.
#include "grayscott_hip.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s rows cols steps out.bin\n", argv[0]);
        return 2;
    }
    const std::size_t rows = std::strtoull(argv[1], nullptr, 10), cols = std::strtoull(argv[2], nullptr, 10);
    const std::size_t steps = std::strtoull(argv[3], nullptr, 10);
    try {
        gs::Simulation sim = gs::Simulation::new_(gs::Parameters());
        std::vector<float> feed(rows * cols), kill(rows * cols);
        for (std::size_t r = 0; r < rows; ++r)
            for (std::size_t c = 0; c < cols; ++c) {
                feed[r * cols + c] = 0.01f + 0.0005f * (float)r;
                kill[r * cols + c] = 0.045f + 0.0002f * (float)c;
            }
        gs::Species species = sim.make_species({rows, cols});
        sim.set_param_map({rows, cols}, feed.data(), kill.data());
        feed.assign(feed.size(), 0.0f); // the library holds its own copy
        sim.perform_steps(species, steps);
        std::vector<float> v(rows * cols);
        species.write_result_view(v.data(), {rows, cols});
        std::FILE *f = std::fopen(argv[4], "wb");
        if (!f) return 4;
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        sim.clear_param_map();
        sim.perform_steps(species, steps);
        species.write_result_view(v.data(), {rows, cols});
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        std::fclose(f);
    } catch (const gs::HipError &e) {
        std::fprintf(stderr, "HipError: %s\n", e.what());
        return 10 - e.code; // GS_ERR_NO_DEVICE (-4) -> 14
    }
    return 0;
}
