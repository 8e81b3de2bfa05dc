// components_merge.cpp -- two device-free checks of the connected components (include/gs_hip.h: gs_fields_components):
//   1. the seam merge of grayscott_amd/csrc/gs_components_merge.h: a plane is cut into 1..5 slabs (one-row slabs included),
//      every slab is labelled by a naive flood fill, its counters and seam rows go through merge_components, and the
//      result must equal the flood fill of the whole plane;
//   2. the phases of grayscott_amd/csrc/gs_components.hip -- tile, border, flatten, tally -- replayed one thread after the
//      other through the find / unite of gs_unionfind.h, with tiles far smaller than the device's so that a small plane has
//      many, against the same flood fill; the invariant parent[i] <= i is checked after every phase.
// Exit status 0 and "ok" when everything agrees.  Stand-alone: it links nothing of the library.
#include "../../grayscott_amd/csrc/gs_components_merge.h"
#include "../../grayscott_amd/csrc/gs_unionfind.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>

namespace {

struct Plane {
    size_t rows, cols;
    std::vector<unsigned char> set;
    bool at(size_t r, size_t c) const { return set[r * cols + c] != 0; }
};

struct Labelled {
    gs_components total{};
    std::vector<uint32_t> root, size; // per cell: the smallest index of its component (kCompUnset: unset), that one's size
};

// Flood fill of rows [r0, r1) of p as a plane of its own.
Labelled flood(const Plane &p, size_t r0, size_t r1, int connectivity)
{
    const size_t rows = r1 - r0, cols = p.cols;
    Labelled out;
    out.root.assign(rows * cols, gsi::kCompUnset);
    out.size.assign(rows * cols, 0u);
    std::vector<size_t> stack, members;
    for (size_t i = 0; i < rows * cols; ++i) {
        if (!p.at(r0 + i / cols, i % cols) || out.root[i] != gsi::kCompUnset) continue;
        stack.assign(1, i);
        members.clear();
        out.root[i] = (uint32_t)i;
        while (!stack.empty()) {
            const size_t x = stack.back();
            stack.pop_back();
            members.push_back(x);
            const long r = (long)(x / cols), c = (long)(x % cols);
            for (long dr = -1; dr <= 1; ++dr)
                for (long dc = -1; dc <= 1; ++dc) {
                    if ((dr == 0 && dc == 0) || (connectivity == 4 && dr != 0 && dc != 0)) continue;
                    const long rr = r + dr, cc = c + dc;
                    if (rr < 0 || rr >= (long)rows || cc < 0 || cc >= (long)cols) continue;
                    const size_t y = (size_t)rr * cols + (size_t)cc;
                    if (!p.at(r0 + (size_t)rr, (size_t)cc) || out.root[y] != gsi::kCompUnset) continue;
                    out.root[y] = (uint32_t)i;
                    stack.push_back(y);
                }
        }
        for (const size_t x : members) out.size[x] = (uint32_t)members.size();
        out.total.components += 1;
        out.total.set_cells += members.size();
        out.total.largest = std::max<uint64_t>(out.total.largest, members.size());
        out.total.by_size[gsi::comp_size_bin(members.size())] += 1;
    }
    return out;
}

bool same(const gs_components &a, const gs_components &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int failures = 0;

void report(const std::string &what, const gs_components &got, const gs_components &want)
{
    if (same(got, want)) return;
    ++failures;
    std::fprintf(stderr, "%s: components %llu set %llu largest %llu, not %llu %llu %llu\n", what.c_str(),
                 (unsigned long long)got.components, (unsigned long long)got.set_cells, (unsigned long long)got.largest,
                 (unsigned long long)want.components, (unsigned long long)want.set_cells, (unsigned long long)want.largest);
}

// ---- 1. the seam merge -------------------------------------------------------------------------------------------------
void check_merge(const Plane &p, const std::vector<size_t> &cuts /* first rows of the slabs, then rows */, int connectivity,
                 const std::string &what)
{
    const size_t nslab = cuts.size() - 1;
    std::vector<Labelled> slab;
    for (size_t s = 0; s < nslab; ++s) slab.push_back(flood(p, cuts[s], cuts[s + 1], connectivity));
    std::vector<gs_components> part;
    std::vector<gsi::CompSeamRows> seam;
    for (size_t s = 0; s < nslab; ++s) {
        const size_t last = (cuts[s + 1] - cuts[s] - 1) * p.cols;
        part.push_back(slab[s].total);
        seam.push_back({slab[s].root.data(), slab[s].size.data(), slab[s].root.data() + last, slab[s].size.data() + last});
    }
    report(what, gsi::merge_components(part.data(), seam.data(), nslab, p.cols, connectivity),
           flood(p, 0, p.rows, connectivity).total);
}

void check_every_cut(const Plane &p, const std::string &what)
{
    for (int connectivity : {4, 8})
        for (size_t nslab = 1; nslab <= 5 && nslab <= p.rows; ++nslab) {
            std::vector<size_t> even, top, bottom; // equal as can be; one-row slabs first; one-row slabs last
            for (size_t s = 0; s <= nslab; ++s) {
                even.push_back(s * p.rows / nslab);
                top.push_back(s < nslab ? s : p.rows);
                bottom.push_back(s == 0 ? 0 : p.rows - (nslab - s));
            }
            const std::string tag = what + ", " + std::to_string(nslab) + " slabs, connectivity " + std::to_string(connectivity);
            check_merge(p, even, connectivity, tag);
            check_merge(p, top, connectivity, tag + ", one-row slabs on top");
            check_merge(p, bottom, connectivity, tag + ", one-row slabs below");
        }
}

// ---- 2. the kernels' phases, one thread after the other ------------------------------------------------------------------
void check_phases(const Plane &p, size_t tr, size_t tc, int connectivity, const std::string &what)
{
    const size_t rows = p.rows, cols = p.cols, total = rows * cols;
    const bool eight = connectivity == 8;
    std::vector<uint32_t> parent(total, 0u), size(total, 0u);
    auto ordered = [&](const char *phase) {
        for (size_t i = 0; i < total; ++i)
            if (parent[i] != kUfUnset && parent[i] > i) {
                ++failures;
                std::fprintf(stderr, "%s: parent[%zu] = %u after the %s phase\n", what.c_str(), i, parent[i], phase);
                return;
            }
    };
    // tile: runs inside the tile, unions with the row above inside the tile, the root as an entry of the plane
    std::vector<uint32_t> lab(tr * tc);
    for (size_t r0 = 0; r0 < rows; r0 += tr)
        for (size_t c0 = 0; c0 < cols; c0 += tc) {
            auto set = [&](size_t lr, size_t lc) { return r0 + lr < rows && c0 + lc < cols && p.at(r0 + lr, c0 + lc); };
            for (size_t lr = 0; lr < tr; ++lr)
                for (size_t lc = 0, run = 0; lc < tc; ++lc) {
                    if (set(lr, lc) && (lc == 0 || !set(lr, lc - 1))) run = lr * tc + lc;
                    lab[lr * tc + lc] = set(lr, lc) ? (uint32_t)run : kUfUnset;
                }
            for (size_t lr = 1; lr < tr; ++lr)
                for (size_t lc = 0; lc < tc; ++lc) {
                    if (!set(lr, lc)) continue;
                    const uint32_t me = (uint32_t)(lr * tc + lc);
                    const bool left = lc > 0 && set(lr, lc - 1), up = set(lr - 1, lc);
                    const bool upleft = lc > 0 && set(lr - 1, lc - 1), upright = lc + 1 < tc && set(lr - 1, lc + 1);
                    if (up) {
                        if (!(left && upleft)) gs_uf_unite(lab.data(), me, me - (uint32_t)tc);
                    } else if (eight) {
                        if (upleft && !left) gs_uf_unite(lab.data(), me, me - (uint32_t)tc - 1);
                        if (upright) gs_uf_unite(lab.data(), me, me - (uint32_t)tc + 1);
                    }
                }
            for (size_t lr = 0; lr < tr && r0 + lr < rows; ++lr)
                for (size_t lc = 0; lc < tc && c0 + lc < cols; ++lc) {
                    uint32_t v = kUfUnset;
                    if (set(lr, lc)) {
                        const uint32_t root = gs_uf_find(lab.data(), (uint32_t)(lr * tc + lc));
                        v = (uint32_t)((r0 + root / tc) * cols + c0 + root % tc);
                    }
                    parent[(r0 + lr) * cols + c0 + lc] = v;
                }
        }
    ordered("tile");
    // border: the first row and the first column of every tile
    auto join = [&](uint32_t me, long r, long c) {
        if (r < 0 || r >= (long)rows || c < 0 || c >= (long)cols) return;
        const uint32_t o = (uint32_t)((size_t)r * cols + (size_t)c);
        if (parent[o] != kUfUnset) gs_uf_unite(parent.data(), me, o);
    };
    for (size_t r = tr; r < rows; r += tr)
        for (size_t c = 0; c < cols; ++c) {
            const uint32_t me = (uint32_t)(r * cols + c);
            if (parent[me] == kUfUnset) continue;
            join(me, (long)r - 1, (long)c);
            if (eight) join(me, (long)r - 1, (long)c - 1), join(me, (long)r - 1, (long)c + 1);
        }
    for (size_t c = tc; c < cols; c += tc)
        for (size_t r = 0; r < rows; ++r) {
            const uint32_t me = (uint32_t)(r * cols + c);
            if (parent[me] == kUfUnset) continue;
            join(me, (long)r, (long)c - 1);
            if (eight) join(me, (long)r - 1, (long)c - 1), join(me, (long)r + 1, (long)c - 1);
        }
    ordered("border");
    // flatten and tally
    for (size_t i = 0; i < total; ++i) {
        if (parent[i] == kUfUnset) continue;
        const uint32_t root = gs_uf_find(parent.data(), (uint32_t)i);
        parent[i] = root;
        size[root] += 1;
    }
    ordered("flatten");
    gs_components got{};
    for (size_t i = 0; i < total; ++i) {
        if (parent[i] != (uint32_t)i) continue;
        got.components += 1;
        got.set_cells += size[i];
        got.largest = std::max<uint64_t>(got.largest, size[i]);
        got.by_size[gsi::comp_size_bin(size[i])] += 1;
    }
    const Labelled want = flood(p, 0, rows, connectivity);
    report(what, got, want.total);
    for (size_t i = 0; i < total; ++i)
        if (parent[i] != want.root[i] || (parent[i] != kUfUnset && size[parent[i]] != want.size[i])) {
            ++failures;
            std::fprintf(stderr, "%s: cell %zu has root %u, not %u\n", what.c_str(), i, parent[i], want.root[i]);
            break;
        }
}

// ---- planes ---------------------------------------------------------------------------------------------------------------
Plane blank(size_t rows, size_t cols) { return Plane{rows, cols, std::vector<unsigned char>(rows * cols, 0)}; }

Plane u_shape(size_t rows, size_t cols) // both arms cross every seam; joined in the first row
{
    Plane p = blank(rows, cols);
    for (size_t r = 0; r < rows; ++r) p.set[r * cols + 1] = p.set[r * cols + cols - 2] = 1;
    for (size_t c = 1; c + 1 < cols; ++c) p.set[c] = 1;
    return p;
}

Plane snake(size_t rows, size_t cols) // columns 0, 2, 4, ... joined at alternating ends: crosses every seam many times
{
    Plane p = blank(rows, cols);
    for (size_t c = 0, k = 0; c < cols; c += 2, ++k) {
        for (size_t r = 0; r < rows; ++r) p.set[r * cols + c] = 1;
        if (c + 2 < cols) p.set[(k % 2 ? 0 : rows - 1) * cols + c + 1] = 1;
    }
    return p;
}

Plane column(size_t rows, size_t cols)
{
    Plane p = blank(rows, cols);
    for (size_t r = 0; r < rows; ++r) p.set[r * cols + cols / 2] = 1;
    return p;
}

Plane staircase(size_t rows, size_t cols) // connected under 8 only
{
    Plane p = blank(rows, cols);
    for (size_t r = 0; r < rows && r < cols; ++r) p.set[r * cols + r] = 1;
    return p;
}

Plane random_plane(size_t rows, size_t cols, double density, unsigned seed)
{
    Plane p = blank(rows, cols);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (auto &x : p.set) x = u(rng) < density ? 1 : 0;
    return p;
}

} // namespace

int main()
{
    std::vector<std::pair<std::string, Plane>> planes;
    planes.push_back({"U", u_shape(11, 9)});
    planes.push_back({"snake", snake(10, 13)});
    planes.push_back({"column", column(7, 5)});
    planes.push_back({"staircase", staircase(12, 14)});
    planes.push_back({"one row", random_plane(1, 17, 0.6, 1)});
    planes.push_back({"one column", random_plane(9, 1, 0.6, 2)});
    planes.push_back({"full", random_plane(6, 7, 1.1, 3)});
    planes.push_back({"empty", random_plane(6, 7, -1.0, 4)});
    unsigned seed = 10;
    for (const double density : {0.2, 0.5, 0.593, 0.8})
        for (const auto &shape : {std::pair<size_t, size_t>{5, 5}, {13, 21}, {30, 17}, {8, 64}})
            planes.push_back({"random " + std::to_string(density), random_plane(shape.first, shape.second, density, seed++)});
    for (const auto &np : planes) {
        check_every_cut(np.second, np.first);
        for (int connectivity : {4, 8})
            for (const auto &tile : {std::pair<size_t, size_t>{2, 4}, {3, 5}, {4, 4}, {16, 256}})
                check_phases(np.second, tile.first, tile.second, connectivity,
                             np.first + ", tiles of " + std::to_string(tile.first) + " x " + std::to_string(tile.second) +
                                 ", connectivity " + std::to_string(connectivity));
    }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
