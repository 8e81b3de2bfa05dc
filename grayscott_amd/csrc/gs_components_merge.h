// gs_components_merge.h -- the seam merge of gs_fields_components (gs_observe.cpp) as a function of plain arrays: no
// device, no context, so that it can be tested on its own (tests/cpp/components_merge.cpp).
//
// Every slab has labelled its own rows as if it were alone: `part[s]` is its result, and for its first and its last row it
// names, per column, the root of the cell's component inside the slab (kCompUnset for an unset cell) and that component's
// size.  A component that touches neither row is final.  One that does is OPEN: it is taken out of its slab's `components`
// and `by_size`, united with the open components it touches across the seams -- by the connectivity rule on the two facing
// rows --, and what the unions leave is added back with the summed sizes.  A component may cross one seam many times, span
// several slabs, or touch a slab's first and last row (one node: the root names it); a one-row slab hands the same row in
// twice.  set_cells is the plain sum; largest is the maximum of the slabs' maxima and the merged sizes, because a merged
// component is never smaller than its parts.  Integers throughout: every rank that merges the same arrays gets the same bits.
//
// merge_component_lists is the same merge for gs_field_component_list's records: every slab hands in its records, rows
// already global, and for its first and its last row the index of every cell's record (kCompUnset for an unset cell) -- a slab
// of a chain lists every component that touches either row, whatever its size.  Records united across the seams become one:
// sizes and sums added, the boxes united, the first cell the smallest in row-major order.  min_size is applied to what the
// unions leave, and the result is in ascending order of the first cell.  With `where` (the match of two planes,
// gs_match_merge.h) the caller also learns what became of every record handed in: where[base(s) + k] is the index in the
// result of slab s's record k -- base(s) the number of records of the slabs before s -- or kCompUnset if the merged record
// fell below min_size.
// The host steps in front of it are here too: records_to_global_rows for a slab's records, which count rows from the slab's
// first, and batch_records_to_planes for a batch of an ensemble's members, planes stacked one after the other.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/gs_hip.h"

namespace gsi {

constexpr uint32_t kCompUnset = 0xffffffffu;

struct CompSeamRows { // of one slab, `cols` entries each
    const uint32_t *first_root, *first_size, *last_root, *last_size;
};

// The bin of gs_components.by_size for a component of `size` >= 1 cells: floor(log2(size)), at most 31.
inline int comp_size_bin(uint64_t size)
{
    int b = 0;
    while (b < 31 && (size >> (b + 1)) != 0) ++b;
    return b;
}

// The slabs in ascending global row order; none is empty.  connectivity: 4 or 8.
inline gs_components merge_components(const gs_components *part, const CompSeamRows *seam, size_t nslab, size_t cols,
                                      int connectivity)
{
    gs_components out{};
    for (size_t s = 0; s < nslab; ++s) {
        out.components += part[s].components;
        out.set_cells += part[s].set_cells;
        out.largest = std::max(out.largest, part[s].largest);
        for (int b = 0; b < 32; ++b) out.by_size[b] += part[s].by_size[b];
    }
    if (nslab < 2) return out;
    // the open components: (slab, root) -> node, each taken once
    struct Open {
        uint64_t key; // slab << 32 | root
        uint32_t size;
    };
    std::vector<Open> open;
    for (size_t s = 0; s < nslab; ++s)
        for (size_t c = 0; c < cols; ++c) {
            if (seam[s].first_root[c] != kCompUnset) open.push_back({(uint64_t)s << 32 | seam[s].first_root[c], seam[s].first_size[c]});
            if (seam[s].last_root[c] != kCompUnset) open.push_back({(uint64_t)s << 32 | seam[s].last_root[c], seam[s].last_size[c]});
        }
    std::sort(open.begin(), open.end(), [](const Open &a, const Open &b) { return a.key < b.key; });
    open.erase(std::unique(open.begin(), open.end(), [](const Open &a, const Open &b) { return a.key == b.key; }), open.end());
    auto node_of = [&](size_t s, uint32_t root) -> size_t {
        const uint64_t key = (uint64_t)s << 32 | root;
        return (size_t)(std::lower_bound(open.begin(), open.end(), key, [](const Open &a, uint64_t k) { return a.key < k; }) -
                        open.begin());
    };
    for (const Open &o : open) {
        out.components -= 1;
        out.by_size[comp_size_bin(o.size)] -= 1;
    }
    // unions across every seam: the cell below with the cells above it
    std::vector<size_t> up(open.size());
    for (size_t i = 0; i < up.size(); ++i) up[i] = i;
    auto find = [&](size_t x) {
        while (up[x] != x) x = up[x] = up[up[x]];
        return x;
    };
    for (size_t s = 0; s + 1 < nslab; ++s) {
        const uint32_t *above = seam[s].last_root, *below = seam[s + 1].first_root;
        for (size_t c = 0; c < cols; ++c) {
            if (below[c] == kCompUnset) continue;
            const size_t me = node_of(s + 1, below[c]);
            const size_t c0 = (connectivity == 8 && c > 0) ? c - 1 : c, c1 = (connectivity == 8 && c + 1 < cols) ? c + 1 : c;
            for (size_t k = c0; k <= c1; ++k) {
                if (above[k] == kCompUnset) continue;
                const size_t a = find(me), b = find(node_of(s, above[k]));
                if (a != b) up[std::max(a, b)] = std::min(a, b);
            }
        }
    }
    std::vector<uint64_t> merged(open.size(), (uint64_t)0);
    for (size_t i = 0; i < open.size(); ++i) merged[find(i)] += open[i].size;
    for (size_t i = 0; i < open.size(); ++i) {
        if (up[i] != i) continue;
        out.components += 1;
        out.by_size[comp_size_bin(merged[i])] += 1;
        out.largest = std::max(out.largest, merged[i]);
    }
    return out;
}

struct ListSeamRows { // of one slab, `cols` entries each: the index of the cell's record among the slab's records
    const uint32_t *first_index, *last_index;
};

inline bool comp_first_cell_before(const gs_component_record &a, const gs_component_record &b)
{
    return a.first_row != b.first_row ? a.first_row < b.first_row : a.first_col < b.first_col;
}

// rec[0 .. n): the records of a slab that begins at row g of the global grid, local rows to global rows.
inline void records_to_global_rows(gs_component_record *rec, size_t n, uint64_t g)
{
    for (size_t k = 0; k < n; ++k) {
        gs_component_record &r = rec[k];
        r.first_row += (uint32_t)g;
        r.row_min += (uint32_t)g;
        r.row_max += (uint32_t)g;
        r.sum_row += r.size * g;
    }
}

// rec[0 .. n): the records of a batch of `planes` planes of `rows` rows each.  A record's plane follows from its first cell,
// whose row becomes the row inside that plane; before[p] is the number of the batch's records in the planes before plane p
// (planes + 1 entries: before[planes] == n).
inline void batch_records_to_planes(gs_component_record *rec, size_t n, uint64_t rows, size_t planes, std::vector<uint64_t> &before)
{
    before.assign(planes + 1, (uint64_t)0);
    for (size_t k = 0; k < n; ++k) {
        const uint64_t plane_of = rec[k].first_row / rows;
        rec[k].first_row = (uint32_t)(rec[k].first_row % rows);
        before[(size_t)plane_of + 1] += 1;
    }
    for (size_t p = 0; p < planes; ++p) before[p + 1] += before[p];
}

// The slabs in ascending global row order; none is empty.  part[s]: slab s's records, n[s] of them.  connectivity: 4 or 8.
inline std::vector<gs_component_record> merge_component_lists(const gs_component_record *const *part, const size_t *n,
                                                              const ListSeamRows *seam, size_t nslab, size_t cols,
                                                              int connectivity, uint64_t min_size,
                                                              std::vector<uint32_t> *where = nullptr)
{
    std::vector<size_t> base(nslab + 1, 0);
    for (size_t s = 0; s < nslab; ++s) base[s + 1] = base[s] + n[s];
    std::vector<gs_component_record> all;
    all.reserve(base[nslab]);
    for (size_t s = 0; s < nslab; ++s) all.insert(all.end(), part[s], part[s] + n[s]);
    std::vector<size_t> up(all.size());
    for (size_t i = 0; i < up.size(); ++i) up[i] = i;
    auto find = [&](size_t x) {
        while (up[x] != x) x = up[x] = up[up[x]];
        return x;
    };
    // unions across every seam: the cell below with the cells above it
    for (size_t s = 0; s + 1 < nslab; ++s) {
        const uint32_t *above = seam[s].last_index, *below = seam[s + 1].first_index;
        for (size_t c = 0; c < cols; ++c) {
            if (below[c] == kCompUnset) continue;
            const size_t c0 = (connectivity == 8 && c > 0) ? c - 1 : c, c1 = (connectivity == 8 && c + 1 < cols) ? c + 1 : c;
            for (size_t k = c0; k <= c1; ++k) {
                if (above[k] == kCompUnset) continue;
                const size_t a = find(base[s + 1] + below[c]), b = find(base[s] + above[k]);
                if (a != b) up[std::max(a, b)] = std::min(a, b);
            }
        }
    }
    for (size_t i = 0; i < all.size(); ++i) {
        const size_t r = find(i);
        if (r == i) continue;
        gs_component_record &to = all[r];
        const gs_component_record &x = all[i];
        to.size += x.size;
        to.sum_row += x.sum_row;
        to.sum_col += x.sum_col;
        if (comp_first_cell_before(x, to)) to.first_row = x.first_row, to.first_col = x.first_col;
        to.row_min = std::min(to.row_min, x.row_min);
        to.row_max = std::max(to.row_max, x.row_max);
        to.col_min = std::min(to.col_min, x.col_min);
        to.col_max = std::max(to.col_max, x.col_max);
    }
    std::vector<gs_component_record> out;
    for (size_t i = 0; i < all.size(); ++i)
        if (up[i] == i && all[i].size >= min_size) out.push_back(all[i]);
    // (every slab's records come in first-cell order and the slabs in row order: only merged records can be out of place)
    if (!std::is_sorted(out.begin(), out.end(), comp_first_cell_before)) std::sort(out.begin(), out.end(), comp_first_cell_before);
    if (where) { // first cells are distinct: a kept root is found again by its own
        where->assign(all.size(), kCompUnset);
        for (size_t i = 0; i < all.size(); ++i) {
            const gs_component_record &root = all[find(i)];
            if (root.size < min_size) continue;
            (*where)[i] = (uint32_t)(std::lower_bound(out.begin(), out.end(), root, comp_first_cell_before) - out.begin());
        }
    }
    return out;
}

} // namespace gsi
