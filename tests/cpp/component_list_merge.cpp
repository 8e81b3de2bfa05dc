// component_list_merge.cpp -- a device-free check of the seam merge of the component lists (include/gs_hip.h:
// gs_field_component_list; grayscott_amd/csrc/gs_components_merge.h: merge_component_lists).  A small plane is cut into 1..5
// slabs (one-row slabs included); every slab is labelled on the host with the find / unite of gs_unionfind.h as if it were
// alone and lists what the device would: the components of at least min_size cells and, in a chain, every component that
// touches the slab's first or last row, in first-cell order, rows counted from the slab's first as the device counts them,
// and the record index of every cell of those two rows.  records_to_global_rows and then the merge of these must equal the
// list of the whole plane, record for record.  A batch of 1..4 planes, some of them empty, stacked as an ensemble's members
// are -- the records in first-cell order over the stack, the first cell's row counted over the stack -- must come apart
// again into every plane's own list (batch_records_to_planes).
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

struct SlabList {
    std::vector<gs_component_record> records; // rows local to the slab
    std::vector<uint32_t> first_index, last_index;
};

// Rows [r0, r1) of p labelled as a plane of its own.  open: also list what touches the first or last row.
SlabList list_rows(const Plane &p, size_t r0, size_t r1, int connectivity, uint64_t min_size, bool open)
{
    const size_t rows = r1 - r0, cols = p.cols, total = rows * cols;
    std::vector<uint32_t> parent(total, kUfUnset);
    for (size_t i = 0; i < total; ++i)
        if (p.at(r0 + i / cols, i % cols)) parent[i] = (uint32_t)i;
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) {
            const uint32_t me = (uint32_t)(r * cols + c);
            if (parent[me] == kUfUnset) continue;
            auto join = [&](long rr, long cc) {
                if (rr < 0 || cc < 0 || cc >= (long)cols) return;
                const uint32_t o = (uint32_t)((size_t)rr * cols + (size_t)cc);
                if (parent[o] != kUfUnset) gs_uf_unite(parent.data(), me, o);
            };
            join((long)r, (long)c - 1);
            join((long)r - 1, (long)c);
            if (connectivity == 8) join((long)r - 1, (long)c - 1), join((long)r - 1, (long)c + 1);
        }
    std::vector<gs_component_record> rec(total);
    std::vector<unsigned char> listed(total, 0);
    for (size_t i = 0; i < total; ++i) {
        if (parent[i] == kUfUnset) continue;
        const uint32_t root = gs_uf_find(parent.data(), (uint32_t)i);
        parent[i] = root;
        const uint32_t r = (uint32_t)(i / cols), c = (uint32_t)(i % cols);
        gs_component_record &x = rec[root];
        if (root == i) x = gs_component_record{0, 0, 0, r, c, r, r, c, c}; // (a root is its component's first cell)
        x.size += 1;
        x.sum_row += r;
        x.sum_col += c;
        x.row_min = std::min(x.row_min, r), x.row_max = std::max(x.row_max, r);
        x.col_min = std::min(x.col_min, c), x.col_max = std::max(x.col_max, c);
        if (open && (i / cols == 0 || i / cols == rows - 1)) listed[root] = 1;
    }
    SlabList out;
    std::vector<uint32_t> index(total, gsi::kCompUnset);
    for (size_t i = 0; i < total; ++i)
        if (parent[i] == i && (rec[i].size >= min_size || listed[i])) {
            index[i] = (uint32_t)out.records.size();
            out.records.push_back(rec[i]);
        }
    for (size_t c = 0; c < cols; ++c) {
        const uint32_t a = parent[c], b = parent[(rows - 1) * cols + c];
        out.first_index.push_back(a == kUfUnset ? gsi::kCompUnset : index[a]);
        out.last_index.push_back(b == kUfUnset ? gsi::kCompUnset : index[b]);
    }
    return out;
}

int failures = 0;

bool same_records(const std::vector<gs_component_record> &got, const std::vector<gs_component_record> &want)
{
    bool same = got.size() == want.size();
    for (size_t i = 0; same && i < got.size(); ++i) {
        const gs_component_record &a = got[i], &b = want[i];
        same = a.size == b.size && a.sum_row == b.sum_row && a.sum_col == b.sum_col && a.first_row == b.first_row &&
               a.first_col == b.first_col && a.row_min == b.row_min && a.row_max == b.row_max && a.col_min == b.col_min &&
               a.col_max == b.col_max;
    }
    return same;
}

// The planes as one batch: every plane listed alone, its first cells' rows counted over the stack, one list after the other.
void check_batch(const std::vector<Plane> &planes, int connectivity, uint64_t min_size, const std::string &what)
{
    const size_t rows = planes[0].rows;
    std::vector<std::vector<gs_component_record>> want;
    std::vector<gs_component_record> batch;
    for (size_t p = 0; p < planes.size(); ++p) {
        want.push_back(list_rows(planes[p], 0, rows, connectivity, min_size, false).records);
        for (gs_component_record r : want[p]) {
            r.first_row += (uint32_t)(p * rows);
            batch.push_back(r);
        }
    }
    std::vector<uint64_t> before;
    gsi::batch_records_to_planes(batch.data(), batch.size(), rows, planes.size(), before);
    bool same = before.size() == planes.size() + 1 && before[0] == 0 && before[planes.size()] == batch.size();
    for (size_t p = 0; same && p < planes.size(); ++p) {
        same = before[p + 1] - before[p] == want[p].size() && before[p + 1] <= batch.size();
        if (same)
            same = same_records(std::vector<gs_component_record>(batch.begin() + (long)before[p], batch.begin() + (long)before[p + 1]), want[p]);
    }
    if (same) return;
    ++failures;
    std::fprintf(stderr, "%s: a batch of %zu planes does not come apart into its planes' lists\n", what.c_str(), planes.size());
}

void check_merge(const Plane &p, const std::vector<size_t> &cuts /* first rows of the slabs, then rows */, int connectivity,
                 uint64_t min_size, const std::vector<gs_component_record> &want, const std::string &what)
{
    const size_t nslab = cuts.size() - 1;
    std::vector<SlabList> slab;
    for (size_t s = 0; s < nslab; ++s) {
        slab.push_back(list_rows(p, cuts[s], cuts[s + 1], connectivity, min_size, nslab > 1));
        gsi::records_to_global_rows(slab[s].records.data(), slab[s].records.size(), cuts[s]);
    }
    std::vector<const gs_component_record *> part;
    std::vector<size_t> n;
    std::vector<gsi::ListSeamRows> seam;
    for (const SlabList &s : slab) {
        part.push_back(s.records.data());
        n.push_back(s.records.size());
        seam.push_back({s.first_index.data(), s.last_index.data()});
    }
    const std::vector<gs_component_record> got =
        gsi::merge_component_lists(part.data(), n.data(), seam.data(), nslab, p.cols, connectivity, min_size);
    if (same_records(got, want)) return;
    ++failures;
    std::fprintf(stderr, "%s: %zu records, not the %zu of the whole plane, or other records\n", what.c_str(), got.size(), want.size());
}

void check_every_cut(const Plane &p, const std::string &what)
{
    for (int connectivity : {4, 8}) {
        const std::vector<gs_component_record> all = list_rows(p, 0, p.rows, connectivity, 1, false).records;
        uint64_t largest = 0;
        for (const gs_component_record &r : all) largest = std::max(largest, r.size);
        for (size_t i = 1; i < all.size(); ++i)
            if (!gsi::comp_first_cell_before(all[i - 1], all[i])) ++failures;
        for (const uint64_t min_size : {(uint64_t)1, (uint64_t)2, (uint64_t)7, largest + 1}) {
            std::vector<gs_component_record> want;
            for (const gs_component_record &r : all)
                if (r.size >= min_size) want.push_back(r);
            for (size_t nslab = 1; nslab <= 5 && nslab <= p.rows; ++nslab) {
                std::vector<size_t> even, top, bottom; // equal as can be; one-row slabs first; one-row slabs last
                for (size_t s = 0; s <= nslab; ++s) {
                    even.push_back(s * p.rows / nslab);
                    top.push_back(s < nslab ? s : p.rows);
                    bottom.push_back(s == 0 ? 0 : p.rows - (nslab - s));
                }
                const std::string tag = what + ", " + std::to_string(nslab) + " slabs, connectivity " + std::to_string(connectivity) +
                                        ", min_size " + std::to_string(min_size);
                check_merge(p, even, connectivity, min_size, want, tag);
                check_merge(p, top, connectivity, min_size, want, tag + ", one-row slabs on top");
                check_merge(p, bottom, connectivity, min_size, want, tag + ", one-row slabs below");
            }
        }
    }
}

// ---- planes ---------------------------------------------------------------------------------------------------------------
Plane blank(size_t rows, size_t cols) { return Plane{rows, cols, std::vector<unsigned char>(rows * cols, 0)}; }

Plane u_shape(size_t rows, size_t cols) // both arms cross every seam; joined in the LAST row: the first cell is in the first slab
{
    Plane p = blank(rows, cols);
    for (size_t r = 0; r < rows; ++r) p.set[r * cols + 1] = p.set[r * cols + cols - 2] = 1;
    for (size_t c = 1; c + 1 < cols; ++c) p.set[(rows - 1) * cols + c] = 1;
    return p;
}

Plane serpentine(size_t rows, size_t cols) // every other row set, joined at alternating ends: spans every slab
{
    Plane p = blank(rows, cols);
    for (size_t r = 0, k = 0; r < rows; r += 2, ++k) {
        for (size_t c = 0; c < cols; ++c) p.set[r * cols + c] = 1;
        if (r + 1 < rows) p.set[(r + 1) * cols + (k % 2 ? 0 : cols - 1)] = 1;
    }
    return p;
}

Plane comb(size_t rows, size_t cols) // teeth that cross every seam many times, joined in the first row
{
    Plane p = blank(rows, cols);
    for (size_t c = 0; c < cols; ++c) p.set[c] = 1;
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; c += 2) p.set[r * cols + c] = 1;
    return p;
}

Plane rings(size_t rows, size_t cols) // every other ring: components that touch a slab's first and last row
{
    Plane p = blank(rows, cols);
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) p.set[r * cols + c] = std::min(std::min(r, rows - 1 - r), std::min(c, cols - 1 - c)) % 2 == 0;
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
    planes.push_back({"serpentine", serpentine(10, 13)});
    planes.push_back({"comb", comb(9, 12)});
    planes.push_back({"rings", rings(12, 14)});
    planes.push_back({"one row", random_plane(1, 17, 0.6, 1)});
    planes.push_back({"one column", random_plane(9, 1, 0.6, 2)});
    planes.push_back({"full", random_plane(6, 7, 1.1, 3)});
    planes.push_back({"empty", random_plane(6, 7, -1.0, 4)});
    unsigned seed = 10;
    for (const double density : {0.3, 0.59, 0.9})
        for (const auto &shape : {std::pair<size_t, size_t>{5, 5}, {13, 21}, {30, 17}, {8, 64}})
            planes.push_back({"random " + std::to_string(density), random_plane(shape.first, shape.second, density, seed++)});
    for (const auto &np : planes) check_every_cut(np.second, np.first);
    // batches of 1..4 planes of one shape: the first, the last, a middle one or every plane with no set cell; one-row planes
    for (const auto &shape : {std::pair<size_t, size_t>{7, 9}, {1, 17}, {12, 5}})
        for (size_t count = 1; count <= 4; ++count)
            for (unsigned empty = 0; empty < (1u << count); ++empty) { // bit p: plane p has no set cell
                std::vector<Plane> batch;
                for (size_t p = 0; p < count; ++p)
                    batch.push_back(random_plane(shape.first, shape.second, (empty >> p) & 1 ? -1.0 : 0.45, seed++));
                for (int connectivity : {4, 8})
                    for (const uint64_t min_size : {(uint64_t)1, (uint64_t)3})
                        check_batch(batch, connectivity, min_size, "batch of " + std::to_string(count) + ", empty planes " + std::to_string(empty));
            }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
