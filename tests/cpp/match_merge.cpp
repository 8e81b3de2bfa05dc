// match_merge.cpp -- a device-free check of the host side of the component matches (include/gs_hip.h: gs_fields_match;
// grayscott_amd/csrc/gs_match_merge.h: map_overlaps, fold_overlaps; gs_components_merge.h: merge_component_lists' `where`).
// Two small planes are cut into 1..5 slabs (one-row slabs included); every slab labels its rows of `before`, of `after` and of
// the cells set in both on the host with the find / unite of gs_unionfind.h as if it were alone, lists what the device would
// -- the components of at least min_size cells and, in a chain, every one that touches the slab's first or last row -- and
// leaves one raw overlap per piece, named through the piece's first cell, a dropped mark where a partner is not listed.  The
// index map of the two list merges and the overlap fold of these must equal the match of the whole planes, overlap for overlap.
// The slabs count rows from their own first row, as the device does; records_to_global_rows makes them global.  A batch of
// 1..4 pairs of planes stacked as an ensemble's members are -- records, pieces and indices counted over the stack, planes
// whose before-list or after-list is empty among them -- must come apart into every pair's own match (batch_records_to_planes,
// fold_batch_overlaps).
// Exit status 0 and "ok" when everything agrees.  Stand-alone: it links nothing of the library.
#include "../../grayscott_amd/csrc/gs_match_merge.h"
#include "../../grayscott_amd/csrc/gs_unionfind.h"

#include <cstdio>
#include <random>
#include <string>

namespace {

struct Plane {
    size_t rows, cols;
    std::vector<unsigned char> set;
};

struct Labels {
    std::vector<uint32_t> parent; // roots, kUfUnset for an unset cell
    std::vector<uint32_t> size;   // of a root
};

// Rows [r0, r1) of a set of cells labelled as a plane of its own.
Labels label_rows(const std::vector<unsigned char> &set, size_t cols, size_t r0, size_t r1, int connectivity)
{
    const size_t rows = r1 - r0, total = rows * cols;
    Labels l{std::vector<uint32_t>(total, kUfUnset), std::vector<uint32_t>(total, 0u)};
    for (size_t i = 0; i < total; ++i)
        if (set[r0 * cols + i]) l.parent[i] = (uint32_t)i;
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) {
            const uint32_t me = (uint32_t)(r * cols + c);
            if (l.parent[me] == kUfUnset) continue;
            auto join = [&](long rr, long cc) {
                if (rr < 0 || cc < 0 || cc >= (long)cols) return;
                const uint32_t o = (uint32_t)((size_t)rr * cols + (size_t)cc);
                if (l.parent[o] != kUfUnset) gs_uf_unite(l.parent.data(), me, o);
            };
            join((long)r, (long)c - 1);
            join((long)r - 1, (long)c);
            if (connectivity == 8) join((long)r - 1, (long)c - 1), join((long)r - 1, (long)c + 1);
        }
    for (size_t i = 0; i < total; ++i) {
        if (l.parent[i] == kUfUnset) continue;
        l.parent[i] = gs_uf_find(l.parent.data(), (uint32_t)i);
        l.size[l.parent[i]] += 1;
    }
    return l;
}

struct SlabList {
    std::vector<gs_component_record> records; // rows local to the slab; only size and the first cell matter to the merge's order
    std::vector<uint32_t> index;              // per cell's ROOT: the record index, or kCompUnset
    std::vector<uint32_t> first_index, last_index;
};

SlabList list_rows(const Labels &l, size_t cols, size_t rows, uint64_t min_size, bool open)
{
    const size_t total = rows * cols;
    std::vector<unsigned char> listed(total, 0);
    for (size_t i = 0; open && i < total; ++i)
        if (l.parent[i] != kUfUnset && (i / cols == 0 || i / cols == rows - 1)) listed[l.parent[i]] = 1;
    SlabList out;
    out.index.assign(total, gsi::kCompUnset);
    for (size_t i = 0; i < total; ++i)
        if (l.parent[i] == i && (l.size[i] >= min_size || listed[i])) {
            out.index[i] = (uint32_t)out.records.size();
            const uint32_t r = (uint32_t)(i / cols), c = (uint32_t)(i % cols);
            out.records.push_back(gs_component_record{l.size[i], 0, 0, r, c, r, r, c, c});
        }
    for (size_t c = 0; c < cols; ++c) {
        const uint32_t a = l.parent[c], b = l.parent[(rows - 1) * cols + c];
        out.first_index.push_back(a == kUfUnset ? gsi::kCompUnset : out.index[a]);
        out.last_index.push_back(b == kUfUnset ? gsi::kCompUnset : out.index[b]);
    }
    return out;
}

struct Match {
    std::vector<gs_component_record> before, after;
    std::vector<gs_component_overlap> overlaps;
};

// Rows [r0, r1) of the two planes as a slab of its own: both lists and the raw overlaps, as the slab counts rows and records.
void match_rows(const Plane &b, const Plane &a, size_t r0, size_t r1, int connectivity, uint64_t min_size, bool chain, SlabList &lb,
                SlabList &la, std::vector<gs_component_overlap> &raw)
{
    const size_t cols = b.cols, rows = r1 - r0;
    std::vector<unsigned char> both(b.set.size());
    for (size_t i = 0; i < both.size(); ++i) both[i] = b.set[i] && a.set[i];
    const Labels xb = label_rows(b.set, cols, r0, r1, connectivity), xa = label_rows(a.set, cols, r0, r1, connectivity);
    const Labels xp = label_rows(both, cols, r0, r1, connectivity);
    lb = list_rows(xb, cols, rows, min_size, chain);
    la = list_rows(xa, cols, rows, min_size, chain);
    for (size_t i = 0; i < rows * cols; ++i) { // what gs_match_pairs_k writes, in first-cell order
        if (xp.parent[i] != i) continue;
        const uint32_t ib = lb.index[xb.parent[i]], ia = la.index[xa.parent[i]];
        const bool listed = ib != gsi::kCompUnset && ia != gsi::kCompUnset;
        raw.push_back(gs_component_overlap{listed ? ib : gsi::kCompUnset, listed ? ia : gsi::kCompUnset, xp.size[i]});
    }
}

Match match_cut(const Plane &b, const Plane &a, const std::vector<size_t> &cuts, int connectivity, uint64_t min_size)
{
    const size_t nslab = cuts.size() - 1, cols = b.cols;
    std::vector<SlabList> lb(nslab), la(nslab);
    std::vector<std::vector<gs_component_overlap>> raw(nslab);
    for (size_t s = 0; s < nslab; ++s) {
        match_rows(b, a, cuts[s], cuts[s + 1], connectivity, min_size, nslab > 1, lb[s], la[s], raw[s]);
        gsi::records_to_global_rows(lb[s].records.data(), lb[s].records.size(), cuts[s]);
        gsi::records_to_global_rows(la[s].records.data(), la[s].records.size(), cuts[s]);
    }
    Match m;
    std::vector<uint32_t> where[2];
    for (int k = 0; k < 2; ++k) {
        const std::vector<SlabList> &side = k ? la : lb;
        std::vector<const gs_component_record *> part;
        std::vector<size_t> n;
        std::vector<gsi::ListSeamRows> seam;
        for (const SlabList &s : side) {
            part.push_back(s.records.data());
            n.push_back(s.records.size());
            seam.push_back({s.first_index.data(), s.last_index.data()});
        }
        (k ? m.after : m.before) =
            gsi::merge_component_lists(part.data(), n.data(), seam.data(), nslab, cols, connectivity, min_size, &where[k]);
    }
    std::vector<gs_component_overlap> all;
    int64_t base[2] = {0, 0};
    for (size_t s = 0; s < nslab; ++s) {
        gsi::map_overlaps(raw[s].data(), raw[s].size(), where[0].data(), base[0], where[1].data(), base[1]);
        all.insert(all.end(), raw[s].begin(), raw[s].end());
        base[0] += (int64_t)lb[s].records.size();
        base[1] += (int64_t)la[s].records.size();
    }
    m.overlaps = gsi::fold_overlaps(all.data(), all.size());
    return m;
}

int failures = 0;

bool same_lists(const std::vector<gs_component_record> &x, const std::vector<gs_component_record> &y)
{
    if (x.size() != y.size()) return false;
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].size != y[i].size || x[i].first_row != y[i].first_row || x[i].first_col != y[i].first_col) return false;
    return true;
}

void check_every_cut(const Plane &b, const Plane &a, const std::string &what)
{
    for (int connectivity : {4, 8})
        for (const uint64_t min_size : {(uint64_t)1, (uint64_t)2, (uint64_t)7}) {
            const Match want = match_cut(b, a, {0, b.rows}, connectivity, min_size);
            // the whole plane's match against its definition: cells counted pair by pair
            uint64_t shared = 0, summed = 0;
            for (size_t i = 0; i < b.set.size(); ++i) shared += b.set[i] && a.set[i];
            for (size_t i = 0; i < want.overlaps.size(); ++i) {
                summed += want.overlaps[i].cells;
                if (i > 0 && !gsi::overlap_before(want.overlaps[i - 1], want.overlaps[i])) ++failures;
                if (want.overlaps[i].cells == 0 || want.overlaps[i].before >= want.before.size() ||
                    want.overlaps[i].after >= want.after.size())
                    ++failures;
            }
            if (min_size == 1 && summed != shared) {
                ++failures;
                std::fprintf(stderr, "%s: the overlaps hold %llu cells, the planes share %llu\n", what.c_str(),
                             (unsigned long long)summed, (unsigned long long)shared);
            }
            for (size_t nslab = 2; nslab <= 5 && nslab <= b.rows; ++nslab) {
                std::vector<size_t> even, top, bottom; // equal as can be; one-row slabs first; one-row slabs last
                for (size_t s = 0; s <= nslab; ++s) {
                    even.push_back(s * b.rows / nslab);
                    top.push_back(s < nslab ? s : b.rows);
                    bottom.push_back(s == 0 ? 0 : b.rows - (nslab - s));
                }
                for (const std::vector<size_t> *cuts : {&even, &top, &bottom}) {
                    const Match got = match_cut(b, a, *cuts, connectivity, min_size);
                    bool same = same_lists(got.before, want.before) && same_lists(got.after, want.after) &&
                                got.overlaps.size() == want.overlaps.size();
                    for (size_t i = 0; same && i < got.overlaps.size(); ++i)
                        same = got.overlaps[i].before == want.overlaps[i].before && got.overlaps[i].after == want.overlaps[i].after &&
                               got.overlaps[i].cells == want.overlaps[i].cells;
                    if (same) continue;
                    ++failures;
                    std::fprintf(stderr, "%s, %zu slabs, connectivity %d, min_size %llu: %zu overlaps, not the %zu of the whole plane, "
                                         "or others\n", what.c_str(), nslab, connectivity, (unsigned long long)min_size,
                                 got.overlaps.size(), want.overlaps.size());
                }
            }
        }
}

bool same_overlaps(const gs_component_overlap *x, size_t n, const std::vector<gs_component_overlap> &y)
{
    if (n != y.size()) return false;
    for (size_t i = 0; i < n; ++i)
        if (x[i].before != y[i].before || x[i].after != y[i].after || x[i].cells != y[i].cells) return false;
    return true;
}

// The pairs as one batch: every pair matched alone; its records one list after the other with the first cells' rows counted
// over the stack, its pieces with the indices of those stacked lists.
void check_batch(const std::vector<std::pair<Plane, Plane>> &pairs, int connectivity, uint64_t min_size, const std::string &what)
{
    const size_t planes = pairs.size(), rows = pairs[0].first.rows;
    std::vector<Match> want;
    std::vector<gs_component_record> rec[2];
    std::vector<gs_component_overlap> raw;
    for (size_t p = 0; p < planes; ++p) {
        SlabList l[2];
        std::vector<gs_component_overlap> pieces;
        match_rows(pairs[p].first, pairs[p].second, 0, rows, connectivity, min_size, false, l[0], l[1], pieces);
        want.push_back(match_cut(pairs[p].first, pairs[p].second, {0, rows}, connectivity, min_size));
        for (gs_component_overlap o : pieces) {
            if (o.before != gsi::kCompUnset) o.before += (uint32_t)rec[0].size(), o.after += (uint32_t)rec[1].size();
            raw.push_back(o);
        }
        for (int k = 0; k < 2; ++k)
            for (gs_component_record r : l[k].records) {
                r.first_row += (uint32_t)(p * rows);
                rec[k].push_back(r);
            }
    }
    std::vector<uint64_t> before[2];
    for (int k = 0; k < 2; ++k) gsi::batch_records_to_planes(rec[k].data(), rec[k].size(), rows, planes, before[k]);
    std::vector<gs_component_overlap> got;
    std::vector<uint64_t> count(planes, 0);
    gsi::fold_batch_overlaps(raw.data(), raw.size(), before[0].data(), before[1].data(), planes, got, count.data());
    size_t at = 0;
    bool same = true;
    for (size_t p = 0; same && p < planes; ++p) {
        same = at + count[p] <= got.size() && same_overlaps(got.data() + at, (size_t)count[p], want[p].overlaps) &&
               before[0][p + 1] - before[0][p] == want[p].before.size() && before[1][p + 1] - before[1][p] == want[p].after.size();
        at += (size_t)count[p];
    }
    if (same && at == got.size()) return;
    ++failures;
    std::fprintf(stderr, "%s, connectivity %d, min_size %llu: a batch of %zu pairs does not come apart into its pairs' matches\n",
                 what.c_str(), connectivity, (unsigned long long)min_size, planes);
}

Plane blank(size_t rows, size_t cols) { return Plane{rows, cols, std::vector<unsigned char>(rows * cols, 0)}; }

Plane random_plane(size_t rows, size_t cols, double density, unsigned seed)
{
    Plane p = blank(rows, cols);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (auto &x : p.set) x = u(rng) < density ? 1 : 0;
    return p;
}

Plane u_shape(size_t rows, size_t cols) // both arms cross every seam; joined in the last row
{
    Plane p = blank(rows, cols);
    for (size_t r = 0; r < rows; ++r) p.set[r * cols + 1] = p.set[r * cols + cols - 2] = 1;
    for (size_t c = 1; c + 1 < cols; ++c) p.set[(rows - 1) * cols + c] = 1;
    return p;
}

Plane bar(size_t rows, size_t cols, size_t row) // one full row
{
    Plane p = blank(rows, cols);
    for (size_t c = 0; c < cols; ++c) p.set[row * cols + c] = 1;
    return p;
}

Plane column(size_t rows, size_t cols, size_t col)
{
    Plane p = blank(rows, cols);
    for (size_t r = 0; r < rows; ++r) p.set[r * cols + col] = 1;
    return p;
}

} // namespace

int main()
{
    // a U against a bar through its arms: ONE overlap made of two pieces, whatever the cut
    {
        const Plane u = u_shape(11, 9), b = bar(11, 9, 3);
        const Match m = match_cut(u, b, {0, 11}, 4, 1);
        if (m.overlaps.size() != 1 || m.overlaps[0].cells != 2 || m.overlaps[0].before != 0 || m.overlaps[0].after != 0) ++failures;
        check_every_cut(u, b, "U against a bar");
        check_every_cut(b, u, "a bar against a U");
    }
    // a column against itself: every slab's piece is smaller than min_size 7, the merged component is not
    check_every_cut(column(9, 5, 2), column(9, 5, 2), "a column against itself");
    check_every_cut(column(9, 5, 2), bar(9, 5, 4), "a column against a bar");
    check_every_cut(random_plane(6, 7, 1.1, 3), random_plane(6, 7, 1.1, 3), "full against full");
    check_every_cut(random_plane(6, 7, 1.1, 3), random_plane(6, 7, -1.0, 4), "full against empty");
    check_every_cut(random_plane(1, 17, 0.6, 1), random_plane(1, 17, 0.6, 2), "one row");
    check_every_cut(random_plane(9, 1, 0.6, 1), random_plane(9, 1, 0.6, 2), "one column");
    unsigned seed = 10;
    for (const double density : {0.3, 0.5, 0.59, 0.8})
        for (const auto &shape : {std::pair<size_t, size_t>{5, 5}, {13, 21}, {30, 17}, {8, 64}}) {
            const Plane b = random_plane(shape.first, shape.second, density, seed), a = random_plane(shape.first, shape.second, density, seed + 100);
            ++seed;
            check_every_cut(b, a, "random " + std::to_string(density));
            check_every_cut(b, b, "random " + std::to_string(density) + " against itself");
        }
    // batches of 1..4 pairs of one shape; bit p of `eb` (`ea`): pair p's before-plane (after-plane) has no set cell -- every
    // choice, so the first, the last and neighbouring planes with an empty before-list or after-list; min_size 7 also empties
    // lists of planes that have set cells, whose pieces are then all dropped marks
    for (const auto &shape : {std::pair<size_t, size_t>{6, 9}, {1, 17}})
        for (size_t count = 1; count <= 4; ++count)
            for (unsigned eb = 0; eb < (1u << count); ++eb)
                for (unsigned ea = 0; ea < (1u << count); ++ea) {
                    std::vector<std::pair<Plane, Plane>> batch;
                    for (size_t p = 0; p < count; ++p, seed += 2)
                        batch.push_back({random_plane(shape.first, shape.second, (eb >> p) & 1 ? -1.0 : 0.55, seed),
                                         random_plane(shape.first, shape.second, (ea >> p) & 1 ? -1.0 : 0.55, seed + 1)});
                    for (int connectivity : {4, 8})
                        for (const uint64_t min_size : {(uint64_t)1, (uint64_t)2, (uint64_t)7})
                            check_batch(batch, connectivity, min_size, "batch, empty before " + std::to_string(eb) + ", after " + std::to_string(ea));
                }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
