// gs_match_merge.h -- the host side of gs_fields_match and gs_members_match (gs_observe.cpp) as functions of plain arrays: no
// device, no context, so that it can be tested on its own (tests/cpp/match_merge.cpp).
//
// The device leaves one RAW overlap per piece -- a connected piece of the cells set in both planes --: the indices of the
// before-record and the after-record it lies in, as the slab (or batch) that formed it counts its records, and the piece's
// cells; both indices are kCompUnset (a dropped mark) where either component is not listed.
//   map_overlaps   turns local indices into those of the plane's final lists: with `where` tables (a slab chain: what
//                  merge_component_lists says became of every slab-local record, gs_components_merge.h) through the table,
//                  offset by the slab's base; a record that fell below min_size after the seam merge maps to kCompUnset, and
//                  the overlap becomes a dropped mark.  Without a table an index moves by `shift` alone (a batch of members:
//                  minus the records of the planes before).
//   fold_overlaps  drops the marks, sorts by (before, after) and adds the cells of equal pairs: two pieces of one pair -- a
//                  U against a bar --, and pieces cut by a seam, become ONE overlap.
//   fold_batch_overlaps  cuts the raw overlaps of a batch of members into the batch's planes and maps and folds each plane's.
// Integers throughout: the result does not depend on the order in which the pieces arrive.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "gs_components_merge.h"

namespace gsi {

// o[0 .. n): before -> where_b[base_b + before] (or before - base_b without a table), after likewise.
inline void map_overlaps(gs_component_overlap *o, size_t n, const uint32_t *where_b, int64_t base_b, const uint32_t *where_a,
                         int64_t base_a)
{
    for (size_t k = 0; k < n; ++k) {
        if (o[k].before == kCompUnset || o[k].after == kCompUnset) {
            o[k].before = o[k].after = kCompUnset;
            continue;
        }
        const uint32_t b = where_b ? where_b[(size_t)(base_b + (int64_t)o[k].before)] : (uint32_t)((int64_t)o[k].before - base_b);
        const uint32_t a = where_a ? where_a[(size_t)(base_a + (int64_t)o[k].after)] : (uint32_t)((int64_t)o[k].after - base_a);
        const bool kept = b != kCompUnset && a != kCompUnset;
        o[k].before = kept ? b : kCompUnset;
        o[k].after = kept ? a : kCompUnset;
    }
}

inline bool overlap_before(const gs_component_overlap &x, const gs_component_overlap &y)
{
    return x.before != y.before ? x.before < y.before : x.after < y.after;
}

// The overlaps of one plane, indices already final.
inline std::vector<gs_component_overlap> fold_overlaps(const gs_component_overlap *o, size_t n)
{
    std::vector<gs_component_overlap> out;
    out.reserve(n);
    for (size_t k = 0; k < n; ++k)
        if (o[k].before != kCompUnset && o[k].after != kCompUnset) out.push_back(o[k]);
    std::sort(out.begin(), out.end(), overlap_before);
    size_t w = 0;
    for (size_t k = 0; k < out.size(); ++k) {
        if (w > 0 && out[w - 1].before == out[k].before && out[w - 1].after == out[k].after)
            out[w - 1].cells += out[k].cells;
        else
            out[w++] = out[k];
    }
    out.resize(w);
    return out;
}

// raw[0 .. n): the raw overlaps of a batch of `planes` planes, indices as the batch counts its records.  The pieces come in
// first-cell order, so plane after plane; a kept piece's plane is that of its before-record: before[p] (after[p]) is the
// number of the batch's before-records (after-records) in the planes before plane p, planes + 1 entries each
// (batch_records_to_planes).  Plane p's overlaps, with the indices of the plane's own two lists and folded, are added to the
// end of `out`, and their number to count[p].
inline void fold_batch_overlaps(gs_component_overlap *raw, size_t n, const uint64_t *before, const uint64_t *after, size_t planes,
                                std::vector<gs_component_overlap> &out, uint64_t *count)
{
    size_t at = 0;
    for (size_t p = 0; p < planes; ++p) {
        const size_t from = at;
        while (at < n && (raw[at].before == kCompUnset || raw[at].before < before[p + 1])) ++at;
        map_overlaps(raw + from, at - from, nullptr, (int64_t)before[p], nullptr, (int64_t)after[p]);
        const std::vector<gs_component_overlap> folded = fold_overlaps(raw + from, at - from);
        out.insert(out.end(), folded.begin(), folded.end());
        count[p] += folded.size();
    }
}

} // namespace gsi
