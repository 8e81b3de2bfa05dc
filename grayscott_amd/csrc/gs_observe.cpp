// gs_observe.cpp -- results formed on the device from planes and ensemble members, without downloading them
// (include/gs_hip.h): summaries (gs_fields_summarize, gs_members_summarize), histograms (gs_fields_histogram,
// gs_members_histogram), bit-quad counts (gs_fields_morphology, gs_members_morphology), two-point pair counts
// (gs_fields_correlation, gs_members_correlation), connected components (gs_fields_components, gs_members_components) and
// component lists (gs_field_component_list, gs_members_component_list), component matches of two states (gs_fields_match,
// gs_members_match) and comparisons of two states (gs_fields_compare, gs_members_compare).  All observe a field list with launches per slab on its
// compute stream into that slab's scratch buffer, fetch what the launches left and combine it here on the host, after the
// results of every slab -- and, in a multi-process context, of every rank (exchange) -- have met; an ensemble's members are
// observed in one launch on slab 0.  Three shapes of result, each with one path:
//   banded results  results per (plane, band of rows), gathered as [plane][band] over slabs and ranks (band_results): a record
//                 per row, folded here in ascending global row order -- summaries, comparisons --, or the regions' results.
//   u64 counters  zeroed, added to by the launch (the plane scans of gs_plane_scan.h), fetched and added over slabs and ranks
//                 (slab_counters; an ensemble's member range: member_counters) -- integers, so the order of the additions
//                 does not show: histograms, morphology, correlations.  A stencil's rows above a slab's first row are staged
//                 into the slab's scratch buffer behind the counters (stage_rows_above), never read from ghost rows.
//   listed records  a record per component of a labelling: counted, read back, record memory sized exactly, filled, fetched
//                 -- over a field's slab chain (ChainListing: the host joins what crosses a seam) or a batch of members
//                 (BatchListing: the host takes the records apart by plane): component lists, both sides of a match.  The
//                 host steps on plain arrays are in gs_components_merge.h and gs_match_merge.h, tested without a device.
// Components keep a slab loop of their own (label memory, seam rows, the ranks' verdict) over the same small helpers.
//   summaries   row records from gs_row_summary_k (gs_summary.hip); the field fold -- rows added in ascending global row
//               order -- is done on the host.  Ensembles fold on the device (gs_summary_fold_k): two records per member travel.
//   histograms  counters of gs_plane_hist_k (gs_histogram.hip).
//   morphology  counters of gs_plane_quads_k (gs_morphology.hip), a stencil with one row staged above a slab.
//   correlations counters of gs_plane_pairs_k (gs_correlation.hip), a stencil with L rows staged above a slab.
//   components  labelled slab by slab (gs_components.hip) in label memory that lives for the call alone; the counters and the
//               (root, size) of every slab's first and last row meet on the host, which joins what crosses the seams
//               (gs_components_merge.h).
//   component lists  the same labelling, then one record per component formed behind it (gs_component_list.hip) in record
//               memory that lives for the call alone; the records and the record indices of every slab's first and last row
//               meet on the host, which joins what crosses the seams (gs_components_merge.h).  Single-process contexts only.
//   component matches  both planes labelled and listed as above, each in label memory of its own, then the pieces they share
//               labelled from the two label arrays and one overlap written per piece (gs_match.hip); the host makes the
//               indices global and adds the cells of equal pairs (gs_match_merge.h).  Single-process contexts only.
//   comparisons row records from gs_row_change_k (gs_change.hip) of pairs of planes, gathered and folded like the summaries'
//               (band_results); ensembles fold on the device (gs_change_fold_k).
//   regional observables  summaries and bit-quad counts of every region of rh x rw cells of a plane (gs_fields_region_summaries,
//               gs_fields_region_morphology; gs_regions.hip): one launch per slab leaves a record or a set of counters per
//               (plane, region) -- a region lies inside one slab, so nothing is staged and nothing is folded on the host --
//               and the slabs' and ranks' region rows meet in the global [plane][region] layout (band_results).  The regions'
//               two-point pair counts (gs_fields_region_correlation; gs_region_pairs.hip) travel the same way.
//               The regions' histograms (gs_fields_region_histogram; gs_region_hist.hip) do too: bins + 3 counters per region.
//               The regions' components (gs_fields_region_components; gs_region_components.hip) are labelled slab by slab in
//               label memory that lives for the call alone, the regions' borders as walls, and tallied per region into the
//               same layout: nt results of 35 counters per region.
//               The regions' changes against a second field list (gs_fields_region_compare; gs_region_change.hip) travel as the
//               summaries do: a gs_change per region, by a wave per region or through row records behind the slab's results.
//   power spectra  (gs_fields_spectrum, gs_members_spectrum; gs_spectrum.hip) a record per segment of 16 tiles behind the slab's
//               results, added per band of T rows on the device: one result per band travels (band_results) and the host adds
//               the bands in ascending global order; an ensemble's members are planes of one launch, their bands added here too.
//               The regions' spectra (gs_fields_region_spectrum; gs_region_spectrum.hip) travel as the regional observables
//               do: a record per segment of a band of a region behind the slab's results, added per region on the device --
//               a region lies inside one slab, so its result is complete -- and one result per region travels
//               (band_results with bands of rh rows); the host only splits each into power and tile counts.
// The device copies that make a state to compare with (gs_fields_copy, gs_members_copy: snapshots and restores) are here too.
// No observation touches ghost rows, the tuner, graphs or the context's counters; a copy leaves its target as an upload does.
#include "gs_internal.h"
#include "gs_components_merge.h"
#include "gs_match_merge.h"

#include <cstdlib>
#include <cstring>
#include <memory>

using namespace gsi;

// What gs_field_component_list and gs_members_component_list return: host memory, independent of the context.
struct gs_component_list {
    uint64_t planes = 0;
    std::vector<uint64_t> offsets; // planes + 1
    std::vector<gs_component_record> records;
};

// What gs_fields_match and gs_members_match return: the two lists and the overlaps, host memory as a list is.
struct gs_component_match {
    gs_component_list before, after;
    std::vector<uint64_t> offsets; // planes + 1
    std::vector<gs_component_overlap> overlaps;
};

namespace gsi {

int32_t ensure_scratch(gs_ctx *ctx, int i, size_t bytes, const char *what)
{
    SlabRt &sl = ctx->slabs[(size_t)i];
    if (sl.scratch_bytes >= bytes) return GS_OK;
    GS_HIP(hipSetDevice(sl.device));
    if (sl.scratch) GS_HIP(hipFree(sl.scratch));
    sl.scratch = nullptr;
    sl.scratch_bytes = 0;
    const hipError_t e = hipMalloc(&sl.scratch, bytes);
    if (e != hipSuccess) return fail(GS_ERR_NOMEM, "%s buffer of %zu bytes: %s", what, bytes, hipGetErrorString(e));
    sl.scratch_bytes = bytes;
    return GS_OK;
}

void destroy_scratch(gs_ctx *ctx)
{
    for (auto &sl : ctx->slabs) {
        if (!sl.scratch) continue;
        if (hipSetDevice(sl.device) == hipSuccess) (void)hipFree(sl.scratch);
        sl.scratch = nullptr;
        sl.scratch_bytes = 0;
    }
}

int32_t check_planes(gs_ctx *ctx, gs_field *const *fields, int32_t n, gs_field *const *others)
{
    if (n < 1 || n > 4) return fail(GS_ERR_INVALID, "%d fields (1..4)", n);
    for (int32_t p = 0; p < n; ++p) {
        if (!fields[p] || fields[p]->ctx != ctx) return fail(GS_ERR_INVALID, "field %d: null or of another context", p);
        if (p > 0) GS_TRY(same_shape(fields[0], fields[p]));
    }
    for (int32_t p = 0; others && p < n; ++p) {
        if (!others[p] || others[p]->ctx != ctx) return fail(GS_ERR_INVALID, "second field %d: null or of another context", p);
        GS_TRY(same_shape(fields[0], others[p]));
    }
    return sync_all(ctx); // (also runs again a persistent window launch that gave up: no stale plane is read)
}

} // namespace gsi

namespace {

// An ensemble of this context, a member range inside it -- `other`, if given: a second ensemble of this context with the
// same shape and member count -- and then every stream idle.
int32_t check_members(gs_ctx *ctx, const gs_ensemble *e, uint64_t first, uint64_t count, const gs_ensemble *other = nullptr,
                      bool two = false)
{
    if (!e || (two && !other)) return fail(GS_ERR_INVALID, "null argument");
    if (e->ctx != ctx || (other && other->ctx != ctx)) return fail(GS_ERR_INVALID, "ensemble belongs to another context");
    GS_TRY(check_member_range(e, first, count));
    if (other && (other->members != e->members || other->rows != e->rows || other->cols != e->cols))
        return fail(GS_ERR_INVALID, "ensembles of %llu x [%llu, %llu] and %llu x [%llu, %llu]", (unsigned long long)e->members,
                    (unsigned long long)e->rows, (unsigned long long)e->cols, (unsigned long long)other->members,
                    (unsigned long long)other->rows, (unsigned long long)other->cols);
    return sync_all(ctx);
}

// Slab i's planes of a field list.
void slab_planes(gs_field *const *fields, int32_t n, size_t i, const float *out[4])
{
    for (int32_t p = 0; p < 4; ++p) out[p] = p < n ? fields[p]->s[i].row0 : nullptr;
}

// U and V of member `first` in the newest state: member first + i's are `cells` floats further on, each a plane of its own.
void member_planes(const gs_ensemble *e, uint64_t first, const float *out[2])
{
    const uint64_t cells = e->rows * e->cols;
    out[0] = e->u[e->cur] + first * cells;
    out[1] = e->v[e->cur] + first * cells;
}

// Rows of slab k of the S slabs of all processes that R global rows are split into (the partition of gs_field_create).
uint64_t global_slab_rows(const gs_ctx *ctx, uint64_t R, uint64_t k)
{
    const uint64_t S = (uint64_t)ctx->total_slabs();
    return (k + 1) * R / S - k * R / S;
}

// Several processes: every rank's bytes to every rank's host.  `bytes[q]` is rank q's share (the same table on every
// rank), `mine` this rank's own; `all` receives the shares in rank order.  Through slab 0's scratch buffer as send | recv,
// on its compute stream, which is idle again on return.
int32_t exchange(gs_ctx *ctx, const void *mine, const std::vector<size_t> &bytes, const char *what, void *all)
{
    size_t total = 0;
    for (const size_t b : bytes) total += b;
    const size_t own = bytes[(size_t)ctx->rank];
    SlabRt &sl = ctx->slabs[0];
    GS_TRY(ensure_scratch(ctx, 0, own + total, what));
    GS_HIP(hipSetDevice(sl.device));
    unsigned char *send = static_cast<unsigned char *>(sl.scratch), *recv = send + own;
    GS_HIP(hipMemcpyAsync(send, mine, own, hipMemcpyHostToDevice, sl.compute));
    GS_TRY(allgather_bytes(ctx, send, recv, bytes, sl.compute));
    GS_HIP(hipMemcpyAsync(all, recv, total, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    return GS_OK;
}

// Banded results of n planes (or pairs of planes) of f0's shape over the WHOLE global grid: a band is rh rows, and every band
// of every plane has RC results of `elem` bytes, gathered as [plane][band][result] into `all` (n * RR * RC * elem bytes, RR
// the bands of the grid).  One launch per slab on its compute stream into the slab's scratch buffer -- zeroed first for
// counters; `launch(slab, results, stream)` leaves results[(p * bands_of_the_slab + i) * RC + j] -- and, in a multi-process
// context, every rank's results to every rank (rank q holds the bands of global slabs [q L, (q + 1) L)).  Every slab of the
// global grid must begin at a multiple of rh rows (the precedent of reduced images): a band then lies inside one slab, slab
// k's bands are [start_k / rh, ...) of the grid's, no ghost row is read and no row is staged; every rank reaches the same
// verdict.  Row records -- summaries, comparisons, which fold `all` plane by plane in ascending global row order -- are bands
// of one row with one 32-byte result, for which that refusal cannot fire; regions are bands of rh rows with RC results.
// band_results' refusal: every slab of the global grid begins at a multiple of rh rows, on every rank the same verdict.
int32_t check_band_seams(const gs_ctx *ctx, const gs_field *f0, int32_t rh)
{
    const uint64_t q = (uint64_t)rh, S = (uint64_t)ctx->total_slabs(), R = f0->rows;
    for (uint64_t k = 1; k < S; ++k)
        if ((k * R / S) % q != 0)
            return fail(GS_ERR_UNSUPPORTED, "slab %llu begins at row %llu, which is not a multiple of the region height %d "
                                            "(a region may not straddle two slabs)",
                        (unsigned long long)k, (unsigned long long)(k * R / S), rh);
    return GS_OK;
}

template <typename Launch>
int32_t band_results(gs_ctx *ctx, const gs_field *f0, int32_t n, int32_t rh, uint64_t RR, uint64_t RC, size_t elem, bool zeroed,
                     const char *what, unsigned char *all, Launch launch)
{
    GS_TRY(check_band_seams(ctx, f0, rh));
    const uint64_t q = (uint64_t)rh, R = f0->rows;
    const size_t nslab = ctx->slabs.size(), line = (size_t)RC * elem; // (line: one band of one plane)
    auto bands_of = [&](uint64_t rows) { return (size_t)((rows + q - 1) / q); };
    size_t local_bands = 0;
    for (const FieldSlab &fs : f0->s) local_bands += bands_of((uint64_t)fs.rows);
    std::vector<unsigned char> gathered;
    unsigned char *local = all; // one process: its bands are the grid's
    if (ctx->world > 1) {
        gathered.resize((size_t)n * local_bands * line);
        local = gathered.data();
    }
    size_t at = 0;
    for (size_t i = 0; i < nslab; ++i) {
        SlabRt &sl = ctx->slabs[i];
        const size_t nb = bands_of((uint64_t)f0->s[i].rows);
        if (nb == 0) continue;
        GS_TRY(ensure_scratch(ctx, (int)i, (size_t)n * nb * line, what));
        GS_HIP(hipSetDevice(sl.device));
        unsigned char *dev = static_cast<unsigned char *>(sl.scratch);
        if (zeroed) GS_HIP(hipMemsetAsync(dev, 0, (size_t)n * nb * line, sl.compute));
        GS_HIP(launch(i, dev, sl.compute));
        for (int32_t p = 0; p < n; ++p)
            GS_HIP(hipMemcpyAsync(local + ((size_t)p * local_bands + at) * line, dev + (size_t)p * nb * line, nb * line,
                                  hipMemcpyDeviceToHost, sl.compute));
        at += nb;
    }
    GS_TRY(sync_compute(ctx));
    if (ctx->world == 1) return GS_OK;
    const uint64_t L = (uint64_t)nslab;
    std::vector<size_t> bytes((size_t)ctx->world, (size_t)0);
    for (uint64_t k = 0; k < (uint64_t)ctx->world * L; ++k)
        bytes[(size_t)(k / L)] += (size_t)n * bands_of(global_slab_rows(ctx, R, k)) * line;
    if (bytes[(size_t)ctx->rank] != gathered.size())
        return fail(GS_ERR_INVALID, "row partition disagrees with this process's slabs");
    std::vector<unsigned char> blocks((size_t)n * (size_t)RR * line);
    GS_TRY(exchange(ctx, gathered.data(), bytes, what, blocks.data()));
    // rank blocks in rank order, each [plane][its bands]: plane p's bands in global order
    for (int32_t p = 0; p < n; ++p) {
        size_t from = 0, row = 0;
        for (int r = 0; r < ctx->world; ++r) {
            const size_t nb = bytes[(size_t)r] / line / (size_t)n;
            std::memcpy(all + ((size_t)p * (size_t)RR + row) * line, blocks.data() + from + (size_t)p * nb * line, nb * line);
            from += (size_t)n * nb * line;
            row += nb;
        }
    }
    return GS_OK;
}

// ---- summaries -------------------------------------------------------------------------------------------------------
static_assert(sizeof(GsRowSummary) == 32, "row record layout");
static_assert(sizeof(gs_summary) == 32 && offsetof(gs_summary, min) == 16 && offsetof(gs_summary, nonfinite) == 24,
              "gs_summary layout");

gs_summary empty_summary()
{
    gs_summary s;
    s.sum = 0.0;
    s.sum_sq = 0.0;
    s.min = HUGE_VALF;
    s.max = -HUGE_VALF;
    s.nonfinite = 0;
    return s;
}

// Rows added one after the other in the order given, from +0.0.
gs_summary fold_rows(const GsRowSummary *rec, size_t rows)
{
    gs_summary s = empty_summary();
    for (size_t r = 0; r < rows; ++r) {
        const GsRowSummary &x = rec[r];
        s.sum = s.sum + x.sum;
        s.sum_sq = s.sum_sq + x.sum_sq;
        s.min = std::fmin(s.min, x.min);
        s.max = std::fmax(s.max, x.max);
        s.nonfinite += x.nonfinite;
    }
    return s;
}

gs_summary from_record(const GsRowSummary &x)
{
    gs_summary s;
    s.sum = x.sum;
    s.sum_sq = x.sum_sq;
    s.min = x.min;
    s.max = x.max;
    s.nonfinite = x.nonfinite;
    return s;
}

// ---- comparisons -----------------------------------------------------------------------------------------------------
static_assert(sizeof(GsRowChange) == 32, "row record layout");
static_assert(sizeof(gs_change) == 40 && sizeof(GsChangeTotal) == 40 && offsetof(gs_change, max_abs) == 16 &&
                  offsetof(gs_change, differing) == 24 && offsetof(gs_change, nonfinite) == 32,
              "gs_change layout");

gs_change no_change()
{
    gs_change c;
    c.sum_abs = 0.0;
    c.sum_sq = 0.0;
    c.max_abs = 0.0;
    c.differing = 0;
    c.nonfinite = 0;
    return c;
}

// Rows added one after the other in the order given, from +0.0.
gs_change fold_rows(const GsRowChange *rec, size_t rows)
{
    gs_change c = no_change();
    for (size_t r = 0; r < rows; ++r) {
        const GsRowChange &x = rec[r];
        c.sum_abs = c.sum_abs + x.sum_abs;
        c.sum_sq = c.sum_sq + x.sum_sq;
        c.max_abs = std::fmax(c.max_abs, x.max_abs);
        c.differing += x.differing;
        c.nonfinite += x.nonfinite;
    }
    return c;
}

// ---- histograms ------------------------------------------------------------------------------------------------------
constexpr int kHistGroupsPerCu = 8; // workgroups of 4 waves a launch may put on a CU: 8 x (4096 + 4) u32 of LDS fit in 160 KiB

// The rule's scale for n ranges, (float)bins / (hi - lo) in f32, or the refusal of gs_hip.h.  No handle is looked at.
int32_t check_ranges(const float *lo, const float *hi, int32_t n, int32_t bins, float *scale)
{
    if (bins < 1 || bins > 4096) return fail(GS_ERR_INVALID, "%d bins (1..4096)", bins);
    for (int32_t i = 0; i < n; ++i) {
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || !(lo[i] < hi[i]))
            return fail(GS_ERR_INVALID, "range %d: [%g, %g] is not lo < hi, both finite", i, (double)lo[i], (double)hi[i]);
        const volatile float width = hi[i] - lo[i]; // (volatile: one f32 subtraction, one f32 division, whatever the host's flags)
        const volatile float s = (float)bins / width;
        if (!std::isnormal(width) || !(width > 0.0f) || !std::isnormal(s) || !(s > 0.0f))
            return fail(GS_ERR_INVALID, "range %d: the width %g of [%g, %g] or the scale %g for %d bins is no normal positive f32",
                        i, (double)width, (double)lo[i], (double)hi[i], (double)s, bins);
        scale[i] = s;
    }
    return GS_OK;
}

int64_t max_groups(const gs_ctx *ctx)
{
    return (int64_t)kHistGroupsPerCu * (ctx->cu_count > 0 ? ctx->cu_count : 256);
}

// ---- morphology ------------------------------------------------------------------------------------------------------
static_assert(sizeof(gs_morphology) == 48, "gs_morphology layout");
constexpr size_t kQuadCounted = 5; // the classes gs_plane_quads_k counts: Q1, Q2, Q3, Q4, QD

// nt thresholds for each of n planes, or the refusal of gs_hip.h: what every thresholded observable checks first.  No handle
// is looked at; a count of planes that is no 1..4 is left to check_planes, whose first refusal it is.
int32_t check_thresholds(const float *thresholds, int32_t n, int32_t nt)
{
    if (nt < 1 || nt > 4) return fail(GS_ERR_INVALID, "%d thresholds (1..4)", nt);
    if (n < 1 || n > 4) n = 0;
    for (int32_t i = 0; i < n * nt; ++i)
        if (std::isnan(thresholds[i])) return fail(GS_ERR_INVALID, "threshold %d of plane %d is NaN", i % nt, i / nt);
    return GS_OK;
}

// The largest lag of a correlation, or the refusal of gs_hip.h.  No handle is looked at.
int32_t check_max_lag(int32_t max_lag)
{
    if (max_lag < 1 || max_lag > 64) return fail(GS_ERR_INVALID, "a largest lag of %d (1..64)", max_lag);
    return GS_OK;
}

// The counted classes of one (plane, threshold) and the complement Q0 of a plane of rows x cols cells.
gs_morphology from_counted(const uint64_t *c, uint64_t rows, uint64_t cols)
{
    gs_morphology m;
    for (size_t k = 0; k < kQuadCounted; ++k) m.quads[1 + k] = c[k];
    m.quads[0] = (rows + 1) * (cols + 1) - (c[0] + c[1] + c[2] + c[3] + c[4]);
    return m;
}

// ---- stencils over slabs: morphology, correlation ------------------------------------------------------------------
// The `depth` global rows above the first row of every slab of this process, of each of n planes, STAGED into the slab's
// scratch buffer behind `counters` bytes (a multiple of 256) as [plane][depth rows][pitch] -- from the slab above inside the
// process (copy_row), from the rank above through `exchange` (every rank's last `depth` rows travel; each rank uploads those
// of the rank above) -- on the slab's compute stream.  Ghost rows are never read, whatever ghost_depth says.  The slab
// that begins at global row 0 has nothing staged.  Every slab above another holds at least `depth` rows (the caller's
// check).  The scratch buffers hold counters + n * depth * pitch floats on return.
int32_t stage_rows_above(gs_ctx *ctx, gs_field *const *fields, int32_t n, size_t depth, size_t counters, const char *what)
{
    const gs_field *f0 = fields[0];
    const size_t nslab = ctx->slabs.size(), pitch = (size_t)f0->pitch, cols = (size_t)f0->cols;
    const size_t block = depth * pitch; // floats of one plane's staged rows
    std::vector<float> upper;           // several processes: the last rows of the rank above, [plane][depth][cols]
    if (ctx->world > 1) {
        const size_t each = (size_t)n * depth * cols, share = each * sizeof(float);
        std::vector<float> mine(each), all((size_t)ctx->world * each);
        SlabRt &sl = ctx->slabs[nslab - 1];
        GS_HIP(hipSetDevice(sl.device));
        for (int32_t p = 0; p < n; ++p) {
            const FieldSlab &fs = fields[p]->s[nslab - 1];
            GS_HIP(hipMemcpy2DAsync(mine.data() + (size_t)p * depth * cols, cols * sizeof(float),
                                    fs.row0 + ((ptrdiff_t)fs.rows - (ptrdiff_t)depth) * (ptrdiff_t)pitch, pitch * sizeof(float),
                                    cols * sizeof(float), depth, hipMemcpyDeviceToHost, sl.compute));
        }
        GS_HIP(hipStreamSynchronize(sl.compute));
        GS_TRY(exchange(ctx, mine.data(), std::vector<size_t>((size_t)ctx->world, share), what, all.data()));
        if (ctx->rank > 0) upper.assign(all.begin() + (ptrdiff_t)((size_t)(ctx->rank - 1) * each),
                                        all.begin() + (ptrdiff_t)((size_t)ctx->rank * each));
    }
    for (size_t i = 0; i < nslab; ++i) {
        SlabRt &sl = ctx->slabs[i];
        GS_TRY(ensure_scratch(ctx, (int)i, counters + (size_t)n * block * sizeof(float), what));
        if (f0->s[i].g_row0 == 0) continue;
        GS_HIP(hipSetDevice(sl.device));
        float *staged = reinterpret_cast<float *>(static_cast<unsigned char *>(sl.scratch) + counters);
        for (int32_t p = 0; p < n; ++p) {
            if (i > 0) { // (every stream is idle: the rows are final, and nobody else uses this slab's scratch buffer)
                // the rows are `pitch` apart on both sides: one copy from the first cell to the last
                const FieldSlab &up = fields[p]->s[i - 1];
                GS_TRY(copy_row(ctx, (int)i - 1, up.row0 + ((ptrdiff_t)up.rows - (ptrdiff_t)depth) * (ptrdiff_t)pitch, (int)i,
                                staged + (size_t)p * block, ((depth - 1) * pitch + cols) * sizeof(float), sl.compute));
            } else {
                GS_HIP(hipMemcpy2DAsync(staged + (size_t)p * block, pitch * sizeof(float), upper.data() + (size_t)p * depth * cols,
                                        cols * sizeof(float), cols * sizeof(float), depth, hipMemcpyHostToDevice, sl.compute));
            }
        }
        // `upper` is pageable and dies with this call: its rows are on the device before it does
        if (i == 0) GS_HIP(hipStreamSynchronize(sl.compute));
    }
    return GS_OK;
}

// `words` u64 counters per slab, [slab][words], added over the slabs and, in a multi-process context, over the ranks
// (every rank's sums to every rank, added in the same way everywhere).  Integers: the order does not show.
int32_t add_counters(gs_ctx *ctx, const std::vector<uint64_t> &part, size_t words, const char *what, uint64_t *sum)
{
    std::fill(sum, sum + words, (uint64_t)0);
    for (size_t i = 0; i < ctx->slabs.size(); ++i)
        for (size_t w = 0; w < words; ++w) sum[w] += part[i * words + w];
    if (ctx->world == 1) return GS_OK;
    std::vector<uint64_t> all((size_t)ctx->world * words);
    GS_TRY(exchange(ctx, sum, std::vector<size_t>((size_t)ctx->world, words * sizeof(uint64_t)), what, all.data()));
    std::fill(sum, sum + words, (uint64_t)0);
    for (int q = 0; q < ctx->world; ++q)
        for (size_t w = 0; w < words; ++w) sum[w] += all[(size_t)q * words + w];
    return GS_OK;
}

// `words` u64 counters of the planes of a field list, added over the slabs and ranks into `out`: per slab its scratch buffer
// is made large enough -- with `depth` > 0 (a stencil) by stage_rows_above, which also leaves the `depth` rows above the
// slab's first row behind the counters --, the counters are zeroed, `launch(i, counters, staged, stream)` adds to them
// (`staged`: [plane][depth rows][pitch], null where nothing is above the slab or depth is 0) and they are fetched.
template <typename Launch>
int32_t slab_counters(gs_ctx *ctx, gs_field *const *fields, int32_t n, size_t words, size_t depth, const char *what,
                      uint64_t *out, Launch launch)
{
    const size_t nslab = ctx->slabs.size(), bytes = words * sizeof(uint64_t);
    const size_t counters = (bytes + 255) / 256 * 256; // (the staged rows start on a 256-byte boundary)
    if (depth) GS_TRY(stage_rows_above(ctx, fields, n, depth, counters, what));
    std::vector<uint64_t> part(nslab * words);
    for (size_t i = 0; i < nslab; ++i) {
        SlabRt &sl = ctx->slabs[i];
        if (!depth) GS_TRY(ensure_scratch(ctx, (int)i, bytes, what));
        GS_HIP(hipSetDevice(sl.device));
        unsigned long long *dev = static_cast<unsigned long long *>(sl.scratch);
        const float *staged = depth && fields[0]->s[i].g_row0 != 0
                                  ? reinterpret_cast<const float *>(static_cast<unsigned char *>(sl.scratch) + counters)
                                  : nullptr;
        GS_HIP(hipMemsetAsync(dev, 0, bytes, sl.compute));
        GS_HIP(launch(i, dev, staged, sl.compute));
        GS_HIP(hipMemcpyAsync(part.data() + i * words, dev, bytes, hipMemcpyDeviceToHost, sl.compute));
    }
    GS_TRY(sync_compute(ctx));
    return add_counters(ctx, part, words, what, out);
}

// `words` u64 counters of members [first, ...) of an ensemble into `host`: one launch on slab 0 -- `launch(planes, counters,
// stream)` with member_planes' planes -- into its scratch buffer, zeroed before and fetched after; zeros for members of no cells.
template <typename Launch>
int32_t member_counters(gs_ctx *ctx, const gs_ensemble *e, uint64_t first, size_t words, const char *what, uint64_t *host,
                        Launch launch)
{
    const size_t bytes = words * sizeof(uint64_t);
    if (e->rows * e->cols == 0) {
        std::fill(host, host + words, (uint64_t)0);
        return GS_OK;
    }
    GS_TRY(ensure_scratch(ctx, 0, bytes, what));
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    unsigned long long *dev = static_cast<unsigned long long *>(sl.scratch);
    const float *planes[2];
    member_planes(e, first, planes);
    GS_HIP(hipMemsetAsync(dev, 0, bytes, sl.compute));
    GS_HIP(launch(planes, dev, sl.compute));
    GS_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    return GS_OK;
}

// ---- connected components ------------------------------------------------------------------------------------------------
static_assert(sizeof(gs_components) == 280 && offsetof(gs_components, by_size) == 24, "gs_components layout");
constexpr size_t kCompWords = sizeof(gs_components) / sizeof(uint64_t); // the counters gs_comp_tally_k adds to

int32_t check_connectivity(int32_t connectivity)
{
    if (connectivity != 4 && connectivity != 8) return fail(GS_ERR_INVALID, "a connectivity of %d (4 or 8)", connectivity);
    return GS_OK;
}

// Label memory of one call: a u32 parent and a u32 size per cell -- and, where a component list asks for them, `marks` u32
// words behind them --, freed when the call returns, however it returns.
struct LabelMemory {
    struct Block {
        int device;
        uint32_t *parent, *size, *marks;
    };
    std::vector<Block> blocks;
    ~LabelMemory()
    {
        for (const Block &b : blocks)
            if (b.parent && hipSetDevice(b.device) == hipSuccess) (void)hipFree(b.parent);
    }
    int32_t add(int device, uint64_t cells, uint64_t marks = 0)
    {
        Block b{device, nullptr, nullptr, nullptr};
        if (cells > 0) {
            GS_HIP(hipSetDevice(device));
            void *p = nullptr;
            const uint64_t bytes = cells * 8 + marks * 4;
            const hipError_t e = hipMalloc(&p, (size_t)bytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(GS_ERR_NOMEM, "label memory of %llu bytes: %s", (unsigned long long)bytes, hipGetErrorString(e));
            }
            b.parent = static_cast<uint32_t *>(p);
            b.size = b.parent + cells;
            b.marks = marks ? b.size + cells : nullptr;
        }
        blocks.push_back(b);
        return GS_OK;
    }
};


// ---- component lists ---------------------------------------------------------------------------------------------------
static_assert(sizeof(gs_component_record) == 48 && sizeof(GsComponentRecord) == 48 && offsetof(gs_component_record, first_row) == 24 &&
                  offsetof(GsComponentRecord, first_row) == 24 && offsetof(gs_component_record, row_min) == 32 &&
                  offsetof(GsComponentRecord, row_min) == 32 && offsetof(gs_component_record, col_max) == 44 &&
                  offsetof(GsComponentRecord, col_max) == 44,
              "gs_component_record layout");

// What a component list checks before any handle is looked at, in the header's order.
int32_t check_list_rule(float threshold, int32_t connectivity, uint64_t min_size)
{
    if (std::isnan(threshold)) return fail(GS_ERR_INVALID, "the threshold is NaN");
    GS_TRY(check_connectivity(connectivity));
    if (min_size == 0) return fail(GS_ERR_INVALID, "a min_size of 0 (at least 1)");
    return GS_OK;
}

// rows * rows * cols or rows * cols * cols >= 2^64: a record's sum of row or column indices could wrap.
int32_t check_list_sums(uint64_t rows, uint64_t cols, bool members)
{
    const unsigned __int128 cells = (unsigned __int128)rows * cols; // (< 2^128)
    if (cells >> 64 ? rows == 0 || cols == 0 : ((cells * rows) >> 64) == 0 && ((cells * cols) >> 64) == 0) return GS_OK;
    return members ? fail(GS_ERR_UNSUPPORTED, "members of %llu x %llu cells: a sum of row or column indices could pass 2^64",
                          (unsigned long long)rows, (unsigned long long)cols)
                   : fail(GS_ERR_UNSUPPORTED, "a grid of %llu x %llu cells: a sum of row or column indices could pass 2^64",
                          (unsigned long long)rows, (unsigned long long)cols);
}

// Labels are u32 cell indices: every slab of this process (gs_fields_components asks every rank's), every member.
int32_t check_slab_labels(const gs_ctx *ctx, const gs_field *f)
{
    for (size_t i = 0; i < ctx->slabs.size(); ++i)
        if ((uint64_t)f->s[i].rows * f->cols >= ((uint64_t)1 << 32))
            return fail(GS_ERR_UNSUPPORTED, "slab %zu holds %llu x %llu cells: labels are 32-bit, fewer than 2^32 cells per slab", i,
                        (unsigned long long)f->s[i].rows, (unsigned long long)f->cols);
    return GS_OK;
}

int32_t check_member_labels(uint64_t cells)
{
    if (cells >= ((uint64_t)1 << 32))
        return fail(GS_ERR_UNSUPPORTED, "a member holds %llu cells: labels are 32-bit, fewer than 2^32 cells", (unsigned long long)cells);
    return GS_OK;
}

// Batches of whole members in one block of label memory: as many of `count` as fit the budget, at least one.
uint64_t member_batch(uint64_t cells, uint64_t count)
{
    const uint64_t batch = (uint64_t)GS_COMPONENTS_BATCH_BYTES / 8 / cells;
    return batch < 1 ? 1 : (batch > count ? count : batch);
}

int32_t refuse_world(const gs_ctx *ctx, const char *what = "component lists")
{
    if (ctx->world > 1)
        return fail(GS_ERR_UNSUPPORTED, "%s in a multi-process context (%d processes): the ranks' record lists are "
                                        "not exchanged", what, ctx->world);
    return GS_OK;
}

// Record memory of one call, freed when the call returns, however it returns.
struct RecordMemory {
    struct Block {
        int device;
        void *p;
    };
    std::vector<Block> blocks;
    ~RecordMemory() { release(); }
    void release()
    {
        for (const Block &b : blocks)
            if (b.p && hipSetDevice(b.device) == hipSuccess) (void)hipFree(b.p);
        blocks.clear();
    }
    int32_t add_bytes(int device, uint64_t bytes, const char *what, void **out)
    {
        GS_HIP(hipSetDevice(device));
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, (size_t)bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(GS_ERR_NOMEM, "%s memory of %llu bytes: %s", what, (unsigned long long)bytes, hipGetErrorString(e));
        }
        blocks.push_back(Block{device, p});
        *out = p;
        return GS_OK;
    }
    int32_t add(int device, uint64_t records, GsComponentRecord **out)
    {
        return add_bytes(device, records * sizeof(GsComponentRecord), "record", reinterpret_cast<void **>(out));
    }
    int32_t add(int device, uint64_t pieces, GsMatchOverlap **out) // (a match's overlaps: one per piece)
    {
        return add_bytes(device, pieces * sizeof(GsMatchOverlap), "overlap", reinterpret_cast<void **>(out));
    }
};

// A slab's (or batch's) scratch buffer as a list's work memory: the number of records, the counts of `entries` entries, then
// room for the record indices of two rows of `cols` cells.
size_t list_work_bytes(uint64_t entries, size_t cols) { return (4 + (size_t)gs_list_groups(entries) + 2 * cols) * sizeof(uint32_t); }
GsListWork list_work(void *scratch, uint32_t *marks)
{
    uint32_t *w = static_cast<uint32_t *>(scratch);
    return GsListWork{marks, w + 4, w};
}
uint32_t *list_seams(void *scratch, uint64_t entries) { return static_cast<uint32_t *>(scratch) + 4 + gs_list_groups(entries); }

// ---- component matches -------------------------------------------------------------------------------------------------
static_assert(sizeof(gs_component_overlap) == 16 && sizeof(GsMatchOverlap) == 16 && offsetof(gs_component_overlap, after) == 4 &&
                  offsetof(GsMatchOverlap, after) == 4 && offsetof(gs_component_overlap, cells) == 8 &&
                  offsetof(GsMatchOverlap, cells) == 8,
              "gs_component_overlap layout");

// A match's work memory in a slab's (or batch's) scratch buffer: three lists' work memories one after the other -- before,
// after, the pieces.
size_t match_work_bytes(uint64_t entries, size_t cols) { return 3 * list_work_bytes(entries, cols); }
void *match_work(void *scratch, uint64_t entries, size_t cols, int k)
{
    return static_cast<unsigned char *>(scratch) + (size_t)k * list_work_bytes(entries, cols);
}

// ---- listings: records behind a labelling ------------------------------------------------------------------------------
// The listing of ONE labelling of a field over this process's slab chain: `labels` holds the labelling, a block per slab, and
// slot k of every slab's scratch buffer is its work memory (match_work; a lone list has slot 0).  Three steps, which the
// caller's two sync_compute keep apart; the launch that labels slab i is the caller's, in front of count(i), and so is the
// device that is current.  In a chain a component that touches a slab's first or last row is listed whatever its size:
// min_size comes after the merge.
struct ChainListing {
    gs_ctx *ctx;
    const gs_field *f;
    const LabelMemory &labels;
    int k;
    uint64_t min_size;
    std::vector<uint32_t> selected;                     // per slab: the records it lists
    std::vector<std::vector<gs_component_record>> part; // per slab: its records
    std::vector<std::vector<uint32_t>> seam;            // per slab of a chain: the record indices of its first and its last row

    ChainListing(gs_ctx *c, const gs_field *field, const LabelMemory &l, int slot, uint64_t least)
        : ctx(c), f(field), labels(l), k(slot), min_size(least), selected(c->slabs.size(), 0u), part(c->slabs.size()), seam(c->slabs.size()) {}
    bool chain() const { return ctx->slabs.size() > 1; }
    uint64_t cells(size_t i) const { return (uint64_t)f->s[i].rows * f->cols; }
    void *work(size_t i) const { return match_work(ctx->slabs[i].scratch, cells(i), (size_t)f->cols, k); }

    // Slab i, not empty: the count, and selected[i] on its way back.
    int32_t count(size_t i)
    {
        const LabelMemory::Block &lb = labels.blocks[i];
        const GsListWork w = list_work(work(i), lb.marks);
        GS_HIP(gs_launch_list_count(lb.parent, lb.size, 1, (int64_t)f->s[i].rows, (int32_t)f->cols, min_size, w, ctx->slabs[i].compute));
        GS_HIP(hipMemcpyAsync(&selected[i], w.selected, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->slabs[i].compute));
        return GS_OK;
    }

    // Slab i, not empty, after the sync_compute that brought selected[i]: exactly that many records in `memory`, filled, and
    // on their way back with, in a chain, the two seam rows.
    int32_t fill(size_t i, RecordMemory &memory)
    {
        const size_t cols = (size_t)f->cols;
        if (chain()) seam[i].assign(2 * cols, kCompUnset);
        if (selected[i] == 0) return GS_OK; // (no set cell in its first or last row either)
        SlabRt &sl = ctx->slabs[i];
        const LabelMemory::Block &lb = labels.blocks[i];
        GsComponentRecord *records = nullptr;
        GS_TRY(memory.add(sl.device, selected[i], &records));
        part[i].resize(selected[i]);
        uint32_t *seams = chain() ? list_seams(work(i), cells(i)) : nullptr;
        GS_HIP(gs_launch_list_fill(lb.parent, lb.size, 1, (int64_t)f->s[i].rows, (int32_t)cols, min_size, list_work(work(i), lb.marks),
                                   records, seams, sl.compute));
        GS_HIP(hipMemcpyAsync(part[i].data(), records, part[i].size() * sizeof(gs_component_record), hipMemcpyDeviceToHost, sl.compute));
        if (chain()) GS_HIP(hipMemcpyAsync(seam[i].data(), seams, 2 * cols * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.compute));
        return GS_OK;
    }

    // After the second sync_compute: rows global, and the slabs' records as the one plane of `list` -- a chain's joined across
    // the seams, `where` then saying what became of every slab's record (merge_component_lists).
    void finish(int32_t connectivity, gs_component_list *list, std::vector<uint32_t> *where = nullptr)
    {
        const size_t nslab = part.size(), cols = (size_t)f->cols;
        for (size_t i = 0; i < nslab; ++i) records_to_global_rows(part[i].data(), part[i].size(), f->s[i].g_row0);
        if (!chain()) {
            list->records.swap(part[0]);
        } else {
            std::vector<const gs_component_record *> recs;
            std::vector<size_t> counts;
            std::vector<ListSeamRows> rows;
            for (size_t i = 0; i < nslab; ++i) {
                if (f->s[i].rows == 0) continue;
                recs.push_back(part[i].data());
                counts.push_back(part[i].size());
                rows.push_back(ListSeamRows{seam[i].data(), seam[i].data() + cols});
            }
            list->records = merge_component_lists(recs.data(), counts.data(), rows.data(), recs.size(), cols, connectivity, min_size, where);
        }
        list->offsets[1] = list->records.size();
    }
};

// The listing of ONE labelling of a batch of an ensemble's members on slab 0, the current device: `lb` holds the labelling of
// up to `batch` members stacked one after the other, and slot k of slab 0's scratch buffer is its work memory.  The launch
// that labels the batch's nb members is the caller's, in front of count(nb), and so is the synchronisation behind it.
struct BatchListing {
    gs_ctx *ctx;
    const gs_ensemble *e;
    const LabelMemory::Block &lb;
    GsListWork work;
    uint64_t min_size;
    uint32_t selected = 0;                 // the records the batch lists
    std::vector<gs_component_record> host; // the batch's records
    std::vector<uint64_t> before;          // the batch's records in the planes before plane p (batch_records_to_planes)

    BatchListing(gs_ctx *c, const gs_ensemble *ens, const LabelMemory::Block &block, uint64_t batch, int k, uint64_t least)
        : ctx(c), e(ens), lb(block), work(list_work(match_work(c->slabs[0].scratch, batch * ens->rows * ens->cols, 0, k), nullptr)),
          min_size(least) {}

    // The count, and `selected` on its way back.
    int32_t count(uint64_t nb)
    {
        hipStream_t s = ctx->slabs[0].compute;
        GS_HIP(gs_launch_list_count(lb.parent, lb.size, (int64_t)nb, (int64_t)e->rows, (int32_t)e->cols, min_size, work, s));
        GS_HIP(hipMemcpyAsync(&selected, work.selected, sizeof selected, hipMemcpyDeviceToHost, s));
        return GS_OK;
    }

    // After the synchronisation that brought `selected`: exactly that many records in `memory` -- nothing for none --, filled
    // and fetched; then the records to planes b0 .. b0 + nb of `list`, whose offsets hold counts until the caller sums them.
    int32_t fill(uint64_t b0, uint64_t nb, RecordMemory &memory, gs_component_list *list)
    {
        host.resize(selected);
        if (selected != 0) {
            SlabRt &sl = ctx->slabs[0];
            GsComponentRecord *records = nullptr;
            GS_TRY(memory.add(sl.device, selected, &records));
            GS_HIP(gs_launch_list_fill(lb.parent, lb.size, (int64_t)nb, (int64_t)e->rows, (int32_t)e->cols, min_size, work, records,
                                       nullptr, sl.compute));
            GS_HIP(hipMemcpyAsync(host.data(), records, host.size() * sizeof(gs_component_record), hipMemcpyDeviceToHost, sl.compute));
            GS_HIP(hipStreamSynchronize(sl.compute));
        }
        batch_records_to_planes(host.data(), host.size(), e->rows, (size_t)nb, before);
        for (size_t p = 0; p < (size_t)nb; ++p) list->offsets[(size_t)b0 + p + 1] += before[p + 1] - before[p];
        list->records.insert(list->records.end(), host.begin(), host.end());
        return GS_OK;
    }
};

// ---- regional observables ------------------------------------------------------------------------------------------------
// The region grid of gs_hip.h for a grid of rows x cols cells, or its refusal.  No handle is looked at.
int32_t region_grid(uint64_t rows, uint64_t cols, int32_t rh, int32_t rw, uint64_t *rr, uint64_t *rc)
{
    if (rh < 1) return fail(GS_ERR_INVALID, "a region height of %d (at least 1)", rh);
    if (rw < 16 || rw % 4 != 0) return fail(GS_ERR_INVALID, "a region width of %d (a multiple of 4, at least 16)", rw);
    const uint64_t RR = rows / (uint64_t)rh + (rows % (uint64_t)rh ? 1 : 0), RC = cols / (uint64_t)rw + (cols % (uint64_t)rw ? 1 : 0);
    if (RR != 0 && RC > (uint64_t)GS_REGIONS_MAX / RR)
        return fail(GS_ERR_INVALID, "%llu x %llu regions (at most %u)", (unsigned long long)RR, (unsigned long long)RC,
                    (unsigned)GS_REGIONS_MAX);
    *rr = RR;
    *rc = RC;
    return GS_OK;
}

// What a regional call checks before any device work, in gs_hip.h's order: the region shape alone, then -- where the first
// field can be read -- the region count of its grid; the handles themselves are check_planes'.
int32_t check_regions(const gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw)
{
    uint64_t rr, rc;
    GS_TRY(region_grid(0, 0, rh, rw, &rr, &rc));
    if (n >= 1 && n <= 4 && fields[0] && fields[0]->ctx == ctx) GS_TRY(region_grid(fields[0]->rows, fields[0]->cols, rh, rw, &rr, &rc));
    return GS_OK;
}

// ---- power spectra ---------------------------------------------------------------------------------------------------------
// The tile size and the window of a spectrum, or the refusal of gs_hip.h.  No handle is looked at.
int32_t check_spectrum(int32_t tile, int32_t window)
{
    if (tile != 16 && tile != 32 && tile != 64 && tile != 128) return fail(GS_ERR_INVALID, "a tile of %d cells (16, 32, 64 or 128)", tile);
    if (window != 0 && window != 1) return fail(GS_ERR_INVALID, "window %d (0: none, 1: periodic Hann)", window);
    return GS_OK;
}

// The tables of gs_hip.h: formed in f64, rounded to f32.
void spectrum_tables(int32_t tile, float *window, float *twiddle)
{
    const double step = 2.0 * 3.14159265358979323846 / (double)tile;
    for (int32_t j = 0; window && j < tile; ++j) window[j] = (float)(0.5 - 0.5 * std::cos(step * (double)j));
    for (int32_t k = 0; twiddle && k < tile / 2; ++k) {
        twiddle[2 * k] = (float)std::cos(step * (double)k);
        twiddle[2 * k + 1] = (float)-std::sin(step * (double)k);
    }
}

// Band results (gs_spectrum_result_bytes each: the sums, then {used, skipped}) of `planes` planes, [plane][bands], into
// power[plane][bins] and tiles[plane][2]: the first `whole` bands of a plane added in ascending order from +0.0.
void fold_bands(const unsigned char *results, size_t planes, size_t bands, size_t whole, int32_t tile, double *power, uint64_t *tiles)
{
    const size_t bins = (size_t)tile * (size_t)(tile / 2 + 1), words = bins + 2;
    for (size_t p = 0; p < planes; ++p) {
        double *sum = power + p * bins;
        std::fill(sum, sum + bins, 0.0);
        tiles[2 * p] = tiles[2 * p + 1] = 0;
        for (size_t b = 0; b < whole; ++b) {
            const unsigned char *band = results + (p * bands + b) * words * 8;
            const double *x = reinterpret_cast<const double *>(band);
            const uint64_t *c = reinterpret_cast<const uint64_t *>(band) + bins;
            for (size_t e = 0; e < bins; ++e) sum[e] = sum[e] + x[e];
            tiles[2 * p] += c[0];
            tiles[2 * p + 1] += c[1];
        }
    }
}

} // namespace

extern "C" {

int32_t gs_spectrum_tables(int32_t tile, float *window, float *twiddle)
{
    GS_TRY(check_spectrum(tile, 0));
    spectrum_tables(tile, window, twiddle);
    return GS_OK;
}

int32_t gs_fields_spectrum(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t tile, int32_t window, double *power,
                           uint64_t *tiles)
{
    GS_TRY(check_spectrum(tile, window));
    if (!power || !tiles) return fail(GS_ERR_INVALID, "null output");
    if (!ctx || !fields) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    const size_t bins = (size_t)tile * (size_t)(tile / 2 + 1), elem = gs_spectrum_result_bytes(tile);
    const uint64_t T = (uint64_t)tile, whole = f0->rows / T, RR = (f0->rows + T - 1) / T;
    if (whole == 0 || f0->cols < T) { // no tile; the same shape on every rank: nobody exchanges anything
        std::fill(power, power + (size_t)n * bins, 0.0);
        std::fill(tiles, tiles + 2 * (size_t)n, (uint64_t)0);
        return GS_OK;
    }
    GS_TRY(check_band_seams(ctx, f0, tile)); // every rank reaches the same verdict before anybody allocates
    // a slab's segment records lie behind its band results in its scratch buffer, which is made large enough here:
    // band_results then finds it so and keeps it (the regional comparison's precedent)
    const size_t nslab = ctx->slabs.size();
    std::vector<size_t> records_at(nslab, (size_t)0);
    for (size_t i = 0; i < nslab; ++i) {
        const uint64_t rows = (uint64_t)f0->s[i].rows;
        if (rows == 0) continue;
        const size_t results = (size_t)n * (size_t)((rows + T - 1) / T) * elem;
        records_at[i] = (results + 255) / 256 * 256;
        GS_TRY(ensure_scratch(ctx, (int)i, records_at[i] + gs_spectrum_record_bytes(n, (int64_t)rows, (int32_t)f0->cols, tile),
                              "spectrum"));
    }
    float h[128], w[128];
    spectrum_tables(tile, h, w);
    std::vector<unsigned char> bands((size_t)n * (size_t)RR * elem);
    GS_TRY(band_results(ctx, f0, n, tile, RR, 1, elem, false, "spectrum", bands.data(),
                        [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *planes[4];
        slab_planes(fields, n, i, planes);
        return gs_launch_spectrum(planes, n, 1, 0, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, tile, window, h, w,
                                  dev + records_at[i], dev, s);
    }));
    fold_bands(bands.data(), (size_t)n, (size_t)RR, (size_t)whole, tile, power, tiles);
    return GS_OK;
}

int32_t gs_members_spectrum(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, int32_t tile, int32_t window,
                            double *power, uint64_t *tiles)
{
    GS_TRY(check_spectrum(tile, window));
    if (!power || !tiles) return fail(GS_ERR_INVALID, "null output");
    if (!ctx) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_members(ctx, e, first, count));
    const size_t bins = (size_t)tile * (size_t)(tile / 2 + 1), elem = gs_spectrum_result_bytes(tile), planes_n = (size_t)(2 * count);
    const uint64_t T = (uint64_t)tile, whole = e->rows / T, RR = (e->rows + T - 1) / T;
    if (whole == 0 || e->cols < T) {
        std::fill(power, power + planes_n * bins, 0.0);
        std::fill(tiles, tiles + 2 * planes_n, (uint64_t)0);
        return GS_OK;
    }
    const size_t out_bytes = planes_n * (size_t)RR * elem, records_at = (out_bytes + 255) / 256 * 256;
    GS_TRY(ensure_scratch(ctx, 0, records_at + gs_spectrum_record_bytes((int64_t)planes_n, (int64_t)e->rows, (int32_t)e->cols, tile),
                          "spectrum"));
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    unsigned char *dev = static_cast<unsigned char *>(sl.scratch);
    float h[128], w[128];
    spectrum_tables(tile, h, w);
    // U and V of a member are two planes of the set, the next member's `cells` floats further on: plane 2 m + s
    const float *planes[2];
    member_planes(e, first, planes);
    GS_HIP(gs_launch_spectrum(planes, 2, (int64_t)count, (int64_t)(e->rows * e->cols), (int64_t)e->cols, (int64_t)e->rows,
                              (int32_t)e->cols, tile, window, h, w, dev + records_at, dev, sl.compute));
    std::vector<unsigned char> bands(out_bytes);
    GS_HIP(hipMemcpyAsync(bands.data(), dev, out_bytes, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    fold_bands(bands.data(), planes_n, (size_t)RR, (size_t)whole, tile, power, tiles);
    return GS_OK;
}

int32_t gs_fields_summarize(gs_ctx *ctx, gs_field *const *fields, int32_t n, gs_summary *out)
{
    if (!ctx || !fields || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    if (f0->rows == 0 || f0->cols == 0) { // the same shape on every rank: nobody exchanges anything
        for (int32_t p = 0; p < n; ++p) out[p] = empty_summary();
        return GS_OK;
    }
    std::vector<GsRowSummary> rec((size_t)n * (size_t)f0->rows); // a row's record: a band of one row with one result
    GS_TRY(band_results(ctx, f0, n, 1, f0->rows, 1, sizeof(GsRowSummary), false, "summary", reinterpret_cast<unsigned char *>(rec.data()),
                        [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *planes[4];
        slab_planes(fields, n, i, planes);
        return gs_launch_row_summary(planes, n, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols,
                                     reinterpret_cast<GsRowSummary *>(dev), s);
    }));
    for (int32_t p = 0; p < n; ++p) out[p] = fold_rows(rec.data() + (size_t)p * (size_t)f0->rows, (size_t)f0->rows);
    return GS_OK;
}

int32_t gs_members_summarize(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, gs_summary *out)
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_members(ctx, e, first, count));
    const uint64_t rows = count * e->rows;
    const size_t rec_bytes = (size_t)(2 * rows) * sizeof(GsRowSummary), out_bytes = (size_t)(2 * count) * sizeof(GsRowSummary);
    GS_TRY(ensure_scratch(ctx, 0, rec_bytes + out_bytes, "summary"));
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GsRowSummary *rec = static_cast<GsRowSummary *>(sl.scratch), *folded = rec + 2 * rows;
    // the members' rows one after the other: one plane of count x rows rows, pitch cols
    const float *planes[2];
    member_planes(e, first, planes);
    GS_HIP(gs_launch_row_summary(planes, 2, (int64_t)e->cols, (int64_t)rows, (int32_t)e->cols, rec, sl.compute));
    GS_HIP(gs_launch_summary_fold(rec, (int64_t)count, (int64_t)e->rows, folded, sl.compute));
    std::vector<GsRowSummary> host((size_t)(2 * count));
    GS_HIP(hipMemcpyAsync(host.data(), folded, out_bytes, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    for (size_t i = 0; i < host.size(); ++i) out[i] = from_record(host[i]);
    return GS_OK;
}

int32_t gs_fields_compare(gs_ctx *ctx, gs_field *const *a, gs_field *const *b, int32_t n, gs_change *out)
{
    if (!ctx || !a || !b || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_planes(ctx, a, n, b));
    const gs_field *f0 = a[0];
    for (int32_t p = 0; p < n; ++p) out[p] = no_change();
    if (f0->rows == 0 || f0->cols == 0) return GS_OK; // the same shape on every rank: nobody exchanges anything
    std::vector<GsRowChange> rec((size_t)n * (size_t)f0->rows); // as the summaries' rows
    GS_TRY(band_results(ctx, f0, n, 1, f0->rows, 1, sizeof(GsRowChange), false, "comparison", reinterpret_cast<unsigned char *>(rec.data()),
                        [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *pa[4], *pb[4];
        slab_planes(a, n, i, pa);
        slab_planes(b, n, i, pb);
        return gs_launch_row_change(pa, pb, n, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols,
                                    reinterpret_cast<GsRowChange *>(dev), s);
    }));
    for (int32_t p = 0; p < n; ++p) out[p] = fold_rows(rec.data() + (size_t)p * (size_t)f0->rows, (size_t)f0->rows);
    return GS_OK;
}

int32_t gs_members_compare(gs_ctx *ctx, gs_ensemble *e, gs_ensemble *ref, uint64_t first, uint64_t count, gs_change *out)
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_members(ctx, e, first, count, ref, true));
    const uint64_t cells = e->rows * e->cols, rows = count * e->rows;
    if (cells == 0) {
        for (uint64_t i = 0; i < 2 * count; ++i) out[i] = no_change();
        return GS_OK;
    }
    const size_t rec_bytes = (size_t)(2 * rows) * sizeof(GsRowChange), out_bytes = (size_t)(2 * count) * sizeof(GsChangeTotal);
    GS_TRY(ensure_scratch(ctx, 0, rec_bytes + out_bytes, "comparison"));
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GsRowChange *rec = static_cast<GsRowChange *>(sl.scratch);
    GsChangeTotal *folded = reinterpret_cast<GsChangeTotal *>(rec + 2 * rows);
    // the members' rows one after the other: one plane of count x rows rows, pitch cols
    const float *pa[2], *pb[2];
    member_planes(e, first, pa);
    member_planes(ref, first, pb);
    GS_HIP(gs_launch_row_change(pa, pb, 2, (int64_t)e->cols, (int64_t)rows, (int32_t)e->cols, rec, sl.compute));
    GS_HIP(gs_launch_change_fold(rec, (int64_t)count, (int64_t)e->rows, folded, sl.compute));
    // (GsChangeTotal is gs_change's layout)
    GS_HIP(hipMemcpyAsync(out, folded, out_bytes, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    return GS_OK;
}

int32_t gs_fields_copy(gs_ctx *ctx, gs_field *const *dst, gs_field *const *src, int32_t n)
{
    if (!ctx || !dst || !src) return fail(GS_ERR_INVALID, "null argument");
    if (n >= 1 && n <= 4) // (a count that is no 1..4 is check_planes' first refusal)
        for (int32_t p = 0; p < n; ++p) {
            if (dst[p] && dst[p] == src[p]) return fail(GS_ERR_INVALID, "field %d would be copied onto itself", p);
            for (int32_t q = 0; q < p; ++q)
                if (dst[p] && dst[p] == dst[q]) return fail(GS_ERR_INVALID, "fields %d and %d: one target named twice", q, p);
        }
    GS_TRY(check_planes(ctx, dst, n, src));
    const gs_field *f0 = dst[0];
    if (f0->rows == 0 || f0->cols == 0) return GS_OK;
    const size_t pitch_bytes = (size_t)f0->pitch * sizeof(float), row_bytes = (size_t)f0->cols * sizeof(float);
    for (size_t i = 0; i < ctx->slabs.size(); ++i) {
        SlabRt &sl = ctx->slabs[i];
        GS_HIP(hipSetDevice(sl.device));
        for (int32_t p = 0; p < n; ++p)
            GS_HIP(hipMemcpy2DAsync(dst[p]->s[i].row0, pitch_bytes, src[p]->s[i].row0, pitch_bytes, row_bytes,
                                    (size_t)f0->s[i].rows, hipMemcpyDeviceToDevice, sl.compute));
    }
    GS_TRY(sync_compute(ctx));
    for (int32_t p = 0; p < n; ++p) dst[p]->ghost_depth = 0; // as after gs_field_upload: the next step refreshes the ghost rows
    return GS_OK;
}

int32_t gs_members_copy(gs_ctx *ctx, gs_ensemble *dst, gs_ensemble *src, uint64_t first, uint64_t count)
{
    if (!ctx) return fail(GS_ERR_INVALID, "null argument");
    if (dst && dst == src) return fail(GS_ERR_INVALID, "an ensemble would be copied onto itself");
    GS_TRY(check_members(ctx, dst, first, count, src, true));
    const size_t cells = (size_t)(dst->rows * dst->cols), off = (size_t)first * cells, bytes = (size_t)count * cells * sizeof(float);
    if (bytes == 0) return GS_OK;
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GS_HIP(hipMemcpyAsync(dst->u[dst->cur] + off, src->u[src->cur] + off, bytes, hipMemcpyDeviceToDevice, sl.compute));
    GS_HIP(hipMemcpyAsync(dst->v[dst->cur] + off, src->v[src->cur] + off, bytes, hipMemcpyDeviceToDevice, sl.compute));
    mark_members_written(dst, first, count);
    GS_HIP(hipStreamSynchronize(sl.compute));
    return GS_OK;
}

int32_t gs_fields_histogram(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *lo, const float *hi, int32_t bins,
                            uint64_t *out)
{
    if (!ctx || !fields || !lo || !hi || !out) return fail(GS_ERR_INVALID, "null argument");
    // the ranges before any handle is looked at; a count that is no 1..4 is check_planes' first refusal
    float scale[4];
    if (n >= 1 && n <= 4) GS_TRY(check_ranges(lo, hi, n, bins, scale));
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    const size_t words = (size_t)n * (size_t)(bins + 3);
    std::fill(out, out + words, (uint64_t)0);
    if (f0->rows == 0 || f0->cols == 0) return GS_OK; // the same shape on every rank: nobody exchanges anything
    return slab_counters(ctx, fields, n, words, 0, "histogram", out,
                         [&](size_t i, unsigned long long *dev, const float *, hipStream_t s) {
        const float *planes[4];
        slab_planes(fields, n, i, planes);
        return gs_launch_histogram(planes, n, 1, 0, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, lo, hi, scale, bins,
                                   max_groups(ctx), dev, s);
    });
}

int32_t gs_members_histogram(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float lo[2], const float hi[2],
                             int32_t bins, uint64_t *out)
{
    if (!ctx || !lo || !hi || !out) return fail(GS_ERR_INVALID, "null argument");
    float scale[2];
    GS_TRY(check_ranges(lo, hi, 2, bins, scale)); // before the ensemble is looked at
    GS_TRY(check_members(ctx, e, first, count));
    const uint64_t cells = e->rows * e->cols;
    const size_t words = (size_t)(2 * count) * (size_t)(bins + 3);
    // member first + i's U and V are planes 2 i and 2 i + 1 of the launch: `cells` floats from one member to the next
    return member_counters(ctx, e, first, words, "histogram", out,
                           [&](const float *const *planes, unsigned long long *dev, hipStream_t s) {
        return gs_launch_histogram(planes, 2, (int64_t)count, (int64_t)cells, (int64_t)e->cols, (int64_t)e->rows,
                                   (int32_t)e->cols, lo, hi, scale, bins, max_groups(ctx), dev, s);
    });
}

int32_t gs_fields_morphology(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *thresholds, const int32_t *above,
                             int32_t nt, gs_morphology *out)
{
    if (!ctx || !fields || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_thresholds(thresholds, n, nt));
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    const size_t results = (size_t)n * (size_t)nt;
    if (f0->rows == 0 || f0->cols == 0) { // the same shape on every rank: nobody exchanges anything
        std::memset(out, 0, results * sizeof(gs_morphology));
        return GS_OK;
    }
    // The quad rows are split into consecutive runs, one per slab: the slab of global rows [r0, r1) counts those whose lower
    // row is r0 .. r1 - 1, the last slab also the one below row R - 1.  A slab with r0 > 0 needs row r0 - 1, which is staged.
    std::vector<uint64_t> sum(results * kQuadCounted);
    GS_TRY(slab_counters(ctx, fields, n, sum.size(), 1, "morphology", sum.data(),
                         [&](size_t i, unsigned long long *dev, const float *staged, hipStream_t s) {
        const bool last = f0->s[i].g_row0 + (uint64_t)f0->s[i].rows == f0->rows;
        const float *planes[4], *row_above[4];
        slab_planes(fields, n, i, planes);
        for (int32_t p = 0; p < 4; ++p) row_above[p] = staged && p < n ? staged + (size_t)p * (size_t)f0->pitch : nullptr;
        return gs_launch_quads(planes, row_above, n, 1, 0, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, last ? 1 : 0,
                               thresholds, above, nt, max_groups(ctx), dev, s);
    }));
    for (size_t j = 0; j < results; ++j) out[j] = from_counted(sum.data() + j * kQuadCounted, f0->rows, f0->cols);
    return GS_OK;
}

int32_t gs_members_morphology(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float *thresholds,
                              const int32_t above[2], int32_t nt, gs_morphology *out)
{
    if (!ctx || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_thresholds(thresholds, 2, nt)); // before the ensemble is looked at
    GS_TRY(check_members(ctx, e, first, count));
    const uint64_t cells = e->rows * e->cols;
    const size_t results = (size_t)(2 * count) * (size_t)nt;
    if (cells == 0) {
        std::memset(out, 0, results * sizeof(gs_morphology));
        return GS_OK;
    }
    // member first + i's U and V are planes 2 i and 2 i + 1 of the launch, `cells` floats from one member to the next; each
    // is a plane of its own: nothing above its first row, padding below its last -- it never sees its neighbours' rows
    std::vector<uint64_t> host(results * kQuadCounted);
    GS_TRY(member_counters(ctx, e, first, host.size(), "morphology", host.data(),
                           [&](const float *const *planes, unsigned long long *dev, hipStream_t s) {
        return gs_launch_quads(planes, nullptr, 2, (int64_t)count, (int64_t)cells, (int64_t)e->cols, (int64_t)e->rows,
                               (int32_t)e->cols, 1, thresholds, above, nt, max_groups(ctx), dev, s);
    }));
    for (size_t j = 0; j < results; ++j) out[j] = from_counted(host.data() + j * kQuadCounted, e->rows, e->cols);
    return GS_OK;
}

int32_t gs_fields_correlation(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *thresholds, const int32_t *above,
                              int32_t nt, int32_t max_lag, uint64_t *out)
{
    if (!ctx || !fields || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_thresholds(thresholds, n, nt));
    GS_TRY(check_max_lag(max_lag)); // before any handle is looked at, too
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    const size_t depth = (size_t)max_lag;
    const size_t words = (size_t)n * (size_t)nt * 4 * (depth + 1);
    std::fill(out, out + words, (uint64_t)0);
    if (f0->rows == 0 || f0->cols == 0) return GS_OK; // the same shape on every rank: nobody exchanges anything
    // A pair belongs to its LOWER row: the slab of global rows [r0, r1) counts the pairs whose lower cell lies in it and needs
    // the min(L, r0) rows above r0.  With several slabs these are the L last rows of the slab above, so every slab -- other
    // processes' too: every rank reaches the same verdict -- must hold L rows.
    const uint64_t S = (uint64_t)ctx->total_slabs();
    for (uint64_t k = 0; S > 1 && k < S; ++k)
        if (global_slab_rows(ctx, f0->rows, k) < (uint64_t)max_lag)
            return fail(GS_ERR_UNSUPPORTED, "slab %llu holds %llu rows, fewer than the largest lag %d (the rows above a slab "
                                            "come from the one slab above it)",
                        (unsigned long long)k, (unsigned long long)global_slab_rows(ctx, f0->rows, k), max_lag);
    return slab_counters(ctx, fields, n, words, depth, "correlation", out,
                         [&](size_t i, unsigned long long *dev, const float *staged, hipStream_t s) {
        const float *planes[4], *rows_above[4];
        slab_planes(fields, n, i, planes);
        for (int32_t p = 0; p < 4; ++p) rows_above[p] = staged && p < n ? staged + (size_t)p * depth * (size_t)f0->pitch : nullptr;
        return gs_launch_pairs(planes, rows_above, staged ? max_lag : 0, n, 1, 0, f0->pitch, (int64_t)f0->s[i].rows,
                               (int32_t)f0->cols, thresholds, above, nt, max_lag, max_groups(ctx), dev, s);
    });
}

int32_t gs_members_correlation(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float *thresholds,
                               const int32_t above[2], int32_t nt, int32_t max_lag, uint64_t *out)
{
    if (!ctx || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_thresholds(thresholds, 2, nt)); // before the ensemble is looked at
    GS_TRY(check_max_lag(max_lag));
    GS_TRY(check_members(ctx, e, first, count));
    const uint64_t cells = e->rows * e->cols;
    const size_t words = (size_t)(2 * count) * (size_t)nt * 4 * (size_t)(max_lag + 1);
    // member first + i's U and V are planes 2 i and 2 i + 1 of the launch, `cells` floats from one member to the next; each
    // is a plane of its own: nothing above its first row -- it never sees its neighbours' rows
    return member_counters(ctx, e, first, words, "correlation", out,
                           [&](const float *const *planes, unsigned long long *dev, hipStream_t s) {
        return gs_launch_pairs(planes, nullptr, 0, 2, (int64_t)count, (int64_t)cells, (int64_t)e->cols, (int64_t)e->rows,
                               (int32_t)e->cols, thresholds, above, nt, max_lag, max_groups(ctx), dev, s);
    });
}

int32_t gs_fields_components(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *thresholds, const int32_t *above,
                             int32_t nt, int32_t connectivity, gs_components *out)
{
    if (!ctx || !fields || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_thresholds(thresholds, n, nt));
    GS_TRY(check_connectivity(connectivity)); // before any handle is looked at, too
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    const size_t results = (size_t)n * (size_t)nt;
    if (f0->rows == 0 || f0->cols == 0) { // the same shape on every rank: nobody exchanges anything
        std::memset(out, 0, results * sizeof(gs_components));
        return GS_OK;
    }
    // every slab of the global grid: every rank reaches the same verdict
    const uint64_t S = (uint64_t)ctx->total_slabs();
    auto slab_rows = [&](uint64_t k) { return global_slab_rows(ctx, f0->rows, k); };
    for (uint64_t k = 0; k < S; ++k)
        if (slab_rows(k) > 0 && slab_rows(k) >= ((uint64_t)1 << 32) / f0->cols + ((((uint64_t)1 << 32) % f0->cols) ? 1 : 0))
            return fail(GS_ERR_UNSUPPORTED, "slab %llu holds %llu x %llu cells: labels are 32-bit, fewer than 2^32 cells per slab",
                        (unsigned long long)k, (unsigned long long)slab_rows(k), (unsigned long long)f0->cols);
    const size_t nslab = ctx->slabs.size(), cols = (size_t)f0->cols;
    for (size_t i = 0; i < nslab; ++i)
        if ((uint64_t)f0->s[i].rows != slab_rows((uint64_t)ctx->global_index((int)i)))
            return fail(GS_ERR_INVALID, "row partition disagrees with this process's slabs");
    // per slab and (field, threshold): the counters, then the first row's roots and sizes and the last row's (u32 each)
    const size_t rec_words = kCompWords + 2 * cols, slab_words = results * rec_words;
    LabelMemory labels;
    int32_t had = GS_OK;
    for (size_t i = 0; i < nslab && had == GS_OK; ++i) had = labels.add(ctx->slabs[i].device, (uint64_t)f0->s[i].rows * (uint64_t)cols);
    if (ctx->world > 1) { // the ranks agree on the verdict before anything else is exchanged: nobody waits for a rank that left
        const uint64_t mine = had == GS_OK ? 0 : 1;
        std::vector<uint64_t> verdicts((size_t)ctx->world);
        GS_TRY(exchange(ctx, &mine, std::vector<size_t>((size_t)ctx->world, sizeof mine), "components", verdicts.data()));
        for (int q = 0; q < ctx->world && had == GS_OK; ++q)
            if (verdicts[(size_t)q]) had = fail(GS_ERR_NOMEM, "rank %d could not have its label memory", q);
    }
    if (had != GS_OK) return had;
    for (size_t i = 0; i < nslab; ++i) GS_TRY(ensure_scratch(ctx, (int)i, slab_words * sizeof(uint64_t), "components"));
    std::vector<uint64_t> local(nslab * slab_words, (uint64_t)0);
    for (size_t i = 0; i < nslab; ++i) {
        if (f0->s[i].rows == 0) continue;
        SlabRt &sl = ctx->slabs[i];
        GS_HIP(hipSetDevice(sl.device));
        unsigned long long *dev = static_cast<unsigned long long *>(sl.scratch);
        GS_HIP(hipMemsetAsync(dev, 0, slab_words * sizeof(uint64_t), sl.compute));
        for (size_t j = 0; j < results; ++j) {
            unsigned long long *rec = dev + j * rec_words;
            GS_HIP(gs_launch_components(fields[j / (size_t)nt]->s[i].row0, 1, 0, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols,
                                        thresholds[j], above[j / (size_t)nt], connectivity, max_groups(ctx), labels.blocks[i].parent,
                                        labels.blocks[i].size, rec, S > 1 ? reinterpret_cast<uint32_t *>(rec + kCompWords) : nullptr,
                                        sl.compute));
        }
        GS_HIP(hipMemcpyAsync(local.data() + i * slab_words, dev, slab_words * sizeof(uint64_t), hipMemcpyDeviceToHost, sl.compute));
    }
    GS_TRY(sync_compute(ctx));
    std::vector<uint64_t> all;
    if (ctx->world == 1) {
        all.swap(local);
    } else { // every rank's slabs to every rank, in rank order: global slab order
        all.resize((size_t)S * slab_words);
        GS_TRY(exchange(ctx, local.data(), std::vector<size_t>((size_t)ctx->world, nslab * slab_words * sizeof(uint64_t)),
                        "components", all.data()));
    }
    std::vector<gs_components> part;
    std::vector<CompSeamRows> seam;
    for (size_t j = 0; j < results; ++j) {
        part.clear();
        seam.clear();
        for (uint64_t k = 0; k < S; ++k) {
            if (slab_rows(k) == 0) continue;
            const uint64_t *rec = all.data() + (size_t)k * slab_words + j * rec_words;
            gs_components c;
            std::memcpy(&c, rec, sizeof c);
            part.push_back(c);
            const uint32_t *rows = reinterpret_cast<const uint32_t *>(rec + kCompWords);
            seam.push_back(CompSeamRows{rows, rows + cols, rows + 2 * cols, rows + 3 * cols});
        }
        out[j] = merge_components(part.data(), seam.data(), part.size(), cols, connectivity);
    }
    return GS_OK;
}

int32_t gs_members_components(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float *thresholds,
                              const int32_t above[2], int32_t nt, int32_t connectivity, gs_components *out)
{
    if (!ctx || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_thresholds(thresholds, 2, nt)); // before the ensemble is looked at
    GS_TRY(check_connectivity(connectivity));
    GS_TRY(check_members(ctx, e, first, count));
    const uint64_t cells = e->rows * e->cols;
    const size_t passes = 2 * (size_t)nt, results = (size_t)count * passes;
    std::memset(out, 0, results * sizeof(gs_components));
    if (cells == 0 || count == 0) return GS_OK;
    GS_TRY(check_member_labels(cells));
    const uint64_t batch = member_batch(cells, count);
    SlabRt &sl = ctx->slabs[0];
    LabelMemory labels;
    GS_TRY(labels.add(sl.device, batch * cells));
    const size_t words = (size_t)batch * passes * kCompWords;
    GS_TRY(ensure_scratch(ctx, 0, words * sizeof(uint64_t), "components"));
    GS_HIP(hipSetDevice(sl.device));
    unsigned long long *dev = static_cast<unsigned long long *>(sl.scratch);
    std::vector<uint64_t> host(words);
    for (uint64_t b0 = 0; b0 < count; b0 += batch) {
        const uint64_t nb = count - b0 < batch ? count - b0 : batch;
        GS_HIP(hipMemsetAsync(dev, 0, words * sizeof(uint64_t), sl.compute));
        // pass q = s * nt + k: species s of the batch's members at threshold k, each member a plane of its own -- `cells` floats
        // from one to the next; it never sees its neighbours' rows
        for (size_t q = 0; q < passes; ++q) {
            const int s = (int)(q / (size_t)nt);
            const float *plane = (s ? e->v[e->cur] : e->u[e->cur]) + (first + b0) * cells;
            GS_HIP(gs_launch_components(plane, (int64_t)nb, (int64_t)cells, (int64_t)e->cols, (int64_t)e->rows, (int32_t)e->cols,
                                        thresholds[q], above[s], connectivity, max_groups(ctx), labels.blocks[0].parent,
                                        labels.blocks[0].size, dev + q * (size_t)nb * kCompWords, nullptr, sl.compute));
        }
        GS_HIP(hipMemcpyAsync(host.data(), dev, words * sizeof(uint64_t), hipMemcpyDeviceToHost, sl.compute));
        GS_HIP(hipStreamSynchronize(sl.compute));
        for (size_t q = 0; q < passes; ++q)
            for (uint64_t i = 0; i < nb; ++i)
                std::memcpy(&out[(size_t)(b0 + i) * passes + q], host.data() + (q * (size_t)nb + (size_t)i) * kCompWords,
                            sizeof(gs_components));
    }
    return GS_OK;
}

int32_t gs_field_component_list(gs_ctx *ctx, gs_field *f, float threshold, int32_t above, int32_t connectivity, uint64_t min_size,
                                gs_component_list **out)
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_list_rule(threshold, connectivity, min_size)); // before any handle is looked at
    if (!f || f->ctx != ctx) return fail(GS_ERR_INVALID, "field: null or of another context");
    GS_TRY(refuse_world(ctx)); // every rank alone, before anything is allocated or sent
    GS_TRY(sync_all(ctx));
    std::unique_ptr<gs_component_list> list(new (std::nothrow) gs_component_list);
    if (!list) return fail(GS_ERR_NOMEM, "a component list");
    list->planes = 1;
    list->offsets.assign(2, (uint64_t)0);
    if (f->rows == 0 || f->cols == 0) {
        *out = list.release();
        return GS_OK;
    }
    GS_TRY(check_list_sums(f->rows, f->cols, false));
    GS_TRY(check_slab_labels(ctx, f));
    const size_t nslab = ctx->slabs.size(), cols = (size_t)f->cols;
    const bool chain = nslab > 1;
    LabelMemory labels;
    for (size_t i = 0; i < nslab; ++i) {
        const uint64_t cells = (uint64_t)f->s[i].rows * (uint64_t)cols;
        GS_TRY(labels.add(ctx->slabs[i].device, cells, chain ? (cells + 31) / 32 : 0));
        GS_TRY(ensure_scratch(ctx, (int)i, list_work_bytes(cells, cols), "component list"));
    }
    ChainListing listing(ctx, f, labels, 0, min_size);
    for (size_t i = 0; i < nslab; ++i) {
        if (f->s[i].rows == 0) continue;
        SlabRt &sl = ctx->slabs[i];
        GS_HIP(hipSetDevice(sl.device));
        GS_HIP(gs_launch_component_labels(f->s[i].row0, 1, 0, f->pitch, (int64_t)f->s[i].rows, (int32_t)cols, threshold, above,
                                          connectivity, labels.blocks[i].parent, labels.blocks[i].size, sl.compute));
        GS_TRY(listing.count(i));
    }
    GS_TRY(sync_compute(ctx)); // the one read-back: the record memory is sized exactly
    RecordMemory memory;
    for (size_t i = 0; i < nslab; ++i)
        if (f->s[i].rows != 0) GS_TRY(listing.fill(i, memory));
    GS_TRY(sync_compute(ctx));
    listing.finish(connectivity, list.get());
    *out = list.release();
    return GS_OK;
}

int32_t gs_members_component_list(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, int32_t species, float threshold,
                                  int32_t above, int32_t connectivity, uint64_t min_size, gs_component_list **out)
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_list_rule(threshold, connectivity, min_size)); // before the ensemble is looked at
    if (species < 0 || species > 1) return fail(GS_ERR_INVALID, "species %d (0 = U, 1 = V)", species);
    if (e && e->ctx == ctx) GS_TRY(refuse_world(ctx)); // (before check_members waits for anything)
    GS_TRY(check_members(ctx, e, first, count));
    std::unique_ptr<gs_component_list> list(new (std::nothrow) gs_component_list);
    if (!list) return fail(GS_ERR_NOMEM, "a component list");
    list->planes = count;
    list->offsets.assign((size_t)count + 1, (uint64_t)0);
    const uint64_t cells = e->rows * e->cols;
    if (cells == 0 || count == 0) {
        *out = list.release();
        return GS_OK;
    }
    GS_TRY(check_member_labels(cells));
    GS_TRY(check_list_sums(e->rows, e->cols, true));
    // batches of whole members in one block of label memory, as gs_members_components takes them
    const uint64_t batch = member_batch(cells, count);
    SlabRt &sl = ctx->slabs[0];
    LabelMemory labels;
    GS_TRY(labels.add(sl.device, batch * cells));
    GS_TRY(ensure_scratch(ctx, 0, list_work_bytes(batch * cells, 0), "component list"));
    GS_HIP(hipSetDevice(sl.device));
    const LabelMemory::Block &lb = labels.blocks[0];
    BatchListing listing(ctx, e, lb, batch, 0, min_size);
    for (uint64_t b0 = 0; b0 < count; b0 += batch) {
        const uint64_t nb = count - b0 < batch ? count - b0 : batch;
        // each member a plane of its own, `cells` floats from one to the next: it never sees its neighbours' rows
        const float *plane = (species ? e->v[e->cur] : e->u[e->cur]) + (first + b0) * cells;
        GS_HIP(gs_launch_component_labels(plane, (int64_t)nb, (int64_t)cells, (int64_t)e->cols, (int64_t)e->rows, (int32_t)e->cols,
                                          threshold, above, connectivity, lb.parent, lb.size, sl.compute));
        GS_TRY(listing.count(nb));
        GS_HIP(hipStreamSynchronize(sl.compute));
        RecordMemory memory; // (of this batch)
        GS_TRY(listing.fill(b0, nb, memory, list.get()));
    }
    for (size_t i = 0; i < (size_t)count; ++i) list->offsets[i + 1] += list->offsets[i];
    *out = list.release();
    return GS_OK;
}

int32_t gs_component_list_view(const gs_component_list *list, uint64_t *planes, const uint64_t **offsets,
                               const gs_component_record **records)
{
    if (!list || !planes || !offsets || !records) return fail(GS_ERR_INVALID, "null argument");
    *planes = list->planes;
    *offsets = list->offsets.data();
    *records = list->records.data();
    return GS_OK;
}

int32_t gs_component_list_destroy(gs_component_list *list)
{
    delete list;
    return GS_OK;
}

int32_t gs_fields_match(gs_ctx *ctx, gs_field *before, gs_field *after, float threshold, int32_t above, int32_t connectivity,
                        uint64_t min_size, gs_component_match **out)
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_list_rule(threshold, connectivity, min_size)); // before any handle is looked at
    if (!before || before->ctx != ctx || !after || after->ctx != ctx) return fail(GS_ERR_INVALID, "field: null or of another context");
    GS_TRY(same_shape(before, after));
    GS_TRY(refuse_world(ctx, "component matches")); // every rank alone, before anything is allocated or sent
    GS_TRY(sync_all(ctx));
    std::unique_ptr<gs_component_match> match(new (std::nothrow) gs_component_match);
    if (!match) return fail(GS_ERR_NOMEM, "a component match");
    gs_field *const side[2] = {before, after};
    gs_component_list *const lists[2] = {&match->before, &match->after};
    for (gs_component_list *l : lists) {
        l->planes = 1;
        l->offsets.assign(2, (uint64_t)0);
    }
    match->offsets.assign(2, (uint64_t)0);
    const gs_field *f = before;
    if (f->rows == 0 || f->cols == 0) {
        *out = match.release();
        return GS_OK;
    }
    GS_TRY(check_list_sums(f->rows, f->cols, false));
    GS_TRY(check_slab_labels(ctx, f));
    const size_t nslab = ctx->slabs.size(), cols = (size_t)f->cols;
    const bool chain = nslab > 1;
    // label memory: 0 before, 1 after, 2 the pieces (no marks: a piece is listed whatever its size)
    LabelMemory labels[3];
    for (size_t i = 0; i < nslab; ++i) {
        const uint64_t cells = (uint64_t)f->s[i].rows * (uint64_t)cols;
        for (int k = 0; k < 3; ++k) GS_TRY(labels[k].add(ctx->slabs[i].device, cells, chain && k < 2 ? (cells + 31) / 32 : 0));
        GS_TRY(ensure_scratch(ctx, (int)i, match_work_bytes(cells, cols), "component match"));
    }
    // (the pieces are counted as a list is; their records are the overlaps below)
    ChainListing listing[3] = {{ctx, f, labels[0], 0, min_size}, {ctx, f, labels[1], 1, min_size}, {ctx, f, labels[2], 2, 1}};
    for (size_t i = 0; i < nslab; ++i) {
        if (f->s[i].rows == 0) continue;
        SlabRt &sl = ctx->slabs[i];
        const int64_t rows = (int64_t)f->s[i].rows;
        GS_HIP(hipSetDevice(sl.device));
        for (int k = 0; k < 3; ++k) {
            const LabelMemory::Block &lb = labels[k].blocks[i];
            if (k < 2)
                GS_HIP(gs_launch_component_labels(side[k]->s[i].row0, 1, 0, side[k]->pitch, rows, (int32_t)cols, threshold, above,
                                                  connectivity, lb.parent, lb.size, sl.compute));
            else
                GS_HIP(gs_launch_piece_labels(labels[0].blocks[i].parent, labels[1].blocks[i].parent, 1, rows, (int32_t)cols,
                                              connectivity, lb.parent, lb.size, sl.compute));
            GS_TRY(listing[k].count(i));
        }
    }
    GS_TRY(sync_compute(ctx)); // the one read-back: record and overlap memory are sized exactly
    RecordMemory memory; // (the records and the overlaps)
    std::vector<std::vector<gs_component_overlap>> raw(nslab);
    for (size_t i = 0; i < nslab; ++i) {
        if (f->s[i].rows == 0) continue;
        SlabRt &sl = ctx->slabs[i];
        GS_HIP(hipSetDevice(sl.device));
        for (int k = 0; k < 2; ++k) GS_TRY(listing[k].fill(i, memory));
        // a piece names records only where both lists have some: otherwise every piece of the slab is dropped
        const uint32_t np = listing[2].selected[i];
        if (np == 0 || listing[0].selected[i] == 0 || listing[1].selected[i] == 0) continue;
        GsMatchOverlap *dev = nullptr;
        GS_TRY(memory.add(sl.device, np, &dev));
        raw[i].resize(np);
        const GsListWork work = list_work(listing[2].work(i), nullptr);
        GS_HIP(gs_launch_match_pairs(labels[0].blocks[i].parent, labels[0].blocks[i].size, labels[1].blocks[i].parent,
                                     labels[1].blocks[i].size, labels[2].blocks[i].parent, labels[2].blocks[i].size, work.counts, 1,
                                     (int64_t)f->s[i].rows, (int32_t)cols, dev, sl.compute));
        GS_HIP(hipMemcpyAsync(raw[i].data(), dev, (size_t)np * sizeof(gs_component_overlap), hipMemcpyDeviceToHost, sl.compute));
    }
    GS_TRY(sync_compute(ctx));
    std::vector<uint32_t> where[2];
    for (int k = 0; k < 2; ++k) listing[k].finish(connectivity, lists[k], &where[k]);
    // slab-local record indices to those of the two lists; then one overlap per pair
    std::vector<gs_component_overlap> all;
    int64_t base[2] = {0, 0};
    for (size_t i = 0; i < nslab; ++i) {
        if (chain)
            map_overlaps(raw[i].data(), raw[i].size(), where[0].data(), base[0], where[1].data(), base[1]);
        all.insert(all.end(), raw[i].begin(), raw[i].end());
        for (int k = 0; k < 2; ++k) base[k] += (int64_t)listing[k].selected[i];
    }
    match->overlaps = fold_overlaps(all.data(), all.size());
    match->offsets[1] = match->overlaps.size();
    *out = match.release();
    return GS_OK;
}

int32_t gs_members_match(gs_ctx *ctx, gs_ensemble *before, gs_ensemble *after, uint64_t first, uint64_t count, int32_t species,
                         float threshold, int32_t above, int32_t connectivity, uint64_t min_size, gs_component_match **out)
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_list_rule(threshold, connectivity, min_size)); // before the ensembles are looked at
    if (species < 0 || species > 1) return fail(GS_ERR_INVALID, "species %d (0 = U, 1 = V)", species);
    if (before && after && before->ctx == ctx && after->ctx == ctx) GS_TRY(refuse_world(ctx, "component matches")); // (before check_members waits)
    GS_TRY(check_members(ctx, after, first, count, before, true));
    std::unique_ptr<gs_component_match> match(new (std::nothrow) gs_component_match);
    if (!match) return fail(GS_ERR_NOMEM, "a component match");
    const gs_ensemble *const side[2] = {before, after};
    gs_component_list *const lists[2] = {&match->before, &match->after};
    for (gs_component_list *l : lists) {
        l->planes = count;
        l->offsets.assign((size_t)count + 1, (uint64_t)0);
    }
    match->offsets.assign((size_t)count + 1, (uint64_t)0);
    const gs_ensemble *e = after;
    const uint64_t cells = e->rows * e->cols;
    if (cells == 0 || count == 0) {
        *out = match.release();
        return GS_OK;
    }
    GS_TRY(check_member_labels(cells));
    GS_TRY(check_list_sums(e->rows, e->cols, true));
    // batches of whole members, as gs_members_component_list takes them: each of the three labellings within the budget
    const uint64_t batch = member_batch(cells, count);
    SlabRt &sl = ctx->slabs[0];
    LabelMemory labels; // blocks 0 before, 1 after, 2 the pieces
    for (int k = 0; k < 3; ++k) GS_TRY(labels.add(sl.device, batch * cells));
    GS_TRY(ensure_scratch(ctx, 0, match_work_bytes(batch * cells, 0), "component match"));
    GS_HIP(hipSetDevice(sl.device));
    const int64_t rows = (int64_t)e->rows;
    const int32_t cols = (int32_t)e->cols;
    // (the pieces are counted as a list is; their records are the overlaps below)
    BatchListing listing[3] = {{ctx, e, labels.blocks[0], batch, 0, min_size}, {ctx, e, labels.blocks[1], batch, 1, min_size},
                               {ctx, e, labels.blocks[2], batch, 2, 1}};
    std::vector<gs_component_overlap> raw;
    for (uint64_t b0 = 0; b0 < count; b0 += batch) {
        const uint64_t nb = count - b0 < batch ? count - b0 : batch;
        for (int k = 0; k < 3; ++k) {
            const LabelMemory::Block &lb = labels.blocks[(size_t)k];
            if (k < 2) {
                // each member a plane of its own, `cells` floats from one to the next: it never sees its neighbours' rows
                const gs_ensemble *m = side[k];
                const float *plane = (species ? m->v[m->cur] : m->u[m->cur]) + (first + b0) * cells;
                GS_HIP(gs_launch_component_labels(plane, (int64_t)nb, (int64_t)cells, (int64_t)cols, rows, cols, threshold, above,
                                                  connectivity, lb.parent, lb.size, sl.compute));
            } else {
                GS_HIP(gs_launch_piece_labels(labels.blocks[0].parent, labels.blocks[1].parent, (int64_t)nb, rows, cols, connectivity,
                                              lb.parent, lb.size, sl.compute));
            }
            GS_TRY(listing[k].count(nb));
        }
        GS_HIP(hipStreamSynchronize(sl.compute));
        RecordMemory memory; // (of this batch: the records and the overlaps)
        for (int k = 0; k < 2; ++k) GS_TRY(listing[k].fill(b0, nb, memory, lists[k]));
        const uint32_t np = listing[2].selected;
        if (np == 0 || listing[0].selected == 0 || listing[1].selected == 0) continue; // (no piece names a record)
        GsMatchOverlap *dev = nullptr;
        GS_TRY(memory.add(sl.device, np, &dev));
        raw.resize(np);
        GS_HIP(gs_launch_match_pairs(labels.blocks[0].parent, labels.blocks[0].size, labels.blocks[1].parent, labels.blocks[1].size,
                                     labels.blocks[2].parent, labels.blocks[2].size, listing[2].work.counts, (int64_t)nb, rows, cols, dev,
                                     sl.compute));
        GS_HIP(hipMemcpyAsync(raw.data(), dev, raw.size() * sizeof(gs_component_overlap), hipMemcpyDeviceToHost, sl.compute));
        GS_HIP(hipStreamSynchronize(sl.compute));
        fold_batch_overlaps(raw.data(), raw.size(), listing[0].before.data(), listing[1].before.data(), (size_t)nb, match->overlaps,
                            &match->offsets[(size_t)b0 + 1]);
    }
    for (size_t i = 0; i < (size_t)count; ++i) {
        for (gs_component_list *l : lists) l->offsets[i + 1] += l->offsets[i];
        match->offsets[i + 1] += match->offsets[i];
    }
    *out = match.release();
    return GS_OK;
}

int32_t gs_component_match_view(const gs_component_match *match, const gs_component_list **before, const gs_component_list **after,
                                uint64_t *planes, const uint64_t **offsets, const gs_component_overlap **overlaps)
{
    if (!match || !before || !after || !planes || !offsets || !overlaps) return fail(GS_ERR_INVALID, "null argument");
    *before = &match->before;
    *after = &match->after;
    *planes = match->before.planes;
    *offsets = match->offsets.data();
    *overlaps = match->overlaps.data();
    return GS_OK;
}

int32_t gs_component_match_destroy(gs_component_match *match)
{
    delete match;
    return GS_OK;
}

int32_t gs_region_grid(uint64_t rows, uint64_t cols, int32_t rh, int32_t rw, uint64_t *rr, uint64_t *rc)
{
    if (!rr || !rc) return fail(GS_ERR_INVALID, "null argument");
    return region_grid(rows, cols, rh, rw, rr, rc);
}

int32_t gs_fields_region_summaries(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw, gs_summary *out)
{
    if (!ctx || !fields || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_regions(ctx, fields, n, rh, rw));
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    uint64_t RR, RC;
    GS_TRY(region_grid(f0->rows, f0->cols, rh, rw, &RR, &RC));
    if (RR * RC == 0) return GS_OK; // an empty plane has no regions; the same shape on every rank: nobody exchanges anything
    // a region's record is gs_summary's layout: the results land in `out` as they are
    static_assert(sizeof(GsRegionSummary) == sizeof(gs_summary) && offsetof(GsRegionSummary, min) == offsetof(gs_summary, min) &&
                      offsetof(GsRegionSummary, nonfinite) == offsetof(gs_summary, nonfinite),
                  "region record layout");
    return band_results(ctx, f0, n, rh, RR, RC, sizeof(GsRegionSummary), false, "region summary",
                        reinterpret_cast<unsigned char *>(out), [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *planes[4];
        slab_planes(fields, n, i, planes);
        return gs_launch_region_summary(planes, n, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, rh, rw,
                                        reinterpret_cast<GsRegionSummary *>(dev), s);
    });
}

int32_t gs_fields_region_morphology(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw, const float *thresholds,
                                    const int32_t *above, int32_t nt, gs_morphology *out)
{
    if (!ctx || !fields || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_thresholds(thresholds, n, nt));
    GS_TRY(check_regions(ctx, fields, n, rh, rw));
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    uint64_t RR, RC;
    GS_TRY(region_grid(f0->rows, f0->cols, rh, rw, &RR, &RC));
    if (RR * RC == 0) return GS_OK;
    // The counters land in `out` as they are -- six words per result, Q0's left zero by the launch: with up to 2^22 regions
    // a buffer between the device and the caller's memory would be tens of MiB of freshly mapped pages in every call, whose
    // first touch under the copy costs more than the launch (profiles/regions.md).
    GS_TRY(band_results(ctx, f0, n, rh, RR, RC, (size_t)nt * sizeof(gs_morphology), true, "region morphology",
                        reinterpret_cast<unsigned char *>(out), [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *planes[4];
        slab_planes(fields, n, i, planes);
        return gs_launch_region_quads(planes, n, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, rh, rw, thresholds, above,
                                      nt, max_groups(ctx), reinterpret_cast<unsigned long long *>(dev), s);
    }));
    const uint64_t q = (uint64_t)rh, w = (uint64_t)rw;
    for (size_t p = 0; p < (size_t)n; ++p)
        for (uint64_t i = 0; i < RR; ++i)
            for (uint64_t j = 0; j < RC; ++j) {
                // the region's own rows and columns: ragged in the last row and column of the region grid
                const uint64_t h = std::min(q, f0->rows - i * q), c = std::min(w, f0->cols - j * w);
                const size_t at = (p * (size_t)RR + (size_t)i) * (size_t)RC + (size_t)j;
                for (size_t k = 0; k < (size_t)nt; ++k) {
                    gs_morphology &m = out[at * (size_t)nt + k];
                    m = from_counted(m.quads + 1, h, c);
                }
            }
    return GS_OK;
}

int32_t gs_fields_region_correlation(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw, const float *thresholds,
                                     const int32_t *above, int32_t nt, int32_t max_lag, uint64_t *out)
{
    if (!ctx || !fields || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    uint64_t RR, RC;
    GS_TRY(region_grid(0, 0, rh, rw, &RR, &RC)); // the region shape alone; no handle is looked at down to check_planes
    GS_TRY(check_thresholds(thresholds, n, nt));
    GS_TRY(check_max_lag(max_lag));
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    GS_TRY(region_grid(f0->rows, f0->cols, rh, rw, &RR, &RC));
    if (RR * RC == 0) return GS_OK; // an empty plane has no regions; the same shape on every rank: nobody exchanges anything
    const uint64_t per_region = (uint64_t)nt * 4 * (uint64_t)(max_lag + 1); // (at most 1040: no product here can wrap)
    if (RR * RC * per_region > (uint64_t)GS_REGION_PAIRS_MAX)
        return fail(GS_ERR_INVALID, "%llu x %llu regions of %llu counters each (at most %u counters per field)",
                    (unsigned long long)RR, (unsigned long long)RC, (unsigned long long)per_region, (unsigned)GS_REGION_PAIRS_MAX);
    // the counters land in `out` as they are, as the bit quads' do
    return band_results(ctx, f0, n, rh, RR, RC, (size_t)per_region * sizeof(uint64_t), true, "region correlation",
                        reinterpret_cast<unsigned char *>(out), [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *planes[4];
        slab_planes(fields, n, i, planes);
        return gs_launch_region_pairs(planes, n, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, rh, rw, thresholds, above,
                                      nt, max_lag, max_groups(ctx), reinterpret_cast<unsigned long long *>(dev), s);
    });
}

int32_t gs_fields_region_histogram(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw, const float *lo,
                                   const float *hi, int32_t bins, uint64_t *out)
{
    if (!ctx || !fields || !lo || !hi || !out) return fail(GS_ERR_INVALID, "null argument");
    uint64_t RR, RC;
    GS_TRY(region_grid(0, 0, rh, rw, &RR, &RC)); // the region shape alone; no handle is looked at down to check_planes
    // bins, then the ranges of fields 0 .. n - 1 (a count that is no 1..4 is check_planes' first refusal: no range is read)
    float scale[4];
    GS_TRY(check_ranges(lo, hi, n >= 1 && n <= 4 ? n : 0, bins, scale));
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    GS_TRY(region_grid(f0->rows, f0->cols, rh, rw, &RR, &RC));
    if (RR * RC == 0) return GS_OK; // an empty plane has no regions; the same shape on every rank: nobody exchanges anything
    const uint64_t per_region = (uint64_t)bins + 3; // (at most 4099: no product here can wrap)
    if (RR * RC * per_region > (uint64_t)GS_REGION_HIST_MAX)
        return fail(GS_ERR_INVALID, "%llu x %llu regions of %llu counters each (at most %u counters per field)",
                    (unsigned long long)RR, (unsigned long long)RC, (unsigned long long)per_region, (unsigned)GS_REGION_HIST_MAX);
    // the counters land in `out` as they are, as the bit quads' do
    return band_results(ctx, f0, n, rh, RR, RC, (size_t)per_region * sizeof(uint64_t), true, "region histogram",
                        reinterpret_cast<unsigned char *>(out), [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *planes[4];
        slab_planes(fields, n, i, planes);
        return gs_launch_region_hist(planes, n, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, rh, rw, lo, hi, scale, bins,
                                     max_groups(ctx), reinterpret_cast<unsigned long long *>(dev), s);
    });
}

int32_t gs_fields_region_components(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw,
                                    const float *thresholds, const int32_t *above, int32_t nt, int32_t connectivity,
                                    gs_components *out)
{
    if (!ctx || !fields || !thresholds || !above || !out) return fail(GS_ERR_INVALID, "null argument");
    uint64_t RR, RC;
    GS_TRY(region_grid(0, 0, rh, rw, &RR, &RC)); // the region shape alone; no handle is looked at down to check_planes
    GS_TRY(check_thresholds(thresholds, n, nt));
    GS_TRY(check_connectivity(connectivity));
    GS_TRY(check_planes(ctx, fields, n));
    GS_TRY(check_regions(ctx, fields, n, rh, rw));
    const gs_field *f0 = fields[0];
    GS_TRY(region_grid(f0->rows, f0->cols, rh, rw, &RR, &RC));
    if (RR * RC == 0) return GS_OK; // an empty plane has no regions; the same shape on every rank: nobody exchanges anything
    if (RR * RC * (uint64_t)nt > (uint64_t)GS_REGION_COMPONENTS_MAX) // (at most 2^24: no product here can wrap)
        return fail(GS_ERR_INVALID, "%llu x %llu regions of %d results each (at most %u results per field)", (unsigned long long)RR,
                    (unsigned long long)RC, nt, (unsigned)GS_REGION_COMPONENTS_MAX);
    // every slab of the global grid: every rank reaches the same verdicts
    GS_TRY(check_band_seams(ctx, f0, rh));
    const uint64_t S = (uint64_t)ctx->total_slabs();
    for (uint64_t k = 0; k < S; ++k) {
        const uint64_t rows = global_slab_rows(ctx, f0->rows, k);
        if (rows > 0 && rows >= ((uint64_t)1 << 32) / f0->cols + ((((uint64_t)1 << 32) % f0->cols) ? 1 : 0))
            return fail(GS_ERR_UNSUPPORTED, "slab %llu holds %llu x %llu cells: labels are 32-bit, fewer than 2^32 cells per slab",
                        (unsigned long long)k, (unsigned long long)rows, (unsigned long long)f0->cols);
    }
    const size_t nslab = ctx->slabs.size();
    LabelMemory labels;
    int32_t had = GS_OK;
    for (size_t i = 0; i < nslab && had == GS_OK; ++i)
        had = labels.add(ctx->slabs[i].device, (uint64_t)f0->s[i].rows * f0->cols);
    if (ctx->world > 1) { // the ranks agree on the verdict before anything else is exchanged: nobody waits for a rank that left
        const uint64_t mine = had == GS_OK ? 0 : 1;
        std::vector<uint64_t> verdicts((size_t)ctx->world);
        GS_TRY(exchange(ctx, &mine, std::vector<size_t>((size_t)ctx->world, sizeof mine), "region components", verdicts.data()));
        for (int q = 0; q < ctx->world && had == GS_OK; ++q)
            if (verdicts[(size_t)q]) had = fail(GS_ERR_NOMEM, "rank %d could not have its label memory", q);
    }
    if (had != GS_OK) return had;
    // the counters land in `out` as they are, as the bit quads' do: a region's nt results of 35 words side by side
    static_assert(sizeof(gs_components) == kCompWords * sizeof(uint64_t), "gs_components is its counters");
    const int64_t region_words = (int64_t)nt * (int64_t)kCompWords;
    return band_results(ctx, f0, n, rh, RR, RC, (size_t)nt * sizeof(gs_components), true, "region components",
                        reinterpret_cast<unsigned char *>(out), [&](size_t i, unsigned char *dev, hipStream_t s) {
        // every (plane, threshold) in turn in the slab's label memory: the launches of one are complete before the next begin
        const size_t line = (size_t)((f0->s[i].rows + (uint64_t)rh - 1) / (uint64_t)rh) * (size_t)RC * (size_t)region_words;
        for (int32_t p = 0; p < n; ++p)
            for (int32_t k = 0; k < nt; ++k) {
                unsigned long long *res = reinterpret_cast<unsigned long long *>(dev) + (size_t)p * line + (size_t)k * kCompWords;
                const hipError_t e = gs_launch_region_components(fields[p]->s[i].row0, f0->pitch, (int64_t)f0->s[i].rows,
                                                                 (int32_t)f0->cols, rh, rw, thresholds[p * nt + k], above[p],
                                                                 connectivity, max_groups(ctx), labels.blocks[i].parent,
                                                                 labels.blocks[i].size, region_words, res, s);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    });
}

int32_t gs_fields_region_compare(gs_ctx *ctx, gs_field *const *a, gs_field *const *b, int32_t n, int32_t rh, int32_t rw, gs_change *out)
{
    if (!ctx || !a || !b || !out) return fail(GS_ERR_INVALID, "null argument");
    uint64_t RR, RC;
    GS_TRY(region_grid(0, 0, rh, rw, &RR, &RC)); // the region shape alone; no handle is looked at down to check_planes
    // the route switch of gs_hip.h: read at every call, before any device work
    int forced = 0; // 0: the library's choice, 1: records, 2: wave
    if (const char *route = std::getenv("GS_HIP_REGION_CHANGE_ROUTE")) {
        if (!std::strcmp(route, "records")) forced = 1;
        else if (!std::strcmp(route, "wave")) forced = 2;
        else if (*route) return fail(GS_ERR_INVALID, "GS_HIP_REGION_CHANGE_ROUTE=%s (records, wave or unset)", route);
    }
    GS_TRY(check_planes(ctx, a, n, b));
    const gs_field *f0 = a[0];
    GS_TRY(region_grid(f0->rows, f0->cols, rh, rw, &RR, &RC));
    if (RR * RC == 0) return GS_OK; // an empty plane has no regions; the same shape on every rank: nobody exchanges anything
    GS_TRY(check_band_seams(ctx, f0, rh)); // every rank reaches the same verdict before anybody allocates
    // a region's result is gs_change's layout: the results land in `out` as they are.  The record route's records lie behind
    // a slab's results in its scratch buffer, which is made large enough here: band_results then finds it so and keeps it.
    static_assert(sizeof(GsChangeTotal) == sizeof(gs_change), "region result layout");
    const size_t nslab = ctx->slabs.size();
    std::vector<size_t> records_at(nslab, (size_t)0); // offset of a slab's records in its scratch buffer; 0: the wave route
    for (size_t i = 0; i < nslab; ++i) {
        const int64_t rows = (int64_t)f0->s[i].rows;
        if (rows == 0) continue;
        const bool want = forced == 1 || (forced == 0 && gs_region_change_wants_records(rows, (int32_t)f0->cols, rh, rw, ctx->cu_count));
        const size_t rec_bytes = gs_region_change_record_bytes(n, rows, (int32_t)f0->cols, rw);
        if (!want || rec_bytes > (size_t)GS_REGION_CHANGE_RECORDS_MAX) continue;
        const size_t results = (size_t)n * (size_t)(((uint64_t)rows + (uint64_t)rh - 1) / (uint64_t)rh) * (size_t)RC * sizeof(gs_change);
        records_at[i] = (results + 255) / 256 * 256;
        GS_TRY(ensure_scratch(ctx, (int)i, records_at[i] + rec_bytes, "region comparison"));
    }
    return band_results(ctx, f0, n, rh, RR, RC, sizeof(gs_change), true, "region comparison", reinterpret_cast<unsigned char *>(out),
                        [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *pa[4], *pb[4];
        slab_planes(a, n, i, pa);
        slab_planes(b, n, i, pb);
        return gs_launch_region_change(pa, pb, n, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, rh, rw,
                                       reinterpret_cast<GsChangeTotal *>(dev), records_at[i] ? dev + records_at[i] : nullptr, s);
    });
}

int32_t gs_fields_region_spectrum(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw, int32_t tile,
                                  int32_t window, double *power, uint64_t *tiles)
{
    if (!power || !tiles) return fail(GS_ERR_INVALID, "null output");
    GS_TRY(check_spectrum(tile, window));
    uint64_t RR, RC;
    GS_TRY(region_grid(0, 0, rh, rw, &RR, &RC)); // the region shape alone; no handle is looked at down to check_planes
    if (!ctx || !fields) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_planes(ctx, fields, n));
    const gs_field *f0 = fields[0];
    GS_TRY(region_grid(f0->rows, f0->cols, rh, rw, &RR, &RC));
    if (RR * RC == 0) return GS_OK; // an empty plane has no regions; the same shape on every rank: nobody exchanges anything
    const size_t bins = (size_t)tile * (size_t)(tile / 2 + 1), words = bins + 2, elem = gs_spectrum_result_bytes(tile);
    if (RR * RC * (uint64_t)words > (uint64_t)GS_REGION_SPECTRUM_MAX) // (at most 2^22 * 8322: no product here can wrap)
        return fail(GS_ERR_INVALID, "%llu x %llu regions of %llu words each (at most %u words per field)", (unsigned long long)RR,
                    (unsigned long long)RC, (unsigned long long)words, (unsigned)GS_REGION_SPECTRUM_MAX);
    // the records of the global grid, whatever its slabs: every rank and every slab count reaches the same verdict
    const uint64_t record_words = (uint64_t)n * gs_region_spectrum_records(f0->rows, f0->cols, rh, rw, tile) * (uint64_t)words;
    if (record_words > (uint64_t)GS_REGION_SPECTRUM_RECORDS_MAX)
        return fail(GS_ERR_INVALID, "%llu words of segment records over the %d fields (at most %llu)",
                    (unsigned long long)record_words, n, (unsigned long long)GS_REGION_SPECTRUM_RECORDS_MAX);
    GS_TRY(check_band_seams(ctx, f0, rh)); // every rank reaches the same verdict before anybody allocates
    // a slab's segment records lie behind its regions' results in its scratch buffer, which is made large enough here:
    // band_results then finds it so and keeps it (the regional comparison's precedent)
    const size_t nslab = ctx->slabs.size();
    std::vector<size_t> records_at(nslab, (size_t)0);
    for (size_t i = 0; i < nslab; ++i) {
        const uint64_t rows = (uint64_t)f0->s[i].rows;
        if (rows == 0) continue;
        const size_t results = (size_t)n * (size_t)((rows + (uint64_t)rh - 1) / (uint64_t)rh) * (size_t)RC * elem;
        records_at[i] = (results + 255) / 256 * 256;
        const size_t rec_bytes = (size_t)n * (size_t)gs_region_spectrum_records(rows, f0->cols, rh, rw, tile) * elem;
        GS_TRY(ensure_scratch(ctx, (int)i, records_at[i] + rec_bytes, "region spectrum"));
    }
    float h[128], w[128];
    spectrum_tables(tile, h, w);
    std::vector<unsigned char> results((size_t)n * (size_t)RR * (size_t)RC * elem);
    GS_TRY(band_results(ctx, f0, n, rh, RR, RC, elem, false, "region spectrum", results.data(),
                        [&](size_t i, unsigned char *dev, hipStream_t s) {
        const float *planes[4];
        slab_planes(fields, n, i, planes);
        return gs_launch_region_spectrum(planes, n, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, rh, rw, tile, window, h,
                                         w, dev + records_at[i], dev, s);
    }));
    // the device has finished every region: the host only takes each result apart
    const size_t regions = (size_t)n * (size_t)RR * (size_t)RC;
    for (size_t r = 0; r < regions; ++r) {
        const unsigned char *from = results.data() + r * elem;
        std::memcpy(power + r * bins, from, bins * 8);
        std::memcpy(tiles + 2 * r, from + bins * 8, 16);
    }
    return GS_OK;
}

} // extern "C"
