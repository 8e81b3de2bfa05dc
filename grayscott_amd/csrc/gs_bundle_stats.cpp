// gs_bundle_stats.cpp -- statistics across the members of a bundle (include/gs_hip.h: gs_members_bundle_stats): every run
// of `span` consecutive members of an ensemble folded per cell into result planes, which are written into members of
// ordinary ensembles (gs_bundle_stats.hip: one pass over the members, nothing but the results written).
// Everything is refused before anything is launched; the call then waits for enqueued work the way the other member
// observables do (sync_all), enqueues on slab 0's compute stream, leaves every result ensemble as gs_members_copy leaves
// its target (mark_members_written: an inactive member is mirrored into its other slot before the next run) and waits.
// No call touches the tuner, the graphs or the context's counters.
#include "gs_internal.h"
#include "gs_plane_scan.h"

using namespace gsi;

extern "C" int32_t gs_members_bundle_stats(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, uint64_t span,
                                           const int32_t *which, int32_t n, const float thresholds[2], const int32_t above[2],
                                           gs_ensemble *const *out, uint64_t out_first)
{
    if (!ctx) return fail(GS_ERR_INVALID, "null argument");
    if (ctx->slabs.size() != 1 || ctx->world != 1) // (gs_ensemble_create's refusal)
        return fail(GS_ERR_UNSUPPORTED, "an ensemble lives on a context of one slab in one process (%d slabs x %d processes)",
                    (int)ctx->slabs.size(), ctx->world);
    if (!e || !which || !out) return fail(GS_ERR_INVALID, "null argument");
    if (e->ctx != ctx) return fail(GS_ERR_INVALID, "ensemble belongs to another context");
    if (span == 0) return fail(GS_ERR_INVALID, "a bundle of no members");
    if (count % span != 0)
        return fail(GS_ERR_INVALID, "%llu members are no whole number of bundles of %llu", (unsigned long long)count,
                    (unsigned long long)span);
    if (count > 0)
        GS_TRY(check_member_range(e, first, count));
    else if (first > e->members)
        return fail(GS_ERR_INVALID, "member %llu outside the ensemble's %llu", (unsigned long long)first, (unsigned long long)e->members);
    if (n < 1 || n > 5) return fail(GS_ERR_INVALID, "%d result planes (1..5)", n);
    bool asked[5] = {false, false, false, false, false};
    for (int32_t i = 0; i < n; ++i) {
        if (which[i] < GS_TSTAT_MEAN || which[i] > GS_TSTAT_OCCUPANCY)
            return fail(GS_ERR_INVALID, "no result plane %d across members (GS_TSTAT_MEAN .. GS_TSTAT_OCCUPANCY)", which[i]);
        if (asked[which[i]]) return fail(GS_ERR_INVALID, "result plane %d asked for twice", which[i]);
        asked[which[i]] = true;
    }
    float t[2] = {0.0f, 0.0f};
    uint32_t flip[2] = {0u, 0u};
    if (asked[GS_TSTAT_OCCUPANCY]) {
        if (!thresholds || !above) return fail(GS_ERR_INVALID, "the occupancy needs a threshold and a sense per species");
        for (int sp = 0; sp < 2; ++sp) {
            if (std::isnan(thresholds[sp])) return fail(GS_ERR_INVALID, "threshold %d is NaN", sp);
            gs_set_rule(thresholds[sp], above[sp], t[sp], flip[sp]);
        }
    }
    const uint64_t bundles = count / span;
    for (int32_t i = 0; i < n; ++i) {
        const gs_ensemble *o = out[i];
        if (!o) return fail(GS_ERR_INVALID, "null argument");
        if (o == e) return fail(GS_ERR_INVALID, "result ensemble %d is the ensemble the members are read from", i);
        for (int32_t k = 0; k < i; ++k)
            if (out[k] == o) return fail(GS_ERR_INVALID, "result ensembles %d and %d: one target named twice", k, i);
        if (o->ctx != ctx) return fail(GS_ERR_INVALID, "result ensemble %d belongs to another context", i);
        if (o->rows != e->rows || o->cols != e->cols)
            return fail(GS_ERR_INVALID, "result ensemble %d of [%llu, %llu], members of [%llu, %llu]", i, (unsigned long long)o->rows,
                        (unsigned long long)o->cols, (unsigned long long)e->rows, (unsigned long long)e->cols);
        if (out_first > o->members || bundles > o->members - out_first)
            return fail(GS_ERR_INVALID, "result ensemble %d: members [%llu, %llu + %llu) outside its %llu", i,
                        (unsigned long long)out_first, (unsigned long long)out_first, (unsigned long long)bundles,
                        (unsigned long long)o->members);
    }
    GS_TRY(sync_all(ctx));
    const uint64_t cells = e->rows * e->cols;
    if (bundles == 0 || cells == 0) return GS_OK;
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    // members are read from, and results written into, the newest slot
    const float *in[2] = {e->u[e->cur] + first * cells, e->v[e->cur] + first * cells};
    float *planes[2][5] = {{nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr}};
    for (int32_t i = 0; i < n; ++i) {
        gs_ensemble *o = out[i];
        planes[0][which[i]] = o->u[o->cur] + out_first * cells;
        planes[1][which[i]] = o->v[o->cur] + out_first * cells;
    }
    GS_HIP(gs_launch_bundle_stats(in, planes, (int64_t)cells, (int64_t)span, (int64_t)bundles, t, flip, sl.compute));
    for (int32_t i = 0; i < n; ++i) mark_members_written(out[i], out_first, bundles);
    GS_HIP(hipStreamSynchronize(sl.compute));
    return GS_OK;
}
