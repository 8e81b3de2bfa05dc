// gs_summary.cpp -- summaries of planes and ensemble members (include/gs_hip.h: gs_fields_summarize,
// gs_members_summarize).  The row records come from gs_row_summary_k (gs_summary.hip), one launch per slab on its compute
// stream; the field fold -- rows added in ascending global row order -- is done here on the host, after the records of
// every slab (and, in a multi-process context, of every rank: allgather_bytes) have met.  Ensembles fold on the device
// (gs_summary_fold_k), so that two records per member travel.  Nothing here touches ghost rows, the tuner, graphs or the
// context's counters.
#include "gs_internal.h"

using namespace gsi;

namespace {

static_assert(sizeof(GsRowSummary) == 32, "row record layout");
static_assert(sizeof(gs_summary) == 32 && offsetof(gs_summary, min) == 16 && offsetof(gs_summary, nonfinite) == 24,
              "gs_summary layout");

int32_t ensure_buffer(gs_ctx *ctx, int i, size_t bytes)
{
    SlabRt &sl = ctx->slabs[(size_t)i];
    if (sl.summary_bytes >= bytes) return GS_OK;
    GS_HIP(hipSetDevice(sl.device));
    if (sl.summary) GS_HIP(hipFree(sl.summary));
    sl.summary = nullptr;
    sl.summary_bytes = 0;
    const hipError_t e = hipMalloc(&sl.summary, bytes);
    if (e != hipSuccess) return fail(GS_ERR_NOMEM, "summary buffer of %zu bytes: %s", bytes, hipGetErrorString(e));
    sl.summary_bytes = bytes;
    return GS_OK;
}

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

} // namespace

namespace gsi {

void destroy_summary_buffers(gs_ctx *ctx)
{
    for (auto &sl : ctx->slabs) {
        if (!sl.summary) continue;
        if (hipSetDevice(sl.device) == hipSuccess) (void)hipFree(sl.summary);
        sl.summary = nullptr;
        sl.summary_bytes = 0;
    }
}

} // namespace gsi

extern "C" {

int32_t gs_fields_summarize(gs_ctx *ctx, gs_field *const *fields, int32_t n, gs_summary *out)
{
    if (!ctx || !fields || !out) return fail(GS_ERR_INVALID, "null argument");
    if (n < 1 || n > 4) return fail(GS_ERR_INVALID, "%d fields (1..4)", n);
    for (int32_t p = 0; p < n; ++p) {
        if (!fields[p] || fields[p]->ctx != ctx) return fail(GS_ERR_INVALID, "field %d: null or of another context", p);
        if (p > 0) GS_TRY(same_shape(fields[0], fields[p]));
    }
    GS_TRY(sync_all(ctx)); // (also runs again a persistent window launch that gave up: no stale plane is read)
    const gs_field *f0 = fields[0];
    if (f0->rows == 0 || f0->cols == 0) { // the same shape on every rank: nobody exchanges anything
        for (int32_t p = 0; p < n; ++p) out[p] = empty_summary();
        return GS_OK;
    }
    // records of this process's rows, [plane][local row]
    const size_t nslab = ctx->slabs.size();
    size_t local_rows = 0;
    for (const FieldSlab &fs : f0->s) local_rows += (size_t)fs.rows;
    std::vector<GsRowSummary> local((size_t)n * local_rows);
    size_t row_at = 0;
    for (size_t i = 0; i < nslab; ++i) {
        SlabRt &sl = ctx->slabs[i];
        const size_t rows = (size_t)f0->s[i].rows;
        GS_TRY(ensure_buffer(ctx, (int)i, (size_t)n * rows * sizeof(GsRowSummary)));
        GS_HIP(hipSetDevice(sl.device));
        const float *planes[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int32_t p = 0; p < n; ++p) planes[p] = fields[p]->s[i].row0;
        GsRowSummary *rec = static_cast<GsRowSummary *>(sl.summary);
        GS_HIP(gs_launch_row_summary(planes, n, f0->pitch, (int64_t)rows, (int32_t)f0->cols, rec, sl.compute));
        for (int32_t p = 0; p < n; ++p)
            GS_HIP(hipMemcpyAsync(local.data() + (size_t)p * local_rows + row_at, rec + (size_t)p * rows,
                                  rows * sizeof(GsRowSummary), hipMemcpyDeviceToHost, sl.compute));
        row_at += rows;
    }
    for (auto &sl : ctx->slabs) {
        GS_HIP(hipSetDevice(sl.device));
        GS_HIP(hipStreamSynchronize(sl.compute));
    }
    if (ctx->world == 1) {
        for (int32_t p = 0; p < n; ++p) out[p] = fold_rows(local.data() + (size_t)p * local_rows, local_rows);
        return GS_OK;
    }
    // Several processes: every rank's records to every rank (rank q holds global rows [q L R / S, (q + 1) L R / S) of
    // S = world x L slabs, the partition of gs_field_create), then the same fold everywhere.
    const uint64_t S = (uint64_t)ctx->total_slabs(), L = (uint64_t)nslab, R = f0->rows;
    std::vector<size_t> bytes((size_t)ctx->world);
    size_t total = 0;
    for (int q = 0; q < ctx->world; ++q) {
        const uint64_t r0 = (uint64_t)q * L * R / S, r1 = (uint64_t)(q + 1) * L * R / S;
        bytes[(size_t)q] = (size_t)n * (size_t)(r1 - r0) * sizeof(GsRowSummary);
        total += bytes[(size_t)q];
    }
    const size_t mine = bytes[(size_t)ctx->rank];
    if (mine != local.size() * sizeof(GsRowSummary)) return fail(GS_ERR_INVALID, "row partition disagrees with this process's slabs");
    SlabRt &sl = ctx->slabs[0];
    GS_TRY(ensure_buffer(ctx, 0, mine + total));
    GS_HIP(hipSetDevice(sl.device));
    unsigned char *send = static_cast<unsigned char *>(sl.summary), *recv = send + mine;
    GS_HIP(hipMemcpyAsync(send, local.data(), mine, hipMemcpyHostToDevice, sl.compute));
    GS_TRY(allgather_bytes(ctx, send, recv, bytes, sl.compute));
    std::vector<GsRowSummary> all(total / sizeof(GsRowSummary));
    GS_HIP(hipMemcpyAsync(all.data(), recv, total, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    // rank blocks in rank order, each [plane][its rows]: plane p's records in global row order, then the one fold
    std::vector<GsRowSummary> plane((size_t)R);
    for (int32_t p = 0; p < n; ++p) {
        size_t at = 0, row = 0;
        for (int q = 0; q < ctx->world; ++q) {
            const size_t rows = bytes[(size_t)q] / sizeof(GsRowSummary) / (size_t)n;
            std::memcpy(plane.data() + row, all.data() + at + (size_t)p * rows, rows * sizeof(GsRowSummary));
            at += (size_t)n * rows;
            row += rows;
        }
        out[p] = fold_rows(plane.data(), plane.size());
    }
    return GS_OK;
}

int32_t gs_members_summarize(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, gs_summary *out)
{
    if (!ctx || !e || !out) return fail(GS_ERR_INVALID, "null argument");
    if (e->ctx != ctx) return fail(GS_ERR_INVALID, "ensemble belongs to another context");
    if (count == 0 || first >= e->members || count > e->members - first)
        return fail(GS_ERR_INVALID, "members [%llu, %llu + %llu) outside the ensemble's %llu", (unsigned long long)first,
                    (unsigned long long)first, (unsigned long long)count, (unsigned long long)e->members);
    GS_TRY(sync_all(ctx));
    const uint64_t cells = e->rows * e->cols, rows = count * e->rows;
    const size_t rec_bytes = (size_t)(2 * rows) * sizeof(GsRowSummary), out_bytes = (size_t)(2 * count) * sizeof(GsRowSummary);
    GS_TRY(ensure_buffer(ctx, 0, rec_bytes + out_bytes));
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GsRowSummary *rec = static_cast<GsRowSummary *>(sl.summary), *folded = rec + 2 * rows;
    // the members' rows one after the other: one plane of count x rows rows, pitch cols
    const float *planes[2] = {e->u[e->cur] + first * cells, e->v[e->cur] + first * cells};
    GS_HIP(gs_launch_row_summary(planes, 2, (int64_t)e->cols, (int64_t)rows, (int32_t)e->cols, rec, sl.compute));
    GS_HIP(gs_launch_summary_fold(rec, (int64_t)count, (int64_t)e->rows, folded, sl.compute));
    std::vector<GsRowSummary> host((size_t)(2 * count));
    GS_HIP(hipMemcpyAsync(host.data(), folded, out_bytes, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    for (size_t i = 0; i < host.size(); ++i) out[i] = from_record(host[i]);
    return GS_OK;
}

} // extern "C"
