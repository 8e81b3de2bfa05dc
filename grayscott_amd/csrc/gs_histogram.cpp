// gs_histogram.cpp -- histograms of planes and ensemble members (include/gs_hip.h: gs_fields_histogram,
// gs_members_histogram).  The counters come from gs_plane_hist_k (gs_histogram.hip), one launch per slab on its compute
// stream into that slab's zeroed u64 counters; the slabs' counters -- and, in a multi-process context, every rank's
// (allgather_bytes) -- are added here on the host.  Integers: the order of the additions does not show.  An ensemble's
// members are counted in one launch and fetched with one copy.  Nothing here touches ghost rows, the tuner, graphs or the
// context's counters.
#include "gs_internal.h"

using namespace gsi;

namespace {

constexpr int kHistGroupsPerCu = 8; // workgroups of 4 waves a launch may put on a CU: 8 x (4096 + 4) u32 of LDS fit in 160 KiB

int32_t ensure_buffer(gs_ctx *ctx, int i, size_t bytes)
{
    SlabRt &sl = ctx->slabs[(size_t)i];
    if (sl.hist_bytes >= bytes) return GS_OK;
    GS_HIP(hipSetDevice(sl.device));
    if (sl.hist) GS_HIP(hipFree(sl.hist));
    sl.hist = nullptr;
    sl.hist_bytes = 0;
    const hipError_t e = hipMalloc(&sl.hist, bytes);
    if (e != hipSuccess) return fail(GS_ERR_NOMEM, "histogram buffer of %zu bytes: %s", bytes, hipGetErrorString(e));
    sl.hist_bytes = bytes;
    return GS_OK;
}

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

} // namespace

namespace gsi {

void destroy_histogram_buffers(gs_ctx *ctx)
{
    for (auto &sl : ctx->slabs) {
        if (!sl.hist) continue;
        if (hipSetDevice(sl.device) == hipSuccess) (void)hipFree(sl.hist);
        sl.hist = nullptr;
        sl.hist_bytes = 0;
    }
}

} // namespace gsi

extern "C" {

int32_t gs_fields_histogram(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *lo, const float *hi, int32_t bins,
                            uint64_t *out)
{
    if (!ctx || !fields || !lo || !hi || !out) return fail(GS_ERR_INVALID, "null argument");
    if (n < 1 || n > 4) return fail(GS_ERR_INVALID, "%d fields (1..4)", n);
    float scale[4];
    GS_TRY(check_ranges(lo, hi, n, bins, scale));
    for (int32_t p = 0; p < n; ++p) {
        if (!fields[p] || fields[p]->ctx != ctx) return fail(GS_ERR_INVALID, "field %d: null or of another context", p);
        if (p > 0) GS_TRY(same_shape(fields[0], fields[p]));
    }
    GS_TRY(sync_all(ctx)); // (also runs again a persistent window launch that gave up: no stale plane is read)
    const gs_field *f0 = fields[0];
    const size_t words = (size_t)n * (size_t)(bins + 3), bytes = words * sizeof(uint64_t);
    std::fill(out, out + words, (uint64_t)0);
    if (f0->rows == 0 || f0->cols == 0) return GS_OK; // the same shape on every rank: nobody exchanges anything
    const size_t nslab = ctx->slabs.size();
    std::vector<uint64_t> part(nslab * words);
    for (size_t i = 0; i < nslab; ++i) {
        SlabRt &sl = ctx->slabs[i];
        GS_TRY(ensure_buffer(ctx, (int)i, bytes));
        GS_HIP(hipSetDevice(sl.device));
        const float *planes[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int32_t p = 0; p < n; ++p) planes[p] = fields[p]->s[i].row0;
        unsigned long long *dev = static_cast<unsigned long long *>(sl.hist);
        GS_HIP(hipMemsetAsync(dev, 0, bytes, sl.compute));
        GS_HIP(gs_launch_histogram(planes, n, 1, 0, f0->pitch, (int64_t)f0->s[i].rows, (int32_t)f0->cols, lo, hi, scale, bins,
                                   max_groups(ctx), dev, sl.compute));
        GS_HIP(hipMemcpyAsync(part.data() + i * words, dev, bytes, hipMemcpyDeviceToHost, sl.compute));
    }
    for (auto &sl : ctx->slabs) {
        GS_HIP(hipSetDevice(sl.device));
        GS_HIP(hipStreamSynchronize(sl.compute));
    }
    for (size_t i = 0; i < nslab; ++i)
        for (size_t w = 0; w < words; ++w) out[w] += part[i * words + w];
    if (ctx->world == 1) return GS_OK;
    // Several processes: every rank's counters to every rank, added in the same way everywhere.
    const std::vector<size_t> sizes((size_t)ctx->world, bytes);
    const size_t total = bytes * (size_t)ctx->world;
    SlabRt &sl = ctx->slabs[0];
    GS_TRY(ensure_buffer(ctx, 0, bytes + total));
    GS_HIP(hipSetDevice(sl.device));
    unsigned char *send = static_cast<unsigned char *>(sl.hist), *recv = send + bytes;
    GS_HIP(hipMemcpyAsync(send, out, bytes, hipMemcpyHostToDevice, sl.compute));
    GS_TRY(allgather_bytes(ctx, send, recv, sizes, sl.compute));
    std::vector<uint64_t> all((size_t)ctx->world * words);
    GS_HIP(hipMemcpyAsync(all.data(), recv, total, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    std::fill(out, out + words, (uint64_t)0);
    for (int q = 0; q < ctx->world; ++q)
        for (size_t w = 0; w < words; ++w) out[w] += all[(size_t)q * words + w];
    return GS_OK;
}

int32_t gs_members_histogram(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float lo[2], const float hi[2],
                             int32_t bins, uint64_t *out)
{
    if (!ctx || !lo || !hi || !out) return fail(GS_ERR_INVALID, "null argument");
    float scale[2];
    GS_TRY(check_ranges(lo, hi, 2, bins, scale));
    if (!e) return fail(GS_ERR_INVALID, "null argument");
    if (e->ctx != ctx) return fail(GS_ERR_INVALID, "ensemble belongs to another context");
    if (count == 0 || first >= e->members || count > e->members - first)
        return fail(GS_ERR_INVALID, "members [%llu, %llu + %llu) outside the ensemble's %llu", (unsigned long long)first,
                    (unsigned long long)first, (unsigned long long)count, (unsigned long long)e->members);
    GS_TRY(sync_all(ctx));
    const uint64_t cells = e->rows * e->cols;
    const size_t words = (size_t)(2 * count) * (size_t)(bins + 3), bytes = words * sizeof(uint64_t);
    if (cells == 0) {
        std::fill(out, out + words, (uint64_t)0);
        return GS_OK;
    }
    GS_TRY(ensure_buffer(ctx, 0, bytes));
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    unsigned long long *dev = static_cast<unsigned long long *>(sl.hist);
    // member first + i's U and V are planes 2 i and 2 i + 1 of the launch: `cells` floats from one member to the next
    const float *planes[2] = {e->u[e->cur] + first * cells, e->v[e->cur] + first * cells};
    GS_HIP(hipMemsetAsync(dev, 0, bytes, sl.compute));
    GS_HIP(gs_launch_histogram(planes, 2, (int64_t)count, (int64_t)cells, (int64_t)e->cols, (int64_t)e->rows, (int32_t)e->cols,
                               lo, hi, scale, bins, max_groups(ctx), dev, sl.compute));
    GS_HIP(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    return GS_OK;
}

} // extern "C"
