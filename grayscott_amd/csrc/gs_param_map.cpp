// gs_param_map.cpp -- parameter maps (gs_ctx_set_param_map in include/gs_hip.h): feed and kill rates that vary from cell to
// cell on one grid.  The context owns two planes in the field layout of the species -- F, and F + K formed on the device
// in the context's float mode -- and the launchers run the map forms of the step kernels (gs_*_mk) while they exist.
// The on-line tuner keeps one set of choices per kernel set: attaching or detaching a map exchanges them.
#include "gs_internal.h"

namespace gsi {

// The map's shape against the species' (gs_step / gs_run).
int32_t check_map_shape(const gs_ctx *ctx, const gs_field *f)
{
    if (!ctx->mapped()) return GS_OK;
    const gs_field *m = ctx->map.feed;
    if (m->rows != f->rows || m->cols != f->cols || m->pitch != f->pitch)
        return fail(GS_ERR_INVALID, "the parameter map is [%llu,%llu], the species are [%llu,%llu]", (unsigned long long)m->rows,
                    (unsigned long long)m->cols, (unsigned long long)f->rows, (unsigned long long)f->cols);
    return GS_OK;
}

void destroy_param_map(gs_ctx *ctx)
{
    if (ctx->map.feed) (void)gs_field_destroy(ctx, ctx->map.feed);
    if (ctx->map.fpk) (void)gs_field_destroy(ctx, ctx->map.fpk);
    ctx->map.feed = ctx->map.fpk = nullptr;
}

} // namespace gsi

using namespace gsi;

extern "C" {

int32_t gs_ctx_set_param_map(gs_ctx *ctx, gs_field *feed, gs_field *kill)
{
    if (!ctx) return fail(GS_ERR_INVALID, "null context");
    if (!feed != !kill) return fail(GS_ERR_INVALID, "a parameter map needs both planes (or neither, to detach it)");
    if (feed) {
        if (feed->ctx != ctx || kill->ctx != ctx) return fail(GS_ERR_INVALID, "field belongs to another context");
        GS_TRY(same_shape(feed, kill));
        if (feed == kill) return fail(GS_ERR_INVALID, "the feed and kill planes must be distinct fields");
        if (ctx->masked())
            return fail(GS_ERR_UNSUPPORTED, "a parameter map and a domain mask cannot be attached together: detach the mask first");
        const int32_t k = ctx->o.kernel;
        if (k == GS_KERNEL_WINDOW || k == GS_KERNEL_LDS || k == GS_KERNEL_TILE)
            return fail(GS_ERR_UNSUPPORTED, "the %s kernel has no parameter-map form",
                        k == GS_KERNEL_WINDOW ? "persistent window" : (k == GS_KERNEL_LDS ? "LDS-staged single-step" : "LDS-window (tile)"));
    }
    GS_TRY(sync_all(ctx)); // (also runs again what a window launch that gave up left undone, with the rates it was enqueued with)
    const bool was = ctx->mapped();
    if (!feed) {
        destroy_param_map(ctx);
        if (was) swap_tuner_sets(ctx, ctx->map);
        ctx->map.gen++;
        return GS_OK;
    }
    // the library's planes, of the caller's shape: new ones for a new shape (the map in force stays if that fails)
    if (!(was && ctx->map.feed->rows == feed->rows && ctx->map.feed->cols == feed->cols && ctx->map.feed->pitch == feed->pitch)) {
        gs_field *f = nullptr, *g = nullptr;
        GS_TRY(gs_field_create(ctx, &f, feed->rows, feed->cols));
        const int32_t st = gs_field_create(ctx, &g, feed->rows, feed->cols);
        if (st != GS_OK) { (void)gs_field_destroy(ctx, f); return st; }
        if (f->pitch != feed->pitch) { // (one context, one shape: one pitch)
            (void)gs_field_destroy(ctx, f); (void)gs_field_destroy(ctx, g);
            return fail(GS_ERR_INVALID, "parameter map planes of pitch %d, fields of pitch %d", f->pitch, feed->pitch);
        }
        destroy_param_map(ctx);
        ctx->map.feed = f;
        ctx->map.fpk = g;
    }
    // Whole blocks, guards, ghost rows and padding included: F as the caller's plane holds it, F + K one add per float;
    // then the ghost rows from the neighbouring slabs (the caller's may be stale after an upload).
    const bool fused = ctx->o.math == GS_MATH_FUSED;
    for (size_t i = 0; i < ctx->slabs.size(); ++i) {
        SlabRt &sl = ctx->slabs[i];
        GS_HIP(hipSetDevice(sl.device));
        const size_t n = (size_t)(feed->s[i].rows + 2 * kGhostRows) * feed->pitch + 2 * kGuardFloats;
        GS_HIP(hipMemcpyAsync(ctx->map.feed->s[i].alloc, feed->s[i].alloc, n * sizeof(float), hipMemcpyDeviceToDevice, sl.compute));
        const hipError_t e = fused ? gs_launch_map_rates_fused(feed->s[i].alloc, kill->s[i].alloc, ctx->map.fpk->s[i].alloc, n, sl.compute)
                                   : gs_launch_map_rates_strict(feed->s[i].alloc, kill->s[i].alloc, ctx->map.fpk->s[i].alloc, n, sl.compute);
        if (e != hipSuccess) return fail(GS_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    }
    GS_TRY(sync_all(ctx));
    ctx->map.feed->ghost_depth = 0;
    ctx->map.fpk->ghost_depth = 0;
    GS_TRY(refresh_ghosts(ctx, ctx->map.feed)); // (collective in a multi-process run)
    GS_TRY(refresh_ghosts(ctx, ctx->map.fpk));
    if (!was) swap_tuner_sets(ctx, ctx->map);
    ctx->map.gen++;
    return GS_OK;
}

} // extern "C"
