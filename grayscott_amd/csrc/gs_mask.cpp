// gs_mask.cpp -- domain masks (gs_ctx_set_mask in include/gs_hip.h): wall cells that hold their values and block
// diffusion on one grid.  The context owns one plane in the field layout of the species, the link plane: a u32 word per
// cell that says which of the cell's eight neighbours -- at the positions the boundary rule reads -- are walls, and
// whether the cell itself is one (gs_cell.h: link_bit).  The words are formed on the device once, at attach time, and
// the launchers run the mask forms of the step kernels (gs_*_wk) while the plane exists.  The on-line tuner keeps the
// masked kernels' choices apart from the uniform and the mapped kernels' (gs_param_map.cpp does the same for maps).
#include "gs_internal.h"

namespace gsi {

// The mask's shape against the species' (gs_step / gs_run).
int32_t check_mask_shape(const gs_ctx *ctx, const gs_field *f)
{
    if (!ctx->masked()) return GS_OK;
    const gs_field *m = ctx->mask.link;
    if (m->rows != f->rows || m->cols != f->cols || m->pitch != f->pitch)
        return fail(GS_ERR_INVALID, "the domain mask is [%llu,%llu], the species are [%llu,%llu]", (unsigned long long)m->rows,
                    (unsigned long long)m->cols, (unsigned long long)f->rows, (unsigned long long)f->cols);
    return GS_OK;
}

// The link words of the context's link plane from the mask plane m (ghost rows up to date), then the plane's ghost rows.
static int32_t form_links(gs_ctx *ctx, gs_field *m)
{
    gs_field *l = ctx->mask.link;
    const int32_t periodic = ctx->o.boundary == GS_BOUNDARY_PERIODIC;
    for (size_t i = 0; i < ctx->slabs.size(); ++i) {
        SlabRt &sl = ctx->slabs[i];
        GS_HIP(hipSetDevice(sl.device));
        const size_t n = (size_t)(l->s[i].rows + 2 * kGhostRows) * l->pitch + 2 * kGuardFloats;
        GS_HIP(hipMemsetAsync(l->s[i].alloc, 0, n * sizeof(float), sl.compute));
        const int g = ctx->global_index((int)i);
        const hipError_t e = gs_launch_mask_links(m->s[i].row0, reinterpret_cast<uint32_t *>(l->s[i].row0), l->pitch, l->s[i].rows,
                                                  (int32_t)l->cols, g > 0, g < ctx->total_slabs() - 1, periodic, sl.compute);
        if (e != hipSuccess) return fail(GS_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    }
    GS_TRY(sync_all(ctx));
    l->ghost_depth = 0;
    return refresh_ghosts(ctx, l); // (collective in a multi-process run)
}

void destroy_mask(gs_ctx *ctx)
{
    if (ctx->mask.link) (void)gs_field_destroy(ctx, ctx->mask.link);
    ctx->mask.link = nullptr;
}

} // namespace gsi

using namespace gsi;

extern "C" {

int32_t gs_ctx_set_mask(gs_ctx *ctx, gs_field *mask)
{
    if (!ctx) return fail(GS_ERR_INVALID, "null context");
    if (mask) {
        if (mask->ctx != ctx) return fail(GS_ERR_INVALID, "field belongs to another context");
        if (ctx->mapped())
            return fail(GS_ERR_UNSUPPORTED, "a domain mask and a parameter map cannot be attached together: detach the map first");
        const int32_t k = ctx->o.kernel;
        if (k == GS_KERNEL_WINDOW || k == GS_KERNEL_LDS || k == GS_KERNEL_TILE)
            return fail(GS_ERR_UNSUPPORTED, "the %s kernel has no domain-mask form",
                        k == GS_KERNEL_WINDOW ? "persistent window" : (k == GS_KERNEL_LDS ? "LDS-staged single-step" : "LDS-window (tile)"));
    }
    GS_TRY(sync_all(ctx)); // (also runs again what a window launch that gave up left undone, without the mask)
    const bool was = ctx->masked();
    if (!mask) {
        destroy_mask(ctx);
        if (was) swap_tuner_sets(ctx, ctx->mask);
        ctx->mask.gen++;
        return GS_OK;
    }
    // The library's copy of the mask, its ghost rows refreshed (the caller's may be stale after an upload): the link words
    // of a slab's edge rows need the neighbouring slabs' rows.  It lives until the words are formed.
    gs_field *m = nullptr;
    GS_TRY(gs_field_create(ctx, &m, mask->rows, mask->cols));
    struct Drop { gs_ctx *c; gs_field *f; ~Drop() { (void)gs_field_destroy(c, f); } } drop{ctx, m};
    if (m->pitch != mask->pitch) // (one context, one shape: one pitch)
        return fail(GS_ERR_INVALID, "mask plane of pitch %d, fields of pitch %d", m->pitch, mask->pitch);
    for (size_t i = 0; i < ctx->slabs.size(); ++i) {
        SlabRt &sl = ctx->slabs[i];
        GS_HIP(hipSetDevice(sl.device));
        const size_t n = (size_t)(mask->s[i].rows + 2 * kGhostRows) * mask->pitch + 2 * kGuardFloats;
        GS_HIP(hipMemcpyAsync(m->s[i].alloc, mask->s[i].alloc, n * sizeof(float), hipMemcpyDeviceToDevice, sl.compute));
    }
    GS_TRY(sync_all(ctx));
    m->ghost_depth = 0;
    GS_TRY(refresh_ghosts(ctx, m)); // (collective in a multi-process run)
    // the link plane, of the caller's shape: a new one for a new shape (the mask in force stays if that fails)
    if (!(was && ctx->mask.link->rows == mask->rows && ctx->mask.link->cols == mask->cols && ctx->mask.link->pitch == mask->pitch)) {
        gs_field *l = nullptr;
        GS_TRY(gs_field_create(ctx, &l, mask->rows, mask->cols));
        destroy_mask(ctx);
        ctx->mask.link = l;
    }
    // Whole blocks zeroed (guards, ghost rows and padding: no walls), then the words of the slabs' own cells; then the
    // ghost rows from the neighbouring slabs -- the marching kernel computes cells in them.  A failure from here on leaves
    // no mask attached.
    const int32_t st = form_links(ctx, m);
    if (st != GS_OK) {
        destroy_mask(ctx);
        if (was) swap_tuner_sets(ctx, ctx->mask);
        ctx->mask.gen++;
        return st;
    }
    if (!was) swap_tuner_sets(ctx, ctx->mask);
    ctx->mask.gen++;
    return GS_OK;
}

} // extern "C"
