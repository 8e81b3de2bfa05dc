// gs_attached.cpp -- a context's per-cell data on one grid (include/gs_hip.h), one kind at a time:
//   parameter maps (gs_ctx_set_param_map): feed and kill rates that vary from cell to cell.  The context owns two planes --
//     F, and F + K formed on the device in the context's float mode -- and the launchers run the map forms of the step
//     kernels (gs_*_mk) while they exist.
//   domain masks (gs_ctx_set_mask): wall cells that hold their values and block diffusion.  The context owns one plane, the
//     link plane: a u32 word per cell that says which of the cell's eight neighbours -- at the positions the boundary rule
//     reads -- are walls, and whether the cell itself is one (gs_cell.h: link_bit).  The words are formed on the device
//     once, at attach time, and the launchers run the mask forms of the step kernels (gs_*_wk) while the plane exists.
//   noise (gs_ctx_set_noise): a seeded stochastic increment per cell and step, a pure function of (seed, step, row, column).
//     The context owns no plane: the sigmas, the seed and the step counter live in gs_ctx::attached.noise, and the launchers
//     run the noise forms of the step kernels (gs_*_zk) with the step keys of each pass (noise_key).
// The first two are planes in the field layout of the species with refreshed ghost rows, kept in gs_ctx::attached; its kind
// selects the kernel set and, with it, the on-line tuner's state (gs_ctx::tuner): the uniform, the mapped, the masked and the
// noise kernels' choices are kept apart.
#include "gs_internal.h"

namespace gsi {

static const char *const kKindName[GS_ATTACH_KINDS] = {"", "parameter map", "domain mask", "noise term"}; // [GsAttached::kind]
static const char *const kKindShort[GS_ATTACH_KINDS] = {"", "map", "mask", "noise"};
static const char *const kKindForm[GS_ATTACH_KINDS] = {"", "parameter-map", "domain-mask", "noise"};

// Philox2x32-10 (include/gs_hip.h), the host's copy: the step keys.
static void philox2x32(uint32_t c0, uint32_t c1, uint32_t k, uint32_t out[2])
{
    for (int i = 0; i < 10; ++i) {
        const uint64_t p = (uint64_t)0xD256D193u * c0;
        c0 = (uint32_t)(p >> 32) ^ k ^ c1;
        c1 = (uint32_t)p;
        k += 0x9E3779B9u;
    }
    out[0] = c0;
    out[1] = c1;
}
uint32_t noise_key(uint64_t seed, uint64_t step)
{
    uint32_t x[2];
    philox2x32((uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, x);
    return x[0] ^ (uint32_t)(seed >> 32);
}

// The attached planes' shape against the species' (gs_step / gs_run).
int32_t check_attached_shape(const gs_ctx *ctx, const gs_field *f)
{
    if (ctx->attached.kind == GS_ATTACH_NONE || ctx->attached.kind == GS_ATTACH_NOISE) return GS_OK; // (the noise has no planes)
    const gs_field *m = ctx->attached.plane[0];
    if (m->rows != f->rows || m->cols != f->cols || m->pitch != f->pitch)
        return fail(GS_ERR_INVALID, "the %s is [%llu,%llu], the species are [%llu,%llu]", kKindName[ctx->attached.kind],
                    (unsigned long long)m->rows, (unsigned long long)m->cols, (unsigned long long)f->rows, (unsigned long long)f->cols);
    return GS_OK;
}

void destroy_attached(gs_ctx *ctx)
{
    for (gs_field *&p : ctx->attached.plane) {
        if (p) (void)gs_field_destroy(ctx, p);
        p = nullptr;
    }
    ctx->attached.kind = GS_ATTACH_NONE;
}

// What the `set` calls refuse before anything is touched: the other kind in force, a pinned kernel without a form for `kind`.
static int32_t refuse_attach(const gs_ctx *ctx, int kind)
{
    const int other = ctx->attached.kind;
    if (other != GS_ATTACH_NONE && other != kind)
        return fail(GS_ERR_UNSUPPORTED, "a %s and a %s cannot be attached together: detach the %s first", kKindName[kind], kKindName[other],
                    kKindShort[other]);
    const int32_t k = ctx->o.kernel;
    if (k == GS_KERNEL_WINDOW || k == GS_KERNEL_LDS || k == GS_KERNEL_TILE)
        return fail(GS_ERR_UNSUPPORTED, "the %s kernel has no %s form",
                    k == GS_KERNEL_WINDOW ? "persistent window" : (k == GS_KERNEL_LDS ? "LDS-staged single-step" : "LDS-window (tile)"),
                    kKindForm[kind]);
    return GS_OK;
}

// The `set` call of `kind` with null planes (a call for the kind that is not in force detaches nothing).
static int32_t detach(gs_ctx *ctx, int kind)
{
    if (ctx->attached.kind == kind) destroy_attached(ctx);
    ctx->attached.gen++;
    return GS_OK;
}

// The library's `np` planes of kind `kind`, of the shape of the caller's plane `like`: new ones for a new shape (what is in
// force stays if that fails).
static int32_t ensure_planes(gs_ctx *ctx, int kind, const gs_field *like, int np, const char *what)
{
    gs_ctx::Attached &at = ctx->attached;
    if (at.kind == kind && at.plane[0]->rows == like->rows && at.plane[0]->cols == like->cols && at.plane[0]->pitch == like->pitch)
        return GS_OK;
    gs_field *f[2] = {nullptr, nullptr};
    int32_t st = GS_OK;
    for (int j = 0; j < np && st == GS_OK; ++j) st = gs_field_create(ctx, &f[j], like->rows, like->cols);
    if (st == GS_OK && f[0]->pitch != like->pitch) // (one context, one shape: one pitch)
        st = fail(GS_ERR_INVALID, "%s of pitch %d, fields of pitch %d", what, f[0]->pitch, like->pitch);
    if (st != GS_OK) {
        for (gs_field *p : f)
            if (p) (void)gs_field_destroy(ctx, p);
        return st;
    }
    destroy_attached(ctx);
    at.kind = kind;
    at.plane[0] = f[0];
    at.plane[1] = f[1];
    return GS_OK;
}

// Fills the `np` planes of one shape: enqueue(i, sl, n) for every local slab i on its device -- n: the floats of a whole
// block of that slab, guards, ghost rows and padding included -- then a wait and the planes' ghost rows from the
// neighbouring slabs (the marching kernel computes cells in them; the caller's may be stale after an upload).
template <typename F>
static int32_t fill_planes(gs_ctx *ctx, gs_field *const *planes, int np, F enqueue)
{
    for (size_t i = 0; i < ctx->slabs.size(); ++i) {
        SlabRt &sl = ctx->slabs[i];
        GS_HIP(hipSetDevice(sl.device));
        GS_TRY(enqueue(i, sl, (size_t)(planes[0]->s[i].rows + 2 * kGhostRows) * planes[0]->pitch + 2 * kGuardFloats));
    }
    GS_TRY(sync_all(ctx));
    for (int j = 0; j < np; ++j) {
        planes[j]->ghost_depth = 0;
        GS_TRY(refresh_ghosts(ctx, planes[j])); // (collective in a multi-process run)
    }
    return GS_OK;
}

static int32_t copy_block(gs_field *dst, const gs_field *src, size_t i, SlabRt &sl, size_t n)
{
    GS_HIP(hipMemcpyAsync(dst->s[i].alloc, src->s[i].alloc, n * sizeof(float), hipMemcpyDeviceToDevice, sl.compute));
    return GS_OK;
}

// The link words of the context's link plane from the mask plane m (ghost rows up to date): whole blocks zeroed (guards,
// ghost rows and padding: no walls), then the words of the slabs' own cells.
static int32_t form_links(gs_ctx *ctx, gs_field *m)
{
    gs_field *l = ctx->attached.plane[0];
    const int32_t periodic = ctx->o.boundary == GS_BOUNDARY_PERIODIC;
    return fill_planes(ctx, &l, 1, [&](size_t i, SlabRt &sl, size_t n) -> int32_t {
        GS_HIP(hipMemsetAsync(l->s[i].alloc, 0, n * sizeof(float), sl.compute));
        const int g = ctx->global_index((int)i);
        const hipError_t e = gs_launch_mask_links(m->s[i].row0, reinterpret_cast<uint32_t *>(l->s[i].row0), l->pitch, l->s[i].rows,
                                                  (int32_t)l->cols, g > 0, g < ctx->total_slabs() - 1, periodic, sl.compute);
        if (e != hipSuccess) return fail(GS_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
        return GS_OK;
    });
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
        GS_TRY(refuse_attach(ctx, GS_ATTACH_MAP));
    }
    GS_TRY(sync_all(ctx)); // (also runs again what a window launch that gave up left undone, with the rates it was enqueued with)
    if (!feed) return detach(ctx, GS_ATTACH_MAP);
    GS_TRY(ensure_planes(ctx, GS_ATTACH_MAP, feed, 2, "parameter map planes"));
    // F as the caller's plane holds it, F + K one add per float
    gs_field *const *plane = ctx->attached.plane;
    GS_TRY(fill_planes(ctx, plane, 2, [&](size_t i, SlabRt &sl, size_t n) -> int32_t {
        GS_TRY(copy_block(plane[0], feed, i, sl, n));
        const hipError_t e = gs_launchers(ctx->o.math).map_rates(feed->s[i].alloc, kill->s[i].alloc, plane[1]->s[i].alloc, n, sl.compute);
        if (e != hipSuccess) return fail(GS_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
        return GS_OK;
    }));
    ctx->attached.gen++;
    return GS_OK;
}

int32_t gs_ctx_set_mask(gs_ctx *ctx, gs_field *mask)
{
    if (!ctx) return fail(GS_ERR_INVALID, "null context");
    if (mask) {
        if (mask->ctx != ctx) return fail(GS_ERR_INVALID, "field belongs to another context");
        GS_TRY(refuse_attach(ctx, GS_ATTACH_MASK));
    }
    GS_TRY(sync_all(ctx)); // (also runs again what a window launch that gave up left undone, without the mask)
    if (!mask) return detach(ctx, GS_ATTACH_MASK);
    // The library's copy of the mask, its ghost rows refreshed: the link words of a slab's edge rows need the neighbouring
    // slabs' rows.  It lives until the words are formed.
    gs_field *m = nullptr;
    GS_TRY(gs_field_create(ctx, &m, mask->rows, mask->cols));
    struct Drop { gs_ctx *c; gs_field *f; ~Drop() { (void)gs_field_destroy(c, f); } } drop{ctx, m};
    if (m->pitch != mask->pitch) // (one context, one shape: one pitch)
        return fail(GS_ERR_INVALID, "mask plane of pitch %d, fields of pitch %d", m->pitch, mask->pitch);
    GS_TRY(fill_planes(ctx, &m, 1, [&](size_t i, SlabRt &sl, size_t n) { return copy_block(m, mask, i, sl, n); }));
    GS_TRY(ensure_planes(ctx, GS_ATTACH_MASK, mask, 1, "link plane"));
    const int32_t st = form_links(ctx, m);
    if (st != GS_OK) destroy_attached(ctx); // a failure once the link plane exists leaves no mask attached
    ctx->attached.gen++;
    return st;
}

int32_t gs_ctx_set_noise(gs_ctx *ctx, const gs_noise *n)
{
    if (!ctx) return fail(GS_ERR_INVALID, "null context");
    if (n) {
        if (!std::isfinite(n->sigma_u) || !std::isfinite(n->sigma_v) || n->sigma_u < 0.0f || n->sigma_v < 0.0f)
            return fail(GS_ERR_INVALID, "the noise's sigmas must be finite and >= 0 (got %g, %g)", (double)n->sigma_u, (double)n->sigma_v);
        GS_TRY(refuse_attach(ctx, GS_ATTACH_NOISE));
        if (ctx->o.use_graph)
            return fail(GS_ERR_UNSUPPORTED, "noise cannot run with use_graph = 1: a replayed graph would replay its step keys");
    }
    GS_TRY(sync_all(ctx)); // (also runs again what a window launch that gave up left undone, without the noise)
    if (!n) return detach(ctx, GS_ATTACH_NOISE);
    ctx->attached.kind = GS_ATTACH_NOISE; // (nothing else is in force: refuse_attach; no planes to make)
    ctx->attached.noise = *n;
    ctx->attached.gen++;
    return GS_OK;
}

int32_t gs_ctx_get_noise(const gs_ctx *ctx, gs_noise *out, int32_t *attached)
{
    if (!ctx || !attached) return fail(GS_ERR_INVALID, "null argument");
    *attached = ctx->noisy() ? 1 : 0;
    if (ctx->noisy() && out) *out = ctx->attached.noise;
    return GS_OK;
}

} // extern "C"
