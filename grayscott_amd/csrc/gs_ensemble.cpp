// gs_ensemble.cpp -- ensembles (include/gs_hip.h): `members` independent grids of one shape, each with its own parameters,
// advanced in shared launches of the kernels of gs_ensemble.h.  The planes are dense [members, rows, cols] (pitch = cols,
// no ghost rows: an ensemble lives on one slab), two slots per species; the ensemble tracks which slot is current.
// Everything is enqueued on the context's compute stream, so gs_sync and the blocking calls see it in order.
#include "gs_internal.h"

using namespace gsi;

int32_t gsi::check_member_range(const gs_ensemble *e, uint64_t first, uint64_t count)
{
    if (count == 0 || first >= e->members || count > e->members - first)
        return fail(GS_ERR_INVALID, "members [%llu, %llu + %llu) outside the ensemble's %llu", (unsigned long long)first,
                    (unsigned long long)first, (unsigned long long)count, (unsigned long long)e->members);
    return GS_OK;
}

namespace {

// A member's cells are indexed with 32-bit integers in the kernels (and its windows must fit one launch).
constexpr uint64_t kMaxMemberCells = 1ull << 28;

int32_t check_ensemble(const gs_ctx *ctx, const gs_ensemble *e)
{
    if (!ctx || !e) return fail(GS_ERR_INVALID, "null argument");
    if (e->ctx != ctx) return fail(GS_ERR_INVALID, "ensemble belongs to another context");
    return GS_OK;
}

void free_planes(gs_ensemble *e)
{
    for (int s = 0; s < 2; ++s) {
        if (e->u[s]) (void)hipFree(e->u[s]);
        if (e->v[s]) (void)hipFree(e->v[s]);
        e->u[s] = e->v[s] = nullptr;
    }
    if (e->params) (void)hipFree(e->params);
    e->params = nullptr;
}

GsEnsParams to_device(const gs_params &p)
{
    GsEnsParams q{};
    std::memcpy(q.w, p.w, sizeof q.w);
    q.du = p.du;
    q.dv = p.dv;
    q.feed = p.feed;
    q.feed_plus_kill = p.feed + p.kill; // the reference's f32 add (compute/naive/src/lib.rs:77), as make_args forms it
    q.dt = p.dt;
    return q;
}

// The .op specialisation (side weights 0.5, dt == 1: gs_tuner.cpp's fast_of) only when every member qualifies.
int fast_of_all(const gs_ctx *ctx, const gs_params *p, uint64_t n)
{
    if (ctx->o.general_kernels || ctx->o.math == GS_MATH_FUSED) return 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float(*w)[3] = p[i].w;
        if (!(w[0][1] == 0.5f && w[1][0] == 0.5f && w[1][2] == 0.5f && w[2][1] == 0.5f && p[i].dt == 1.0f)) return 0;
    }
    return 3;
}

} // namespace

extern "C" {

int32_t gs_ensemble_create(gs_ctx *ctx, gs_ensemble **out, uint64_t members, uint64_t rows, uint64_t cols)
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (ctx->slabs.size() != 1 || ctx->world != 1)
        return fail(GS_ERR_UNSUPPORTED, "an ensemble lives on a context of one slab in one process (%d slabs x %d processes)",
                    (int)ctx->slabs.size(), ctx->world);
    if (members == 0 || rows == 0 || cols == 0)
        return fail(GS_ERR_INVALID, "empty ensemble (%llu members of %llu x %llu)", (unsigned long long)members,
                    (unsigned long long)rows, (unsigned long long)cols);
    if (rows > kMaxMemberCells || cols > kMaxMemberCells || rows * cols > kMaxMemberCells)
        return fail(GS_ERR_UNSUPPORTED, "members of more than 2^28 cells: run them as Species");
    const uint64_t cells = rows * cols;
    if (members > (~0ull / 4) / cells) return fail(GS_ERR_INVALID, "ensemble too large");
    gs_ensemble *e = new (std::nothrow) gs_ensemble();
    if (!e) return fail(GS_ERR_NOMEM, "out of host memory");
    e->ctx = ctx;
    e->members = members;
    e->rows = rows;
    e->cols = cols;
    const size_t bytes = (size_t)(members * cells) * sizeof(float);
    SlabRt &sl = ctx->slabs[0];
    hipError_t err = hipSetDevice(sl.device);
    for (int s = 0; s < 2 && err == hipSuccess; ++s) {
        err = hipMalloc(reinterpret_cast<void **>(&e->u[s]), bytes);
        if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void **>(&e->v[s]), bytes);
        if (err == hipSuccess) err = hipMemsetAsync(e->u[s], 0, bytes, sl.compute);
        if (err == hipSuccess) err = hipMemsetAsync(e->v[s], 0, bytes, sl.compute);
    }
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void **>(&e->params), (size_t)members * sizeof(GsEnsParams));
    if (err == hipSuccess) {
        const std::vector<GsEnsParams> table((size_t)members, to_device(ctx->p));
        err = hipMemcpy(e->params, table.data(), table.size() * sizeof(GsEnsParams), hipMemcpyHostToDevice);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(sl.compute);
    if (err != hipSuccess) {
        free_planes(e);
        delete e;
        return fail(err == hipErrorOutOfMemory ? GS_ERR_NOMEM : GS_ERR_HIP, "ensemble allocation failed: %s", hipGetErrorString(err));
    }
    e->fast = fast_of_all(ctx, &ctx->p, 1);
    *out = e;
    return GS_OK;
}

int32_t gs_ensemble_destroy(gs_ctx *ctx, gs_ensemble *e)
{
    if (!e) return GS_OK;
    if (!ctx || e->ctx != ctx) return fail(GS_ERR_INVALID, "ensemble destroyed with another context");
    (void)hipSetDevice(ctx->slabs[0].device);
    (void)hipStreamSynchronize(ctx->slabs[0].compute); // no launch may still use the planes
    free_planes(e);
    delete e;
    return GS_OK;
}

int32_t gs_ensemble_shape(const gs_ensemble *e, uint64_t *members, uint64_t *rows, uint64_t *cols)
{
    if (!e) return fail(GS_ERR_INVALID, "null ensemble");
    if (members) *members = e->members;
    if (rows) *rows = e->rows;
    if (cols) *cols = e->cols;
    return GS_OK;
}

int32_t gs_ensemble_set_params(gs_ctx *ctx, gs_ensemble *e, const gs_params *params, uint64_t count)
{
    GS_TRY(check_ensemble(ctx, e));
    if (!params) return fail(GS_ERR_INVALID, "null parameters");
    if (count != 1 && count != e->members)
        return fail(GS_ERR_INVALID, "%llu parameter sets for %llu members (1 or one per member)", (unsigned long long)count,
                    (unsigned long long)e->members);
    for (uint64_t i = 0; i < count; ++i) GS_TRY(check_math(params[i], ctx->o.math));
    std::vector<GsEnsParams> table((size_t)e->members);
    for (uint64_t i = 0; i < e->members; ++i) table[i] = to_device(params[count == 1 ? 0 : i]);
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GS_HIP(hipStreamSynchronize(sl.compute)); // launches in flight read the table
    GS_HIP(hipMemcpy(e->params, table.data(), table.size() * sizeof(GsEnsParams), hipMemcpyHostToDevice));
    e->fast = fast_of_all(ctx, params, count);
    return GS_OK;
}

int32_t gs_ensemble_seed(gs_ctx *ctx, gs_ensemble *e)
{
    GS_TRY(check_ensemble(ctx, e));
    // Species::new (data/src/concentration/mod.rs:36-59): rows [7/16 rows - 4, 8/16 rows - 4), columns [7/16, 8/16)
    const long rows = (long)e->rows, cols = (long)e->cols;
    const long r0 = std::max(rows * 7 / 16 - 4, 0L), r1 = std::max(rows * 8 / 16 - 4, 0L);
    const long c0 = cols * 7 / 16, c1 = cols * 8 / 16;
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GS_HIP(gs_launch_ens_seed(e->u[e->cur], e->v[e->cur], e->members, (int32_t)rows, (int32_t)cols, (int32_t)r0, (int32_t)r1,
                              (int32_t)c0, (int32_t)c1, sl.compute));
    return GS_OK;
}

int32_t gs_ensemble_upload(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float *u, const float *v)
{
    GS_TRY(check_ensemble(ctx, e));
    if (!u && !v) return fail(GS_ERR_INVALID, "null host arrays");
    GS_TRY(check_member_range(e, first, count));
    const size_t cells = (size_t)(e->rows * e->cols), off = (size_t)first * cells, bytes = (size_t)count * cells * sizeof(float);
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    if (u) GS_HIP(hipMemcpyAsync(e->u[e->cur] + off, u, bytes, hipMemcpyHostToDevice, sl.compute));
    if (v) GS_HIP(hipMemcpyAsync(e->v[e->cur] + off, v, bytes, hipMemcpyHostToDevice, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    return GS_OK;
}

int32_t gs_ensemble_download(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, int32_t species, float *host)
{
    GS_TRY(check_ensemble(ctx, e));
    if (!host) return fail(GS_ERR_INVALID, "null host array");
    if (species != 0 && species != 1) return fail(GS_ERR_INVALID, "species %d (0 = U, 1 = V)", species);
    GS_TRY(check_member_range(e, first, count));
    const size_t cells = (size_t)(e->rows * e->cols), off = (size_t)first * cells, bytes = (size_t)count * cells * sizeof(float);
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    const float *src = (species == 0 ? e->u[e->cur] : e->v[e->cur]) + off;
    GS_HIP(hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, sl.compute));
    GS_HIP(hipStreamSynchronize(sl.compute));
    return GS_OK;
}

int32_t gs_ensemble_run(gs_ctx *ctx, gs_ensemble *e, uint64_t steps)
{
    GS_TRY(check_ensemble(ctx, e));
    if (steps == 0) return GS_OK;
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    const bool fused = ctx->o.math == GS_MATH_FUSED;
    GsEnsArgs a;
    std::memset(&a, 0, sizeof a);
    a.params = e->params;
    a.first = 0;
    a.members = (int32_t)std::min<uint64_t>(e->members, 0x7fffffff);
    a.rows = (int32_t)e->rows;
    a.cols = (int32_t)e->cols;
    a.zero_halo = ctx->o.boundary; // gs_boundary: 0, 1, 2 or 3 (gs_ctx_create admits no other value)
    // The launchers split at kGsEnsMaxGroups workgroups; a `members` above 2^31 goes in slices here.
    auto for_slices = [&](auto &&launch) -> int32_t {
        for (uint64_t m0 = 0; m0 < e->members; m0 += 0x40000000ull) {
            GsEnsArgs s = a;
            s.first = (int64_t)m0;
            s.members = (int32_t)std::min<uint64_t>(e->members - m0, 0x40000000ull);
            const hipError_t err = launch(s);
            if (err != hipSuccess) return fail(GS_ERR_HIP, "ensemble kernel launch failed: %s", hipGetErrorString(err));
        }
        return GS_OK;
    };
    // Resident form: the whole call in one launch per member, while the member fits one workgroup's LDS and registers.
    // A member of more than kGsResidentCells cells is only kept on one CU when the members fill the chip; with fewer of
    // them the windows of the tile form spread each member over several CUs (gs_run's reason for its 1536-cell cap).
    const int cpt = gs_ens_resident_cpt((long)e->rows, (long)e->cols, a.zero_halo);
    const uint64_t cells = e->rows * e->cols;
    const uint64_t cus = ctx->cu_count > 0 ? (uint64_t)ctx->cu_count : 256;
    if (cpt && (cells <= (uint64_t)kGsResidentCells || e->members >= cus)) {
        uint64_t left = steps;
        while (left > 0) { // the step count is an int in the kernel
            const int n = left > 0x40000000ull ? 0x40000000 : (int)left;
            const char *name = nullptr;
            a.in_u = e->u[e->cur];
            a.in_v = e->v[e->cur];
            a.out_u = e->u[e->cur ^ 1];
            a.out_v = e->v[e->cur ^ 1];
            GS_TRY(for_slices([&](const GsEnsArgs &s) {
                return fused ? gs_launch_ens_resident_fused(s, n, e->fast, sl.compute, &name)
                             : gs_launch_ens_resident_strict(s, n, e->fast, sl.compute, &name);
            }));
            ctx->last_kernel = name;
            ctx->launches++;
            e->cur ^= n & 1;
            left -= (uint64_t)n;
        }
        return GS_OK;
    }
    // Windowed form: window shape and steps per launch from gs_run's cost model, counting the workgroups of every member.
    int shape = 0, kmax = 8;
    pick_tile_config((long)e->rows, (long)e->cols, &shape, &kmax, (long)e->members);
    uint64_t left = steps;
    const char *full_name = nullptr;
    while (left > 0) { // the short launch first, then full ones
        const int n = left % (uint64_t)kmax ? (int)(left % (uint64_t)kmax) : kmax;
        const char *name = nullptr;
        a.in_u = e->u[e->cur];
        a.in_v = e->v[e->cur];
        a.out_u = e->u[e->cur ^ 1];
        a.out_v = e->v[e->cur ^ 1];
        GS_TRY(for_slices([&](const GsEnsArgs &s) {
            return fused ? gs_launch_ens_tile_fused(s, n, shape, e->fast, sl.compute, &name)
                         : gs_launch_ens_tile_strict(s, n, shape, e->fast, sl.compute, &name);
        }));
        if (!full_name || n == kmax) full_name = name;
        ctx->launches++;
        e->cur ^= 1;
        left -= (uint64_t)n;
    }
    ctx->last_kernel = full_name;
    return GS_OK;
}

} // extern "C"
