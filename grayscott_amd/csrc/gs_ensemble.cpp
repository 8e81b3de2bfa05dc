// gs_ensemble.cpp -- ensembles (include/gs_hip.h): `members` independent grids of one shape, each with its own parameters,
// advanced in shared launches of the kernels of gs_ensemble.h.  The planes are dense [members, rows, cols] (pitch = cols,
// no ghost rows: an ensemble lives on one slab), two slots per species; the ensemble tracks which slot is current.
// Everything is enqueued on the context's compute stream, so gs_sync and the blocking calls see it in order.
// Active sets (gs_members_set_active): gs_ensemble_run advances the active members only, through the listed forms of the
// kernels and a device list of their indices.  `cur` flips for the whole ensemble, so an inactive member must read the same
// through either slot: before its first launch a run copies every inactive member whose newest slot has changed since the
// last run (retired, or written while inactive) into the other slot, in one launch of gs_members_mirror_k.
// Noise (gs_members_set_noise): a second device table, one GsEnsNoise per member, and the noise forms of the two kernels
// (gs_ens_resident_z*, gs_ens_tile_z*), which take the table, the nullable list of active members and the ensemble's
// run_steps; a member's step index is run_steps plus its offset in the table (gs_internal.h: gs_ensemble::noise).
#include "gs_internal.h"

using namespace gsi;

int32_t gsi::check_member_range(const gs_ensemble *e, uint64_t first, uint64_t count)
{
    if (count == 0 || first >= e->members || count > e->members - first)
        return fail(GS_ERR_INVALID, "members [%llu, %llu + %llu) outside the ensemble's %llu", (unsigned long long)first,
                    (unsigned long long)first, (unsigned long long)count, (unsigned long long)e->members);
    return GS_OK;
}

void gsi::mark_members_written(gs_ensemble *e, uint64_t first, uint64_t count)
{
    if (e->all_active()) return;
    for (uint64_t i = first; i < first + count; ++i)
        if (!e->active[i] && !e->stale[i]) {
            e->stale[i] = 1;
            e->stale_count++;
        }
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
    if (e->active_list) (void)hipFree(e->active_list);
    if (e->mirror_list) (void)hipFree(e->mirror_list);
    if (e->noise_table) (void)hipFree(e->noise_table);
    e->params = nullptr;
    e->active_list = e->mirror_list = nullptr;
    e->noise_table = nullptr;
}

uint64_t noise_offset(const GsEnsNoise &n) { return (uint64_t)n.offset_hi << 32 | n.offset_lo; }
void set_noise_offset(GsEnsNoise &n, uint64_t offset)
{
    n.offset_lo = (uint32_t)offset;
    n.offset_hi = (uint32_t)(offset >> 32);
}

// What a run does first when members are inactive: slot cur of every stale member into slot cur ^ 1, in one launch behind
// the enqueued work.  (The list travels from the host: the call waits for the stream first, because an earlier mirror
// launch may still read the buffer.)
int32_t mirror_stale(gs_ensemble *e, SlabRt &sl)
{
    if (e->stale_count == 0) return GS_OK;
    std::vector<uint32_t> list;
    list.reserve((size_t)e->stale_count);
    for (uint64_t i = 0; i < e->members; ++i)
        if (e->stale[i]) list.push_back((uint32_t)i);
    GS_HIP(hipStreamSynchronize(sl.compute));
    GS_HIP(hipMemcpy(e->mirror_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    GS_HIP(gs_launch_members_mirror(e->mirror_list, list.size(), e->u[e->cur], e->v[e->cur], e->u[e->cur ^ 1], e->v[e->cur ^ 1],
                                    e->rows * e->cols, sl.compute));
    for (uint32_t i : list) e->stale[i] = 0;
    e->stale_count = 0;
    return GS_OK;
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
    mark_members_written(e, 0, e->members);
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
    mark_members_written(e, first, count);
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
    const GsLaunchers &launch = gs_launchers(ctx->o.math);
    GsEnsArgs a;
    std::memset(&a, 0, sizeof a);
    a.params = e->params;
    a.first = 0;
    a.members = (int32_t)std::min<uint64_t>(e->members, 0x7fffffff);
    a.rows = (int32_t)e->rows;
    a.cols = (int32_t)e->cols;
    a.zero_halo = ctx->o.boundary; // gs_boundary: 0, 1, 2 or 3 (gs_ctx_create admits no other value)
    // With an active set: the members that run, through the launchers' listed forms and the list of their indices (GsEnsArgs::first
    // is then a position in the list); with every member active, today's launchers exactly.
    const bool listed = !e->all_active();
    const uint64_t running = listed ? e->active_count : e->members;
    if (running == 0) return GS_OK; // nobody advances: no launch, no flip
    if (listed) GS_TRY(mirror_stale(e, sl));
    const uint32_t *list = listed ? e->active_list : nullptr; // (allocated before a member can be inactive)
    // With noise attached: the noise forms, one per kernel whether or not a list is in use (GsEnsNoiseArgs::list).
    const bool noisy = !e->noise.empty();
    GsEnsNoiseArgs z{e->noise_table, list, 0};
    // The launchers split at kGsEnsMaxGroups workgroups; a `members` above 2^31 goes in slices here.
    auto for_slices = [&](auto &&launch_slice) -> int32_t {
        for (uint64_t m0 = 0; m0 < running; m0 += 0x40000000ull) {
            GsEnsArgs s = a;
            s.first = (int64_t)m0;
            s.members = (int32_t)std::min<uint64_t>(running - m0, 0x40000000ull);
            const hipError_t err = launch_slice(s);
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
    if (cpt && (cells <= (uint64_t)kGsResidentCells || running >= cus)) {
        uint64_t left = steps;
        while (left > 0) { // the step count is an int in the kernel
            const int n = left > 0x40000000ull ? 0x40000000 : (int)left;
            const char *name = nullptr;
            a.in_u = e->u[e->cur];
            a.in_v = e->v[e->cur];
            a.out_u = e->u[e->cur ^ 1];
            a.out_v = e->v[e->cur ^ 1];
            z.step0 = e->run_steps;
            GS_TRY(for_slices([&](const GsEnsArgs &s) {
                return noisy ? launch.ens_resident_noise(s, z, n, e->fast, sl.compute, &name)
                             : launch.ens_resident(s, list, n, e->fast, sl.compute, &name);
            }));
            ctx->last_kernel = name;
            ctx->launches++;
            e->cur ^= n & 1;
            e->run_steps += (uint64_t)n;
            left -= (uint64_t)n;
        }
        return GS_OK;
    }
    // Windowed form: window shape and steps per launch from gs_run's cost model, counting the workgroups of every member.
    int shape = 0, kmax = 8;
    pick_tile_config((long)e->rows, (long)e->cols, &shape, &kmax, (long)running);
    uint64_t left = steps;
    const char *full_name = nullptr;
    while (left > 0) { // the short launch first, then full ones
        const int n = left % (uint64_t)kmax ? (int)(left % (uint64_t)kmax) : kmax;
        const char *name = nullptr;
        a.in_u = e->u[e->cur];
        a.in_v = e->v[e->cur];
        a.out_u = e->u[e->cur ^ 1];
        a.out_v = e->v[e->cur ^ 1];
        z.step0 = e->run_steps;
        GS_TRY(for_slices([&](const GsEnsArgs &s) {
            return noisy ? launch.ens_tile_noise(s, z, n, shape, e->fast, sl.compute, &name)
                         : launch.ens_tile(s, list, n, shape, e->fast, sl.compute, &name);
        }));
        if (!full_name || n == kmax) full_name = name;
        ctx->launches++;
        e->cur ^= 1;
        e->run_steps += (uint64_t)n;
        left -= (uint64_t)n;
    }
    ctx->last_kernel = full_name;
    return GS_OK;
}

int32_t gs_members_set_active(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const uint8_t *active)
{
    GS_TRY(check_ensemble(ctx, e));
    if (!active) return fail(GS_ERR_INVALID, "null active flags");
    GS_TRY(check_member_range(e, first, count));
    if (e->members > 0x80000000ull)
        return fail(GS_ERR_UNSUPPORTED, "an active set on more than 2^31 members (the list of active members holds 32-bit indices)");
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GS_HIP(hipStreamSynchronize(sl.compute)); // launches in flight read the list
    std::vector<uint32_t> list;
    try {
        list.reserve((size_t)e->members);
        if (e->active.empty()) { // the first call: every member active so far (`active` last: the ensemble is as before if one throws)
            e->missed.assign((size_t)e->members, 0);
            e->retired_at.assign((size_t)e->members, 0);
            e->stale.assign((size_t)e->members, 0);
            e->active.assign((size_t)e->members, 1);
            e->active_count = e->members;
        }
    } catch (const std::bad_alloc &) {
        return fail(GS_ERR_NOMEM, "out of host memory");
    }
    for (int b = 0; b < 2; ++b) {
        uint32_t *&buf = b ? e->mirror_list : e->active_list;
        if (buf) continue;
        const hipError_t err = hipMalloc(reinterpret_cast<void **>(&buf), (size_t)e->members * sizeof(uint32_t));
        if (err != hipSuccess) {
            buf = nullptr;
            return fail(err == hipErrorOutOfMemory ? GS_ERR_NOMEM : GS_ERR_HIP, "active list allocation failed: %s", hipGetErrorString(err));
        }
    }
    bool noise_moved = false;
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t m = first + i;
        const uint8_t want = active[i] ? 1 : 0;
        if (want == e->active[m]) continue;
        e->active[m] = want;
        if (want) { // reactivated: its newest slot is valid as it is; the steps it sat out are settled
            e->active_count++;
            e->missed[m] += e->run_steps - e->retired_at[m];
            if (!e->noise.empty()) { // ... and its noise goes on from the step it stopped at
                set_noise_offset(e->noise[m], noise_offset(e->noise[m]) - (e->run_steps - e->retired_at[m]));
                noise_moved = true;
            }
            e->stale_count -= e->stale[m];
            e->stale[m] = 0;
        } else { // retired: the other slot holds an older state (or none) until the next run mirrors it
            e->active_count--;
            e->retired_at[m] = e->run_steps;
            e->stale[m] = 1;
            e->stale_count++;
        }
    }
    for (uint64_t i = 0; i < e->members; ++i)
        if (e->active[i]) list.push_back((uint32_t)i);
    if (!list.empty()) GS_HIP(hipMemcpy(e->active_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (noise_moved) GS_HIP(hipMemcpy(e->noise_table, e->noise.data(), e->noise.size() * sizeof(GsEnsNoise), hipMemcpyHostToDevice));
    return GS_OK;
}

int32_t gs_members_get_active(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, uint8_t *active, uint64_t *steps_taken,
                              uint64_t *active_total)
{
    GS_TRY(check_ensemble(ctx, e));
    if (!active && !steps_taken && !active_total) return fail(GS_ERR_INVALID, "null outputs");
    GS_TRY(check_member_range(e, first, count));
    const bool untouched = e->active.empty();
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t m = first + i;
        const bool on = untouched || e->active[m];
        if (active) active[i] = on ? 1 : 0;
        if (steps_taken)
            steps_taken[i] = untouched ? e->run_steps : e->run_steps - e->missed[m] - (on ? 0 : e->run_steps - e->retired_at[m]);
    }
    if (active_total) *active_total = untouched ? e->members : e->active_count;
    return GS_OK;
}

int32_t gs_members_set_noise(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const gs_noise *noise, uint64_t entries)
{
    GS_TRY(check_ensemble(ctx, e));
    if (!noise) return fail(GS_ERR_INVALID, "null noise");
    GS_TRY(check_member_range(e, first, count));
    if (entries != 1 && entries != count)
        return fail(GS_ERR_INVALID, "%llu noise structs for %llu members (1 or one per member)", (unsigned long long)entries,
                    (unsigned long long)count);
    for (uint64_t i = 0; i < entries; ++i)
        if (!(std::isfinite(noise[i].sigma_u) && std::isfinite(noise[i].sigma_v) && noise[i].sigma_u >= 0.0f && noise[i].sigma_v >= 0.0f))
            return fail(GS_ERR_INVALID, "the noise's sigmas must be finite and >= 0 (entry %llu: %g, %g)", (unsigned long long)i,
                        (double)noise[i].sigma_u, (double)noise[i].sigma_v);
    if (e->members > 0x80000000ull)
        return fail(GS_ERR_UNSUPPORTED, "noise on more than 2^31 members (the noise kernels take the list of active members, 32-bit indices)");
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GS_HIP(hipStreamSynchronize(sl.compute)); // launches in flight read the table
    if (!e->noise_table) {
        const hipError_t err = hipMalloc(reinterpret_cast<void **>(&e->noise_table), (size_t)e->members * sizeof(GsEnsNoise));
        if (err != hipSuccess) {
            e->noise_table = nullptr;
            return fail(err == hipErrorOutOfMemory ? GS_ERR_NOMEM : GS_ERR_HIP, "noise table allocation failed: %s", hipGetErrorString(err));
        }
    }
    if (e->noise.empty()) { // the first call attaches: members never named hold sigmas 0, seed 0 and step 0 from here on
        try {
            e->noise.assign((size_t)e->members, GsEnsNoise{});
        } catch (const std::bad_alloc &) {
            return fail(GS_ERR_NOMEM, "out of host memory");
        }
        for (uint64_t m = 0; m < e->members; ++m) set_noise_offset(e->noise[m], 0 - e->noise_clock(m));
    }
    for (uint64_t i = 0; i < count; ++i) {
        const gs_noise &n = noise[entries == 1 ? 0 : i];
        GsEnsNoise &q = e->noise[first + i];
        q.sigma_u = n.sigma_u;
        q.sigma_v = n.sigma_v;
        q.seed_lo = (uint32_t)n.seed;
        q.seed_hi = (uint32_t)(n.seed >> 32);
        set_noise_offset(q, n.step - e->noise_clock(first + i));
    }
    GS_HIP(hipMemcpy(e->noise_table, e->noise.data(), e->noise.size() * sizeof(GsEnsNoise), hipMemcpyHostToDevice));
    return GS_OK;
}

int32_t gs_members_get_noise(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, gs_noise *out, int32_t *attached)
{
    GS_TRY(check_ensemble(ctx, e));
    if (!out && !attached) return fail(GS_ERR_INVALID, "null outputs");
    GS_TRY(check_member_range(e, first, count));
    if (attached) *attached = e->noise.empty() ? 0 : 1;
    if (e->noise.empty() || !out) return GS_OK;
    for (uint64_t i = 0; i < count; ++i) {
        const GsEnsNoise &q = e->noise[first + i];
        out[i].sigma_u = q.sigma_u;
        out[i].sigma_v = q.sigma_v;
        out[i].seed = (uint64_t)q.seed_hi << 32 | q.seed_lo;
        out[i].step = e->noise_clock(first + i) + noise_offset(q);
    }
    return GS_OK;
}

int32_t gs_members_clear_noise(gs_ctx *ctx, gs_ensemble *e)
{
    GS_TRY(check_ensemble(ctx, e));
    if (e->noise.empty()) return GS_OK;
    SlabRt &sl = ctx->slabs[0];
    GS_HIP(hipSetDevice(sl.device));
    GS_HIP(hipStreamSynchronize(sl.compute)); // launches in flight read the table
    (void)hipFree(e->noise_table);
    e->noise_table = nullptr;
    std::vector<GsEnsNoise>().swap(e->noise);
    return GS_OK;
}

} // extern "C"
