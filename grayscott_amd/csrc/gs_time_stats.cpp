// gs_time_stats.cpp -- time statistics (include/gs_hip.h: gs_time_stats_*, gs_members_time_stats_*): per-cell accumulators
// over the samples of a run, kept on the device and added to by one launch per slab and sample (gs_time_stats.hip).
//   species form   one set of accumulators per slab on that slab's device, with the slab's rows and the fields' pitch: every
//                  cell is independent, so no rank exchanges anything and nothing is folded on the host.
//   ensemble form  the members' dense planes as one tall plane per species (pitch = cols) on slab 0.
// accumulate waits for enqueued work the way the other observables do (sync_all, which also runs again a persistent window
// launch that gave up), enqueues on the compute streams and returns; whatever reads or frees the accumulators waits first.
// No call touches the fields, their ghost rows, the tuner, the graphs or the context's counters.
#include "gs_internal.h"
#include "gs_plane_scan.h"

using namespace gsi;

struct gs_time_stats {
    gs_ctx *ctx = nullptr;
    uint64_t rows = 0, cols = 0; // of a plane: the global grid, or a member
    int32_t n = 0;               // planes
    uint32_t groups = 0;
    float t[4] = {0, 0, 0, 0};   // the set rule per plane as gs_is_set takes it
    uint32_t flip[4] = {0, 0, 0, 0};
    uint64_t samples = 0;
    bool members = false;        // the ensemble form ...
    uint64_t first = 0, count = 0; // ... of these members
    struct Slab {
        void *alloc = nullptr;
        GsTstatAcc acc{};
        int64_t rows = 0;  // of this slab (ensemble form: count x rows)
        uint64_t g_row0 = 0;
    };
    std::vector<Slab> s;
    int64_t pitch = 0;
};

namespace {

constexpr uint32_t kAllGroups = GS_TSTAT_SUM | GS_TSTAT_SQUARES | GS_TSTAT_EXTREMES | GS_TSTAT_CROSSINGS;
constexpr int kTstatGroupsPerCu = 8; // workgroups of 4 waves a launch may put on a CU, as the other plane scans

int64_t max_groups(const gs_ctx *ctx) { return (int64_t)kTstatGroupsPerCu * (ctx->cu_count > 0 ? ctx->cu_count : 256); }

// What both forms check before anything else: the groups, and the set rule where crossings are counted.
int32_t check_groups(gs_time_stats &ts, int32_t n, uint32_t groups, const float *thresholds, const int32_t *above)
{
    if (groups == 0 || (groups & ~kAllGroups)) return fail(GS_ERR_INVALID, "groups 0x%x: none, or unknown bits", groups);
    if (n < 1 || n > 4) return fail(GS_ERR_INVALID, "%d planes (1..4)", n);
    if (groups & GS_TSTAT_CROSSINGS) {
        if (!thresholds || !above) return fail(GS_ERR_INVALID, "crossings need a threshold and a sense per plane");
        for (int32_t i = 0; i < n; ++i) {
            if (std::isnan(thresholds[i])) return fail(GS_ERR_INVALID, "threshold %d is NaN", i);
            gs_set_rule(thresholds[i], above[i], ts.t[i], ts.flip[i]);
        }
    }
    ts.n = n;
    ts.groups = groups;
    return GS_OK;
}

// The group a result plane or a raw accumulator belongs to (0: no such plane), and a raw accumulator's element size.
uint32_t group_of_result(int32_t which)
{
    switch (which) {
    case GS_TSTAT_MEAN: return GS_TSTAT_SUM;
    case GS_TSTAT_VARIANCE: return GS_TSTAT_SUM | GS_TSTAT_SQUARES;
    case GS_TSTAT_MIN: case GS_TSTAT_MAX: return GS_TSTAT_EXTREMES;
    case GS_TSTAT_OCCUPANCY: case GS_TSTAT_ARRIVAL: return GS_TSTAT_CROSSINGS;
    default: return 0;
    }
}

uint32_t group_of_raw(int32_t raw, size_t *elem)
{
    *elem = raw <= GS_TSTAT_RAW_SQUARES ? sizeof(double) : sizeof(float);
    switch (raw) {
    case GS_TSTAT_RAW_SUM: return GS_TSTAT_SUM;
    case GS_TSTAT_RAW_SQUARES: return GS_TSTAT_SQUARES;
    case GS_TSTAT_RAW_MIN: case GS_TSTAT_RAW_MAX: return GS_TSTAT_EXTREMES;
    case GS_TSTAT_RAW_SET_COUNT: case GS_TSTAT_RAW_FIRST_STAMP: return GS_TSTAT_CROSSINGS;
    default: return 0;
    }
}

const void *raw_base(const GsTstatAcc &acc, int32_t raw)
{
    switch (raw) {
    case GS_TSTAT_RAW_SUM: return acc.sum;
    case GS_TSTAT_RAW_SQUARES: return acc.squares;
    case GS_TSTAT_RAW_MIN: return acc.mn;
    case GS_TSTAT_RAW_MAX: return acc.mx;
    case GS_TSTAT_RAW_SET_COUNT: return acc.set_count;
    default: return acc.first_stamp;
    }
}

void free_slabs(gs_time_stats *ts)
{
    for (size_t i = 0; i < ts->s.size(); ++i)
        if (ts->s[i].alloc) {
            (void)hipSetDevice(ts->ctx->slabs[i].device);
            (void)hipFree(ts->s[i].alloc);
        }
    delete ts;
}

// Slab i's accumulators: one block, every selected array of n planes `plane_stride` elements apart -- a multiple of 64, so
// that every plane of every array begins on 256 bytes (hipMalloc's blocks do) -- at the reset values.
int32_t allocate_slab(gs_time_stats *ts, size_t i)
{
    gs_time_stats::Slab &sl = ts->s[i];
    const int64_t cells = sl.rows * ts->pitch;
    GsTstatAcc &acc = sl.acc;
    acc.plane_stride = (cells + 63) / 64 * 64;
    if (cells == 0) return GS_OK;
    const size_t count = (size_t)ts->n * (size_t)acc.plane_stride;
    size_t bytes = 0;
    if (ts->groups & GS_TSTAT_SUM) bytes += count * sizeof(double);
    if (ts->groups & GS_TSTAT_SQUARES) bytes += count * sizeof(double);
    if (ts->groups & GS_TSTAT_EXTREMES) bytes += 2 * count * sizeof(float);
    if (ts->groups & GS_TSTAT_CROSSINGS) bytes += 2 * count * sizeof(uint32_t);
    SlabRt &rt = ts->ctx->slabs[i];
    GS_HIP(hipSetDevice(rt.device));
    const hipError_t e = hipMalloc(&sl.alloc, bytes);
    if (e != hipSuccess) {
        sl.alloc = nullptr;
        (void)hipGetLastError(); // (the runtime keeps the failure as its last error: the next launch's check would report it)
        return fail(e == hipErrorOutOfMemory ? GS_ERR_NOMEM : GS_ERR_HIP, "time statistics of %zu bytes: %s", bytes, hipGetErrorString(e));
    }
    unsigned char *at = static_cast<unsigned char *>(sl.alloc);
    if (ts->groups & GS_TSTAT_SUM) acc.sum = reinterpret_cast<double *>(at), at += count * sizeof(double);
    if (ts->groups & GS_TSTAT_SQUARES) acc.squares = reinterpret_cast<double *>(at), at += count * sizeof(double);
    if (ts->groups & GS_TSTAT_EXTREMES) {
        acc.mn = reinterpret_cast<float *>(at), at += count * sizeof(float);
        acc.mx = reinterpret_cast<float *>(at), at += count * sizeof(float);
    }
    if (ts->groups & GS_TSTAT_CROSSINGS) {
        acc.set_count = reinterpret_cast<uint32_t *>(at), at += count * sizeof(uint32_t);
        acc.first_stamp = reinterpret_cast<uint32_t *>(at);
    }
    GS_HIP(gs_launch_tstat_reset(ts->n, ts->groups, acc, rt.compute));
    return GS_OK;
}

int32_t finish_create(gs_time_stats *ts, gs_time_stats **out)
{
    int32_t st = GS_OK;
    for (size_t i = 0; i < ts->s.size() && st == GS_OK; ++i) st = allocate_slab(ts, i);
    if (st == GS_OK) st = sync_compute(ts->ctx);
    if (st != GS_OK) {
        free_slabs(ts);
        return st;
    }
    ts->ctx->time_stats.push_back(ts); // the context owns it: freed with the context at the latest
    *out = ts;
    return GS_OK;
}

int32_t check_object(const gs_ctx *ctx, const gs_time_stats *ts, bool members)
{
    if (!ctx || !ts) return fail(GS_ERR_INVALID, "null argument");
    if (ts->ctx != ctx) return fail(GS_ERR_INVALID, "time statistics of another context");
    if (ts->members != members)
        return fail(GS_ERR_INVALID, members ? "time statistics of fields, not of ensemble members" : "time statistics of ensemble members, not of fields");
    return GS_OK;
}

int32_t check_result(const gs_time_stats *ts, int32_t plane, int32_t which)
{
    const uint32_t need = group_of_result(which);
    if (need == 0) return fail(GS_ERR_INVALID, "no result plane %d", which);
    if ((ts->groups & need) != need) return fail(GS_ERR_INVALID, "result plane %d needs groups 0x%x, selected 0x%x", which, need, ts->groups);
    if (plane < 0 || plane >= ts->n) return fail(GS_ERR_INVALID, "plane %d of %d", plane, ts->n);
    if (ts->samples == 0) return fail(GS_ERR_INVALID, "no sample yet");
    return GS_OK;
}

// One sample of slab i's planes; a dense plane (pitch == cols) is scanned as rows of up to 4096 columns where its cells divide
// so: every cell is independent and keeps its place, and short rows would leave most of a wave's lanes idle.
int32_t accumulate_slab(gs_time_stats *ts, size_t i, const float *const *planes, uint32_t stamp)
{
    const gs_time_stats::Slab &sl = ts->s[i];
    if (sl.rows == 0 || ts->cols == 0) return GS_OK;
    SlabRt &rt = ts->ctx->slabs[i];
    GS_HIP(hipSetDevice(rt.device));
    int64_t rows = sl.rows, cols = (int64_t)ts->cols, pitch = ts->pitch;
    if (pitch == cols)
        for (int64_t w = 4096; w > cols; w /= 2)
            if ((rows * cols) % w == 0) {
                rows = rows * cols / w, cols = pitch = w;
                break;
            }
    GS_HIP(gs_launch_tstat_accumulate(planes, ts->n, pitch, rows, (int32_t)cols, ts->groups, sl.acc, ts->t, ts->flip, stamp,
                                      max_groups(ts->ctx), rt.compute));
    return GS_OK;
}

} // namespace

namespace gsi {

// gs_ctx_destroy: whatever time statistics the context still owns go with it (their handles are dead from then on).
void destroy_time_stats(gs_ctx *ctx)
{
    if (ctx->time_stats.empty()) return;
    (void)sync_all(ctx);
    for (gs_time_stats *ts : ctx->time_stats) free_slabs(ts);
    ctx->time_stats.clear();
}

} // namespace gsi

extern "C" {

int32_t gs_time_stats_create(gs_ctx *ctx, gs_time_stats **out, uint64_t rows, uint64_t cols, int32_t n, uint32_t groups,
                             const float *thresholds, const int32_t *above)
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    *out = nullptr;
    gs_time_stats proto;
    GS_TRY(check_groups(proto, n, groups, thresholds, above));
    PlaneLayout layout; // the slabs and the pitch of a field of this shape, with gs_field_create's refusals
    GS_TRY(plane_layout(ctx, rows, cols, layout));
    gs_time_stats *ts = new (std::nothrow) gs_time_stats(proto);
    if (!ts) return fail(GS_ERR_NOMEM, "out of host memory");
    ts->ctx = ctx;
    ts->rows = rows, ts->cols = cols, ts->pitch = (int64_t)layout.pitch;
    ts->s.resize(layout.slabs.size());
    for (size_t i = 0; i < ts->s.size(); ++i) {
        ts->s[i].g_row0 = layout.slabs[i].first;
        ts->s[i].rows = (int64_t)layout.slabs[i].second;
    }
    return finish_create(ts, out);
}

int32_t gs_members_time_stats_create(gs_ctx *ctx, gs_time_stats **out, gs_ensemble *like, uint64_t first, uint64_t count,
                                     uint32_t groups, const float thresholds[2], const int32_t above[2])
{
    if (!ctx || !out) return fail(GS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (ctx->slabs.size() != 1 || ctx->world != 1) // (gs_ensemble_create's refusal)
        return fail(GS_ERR_UNSUPPORTED, "an ensemble lives on a context of one slab in one process (%d slabs x %d processes)",
                    (int)ctx->slabs.size(), ctx->world);
    gs_time_stats proto;
    GS_TRY(check_groups(proto, 2, groups, thresholds, above));
    if (!like) return fail(GS_ERR_INVALID, "null argument");
    if (like->ctx != ctx) return fail(GS_ERR_INVALID, "ensemble belongs to another context");
    GS_TRY(check_member_range(like, first, count));
    gs_time_stats *ts = new (std::nothrow) gs_time_stats(proto);
    if (!ts) return fail(GS_ERR_NOMEM, "out of host memory");
    ts->ctx = ctx;
    ts->members = true;
    ts->first = first, ts->count = count;
    ts->rows = like->rows, ts->cols = like->cols, ts->pitch = (int64_t)like->cols;
    ts->s.resize(1);
    ts->s[0].rows = (int64_t)(count * like->rows);
    return finish_create(ts, out);
}

int32_t gs_time_stats_destroy(gs_ctx *ctx, gs_time_stats *ts)
{
    if (!ts) return GS_OK;
    if (!ctx || ts->ctx != ctx) return fail(GS_ERR_INVALID, "time statistics destroyed with another context");
    (void)sync_all(ctx); // no launch may still use the accumulators
    ctx->time_stats.erase(std::remove(ctx->time_stats.begin(), ctx->time_stats.end(), ts), ctx->time_stats.end());
    free_slabs(ts);
    return GS_OK;
}

int32_t gs_time_stats_reset(gs_ctx *ctx, gs_time_stats *ts)
{
    if (!ctx || !ts) return fail(GS_ERR_INVALID, "null argument");
    if (ts->ctx != ctx) return fail(GS_ERR_INVALID, "time statistics of another context");
    GS_TRY(sync_all(ctx));
    for (size_t i = 0; i < ts->s.size(); ++i) {
        if (!ts->s[i].alloc) continue;
        GS_HIP(hipSetDevice(ctx->slabs[i].device));
        GS_HIP(gs_launch_tstat_reset(ts->n, ts->groups, ts->s[i].acc, ctx->slabs[i].compute));
    }
    GS_TRY(sync_compute(ctx));
    ts->samples = 0;
    return GS_OK;
}

int32_t gs_time_stats_accumulate(gs_ctx *ctx, gs_time_stats *ts, gs_field *const *fields, int32_t n, uint32_t stamp)
{
    if (!fields) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_object(ctx, ts, false));
    if (n != ts->n) return fail(GS_ERR_INVALID, "%d fields for time statistics of %d planes", n, ts->n);
    if (stamp == 0xffffffffu) return fail(GS_ERR_INVALID, "stamp 0xffffffff marks a cell that was never set");
    for (int32_t p = 0; p < n; ++p) {
        if (!fields[p] || fields[p]->ctx != ctx) return fail(GS_ERR_INVALID, "field %d: null or of another context", p);
        if (fields[p]->rows != ts->rows || fields[p]->cols != ts->cols || (int64_t)fields[p]->pitch != ts->pitch)
            return fail(GS_ERR_INVALID, "field %d of [%llu, %llu], time statistics of [%llu, %llu]", p, (unsigned long long)fields[p]->rows,
                        (unsigned long long)fields[p]->cols, (unsigned long long)ts->rows, (unsigned long long)ts->cols);
    }
    GS_TRY(sync_all(ctx)); // (also runs again a persistent window launch that gave up: no stale plane is sampled)
    for (size_t i = 0; i < ts->s.size(); ++i) {
        const float *planes[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int32_t p = 0; p < n; ++p) planes[p] = fields[p]->s[i].row0;
        GS_TRY(accumulate_slab(ts, i, planes, stamp));
    }
    ts->samples += 1;
    return GS_OK;
}

int32_t gs_members_time_stats_accumulate(gs_ctx *ctx, gs_time_stats *ts, gs_ensemble *e, uint32_t stamp)
{
    if (!e) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_object(ctx, ts, true));
    if (e->ctx != ctx) return fail(GS_ERR_INVALID, "ensemble belongs to another context");
    if (e->rows != ts->rows || e->cols != ts->cols)
        return fail(GS_ERR_INVALID, "members of [%llu, %llu], time statistics of [%llu, %llu]", (unsigned long long)e->rows,
                    (unsigned long long)e->cols, (unsigned long long)ts->rows, (unsigned long long)ts->cols);
    GS_TRY(check_member_range(e, ts->first, ts->count));
    if (stamp == 0xffffffffu) return fail(GS_ERR_INVALID, "stamp 0xffffffff marks a cell that was never set");
    GS_TRY(sync_all(ctx));
    const uint64_t cells = e->rows * e->cols;
    const float *planes[4] = {e->u[e->cur] + ts->first * cells, e->v[e->cur] + ts->first * cells, nullptr, nullptr};
    GS_TRY(accumulate_slab(ts, 0, planes, stamp));
    ts->samples += 1;
    return GS_OK;
}

int32_t gs_time_stats_samples(const gs_time_stats *ts, uint64_t *n)
{
    if (!ts || !n) return fail(GS_ERR_INVALID, "null argument");
    *n = ts->samples;
    return GS_OK;
}

int32_t gs_time_stats_result(gs_ctx *ctx, gs_time_stats *ts, int32_t plane, int32_t which, gs_field *out)
{
    if (!out) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_object(ctx, ts, false));
    GS_TRY(check_result(ts, plane, which));
    if (out->ctx != ctx) return fail(GS_ERR_INVALID, "result field of another context");
    if (out->rows != ts->rows || out->cols != ts->cols || (int64_t)out->pitch != ts->pitch)
        return fail(GS_ERR_INVALID, "result field of [%llu, %llu], time statistics of [%llu, %llu]", (unsigned long long)out->rows,
                    (unsigned long long)out->cols, (unsigned long long)ts->rows, (unsigned long long)ts->cols);
    GS_TRY(sync_all(ctx));
    for (size_t i = 0; i < ts->s.size(); ++i) {
        if (!ts->s[i].alloc) continue;
        GS_HIP(hipSetDevice(ctx->slabs[i].device));
        GS_HIP(gs_launch_tstat_result(which, plane, ts->s[i].acc, ts->pitch, ts->s[i].rows, (int32_t)ts->cols, ts->samples,
                                      out->s[i].row0, ctx->slabs[i].compute));
    }
    GS_TRY(sync_compute(ctx));
    out->ghost_depth = 0; // as after gs_fields_copy: the next step refreshes the ghost rows
    return GS_OK;
}

int32_t gs_members_time_stats_result(gs_ctx *ctx, gs_time_stats *ts, int32_t species, int32_t which, float *host)
{
    if (!host) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(check_object(ctx, ts, true));
    GS_TRY(check_result(ts, species, which));
    GS_TRY(sync_all(ctx));
    const gs_time_stats::Slab &sl = ts->s[0];
    const size_t bytes = (size_t)sl.rows * (size_t)ts->cols * sizeof(float);
    GS_TRY(ensure_scratch(ctx, 0, bytes, "time statistics"));
    SlabRt &rt = ctx->slabs[0];
    GS_HIP(hipSetDevice(rt.device));
    float *dev = static_cast<float *>(rt.scratch);
    GS_HIP(gs_launch_tstat_result(which, species, sl.acc, ts->pitch, sl.rows, (int32_t)ts->cols, ts->samples, dev, rt.compute));
    GS_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, rt.compute));
    GS_HIP(hipStreamSynchronize(rt.compute));
    return GS_OK;
}

int32_t gs_time_stats_download(gs_ctx *ctx, gs_time_stats *ts, int32_t plane, int32_t raw, void *host)
{
    if (!ctx || !ts) return fail(GS_ERR_INVALID, "null argument");
    if (ts->ctx != ctx) return fail(GS_ERR_INVALID, "time statistics of another context");
    size_t elem = 0;
    const uint32_t need = group_of_raw(raw, &elem);
    if (need == 0) return fail(GS_ERR_INVALID, "no raw accumulator %d", raw);
    if (!(ts->groups & need)) return fail(GS_ERR_INVALID, "raw accumulator %d needs group 0x%x, selected 0x%x", raw, need, ts->groups);
    if (plane < 0 || plane >= ts->n) return fail(GS_ERR_INVALID, "plane %d of %d", plane, ts->n);
    bool empty = ts->cols == 0; // nothing to copy: host may be null, as for gs_field_download
    if (!empty) {
        empty = true;
        for (const gs_time_stats::Slab &sl : ts->s) empty = empty && sl.rows == 0;
    }
    if (!empty && !host) return fail(GS_ERR_INVALID, "null argument");
    GS_TRY(sync_all(ctx));
    if (empty) return GS_OK;
    const uint64_t first = ts->s.front().g_row0;
    for (size_t i = 0; i < ts->s.size(); ++i) {
        const gs_time_stats::Slab &sl = ts->s[i];
        if (!sl.alloc) continue;
        GS_HIP(hipSetDevice(ctx->slabs[i].device));
        const unsigned char *src = static_cast<const unsigned char *>(raw_base(sl.acc, raw)) + (size_t)plane * (size_t)sl.acc.plane_stride * elem;
        GS_HIP(hipMemcpy2D(static_cast<unsigned char *>(host) + (size_t)(sl.g_row0 - first) * ts->cols * elem, (size_t)ts->cols * elem, src,
                           (size_t)ts->pitch * elem, (size_t)ts->cols * elem, (size_t)sl.rows, hipMemcpyDeviceToHost));
    }
    return GS_OK;
}

} // extern "C"
