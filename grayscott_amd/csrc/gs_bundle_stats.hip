// gs_bundle_stats.hip -- per-cell statistics across the members of a bundle (include/gs_hip.h: gs_members_bundle_stats): a
// bundle is `span` consecutive members of an ensemble, and one launch forms the result planes of many bundles in one pass.
//
// A member's plane is dense (pitch = cols), so a bundle is `span` flat arrays of `cells` floats, one member apart.
// gs_bundle_stats_k<GROUPS, VEC>: grid (blocks of 1024 cells, bundles, species).  A lane owns four consecutive cells of the
// flat plane for one bundle; it keeps the accumulators of the selected groups in registers (GROUPS, the bits of
// gs_time_stats.hip: a group that is not selected costs no instruction), walks the members in ascending order -- the loads
// of kAhead members are issued before the first addition, as gs_tstat_accumulate_k issues those of kUnroll blocks; a span's
// remainder goes in groups of 4, 2 and 1, never behind a condition per member, which made the compiler keep one load in
// flight -- and writes the requested result planes alone.  The accumulators and the result formulas are those of
// gs_time_stats.hip, word for word, with member j in the place of sample j: sum and squares are plain sequential f64
// additions in member order -- no span is ever split over lanes, waves or launches --, so a bundle's planes are the bits of
// the time statistics of a lone Species sampled through the members' states.
// Traffic: 4 bytes read per cell, member and species, 4 n / span written; no accumulator memory, no read-modify-write.
// VEC = true: one 16-byte load per member and one 16-byte store per result (every member begins on 16 bytes: cells is a
// multiple of 4, so no quad is ragged either); VEC = false: per-cell loads at clamped cells, stores to cells below `cells`.
// All offsets are 64-bit.
//
// Built with hipcc's default float mode (f32 denormals kept): a sub-normal value counts as the value it is.
#include "gs_kernels.h"
#include "gs_plane_scan.h"

namespace {

constexpr uint32_t kSum = 1, kSquares = 2, kExtremes = 4, kCrossings = 8;           // GS_TSTAT_SUM .. GS_TSTAT_CROSSINGS
constexpr int kMean = 0, kVariance = 1, kMin = 2, kMax = 3, kOccupancy = 4;          // GS_TSTAT_MEAN .. GS_TSTAT_OCCUPANCY
// Members whose loads a lane issues before it adds the first: 4 VGPRs each, beside at most 28 of accumulators.
constexpr int kAhead = 8;

struct GsBundleLaunch {
    const float *in[2];  // U, V of the first bundle's first member
    float *out[2][5];    // [species][result code]: the plane of the first bundle's result, null where not requested
    int64_t cells;       // of a member: the distance between two members, in and out
    int64_t span;
    double n;            // (double)span
    float t[2];
    uint32_t flip[2];
};

// Cells i .. i + 3 of the member at `p`.
template <bool VEC>
__device__ __forceinline__ void load_cells(float (&v)[4], const float *p, int64_t i, int64_t last)
{
    if (VEC) {
        const float4 x = *reinterpret_cast<const float4 *>(p + i);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[i + j < last ? i + j : last];
    }
}

template <bool VEC>
__device__ __forceinline__ void store_cells(float *p, const float (&v)[4], int64_t i, int64_t cells)
{
    if (VEC) {
        *reinterpret_cast<float4 *>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < cells) p[i + j] = v[j];
    }
}

// N consecutive members from the one at `p`, cells i .. i + 3: every load is issued before the first addition, and the
// members are added in ascending order.
template <int N, uint32_t GROUPS, bool VEC>
__device__ __forceinline__ void add_members(const float *p, int64_t cells, int64_t i, int64_t last, uint32_t flip, float t,
                                            double (&s)[4], double (&q)[4], float (&mn)[4], float (&mx)[4], uint32_t (&cnt)[4])
{
    constexpr bool S = (GROUPS & kSum) != 0, Q = (GROUPS & kSquares) != 0, E = (GROUPS & kExtremes) != 0,
                   C = (GROUPS & kCrossings) != 0;
    float x[N][4];
#pragma unroll
    for (int u = 0; u < N; ++u) load_cells<VEC>(x[u], p + u * cells, i, last);
#pragma unroll
    for (int u = 0; u < N; ++u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = x[u][j];
            if (S) s[j] = s[j] + (double)v;
            if (Q) q[j] = q[j] + (double)v * (double)v;
            if (E) {
                mn[j] = v < mn[j] ? v : mn[j];
                mx[j] = v > mx[j] ? v : mx[j];
            }
            if (C) cnt[j] += gs_is_set(v, flip, t) ? 1u : 0u;
        }
    }
}

template <uint32_t GROUPS, bool VEC>
__global__ __launch_bounds__(256) void gs_bundle_stats_k(GsBundleLaunch a)
{
    constexpr bool S = (GROUPS & kSum) != 0, Q = (GROUPS & kSquares) != 0, E = (GROUPS & kExtremes) != 0,
                   C = (GROUPS & kCrossings) != 0;
    const int64_t cells = a.cells, span = a.span;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= cells) return;
    const int sp = (int)blockIdx.z;
    const int64_t bundle = blockIdx.y;
    const float *in = a.in[sp] + bundle * span * cells;
    const float t = a.t[sp];
    const uint32_t flip = a.flip[sp];
    const int64_t last = cells - 1;

    double s[4], q[4];
    float mn[4], mx[4];
    uint32_t cnt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[j] = 0.0, q[j] = 0.0;
        mn[j] = __builtin_inff(), mx[j] = -__builtin_inff();
        cnt[j] = 0u;
    }
    // whole groups of kAhead members, then the rest as groups of 4, 2 and 1: ascending order throughout
    int64_t m = 0;
    for (; m + kAhead <= span; m += kAhead) add_members<kAhead, GROUPS, VEC>(in + m * cells, cells, i, last, flip, t, s, q, mn, mx, cnt);
    if (kAhead > 4 && m + 4 <= span) add_members<4, GROUPS, VEC>(in + m * cells, cells, i, last, flip, t, s, q, mn, mx, cnt), m += 4;
    if (m + 2 <= span) add_members<2, GROUPS, VEC>(in + m * cells, cells, i, last, flip, t, s, q, mn, mx, cnt), m += 2;
    if (m < span) add_members<1, GROUPS, VEC>(in + m * cells, cells, i, last, flip, t, s, q, mn, mx, cnt);
    // the result planes: gs_tstat_result_k's formulas -- f64 throughout, every operation rounded once, the divisions the
    // compiler's IEEE sequence, one conversion to f32 at the end
    const int64_t at = bundle * cells;
    const double n = a.n;
    float r[4];
    if (S && a.out[sp][kMean]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (float)(s[j] / n);
        store_cells<VEC>(a.out[sp][kMean] + at, r, i, cells);
    }
    if (S && Q && a.out[sp][kVariance]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double m = s[j] / n;
            const double d = q[j] / n - m * m;
            r[j] = (float)(!(d <= 0.0) ? d : 0.0); // (a NaN stays NaN)
        }
        store_cells<VEC>(a.out[sp][kVariance] + at, r, i, cells);
    }
    if (E && a.out[sp][kMin]) store_cells<VEC>(a.out[sp][kMin] + at, mn, i, cells);
    if (E && a.out[sp][kMax]) store_cells<VEC>(a.out[sp][kMax] + at, mx, i, cells);
    if (C && a.out[sp][kOccupancy]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (float)((double)cnt[j] / n);
        store_cells<VEC>(a.out[sp][kOccupancy] + at, r, i, cells);
    }
}

template <uint32_t GROUPS>
void launch_bundles(bool vec, dim3 grid, const GsBundleLaunch &a, hipStream_t s)
{
    if (vec)
        hipLaunchKernelGGL((gs_bundle_stats_k<GROUPS, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((gs_bundle_stats_k<GROUPS, false>), grid, dim3(256), 0, s, a);
}

} // namespace

hipError_t gs_launch_bundle_stats(const float *const in[2], float *const out[2][5], int64_t cells, int64_t span, int64_t bundles,
                                  const float t[2], const uint32_t flip[2], hipStream_t s)
{
    if (cells <= 0 || span <= 0 || bundles <= 0) return hipSuccess;
    uint32_t groups = 0;
    bool vec = cells % 4 == 0;
    for (int sp = 0; sp < 2; ++sp) {
        vec = vec && reinterpret_cast<uintptr_t>(in[sp]) % 16 == 0;
        for (int w = 0; w < 5; ++w) {
            if (!out[sp][w]) continue;
            vec = vec && reinterpret_cast<uintptr_t>(out[sp][w]) % 16 == 0;
            groups |= w == kMean ? kSum : w == kVariance ? kSum | kSquares : w == kOccupancy ? kCrossings : kExtremes;
        }
    }
    if (groups == 0) return hipErrorInvalidValue;
    const int64_t blocks = (cells + 1023) / 1024;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    constexpr int64_t kMaxY = 65535; // bundles of one launch: a grid's second dimension
    for (int64_t b0 = 0; b0 < bundles; b0 += kMaxY) {
        const int64_t nb = bundles - b0 < kMaxY ? bundles - b0 : kMaxY;
        GsBundleLaunch a{};
        a.cells = cells, a.span = span, a.n = (double)(uint64_t)span;
        for (int sp = 0; sp < 2; ++sp) {
            a.in[sp] = in[sp] + b0 * span * cells;
            a.t[sp] = t[sp], a.flip[sp] = flip[sp];
            for (int w = 0; w < 5; ++w) a.out[sp][w] = out[sp][w] ? out[sp][w] + b0 * cells : nullptr;
        }
        const dim3 grid((unsigned)blocks, (unsigned)nb, 2);
        switch (groups) {
#define GS_BUNDLE_CASE(G) case G: launch_bundles<G>(vec, grid, a, s); break;
            // (squares are kept for the variance alone, which needs the sum: 2, 6, 10 and 14 do not occur)
            GS_BUNDLE_CASE(1) GS_BUNDLE_CASE(3) GS_BUNDLE_CASE(4) GS_BUNDLE_CASE(5) GS_BUNDLE_CASE(7) GS_BUNDLE_CASE(8)
            GS_BUNDLE_CASE(9) GS_BUNDLE_CASE(11) GS_BUNDLE_CASE(12) GS_BUNDLE_CASE(13) GS_BUNDLE_CASE(15)
#undef GS_BUNDLE_CASE
        default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
