// gs_regions.hip -- regional observables on the device (include/gs_hip.h: gs_fields_region_summaries,
// gs_fields_region_morphology): the summary and the bit-quad counts of every region of rh x rw cells of a plane, each bit for
// bit what gs_summary.hip and gs_morphology.hip return for a plane that holds that region's cells alone.  rw is a multiple of
// 4 (a lane's four columns never straddle two regions, and its 16-byte load is aligned wherever the whole-grid kernels' are);
// the regions of the last row and column of the region grid may be ragged.  Both kernels read every cell once, 16 B per lane.
//
// gs_region_summary_k: a wave owns a unit -- one row of the region grid x as many regions as fit side by side in a wave row of
// 256 columns (one region when rw >= 256) -- and marches down it with the field fold in registers: no record leaves the wave
// but the region's own.  A region of rw < 256 columns takes the rw / 4 lanes of its segment; the row partial of gs_hip.h with
// columns counted from the region's first one is the halving tree over the 64 lanes of which those past the segment hold
// +0.0, so a shuffle from lane + m whose partner lies outside the segment is read as +0.0 (adding +0.0 leaves an accumulator
// that started at +0.0 as it was: take() in gs_summary.hip).  Narrow regions load kSumUnroll rows ahead and run the trees of
// those rows side by side; wide ones (rw >= 256) load kSumUnroll chunks of 256 columns ahead, as gs_row_summary_k does.
// min, max and the non-finite count are order-free: they stay per lane until the region's end.
//
// gs_region_quads_k: gs_plane_quads_k's second form.  Strips of 256 columns of the plane as there; a unit is a strip x a run of
// quad rows of ONE row of the region grid, so a lane stays inside one region for a unit.  The region's image is padded with its
// own ring of unset cells: the lane whose first column is a region's first column counts the left padding quads, the lane whose
// last column is a region's last one sees an unset right neighbour, the row above a region's first row is unset and never read,
// and the quad row below its last row is always counted.  At a unit's end the lane counters are added over each run of lanes
// of one region (a segmented shuffle sum: integers, order-free) and the run's first lane adds them to the region's u64 counters.
//
// Built with hipcc's default float mode (f32 denormals kept), as their whole-grid twins are.
#include "gs_kernels.h"
#include "gs_plane_scan.h"

namespace {

// ---- summaries -------------------------------------------------------------------------------------------------------
constexpr int kSumUnroll = 8; // rows (narrow regions) or chunks of 256 columns (wide ones) whose loads a wave issues before it adds them

struct GsRegionSumArgs {
    GsPlaneSet set;     // the slab's planes (no repeats)
    int32_t rh, rw;     // the region shape
    int32_t seg;        // lanes of a region in a wave row: min(rw / 4, 64)
    int32_t side;       // regions side by side in a wave row: 64 / seg (1 when rw >= 256)
    int32_t rr, rc;     // rows of the region grid in this slab, columns of the region grid: rr * rc <= GS_REGIONS_MAX, so
    int32_t col_groups; // ceil(rc / side), and the units of a plane, are 32-bit numbers
    GsRegionSummary *out; // [plane][rr][rc]
};

// One cell: gs_summary.hip's take() with the order-free parts kept apart.
__device__ __forceinline__ void take_cell(double &s, double &q, float &mn, float &mx, uint32_t &nf, float x, bool valid)
{
    const bool fin = valid && __builtin_isfinite(x);
    const double d = fin ? (double)x : 0.0;
    s += d;
    q += d * d; // exact: a 24-bit significand squared fits in 53 bits
    mn = fminf(mn, fin ? x : __builtin_huge_valf());
    mx = fmaxf(mx, fin ? x : -__builtin_huge_valf());
    nf += (valid && !fin) ? 1u : 0u;
}

// grid (unit groups, planes), 4 waves per workgroup, one unit per wave at a time (grid-stride over units).
template <bool WIDE>
__global__ __launch_bounds__(256) void gs_region_summary_k(GsRegionSumArgs a)
{
    const int lane = (int)(threadIdx.x & 63);
    const float *plane = a.set.p[blockIdx.y];
    const int cols = a.set.cols;
    const int64_t rows = a.set.rows, pitch = a.set.pitch;
    const int g = lane / a.seg, v = lane - g * a.seg; // the lane's region of the wave row, and its place in that region
    const int units = a.rr * a.col_groups;
    for (int u = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); u < units; u += (int)gridDim.x * 4) {
        const int i = u / a.col_groups, j = (u - i * a.col_groups) * a.side + g;
        const bool mine = g < a.side && j < a.rc;
        const int64_t r0 = (int64_t)i * a.rh, r1 = r0 + a.rh < rows ? r0 + a.rh : rows;
        // the region's columns [cb, ce); a lane without a region holds none
        const int cb = mine ? j * a.rw : cols; // (j rw < cols)
        const int ce = (int64_t)cb + a.rw < cols ? cb + a.rw : cols;
        double fs = 0.0, fq = 0.0; // the field fold of the region, rows added from +0.0
        float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
        uint32_t nf = 0u;

        if (!WIDE) {
            const int c = mine ? cb + 4 * v : cols;
            const GsLaneColumns at = gs_lane_columns(c, cols);
            const bool ok0 = c < ce, ok1 = ok0 && c + 1 < ce, ok2 = ok0 && c + 2 < ce, ok3 = ok0 && c + 3 < ce;
            for (int64_t r = r0; r < r1; r += kSumUnroll) { // (scalar: no lane leaves early)
                float4 x[kSumUnroll];
#pragma unroll
                for (int k = 0; k < kSumUnroll; ++k) {
                    const int64_t row = r + k < r1 ? r + k : r1 - 1;
                    x[k] = gs_load_columns<true>(plane + row * pitch, at);
                }
                double s[kSumUnroll], q[kSumUnroll];
#pragma unroll
                for (int k = 0; k < kSumUnroll; ++k) {
                    const bool live = r + k < r1; // a row past the region adds +0.0 everywhere
                    s[k] = 0.0;
                    q[k] = 0.0;
                    take_cell(s[k], q[k], mn, mx, nf, x[k].x, live && ok0);
                    take_cell(s[k], q[k], mn, mx, nf, x[k].y, live && ok1);
                    take_cell(s[k], q[k], mn, mx, nf, x[k].z, live && ok2);
                    take_cell(s[k], q[k], mn, mx, nf, x[k].w, live && ok3);
                }
                // lane combine inside the segment: lane v ends the step of offset m with (its sum) + (lane v + m's, +0.0
                // past the segment); the segment's first lane ends with the halving order of gs_hip.h
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) {
                    const bool in = v + m < a.seg;
#pragma unroll
                    for (int k = 0; k < kSumUnroll; ++k) {
                        const double ps = __shfl_down(s[k], m), pq = __shfl_down(q[k], m);
                        s[k] = s[k] + (in ? ps : 0.0);
                        q[k] = q[k] + (in ? pq : 0.0);
                    }
                }
#pragma unroll
                for (int k = 0; k < kSumUnroll; ++k) {
                    fs = fs + s[k];
                    fq = fq + q[k];
                }
            }
        } else {
            const int w = ce - cb; // (one region per wave: seg == 64, v == lane)
            for (int64_t r = r0; r < r1; ++r) {
                const float *row = plane + r * pitch + cb;
                double s = 0.0, q = 0.0;
                for (int c0 = 4 * lane; c0 < w; c0 += 256 * kSumUnroll) {
                    float4 x[kSumUnroll];
#pragma unroll
                    for (int k = 0; k < kSumUnroll; ++k) {
                        const int c = c0 + 256 * k;
                        // (16 bytes that begin inside the region end inside the row's pitch; what lies past the region is masked)
                        x[k] = *reinterpret_cast<const float4 *>(row + (c < w ? c : 0));
                    }
#pragma unroll
                    for (int k = 0; k < kSumUnroll; ++k) {
                        const int c = c0 + 256 * k;
                        take_cell(s, q, mn, mx, nf, x[k].x, c < w);
                        take_cell(s, q, mn, mx, nf, x[k].y, c + 1 < w);
                        take_cell(s, q, mn, mx, nf, x[k].z, c + 2 < w);
                        take_cell(s, q, mn, mx, nf, x[k].w, c + 3 < w);
                    }
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) {
                    const bool in = lane + m < 64;
                    const double ps = __shfl_down(s, m), pq = __shfl_down(q, m);
                    s = s + (in ? ps : 0.0);
                    q = q + (in ? pq : 0.0);
                }
                fs = fs + s;
                fq = fq + q;
            }
        }
        // the order-free parts, over the segment (a lane's count fits 32 bits, a large region's need not)
        unsigned long long nfs = nf;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const bool in = v + m < a.seg;
            const float pmn = __shfl_down(mn, m), pmx = __shfl_down(mx, m);
            const unsigned long long pnf = __shfl_down(nfs, m);
            mn = fminf(mn, in ? pmn : __builtin_huge_valf());
            mx = fmaxf(mx, in ? pmx : -__builtin_huge_valf());
            nfs += in ? pnf : 0ull;
        }
        if (mine && v == 0) {
            GsRegionSummary o;
            o.sum = fs;
            o.sum_sq = fq;
            o.min = mn;
            o.max = mx;
            o.nonfinite = nfs;
            a.out[((int64_t)blockIdx.y * a.rr + i) * a.rc + j] = o;
        }
    }
}

// ---- bit quads ---------------------------------------------------------------------------------------------------------
constexpr int kQuadRows = 32;  // quad rows a unit holds at least when its region has that many: one row in kQuadRows + 1 is read twice
constexpr int kQuadUnroll = 8; // rows whose loads a wave issues before it classifies them
constexpr int kQuadClasses = 5; // Q1, Q2, Q3, Q4, QD
constexpr int kQuadSlots = 6;   // a result is gs_morphology's six words: Q0's is left to the host, the five counted follow it

// A lane's u32 counters live for one unit: at most 2 kQuadRows quad rows (the launcher's chunk_rows) of 5 quads, so a lane
// counter stays below 5 * 2^6 and the sum over the 64 lanes of a wave below 2^15 -- no u32 on the way can wrap whatever the
// plane; the region's counters are u64.
struct GsRegionQuadArgs {
    float t[4][4];      // per set.p[]: the thresholds and ...
    uint32_t flip[4];   // ... the sign flip of gs_is_set
    GsPlaneSet set;     // the slab's planes (no repeats)
    int32_t rh, rw;     // the region shape
    int32_t chunks;     // units a region's rh + 1 quad rows are cut into ...
    int32_t chunk_rows; // ... and the quad rows of each (the last may hold fewer)
    int64_t rr, rc;     // rows of the region grid in this slab, columns of the region grid
    int64_t groups;     // workgroups per plane
    unsigned long long *out; // [plane][rr][rc][nt][kQuadSlots], zeroed by the caller
};

// Lane l receives lane l + 1's `w`; lane 63, which has no such neighbour, keeps `last`.  Every lane active.
__device__ __forceinline__ unsigned from_right(unsigned w, unsigned last)
{
    return (unsigned)__builtin_amdgcn_update_dpp((int)last, (int)w, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

// The set bits of four cells at bits 1..4 of byte k for threshold k.
template <int NT>
__device__ __forceinline__ unsigned bits_of(float4 x, const float *t, uint32_t flip)
{
    unsigned w = 0u;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        w |= (gs_is_set(x.x, flip, t[k]) ? 2u : 0u) << (8 * k);
        w |= (gs_is_set(x.y, flip, t[k]) ? 4u : 0u) << (8 * k);
        w |= (gs_is_set(x.z, flip, t[k]) ? 8u : 0u) << (8 * k);
        w |= (gs_is_set(x.w, flip, t[k]) ? 16u : 0u) << (8 * k);
    }
    return w;
}

// 1-D grid of planes x groups workgroups of 4 waves.
template <int NT>
__global__ __launch_bounds__(256) void gs_region_quads_k(GsRegionQuadArgs a)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t y = (int64_t)blockIdx.x / a.groups, g = (int64_t)blockIdx.x % a.groups;
    int which;
    const float *plane = gs_plane_at(a.set, y, which);
    const uint32_t flip = a.flip[which];
    float t[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k] = a.t[which][k];

    const int cols = a.set.cols;
    const int64_t rows = a.set.rows, pitch = a.set.pitch;
    const int64_t strips = ((int64_t)cols + 255) / 256;
    const int64_t units = strips * a.rr * a.chunks;

    for (int64_t u = g * 4 + wave; u < units; u += a.groups * 4) {
        const int64_t band = u / strips, i = band / a.chunks;
        const int64_t r0 = i * a.rh;                                 // the region's first row, and its rows:
        const int64_t h = r0 + a.rh < rows ? a.rh : rows - r0;       // quad row q of it is its rows q - 1 and q, q = 0 .. h
        const int64_t q0 = (band % a.chunks) * a.chunk_rows;
        if (q0 > h) continue; // (scalar: a ragged region's last chunks are empty)
        const int64_t q1 = q0 + a.chunk_rows < h + 1 ? q0 + a.chunk_rows : h + 1;
        const int c0 = (int)(u % strips) * 256, c = c0 + 4 * lane;
        // own columns inside the row, in every byte; the extra cell at column c0 + 256 (wave-uniform)
        unsigned own = (c < cols ? 2u : 0u) | (c + 1 < cols ? 4u : 0u) | (c + 2 < cols ? 8u : 0u) | (c + 3 < cols ? 16u : 0u);
        own *= 0x01010101u;
        const unsigned extra_live = c0 + 256 < cols ? 0x02020202u : 0u;
        const int ce = c0 + 256 < cols ? c0 + 256 : cols - 1;
        const GsLaneColumns at = gs_lane_columns(c, cols);
        // the lane's region column and its place in it (rw is a multiple of 4: all four columns lie in one region)
        const unsigned jreg = (unsigned)c / (unsigned)a.rw, cin = (unsigned)c - jreg * (unsigned)a.rw;
        // the right corners of quad 0 count in a region's first lane alone: there the column to the left is the padding
        const unsigned right = (cin == 0u) ? 0x1f1f1f1fu : 0x1e1e1e1eu;
        // the column to the right of a region's last lane is the region's padding: never set
        const unsigned beyond = (cin + 4u == (unsigned)a.rw) ? 0u : 0x20202020u;

        // row r of the region as the wave reads it: an address that exists, and whether its cells count (both wave-uniform)
        auto row_at = [&](int64_t r, unsigned &live) -> const float * {
            live = (r >= 0 && r < h) ? ~0u : 0u;
            return plane + (r0 + (r < 0 ? 0 : (r < h ? r : h - 1))) * pitch;
        };
        auto load = [&](const float *row, float4 &x, float &xe) {
            x = gs_load_columns<true>(row, at);
            xe = row[ce];
        };
        // the row's word: bits 1..4 the lane's columns, bit 5 the column to its right, of every threshold's byte
        auto word = [&](float4 x, float xe, unsigned live) -> unsigned {
            const unsigned w = bits_of<NT>(x, t, flip) & own;
            const unsigned e = bits_of<NT>(make_float4(xe, xe, xe, xe), t, flip) & extra_live;
            const unsigned nb = from_right(w, e);
            return (w | (((nb & 0x02020202u) << 4) & beyond)) & live;
        };

        unsigned n[NT][kQuadClasses];
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int cl = 0; cl < kQuadClasses; ++cl) n[k][cl] = 0u;

        unsigned live0;
        float4 x0;
        float xe0;
        load(row_at(q0 - 1, live0), x0, xe0);
        const unsigned top = word(x0, xe0, live0);
        unsigned tl = top & 0x1f1f1f1fu, tr = (top >> 1) & right; // the corners of the row above, left and right

        for (int64_t q = q0; q < q1; q += kQuadUnroll) { // (scalar: no lane leaves early)
            float4 x[kQuadUnroll];
            float xe[kQuadUnroll];
            unsigned live[kQuadUnroll];
#pragma unroll
            for (int k = 0; k < kQuadUnroll; ++k) load(row_at(q + k, live[k]), x[k], xe[k]);
#pragma unroll
            for (int k = 0; k < kQuadUnroll; ++k) {
                if (q + k >= q1) break; // (scalar)
                const unsigned w = word(x[k], xe[k], live[k]);
                const unsigned bl = w & 0x1f1f1f1fu, br = (w >> 1) & right;
                // corners set, bit-sliced: b0 + 2 b1 + 4 q4
                const unsigned s1 = tl ^ tr, c1 = tl & tr, s2 = bl ^ br, c2 = bl & br;
                const unsigned b0 = s1 ^ s2, b1 = c1 ^ c2 ^ (s1 & s2), q4 = c1 & c2;
                const unsigned two = b1 & ~b0, side = tl ^ br; // of two set corners: tl != br <=> they share a side
                const unsigned m[kQuadClasses] = {b0 & ~b1, two & side, b0 & b1, q4, two & ~side};
#pragma unroll
                for (int kk = 0; kk < NT; ++kk)
#pragma unroll
                    for (int cl = 0; cl < kQuadClasses; ++cl)
                        n[kk][cl] += (unsigned)__popc(NT == 1 ? m[cl] : (m[cl] & (0x1fu << (8 * kk))));
                tl = bl;
                tr = br;
            }
        }

        // The lanes of one region are a run of the wave: after the step of offset m a lane holds the sum over the lanes
        // [l, l + 2 m) of its run, so the run's first lane ends with the whole of it.
        bool same[6]; // (every shuffle with every lane active)
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const unsigned pj = (unsigned)__shfl_down((int)jreg, 1 << s);
            same[s] = lane + (1 << s) < 64 && pj == jreg;
        }
        const unsigned left = (unsigned)__shfl_up((int)jreg, 1);
        const bool leader = (lane == 0 || left != jreg) && (int64_t)jreg < a.rc;
        unsigned long long *region = a.out + ((y * a.rr + i) * a.rc + ((int64_t)jreg < a.rc ? jreg : 0)) * (NT * kQuadSlots);
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int cl = 0; cl < kQuadClasses; ++cl) {
                unsigned v = n[k][cl];
#pragma unroll
                for (int s = 0; s < 6; ++s) {
                    const unsigned pv = (unsigned)__shfl_down((int)v, 1 << s);
                    v += same[s] ? pv : 0u;
                }
                if (leader && v) atomicAdd(&region[k * kQuadSlots + 1 + cl], (unsigned long long)v);
            }
    }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

} // namespace

hipError_t gs_launch_region_summary(const float *const *planes, int n, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                    int32_t rw, GsRegionSummary *out, hipStream_t s)
{
    if (n < 1 || n > 4 || rh < 1 || rw < 16 || rw % 4 != 0) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsRegionSumArgs a{};
    // 16-byte loads only: a field's planes and rows begin on 16-byte boundaries (gs_field_create), and there is no other form
    if (!gs_plane_set(a.set, planes, n, 1, 0, pitch, rows, cols)) return hipErrorInvalidValue;
    const bool wide = rw >= 256;
    a.rh = rh < rows ? rh : (int32_t)rows; // (one row of regions either way)
    a.rw = rw;
    a.seg = wide ? 64 : rw / 4;
    a.side = 64 / a.seg;
    const int64_t rr = ceil_div(rows, a.rh), rc = ceil_div(cols, rw);
    if (rr * rc > (int64_t)1 << 22) return hipErrorInvalidValue; // (GS_REGIONS_MAX: the host's refusal, restated)
    a.rr = (int32_t)rr;
    a.rc = (int32_t)rc;
    a.col_groups = (int32_t)ceil_div(rc, a.side);
    a.out = out;
    const int64_t groups = ceil_div((int64_t)a.rr * a.col_groups, 4);
    const dim3 grid((unsigned)(groups < 65536 ? groups : 65536), (unsigned)n);
    if (wide)
        hipLaunchKernelGGL(gs_region_summary_k<true>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(gs_region_summary_k<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t gs_launch_region_quads(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                  int32_t rw, const float *thresholds, const int32_t *sense, int32_t nt, int64_t max_groups,
                                  unsigned long long *out, hipStream_t s)
{
    if (np < 1 || np > 4 || nt < 1 || nt > 4 || rh < 1 || rw < 16 || rw % 4 != 0) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsRegionQuadArgs a{};
    if (!gs_plane_set(a.set, planes, np, 1, 0, pitch, rows, cols)) return hipErrorInvalidValue; // (16-byte loads only, as above)
    gs_set_rules(a.t, a.flip, thresholds, sense, np, nt);
    a.rh = rh < rows ? rh : (int32_t)rows; // (one row of regions either way)
    a.rw = rw;
    // rh + 1 quad rows in chunks of kQuadRows .. 2 kQuadRows - 1 (fewer when the region has fewer): no chunk of a row or two
    const int64_t quad_rows = (int64_t)a.rh + 1;
    a.chunks = (int32_t)(quad_rows / kQuadRows > 1 ? quad_rows / kQuadRows : 1);
    a.chunk_rows = (int32_t)ceil_div(quad_rows, a.chunks);
    a.rr = ceil_div(rows, a.rh);
    a.rc = ceil_div(cols, rw);
    a.out = out;
    const int64_t units = (((int64_t)cols + 255) / 256) * a.rr * a.chunks;
    if (!gs_scan_groups(units, 0, max_groups, np, a.groups)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.groups * np));
    switch (nt) {
    case 1: hipLaunchKernelGGL(gs_region_quads_k<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(gs_region_quads_k<2>, grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL(gs_region_quads_k<3>, grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(gs_region_quads_k<4>, grid, dim3(256), 0, s, a); break;
    }
    return hipGetLastError();
}
