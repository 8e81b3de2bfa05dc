// gs_region_change.hip -- regional state comparison on the device (include/gs_hip.h: gs_fields_region_compare): the change of
// every region of rh x rw cells between two planes, each bit for bit what gs_change.hip and the field fold return for two
// planes that hold that region's cells alone.  Regions as in gs_regions.hip: rw a multiple of 4, a lane's four columns never
// straddle two regions, every load 16 B per lane and plane, ragged regions at the lower and right edge kept.
//
// gs_region_change_k is gs_region_summary_k's two-plane form, and its geometry is that kernel's: a wave row of 256 columns
// holds as many regions side by side as fit (one from rw = 256; wider ones take the wide branch, which walks a region row in
// chunks of 256 columns); a region of rw <= 256 columns takes the rw / 4 lanes of its segment, and the row partial with columns counted
// from the region's first one is the halving tree over 64 lanes of which those past the segment hold +0.0.  Narrow regions
// load kRegionChangeUnroll rows of both planes before the adds and run those rows' trees side by side; wide ones load
// kRegionChangeUnroll chunks of both planes.  max_abs and the two counts are order-free: they stay per lane to the unit's end.
// Two routes, one kernel body:
//   wave     a wave's unit is a whole region (row of the region grid x group of regions side by side): the rows' partials are
//            added in registers in ascending order from +0.0 and the region's result is written once.  No other memory.
//   records  a unit is a band of kRegionChangeBand rows of a region: every (row, region column) leaves one 16-byte record, the
//            row partials of |d| and d * d; the order-free parts of the band go to the region's result with integer atomics
//            (max_abs as its bit pattern: a non-negative f64 orders as the u64 it is).  gs_region_change_fold_k then adds each
//            region's records in ascending row order from +0.0, a thread per region.  A region of 1024 x 1024 cells is 64
//            units instead of one: the device is filled where the wave route leaves most of it idle.
// The bits are the same on both routes: the same lane accumulators, the same tree, the same row order.
//
// Built with hipcc's default float mode (f32 denormals kept), as gs_change.hip is.
#include "gs_kernels.h"
#include "gs_plane_scan.h"

namespace {

constexpr int kUnroll = kRegionChangeUnroll;
constexpr int kFoldUnroll = 16; // records a fold thread loads before it adds them

struct GsRegionChangeArgs {
    const float *a[4], *b[4]; // the slab's pairs of planes
    int64_t pitch, rows;      // of every plane
    int32_t cols;
    int32_t rh, rw;           // the region shape (rh <= rows)
    int32_t seg;              // lanes of a region in a wave row: min(rw / 4, 64)
    int32_t side;             // regions side by side in a wave row: 64 / seg (1 from rw = 256)
    int32_t rr, rc;           // rows of the region grid in this slab, columns of the region grid
    int32_t col_groups;       // ceil(rc / side)
    int32_t bands, band_rows; // units a region's rows are cut into, and the rows of each (wave route: 1, rh)
    uint32_t units;           // rr * bands * col_groups: a 32-bit number (the launcher refuses any other)
    GsChangeTotal *out;       // [pair][rr][rc]; records route: zeroed by the caller
    double2 *rec;             // records route: [pair][rows][rc], (sum |d|, sum d * d) of a region's row
};

// One cell pair: gs_change.hip's take() with the counts kept in u32 for a block of rows.  A cell that is not comparable adds
// +0.0, which leaves an accumulator that started at +0.0 bit for bit as it was; a cell outside the region arrives here as the
// pair (+0.0, +0.0) (masked()), which is comparable, does not differ and adds +0.0 too.
__device__ __forceinline__ void take_pair(double &s, double &q, double &mx, uint32_t &df, uint32_t &nf, float x, float y)
{
    const bool fin = __builtin_isfinite(x) && __builtin_isfinite(y);
    const double d = fin ? (double)x - (double)y : 0.0; // one f64 subtraction
    const double ad = __builtin_fabs(d);
    s += ad;
    q += d * d;
    mx = fmax(mx, ad);
    df += __float_as_uint(x) != __float_as_uint(y) ? 1u : 0u;
    nf += fin ? 0u : 1u;
}

// The four cells of a lane with those outside the region (or the band) replaced by +0.0: m holds all ones for a cell
// that counts and zero for one that does not (bit masks in registers: nothing to keep in scalar lane masks).
__device__ __forceinline__ float4 masked(float4 x, uint4 m)
{
    return make_float4(__uint_as_float(__float_as_uint(x.x) & m.x), __uint_as_float(__float_as_uint(x.y) & m.y),
                       __uint_as_float(__float_as_uint(x.z) & m.z), __uint_as_float(__float_as_uint(x.w) & m.w));
}

// Cells 0 .. 3 of a lane of which the first nv (<= 0: none, >= 4: all) count.
__device__ __forceinline__ uint4 first_cells(int nv)
{
    return make_uint4(nv > 0 ? ~0u : 0u, nv > 1 ? ~0u : 0u, nv > 2 ? ~0u : 0u, nv > 3 ? ~0u : 0u);
}

// The lanes from this one to its segment's end, as a value the compiler takes for new at every use: the six compares of a
// halving tree are then made where they are needed (one VALU instruction each) and not kept as six lane masks in scalar
// registers across the whole kernel, which is what spills them.
__device__ __forceinline__ int lanes_to_end(int n)
{
    asm volatile("" : "+v"(n));
    return n;
}

__device__ __forceinline__ void take_four(double &s, double &q, double &mx, uint32_t &df, uint32_t &nf, float4 x, float4 y)
{
    take_pair(s, q, mx, df, nf, x.x, y.x);
    take_pair(s, q, mx, df, nf, x.y, y.y);
    take_pair(s, q, mx, df, nf, x.z, y.z);
    take_pair(s, q, mx, df, nf, x.w, y.w);
}

// grid (ceil(units / 4), pairs), 4 waves per workgroup, one unit per wave: no loop over units, so that nothing of a unit's
// set-up stays live across another (with such a loop the kernel arguments alone spill scalar registers).
template <bool WIDE, bool RECORDS>
__global__ __launch_bounds__(256) void gs_region_change_k(GsRegionChangeArgs a)
{
    const int lane = (int)(threadIdx.x & 63);
    const float *plane_a = a.a[blockIdx.y], *plane_b = a.b[blockIdx.y];
    const int cols = a.cols;
    const int64_t rows = a.rows, pitch = a.pitch;
    const int g = lane / a.seg, v = lane - g * a.seg; // the lane's region of the wave row, and its place in that region
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (the same in every lane: units are scalar)
    const uint32_t u = blockIdx.x * 4u + wave;
    if (u >= a.units) return; // (scalar)
    const uint32_t t = u / (uint32_t)a.col_groups;
    const int i = (int)(t / (uint32_t)a.bands), band = (int)(t - (uint32_t)i * (uint32_t)a.bands);
    const int j = (int)(u - t * (uint32_t)a.col_groups) * a.side + g;
    const bool mine = g < a.side && j < a.rc;
    const int64_t top = (int64_t)i * a.rh, end = top + a.rh < rows ? top + a.rh : rows;
    const int64_t r0 = top + (int64_t)band * a.band_rows, r1 = r0 + a.band_rows < end ? r0 + a.band_rows : end;
    if (r0 >= r1) return; // (scalar: a ragged region's last bands are empty)
    // the region's columns [cb, ce); a lane without a region holds none
    const int cb = mine ? j * a.rw : cols; // (j rw < cols)
    const int ce = (int64_t)cb + a.rw < cols ? cb + a.rw : cols;
    double fs = 0.0, fq = 0.0; // wave route: the field fold of the region, rows added from +0.0
    double mx = 0.0;
    unsigned long long dfs = 0ull, nfs = 0ull; // (a lane's count of a block of rows fits 32 bits, a large region's need not)
    double2 *rec = RECORDS ? a.rec + ((int64_t)blockIdx.y * rows) * a.rc + (mine ? j : 0) : nullptr;

    if (!WIDE) {
        const int c = mine ? cb + 4 * v : cols;
        const int cv = c < cols ? c : 0; // (16 bytes that begin inside the row end inside its pitch)
        const uint4 own = first_cells(ce - c); // (a lane without a region: ce - c == 0)
        const float *pa = plane_a + r0 * pitch + cv, *pb = plane_b + r0 * pitch + cv;
        double2 *at = RECORDS ? rec + r0 * a.rc : nullptr;
        // `left` rows of the band are still to come (a band's rows fit 32 bits); scalar: no lane leaves early
        for (int left = (int)(r1 - r0); left > 0; left -= kUnroll, pa += kUnroll * pitch, pb += kUnroll * pitch) {
            float4 x[kUnroll], y[kUnroll];
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) {
                const int64_t off = (int64_t)(k < left ? k : left - 1) * pitch; // (a row past the band: its last row again)
                x[k] = *reinterpret_cast<const float4 *>(pa + off);
                y[k] = *reinterpret_cast<const float4 *>(pb + off);
            }
            double s[kUnroll], q[kUnroll];
            uint32_t df = 0u, nf = 0u;
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) {
                const uint32_t live = k < left ? ~0u : 0u; // a row past the band adds +0.0 everywhere
                const uint4 m = make_uint4(own.x & live, own.y & live, own.z & live, own.w & live);
                s[k] = 0.0;
                q[k] = 0.0;
                take_four(s[k], q[k], mx, df, nf, masked(x[k], m), masked(y[k], m));
                __builtin_amdgcn_sched_barrier(0); // one row at a time: the rows' lane masks are not all held at once
            }
            dfs += df;
            nfs += nf;
            // lane combine inside the segment: lane v ends the step of offset m with (its sum) + (lane v + m's, +0.0
            // past the segment); the segment's first lane ends with the halving order of gs_hip.h
            const int reach = lanes_to_end(a.seg - v);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const bool in = m < reach;
#pragma unroll
                for (int k = 0; k < kUnroll; ++k) {
                    const double ps = __shfl_down(s[k], m), pq = __shfl_down(q[k], m);
                    s[k] = s[k] + (in ? ps : 0.0);
                    q[k] = q[k] + (in ? pq : 0.0);
                }
            }
            if (RECORDS) {
                if (lanes_to_end(mine && v == 0 ? 1 : 0)) { // the segments' first lanes: one record per row and region
#pragma unroll
                    for (int k = 0; k < kUnroll; ++k)
                        if (k < left) at[(int64_t)k * a.rc] = make_double2(s[k], q[k]); // (scalar)
                }
                at += (int64_t)kUnroll * a.rc;
            } else {
#pragma unroll
                for (int k = 0; k < kUnroll; ++k) {
                    fs = fs + s[k];
                    fq = fq + q[k];
                }
            }
        }
    } else {
        const int w = ce - cb; // (one region per wave: seg == 64, v == lane)
        for (int64_t r = r0; r < r1; ++r) {
            const float *ra = plane_a + r * pitch + cb, *rb = plane_b + r * pitch + cb;
            double s = 0.0, q = 0.0;
            uint32_t df = 0u, nf = 0u;
            for (int c0 = 4 * lane; c0 < w; c0 += 256 * kUnroll) {
                float4 x[kUnroll], y[kUnroll];
#pragma unroll
                for (int k = 0; k < kUnroll; ++k) {
                    const int c = c0 + 256 * k;
                    // (16 bytes that begin inside the region end inside the row's pitch; what lies past the region is masked)
                    x[k] = *reinterpret_cast<const float4 *>(ra + (c < w ? c : 0));
                    y[k] = *reinterpret_cast<const float4 *>(rb + (c < w ? c : 0));
                }
#pragma unroll
                for (int k = 0; k < kUnroll; ++k) {
                    const int c = c0 + 256 * k;
                    const uint4 m = first_cells(w - c);
                    take_four(s, q, mx, df, nf, masked(x[k], m), masked(y[k], m));
                    __builtin_amdgcn_sched_barrier(0); // one chunk at a time: the chunks' lane masks are not all held at once
                }
            }
            dfs += df;
            nfs += nf;
            const int reach = lanes_to_end(64 - lane);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const bool in = m < reach;
                const double ps = __shfl_down(s, m), pq = __shfl_down(q, m);
                s = s + (in ? ps : 0.0);
                q = q + (in ? pq : 0.0);
            }
            if (RECORDS) {
                if (mine && lane == 0) rec[r * a.rc] = make_double2(s, q);
            } else {
                fs = fs + s;
                fq = fq + q;
            }
        }
    }
    // the order-free parts, over the segment
    const int reach = lanes_to_end(a.seg - v);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const bool in = m < reach;
        const double pmx = __shfl_down(mx, m);
        const unsigned long long pdf = __shfl_down(dfs, m), pnf = __shfl_down(nfs, m);
        mx = fmax(mx, in ? pmx : 0.0);
        dfs += in ? pdf : 0ull;
        nfs += in ? pnf : 0ull;
    }
    if (mine && v == 0) {
        GsChangeTotal *o = a.out + ((int64_t)blockIdx.y * a.rr + i) * a.rc + j;
        if (RECORDS) {
            // (zeroed by the caller; |d| >= +0.0 and never NaN: the u64 order of the bits is the f64 order)
            if (mx > 0.0) atomicMax(reinterpret_cast<unsigned long long *>(&o->max_abs), (unsigned long long)__double_as_longlong(mx));
            if (dfs) atomicAdd(reinterpret_cast<unsigned long long *>(&o->differing), dfs);
            if (nfs) atomicAdd(reinterpret_cast<unsigned long long *>(&o->nonfinite), nfs);
        } else {
            GsChangeTotal res;
            res.sum_abs = fs;
            res.sum_sq = fq;
            res.max_abs = mx;
            res.differing = dfs;
            res.nonfinite = nfs;
            *o = res;
        }
    }
}

// One thread per (pair, region): the region's row records added in ascending row order from +0.0 (gs_change_fold_k's
// pattern); neighbouring threads read neighbouring records.  The order-free parts are already in out[].
__global__ __launch_bounds__(256) void gs_region_change_fold_k(const double2 *rec, int64_t rows, int32_t rh, int32_t rr, int32_t rc,
                                                               int32_t n, GsChangeTotal *out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)n * rr * rc) return;
    const int64_t t = g / rc, p = t / rr;
    const int64_t i = t - p * rr;
    const int64_t r0 = i * rh, r1 = r0 + rh < rows ? r0 + rh : rows;
    const double2 *mine = rec + (p * rows) * rc + (g - t * rc);
    double s = 0.0, q = 0.0;
    for (int64_t r = r0; r < r1; r += kFoldUnroll) {
        double2 x[kFoldUnroll];
#pragma unroll
        for (int k = 0; k < kFoldUnroll; ++k) x[k] = mine[(r + k < r1 ? r + k : r1 - 1) * rc];
#pragma unroll
        for (int k = 0; k < kFoldUnroll; ++k) {
            const bool live = r + k < r1; // (a record past the region adds +0.0: s and q hold sums of values >= +0.0)
            s = s + (live ? x[k].x : 0.0);
            q = q + (live ? x[k].y : 0.0);
        }
    }
    out[g].sum_abs = s;
    out[g].sum_sq = q;
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

} // namespace

bool gs_region_change_wants_records(int64_t rows, int32_t cols, int32_t rh, int32_t rw, int cu_count)
{
    if (rows <= 0 || cols <= 0 || rh < 1 || rw < 16) return false;
    const int64_t h = rh < rows ? rh : rows;
    const int64_t side = rw >= 256 ? 1 : 64 / (rw / 4);
    const int64_t units = ceil_div(rows, h) * ceil_div(ceil_div(cols, rw), side); // waves of the wave route
    const int64_t cus = cu_count > 0 ? cu_count : 256;
    return h >= 2 * kRegionChangeBand && units < kRegionChangeWavesPerCu * cus;
}

size_t gs_region_change_record_bytes(int n, int64_t rows, int32_t cols, int32_t rw)
{
    if (n < 1 || rows <= 0 || cols <= 0 || rw < 16) return 0;
    return (size_t)n * (size_t)rows * (size_t)ceil_div(cols, rw) * sizeof(double2);
}

hipError_t gs_launch_region_change(const float *const *pa, const float *const *pb, int n, int64_t pitch, int64_t rows, int32_t cols,
                                   int32_t rh, int32_t rw, GsChangeTotal *out, void *records, hipStream_t s)
{
    if (n < 1 || n > 4 || rh < 1 || rw < 16 || rw % 4 != 0) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsRegionChangeArgs a{};
    // 16-byte loads only: a field's planes and rows begin on 16-byte boundaries (gs_field_create), and there is no other form
    if (!gs_reads_16_bytes(pa, n, 1, 0, pitch) || !gs_reads_16_bytes(pb, n, 1, 0, pitch)) return hipErrorInvalidValue;
    for (int p = 0; p < n; ++p) {
        a.a[p] = pa[p];
        a.b[p] = pb[p];
    }
    a.pitch = pitch;
    a.rows = rows;
    a.cols = cols;
    const bool wide = rw > 256; // (a region of exactly 256 columns is one chunk a row: the narrow branch, which loads several rows ahead)
    a.rh = rh < rows ? rh : (int32_t)rows; // (one row of regions either way)
    a.rw = rw;
    a.seg = wide ? 64 : rw / 4;
    a.side = 64 / a.seg;
    const int64_t rr = ceil_div(rows, a.rh), rc = ceil_div(cols, rw);
    if (rr * rc > (int64_t)1 << 22) return hipErrorInvalidValue; // (GS_REGIONS_MAX: the host's refusal, restated)
    a.rr = (int32_t)rr;
    a.rc = (int32_t)rc;
    a.col_groups = (int32_t)ceil_div(rc, a.side);
    a.bands = records ? (int32_t)ceil_div(a.rh, kRegionChangeBand) : 1;
    a.band_rows = records ? kRegionChangeBand : a.rh;
    a.out = out;
    a.rec = static_cast<double2 *>(records);
    const int64_t units = (int64_t)a.rr * a.bands * a.col_groups;
    if (units > INT32_MAX) return hipErrorInvalidValue; // (a band is 16 rows x 256 columns or more: no plane that fits a device has as many)
    a.units = (uint32_t)units;
    const int64_t groups = ceil_div(units, 4);
    const dim3 grid((unsigned)groups, (unsigned)n);
    if (!records) {
        if (wide)
            hipLaunchKernelGGL((gs_region_change_k<true, false>), grid, dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((gs_region_change_k<false, false>), grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (wide)
        hipLaunchKernelGGL((gs_region_change_k<true, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((gs_region_change_k<false, true>), grid, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t regions = (int64_t)n * rr * rc;
    hipLaunchKernelGGL(gs_region_change_fold_k, dim3((unsigned)ceil_div(regions, 256)), dim3(256), 0, s, a.rec, rows, a.rh, a.rr, a.rc,
                       (int32_t)n, out);
    return hipGetLastError();
}
